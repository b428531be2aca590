"""Drop-in for utils/inference/masks.py on MI355X: the paste-back masks built on the device.

``face_mask_static(image, landmarks, landmarks_tgt, params=None)`` keeps the reference signature and return
convention (masks.py:38-86: ``(mask, [erode, sigmaX, sigmaY])`` when params is None, else ``mask``), with the
mask a float32 device tensor [H, W] instead of a float64 numpy array (it feeds the device blend directly;
``.cpu().numpy()`` gives the reference's values as float32).  ``face_masks`` does a whole batch of frames
in three launches (``ghost_face_masks``): the video path builds every frame's mask of an identity at once.

Split as in the reference: the parameter choice (masks.py:43-65) and, in the native library's host code,
the eyebrow expansion on int32 landmarks and the convex hull (``ghost_mask_polygons``, C++ on the CPU);
the raster (cv2.fillConvexPoly), the box erode / dilate, the border fade and the Gaussian blur run on the GPU
(ghost_amd/csrc/masks.hip).  The OpenCV calls are restated from OpenCV 4.x's published algorithms; cv2 is
absent here, so the masks are checked against the CPU restatement oracle/mask_ref.py (parity unpinned).

``mask_polygons_device`` and ``face_masks_device`` are the same step for landmarks that are on the device already:
the parameter choice, the eyebrow expansion and the convex hull in one more launch (ghost_amd/csrc/mask_poly.hip),
equal bit for bit to the host functions above and without a device -> host copy.  Nothing here calls them by default.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _lib

MAX_V = 128   # hull vertices per frame (masks.hip kMaxV)


def mask_params(landmarks, landmarks_tgt):
    """face_mask_static's (erode, sigmaX, sigmaY) when params is None (masks.py:43-65)."""
    lm, lt = np.asarray(landmarks), np.asarray(landmarks_tgt)
    left = np.sum((lm[1][0] - lt[1][0], lm[2][0] - lt[2][0], lm[13][0] - lt[13][0]))
    right = np.sum((lt[17][0] - lm[17][0], lt[18][0] - lm[18][0], lt[29][0] - lm[29][0]))
    offset = max(left, right)
    if offset > 6:
        return [15, 15, 10]
    if offset > 3:
        return [10, 10, 8]
    if offset < -3:
        return [-5, 5, 10]
    return [5, 5, 5]


def mask_polygons(landmarks: np.ndarray, params: np.ndarray):
    """Host half (ghost_mask_polygons): eyebrow expansion + convex hull -> (poly int32 [F,128,2], nv int32 [F])."""
    lib = _lib.load()
    lm = np.ascontiguousarray(np.asarray(landmarks, dtype=np.float32).reshape(-1, 106, 2))
    F = lm.shape[0]
    pr = np.ascontiguousarray(np.asarray(params, dtype=np.int32).reshape(F, 3))
    poly = np.zeros((F, MAX_V, 2), dtype=np.int32)
    nv = np.zeros(F, dtype=np.int32)
    _lib.check(lib.ghost_mask_polygons(lm.ctypes.data, F, 106, pr.ctypes.data, poly.ctypes.data, nv.ctypes.data),
               "ghost_mask_polygons")
    return poly, nv


MAX_SIGMA = 42   # 6 sigma + 1 = 253 taps, the most the blur kernel holds (masks.hip kMaxTaps = 256)
MAX_ERODE = 256  # a larger box than the tallest image (masks.hip kMaxRows) erases or fills every mask


def check_params(params) -> np.ndarray:
    """params as int32 [F,3] (erode, sigmaX, sigmaY), or ValueError: a sigma outside 1..42 has no blur on the device
    (cv2 raises for sigma 0; the kernel has no room for the taps of sigma >= 43 and would return an all-zero mask)
    and |erode| > 256 is no face mask.  Host data only: nothing here touches the device."""
    pr = np.asarray(params, dtype=np.int32).reshape(-1, 3)
    bad = (pr[:, 1:] < 1) | (pr[:, 1:] > MAX_SIGMA)
    if bad.any():
        f = int(np.flatnonzero(bad.any(axis=1))[0])
        raise ValueError(f"ghost_amd: face mask sigmaX / sigmaY must be in 1..{MAX_SIGMA}, got params "
                         f"{pr[f].tolist()} for frame {f}")
    if (np.abs(pr[:, 0].astype(np.int64)) > MAX_ERODE).any():
        f = int(np.flatnonzero(np.abs(pr[:, 0].astype(np.int64)) > MAX_ERODE)[0])
        raise ValueError(f"ghost_amd: face mask |erode| must be at most {MAX_ERODE}, got params {pr[f].tolist()} "
                         f"for frame {f}")
    return pr


def face_masks(landmarks, params, H: int = 224, W: int = 224, device=None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Masks of F frames: landmarks [F,106,2] (the swap's, as the landmark model returns them), params [F,3]
    (erode, sigmaX, sigmaY) -> float32 [F,H,W] on ``device`` (face_mask_static's mask / 255 per frame).
    ValueError, before anything touches the device, for a sigma outside 1..42 or |erode| > 256 (``check_params``)."""
    pr = check_params(params)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError("ghost_amd: face_masks runs on the GPU only (no CPU path)")
    poly, nv = mask_polygons(landmarks, pr)
    F = poly.shape[0]
    if F == 0:
        return torch.empty(0, H, W, dtype=torch.float32, device=dev)
    if out is None:
        out = torch.empty(F, H, W, dtype=torch.float32, device=dev)
    elif out.shape != (F, H, W) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise RuntimeError(f"ghost_amd: out must be a contiguous float32 [{F},{H},{W}] tensor on {dev}")
    lib = _lib.load()
    with torch.cuda.device(dev):
        d_poly = torch.from_numpy(poly).to(dev, non_blocking=True)
        d_nv = torch.from_numpy(nv).to(dev, non_blocking=True)
        d_pr = torch.from_numpy(pr).to(dev, non_blocking=True)
        ws = torch.empty(int(lib.ghost_face_masks_workspace_bytes(F, H, W)), dtype=torch.uint8, device=dev)
        _lib.check(lib.ghost_face_masks(d_poly.data_ptr(), d_nv.data_ptr(), d_pr.data_ptr(), F, H, W, out.data_ptr(),
                                        H * W, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)), "ghost_face_masks")
    return out


def _dev_arg(t: torch.Tensor, dtype, shape, dev, name: str) -> torch.Tensor:
    if not torch.is_tensor(t) or t.device != dev or t.dtype != dtype or not t.is_contiguous() or \
            any(s is not None and s != d for s, d in zip(shape, t.shape)) or t.dim() != len(shape):
        want = "[" + ",".join("*" if s is None else str(s) for s in shape) + "]"
        raise RuntimeError(f"ghost_amd: {name} must be a contiguous {dtype} {want} tensor on {dev}")
    return t


def mask_polygons_device(landmarks: torch.Tensor, params: Optional[torch.Tensor] = None, *,
                         landmarks_ref: Optional[torch.Tensor] = None, ref_index: Optional[torch.Tensor] = None,
                         landmarks_tgt: Optional[torch.Tensor] = None, tgt_index: Optional[torch.Tensor] = None):
    """``mask_polygons`` (and, without ``params``, ``mask_params``) on the device (ghost_mask_polygons_dev, one
    launch, no host copy): landmarks float32 [F,106,2] on the GPU -> device (poly int32 [F,128,2], nv int32 [F],
    params int32 [F,3]), equal bit for bit to the host functions' results.

    Either ``params`` (int32 [F,3], returned as they are) or both reference sets: face f's parameters are
    ``mask_params(landmarks_ref[ref_index[f]], landmarks_tgt[tgt_index[f]])`` (float32 [*,106,2] sets, int32 [F]
    indices; an index outside its set gives params 0, 0, 0).  ``ghost_face_masks`` gives a frame whose sigmaX or
    sigmaY is outside 1..42, such params included, an all-zero mask (never NaN): the paste-back leaves it untouched."""
    _lib.require_gpu(landmarks, "mask_polygons_device")
    dev = landmarks.device
    lm = _dev_arg(landmarks, torch.float32, (None, 106, 2), dev, "landmarks")
    F = lm.shape[0]
    refs = (landmarks_ref, ref_index, landmarks_tgt, tgt_index)
    if (params is not None) == any(r is not None for r in refs) or \
            any(r is not None for r in refs) != all(r is not None for r in refs):
        raise RuntimeError("ghost_amd: mask_polygons_device takes either params or all of landmarks_ref, ref_index, "
                           "landmarks_tgt, tgt_index")
    n_ref = n_tgt = 0
    if params is not None:
        params = _dev_arg(params, torch.int32, (F, 3), dev, "params")
    else:
        landmarks_ref = _dev_arg(landmarks_ref, torch.float32, (None, 106, 2), dev, "landmarks_ref")
        landmarks_tgt = _dev_arg(landmarks_tgt, torch.float32, (None, 106, 2), dev, "landmarks_tgt")
        ref_index = _dev_arg(ref_index, torch.int32, (F,), dev, "ref_index")
        tgt_index = _dev_arg(tgt_index, torch.int32, (F,), dev, "tgt_index")
        n_ref, n_tgt = landmarks_ref.shape[0], landmarks_tgt.shape[0]
    poly = torch.empty(F, MAX_V, 2, dtype=torch.int32, device=dev)
    nv = torch.empty(F, dtype=torch.int32, device=dev)
    out = torch.empty(F, 3, dtype=torch.int32, device=dev)
    if F == 0:
        return poly, nv, out
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.ghost_mask_polygons_dev(lm.data_ptr(), _lib.ptr(params), _lib.ptr(landmarks_ref),
                                               _lib.ptr(ref_index), n_ref, _lib.ptr(landmarks_tgt),
                                               _lib.ptr(tgt_index), n_tgt, out.data_ptr(), poly.data_ptr(),
                                               nv.data_ptr(), F, _lib.stream_ptr(dev)), "ghost_mask_polygons_dev")
    return poly, nv, out


def face_masks_device(landmarks: torch.Tensor, params: torch.Tensor, H: int = 224, W: int = 224,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``face_masks`` from device inputs: landmarks float32 [F,106,2] and params int32 [F,3] on the GPU -> float32
    [F,H,W] there, the same bits as ``face_masks`` gives for their host copies.  Four launches, no host copy of the
    landmarks and no synchronisation."""
    poly, nv, pr = mask_polygons_device(landmarks, params)
    return _raster(poly, nv, pr, H, W, out)


def _raster(poly: torch.Tensor, nv: torch.Tensor, pr: torch.Tensor, H: int, W: int,
            out: Optional[torch.Tensor]) -> torch.Tensor:
    """ghost_face_masks on device polygons."""
    dev, F = poly.device, poly.shape[0]
    if F == 0:
        return torch.empty(0, H, W, dtype=torch.float32, device=dev)
    if out is None:
        out = torch.empty(F, H, W, dtype=torch.float32, device=dev)
    elif out.shape != (F, H, W) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise RuntimeError(f"ghost_amd: out must be a contiguous float32 [{F},{H},{W}] tensor on {dev}")
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = torch.empty(int(lib.ghost_face_masks_workspace_bytes(F, H, W)), dtype=torch.uint8, device=dev)
        _lib.check(lib.ghost_face_masks(poly.data_ptr(), nv.data_ptr(), pr.data_ptr(), F, H, W, out.data_ptr(),
                                        H * W, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)), "ghost_face_masks")
    return out


def face_mask_static(image, landmarks, landmarks_tgt=None, params: Optional[Sequence[int]] = None, device=None):
    """masks.py:38-86 for one frame: ``image`` gives the mask size ([H,W,...] array or tensor)."""
    H, W = int(image.shape[0]), int(image.shape[1])
    p = mask_params(landmarks, landmarks_tgt) if params is None else list(params)
    if device is None and isinstance(image, torch.Tensor) and image.is_cuda:
        device = image.device
    m = face_masks(np.asarray(landmarks)[None], np.asarray(p)[None], H, W, device)[0]
    return (m, p) if params is None else m
