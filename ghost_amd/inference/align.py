"""Face alignment from detector keypoints to device-resident crops.

Everything between "the detector returned 5 keypoints" and "uint8 crops on the device":

* host geometry, numpy float64, no GPU needed:
  ``similarity_transform`` (skimage's ``SimilarityTransform.estimate``: Umeyama's closed form with scale),
  ``estimate_norm`` (insightface's ``face_align.estimate_norm(lmk, image_size, mode='None')``) and
  ``smooth_landmarks`` (utils/inference/video_processing.py:86-108);
* ``align_crops`` — ``cv2.warpAffine(frame, M, (crop_size, crop_size), borderValue=0.0)`` for many faces at once and
  the 224 -> 256 ``cv2.resize`` of resize_frames (video_processing.py:174-188), taken by one HIP launch
  (``ghost_align_crops_u8``) from the uint8 frames that ``blend.blend_swaps`` later composites into;
* ``crop_face`` (utils/inference/image_processing.py:13-20) and ``crop_frames_and_get_transforms``
  (video_processing.py:111-171) with the detector's result given, so that
  ``crop_frames_and_get_transforms`` -> ``core.swap_identity_frames`` -> ``masks.face_masks`` ->
  ``blend.blend_swaps`` is one device-resident chain and a frame crosses the host link once in each direction.

Detection stays on the host (the detector model is the reference's).  skimage, insightface and cv2 are absent here:
the fit, the template choice and the warp are restatements of their published algorithms, parity unpinned like the
rest of the paste-back (the warp and the resize are bit-exact against oracle/blend_ref.py).  insightface's 5-pose
template table ``face_align.src_map[crop_size]`` is not restated: it is a required argument (INTEGRATION.md shows
the line that passes it).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from .blend import _fstride, _invert_affine_cv, resize_u8

MAX_CROPS_PER_CALL = 65535          # ghost_align_crops_u8's N limit (one grid row per crop)


# ---------------------------------------------------------------------------------------------------------
# host geometry
# ---------------------------------------------------------------------------------------------------------
def similarity_transform(src, dst) -> np.ndarray:
    """The least-squares similarity (scale, rotation, translation) taking ``src`` [K,2] onto ``dst`` [K,2] as a
    [3,3] homogeneous matrix: skimage's ``SimilarityTransform.estimate`` (Umeyama 1991, eq. 40-43, with scale).
    A reflection is never returned (the smallest singular direction is flipped instead), and a rank-deficient
    covariance (collinear points) takes Umeyama's special case; a rank-0 one (all points equal) gives NaN."""
    src = np.asarray(src, np.float64)
    dst = np.asarray(dst, np.float64)
    num, dim = src.shape
    src_mean, dst_mean = src.mean(axis=0), dst.mean(axis=0)
    src_demean, dst_demean = src - src_mean, dst - dst_mean
    A = dst_demean.T @ src_demean / num
    d = np.ones((dim,), np.float64)
    if np.linalg.det(A) < 0:
        d[dim - 1] = -1
    T = np.eye(dim + 1, dtype=np.float64)
    U, S, V = np.linalg.svd(A)
    rank = np.linalg.matrix_rank(A)
    if rank == 0:
        return np.nan * T
    if rank == dim - 1:
        if np.linalg.det(U) * np.linalg.det(V) > 0:
            T[:dim, :dim] = U @ V
        else:
            s = d[dim - 1]
            d[dim - 1] = -1
            T[:dim, :dim] = U @ np.diag(d) @ V
            d[dim - 1] = s
    else:
        T[:dim, :dim] = U @ np.diag(d) @ V
    scale = 1.0 / src_demean.var(axis=0).sum() * (S @ d)
    T[:dim, dim] = dst_mean - scale * (T[:dim, :dim] @ src_mean.T)
    T[:dim, :dim] *= scale
    return T


def estimate_norm(lmk, image_size: int, templates) -> Tuple[np.ndarray, int]:
    """insightface's ``face_align.estimate_norm(lmk, image_size, mode='None')``: fit every template [T,5,2] and
    return (M [2,3] float64, index) of the one with the smallest ``sum_k |M [lmk_k, 1] - template_k|`` (the first
    on a tie).  ``templates`` is insightface's ``face_align.src_map[image_size]``; ``image_size`` only names it."""
    lmk = np.asarray(lmk, np.float64)
    templates = np.asarray(templates, np.float64)
    if lmk.shape != (5, 2) or templates.ndim != 3 or templates.shape[1:] != (5, 2):
        raise ValueError(f"estimate_norm takes landmarks [5,2] and templates [T,5,2], got {lmk.shape}, {templates.shape}")
    lmk_tran = np.insert(lmk, 2, values=np.ones(5), axis=1)
    min_M, min_index, min_error = None, -1, float("inf")
    for i in range(templates.shape[0]):
        M = similarity_transform(lmk, templates[i])[0:2, :]
        results = (M @ lmk_tran.T).T
        error = np.sum(np.sqrt(np.sum((results - templates[i]) ** 2, axis=1)))
        if error < min_error:
            min_error, min_M, min_index = error, M, i
    if min_M is None:
        raise ValueError("estimate_norm: no template gives a finite fit")
    return min_M, min_index


def _empty(k) -> bool:
    return k is None or len(k) == 0


def smooth_landmarks(kps_arr: Sequence[Sequence], n: int = 2) -> List[List]:
    """video_processing.py:86-108.  Per identity, the per-frame keypoints ([5,2], or ``[]`` without a face) are cut
    into segments — a new one starts where an entry or its predecessor is empty, or where point 0 or point 2 moved
    more than 5 px since the previous frame — and inside a segment entry i becomes the mean over [i-q, i+q],
    q = min(i, len-1-i, n).  Empty entries come back as ``[]``."""
    out = []
    for ka in kps_arr:
        segs: List[List] = []
        for i, k in enumerate(ka):
            if i == 0 or _empty(k) or _empty(ka[i - 1]):
                segs.append([k])
            else:
                a, b = np.asarray(k, np.float64), np.asarray(ka[i - 1], np.float64)
                if np.linalg.norm(a[0] - b[0]) > 5 or np.linalg.norm(a[2] - b[2]) > 5:
                    segs.append([k])
                else:
                    segs[-1].append(k)
        smooth: List = []
        for seg in segs:
            if _empty(seg[0]):
                smooth.append([])
                continue
            arr = np.asarray(seg, np.float64)
            for i in range(len(seg)):
                q = min(i, len(seg) - i - 1, n)
                smooth.append(arr[i - q:i + 1 + q].mean(axis=0))
        out.append(smooth)
    return out


def frames_to_match(kps_per_frame: Sequence, set_target: bool) -> List[int]:
    """The frames whose faces go through ArcFace matching (video_processing.py:130): more than one face, or any
    face with ``set_target``."""
    return [i for i, k in enumerate(kps_per_frame) if not _empty(k) and (len(k) > 1 or set_target)]


def select_keypoints(kps_per_frame: Sequence, n_targets: int, set_target: bool, matches) -> List[List]:
    """The keypoint bookkeeping of video_processing.py:127-155: ``kps_array[q][i]`` = the [5,2] keypoints identity q
    follows in frame i, or ``[]``.  ``matches[i]`` = (best_idx [T], accepted [T]) for every frame of
    ``frames_to_match``.  Every identity gets exactly one entry per frame (see crop_frames_and_get_transforms)."""
    kps_array: List[List] = [[] for _ in range(n_targets)]
    for i, kps in enumerate(kps_per_frame):
        if _empty(kps):
            for q in range(n_targets):
                kps_array[q].append([])
        elif len(kps) > 1 or set_target:
            best, ok = matches[i]
            for q in range(n_targets):
                kps_array[q].append(np.asarray(kps[int(best[q])], np.float64) if bool(ok[q]) else [])
        else:
            kps_array[0].append(np.asarray(kps[0], np.float64))
            for q in range(1, n_targets):
                kps_array[q].append([])
    return kps_array


def frame_transforms(kps_array: Sequence[Sequence], crop_size: int, templates):
    """video_processing.py:157-168 without the warp: smooth each identity's keypoints, then estimate_norm per
    (identity, frame).  Returns (present: per identity float64 [F] of 1/0, tfm_array: per identity a list of
    M [2,3] float64 or ``[]``)."""
    smooth = smooth_landmarks(kps_array, n=2)
    present, tfm_array = [], []
    for ks in smooth:
        p, tf = np.ones(len(ks)), []
        for i, k in enumerate(ks):
            if _empty(k):
                p[i] = 0
                tf.append([])
            else:
                tf.append(estimate_norm(k, crop_size, templates)[0])
        present.append(p)
        tfm_array.append(tf)
    return present, tfm_array


# ---------------------------------------------------------------------------------------------------------
# device crops
# ---------------------------------------------------------------------------------------------------------
def _check_frames(frames: torch.Tensor, what: str) -> None:
    if not torch.is_tensor(frames):
        raise RuntimeError(f"ghost_amd: {what} takes a uint8 [F,H,W,3] device tensor")
    _lib.require_gpu(frames, what)
    if frames.dtype != torch.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise RuntimeError("ghost_amd: frames must be a contiguous uint8 [F,H,W,3] device tensor")


def _upload(a: np.ndarray, dev: torch.device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)


def fused_resize_supported(crop_size: int, resize_to: int) -> bool:
    """The ratios ghost_align_crops_u8 resizes out of LDS: 8/7 (224 -> 256)."""
    return crop_size % 7 == 0 and resize_to == crop_size // 7 * 8


def align_crops(frames: torch.Tensor, tfms, frame_index, crop_size: int = 224, resize_to: Optional[int] = None,
                want_crops: bool = True, valid=None):
    """``cv2.warpAffine(frames[frame_index[n]], tfms[n], (crop_size, crop_size), borderValue=0.0)`` for N faces, and
    with ``resize_to=R`` also ``cv2.resize(crop, (R, R))``.  frames: contiguous uint8 [F,H,W,3] on the device (the
    tensor blend_swaps takes); tfms: [N,2,3] float64 on the host (estimate_norm's M), inverted here as
    cv2.invertAffineTransform does; frame_index: N ints (host: range-checked, IndexError; a device int32 tensor is
    used as it is and the kernel skips rows whose index is out of range); valid: optional [N], rows with 0 are left
    untouched (uninitialised memory of the returned tensors).  Returns (crops [N,S,S,3] or None without
    ``want_crops``, resized [N,R,R,3] or None without ``resize_to``), uint8 on the device.  The small arrays go up
    through pinned memory on the current stream; nothing synchronises."""
    _check_frames(frames, "align_crops")
    dev = frames.device
    S = int(crop_size)
    R = None if resize_to is None else int(resize_to)
    if S <= 0 or (R is not None and R <= 0):
        raise RuntimeError("ghost_amd: align_crops needs positive sizes")
    if not want_crops and R is None:
        raise RuntimeError("ghost_amd: align_crops has nothing to return (want_crops=False and no resize_to)")
    t = np.asarray(tfms.cpu() if torch.is_tensor(tfms) else tfms, np.float64)
    N = t.shape[0] if t.ndim == 3 else 0
    if t.size and (t.ndim != 3 or t.shape[1:] != (2, 3)):
        raise RuntimeError(f"ghost_amd: tfms must be [N,2,3], got {t.shape}")
    F_, H, W = frames.shape[:3]
    if torch.is_tensor(frame_index) and frame_index.is_cuda:
        _lib.require_same_device(frame_index, dev, "frame_index")
        idx = frame_index.to(torch.int32).contiguous()
        if idx.numel() != N:
            raise RuntimeError("ghost_amd: frame_index and tfms differ in length")
    else:
        ih = np.asarray(frame_index.cpu() if torch.is_tensor(frame_index) else frame_index).reshape(-1)
        if ih.size != N:
            raise RuntimeError("ghost_amd: frame_index and tfms differ in length")
        if N and (ih.min() < 0 or ih.max() >= F_):
            raise IndexError(f"ghost_amd: frame_index out of range for {F_} frames")
        idx = _upload(ih.astype(np.int32), dev) if N else None
    v = None
    if valid is not None:
        if torch.is_tensor(valid) and valid.is_cuda:
            _lib.require_same_device(valid, dev, "valid")
            v = valid.to(torch.int32).contiguous()
        else:
            v = np.asarray(valid.cpu() if torch.is_tensor(valid) else valid).reshape(-1)
            v = _upload((v != 0).astype(np.int32), dev) if N else None
        if v is not None and v.numel() != N:
            raise RuntimeError("ghost_amd: valid and tfms differ in length")
    fused = R is not None and fused_resize_supported(S, R)
    need_crops = want_crops or (R is not None and not fused)
    crops = torch.empty(N, S, S, 3, dtype=torch.uint8, device=dev) if need_crops else None
    resized = torch.empty(N, R, R, 3, dtype=torch.uint8, device=dev) if fused else None
    if N:
        maps = _upload(np.stack([_invert_affine_cv(m) for m in t]).reshape(N, 6), dev)
        lib, st = _lib.load(), _lib.stream_ptr(dev)
        for lo in range(0, N, MAX_CROPS_PER_CALL):
            hi = min(N, lo + MAX_CROPS_PER_CALL)
            _lib.check(lib.ghost_align_crops_u8(
                frames.data_ptr(), _fstride(frames), F_, H, W, idx[lo:hi].data_ptr(), maps[lo:hi].data_ptr(),
                None if v is None else v[lo:hi].data_ptr(), hi - lo, S,
                None if crops is None else crops[lo:hi].data_ptr(), S * S * 3,
                None if resized is None else resized[lo:hi].data_ptr(), 0 if resized is None else R * R * 3,
                0 if resized is None else R, st), "align_crops")
    if R is not None and not fused:
        # a ratio the kernel does not fuse: the crop, then the stand-alone cv2.resize kernel
        resized = crops if R == S else (resize_u8(crops, (R, R)) if N else
                                        torch.empty(0, R, R, 3, dtype=torch.uint8, device=dev))
    return (crops if want_crops else None), resized


def crop_face(frame: torch.Tensor, kps, crop_size: int, templates) -> List[torch.Tensor]:
    """image_processing.py:13-20 with ``kps = app.get(image_full, crop_size)`` given: the aligned crop of the first
    face of a device uint8 [H,W,3] frame, as a one-element list.  ``kps`` None (no face) raises TypeError, as
    subscripting the detector's None does in the reference (get_target relies on it)."""
    if kps is None:
        raise TypeError("crop_face: the detector found no face")
    if not torch.is_tensor(frame) or frame.ndim != 3:
        raise RuntimeError("ghost_amd: crop_face takes a uint8 [H,W,3] device tensor")
    M, _ = estimate_norm(kps[0], crop_size, templates)
    crops, _ = align_crops(frame[None], M[None], [0], crop_size)
    return [crops[0]]


def crop_frames_and_get_transforms(frames: torch.Tensor, kps_per_frame: Sequence, target_embeds: torch.Tensor, netArc,
                                   crop_size: int, set_target: bool, similarity_th: float, templates,
                                   embed_batch: int = 64):
    """video_processing.py:111-171 on device-resident frames, with ``app.get(frame, crop_size)`` given per frame:
    ``kps_per_frame[i]`` is a [k,5,2] array, or None for a frame without a face.

    Frames with more than one face (or any face with ``set_target``) are matched to the targets: all their faces are
    cropped in one ``align_crops``, embedded with ``netArc.embed_u8`` in batches of ``embed_batch`` and matched per
    frame with ``match_faces``.  Then smooth_landmarks, estimate_norm per (identity, frame) and one
    ``align_crops(..., resize_to=256)`` per identity.

    Returns four lists indexed by identity q: the device crops [n_q,S,S,3] of the frames where q is present (frame
    order), the 256 x 256 device crops (what resize_frames returns), ``present`` float64 [F] and ``tfm_array`` (M or
    ``[]`` per frame): the inputs of ``core.swap_identity_frames`` and ``blend.blend_swaps(..., valid=present)``.

    One deliberate difference from the reference: every identity gets exactly one entry per frame.  The reference
    leaves its lists ragged when there are T > 1 targets and a frame has one face without ``set_target`` (it appends
    to identity 0 only), and for a faceless frame (it appends T entries to identity 0); here identities q > 0, and
    faceless frames, get ``[]``.  For T = 1 the bookkeeping is the reference's."""
    _check_frames(frames, "crop_frames_and_get_transforms")
    dev = frames.device
    if len(kps_per_frame) != frames.shape[0]:
        raise RuntimeError("ghost_amd: one keypoint entry per frame is needed")
    T = target_embeds.shape[0]
    matches = {}
    todo = frames_to_match(kps_per_frame, set_target)
    if todo:
        from ..arcface.pipeline import match_faces
        _lib.require_same_device(target_embeds, dev, "target_embeds")
        tf, fi, start = [], [], {}
        for i in todo:
            start[i] = len(tf)
            for p in kps_per_frame[i]:
                tf.append(estimate_norm(p, crop_size, templates)[0])
                fi.append(i)
        faces, _ = align_crops(frames, np.stack(tf), fi, crop_size)
        embeds = torch.cat([netArc.embed_u8(faces[lo:lo + embed_batch]) for lo in range(0, len(tf), embed_batch)])
        res = [match_faces(embeds[start[i]:start[i] + len(kps_per_frame[i])], target_embeds, similarity_th)
               for i in todo]
        best = torch.stack([r[0] for r in res]).cpu().numpy()      # one copy back for all matched frames
        ok = torch.stack([r[2] for r in res]).cpu().numpy()
        matches = {i: (best[j], ok[j]) for j, i in enumerate(todo)}
    kps_array = select_keypoints(kps_per_frame, T, set_target, matches)
    present, tfm_array = frame_transforms(kps_array, crop_size, templates)
    crop_frames, resized_frames = [], []
    for q in range(T):
        fi = [i for i, m in enumerate(tfm_array[q]) if not _empty(m)]
        tf = np.stack([tfm_array[q][i] for i in fi]) if fi else np.zeros((0, 2, 3))
        c, r = align_crops(frames, tf, fi, crop_size, resize_to=256)
        crop_frames.append(c)
        resized_frames.append(r)
    return crop_frames, resized_frames, present, tfm_array
