"""``Handler`` (coordinate_reg/image_infer.py:96-157) and the landmark + mask step of ``get_final_video``
(utils/inference/video_processing.py:210-223) on the device."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from ..inference.blend import resize_u8
from ..inference.masks import _raster, face_masks, mask_params, mask_polygons_device


class Handler:
    """``handler.get_without_detection_without_transform(img)`` as the reference's ``Handler`` answers it, with the
    network on the GPU.  ``net`` is a ``Landmark106`` whose parameters are on the device.  The detector-based
    entries (``get``, ``get_without_detection``) stay the reference's."""

    def __init__(self, net, device=None):
        self.net = net
        self.device = torch.device(device) if device is not None else next(net.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("ghost_amd: Handler runs on a ROCm GPU only (no CPU path)")

    def get_without_detection_without_transform(self, img) -> np.ndarray:
        """img: uint8 BGR [224,224,3], a host array or a device tensor -> np.float32 [106,2]."""
        t = img if torch.is_tensor(img) else torch.from_numpy(np.ascontiguousarray(img))
        if t.dtype != torch.uint8 or tuple(t.shape) != (224, 224, 3):
            raise RuntimeError(f"ghost_amd: Handler takes a uint8 [224,224,3] BGR crop, got {t.dtype} {tuple(t.shape)}")
        lm = self.net.landmarks_u8(t.to(self.device)[None])
        return lm[0].cpu().numpy()


def present_runs(present: Sequence) -> List[Tuple[int, int]]:
    """[start, stop) of every run of consecutive present frames: at each start the reference's ``params[j]`` is None
    (video_processing.py:214-216 resets it on an absent frame), so the target crop's landmarks and the mask
    parameters are computed there and kept to the end of the run."""
    runs, start = [], None
    for i, p in enumerate(list(present) + [0]):
        if p and start is None:
            start = i
        elif not p and start is not None:
            runs.append((start, i))
            start = None
    return runs


def identity_masks(net, swaps256_u8: torch.Tensor, crops224_u8: torch.Tensor, present, H: int = 224, W: int = 224):
    """One identity's masks for ``blend_swaps``: swaps uint8 [F,S,S,3] (the generator's output, resized to 224 as
    video_processing.py:212 does), crops uint8 [F,224,224,3] (the target crops), present [F] (frames where the
    identity was found).  Returns (masks float32 [F,H,W] on the device, zero on absent frames; the 224 x 224 swaps;
    landmarks np.float32 [F,106,2]; params int32 [F,3]).

    The swaps' landmarks come from one batched call, the target crops' from one call over the first frame of every
    run; one device -> host copy carries the landmarks to the host-side convex hull (ghost_mask_polygons)."""
    _lib.require_gpu(swaps256_u8, "identity_masks")
    _lib.require_gpu(crops224_u8, "identity_masks")
    dev = swaps256_u8.device
    F_ = swaps256_u8.shape[0]
    pres = np.asarray(present.cpu() if torch.is_tensor(present) else present).astype(bool).reshape(-1)
    if pres.shape[0] != F_ or crops224_u8.shape[0] != F_:
        raise RuntimeError("ghost_amd: identity_masks needs F swaps, F crops and F present flags")
    swaps = swaps256_u8 if tuple(swaps256_u8.shape[1:3]) == (224, 224) else resize_u8(swaps256_u8, (224, 224))
    masks = torch.zeros(F_, H, W, dtype=torch.float32, device=dev)
    lm_all, params, idx = identity_landmarks(net, swaps, crops224_u8, pres)
    if len(idx):
        masks[torch.from_numpy(idx).to(dev)] = face_masks(lm_all[idx], params[idx], H, W, dev)
    return masks, swaps, lm_all, params


def run_indices(present: Sequence):
    """Host-side index arrays of ``identity_masks_device``, from ``present`` alone: ``idx`` int64 [P] the present
    frames, ``starts`` int64 [R] the first frame of every run (``present_runs``), and per present frame k (int32 [P])
    ``ref_index[k]`` the position in ``idx`` of the first frame of k's run (so ``idx[ref_index[k]]`` is that frame)
    and ``tgt_index[k]`` the number of k's run: where the landmarks of the present swaps and of the runs' first
    target crops stand in the two batches the network is given."""
    pres = np.asarray(present).astype(bool).reshape(-1)
    idx = np.flatnonzero(pres).astype(np.int64)
    prev = np.concatenate([[False], pres[:-1]])
    first = (pres & ~prev)[idx]                       # per present frame: it starts a run
    starts = idx[first]
    tgt_index = (np.cumsum(first) - 1).astype(np.int32)
    ref_index = np.flatnonzero(first).astype(np.int32)[tgt_index] if len(idx) else np.zeros(0, np.int32)
    return idx, starts, ref_index, tgt_index


def identity_masks_device(net, swaps256_u8: torch.Tensor, crops224_u8: torch.Tensor, present, H: int = 224,
                          W: int = 224):
    """``identity_masks`` without the round trip: the same inputs (``present`` is host data) and the same masks,
    swaps, landmarks and params bit for bit, with ``landmarks`` (float32 [F,106,2]) and ``params`` (int32 [F,3])
    device tensors, zero on absent frames.

    The parameter choice, the eyebrow expansion and the convex hull run in one launch on the landmarks where the
    network left them (ghost_mask_polygons_dev); only the index arrays of ``run_indices`` go up, without waiting.
    Between entry and return nothing is copied to the host and nothing synchronises."""
    _lib.require_gpu(swaps256_u8, "identity_masks_device")
    _lib.require_gpu(crops224_u8, "identity_masks_device")
    if torch.is_tensor(present) and present.is_cuda:
        raise RuntimeError("ghost_amd: identity_masks_device takes present as host data (a device tensor would "
                           "have to be copied back)")
    dev = swaps256_u8.device
    F_ = swaps256_u8.shape[0]
    pres = np.asarray(present).astype(bool).reshape(-1)
    if pres.shape[0] != F_ or crops224_u8.shape[0] != F_:
        raise RuntimeError("ghost_amd: identity_masks_device needs F swaps, F crops and F present flags")
    swaps = swaps256_u8 if tuple(swaps256_u8.shape[1:3]) == (224, 224) else resize_u8(swaps256_u8, (224, 224))
    masks = torch.zeros(F_, H, W, dtype=torch.float32, device=dev)
    lm_all = torch.zeros(F_, 106, 2, dtype=torch.float32, device=dev)
    params = torch.zeros(F_, 3, dtype=torch.int32, device=dev)
    idx, starts, ref_index, tgt_index = run_indices(pres)
    if not len(idx):
        return masks, swaps, lm_all, params
    d_idx, d_starts, d_ref, d_tgt = (torch.from_numpy(a).to(dev, non_blocking=True)
                                     for a in (idx, starts, ref_index, tgt_index))
    lm_sw = net.landmarks_u8(swaps.index_select(0, d_idx)).contiguous()
    lm_tg = net.landmarks_u8(crops224_u8.index_select(0, d_starts)).contiguous()
    poly, nv, pr = mask_polygons_device(lm_sw, landmarks_ref=lm_sw, ref_index=d_ref, landmarks_tgt=lm_tg,
                                        tgt_index=d_tgt)
    masks.index_copy_(0, d_idx, _raster(poly, nv, pr, H, W, None))
    lm_all.index_copy_(0, d_idx, lm_sw)
    params.index_copy_(0, d_idx, pr)
    return masks, swaps, lm_all, params


def identity_landmarks(net, swaps224_u8: torch.Tensor, crops224_u8: torch.Tensor, pres: np.ndarray):
    """The landmark calls and the parameter choice of ``identity_masks``: (landmarks np.float32 [F,106,2] of the
    swaps, zero on absent frames; params int32 [F,3]; the indices of the present frames).  ``net`` needs only
    ``landmarks_u8``."""
    F_ = swaps224_u8.shape[0]
    dev = swaps224_u8.device
    lm_all = np.zeros((F_, 106, 2), np.float32)
    params = np.zeros((F_, 3), np.int32)
    runs = present_runs(pres)
    idx = np.flatnonzero(pres)
    if not runs:
        return lm_all, params, idx
    starts = np.array([r[0] for r in runs])
    lm_dev = torch.cat([net.landmarks_u8(swaps224_u8.index_select(0, torch.from_numpy(idx).to(dev))),
                        net.landmarks_u8(crops224_u8.index_select(0, torch.from_numpy(starts).to(dev)))])
    lm_host = lm_dev.cpu().numpy()                      # the one device -> host copy
    lm_all[idx] = lm_host[:len(idx)]
    lm_tgt = lm_host[len(idx):]
    for r, (a, b) in enumerate(runs):
        params[a:b] = mask_params(lm_all[a], lm_tgt[r])
    return lm_all, params, idx
