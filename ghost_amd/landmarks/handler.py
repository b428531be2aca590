"""``Handler`` (coordinate_reg/image_infer.py:96-157) and the landmark + mask step of ``get_final_video``
(utils/inference/video_processing.py:210-223) on the device."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from ..inference.blend import resize_u8
from ..inference.masks import face_masks, mask_params


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
