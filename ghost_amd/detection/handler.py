"""``Face_detect_crop`` (insightface_func/face_detect_crop_multi.py) as far as the video chain uses it: the five
keypoints of every detected face, with the detector on the device."""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from .pack import select_max_num


class Face_detect_crop:
    """``app = Face_detect_crop(model); app.prepare(ctx_id, det_thresh, det_size)``, then ``get`` per image or
    ``get_frames`` per clip.  ``model`` is an ``SCRFD`` whose parameters are on the device."""

    def __init__(self, model, device=None):
        self.model = model
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("ghost_amd: Face_detect_crop runs on a ROCm GPU only (no CPU path)")
        self.det_thresh = 0.5
        self.max_faces = 256

    def prepare(self, ctx_id=0, det_thresh: float = 0.5, det_size=(640, 640)) -> None:
        self.det_thresh = float(det_thresh)
        self.model.set_det_size(det_size)

    def get_frames(self, frames, max_num: int = 0) -> List[Optional[np.ndarray]]:
        """frames: uint8 BGR [F,H,W,3], a device tensor (or a host array, uploaded once) -> per frame the keypoints
        np.float32 [k,5,2] in the detector's order, or None where no face passes the threshold: the
        ``kps_per_frame`` of ``crop_frames_and_get_transforms``.  One detector call, one device -> host copy."""
        t = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames))
        t = t.to(self.device)
        F_, H, W = t.shape[:3]
        det, kps, count = self.model.detect_frames(t, self.det_thresh, self.max_faces)
        m = self.max_faces
        # counts are below 2^24: exact as float32
        host = torch.cat([det.reshape(F_, m * 5), kps.reshape(F_, m * 10), count.float()], 1).cpu().numpy()
        cnt = host[:, m * 15:].astype(np.int64)
        self.model.check_counts(cnt)
        out: List[Optional[np.ndarray]] = []
        for f in range(F_):
            k = min(int(cnt[f, 0]), m)
            if k == 0:
                out.append(None)
                continue
            d = host[f, :m * 5].reshape(m, 5)[:k]
            p = host[f, m * 5:m * 15].reshape(m, 5, 2)[:k]
            out.append(np.ascontiguousarray(p[select_max_num(d, max_num, H, W)], dtype=np.float32))
        return out

    def get(self, img, crop_size=None, max_num: int = 0) -> Optional[List[np.ndarray]]:
        """img: uint8 BGR [H,W,3], a host array or a device tensor -> a list of np.float32 [5,2] keypoint arrays, or
        None when no face is found.  ``crop_size`` is accepted for the reference's signature; alignment is
        ``ghost_amd.inference.crop_frames_and_get_transforms``'s."""
        t = img if torch.is_tensor(img) else torch.from_numpy(np.ascontiguousarray(img))
        if t.ndim != 3:
            raise RuntimeError(f"ghost_amd: Face_detect_crop.get takes one [H,W,3] image, got {tuple(t.shape)}")
        k = self.get_frames(t[None], max_num)[0]
        return None if k is None else [k[i] for i in range(k.shape[0])]
