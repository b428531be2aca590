"""The ``--use_sr`` surface around the generator: ``Pix2PixModel`` (models/pix2pix_model.py, inference mode only)
and ``face_enhancement`` (utils/inference/video_processing.py:263-285)."""
from __future__ import annotations

from typing import List

import numpy as np
import torch

from .generator import LIPSPADEGenerator


class Pix2PixModel:
    """``Pix2PixModel(opt)`` with ``.netG`` and ``model(data, mode='inference2') -> netG(data['label'])``
    (inference.py:44-50 builds it, loads netG's checkpoint, and calls ``netG.train()``: the generator here always
    runs with train-mode semantics).  ``state_dict``: optional generator checkpoint to load (strict)."""

    def __init__(self, opt=None, state_dict=None, **netg_kwargs):
        self.opt = opt
        self.netG = LIPSPADEGenerator(opt, **netg_kwargs)
        if state_dict is not None:
            self.netG.load_state_dict(state_dict, strict=True)

    def __call__(self, data, mode="inference2"):
        if mode != "inference2":
            raise NotImplementedError(f"ghost_amd: Pix2PixModel supports only mode='inference2', got {mode!r}")
        return self.netG(data["label"])


def _device_of(model) -> torch.device:
    netg = getattr(model, "netG", None)
    if isinstance(netg, torch.nn.Module):
        return next(netg.parameters()).device
    dev = getattr(model, "device", None)
    if dev is None:
        raise RuntimeError("ghost_amd: face_enhancement needs a model with .netG (or .device)")
    return torch.device(dev)


@torch.no_grad()
def face_enhancement(final_frames: List, model, batch_size: int = 20, return_device: bool = False):
    """Run every swapped 256 x 256 crop through the enhancer, list in / list out as the reference:
    ``final_frames[i]`` is the crop list of target i, uint8 BGR [256,256,3] arrays with ``[]`` where a frame has no
    face (kept in place).  Faces are taken in order in chunks of ``batch_size``; a chunk is one generator call, and
    since the generator normalises with its batch's statistics the chunking (20 in the reference) is part of the
    result.  Per chunk: BGR u8 -> RGB / 255 -> generator -> clamp(. * 255, 0, 255) truncated to u8 -> BGR.

    An entry may be a host array, a host tensor or a device uint8 tensor; ``final_frames[i]`` may also be one
    device uint8 tensor [n,256,256,3].  Returns the list of lists of host arrays; with ``return_device`` also, per
    target, the device uint8 BGR tensor [faces,256,256,3] (None without faces)."""
    if batch_size < 1:
        raise ValueError("ghost_amd: batch_size must be >= 1")
    dev = _device_of(model)      # a generator on the host raises in its forward: there is no CPU path
    out_all, dev_all = [], []
    for frames in final_frames:
        if isinstance(frames, torch.Tensor):
            frames = list(frames.unbind(0))
        enhanced = list(frames)
        face_idx = [j for j, x in enumerate(frames) if not isinstance(x, list)]      # [] marks a frame without a face
        faces = []
        for j in face_idx:
            f = frames[j]
            t = f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f))
            if t.dtype != torch.uint8 or tuple(t.shape) != (256, 256, 3):
                raise RuntimeError(f"ghost_amd: crops must be uint8 [256,256,3], got {t.dtype} {tuple(t.shape)}")
            faces.append(t.to(dev, non_blocking=True))
        results = []
        for k in range(0, len(faces), batch_size):
            chunk = torch.stack(faces[k:k + batch_size])                        # [b,256,256,3] BGR u8
            # RGB in [0,1] as ToTensor's v / 255: a tensor divisor, because a device division by a Python scalar
            # multiplies by the rounded reciprocal and lands one ulp off for some bytes
            x = chunk.flip(-1).permute(0, 3, 1, 2).float() / torch.full((), 255.0, device=chunk.device)
            y = model({"image": x, "label": x}, mode="inference2")
            y = torch.clamp(y.float() * 255, 0, 255).to(torch.uint8)
            results.append(y.permute(0, 2, 3, 1).flip(-1).contiguous())
        dres = torch.cat(results) if results else None
        if dres is not None:
            host = dres.cpu().numpy()
            for n, j in enumerate(face_idx):
                enhanced[j] = host[n]
        out_all.append(enhanced)
        dev_all.append(dres)
    return (out_all, dev_all) if return_device else out_all


__all__ = ["Pix2PixModel", "face_enhancement"]
