"""The scrfd_10g_bnkps graph as one table, and its tensors -> the slots of det_runtime.hip.

The graph is recalled from the public sources (insightface ``detection/scrfd`` config ``scrfd_10g_bnkps`` on mmdet
2.x, and ``insightface/model_zoo/scrfd.py``), not verified: neither the ONNX file nor onnx / onnxruntime are available
offline (DESIGN.md §12 lists what a reader with the file should check first).  ``units()`` is the whole graph: a
correction of a width, a kernel or an order is an edit of this table (and of the mirror in det_runtime.hip's
``det_plan``, which walks the same names).

Unit names follow the mmdet checkpoint (``backbone.…``, ``neck.…``, ``bbox_head.…``) with BatchNorm folded into the
convolution it follows, as an eval-mode ONNX export has it; ``fold_bn`` does that for a training checkpoint.

Slot layouts (Npad = Cout rounded up to 128, Kpad = K rounded up to 32, zero padded):

  backbone.stem.0.w          fp32 [27][28]        K = (ky*3 + kx)*3 + rgb channel
  <unit>.w                   dtype [Npad][Kpad]   network.pack.pack_conv: K = (ky*kw + kx)*Cin + c (and the blocked
                                                  order of pack_conv where Cin % 32 == 0: the 224-channel units)
  <avg-down unit>.w          the same for the conv 2x2/s2 whose four taps are w/4: AvgPool 2x2/s2 then conv1x1, exactly
  <unit>.b                   fp32 [128k]          the bias, zero padded
  bbox_head.out.S.w          fp32 [720][30]       stride S's stride_cls | stride_reg | stride_kps as one conv 80 -> 30 (the
                                                  head kernel of det.hip): K = (ky*3 + kx)*80 + c, columns 0-1 | 2-9 | 10-29
  bbox_head.out.S.b          fp32 [32]            their biases in that order, zero padded
  bbox_head.out.S.m          fp32 [32]            the multiplier after the bias: bbox_scale on columns 2-9, 1 elsewhere
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Tuple

import numpy as np
import torch

from ..network.pack import pack_conv, rup

STEM = (28, 28, 56)                 # the deep stem's widths (recalled)
PLANES = (56, 88, 88, 224)
BLOCKS = (3, 4, 2, 3)
NECK, TOWER = 56, 80
STRIDES = (8, 16, 32)
NUM_ANCHORS = 2
MAX_CANDIDATES = 4096               # per frame, det.h kDetMaxCap
IN_SCALARS = (127.5, 128.0)         # (byte - 127.5) / 128, B <-> R swapped
NMS_THRESH = 0.4
TAPS = [("stem", 56, 4), ("layer1", 56, 4), ("layer4", 224, 32), ("p3", 56, 8)]   # name, channels, stride


class Unit(NamedTuple):
    name: str
    cin: int
    cout: int
    k: int
    stride: int
    pad: int
    relu: bool       # followed by ReLU (for a block's conv2: after the identity is added)
    role: str        # stem | conv | avgdown | cls | reg | kps


def units() -> List[Unit]:
    """Every conv unit in graph order."""
    u = [Unit("backbone.stem.0", 3, STEM[0], 3, 2, 1, True, "stem"),
         Unit("backbone.stem.3", STEM[0], STEM[1], 3, 1, 1, True, "conv"),
         Unit("backbone.stem.6", STEM[1], STEM[2], 3, 1, 1, True, "conv")]
    cin = STEM[2]
    for st, (pl, nb) in enumerate(zip(PLANES, BLOCKS)):
        for b in range(nb):
            s = 2 if st > 0 and b == 0 else 1
            nm = f"backbone.layer{st + 1}.{b}"
            u.append(Unit(f"{nm}.conv1", cin, pl, 3, s, 1, True, "conv"))
            if s == 2:   # avg_down: AvgPool 2x2/s2, then conv1x1 (downsample.0 is the pool)
                u.append(Unit(f"{nm}.downsample.1", cin, pl, 1, 1, 0, False, "avgdown"))
            u.append(Unit(f"{nm}.conv2", pl, pl, 3, 1, 1, True, "conv"))
            cin = pl
    for i in range(3):
        u.append(Unit(f"neck.lateral_convs.{i}.conv", PLANES[i + 1], NECK, 1, 1, 0, False, "conv"))
    for i in range(3):
        u.append(Unit(f"neck.fpn_convs.{i}.conv", NECK, NECK, 3, 1, 1, False, "conv"))
    for i in range(2):
        u.append(Unit(f"neck.downsample_convs.{i}.conv", NECK, NECK, 3, 2, 1, False, "conv"))
    for i in range(2):
        u.append(Unit(f"neck.pafpn_convs.{i}.conv", NECK, NECK, 3, 1, 1, False, "conv"))
    for s in STRIDES:
        for j in range(3):
            u.append(Unit(f"bbox_head.cls_stride_convs.{s}.{j}.conv", NECK if j == 0 else TOWER, TOWER, 3, 1, 1, True,
                          "conv"))
        u.append(Unit(f"bbox_head.stride_cls.{s}", TOWER, NUM_ANCHORS, 3, 1, 1, False, "cls"))
        u.append(Unit(f"bbox_head.stride_reg.{s}", TOWER, NUM_ANCHORS * 4, 3, 1, 1, False, "reg"))
        u.append(Unit(f"bbox_head.stride_kps.{s}", TOWER, NUM_ANCHORS * 10, 3, 1, 1, False, "kps"))
    return u


def scale_names() -> List[str]:
    return [f"bbox_head.scales.{i}.scale" for i in range(len(STRIDES))]


def param_specs() -> List[Tuple[str, Tuple[int, ...]]]:
    """(parameter name, shape): ``<unit>.weight`` [Co,Ci,k,k] and ``<unit>.bias`` [Co] per unit, then the three
    ``bbox_scale`` scalars."""
    s: List[Tuple[str, Tuple[int, ...]]] = []
    for u in units():
        s.append((f"{u.name}.weight", (u.cout, u.cin, u.k, u.k)))
        s.append((f"{u.name}.bias", (u.cout,)))
    return s + [(n, ()) for n in scale_names()]


def fold_bn(weight, gamma, beta, mean, var, eps: float = 1e-5):
    """A bias-free conv followed by BatchNorm (a training checkpoint) -> the conv unit of an eval-mode export:
    (weight * g, beta - mean * g) with g = gamma / sqrt(var + eps), computed in float64 and rounded once to float32."""
    w, ga, be, mu, va = (np.asarray(v, np.float64) for v in (weight, gamma, beta, mean, var))
    g = ga / np.sqrt(va + eps)
    return (w * g.reshape(-1, 1, 1, 1)).astype(np.float32), (be - mu * g).astype(np.float32)


def _pad128(v: torch.Tensor) -> torch.Tensor:
    out = torch.zeros(rup(v.numel(), 128), dtype=torch.float32, device=v.device)
    out[:v.numel()] = v.float().reshape(-1)
    return out


def slot_names() -> List[str]:
    names = []
    for u in units():
        if u.role not in ("cls", "reg", "kps"):
            names += [f"{u.name}.w", f"{u.name}.b"]
    for s in STRIDES:
        names += [f"bbox_head.out.{s}.{k}" for k in ("w", "b", "m")]
    return names


def pack_detector(sd: Dict[str, torch.Tensor], dtype: torch.dtype) -> Dict[str, torch.Tensor]:
    """Every runtime slot -> a contiguous device tensor."""
    slots: Dict[str, torch.Tensor] = {}
    for u in units():
        if u.role in ("cls", "reg", "kps"):
            continue
        w, b = sd[f"{u.name}.weight"].float(), sd[f"{u.name}.bias"].float()
        if u.role == "stem":
            slots[f"{u.name}.w"] = w.permute(2, 3, 1, 0).reshape(27, u.cout)
        elif u.role == "avgdown":
            slots[f"{u.name}.w"] = pack_conv((w * 0.25).expand(u.cout, u.cin, 2, 2), dtype)
        else:
            slots[f"{u.name}.w"] = pack_conv(w, dtype)
        slots[f"{u.name}.b"] = _pad128(b)
    for level, s in enumerate(STRIDES):
        parts = [f"bbox_head.stride_{k}.{s}" for k in ("cls", "reg", "kps")]
        w = torch.cat([sd[f"{n}.weight"].float() for n in parts])                  # [30,80,3,3]
        b = torch.cat([sd[f"{n}.bias"].float() for n in parts])
        m = torch.ones(32, dtype=torch.float32, device=w.device)
        m[2:10] = sd[scale_names()[level]].float().reshape(())
        slots[f"bbox_head.out.{s}.w"] = w.permute(2, 3, 1, 0).reshape(9 * TOWER, w.shape[0])
        slots[f"bbox_head.out.{s}.b"] = torch.cat([b, b.new_zeros(2)])
        slots[f"bbox_head.out.{s}.m"] = m
    return {k: v.contiguous() for k, v in slots.items()}


def letterbox_geometry(H: int, W: int, det_size=(640, 640)) -> Tuple[int, int, float]:
    """SCRFD.detect's resize: (new_h, new_w, det_scale) for an H x W image and det_size = (Wd, Hd), in Python floats
    truncated as insightface does; det_scale is the double new_h / H (used as float32)."""
    Wd, Hd = det_size
    im_ratio = float(H) / W
    model_ratio = float(Hd) / Wd
    if im_ratio > model_ratio:
        new_h = Hd
        new_w = int(new_h / im_ratio)
    else:
        new_w = Wd
        new_h = int(new_w * im_ratio)
    return new_h, new_w, float(new_h) / H


def select_max_num(det: np.ndarray, max_num: int, H: int, W: int) -> np.ndarray:
    """SCRFD.detect's ``max_num > 0`` rule on the host: the indices (in its order) of the ``max_num`` rows of det
    [k,5] with the largest ``area - 2 * offset_dist^2`` from the image centre (H // 2, W // 2)."""
    if max_num <= 0 or det.shape[0] <= max_num:
        return np.arange(det.shape[0])
    area = (det[:, 2] - det[:, 0]) * (det[:, 3] - det[:, 1])
    cy, cx = H // 2, W // 2
    offsets = np.vstack([(det[:, 0] + det[:, 2]) / 2 - cx, (det[:, 1] + det[:, 3]) / 2 - cy])
    values = area - np.sum(np.power(offsets, 2.0), 0) * 2.0
    return np.argsort(values)[::-1][:max_num]
