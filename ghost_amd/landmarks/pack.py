"""The 2d106det layer table and its checkpoint tensors -> the slots of lmk_runtime.hip.

The table restates coordinate_reg/model/2d106det-symbol.json of the reference (tests/golden/landmark_2d106det.npz
records the file's own nodes; tests/test_landmark_cpu.py compares).  Slot layouts:

  stem.w      fp32 [27][16]              K = (ky*3 + kx)*3 + rgb channel      conv_1_conv2d_weight [16,3,3,3]
  cK.dw.w     fp32 [9][Cin]              tap ky*3 + kx                        conv_K_dw_conv2d_weight [Cin,1,3,3]
  cK.pw.w     dtype [rup(Cout,128)][rup(Cin,32)]  (network.pack.pack_conv)    conv_K_conv2d_weight [Cout,Cin,1,1]
  c15.w       dtype [128][4608]          (network.pack.pack_conv)             conv_15_conv2d_weight [64,512,3,3]
  X.scale     fp32 1 / sqrt(moving_var + BN_EPS)            gamma counts as 1 (fix_gamma), whatever is stored
  X.shift     fp32 beta - moving_mean * scale
  X.prelu     fp32 the *_relu_gamma slopes                  (X.* padded with zeros to a multiple of 128)
  fc.w        fp32 [576][212]            K = (y*3 + x)*64 + c  <- fc1_weight [212][c*9 + y*3 + x] (Flatten is NCHW)
  fc.bias     fp32 [212]
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch

from ..network.pack import pack_conv, rup

# mxnet's BatchNorm default: the symbol file sets no eps.  Recalled from mxnet's operator documentation, not
# verified (mxnet is not installed here); so is fix_gamma=True making gamma count as 1.  DESIGN.md §11.
BN_EPS = 1e-3
IN_SCALARS = (127.5, 0.0078125)     # _minusscalar0, _mulscalar0
IN_SIZE, CROP_SIZE, N_POINTS = 192, 224, 106

# (name, Cin, Cout, stride, input resolution) of the depthwise-separable blocks
DWSEP = [(2, 16, 32, 1, 96), (3, 32, 64, 2, 96), (4, 64, 64, 1, 48), (5, 64, 128, 2, 48), (6, 128, 128, 1, 24),
         (7, 128, 256, 2, 24)] + [(k, 256, 256, 1, 12) for k in range(8, 13)] + [(13, 256, 512, 2, 12),
                                                                                 (14, 512, 512, 1, 6)]
TAPS = [("conv_2", 32, 96), ("conv_7", 256, 12), ("conv_14", 512, 6), ("conv_15", 64, 3)]   # name, channels, size


def conv_layers() -> List[Tuple[str, int, int, int, int, int, int]]:
    """Every Convolution in graph order: (prefix, Cin, filters, kernel, stride, pad, groups).  Each is followed by
    ``<prefix>_batchnorm`` and ``<prefix>_relu`` (a per-channel PReLU)."""
    out = [("conv_1", 3, 16, 3, 2, 1, 1)]
    for k, ci, co, s, _ in DWSEP:
        out.append((f"conv_{k}_dw", ci, ci, 3, s, 1, ci))
        out.append((f"conv_{k}", ci, co, 1, 1, 0, 1))
    out.append(("conv_15", 512, 64, 3, 2, 1, 1))
    return out


def param_specs() -> List[Tuple[str, Tuple[int, ...], str]]:
    """(checkpoint name, shape, 'arg' | 'aux') in the symbol file's order."""
    s: List[Tuple[str, Tuple[int, ...], str]] = []
    for pre, ci, co, k, _st, _p, g in conv_layers():
        s.append((f"{pre}_conv2d_weight", (co, ci // g, k, k), "arg"))
        s.append((f"{pre}_batchnorm_gamma", (co,), "arg"))
        s.append((f"{pre}_batchnorm_beta", (co,), "arg"))
        s.append((f"{pre}_batchnorm_moving_mean", (co,), "aux"))
        s.append((f"{pre}_batchnorm_moving_var", (co,), "aux"))
        s.append((f"{pre}_relu_gamma", (co,), "arg"))
    s.append(("fc1_weight", (2 * N_POINTS, 64 * 3 * 3), "arg"))
    s.append(("fc1_bias", (2 * N_POINTS,), "arg"))
    return s


def _pad128(v: torch.Tensor) -> torch.Tensor:
    out = torch.zeros(rup(v.numel(), 128), dtype=torch.float32, device=v.device)
    out[:v.numel()] = v.float().reshape(-1)
    return out


def bn_prelu(sd: Dict[str, torch.Tensor], pre: str) -> Dict[str, torch.Tensor]:
    """BatchNorm(fix_gamma=True) in inference + the PReLU slopes of conv ``pre``: scale, shift, prelu."""
    scale = 1.0 / torch.sqrt(sd[f"{pre}_batchnorm_moving_var"].float() + BN_EPS)
    shift = sd[f"{pre}_batchnorm_beta"].float() - sd[f"{pre}_batchnorm_moving_mean"].float() * scale
    return {"scale": _pad128(scale), "shift": _pad128(shift), "prelu": _pad128(sd[f"{pre}_relu_gamma"])}


def slot_names() -> List[str]:
    names = ["stem.w"] + [f"stem.{s}" for s in ("scale", "shift", "prelu")]
    for k, *_ in DWSEP:
        for part in ("dw", "pw"):
            names += [f"c{k}.{part}.w"] + [f"c{k}.{part}.{s}" for s in ("scale", "shift", "prelu")]
    names += ["c15.w"] + [f"c15.{s}" for s in ("scale", "shift", "prelu")] + ["fc.w", "fc.bias"]
    return names


def pack_landmark(sd: Dict[str, torch.Tensor], dtype: torch.dtype) -> Dict[str, torch.Tensor]:
    """Every runtime slot -> a contiguous device tensor."""
    slots: Dict[str, torch.Tensor] = {}

    def put(slot, pre):
        for k, v in bn_prelu(sd, pre).items():
            slots[f"{slot}.{k}"] = v

    slots["stem.w"] = sd["conv_1_conv2d_weight"].float().permute(2, 3, 1, 0).reshape(27, 16)
    put("stem", "conv_1")
    for k, ci, co, _s, _h in DWSEP:
        slots[f"c{k}.dw.w"] = sd[f"conv_{k}_dw_conv2d_weight"].float().reshape(ci, 9).t()
        put(f"c{k}.dw", f"conv_{k}_dw")
        slots[f"c{k}.pw.w"] = pack_conv(sd[f"conv_{k}_conv2d_weight"], dtype)
        put(f"c{k}.pw", f"conv_{k}")
    slots["c15.w"] = pack_conv(sd["conv_15_conv2d_weight"], dtype)
    put("c15", "conv_15")
    fw = sd["fc1_weight"].float()
    slots["fc.w"] = fw.reshape(fw.shape[0], 64, 3, 3).permute(2, 3, 1, 0).reshape(576, fw.shape[0])
    slots["fc.bias"] = sd["fc1_bias"].float()
    return {k: v.contiguous() for k, v in slots.items()}
