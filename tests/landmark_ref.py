"""CPU restatement of the 106-point landmark network (test infrastructure only; the product never imports it).

Written in torch from the network's description (coordinate_reg/model/2d106det-symbol.json of the reference, as
tests/golden/landmark_2d106det.npz records it) and from ``Handler.get_without_detection_without_transform``
(coordinate_reg/image_infer.py:141-157):

    data [N,3,192,192] RGB 0..255 -> (x - 127.5) * 0.0078125
    conv_1      Convolution 3x3 s2 p1 3 -> 16, no bias
    conv_k_dw   Convolution 3x3 s1|s2 p1, groups = channels       k = 2 .. 14
    conv_k      Convolution 1x1
    conv_15     Convolution 3x3 s2 p1 512 -> 64
      each followed by BatchNorm(fix_gamma=True): (x - moving_mean) / sqrt(moving_var + eps) + beta, the stored gamma
      ignored, eps = 1e-3, and LeakyReLU(act_type='prelu'): x > 0 ? x : x * gamma[c]
    flatten0 (NCHW order) -> fc1 576 -> 212 with bias
    landmarks = ((pred.reshape(106, 2) + 1) * 96) * 1.75 - 56

fix_gamma's meaning and eps = 1e-3 are recalled from mxnet's documentation, not verified: mxnet is not installed and
there is no checkpoint, so nothing here is a reference run (numerics against mxnet are unpinned).

``store=`` emulates the 16-bit device path: the tensors the GPU path materialises in the storage type — the stem's,
every depthwise, every pointwise and conv_15's output, and the pointwise / conv_15 weights — are rounded to that
dtype; the input, every other parameter, the arithmetic in between and the fc stay in the evaluation dtype.
"""
from __future__ import annotations

import zlib
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3
DWSEP = [(2, 16, 32, 1), (3, 32, 64, 2), (4, 64, 64, 1), (5, 64, 128, 2), (6, 128, 128, 1), (7, 128, 256, 2),
         (8, 256, 256, 1), (9, 256, 256, 1), (10, 256, 256, 1), (11, 256, 256, 1), (12, 256, 256, 1),
         (13, 256, 512, 2), (14, 512, 512, 1)]
TAP_NAMES = ["conv_2", "conv_7", "conv_14", "conv_15"]
M = np.array([[0.57142857, 0., 32.], [0., 0.57142857, 32.]])       # image_infer.py:13


def conv_names() -> List[Tuple[str, Tuple[int, int, int, int]]]:
    """(prefix, weight shape) of every Convolution in graph order."""
    out = [("conv_1", (16, 3, 3, 3))]
    for k, ci, co, _s in DWSEP:
        out += [(f"conv_{k}_dw", (ci, 1, 3, 3)), (f"conv_{k}", (co, ci, 1, 1))]
    return out + [("conv_15", (64, 512, 3, 3))]


def _rng(name: str) -> np.random.Generator:
    return np.random.Generator(np.random.PCG64(zlib.crc32(name.encode())))


def make_weights() -> Dict[str, torch.Tensor]:
    """The project's key-hashed recipe: every tensor from PCG64(crc32(name)), float32."""
    p: Dict[str, np.ndarray] = {}
    for pre, shape in conv_names():
        co = shape[0]
        fan_in = shape[1] * shape[2] * shape[3]          # Cin / groups * k^2
        n = f"{pre}_conv2d_weight"
        p[n] = _rng(n).normal(0.0, np.sqrt(2.0 / fan_in), shape)
        n = f"{pre}_batchnorm_gamma"
        p[n] = _rng(n).uniform(0.5, 1.5, co)             # stored, and ignored by fix_gamma: a wrong use shows
        n = f"{pre}_batchnorm_beta"
        p[n] = _rng(n).normal(0.0, 0.1, co)
        n = f"{pre}_batchnorm_moving_mean"
        p[n] = _rng(n).normal(0.0, 0.1, co)
        n = f"{pre}_batchnorm_moving_var"
        p[n] = _rng(n).uniform(0.5, 1.5, co)
        n = f"{pre}_relu_gamma"
        p[n] = _rng(n).uniform(0.05, 0.45, co)
    p["fc1_weight"] = _rng("fc1_weight").normal(0.0, 0.1 / np.sqrt(576.0), (212, 576))
    p["fc1_bias"] = _rng("fc1_bias").normal(0.0, 0.1, 212)
    return {k: torch.from_numpy(v.astype(np.float32)) for k, v in p.items()}


def make_input(n: int, size: int = 192) -> torch.Tensor:
    """uint8 [n,size,size,3] from PCG64(7)."""
    g = np.random.Generator(np.random.PCG64(7))
    return torch.from_numpy(g.integers(0, 256, (n, size, size, 3), dtype=np.uint8))


def bn_prelu(p, pre, x):
    dt = x.dtype
    v = lambda s: p[f"{pre}_{s}"].to(dt).view(1, -1, 1, 1)
    x = (x - v("batchnorm_moving_mean")) / torch.sqrt(v("batchnorm_moving_var") + EPS) + v("batchnorm_beta")
    return torch.where(x > 0, x, x * v("relu_gamma"))


def forward(p: Dict[str, torch.Tensor], x_u8: torch.Tensor, bgr: bool = True, dtype=torch.float64,
            store: Optional[torch.dtype] = None):
    """x_u8 [N,192,192,3] -> (pred [N,212], {tap name: NCHW tensor}) in ``dtype``."""
    rnd = (lambda t: t.to(store).to(dtype)) if store is not None else (lambda t: t)
    x = x_u8.flip(-1) if bgr else x_u8
    x = (x.permute(0, 3, 1, 2).to(dtype) - 127.5) * 0.0078125
    w = lambda n: p[n].to(dtype)
    taps = {}
    x = rnd(bn_prelu(p, "conv_1", F.conv2d(x, w("conv_1_conv2d_weight"), stride=2, padding=1)))
    for k, ci, _co, s in DWSEP:
        x = rnd(bn_prelu(p, f"conv_{k}_dw", F.conv2d(x, w(f"conv_{k}_dw_conv2d_weight"), stride=s, padding=1,
                                                      groups=ci)))
        x = rnd(bn_prelu(p, f"conv_{k}", F.conv2d(x, rnd(w(f"conv_{k}_conv2d_weight")))))
        if f"conv_{k}" in TAP_NAMES:
            taps[f"conv_{k}"] = x
    x = rnd(bn_prelu(p, "conv_15", F.conv2d(x, rnd(w("conv_15_conv2d_weight")), stride=2, padding=1)))
    taps["conv_15"] = x
    pred = x.flatten(1) @ w("fc1_weight").t() + w("fc1_bias")
    return pred, taps


def landmarks_of(pred: torch.Tensor) -> torch.Tensor:
    """[N,212] -> [N,106,2] in the 224 crop's pixel coordinates (image_infer.py:152-155, IM = [[1.75,0,-56],...])."""
    return (pred.reshape(pred.shape[0], 106, 2) + 1.0) * 96.0 * 1.75 - 56.0
