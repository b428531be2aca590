"""Drop-in for the mxnet ``2d106det`` model behind ``coordinate_reg.image_infer.Handler``.

The reference loads ``coordinate_reg/model/2d106det`` with ``mx.model.load_checkpoint`` and runs it on the host, one
192 x 192 crop per call (image_infer.py:111-157).  ``Landmark106`` holds the same tensors under the checkpoint's own
names, so ``state_dict()`` keys are the checkpoint's keys, and runs the network on the MI355X in one call into
libghost_amd.so (lmk_runtime.hip): the uint8 stem, one fused depthwise-separable kernel per conv_2 .. conv_14, the
implicit-GEMM conv_15 and an fp32 fc.  fp32 parameters run the exact path (the default, as the reference's mxnet
run); ``.half()`` or ``compute_dtype=torch.float16`` / ``torch.bfloat16`` stores activations and the 1x1 / conv_15
weights in 16 bits (fp16 is the sensible 16-bit choice here: DESIGN.md §11).  There is no CPU path.  Parity against
mxnet is unpinned: no mxnet and no checkpoint are available offline.
"""
from __future__ import annotations

from typing import Mapping, Optional

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from .._packed import NativeRuntime, PackedModule, load_named, u8_rows
from .pack import CROP_SIZE, IN_SIZE, N_POINTS, TAPS, pack_landmark, param_specs


class _Runtime(NativeRuntime):
    def __init__(self, dtype, slots):
        super().__init__("lmk", "landmark ", dtype, slots, _lib.gdtype(dtype))


class Landmark106(PackedModule):
    def __init__(self, compute_dtype: Optional[torch.dtype] = None):
        super().__init__()
        self.compute_dtype = compute_dtype
        g = torch.Generator().manual_seed(0)
        for name, shape, kind in param_specs():
            if kind == "aux":
                t = torch.ones(shape) if name.endswith("moving_var") else torch.zeros(shape)
                self.register_buffer(name, t)
                continue
            if name.endswith("_relu_gamma"):
                t = torch.full(shape, 0.25)
            elif name.endswith("_gamma"):
                t = torch.ones(shape)
            elif name.endswith("weight"):
                fan_in = int(np.prod(shape[1:]))
                t = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
            else:
                t = torch.zeros(shape)
            self.register_parameter(name, nn.Parameter(t, requires_grad=False))
        self._init_packed()

    # -- weights ---------------------------------------------------------------------
    def load_mxnet_params(self, arg_params: Mapping, aux_params: Optional[Mapping] = None) -> None:
        """Load what ``mx.model.load_checkpoint`` (two mappings) or ``mx.nd.load`` (one mapping with ``arg:`` /
        ``aux:`` prefixed keys) returns: values are numpy arrays, torch tensors or anything with ``.asnumpy()``."""
        given = {}
        for m in (arg_params, aux_params or {}):
            for k, v in m.items():
                k = k.split(":", 1)[1] if k.startswith(("arg:", "aux:")) else k
                given[k] = v
        own = dict(self.named_parameters())
        own.update(dict(self.named_buffers()))
        load_named(own, {n: s for n, s, _ in param_specs()}, given, "2d106det")
        self._invalidate()

    def _dtype(self):
        if self.compute_dtype is not None:
            return self.compute_dtype
        return self.fc1_weight.dtype if self.fc1_weight.dtype in (torch.float16, torch.bfloat16) else torch.float32

    def _runtime(self, device):
        dt = self._dtype()
        return self._cached_runtime(device, dt, lambda sd: _Runtime(dt, pack_landmark(sd, dt)))

    # -- execution -------------------------------------------------------------------
    @staticmethod
    def _check_u8(x, size, what):
        _lib.require_gpu(x, what)
        if x.dtype != torch.uint8 or x.ndim != 4 or tuple(x.shape[1:]) != (size, size, 3):
            raise RuntimeError(f"ghost_amd: {what} takes uint8 [N,{size},{size},3], got {x.dtype} {tuple(x.shape)}")
        return u8_rows(x)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, bgr: bool = True) -> torch.Tensor:
        """x: uint8 [N,192,192,3] on the GPU (the warped crop; B,G,R order unless ``bgr=False``) -> fc1's output,
        float32 [N,212].  The batch dimension may be strided."""
        x, bs = self._check_u8(x, IN_SIZE, "Landmark106.forward")
        rt = self._runtime(x.device)
        N = x.shape[0]
        pred = torch.empty(N, 2 * N_POINTS, dtype=torch.float32, device=x.device)
        if N == 0:
            return pred
        ws = rt.batch_workspace(N, x.device)
        _lib.check(rt.lib.ghost_lmk_forward(rt.h, x.data_ptr(), bs, 1 if bgr else 0, N, pred.data_ptr(), ws.data_ptr(),
                                            ws.numel(), _lib.stream_ptr(x.device)), "Landmark106.forward")
        return pred

    @torch.no_grad()
    def forward_taps(self, x: torch.Tensor, bgr: bool = True):
        """forward + the stored outputs of conv_2, conv_7, conv_14 and conv_15 as NCHW views in the compute dtype."""
        x, _ = self._check_u8(x, IN_SIZE, "Landmark106.forward_taps")
        rt = self._runtime(x.device)
        N = x.shape[0]
        bufs = [torch.empty(N, s, s, c, dtype=rt.dtype, device=x.device) for _n, c, s in TAPS]
        with rt.taps([t.data_ptr() for t in bufs], "landmark taps"):
            pred = self.forward(x, bgr)
        return pred, [t.permute(0, 3, 1, 2) for t in bufs]

    @torch.no_grad()
    def landmarks_u8(self, crops: torch.Tensor, return_pred: bool = False):
        """``get_without_detection_without_transform`` over a batch: uint8 BGR crops [N,224,224,3] on the GPU ->
        float32 [N,106,2] on the GPU, in the crop's pixel coordinates (and fc1's output with ``return_pred``)."""
        crops, bs = self._check_u8(crops, CROP_SIZE, "Landmark106.landmarks_u8")
        rt = self._runtime(crops.device)
        N = crops.shape[0]
        lm = torch.empty(N, N_POINTS, 2, dtype=torch.float32, device=crops.device)
        pred = torch.empty(N, 2 * N_POINTS, dtype=torch.float32, device=crops.device) if return_pred else None
        if N:
            ws = rt.batch_workspace(N, crops.device)
            _lib.check(rt.lib.ghost_lmk_landmarks_u8(rt.h, crops.data_ptr(), bs, N, lm.data_ptr(), _lib.ptr(pred),
                                                     ws.data_ptr(), ws.numel(), _lib.stream_ptr(crops.device)),
                       "Landmark106.landmarks_u8")
        return (lm, pred) if return_pred else lm
