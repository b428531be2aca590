"""Drop-in for insightface's ``SCRFD`` (``scrfd_10g_bnkps``) behind ``Face_detect_crop``.

The reference runs the detector through onnxruntime on the host, one letterboxed 640 x 640 image per call
(insightface_func/face_detect_crop_multi.py:54-93).  ``SCRFD`` holds the network's tensors under the mmdet
checkpoint's names with BatchNorm folded (pack.py) and runs the letterbox, the network and ``SCRFD.detect``'s
post-processing for a batch of device-resident frames in one call into libghost_amd.so (det_runtime.hip).  fp32
parameters run the exact path (the default, as the reference's onnxruntime run); ``.half()`` or
``compute_dtype=torch.float16`` / ``torch.bfloat16`` stores activations and the MFMA convs' weights in 16 bits; the
first stem conv, the output convs, the nine maps and the post-processing stay fp32 (DESIGN.md §12 says which 16-bit
type to prefer).
There is no CPU path.  The graph and parity against onnxruntime are unpinned.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Mapping, Optional

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from .._packed import NativeRuntime, PackedModule, load_named, u8_rows
from .pack import (MAX_CANDIDATES, NMS_THRESH, NUM_ANCHORS, STRIDES, TAPS, letterbox_geometry, pack_detector,
                   param_specs, units)

# frames per native call at 640 x 640 (scaled by the canvas area otherwise): bounds the workspace, which is
# ghost_det_workspace_bytes(chunk) per stream — about 80 MB per 640 x 640 frame in fp32, half that in 16 bits
CHUNK_640 = 8


class _Runtime(NativeRuntime):
    def __init__(self, dtype, det_size, slots):
        super().__init__("det", "detector ", dtype, slots, _lib.gdtype(dtype), det_size[0], det_size[1])
        self.det_size = det_size


class SCRFD(PackedModule):
    def __init__(self, det_size=(640, 640), compute_dtype: Optional[torch.dtype] = None):
        super().__init__()
        self.compute_dtype = compute_dtype
        self.det_size = self._check_size(det_size)
        relu = {u.name: u.relu and not u.name.endswith(".conv2") for u in units()}
        g = torch.Generator().manual_seed(0)
        for name, shape in param_specs():
            if name.endswith(".weight"):
                fan_in = int(np.prod(shape[1:]))
                t = torch.randn(shape, generator=g) * ((2.0 if relu[name[:-7]] else 0.5) / fan_in) ** 0.5
            elif name.endswith(".bias"):
                t = torch.zeros(shape)
            else:
                t = torch.ones(shape)
            self._register(name, t)
        self._init_packed()

    def _register(self, name: str, t: torch.Tensor) -> None:
        """A parameter under its dotted checkpoint name: the containers in between are plain modules, so
        ``state_dict()`` keys are the checkpoint's."""
        mod = self
        *path, leaf = name.split(".")
        for part in path:
            if not hasattr(mod, part):
                mod.add_module(part, nn.Module())
            mod = getattr(mod, part)
        mod.register_parameter(leaf, nn.Parameter(t, requires_grad=False))

    @staticmethod
    def _check_size(det_size):
        w, h = int(det_size[0]), int(det_size[1])
        if w <= 0 or h <= 0 or w % 32 or h % 32:
            raise ValueError(f"ghost_amd: det_size must be positive multiples of 32, got {det_size}")
        return (w, h)

    def set_det_size(self, det_size) -> None:
        """``prepare(det_size=...)``: (Wd, Hd)."""
        det_size = self._check_size(det_size)
        if det_size != self.det_size:
            self.det_size = det_size
            self._invalidate()

    # -- weights ---------------------------------------------------------------------
    def load_arrays(self, mapping: Mapping) -> None:
        """Load ``{name: array}`` with exactly ``pack.param_specs()``'s names and shapes; values are numpy arrays,
        torch tensors or anything with ``.asnumpy()``."""
        load_named(dict(self.named_parameters()), dict(param_specs()), mapping, "SCRFD")
        self._invalidate()

    def _dtype(self):
        if self.compute_dtype is not None:
            return self.compute_dtype
        dt = next(self.parameters()).dtype
        return dt if dt in (torch.float16, torch.bfloat16) else torch.float32

    def _runtime(self, device):
        dt, size = self._dtype(), self.det_size
        return self._cached_runtime(device, (dt, size), lambda sd: _Runtime(dt, size, pack_detector(sd, dt)))

    def chunk_frames(self) -> int:
        """Frames per native call."""
        return max(1, CHUNK_640 * 640 * 640 // (self.det_size[0] * self.det_size[1]))

    def _workspace(self, rt, dev):
        """One workspace per stream, sized for a full chunk and used for a shorter last chunk as well: a module holds
        at most ``ghost_det_workspace_bytes(chunk_frames())`` per stream it is called on (4 streams are kept)."""
        return rt.batch_workspace(self.chunk_frames(), dev)

    def plan(self, N: int) -> list:
        """The launches of one detect call over N frames (ghost_det_plan; needs no device)."""
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(lib.ghost_det_create(_lib.gdtype(self._dtype()), self.det_size[0], self.det_size[1], C.byref(h)),
                   "ghost_det_create")
        try:
            need = lib.ghost_det_plan(h, N, None, 0)
            if need < 0:
                _lib.check(int(need), "ghost_det_plan")
            buf = C.create_string_buffer(int(need))
            lib.ghost_det_plan(h, N, buf, need)
            return [s for s in buf.value.decode().split("\n") if s]
        finally:
            lib.ghost_det_destroy(h)

    # -- execution -------------------------------------------------------------------
    @staticmethod
    def _check_frames(x, what):
        _lib.require_gpu(x, what)
        if x.dtype != torch.uint8 or x.ndim != 4 or x.shape[3] != 3 or x.shape[1] < 1 or x.shape[2] < 1:
            raise RuntimeError(f"ghost_amd: {what} takes uint8 BGR frames [F,H,W,3], got {x.dtype} {tuple(x.shape)}")
        return u8_rows(x)

    def _maps(self, N, dev):
        Wd, Hd = self.det_size
        out = []
        for ch in (NUM_ANCHORS, NUM_ANCHORS * 4, NUM_ANCHORS * 10):
            out += [torch.empty(N, Hd // s, Wd // s, ch, dtype=torch.float32, device=dev) for s in STRIDES]
        return out

    def _forward(self, x, bs, taps=None):
        rt = self._runtime(x.device)
        F_, H, W = x.shape[:3]
        maps = self._maps(F_, x.device)
        if F_:
            new_h, new_w, _ = letterbox_geometry(H, W, self.det_size)
            ws = self._workspace(rt, x.device)
            step = self.chunk_frames()
            for a in range(0, F_, step):
                n = min(step, F_ - a)
                ptrs = (C.c_void_p * 9)(*[t[a].data_ptr() for t in maps])
                with rt.taps([t[a].data_ptr() for t in taps], "detector taps") if taps else contextlib.nullcontext():
                    _lib.check(rt.lib.ghost_det_forward_u8(rt.h, x[a].data_ptr(), bs, n, H, W, new_h, new_w, ptrs,
                                                           ws.data_ptr(), ws.numel(), _lib.stream_ptr(x.device)),
                               "SCRFD.forward")
        return [t.permute(0, 3, 1, 2) for t in maps]

    @torch.no_grad()
    def forward(self, frames: torch.Tensor):
        """frames: uint8 BGR [F,H,W,3] on the GPU -> the nine maps as float32 NCHW views: scores [F,2,Hl,Wl], boxes
        [F,8,Hl,Wl] and keypoints [F,20,Hl,Wl] for strides 8, 16, 32 (scores x 3, boxes x 3, keypoints x 3).  Frames
        go to the native call ``chunk_frames()`` at a time, as in ``detect_frames``."""
        return self._forward(*self._check_frames(frames, "SCRFD.forward"))

    @torch.no_grad()
    def forward_taps(self, frames: torch.Tensor):
        """forward + the stored outputs of the stem (after its pool), stage 1, stage 4 and P3 as NCHW views in the
        compute dtype."""
        x, bs = self._check_frames(frames, "SCRFD.forward_taps")
        rt = self._runtime(x.device)
        Wd, Hd = self.det_size
        bufs = [torch.empty(x.shape[0], Hd // s, Wd // s, c, dtype=rt.dtype, device=x.device) for _n, c, s in TAPS]
        maps = self._forward(x, bs, bufs)
        return maps, [t.permute(0, 3, 1, 2) for t in bufs]

    @torch.no_grad()
    def detect_frames(self, frames: torch.Tensor, thresh: float = 0.5, max_faces: int = 256,
                      return_anchor: bool = False):
        """``SCRFD.detect`` for every frame of a uint8 BGR [F,H,W,3] device tensor: det float32 [F,max_faces,5]
        (x1, y1, x2, y2, score in frame pixels), kps float32 [F,max_faces,5,2] and count int32 [F,2] = (kept,
        candidates), on the device, in kept order and zero beyond (with ``return_anchor`` also the kept candidates'
        anchor indices, int32 [F,max_faces]).  Nothing is copied to the host and nothing synchronises; ``check_counts``
        judges the counts once they are on the host.  Frames go to the native call ``chunk_frames()`` at a time."""
        x, bs = self._check_frames(frames, "SCRFD.detect_frames")
        if max_faces <= 0:
            raise ValueError("ghost_amd: max_faces must be positive")
        rt = self._runtime(x.device)
        F_, H, W = x.shape[:3]
        dev = x.device
        det = torch.empty(F_, max_faces, 5, dtype=torch.float32, device=dev)
        kps = torch.empty(F_, max_faces, 5, 2, dtype=torch.float32, device=dev)
        anchor = torch.empty(F_, max_faces, dtype=torch.int32, device=dev)
        count = torch.empty(F_, 2, dtype=torch.int32, device=dev)
        new_h, new_w, det_scale = letterbox_geometry(H, W, self.det_size)
        step = self.chunk_frames()
        ws = self._workspace(rt, dev) if F_ else None
        for a in range(0, F_, step):
            n = min(step, F_ - a)
            _lib.check(rt.lib.ghost_det_detect_u8(rt.h, x[a].data_ptr(), bs, n, H, W, new_h, new_w, det_scale,
                                                  float(thresh), NMS_THRESH, max_faces, det[a].data_ptr(),
                                                  kps[a].data_ptr(), anchor[a].data_ptr(), count[a].data_ptr(),
                                                  ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)),
                       "SCRFD.detect_frames")
        return (det, kps, count, anchor) if return_anchor else (det, kps, count)

    @staticmethod
    def check_counts(count) -> None:
        """count: host [F,2].  More than 4096 candidates in a frame (only the first 4096 in anchor order were
        considered) is an error that names the frame."""
        c = np.asarray(count)
        over = np.flatnonzero(c[:, 1] > MAX_CANDIDATES)
        if len(over):
            raise RuntimeError(f"ghost_amd: frame {int(over[0])} has {int(c[over[0], 1])} detector candidates, above "
                               f"the capacity of {MAX_CANDIDATES}; raise the threshold")
