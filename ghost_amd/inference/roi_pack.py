"""Packed ROI transfer: the rectangles of a plan cross the host link as one copy per chunk of patches, not as one 2-D
copy per rectangle.

``upload_rois`` / ``download_rois`` issue one ``hipMemcpy2DAsync`` per patch; those copies run at 5-11 GB/s, bound the
ROI chain and are asynchronous only from pinned frames.  Here, per chunk of patches:

* up: worker threads pack the rectangles' rows into a pinned staging buffer (``ghost_roi_pack_host``), one plain copy
  moves the chunk's byte range, and ``ghost_roi_unpack_u8`` spreads the packed rows over the canvas;
* down: ``ghost_roi_unpack_u8`` gathers the canvas rectangles into packed rows, one copy brings the chunk back, and the
  worker threads scatter it into the frames.

Only the staging buffer is pinned: the frames can be any host memory.  The layout is the library's
(``ghost_roi_packed_layout``); the canvas, the plan and every check are those of ``roi.py``.  The path is opt-in; the
per-patch functions are unchanged.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from .roi import RoiPlan, _check_patches, _frame_pointers

# defaults taken from the sweep of tools/bench_roi_packed.py (profiles/roi_packed_ab.txt)
DEFAULT_THREADS = 8
DEFAULT_CHUNK_BYTES = 32 << 20


def packed_layout(plan: RoiPlan) -> Tuple[np.ndarray, int]:
    """``(offsets int64 [Np], total)``: where each rectangle of the plan starts in a packed buffer, and the buffer's
    size in bytes (``ghost_roi_packed_layout``; cached on the plan)."""
    got = getattr(plan, "_packed_layout", None)
    if got is None:
        rects = np.ascontiguousarray(plan.rects, np.int32)
        offsets = np.zeros(plan.n_patches, np.int64)
        total = C.c_int64(0)
        _lib.check(_lib.load().ghost_roi_packed_layout(rects.ctypes.data, plan.n_patches, offsets.ctypes.data,
                                                       C.byref(total)), "packed_layout")
        offsets.flags.writeable = False
        got = plan._packed_layout = (offsets, int(total.value))
    return got


class RoiStaging:
    """One pinned host buffer and one device buffer of ``nbytes`` for the packed transfers, reusable for any plan whose
    packed total fits.  It remembers an event recorded after the last host-to-device copy that read its host buffer
    and one after the last device-to-host copy that wrote it (and one after the last kernel that used its device
    buffer); every later use waits on them before touching the buffers again, so back-to-back calls need no
    synchronise in between."""

    def __init__(self, nbytes: int, device):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"ghost_amd: RoiStaging lives on a ROCm GPU (MI355X); got device {dev}")
        if int(nbytes) < 0:
            raise RuntimeError("ghost_amd: RoiStaging needs nbytes >= 0")
        self.nbytes = int(nbytes)
        self.device = torch.device(dev.type, torch.cuda.current_device() if dev.index is None else dev.index)
        self.host = torch.empty(self.nbytes, dtype=torch.uint8, pin_memory=True)
        self.dev = torch.empty(self.nbytes, dtype=torch.uint8, device=self.device)
        self.h2d_event: Optional[torch.cuda.Event] = None
        self.d2h_event: Optional[torch.cuda.Event] = None
        self.dev_event: Optional[torch.cuda.Event] = None

    def acquire(self, stream) -> None:
        """Before the buffers are touched again: the host waits for the copies that still use the host buffer, and
        ``stream`` for whatever still uses the device buffer."""
        for ev in (self.h2d_event, self.d2h_event):
            if ev is not None:
                ev.synchronize()
        for ev in (self.h2d_event, self.d2h_event, self.dev_event):
            if ev is not None:
                stream.wait_event(ev)


def _device(device, what: str) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"ghost_amd: {what} runs only on a ROCm GPU (MI355X); got device {dev}")
    return dev


def _same_device(a: torch.device, b: torch.device) -> bool:
    ia = torch.cuda.current_device() if a.index is None else a.index
    ib = torch.cuda.current_device() if b.index is None else b.index
    return a.type == b.type and ia == ib


def _staging(staging, plan: RoiPlan, dev: torch.device, total: int, what: str) -> RoiStaging:
    if staging is None:
        cache = plan.__dict__.setdefault("_packed_staging", {})
        staging = cache.get(str(dev))
        if staging is None:
            staging = cache[str(dev)] = RoiStaging(total, dev)
        return staging
    if not isinstance(staging, RoiStaging):
        raise RuntimeError(f"ghost_amd: {what}: staging must be a RoiStaging")
    if staging.nbytes < total:
        raise RuntimeError(f"ghost_amd: {what}: the staging buffer holds {staging.nbytes} bytes, the plan packs to "
                           f"{total}")
    if not _same_device(staging.device, dev):
        raise RuntimeError(f"ghost_amd: {what}: the staging buffer is on {staging.device}, not on {dev}")
    return staging


def _threads(threads) -> int:
    t = int(threads)
    if t < 0:
        raise RuntimeError("ghost_amd: threads must be >= 0 (0: the default)")
    return t or DEFAULT_THREADS


def _chunks(plan: RoiPlan, chunk_bytes) -> List[Tuple[int, int, int, int]]:
    """Patch ranges of about ``chunk_bytes`` packed bytes: (p0, p1, first byte, end byte) each, at least one patch."""
    offsets, total = packed_layout(plan)
    cb = DEFAULT_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    if cb <= 0:
        raise RuntimeError("ghost_amd: chunk_bytes must be positive")
    Np, out, p0 = plan.n_patches, [], 0
    ends = np.append(offsets[1:], total)
    while p0 < Np:
        # the last patch whose end lies within chunk_bytes of the chunk's first byte (one patch at the least), and no
        # more than one launch takes
        p1 = int(np.searchsorted(ends, offsets[p0] + cb, side="right"))
        p1 = min(max(p1, p0 + 1), p0 + 65535, Np)
        out.append((p0, p1, int(offsets[p0]), int(ends[p1 - 1])))
        p0 = p1
    return out


class _Call:
    """The arguments one packed transfer hands the library for every chunk."""

    def __init__(self, patches, plan, ptrs, staging):
        self.lib, self.plan, self.patches, self.st = _lib.load(), plan, patches, staging
        self.offsets, self.total = packed_layout(plan)
        self.rects = np.ascontiguousarray(plan.rects, np.int32)
        self.per_patch = np.ascontiguousarray(ptrs[plan.frame])
        dev = patches.device
        self.rects_d = plan.device("rects", dev)
        key = ("packed_offsets", str(dev))
        if key not in plan._dev:
            plan._dev[key] = torch.from_numpy(np.array(self.offsets)).to(dev)
        self.offsets_d = plan._dev[key]

    def host(self, p0: int, p1: int, to_staging: bool, threads: int, what: str) -> None:
        H, W = self.plan.frame_hw
        _lib.check(self.lib.ghost_roi_pack_host(
            self.st.host.data_ptr(), self.st.nbytes, self.rects.ctypes.data, self.offsets.ctypes.data,
            self.per_patch.ctypes.data, self.plan.n_patches, p0, p1, H, W, 1 if to_staging else 0, threads), what)

    def kernel(self, p0: int, p1: int, to_canvas: bool, what: str) -> None:
        Ph, Pw = self.plan.canvas
        _lib.check(self.lib.ghost_roi_unpack_u8(
            self.patches.data_ptr(), Ph * Pw * 3, self.plan.n_patches, Ph, Pw, self.rects_d.data_ptr(),
            self.offsets_d.data_ptr(), self.st.dev.data_ptr(), self.st.nbytes, p0, p1, 1 if to_canvas else 0,
            _lib.stream_ptr(self.patches.device)), what)


def upload_rois_packed(frames_host, plan: RoiPlan, device, out: Optional[torch.Tensor] = None,
                       staging: Optional[RoiStaging] = None, chunk_bytes: Optional[int] = None,
                       threads: int = 0) -> torch.Tensor:
    """``upload_rois`` through a packed staging buffer: the same frame types and checks, the same canvas (inside the
    rectangles the same bytes, outside them nothing is written), but the frames need not be pinned.  Per chunk of
    about ``chunk_bytes`` packed bytes the host packs the rectangles' rows (``threads`` workers), one copy on the
    current stream moves the chunk and one kernel spreads it over the canvas; the host packs chunk k+1 while chunk k
    is in flight.  ``staging``: a ``RoiStaging`` to reuse (default: one kept on the plan)."""
    what = "upload_rois_packed"
    ptrs = _frame_pointers(frames_host, plan, what, writable=False)
    dev = _device(device, what)
    nt = _threads(threads)
    chunks = _chunks(plan, chunk_bytes)
    total = packed_layout(plan)[1]
    if staging is not None:
        _staging(staging, plan, dev, total, what)
    if out is None:
        out = torch.empty(plan.n_patches, plan.canvas[0], plan.canvas[1], 3, dtype=torch.uint8, device=dev)
    _check_patches(out, plan, what)
    if staging is not None and not _same_device(staging.device, out.device):
        raise RuntimeError(f"ghost_amd: {what}: the staging buffer is on {staging.device}, the canvas on {out.device}")
    if not plan.n_patches or not total:
        return out
    st = _staging(staging, plan, out.device, total, what)
    call = _Call(out, plan, ptrs, st)
    with torch.cuda.device(out.device):
        cur = torch.cuda.current_stream(out.device)
        st.acquire(cur)
        for p0, p1, b0, b1 in chunks:
            if b1 == b0:
                continue
            call.host(p0, p1, True, nt, what)
            st.dev[b0:b1].copy_(st.host[b0:b1], non_blocking=True)
            st.h2d_event = torch.cuda.Event()
            st.h2d_event.record(cur)
            call.kernel(p0, p1, True, what)
        st.dev_event = torch.cuda.Event()
        st.dev_event.record(cur)
    return out


def download_rois_packed(patches: torch.Tensor, plan: RoiPlan, frames_host, staging: Optional[RoiStaging] = None,
                         chunk_bytes: Optional[int] = None, threads: int = 0) -> None:
    """``download_rois`` through a packed staging buffer.  Per chunk: one kernel gathers the canvas rectangles into
    packed rows, one copy on the current stream brings them to the host, and an event marks the chunk; the host waits
    for chunk k's event and scatters it into the frames (``threads`` workers) while the later chunks copy.  Unlike
    ``download_rois`` it returns with the frames written; it waits on its own events only, never on the device."""
    what = "download_rois_packed"
    _check_patches(patches, plan, what)
    ptrs = _frame_pointers(frames_host, plan, what, writable=True)
    nt = _threads(threads)
    chunks = _chunks(plan, chunk_bytes)
    total = packed_layout(plan)[1]
    if not plan.n_patches or not total:
        if staging is not None:
            _staging(staging, plan, patches.device, total, what)
        return
    st = _staging(staging, plan, patches.device, total, what)
    call = _Call(patches, plan, ptrs, st)
    with torch.cuda.device(patches.device):
        cur = torch.cuda.current_stream(patches.device)
        st.acquire(cur)
        done = []
        for p0, p1, b0, b1 in chunks:
            if b1 == b0:
                continue
            call.kernel(p0, p1, False, what)
            st.host[b0:b1].copy_(st.dev[b0:b1], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cur)
            done.append((p0, p1, ev))
        if done:
            st.d2h_event = st.dev_event = done[-1][2]
        for p0, p1, ev in done:
            ev.synchronize()
            call.host(p0, p1, False, nt, what)
