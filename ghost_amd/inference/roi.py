"""The ROI (region of interest) video path: the frames stay on the host and only each face's rectangle is uploaded,
aligned, blended and downloaded.

``align.crop_frames_and_get_transforms`` -> ``core.swap_identity_frames`` -> ``masks.face_masks`` ->
``blend.blend_swaps`` carries every full frame over the host link once in each direction.  Almost none of those bytes
are needed: ``cv2.warpAffine(frame, M, (S, S))`` reads only the preimage of the S x S crop, and the composite
``uint8(mask_t*swap_t + (1-mask_t)*frame)`` returns the frame's own byte wherever ``mask_t == 0``, so nothing outside
the preimage of the crop square can change.  Here, per (identity, frame):

* ``face_rois`` / ``plan_rois`` — host geometry, numpy, no GPU needed: the rectangle of the frame that holds every
  source pixel the warp reads and every pixel the paste-back may write, and the plan that gives each rectangle a
  patch of one device canvas [Np,Ph,Pw,3] (intersecting rectangles of one frame share their union);
* ``upload_rois`` / ``download_rois`` — one 2-D copy per patch between the host frames and the canvas
  (``ghost_roi_copy_u8``);
* ``align_crops_roi`` / ``blend_swaps_roi`` — ``align.align_crops`` and ``blend.blend_swaps`` on the patches
  (``ghost_align_crops_roi_u8``, ``ghost_blend_swaps_roi_u8``: the same device code, the same bytes);
* ``crop_frames_and_get_transforms_roi`` — ``align.crop_frames_and_get_transforms`` from host frames.

The path is opt-in; the full-frame functions are unchanged.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from .align import (MAX_CROPS_PER_CALL, _empty, _upload, estimate_norm, frame_transforms, frames_to_match,
                    fused_resize_supported, select_keypoints)
from .blend import _fstride, _invert_affine_cv, resize_u8

_BIG = float(1 << 40)         # coordinates are clipped here before they become int64 (far outside any frame)


# ---------------------------------------------------------------------------------------------------------
# host geometry
# ---------------------------------------------------------------------------------------------------------
def _rint64(v) -> np.ndarray:
    return np.rint(np.clip(v, -_BIG, _BIG)).astype(np.int64)


def face_rois(tfms, crop_size: int, frame_hw: Tuple[int, int], margin: int = 2) -> np.ndarray:
    """Per transform M (frame -> crop, [N,2,3] float64) the rectangle (x0, y0, w, h), int32 [N,4], of an H x W frame
    that holds

    (a) every source pixel ``cv2.warpAffine(frame, M, (S, S))`` reads: OpenCV's fixed point (csrc/cv_warp.h) in int64
        with A = cv2.invertAffineTransform(M): adelta = rint(A0 x 1024), X0 = rint((A1 y + A2) 1024) + 16,
        sx = ((X0 + adelta) >> 5) >> 5, likewise sy, at x, y in {0, S-1} (each term is monotone in its axis, so the
        four corners give the exact extremes), with the taps sx..sx+1, sy..sy+1; and
    (b) every frame pixel the paste-back (csrc/blend_pixel.h) may write: the preimage under M of the open square
        (-1, S)^2, floor / ceil of its four corners mapped by A, grown by ``margin`` pixels for the kernel's float32
        evaluation of M (x, y, 1),

    clipped to the frame; (0, 0, 0, 0) when nothing of it lies in the frame.  A singular or non-finite M gets the
    whole frame."""
    t = np.asarray(tfms, np.float64)
    if t.size == 0:
        return np.zeros((0, 4), np.int32)
    if t.ndim != 3 or t.shape[1:] != (2, 3):
        raise RuntimeError(f"ghost_amd: tfms must be [N,2,3], got {t.shape}")
    S, (H, W), mg = int(crop_size), (int(frame_hw[0]), int(frame_hw[1])), int(margin)
    if S <= 0 or H <= 0 or W <= 0 or mg < 0:
        raise RuntimeError("ghost_amd: face_rois needs positive sizes and a margin >= 0")
    with np.errstate(all="ignore"):
        det = t[:, 0, 0] * t[:, 1, 1] - t[:, 0, 1] * t[:, 1, 0]
        whole = ~np.isfinite(t).all(axis=(1, 2)) | (det == 0) | ~np.isfinite(1.0 / det)
        # cv2.invertAffineTransform, the operations of blend._invert_affine_cv for all N at once
        D = np.where(whole, 0.0, 1.0 / np.where(whole, 1.0, det))
        A11, A22, A12, A21 = t[:, 1, 1] * D, t[:, 0, 0] * D, -t[:, 0, 1] * D, -t[:, 1, 0] * D
        A = np.stack([np.stack([A11, A12, -A11 * t[:, 0, 2] - A12 * t[:, 1, 2]], 1),
                      np.stack([A21, A22, -A21 * t[:, 0, 2] - A22 * t[:, 1, 2]], 1)], 1)
        A = np.where(whole[:, None, None], 0.0, A)
    c2 = np.array([0.0, S - 1.0])                 # crop corners of (a)
    c4 = np.array([-1.0, float(S)])               # and of (b)
    lo, hi = [], []
    for ax in range(2):                           # the x axis of the frame, then the y axis
        a0, a1, a2 = A[:, ax, 0, None], A[:, ax, 1, None], A[:, ax, 2, None]
        adelta = _rint64(a0 * c2 * 1024.0)                                 # [N, x]
        X0 = _rint64((a1 * c2 + a2) * 1024.0) + 16                         # [N, y]
        s = ((X0[:, :, None] + adelta[:, None, :]) >> 5) >> 5
        f = np.clip(a0[:, :, None] * c4[None, None, :] + a1[:, :, None] * c4[None, :, None] + a2[:, :, None],
                    -_BIG, _BIG)
        lo.append(np.minimum(s.min(axis=(1, 2)), np.floor(f.min(axis=(1, 2))).astype(np.int64) - mg))
        hi.append(np.maximum(s.max(axis=(1, 2)) + 1, np.ceil(f.max(axis=(1, 2))).astype(np.int64) + mg))
    x0, x1 = np.maximum(lo[0], 0), np.minimum(hi[0], W - 1)
    y0, y1 = np.maximum(lo[1], 0), np.minimum(hi[1], H - 1)
    out = np.stack([x0, y0, x1 - x0 + 1, y1 - y0 + 1], 1)
    out[(x0 > x1) | (y0 > y1)] = 0
    out[whole] = (0, 0, W, H)
    return out.astype(np.int32)


def _merge(rects: List[List[int]]) -> List[int]:
    """Merge intersecting rectangles [x0, y0, x1, y1) (in place) into their union until all are disjoint; returns the
    group of each input."""
    group = list(range(len(rects)))
    alive = list(range(len(rects)))
    merged = True
    while merged:
        merged = False
        for ai in range(len(alive)):
            for bi in range(ai + 1, len(alive)):
                a, b = rects[alive[ai]], rects[alive[bi]]
                if a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3]:
                    rects[alive[ai]] = [min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3])]
                    group = [alive[ai] if g == alive[bi] else g for g in group]
                    del alive[bi]
                    merged = True
                    break
            if merged:
                break
    return group


class RoiPlan:
    """What ``plan_rois`` returns.  ``rects`` int32 [Np,4] (x0, y0, w, h); ``frame`` int32 [Np], the frame of each
    patch; ``patch_of`` int32 [T,F], the patch of identity q in frame i (-1 where q has no face there or its
    rectangle is empty); ``canvas`` = (Ph, Pw), the largest h and w with Pw rounded up to a multiple of 4;
    ``tfms`` [T,F,2,3] float64 and ``has_face`` bool [T,F], the transforms the rectangles were made for."""

    def __init__(self, rects, frame, patch_of, canvas, tfms, has_face, crop_size, frame_hw, margin):
        self.rects, self.frame, self.patch_of, self.canvas = rects, frame, patch_of, canvas
        self.tfms, self.has_face = tfms, has_face
        self.crop_size, self.frame_hw, self.margin = crop_size, frame_hw, margin
        self._dev = {}

    @property
    def n_patches(self) -> int:
        return int(self.rects.shape[0])

    @property
    def n_frames(self) -> int:
        return int(self.patch_of.shape[1])

    def frames_of(self, q: int) -> np.ndarray:
        """The frames where identity q has a face, in order: the rows of align_crops_roi."""
        return np.nonzero(self.has_face[q])[0]

    def link_bytes(self) -> int:
        """Bytes one upload_rois (or one download_rois) moves."""
        return int((self.rects[:, 2].astype(np.int64) * self.rects[:, 3]).sum() * 3)

    def device(self, name: str, dev: torch.device) -> torch.Tensor:
        """``rects`` or ``patch_of`` on the device (uploaded once per device, on the current stream)."""
        key = (name, str(dev))
        if key not in self._dev:
            self._dev[key] = _upload(getattr(self, name), dev)
        return self._dev[key]


def plan_rois(tfm_array: Sequence[Sequence], crop_size: int, frame_hw: Tuple[int, int], margin: int = 2) -> RoiPlan:
    """The patches of a video: ``tfm_array[q][i]`` = the M [2,3] of identity q in frame i, or ``[]`` (what
    ``align.frame_transforms`` returns).  Every (identity, frame) with a non-empty ``face_rois`` rectangle gets a
    patch; rectangles of different identities in one frame that intersect are merged into their union, repeatedly
    until they are disjoint, and those identities share the patch (the reference composites identities in order into
    the same pixels; separate copies would lose that)."""
    T = len(tfm_array)
    F_ = len(tfm_array[0]) if T else 0
    if any(len(t) != F_ for t in tfm_array):
        raise RuntimeError("ghost_amd: plan_rois needs one entry per frame for every identity")
    has_face = np.array([[not _empty(m) for m in t] for t in tfm_array], bool).reshape(T, F_)
    tfms = np.zeros((T, F_, 2, 3), np.float64)
    for q, i in zip(*np.nonzero(has_face)):
        tfms[q, i] = np.asarray(tfm_array[q][i], np.float64).reshape(2, 3)
    face = face_rois(tfms[has_face], crop_size, frame_hw, margin) if has_face.any() else np.zeros((0, 4), np.int32)
    rect_of = np.zeros((T, F_, 4), np.int64)
    rect_of[has_face] = face
    patch_of = np.full((T, F_), -1, np.int32)
    rects, frame = [], []
    for i in range(F_):
        qs = [q for q in range(T) if rect_of[q, i, 2] > 0 and rect_of[q, i, 3] > 0]
        if not qs:
            continue
        boxes = [[int(r[0]), int(r[1]), int(r[0] + r[2]), int(r[1] + r[3])] for r in (rect_of[q, i] for q in qs)]
        group = _merge(boxes) if len(qs) > 1 else [0]
        first = {}
        for k, q in enumerate(qs):
            g = group[k]
            if g not in first:
                first[g] = len(rects)
                b = boxes[g]
                rects.append((b[0], b[1], b[2] - b[0], b[3] - b[1]))
                frame.append(i)
            patch_of[q, i] = first[g]
    rects = np.asarray(rects, np.int32).reshape(-1, 4)
    Ph = int(rects[:, 3].max()) if len(rects) else 0
    Pw = (int(rects[:, 2].max()) + 3) // 4 * 4 if len(rects) else 0
    return RoiPlan(rects, np.asarray(frame, np.int32), patch_of, (Ph, Pw), tfms, has_face, int(crop_size),
                   (int(frame_hw[0]), int(frame_hw[1])), int(margin))


# ---------------------------------------------------------------------------------------------------------
# host frames <-> device patches
# ---------------------------------------------------------------------------------------------------------
def _frame_pointers(frames_host, plan: RoiPlan, what: str, writable: bool) -> np.ndarray:
    """The address of each frame of ``frames_host`` (a list of C-contiguous uint8 [H,W,3] arrays, or one CPU array
    or tensor [F,H,W,3]), checked against the plan; uint64 [F]."""
    H, W = plan.frame_hw
    bad = RuntimeError(f"ghost_amd: {what} takes host frames: a list of C-contiguous uint8 [{H},{W},3] arrays or one "
                       f"CPU uint8 array / tensor [F,{H},{W},3]")
    if torch.is_tensor(frames_host):
        t = frames_host
        if t.is_cuda or t.dtype != torch.uint8 or t.ndim != 4 or tuple(t.shape[1:]) != (H, W, 3) or \
                not t.is_contiguous():
            raise bad
        ptrs = t.data_ptr() + np.arange(t.shape[0], dtype=np.uint64) * np.uint64(H * W * 3)
    elif isinstance(frames_host, np.ndarray):
        a = frames_host
        if a.dtype != np.uint8 or a.ndim != 4 or a.shape[1:] != (H, W, 3) or not a.flags.c_contiguous or \
                (writable and not a.flags.writeable):
            raise bad
        ptrs = a.ctypes.data + np.arange(a.shape[0], dtype=np.uint64) * np.uint64(H * W * 3)
    else:
        ptrs = np.zeros(len(frames_host), np.uint64)
        for i, a in enumerate(frames_host):
            if torch.is_tensor(a):
                if a.is_cuda or a.dtype != torch.uint8 or tuple(a.shape) != (H, W, 3) or not a.is_contiguous():
                    raise bad
                ptrs[i] = a.data_ptr()
            elif isinstance(a, np.ndarray):
                if a.dtype != np.uint8 or a.shape != (H, W, 3) or not a.flags.c_contiguous or \
                        (writable and not a.flags.writeable):
                    raise bad
                ptrs[i] = a.ctypes.data
            else:
                raise bad
    if len(ptrs) != plan.n_frames:
        raise RuntimeError(f"ghost_amd: {what}: the plan was made for {plan.n_frames} frames, got {len(ptrs)}")
    return ptrs


def _check_patches(patches, plan: RoiPlan, what: str) -> None:
    if not torch.is_tensor(patches):
        raise RuntimeError(f"ghost_amd: {what} takes the uint8 [Np,Ph,Pw,3] device tensor of upload_rois")
    _lib.require_gpu(patches, what)
    want = (plan.n_patches, plan.canvas[0], plan.canvas[1], 3)
    if patches.dtype != torch.uint8 or tuple(patches.shape) != want or not patches.is_contiguous():
        raise RuntimeError(f"ghost_amd: {what}: patches must be a contiguous uint8 {list(want)} device tensor "
                           "(the plan's canvas)")


def _copy(patches: torch.Tensor, plan: RoiPlan, ptrs: np.ndarray, to_device: bool, what: str) -> None:
    if not plan.n_patches:
        return
    per_patch = np.ascontiguousarray(ptrs[plan.frame])
    rects = np.ascontiguousarray(plan.rects, np.int32)
    Ph, Pw = plan.canvas
    _lib.check(_lib.load().ghost_roi_copy_u8(
        patches.data_ptr(), Ph * Pw * 3, plan.n_patches, Ph, Pw, rects.ctypes.data, per_patch.ctypes.data,
        plan.frame_hw[0], plan.frame_hw[1], 1 if to_device else 0, _lib.stream_ptr(patches.device)), what)


def upload_rois(frames_host, plan: RoiPlan, device, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Copy every rectangle of the plan from the host frames into its patch: uint8 [Np,Ph,Pw,3] on ``device``
    (``out`` to reuse one).  frames_host: a list of C-contiguous uint8 [H,W,3] arrays, or one CPU array or tensor
    [F,H,W,3]; from pinned memory the copies are asynchronous on the current stream, pageable memory works too.
    The canvas outside the rectangles is not written (and never read by align_crops_roi / blend_swaps_roi)."""
    ptrs = _frame_pointers(frames_host, plan, "upload_rois", writable=False)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"ghost_amd: upload_rois runs only on a ROCm GPU (MI355X); got device {dev}")
    if out is None:
        out = torch.empty(plan.n_patches, plan.canvas[0], plan.canvas[1], 3, dtype=torch.uint8, device=dev)
    _check_patches(out, plan, "upload_rois")
    _copy(out, plan, ptrs, True, "upload_rois")
    return out


def download_rois(patches: torch.Tensor, plan: RoiPlan, frames_host) -> None:
    """Copy every rectangle back from its patch into the host frames, in place, on the current stream (synchronise
    it before the frames are read).  A frame without a patch is never touched."""
    _check_patches(patches, plan, "download_rois")
    ptrs = _frame_pointers(frames_host, plan, "download_rois", writable=True)
    _copy(patches, plan, ptrs, False, "download_rois")


# ---------------------------------------------------------------------------------------------------------
# crops from, and swaps into, the patches
# ---------------------------------------------------------------------------------------------------------
def _identity(plan: RoiPlan, q) -> int:
    q = int(q)
    if q < 0 or q >= plan.patch_of.shape[0]:
        raise IndexError(f"ghost_amd: identity {q} out of range for a plan of {plan.patch_of.shape[0]}")
    return q


def _canvas_args(patches: torch.Tensor, plan: RoiPlan):
    Ph, Pw = plan.canvas
    return patches.data_ptr(), Ph * Pw * 3, plan.n_patches, Ph, Pw, plan.device("rects", patches.device).data_ptr()


def align_crops_roi(patches: torch.Tensor, plan: RoiPlan, q: int, tfms, crop_size: int = 224,
                    resize_to: Optional[int] = None, want_crops: bool = True):
    """``align.align_crops`` for identity q of the plan, taken from the patches: row n is the crop of frame
    ``plan.frames_of(q)[n]`` through ``tfms[n]`` ([N,2,3] float64: the transforms the plan was made for).  Same
    returns and the same handling of an unfused (S, R) as align_crops; a face whose rectangle is empty (wholly
    outside the frame) gives an all-zero crop, as cv2's constant border does."""
    _check_patches(patches, plan, "align_crops_roi")
    q = _identity(plan, q)
    dev = patches.device
    S = int(crop_size)
    R = None if resize_to is None else int(resize_to)
    if S <= 0 or (R is not None and R <= 0):
        raise RuntimeError("ghost_amd: align_crops_roi needs positive sizes")
    if not want_crops and R is None:
        raise RuntimeError("ghost_amd: align_crops_roi has nothing to return (want_crops=False and no resize_to)")
    t = np.asarray(tfms.cpu() if torch.is_tensor(tfms) else tfms, np.float64)
    N = t.shape[0] if t.ndim == 3 else 0
    if t.size and (t.ndim != 3 or t.shape[1:] != (2, 3)):
        raise RuntimeError(f"ghost_amd: tfms must be [N,2,3], got {t.shape}")
    rows = plan.frames_of(q)
    if S != plan.crop_size or N != len(rows) or (N and not np.array_equal(t, plan.tfms[q, rows])):
        raise RuntimeError("ghost_amd: align_crops_roi: crop_size / tfms are not those the plan was made for "
                           f"(identity {q}: {len(rows)} faces, crop_size {plan.crop_size})")
    index = plan.patch_of[q, rows]
    fused = R is not None and fused_resize_supported(S, R)
    need_crops = want_crops or (R is not None and not fused)
    # a face without a patch is skipped by the kernel: its crop is the zero border
    new = torch.zeros if N and (index < 0).any() else torch.empty
    crops = new(N, S, S, 3, dtype=torch.uint8, device=dev) if need_crops else None
    resized = new(N, R, R, 3, dtype=torch.uint8, device=dev) if fused else None
    if N and plan.n_patches:
        maps = _upload(np.stack([_invert_affine_cv(m) for m in t]).reshape(N, 6), dev)
        idx = _upload(index.astype(np.int32), dev)
        lib, st = _lib.load(), _lib.stream_ptr(dev)
        canvas = _canvas_args(patches, plan)
        for lo in range(0, N, MAX_CROPS_PER_CALL):
            hi = min(N, lo + MAX_CROPS_PER_CALL)
            _lib.check(lib.ghost_align_crops_roi_u8(
                *canvas, idx[lo:hi].data_ptr(), maps[lo:hi].data_ptr(), None, hi - lo, S,
                None if crops is None else crops[lo:hi].data_ptr(), S * S * 3,
                None if resized is None else resized[lo:hi].data_ptr(), 0 if resized is None else R * R * 3,
                0 if resized is None else R, st), "align_crops_roi")
    if R is not None and not fused:
        resized = crops if R == S else (resize_u8(crops, (R, R)) if N else
                                        torch.empty(0, R, R, 3, dtype=torch.uint8, device=dev))
    return (crops if want_crops else None), resized


def blend_swaps_roi(patches: torch.Tensor, plan: RoiPlan, q: int, swaps: torch.Tensor, masks: torch.Tensor, tfms,
                    valid=None, resize_to: Optional[int] = None) -> torch.Tensor:
    """``blend.blend_swaps`` for identity q of the plan, composited in place into the patches (returned): swaps u8
    [F,S,S,3], masks f32 [F,M,M], tfms [F,2,3] (an array or tensor, or the identity's ``tfm_array`` list with ``[]``
    entries) and valid [F], all indexed by frame as for blend_swaps.  Frames where q has no patch are skipped.
    Several identities: one call each, in the reference's order (identities that share a patch see each other's
    result, as they do on the full frame)."""
    _check_patches(patches, plan, "blend_swaps_roi")
    q = _identity(plan, q)
    dev = patches.device
    F_ = plan.n_frames
    if not torch.is_tensor(tfms) and not isinstance(tfms, np.ndarray):
        tfms = np.stack([np.zeros((2, 3)) if _empty(m) else np.asarray(m, np.float64).reshape(2, 3) for m in tfms]) \
            if len(tfms) else np.zeros((0, 2, 3))
    m_host = np.asarray(tfms.detach().cpu() if torch.is_tensor(tfms) else tfms)
    index = plan.patch_of[q]
    rows = index >= 0
    if m_host.shape != (F_, 2, 3) or not np.array_equal(m_host[rows].astype(np.float32),
                                                        plan.tfms[q, rows].astype(np.float32)):
        raise RuntimeError("ghost_amd: blend_swaps_roi: tfms are not those the plan was made for "
                           f"([{F_},2,3], indexed by frame)")
    used = index[rows]
    if len(np.unique(used)) != len(used):
        raise RuntimeError("ghost_amd: blend_swaps_roi: the entries of one call must reference distinct patches")
    if not torch.is_tensor(swaps) or not torch.is_tensor(masks):
        raise RuntimeError("ghost_amd: blend_swaps_roi takes swaps and masks as tensors")
    swaps = swaps.to(dev).contiguous()
    if resize_to is not None and tuple(swaps.shape[1:3]) != (resize_to, resize_to):
        swaps = resize_u8(swaps, (resize_to, resize_to))
    masks = masks.to(dev, torch.float32).contiguous()
    if swaps.dtype != torch.uint8 or swaps.ndim != 4 or swaps.shape[0] != F_ or swaps.shape[3] != 3:
        raise RuntimeError("ghost_amd: swaps must be uint8 [F,S,S,3]")
    S_h, S_w = swaps.shape[1:3]
    if tuple(masks.shape) != (F_, S_h, S_w):
        raise RuntimeError("ghost_amd: masks must be [F,S,S] matching the (resized) swaps")
    if (S_h, S_w) != (plan.crop_size, plan.crop_size):
        raise RuntimeError(f"ghost_amd: blend_swaps_roi: the plan was made for {plan.crop_size}-pixel crops")
    v = None
    if valid is not None:
        v = torch.as_tensor(np.asarray(valid) if not torch.is_tensor(valid) else valid).to(dev, torch.int32).contiguous()
        if v.numel() != F_:
            raise RuntimeError("ghost_amd: valid must have one entry per frame")
    if not F_ or not plan.n_patches or not rows.any():
        return patches
    m = torch.from_numpy(np.ascontiguousarray(m_host.astype(np.float32))).to(dev).reshape(F_, 6)
    idx = plan.device("patch_of", dev)[q]
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    canvas = _canvas_args(patches, plan)
    for lo in range(0, F_, MAX_CROPS_PER_CALL):
        hi = min(F_, lo + MAX_CROPS_PER_CALL)
        _lib.check(lib.ghost_blend_swaps_roi_u8(
            *canvas, idx[lo:hi].data_ptr(), hi - lo, swaps[lo:hi].data_ptr(), _fstride(swaps), S_h, S_w,
            masks[lo:hi].data_ptr(), _fstride(masks), m[lo:hi].data_ptr(), None if v is None else v[lo:hi].data_ptr(),
            st), "blend_swaps_roi")
    return patches


# ---------------------------------------------------------------------------------------------------------
# the alignment stage of a video, from host frames
# ---------------------------------------------------------------------------------------------------------
def _frame_hw(frames_host) -> Tuple[int, int]:
    if torch.is_tensor(frames_host) and frames_host.is_cuda:
        raise RuntimeError("ghost_amd: the ROI path takes host frames (use crop_frames_and_get_transforms for "
                           "device-resident ones)")
    try:
        first = frames_host[0]
        if torch.is_tensor(first) and first.is_cuda:
            raise RuntimeError("ghost_amd: the ROI path takes host frames (use crop_frames_and_get_transforms for "
                               "device-resident ones)")
        shape = tuple(first.shape)
    except (IndexError, AttributeError, TypeError):
        raise RuntimeError("ghost_amd: the ROI path needs at least one uint8 [H,W,3] host frame") from None
    if len(shape) != 3 or shape[2] != 3:
        raise RuntimeError(f"ghost_amd: frames must be uint8 [H,W,3], got {list(shape)}")
    return int(shape[0]), int(shape[1])


def crop_frames_and_get_transforms_roi(frames_host, kps_per_frame: Sequence, target_embeds: torch.Tensor, netArc,
                                       crop_size: int, set_target: bool, similarity_th: float, templates, device,
                                       embed_batch: int = 64, packed: bool = False):
    """``align.crop_frames_and_get_transforms`` with the frames on the host: the same bookkeeping and the same first
    four returns (crops, 256 x 256 crops, ``present``, ``tfm_array``, per identity), plus ``plan, patches`` for
    ``blend_swaps_roi`` / ``download_rois``.  The ArcFace matching of multi-face and ``set_target`` frames takes its
    crops from a temporary plan over the detector's unsmoothed transforms; the final crops come from the plan over
    the smoothed ones, whose patches are returned.  ``packed=True`` uploads through ``roi_pack.upload_rois_packed``
    (one copy per chunk of patches; the frames need not be pinned): the same returns, the same bytes."""
    if packed:
        from .roi_pack import upload_rois_packed as upload
    else:
        upload = upload_rois
    hw = _frame_hw(frames_host)
    dev = torch.device(device)
    if len(kps_per_frame) != len(frames_host):
        raise RuntimeError("ghost_amd: one keypoint entry per frame is needed")
    n_frames = len(kps_per_frame)
    T = target_embeds.shape[0]
    matches = {}
    todo = frames_to_match(kps_per_frame, set_target)
    if todo:
        from ..arcface.pipeline import match_faces
        _lib.require_same_device(target_embeds, dev, "target_embeds")
        # the k-th face of every matched frame is the k-th "identity" of a temporary plan
        K = max(len(kps_per_frame[i]) for i in todo)
        det: List[List] = [[[] for _ in range(n_frames)] for _ in range(K)]
        start, total = {}, 0
        for i in todo:
            start[i] = total
            total += len(kps_per_frame[i])
            for k, p in enumerate(kps_per_frame[i]):
                det[k][i] = estimate_norm(p, crop_size, templates)[0]
        tmp = plan_rois(det, crop_size, hw)
        tmp_patches = upload(frames_host, tmp, dev)
        faces = torch.empty(total, crop_size, crop_size, 3, dtype=torch.uint8, device=dev)
        for k in range(K):
            rows = tmp.frames_of(k)
            c, _ = align_crops_roi(tmp_patches, tmp, k, tmp.tfms[k, rows], crop_size)
            faces[torch.as_tensor([start[int(i)] + k for i in rows], dtype=torch.long, device=dev)] = c
        del tmp_patches
        embeds = torch.cat([netArc.embed_u8(faces[lo:lo + embed_batch]) for lo in range(0, total, embed_batch)])
        res = [match_faces(embeds[start[i]:start[i] + len(kps_per_frame[i])], target_embeds, similarity_th)
               for i in todo]
        best = torch.stack([r[0] for r in res]).cpu().numpy()      # one copy back for all matched frames
        ok = torch.stack([r[2] for r in res]).cpu().numpy()
        matches = {i: (best[j], ok[j]) for j, i in enumerate(todo)}
    kps_array = select_keypoints(kps_per_frame, T, set_target, matches)
    present, tfm_array = frame_transforms(kps_array, crop_size, templates)
    plan = plan_rois(tfm_array, crop_size, hw)
    patches = upload(frames_host, plan, dev)
    crop_frames, resized_frames = [], []
    for q in range(T):
        c, r = align_crops_roi(patches, plan, q, plan.tfms[q, plan.frames_of(q)], crop_size, resize_to=256)
        crop_frames.append(c)
        resized_frames.append(r)
    return crop_frames, resized_frames, present, tfm_array, plan, patches
