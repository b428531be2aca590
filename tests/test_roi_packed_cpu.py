"""The packed ROI transfer without a GPU (ghost_roi_packed_layout, ghost_roi_pack_host and the argument checks of
ghost_amd.inference.roi_pack): the layout rule, the host packer's bytes in both directions, its independence of the
thread count and of how the patches are split into ranges, every refusal, and the same host code under the
sanitizers as a stand-alone program (tools/asan_roi_pack.sh)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import roi_cases
import roi_pack_cases as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FILL = 0xEE


@pytest.fixture(scope="module")
def lib():
    from ghost_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "ghost_roi_pack_host")
    return lib


def _layout(lib, rects):
    rects = np.ascontiguousarray(rects, np.int32).reshape(-1, 4)
    offsets = np.full(len(rects), -7, np.int64)
    total = C.c_int64(-7)
    rc = lib.ghost_roi_packed_layout(rects.ctypes.data if len(rects) else None, len(rects),
                                     offsets.ctypes.data if len(rects) else None, C.byref(total))
    return rc, offsets, int(total.value)


class _Hand:
    """The hand-made rectangles, their frames, the library's layout and the expected packed buffer."""

    def __init__(self, lib):
        self.rects, self.frame_of = P.hand_rects()
        self.n = len(self.rects)
        self.src = P.frames()
        rc, self.offsets, self.total = _layout(lib, self.rects)
        assert rc == 0
        self.packed = P.packed_ref(self.rects, self.frame_of, self.offsets, self.total, self.src, FILL)

    def ptrs(self, frames):
        return np.array([frames[f].ctypes.data for f in self.frame_of], np.uint64)


@pytest.fixture(scope="module")
def hand(lib):
    return _Hand(lib)


def _pack(lib, staging, rects, offsets, ptrs, p0, p1, to_staging, threads=0, nbytes=None, Np=None, hw=(P.H, P.W)):
    rects = np.ascontiguousarray(rects, np.int32)
    offsets = np.ascontiguousarray(offsets, np.int64)
    ptrs = np.ascontiguousarray(ptrs, np.uint64)
    return lib.ghost_roi_pack_host(staging.ctypes.data, len(staging) if nbytes is None else nbytes, rects.ctypes.data,
                                   offsets.ctypes.data, ptrs.ctypes.data, len(rects) if Np is None else Np, p0, p1,
                                   hw[0], hw[1], to_staging, threads)


def test_hand_made_rectangles_cover_the_table(hand):
    r = hand.rects
    full = r[(r[:, 2] > 0) & (r[:, 3] > 0)]
    assert set(full[:, 2].tolist()) == P.WIDTHS and set(full[:, 3].tolist()) == P.HEIGHTS
    assert {0, 1} == set((full[:, 0] % 2).tolist())
    assert (full[:, 0] + full[:, 2] == P.W).any() and (full[:, 1] + full[:, 3] == P.H).any()
    assert ((r[:, 2] == 0) | (r[:, 3] == 0))[1:-1].sum() == 2               # the empty ones, in the middle
    for f in range(3):                                                      # disjoint within a frame
        seen = np.zeros((P.H, P.W), np.int32)
        for x0, y0, w, h in r[hand.frame_of == f].tolist():
            seen[y0:y0 + h, x0:x0 + w] += 1
        assert seen.max() == 1


def test_layout_is_the_stated_rule(lib, hand):
    want, total = P.layout_ref(hand.rects)
    assert np.array_equal(hand.offsets, want) and hand.total == total
    assert (hand.offsets % 256 == 0).all() and hand.total % 256 == 0
    ends = hand.offsets + np.array([P.pitch(w) * h if w > 0 and h > 0 else 0 for _, _, w, h in hand.rects.tolist()])
    assert (ends[:-1] <= hand.offsets[1:]).all() and ends[-1] <= hand.total          # ascending and disjoint
    k = 13
    assert hand.rects[k, 2] == 0 and hand.offsets[k] == hand.offsets[k + 1]           # an empty one takes no bytes
    # a second set: random sizes, pitch a multiple of 16 that holds 3 w bytes
    g = np.random.Generator(np.random.PCG64(3))
    rects = np.stack([g.integers(0, 50, 40), g.integers(0, 50, 40), g.integers(0, 700, 40), g.integers(0, 9, 40)], 1)
    rc, offsets, total = _layout(lib, rects)
    want, want_total = P.layout_ref(rects)
    assert rc == 0 and np.array_equal(offsets, want) and total == want_total


def test_layout_refuses_negative_sizes_and_accepts_none(lib):
    for bad in [(0, 0, -1, 4), (0, 0, 4, -1)]:
        rc, offsets, total = _layout(lib, [(0, 0, 4, 4), bad])
        assert rc == EINVAL and b"negative" in lib.ghost_last_error()
        assert (offsets == -7).all() and total == -7                        # nothing written
    rc, _, total = _layout(lib, np.zeros((0, 4), np.int32))
    assert rc == 0 and total == 0
    assert lib.ghost_roi_packed_layout(None, 2, None, None) == EINVAL


def test_pack_writes_the_rows_and_nothing_else(lib, hand):
    staging = np.full(hand.total, FILL, np.uint8)
    src = hand.src.copy()
    assert _pack(lib, staging, hand.rects, hand.offsets, hand.ptrs(src), 0, hand.n, 1) == 0
    assert np.array_equal(staging, hand.packed)          # rows = the numpy slices; padding and gaps still 0xEE
    assert (hand.packed == FILL).sum() > 1000 and np.array_equal(src, hand.src)
    for p in (0, 5, hand.n - 1):                         # spelled out for three of them
        x0, y0, w, h = hand.rects[p].tolist()
        rows = staging[hand.offsets[p]:hand.offsets[p] + P.pitch(w) * h].reshape(h, P.pitch(w))
        assert np.array_equal(rows[:, :3 * w].reshape(h, w, 3), hand.src[hand.frame_of[p]][y0:y0 + h, x0:x0 + w])
        assert (rows[:, 3 * w:] == FILL).all()


def test_unpack_replaces_the_rectangles_and_nothing_else(lib, hand):
    other = P.frames(seed=5)
    dst = other.copy()
    staging = hand.packed.copy()
    assert _pack(lib, staging, hand.rects, hand.offsets, hand.ptrs(dst), 0, hand.n, 0) == 0
    want = other.copy()
    for (x0, y0, w, h), f in zip(hand.rects.tolist(), hand.frame_of):
        want[f, y0:y0 + h, x0:x0 + w] = hand.src[f, y0:y0 + h, x0:x0 + w]
    assert np.array_equal(dst, want) and not np.array_equal(dst, other)
    assert np.array_equal(dst[0], hand.src[0]) and np.array_equal(staging, hand.packed)


def test_threads_and_ranges_give_the_same_bytes(lib, hand):
    # large enough that the workers really split it: 12 faces of about 300 x 300, each in its own 320 x 400 frame
    g = np.random.Generator(np.random.PCG64(8))
    big = g.integers(0, FILL, size=(12, 320, 400, 3), dtype=np.uint8)
    rects = np.array([(g.integers(0, 100), g.integers(0, 20), 300 - k, 300 - 2 * k) for k in range(12)], np.int32)
    frame_of = np.arange(12)
    rc, offsets, total = _layout(lib, rects)
    want = P.packed_ref(rects, frame_of, offsets, total, big, FILL)
    ptrs = np.array([big[f].ctypes.data for f in frame_of], np.uint64)
    for threads in (1, 3, 16, 0, 99):
        staging = np.full(total, FILL, np.uint8)
        assert _pack(lib, staging, rects, offsets, ptrs, 0, 12, 1, threads, hw=(320, 400)) == 0
        assert np.array_equal(staging, want), threads
        back = np.zeros_like(big)
        bptrs = np.array([back[f].ctypes.data for f in frame_of], np.uint64)
        assert _pack(lib, staging, rects, offsets, bptrs, 0, 12, 0, threads, hw=(320, 400)) == 0
        mask = np.zeros(big.shape[:3], bool)
        for (x0, y0, w, h), f in zip(rects.tolist(), frame_of):
            mask[f, y0:y0 + h, x0:x0 + w] = True
        assert np.array_equal(back[mask], big[mask]) and not back[~mask].any(), threads
    # the hand-made set: every split point, and every single patch
    src = hand.src.copy()
    for threads in (1, 3, 16):
        for cut in range(hand.n + 1):
            staging = np.full(hand.total, FILL, np.uint8)
            assert _pack(lib, staging, hand.rects, hand.offsets, hand.ptrs(src), 0, cut, 1, threads) == 0
            if cut < hand.n:
                assert (staging[hand.offsets[cut]:] == FILL).all()           # only its own range
            assert _pack(lib, staging, hand.rects, hand.offsets, hand.ptrs(src), cut, hand.n, 1, threads) == 0
            assert np.array_equal(staging, hand.packed), (threads, cut)
    staging = np.full(hand.total, FILL, np.uint8)
    for p in range(hand.n):
        assert _pack(lib, staging, hand.rects, hand.offsets, hand.ptrs(src), p, p + 1, 1) == 0
    assert np.array_equal(staging, hand.packed)
    assert _pack(lib, staging, hand.rects, hand.offsets, hand.ptrs(src), 4, 4, 1) == 0          # p0 == p1


def test_refusals_leave_staging_and_frames_untouched(lib, hand):
    n = hand.n
    last = n - 1                                         # the last one: every copy before it would have run
    cases = []
    for bad in [(100, 0, 40, 40), (0, 90, 10, 10), (-1, 0, 10, 10), (0, 0, 10, -3), (0, -2, 4, 4)]:
        rects = hand.rects.copy()
        rects[last] = bad
        cases.append(("leaves the frame", dict(rects=rects)))
    for k, delta in [(last, 8), (3, 1), (last, -hand.total - 256)]:        # unaligned, unaligned, negative
        offsets = hand.offsets.copy()
        offsets[k] += delta
        cases.append(("offset", dict(offsets=offsets)))
    offsets = hand.offsets.copy()
    offsets[8] = offsets[7] + 16                         # patch 7 (1 x 96, 1 536 bytes) runs into patch 8
    cases.append(("overlap or descend", dict(offsets=offsets)))
    offsets = hand.offsets.copy()
    offsets[[2, 3]] = offsets[[3, 2]]                    # descending
    cases.append(("overlap or descend", dict(offsets=offsets)))
    end = int(hand.offsets[last]) + P.pitch(hand.rects[last, 2]) * int(hand.rects[last, 3])
    cases.append(("staging buffer", dict(nbytes=end - 1)))                 # one byte short
    ptrs = hand.ptrs(hand.src).copy()
    ptrs[last] = 0
    cases.append(("null", dict(ptrs=ptrs)))
    for to_staging in (1, 0):
        for msg, kw in cases:
            frames = hand.src.copy()
            staging = hand.packed.copy() if not to_staging else np.full(hand.total, FILL, np.uint8)
            before = staging.copy()
            ptrs = kw.get("ptrs")
            if ptrs is None:
                ptrs = hand.ptrs(frames)
            else:
                ptrs = np.where(ptrs == 0, 0, hand.ptrs(frames)).astype(np.uint64)
            rc = _pack(lib, staging, kw.get("rects", hand.rects), kw.get("offsets", hand.offsets), ptrs, 0, n,
                       to_staging, 3, nbytes=kw.get("nbytes"))
            assert rc == EINVAL and msg.encode() in lib.ghost_last_error(), (msg, lib.ghost_last_error())
            assert np.array_equal(staging, before) and np.array_equal(frames, hand.src), msg
    # the buffer of exactly the needed size is accepted
    staging = np.full(hand.total, FILL, np.uint8)
    assert _pack(lib, staging, hand.rects, hand.offsets, hand.ptrs(hand.src.copy()), 0, n, 1, nbytes=end) == 0
    # bad ranges and null arguments
    for p0, p1 in [(-1, 2), (3, 2), (0, n + 1)]:
        assert _pack(lib, staging, hand.rects, hand.offsets, hand.ptrs(hand.src), p0, p1, 1) == EINVAL
    assert lib.ghost_roi_pack_host(None, 0, None, None, None, n, 0, n, P.H, P.W, 1, 0) == EINVAL
    assert b"null" in lib.ghost_last_error()


def test_packed_layout_is_cached_on_the_plan(hand):
    from ghost_amd.inference import packed_layout
    plan = P.hand_plan()
    offsets, total = packed_layout(plan)
    assert offsets.dtype == np.int64 and np.array_equal(offsets, hand.offsets) and total == hand.total
    again = packed_layout(plan)
    assert again[0] is offsets and again[1] == total
    with pytest.raises(ValueError):
        offsets[0] = 1                                   # shared: read-only
    from ghost_amd.inference import plan_rois
    empty = plan_rois([[[], []]], roi_cases.S, (roi_cases.H, roi_cases.W))
    assert packed_layout(empty)[1] == 0 and packed_layout(empty)[0].shape == (0,)


def test_python_refuses_before_anything_runs():
    from ghost_amd.inference import (RoiStaging, crop_frames_and_get_transforms_roi, download_rois_packed, plan_rois,
                                     upload_rois_packed)
    Cc = roi_cases
    M = Cc.tfm(2.0, 0.0, 25.0, 25.0)
    plan = plan_rois(Cc.tfm_lists([{0: M, 1: M}], 2), Cc.S, (Cc.H, Cc.W))
    frames = np.zeros((2, Cc.H, Cc.W, 3), np.uint8)
    for bad in (frames.astype(np.float32),                     # dtype
                frames[:, :, ::-1],                            # layout
                frames[:1],                                    # not the plan's frame count
                [frames[0], np.zeros((Cc.H + 2, Cc.W, 3), np.uint8)],      # frames of differing size
                [frames[0], frames[1, :, :, ::-1]],
                torch.zeros(2, Cc.H, Cc.W, 3),                 # a float tensor
                np.zeros((2, Cc.H, Cc.W, 4), np.uint8)):
        with pytest.raises(RuntimeError):
            upload_rois_packed(bad, plan, "cuda:0")
    with pytest.raises(RuntimeError):
        upload_rois_packed(frames, plan, "cpu")
    for kw in (dict(chunk_bytes=0), dict(threads=-1), dict(staging=object())):
        with pytest.raises(RuntimeError):
            upload_rois_packed(frames, plan, "cuda:0", **kw)
    patches = torch.zeros(plan.n_patches, plan.canvas[0], plan.canvas[1], 3, dtype=torch.uint8)   # on the host
    with pytest.raises(RuntimeError):
        download_rois_packed(patches, plan, frames)
    with pytest.raises(RuntimeError):
        upload_rois_packed(frames, plan, "cuda:0", out=patches)
    with pytest.raises(RuntimeError):
        RoiStaging(1024, "cpu")
    with pytest.raises(RuntimeError):                          # one keypoint entry per frame
        crop_frames_and_get_transforms_roi(frames, [None], torch.zeros(1, 512), None, Cc.S, False, 0.15, None,
                                           "cuda:0", packed=True)
    assert not frames.any()


def test_host_packer_under_the_sanitizers():
    """tests/asan/roi_pack_main.cpp linked with roi_pack.hip alone, built twice by tools/asan_roi_pack.sh (address +
    undefined, then thread) and run on the CPU: layout, pack, unpack, threads 1 / 4 / 16 and every refusal."""
    r = subprocess.run(["bash", os.path.join(REPO, "tools", "asan_roi_pack.sh")], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.count("0 failed checks") == 2 and r.stdout.count("failed checks") == 2, r.stdout[-2000:]
    for report in ("ERROR: AddressSanitizer", "WARNING: ThreadSanitizer", "runtime error:", "LeakSanitizer"):
        assert report not in r.stderr and report not in r.stdout, r.stderr[-4000:]
