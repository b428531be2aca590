"""The packed ROI transfer on the GPU (ghost_roi_unpack_u8 and ghost_amd.inference.roi_pack): the canvases and host
frames of the per-patch path (upload_rois / download_rois), from one copy per chunk of patches.  Every canvas is
prefilled with 0xFF before an upload, so a byte written outside a rectangle would show."""
import numpy as np
import pytest
import torch

import roi_cases as C
import roi_pack_cases as P
from oracle import blend_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FRONTAL = np.array([[38.0, 52.0], [74.0, 51.0], [56.0, 72.0], [41.0, 92.0], [71.0, 91.0]])


def _canvas(plan):
    return torch.full((plan.n_patches, plan.canvas[0], plan.canvas[1], 3), 0xFF, dtype=torch.uint8, device=DEV)


def _packed(frames_host, plan, **kw):
    from ghost_amd.inference import upload_rois_packed
    canvas = _canvas(plan)
    out = upload_rois_packed(frames_host, plan, DEV, out=canvas, **kw)
    assert out is canvas
    return canvas


def _per_patch(frames_host, plan):
    from ghost_amd.inference import upload_rois
    return upload_rois(frames_host, plan, DEV, out=_canvas(plan))


class _Small:
    """The ``solo`` and ``shared`` plans of test_roi_gpu.py's _Small, rebuilt from roi_cases, and the hand-made plan."""

    def __init__(self):
        from ghost_amd.inference import plan_rois
        g = np.random.Generator(np.random.PCG64(2024))
        self.frames = g.integers(0, 255, size=(3, C.H, C.W, 3), dtype=np.uint8)        # no 0xFF byte in a frame
        self.tfms = C.small_tfms()
        self.solo_frames = [self.frames[f] for f in C.SMALL_FRAME]
        self.solo = plan_rois([list(self.tfms)], C.S, (C.H, C.W))
        self.who = [{2: 0, 0: 1, 1: 3}, {0: 2, 2: 4, 1: 5}, {0: 6}]
        self.shared = plan_rois(C.tfm_lists([{f: self.tfms[n] for f, n in d.items()} for d in self.who], 3), C.S,
                                (C.H, C.W))
        self.pinned = torch.from_numpy(self.frames).pin_memory()
        self.hand = P.hand_plan()
        self.hand_frames = P.frames()


@pytest.fixture(scope="module")
def small():
    return _Small()


def _check_canvas(canvas, plan, frames):
    got = canvas.cpu().numpy()
    for p, (x0, y0, w, h) in enumerate(plan.rects.tolist()):
        assert np.array_equal(got[p, :h, :w], np.asarray(frames[plan.frame[p]])[y0:y0 + h, x0:x0 + w]), p
        assert (got[p, h:] == 0xFF).all() and (got[p, :, w:] == 0xFF).all(), p          # the rest was not written


def test_upload_equals_the_per_patch_upload(small):
    assert small.solo.n_patches == 6 and small.shared.n_patches == 3
    for frames, plan in [(small.solo_frames, small.solo),           # a list of pageable arrays
                         (small.pinned, small.shared),              # one pinned tensor
                         (small.frames, small.shared)]:             # one numpy array
        got = _packed(frames, plan)
        assert torch.equal(got, _per_patch(frames, plan))           # over the whole tensor
        _check_canvas(got, plan, frames)


def test_hand_made_widths(small):
    plan = small.hand
    assert plan.canvas == (96, 128)
    got = _packed(small.hand_frames, plan)
    _check_canvas(got, plan, small.hand_frames)
    assert torch.equal(got, _per_patch(small.hand_frames, plan))
    for p in np.nonzero((plan.rects[:, 2] == 0) | (plan.rects[:, 3] == 0))[0]:
        assert (got[int(p)] == 0xFF).all()                          # an empty rectangle's patch


def _xor(canvas):
    return canvas ^ torch.tensor(0x5A, dtype=torch.uint8, device=DEV)


def _rect_mask(plan, n_frames):
    mask = np.zeros((n_frames, plan.frame_hw[0], plan.frame_hw[1]), bool)
    for (x0, y0, w, h), f in zip(plan.rects.tolist(), plan.frame):
        mask[f, y0:y0 + h, x0:x0 + w] = True
    return mask


@pytest.mark.parametrize("which", ["shared", "hand"])
def test_download_equals_the_per_patch_download(small, which):
    from ghost_amd.inference import download_rois, download_rois_packed
    plan, frames = (small.shared, small.frames) if which == "shared" else (small.hand, small.hand_frames)
    canvas = _xor(_per_patch(frames, plan))
    a, b = frames.copy(), frames.copy()
    download_rois_packed(canvas, plan, a)                           # returns with the frames written
    a = a.copy()                                                    # (as they are at this moment)
    download_rois(canvas, plan, b)
    torch.cuda.synchronize()
    assert np.array_equal(a, b)
    mask = _rect_mask(plan, len(frames))
    assert np.array_equal(a[~mask], frames[~mask]) and np.array_equal(a[mask], frames[mask] ^ 0x5A)
    # into a list of frames, and a tensor
    lst = [f.copy() for f in frames]
    download_rois_packed(canvas, plan, lst)
    t = torch.from_numpy(frames.copy())
    download_rois_packed(canvas, plan, t)
    assert np.array_equal(np.stack(lst), b) and np.array_equal(t.numpy(), b)


def test_chunking_and_threads_change_nothing(small):
    from ghost_amd.inference import download_rois_packed, packed_layout
    from ghost_amd.inference.roi_pack import _chunks
    plan, frames = small.hand, small.hand_frames
    n = plan.n_patches
    assert [c[:2] for c in _chunks(plan, 1)] == [(p, p + 1) for p in range(n)]          # one patch per chunk
    assert [c[:2] for c in _chunks(plan, 1 << 40)] == [(0, n)]                          # one chunk
    mid = int(packed_layout(plan)[0][n // 2])
    assert 1 < len(_chunks(plan, mid)) < n
    want = _per_patch(frames, plan)
    want_frames = None
    for chunk_bytes in (1, mid, 1 << 40, None):
        for threads in (1, 16):
            got = _packed(frames, plan, chunk_bytes=chunk_bytes, threads=threads)
            assert torch.equal(got, want), (chunk_bytes, threads)
            back = frames.copy()
            download_rois_packed(_xor(got), plan, back, chunk_bytes=chunk_bytes, threads=threads)
            if want_frames is None:
                want_frames = back
                assert not np.array_equal(back, frames)
            assert np.array_equal(back, want_frames), (chunk_bytes, threads)


def test_one_staging_buffer_back_to_back(small):
    from ghost_amd.inference import RoiStaging, download_rois_packed, packed_layout, upload_rois_packed
    plan = small.hand
    total = packed_layout(plan)[1]
    st = RoiStaging(total + 512, DEV)
    other = P.frames(seed=123)
    c1, c2 = _canvas(plan), _canvas(plan)
    upload_rois_packed(small.hand_frames, plan, DEV, out=c1, staging=st)       # no synchronise in between
    upload_rois_packed(other, plan, DEV, out=c2, staging=st, chunk_bytes=4096)
    _check_canvas(c1, plan, small.hand_frames)
    _check_canvas(c2, plan, other)
    # and down again through the same buffer, then up once more
    back = np.zeros_like(other)
    download_rois_packed(c1, plan, back, staging=st)
    c3 = _canvas(plan)
    upload_rois_packed(other, plan, DEV, out=c3, staging=st)
    mask = _rect_mask(plan, 3)
    assert np.array_equal(back[mask], small.hand_frames[mask]) and not back[~mask].any()
    _check_canvas(c3, plan, other)
    # refused before any copy or launch
    before = c1.clone()
    for call in (lambda: upload_rois_packed(other, plan, DEV, out=c1, staging=RoiStaging(total - 1, DEV)),
                 lambda: download_rois_packed(c1, plan, back, staging=RoiStaging(256, DEV)),
                 lambda: upload_rois_packed(torch.from_numpy(other).to(DEV), plan, DEV, out=c1),      # device frames
                 lambda: download_rois_packed(c1, plan, torch.from_numpy(other).to(DEV)),
                 lambda: upload_rois_packed(other, plan, DEV, out=c1[:2]),                            # not the canvas
                 lambda: download_rois_packed(c1[:, :, :4], plan, back),
                 lambda: upload_rois_packed(other, small.shared, DEV, out=c1),                        # another plan
                 lambda: upload_rois_packed(other.astype(np.int8), plan, DEV, out=c1)):
        with pytest.raises(RuntimeError):
            call()
    torch.cuda.synchronize()
    assert torch.equal(c1, before)


def _raw(lib, canvas, plan, rects_d, offsets_d, packed, packed_bytes, p0, p1, to_canvas, Np=None):
    from ghost_amd import _lib
    Ph, Pw = plan.canvas
    return lib.ghost_roi_unpack_u8(None if canvas is None else canvas.data_ptr(), Ph * Pw * 3,
                                   plan.n_patches if Np is None else Np, Ph, Pw,
                                   None if rects_d is None else rects_d.data_ptr(),
                                   None if offsets_d is None else offsets_d.data_ptr(),
                                   None if packed is None else packed.data_ptr(), packed_bytes, p0, p1, to_canvas,
                                   _lib.stream_ptr(torch.device(DEV)))


def test_raw_unpack_skips_clamps_and_refuses(small):
    from ghost_amd import _lib
    from ghost_amd.inference import packed_layout
    lib = _lib.load()
    plan = small.hand
    n = plan.n_patches
    offsets, total = packed_layout(plan)
    ref = P.packed_ref(plan.rects, plan.frame, offsets, total, small.hand_frames, 0xEE)
    packed = torch.from_numpy(ref).to(DEV)
    rects_d = torch.from_numpy(plan.rects.copy()).to(DEV)
    off_d = torch.from_numpy(offsets.copy()).to(DEV)
    # a range touches only its own patches
    canvas = _canvas(plan)
    assert _raw(lib, canvas, plan, rects_d, off_d, packed, total, 3, 12, 1) == 0
    got = canvas.cpu().numpy()
    assert (got[:3] == 0xFF).all() and (got[12:] == 0xFF).all()
    full = _per_patch(small.hand_frames, plan).cpu().numpy()
    assert np.array_equal(got[3:12], full[3:12])
    # patches with a bad offset stay 0xFF, their neighbours are right
    bad = offsets.copy()
    bad[2] += 8                                        # unaligned
    bad[5] = -256                                      # negative
    bad[9] = total                                     # past packed_bytes
    bad[11] = total - 256                              # its last rows would leave the buffer (21 x 5: 320 bytes)
    canvas = _canvas(plan)
    assert _raw(lib, canvas, plan, rects_d, torch.from_numpy(bad).to(DEV), packed, total, 0, n, 1) == 0
    got = canvas.cpu().numpy()
    for p in range(n):
        assert np.array_equal(got[p], np.full_like(full[p], 0xFF) if p in (2, 5, 9, 11) else full[p]), p
    # packed_bytes one short of the last patch's end: that patch alone is skipped
    end = int(offsets[n - 1]) + P.pitch(plan.rects[n - 1, 2]) * int(plan.rects[n - 1, 3])
    canvas = _canvas(plan)
    assert _raw(lib, canvas, plan, rects_d, off_d, packed, end - 1, 0, n, 1) == 0
    got = canvas.cpu().numpy()
    assert (got[n - 1] == 0xFF).all() and np.array_equal(got[:n - 1], full[:n - 1])
    # w > Pw and h > Ph are clamped to the canvas: the packed pitch stays that of the stated width
    wide = np.array([(0, 0, 200, 100)], np.int32)
    src = np.random.Generator(np.random.PCG64(4)).integers(0, 255, size=(100, 608), dtype=np.uint8)   # pitch of 200
    tiny = torch.full((2, 96, 128, 3), 0xFF, dtype=torch.uint8, device=DEV)            # patch 1 guards the end
    wide_d, zero_d, src_d = torch.from_numpy(wide).to(DEV), torch.zeros(1, dtype=torch.int64, device=DEV), \
        torch.from_numpy(src).to(DEV)
    assert lib.ghost_roi_unpack_u8(tiny.data_ptr(), 96 * 128 * 3, 1, 96, 128, wide_d.data_ptr(), zero_d.data_ptr(),
                                   src_d.data_ptr(), src.size, 0, 1, 1, _lib.stream_ptr(torch.device(DEV))) == 0
    got = tiny.cpu().numpy()
    assert np.array_equal(got[0].reshape(96, 384), src[:96, :384]) and (got[1] == 0xFF).all()
    # toward the packed buffer: rows up to their pitch, nothing past offset + pitch h, nothing of other patches
    out = torch.full((total,), 0xEE, dtype=torch.uint8, device=DEV)
    full_d = torch.from_numpy(full).to(DEV)
    assert _raw(lib, full_d, plan, rects_d, off_d, out, total, 3, 12, 0) == 0
    got = out.cpu().numpy()
    assert (got[:offsets[3]] == 0xEE).all() and (got[offsets[12]:] == 0xEE).all()
    for p in range(3, 12):
        x0, y0, w, h = plan.rects[p].tolist()
        assert w > 0 and h > 0
        lo, hi = int(offsets[p]), int(offsets[p]) + P.pitch(w) * h
        rows = got[lo:hi].reshape(h, -1)
        assert np.array_equal(rows[:, :3 * w], ref[lo:hi].reshape(rows.shape)[:, :3 * w]), p
        assert (got[hi:offsets[p + 1]] == 0xEE).all(), p                                # the gap to the next patch
    # return codes
    canvas = _canvas(plan)
    assert _raw(lib, canvas, plan, rects_d, off_d, packed, total, 4, 4, 1) == 0                      # p0 == p1
    for args in [(None, rects_d, off_d, packed), (canvas, None, off_d, packed), (canvas, rects_d, None, packed),
                 (canvas, rects_d, off_d, None)]:
        assert _raw(lib, args[0], plan, args[1], args[2], args[3], total, 0, n, 1) == -1
        assert b"null" in lib.ghost_last_error()
    assert _raw(lib, canvas, plan, rects_d, off_d, packed, total, 0, 65536, 1, Np=70000) == -1       # GHOST_EINVAL
    assert _raw(lib, canvas, plan, rects_d, off_d, packed, total, 0, n + 1, 1) == -1
    assert _raw(lib, canvas, plan, rects_d, off_d, packed, total, 0, n, 1, Np=0) == -1
    torch.cuda.synchronize()
    assert (canvas == 0xFF).all()                       # refused on the host: nothing was launched


def test_offsets_past_two_gib():
    """A packed buffer of 2^31 + 1 MiB bytes, uninitialised apart from one rectangle whose offset lies past 2^31:
    32-bit address arithmetic anywhere would miss it."""
    from ghost_amd import _lib
    lib = _lib.load()
    nbytes = (1 << 31) + (1 << 20)
    packed = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    w, h = 43, 5
    off = (1 << 31) + 4096
    g = np.random.Generator(np.random.PCG64(6))
    rows = g.integers(0, 255, size=(h, P.pitch(w)), dtype=np.uint8)
    packed[off:off + rows.size] = torch.from_numpy(rows.reshape(-1)).to(DEV)
    rects = torch.tensor([[0, 0, 0, 0], [3, 4, w, h]], dtype=torch.int32, device=DEV)
    offs = torch.tensor([0, off], dtype=torch.int64, device=DEV)
    canvas = torch.full((2, 8, 44, 3), 0xFF, dtype=torch.uint8, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))

    def run(to_canvas):
        return lib.ghost_roi_unpack_u8(canvas.data_ptr(), 8 * 44 * 3, 2, 8, 44, rects.data_ptr(), offs.data_ptr(),
                                       packed.data_ptr(), nbytes, 0, 2, to_canvas, st)

    assert run(1) == 0
    got = canvas.cpu().numpy()
    assert np.array_equal(got[1, :h, :w].reshape(h, 3 * w), rows[:, :3 * w])
    assert (got[0] == 0xFF).all() and (got[1, h:] == 0xFF).all() and (got[1, :, w:] == 0xFF).all()
    canvas[1, :h, :w] ^= 0x5A
    guard = slice(off - 256, off + rows.size + 256)
    packed[guard] = 0xEE
    assert run(0) == 0
    back = packed[guard].cpu().numpy()
    assert (back[:256] == 0xEE).all() and (back[-256:] == 0xEE).all()
    assert np.array_equal(back[256:-256].reshape(h, -1)[:, :3 * w], rows[:, :3 * w] ^ 0x5A)


class _PixelArc:
    """Stands in for netArc: a crop's embedding is an 8 x 8 grid of its pixels (test_roi_gpu.py)."""

    def embed_u8(self, crops):
        return crops[:, 14::28, 14::28, :].reshape(crops.shape[0], -1).float() - 127.5


def test_the_chain_with_packed_transfers_matches_the_per_patch_chain():
    from ghost_amd.inference import (align, blend_swaps_roi, crop_frames_and_get_transforms_roi, download_rois,
                                     download_rois_packed)
    g = np.random.Generator(np.random.PCG64(91))
    tex = g.integers(0, 256, size=(2, 48, 48, 3), dtype=np.uint8)          # the two "faces"
    templates = FRONTAL[None] * 2.0
    layout = [[(0, (5, 10)), (1, (70, 30))], [(1, (72, 31)), (0, (6, 10))], [(0, (7, 11))], [(1, (71, 33))], None,
              [(1, (40, 33)), (0, (8, 12))]]
    n = len(layout)
    frames = g.integers(0, 40, size=(n, C.H, C.W, 3), dtype=np.uint8)
    kps = []
    for i, faces in enumerate(layout):
        if faces is None:
            kps.append(None)
            continue
        for who, (x, y) in faces:
            frames[i, y:y + 48, x:x + 48] = tex[who]
        kps.append(np.stack([FRONTAL * 0.4 + np.array([x + 1.0, y + 1.0]) for _, (x, y) in faces]))
    arc = _PixelArc()
    first = R.warp_affine_cv(frames[0], align.estimate_norm(kps[0][0], 224, templates)[0], (224, 224), "constant")
    target = arc.embed_u8(torch.from_numpy(first[None])).to(DEV)
    hosts, outs = {}, {}
    for packed in (False, True):
        host = [f.copy() for f in frames]                                   # pageable
        crops, rz, present, tfm, plan, patches = crop_frames_and_get_transforms_roi(
            host, kps, target, arc, 224, True, 0.5, templates, DEV, embed_batch=4, packed=packed)
        outs[packed] = (crops, rz, patches.clone(), plan)
        idx = torch.from_numpy(np.maximum(np.cumsum(present[0]) - 1, 0).astype(np.int64)).to(DEV)
        swaps = rz[0].index_select(0, idx)
        masks = torch.ones(n, 224, 224, device=DEV) * 0.75
        valid = torch.from_numpy(present[0].astype(np.int32))
        blend_swaps_roi(patches, plan, 0, swaps, masks, tfm[0], valid=valid, resize_to=224)
        if packed:
            download_rois_packed(patches, plan, host)
        else:
            download_rois(patches, plan, host)
            torch.cuda.synchronize()
        hosts[packed] = np.stack(host)
    a, b = outs[False], outs[True]
    assert a[3].patch_of[0].tolist() == b[3].patch_of[0].tolist() == [0, 1, 2, -1, -1, 3]
    assert np.array_equal(a[3].rects, b[3].rects)
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[1][0], b[1][0]) and a[0][0].shape[0] == 4
    mask = torch.from_numpy(np.zeros(a[2].shape[:3], bool))
    for p, (_, _, w, h) in enumerate(a[3].rects.tolist()):
        mask[p, :h, :w] = True
    mask = mask.to(DEV)
    assert torch.equal(a[2][mask], b[2][mask])                              # the patches, inside the rectangles
    assert np.array_equal(hosts[False], hosts[True])
    assert not np.array_equal(hosts[True][0], frames[0]) and np.array_equal(hosts[True][3:5], frames[3:5])
