"""The ROI video path on the GPU (ghost_roi_copy_u8, ghost_align_crops_roi_u8, ghost_blend_swaps_roi_u8 and
ghost_amd.inference.roi): the bytes of the full-frame path, from patches that hold only each face's rectangle.
Every canvas is prefilled with 0xFF before the upload, so a kernel that read it outside a rectangle would show."""
import numpy as np
import pytest
import torch

import roi_cases as C
from oracle import blend_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FRONTAL = np.array([[38.0, 52.0], [74.0, 51.0], [56.0, 72.0], [41.0, 92.0], [71.0, 91.0]])


def _upload_prefilled(frames_host, plan):
    from ghost_amd.inference import upload_rois
    canvas = torch.full((plan.n_patches, plan.canvas[0], plan.canvas[1], 3), 0xFF, dtype=torch.uint8, device=DEV)
    out = upload_rois(frames_host, plan, DEV, out=canvas)
    assert out is canvas
    return canvas


class _Small:
    """3 frames of 96 x 128, S = 56 (2 x 2 tiles), the seven transforms of test_align_gpu's _Small, laid out twice:
    ``solo``: one identity over seven "frames" (a list of arrays, one face each: every face has its own patch);
    ``shared``: three identities over the three frames (the faces of a frame intersect: merged patches)."""
    S, Rz = C.S, 64

    def __init__(self):
        from ghost_amd.inference import plan_rois
        g = np.random.Generator(np.random.PCG64(2024))
        self.frames = g.integers(0, 255, size=(3, C.H, C.W, 3), dtype=np.uint8)        # no 0xFF byte in a frame
        self.tfms = C.small_tfms()
        self.crops = np.stack([R.warp_affine_cv(self.frames[f], M, (self.S, self.S), "constant")
                               for f, M in zip(C.SMALL_FRAME, self.tfms)])
        self.rz = np.stack([R.resize_linear_u8(c, (self.Rz, self.Rz)) for c in self.crops])
        self.rz48 = np.stack([R.resize_linear_u8(c, (48, 48)) for c in self.crops])
        self.dev_frames = torch.from_numpy(self.frames).to(DEV)
        self.solo_frames = [self.frames[f] for f in C.SMALL_FRAME]
        self.solo = plan_rois([list(self.tfms)], self.S, (C.H, C.W))
        # identity -> {frame: face}
        self.who = [{2: 0, 0: 1, 1: 3}, {0: 2, 2: 4, 1: 5}, {0: 6}]
        self.shared = plan_rois(C.tfm_lists([{f: self.tfms[n] for f, n in d.items()} for d in self.who], 3), self.S,
                                (C.H, C.W))
        self.pinned = torch.from_numpy(self.frames).pin_memory()


@pytest.fixture(scope="module")
def small():
    return _Small()


def _check_canvas(canvas, plan, frames):
    got = canvas.cpu().numpy()
    for p, (x0, y0, w, h) in enumerate(plan.rects):
        assert np.array_equal(got[p, :h, :w], np.asarray(frames[plan.frame[p]])[y0:y0 + h, x0:x0 + w]), p
        assert (got[p, h:] == 0xFF).all() and (got[p, :, w:] == 0xFF).all(), p          # the rest was not written


def test_upload_copies_exactly_the_rectangles(small):
    assert small.solo.n_patches == 6 and small.solo.patch_of[0].tolist() == [0, 1, 2, 3, 4, 5, -1]
    assert small.shared.n_patches == 3 and small.shared.frame.tolist() == [0, 1, 2]    # every frame's faces merged
    assert small.shared.patch_of[2, 0] == -1                                           # but not the one off the frame
    _check_canvas(_upload_prefilled(small.solo_frames, small.solo), small.solo, small.solo_frames)       # pageable
    _check_canvas(_upload_prefilled(small.pinned, small.shared), small.shared, small.frames)            # pinned
    _check_canvas(_upload_prefilled(small.frames, small.shared), small.shared, small.frames)            # one array


@pytest.mark.parametrize("layout", ["solo", "shared"])
def test_align_crops_roi_is_byte_exact(small, layout):
    from ghost_amd.inference import align_crops, align_crops_roi
    if layout == "solo":
        plan, patches, faces = small.solo, _upload_prefilled(small.solo_frames, small.solo), [list(range(7))]
    else:
        plan, patches = small.shared, _upload_prefilled(small.pinned, small.shared)
        faces = [[d[f] for f in sorted(d)] for d in small.who]
    for q, rows in enumerate(faces):
        tf = small.tfms[rows]
        assert plan.frames_of(q).tolist() == (list(range(7)) if layout == "solo" else sorted(small.who[q]))
        full_c, full_r = align_crops(small.dev_frames, tf, [C.SMALL_FRAME[n] for n in rows], small.S,
                                     resize_to=small.Rz)
        crops, rz = align_crops_roi(patches, plan, q, tf, small.S, resize_to=small.Rz)              # fused, R = 64
        assert crops.shape == (len(rows), 56, 56, 3) and rz.shape == (len(rows), 64, 64, 3)
        assert np.array_equal(crops.cpu().numpy(), small.crops[rows]) and torch.equal(crops, full_c)
        assert np.array_equal(rz.cpu().numpy(), small.rz[rows]) and torch.equal(rz, full_r)
        crops, rz = align_crops_roi(patches, plan, q, tf, small.S)                                   # crops only
        assert rz is None and np.array_equal(crops.cpu().numpy(), small.crops[rows])
        crops, rz = align_crops_roi(patches, plan, q, tf, small.S, resize_to=small.Rz, want_crops=False)
        assert crops is None and np.array_equal(rz.cpu().numpy(), small.rz[rows])                    # resized only
        crops, rz = align_crops_roi(patches, plan, q, tf, small.S, resize_to=48, want_crops=False)   # unfused, R = 48
        assert crops is None and np.array_equal(rz.cpu().numpy(), small.rz48[rows])
        if 6 in rows:                                       # the face wholly outside the frame: the zero border
            crops, rz = align_crops_roi(patches, plan, q, tf, small.S, resize_to=small.Rz)
            assert not crops[rows.index(6)].any() and not rz[rows.index(6)].any() and not small.crops[6].any()


def _raw_align(lib, patches, plan, index, maps, valid, N, S, crops, cstride, rz, rstride, Rz, Np=None):
    from ghost_amd import _lib
    Ph, Pw = plan.canvas
    return lib.ghost_align_crops_roi_u8(
        patches.data_ptr(), Ph * Pw * 3, plan.n_patches if Np is None else Np, Ph, Pw,
        plan.device("rects", patches.device).data_ptr(), index.data_ptr(), maps.data_ptr(),
        None if valid is None else valid.data_ptr(), N, S, None if crops is None else crops.data_ptr(), cstride,
        None if rz is None else rz.data_ptr(), rstride, Rz, _lib.stream_ptr(patches.device))


def _solo_device_args(small):
    from ghost_amd.inference.blend import _invert_affine_cv
    maps = torch.from_numpy(np.stack([_invert_affine_cv(m) for m in small.tfms]).reshape(-1, 6)).to(DEV)
    return maps, torch.from_numpy(small.solo.patch_of[0].copy()).to(DEV)


@pytest.mark.parametrize("pad", [40, 13])      # dword-aligned rows (packed stores) and odd ones (byte stores)
def test_valid_rows_bad_indices_and_strided_outputs(small, pad):
    from ghost_amd import _lib
    lib = _lib.load()
    patches = _upload_prefilled(small.solo_frames, small.solo)
    maps, index = _solo_device_args(small)
    index[3] = small.solo.n_patches                                   # out of range: skipped like index 6's -1
    S, Rz, N = small.S, small.Rz, 7
    valid = torch.tensor([1, 0, 1, 1, 0, 1, 1], dtype=torch.int32, device=DEV)
    cs, rs = S * S * 3 + pad, Rz * Rz * 3 + pad
    cbuf = torch.full((N, cs), 0xA5, dtype=torch.uint8, device=DEV)
    rbuf = torch.full((N, rs), 0x5A, dtype=torch.uint8, device=DEV)
    assert _raw_align(lib, patches, small.solo, index, maps, valid, N, S, cbuf, cs, rbuf, rs, Rz) == 0
    c, r = cbuf.cpu().numpy(), rbuf.cpu().numpy()
    assert (c[:, S * S * 3:] == 0xA5).all() and (r[:, Rz * Rz * 3:] == 0x5A).all()      # the gaps of the view
    for n in range(N):
        if n in (0, 2, 5):
            assert np.array_equal(c[n, :S * S * 3].reshape(S, S, 3), small.crops[n]), n
            assert np.array_equal(r[n, :Rz * Rz * 3].reshape(Rz, Rz, 3), small.rz[n]), n
        else:
            assert (c[n] == 0xA5).all() and (r[n] == 0x5A).all(), n


def _mask(S):
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    r = np.sqrt((yy - S / 2) ** 2 + (xx - S / 2) ** 2) / (S / 2)
    return np.clip(1.3 - r, 0.0, 1.0).astype(np.float32)


def _both_paths(frames, lists, swaps, masks, valid=None, resize_to=None, S=C.S):
    """Composite every identity, in order, on the full frames and through the patches; returns (full, roi, plan)."""
    from ghost_amd.inference import blend_swaps_roi, download_rois, plan_rois
    from ghost_amd.inference.blend import blend_swaps
    F_, H, W = frames.shape[:3]
    plan = plan_rois(lists, S, (H, W))
    full = torch.from_numpy(frames).to(DEV)
    host = frames.copy()
    patches = _upload_prefilled(host, plan)
    for q, tf in enumerate(lists):
        mats = np.stack([np.zeros((2, 3)) if len(m) == 0 else m for m in tf])
        present = torch.tensor([len(m) > 0 for m in tf], dtype=torch.int32)
        v = present if valid is None else present * torch.as_tensor(valid[q], dtype=torch.int32)
        blend_swaps(full, swaps[q], masks[q], mats, v, resize_to=resize_to)
        out = blend_swaps_roi(patches, plan, q, swaps[q], masks[q], tf if q % 2 else mats,
                              valid=None if valid is None else valid[q], resize_to=resize_to)
        assert out is patches
    download_rois(patches, plan, host)
    torch.cuda.synchronize()
    return full.cpu().numpy(), host, plan


def test_blend_and_download_match_the_full_frame_path():
    g = np.random.Generator(np.random.PCG64(11))
    frames = g.integers(0, 256, size=(4, C.H, C.W, 3), dtype=np.uint8)
    a, b, near = C.tfm(2.0, 0.0, 25.0, 25.0), C.tfm(2.0, 0.1, 100.0, 70.0), C.tfm(2.0, 0.0, 40.0, 30.0)
    # frame 0: disjoint rectangles; 1: intersecting ones (a shared patch, order-dependent pixels); 2: faceless;
    # 3: identity 0 rotated and half off the frame, identity 1 masked off by valid
    lists = C.tfm_lists([{0: a, 1: a, 3: C.tfm(1.0, 0.4, 118.0, 10.0)}, {0: b, 1: near, 3: b}], 4)
    swaps = [torch.from_numpy(g.integers(0, 256, size=(4, C.S, C.S, 3), dtype=np.uint8)) for _ in range(2)]
    masks = [torch.from_numpy(np.stack([_mask(C.S)] * 4) * s) for s in (1.0, 0.8)]
    valid = [np.array([1, 1, 1, 1]), np.array([1, 1, 1, 0])]
    full, roi, plan = _both_paths(frames, lists, swaps, masks, valid)
    assert plan.patch_of[0, 0] != plan.patch_of[1, 0] and plan.patch_of[0, 1] == plan.patch_of[1, 1] >= 0
    assert np.array_equal(roi, full)
    assert not np.array_equal(full[:2], frames[:2]) and not np.array_equal(full[3], frames[3])       # faces pasted
    assert 2 not in plan.frame.tolist() and np.array_equal(roi[2], frames[2])                        # never copied
    # where both identities of frame 1 paste, the second went on top of the first's result
    only0, _, _ = _both_paths(frames, [lists[0], [[]] * 4], swaps, masks, valid)
    only1, _, _ = _both_paths(frames, [[[]] * 4, lists[1]], swaps, masks, valid)
    both = (only0[1] != frames[1]).any(axis=2) & (only1[1] != frames[1]).any(axis=2)
    assert both.sum() > 100 and not np.array_equal(full[1][both], only1[1][both])
    # valid switched identity 1 off in frame 3
    assert np.array_equal(full[3], only0[3])


def test_blend_roi_workload_shape_and_the_reference_gate():
    """270 x 480 frames, S = 224, 256 x 256 swaps resized first (resize_to=224): the bytes of blend_swaps, and within
    the gate of tests/test_blend.py (<= 1 LSB on < 0.5 % of the pixels) of paste_back_video."""
    from ghost_amd.inference import align_crops_roi, upload_rois
    cases = [R.make_case(s) for s in (20, 21)]
    frames = np.stack([c[0] for c in cases])
    mats = [c[3] for c in cases]                                    # float32, as blend_swaps takes them
    lists = [[m.astype(np.float64) for m in mats]]
    g = np.random.default_rng(9)
    swaps256 = g.integers(0, 256, (2, 256, 256, 3), dtype=np.uint8)
    masks = np.stack([c[2] for c in cases])
    full, roi, plan = _both_paths(frames, lists, [torch.from_numpy(swaps256)], [torch.from_numpy(masks)],
                                  resize_to=224, S=224)
    assert np.array_equal(roi, full)
    assert plan.link_bytes() < frames.nbytes
    for f in range(2):
        ref = R.paste_back_video(frames[f], swaps256[f], masks[f], mats[f])
        d = np.abs(roi[f].astype(np.int16) - ref.astype(np.int16))
        assert not np.array_equal(ref, frames[f])
        assert d.max() <= 1 and (d > 0).mean() < 5e-3, (f, d.max(), (d > 0).mean())
    # and the 224 crop with its 256 resize from the same patches
    tf = np.stack(lists[0])
    crops, rz = align_crops_roi(upload_rois(frames, plan, DEV), plan, 0, tf, 224, resize_to=256)
    ref_c = np.stack([R.warp_affine_cv(frames[f], tf[f], (224, 224), "constant") for f in range(2)])
    assert np.array_equal(crops.cpu().numpy(), ref_c)
    assert np.array_equal(rz.cpu().numpy(), np.stack([R.resize_linear_u8(c, (256, 256)) for c in ref_c]))


class _PixelArc:
    """Stands in for netArc: a crop's embedding is an 8 x 8 grid of its pixels, so equal crops match with cosine 1
    and crops of independent textures with about 0."""

    def embed_u8(self, crops):
        return crops[:, 14::28, 14::28, :].reshape(crops.shape[0], -1).float() - 127.5


def test_the_chain_for_one_target_matches_the_full_frame_chain():
    from ghost_amd.inference import (align, blend_swaps_roi, crop_frames_and_get_transforms,
                                     crop_frames_and_get_transforms_roi, download_rois)
    from ghost_amd.inference.blend import blend_swaps
    from ghost_amd.inference.masks import face_masks, mask_params
    g = np.random.Generator(np.random.PCG64(91))
    tex = g.integers(0, 256, size=(2, 48, 48, 3), dtype=np.uint8)          # the two "faces"
    templates = FRONTAL[None] * 2.0                                         # crop = 5 (frame - offset)
    # per frame: (who, top-left corner) of each face in the detector's order; None: faceless.  With set_target every
    # frame that has a face is matched; the lone stranger of frame 3 is rejected.
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
    target = arc.embed_u8(torch.from_numpy(first[None])).to(DEV)           # the one target: face 0
    dev_frames = torch.from_numpy(frames).to(DEV)
    want = crop_frames_and_get_transforms(dev_frames, kps, target, arc, 224, True, 0.5, templates, embed_batch=4)
    host = [f.copy() for f in frames]                                       # the reference's list of frames
    crops, rz, present, tfm, plan, patches = crop_frames_and_get_transforms_roi(host, kps, target, arc, 224, True, 0.5,
                                                                                templates, DEV, embed_batch=4)
    assert present[0].tolist() == want[2][0].tolist() == [1, 1, 1, 0, 0, 1]
    for i in range(n):
        assert np.array_equal(np.asarray(tfm[0][i]), np.asarray(want[3][0][i])), i
    assert torch.equal(crops[0], want[0][0]) and torch.equal(rz[0], want[1][0]) and crops[0].shape[0] == 4
    assert plan.patch_of[0].tolist() == [0, 1, 2, -1, -1, 3] and plan.link_bytes() < 0.6 * frames.nbytes
    # swaps = the 256 crops themselves, frame-indexed; face_mask_static's masks from synthetic landmarks
    idx = torch.from_numpy(np.maximum(np.cumsum(present[0]) - 1, 0).astype(np.int64)).to(DEV)
    swaps = rz[0].index_select(0, idx)
    t_ = np.linspace(0.15 * np.pi, 0.85 * np.pi, 33) + np.pi
    base = np.concatenate([np.stack([112 + 78 * np.cos(-t_), 118 + 92 * np.sin(-t_)], 1),
                           np.stack([112 + g.uniform(-60, 60, 73), 118 + g.uniform(-70, 60, 73)], 1)])
    lms = (base[None] + g.normal(0, 1.5, (n, 106, 2))).astype(np.float32)
    params = np.tile(np.array(mask_params(lms[0], lms[1]), np.int32), (n, 1))
    masks = face_masks(lms, params, 224, 224, DEV)
    mats = np.stack([np.zeros((2, 3)) if len(m) == 0 else m for m in tfm[0]])
    valid = torch.from_numpy(present[0].astype(np.int32))
    blend_swaps(dev_frames, swaps, masks, mats, valid, resize_to=224)
    blend_swaps_roi(patches, plan, 0, swaps, masks, tfm[0], valid=valid, resize_to=224)
    download_rois(patches, plan, host)
    torch.cuda.synchronize()
    got, full = np.stack(host), dev_frames.cpu().numpy()
    assert np.array_equal(got, full)
    assert not np.array_equal(full[0], frames[0]) and np.array_equal(got[3:5], frames[3:5])


def test_python_refusals_before_any_copy_or_launch(small):
    from ghost_amd.inference import align_crops_roi, blend_swaps_roi, download_rois, plan_rois, upload_rois
    plan = small.shared
    patches = _upload_prefilled(small.pinned, plan)
    before = patches.clone()
    tf0 = small.tfms[[1, 3, 0]]                                             # identity 0, frames 0, 1, 2
    sw, mk = torch.zeros(3, C.S, C.S, 3, dtype=torch.uint8), torch.ones(3, C.S, C.S)
    for call in (lambda: upload_rois(small.dev_frames, plan, DEV),          # device frames
                 lambda: download_rois(patches, plan, small.dev_frames),
                 lambda: upload_rois(small.frames, plan, DEV, out=patches[:2]),                     # not the canvas
                 lambda: download_rois(patches[:, :, :4], plan, small.frames.copy()),
                 lambda: align_crops_roi(patches, small.solo, 0, small.tfms, C.S),                   # another plan
                 lambda: align_crops_roi(patches, plan, 0, tf0[:2], C.S),                            # a face missing
                 lambda: align_crops_roi(patches, plan, 0, tf0[::-1], C.S),                          # other transforms
                 lambda: align_crops_roi(patches, plan, 0, tf0, 63),                                 # other crop size
                 lambda: align_crops_roi(patches, plan, 0, tf0, C.S, want_crops=False),              # nothing to return
                 lambda: blend_swaps_roi(patches, plan, 0, sw, mk, tf0[::-1]),
                 lambda: blend_swaps_roi(patches, plan, 0, sw[:2], mk[:2], tf0),
                 lambda: blend_swaps_roi(patches, plan, 0, sw, mk[:, :40], tf0),
                 lambda: blend_swaps_roi(patches, plan, 0, sw, mk, tf0, valid=[1, 1])):
        with pytest.raises(RuntimeError):
            call()
    for q in (3, -1):
        with pytest.raises(IndexError):
            align_crops_roi(patches, plan, q, tf0, C.S)
        with pytest.raises(IndexError):
            blend_swaps_roi(patches, plan, q, sw, mk, tf0)
    # two rows of one call on the same patch would race on its pixels
    twice = plan_rois(C.tfm_lists([{0: small.tfms[1]}], 3), C.S, (C.H, C.W))
    twice.patch_of[0, 1] = twice.patch_of[0, 0]
    twice.tfms[0, 1] = twice.tfms[0, 0]
    with pytest.raises(RuntimeError, match="distinct"):
        blend_swaps_roi(_upload_prefilled(small.frames, twice), twice, 0, sw, mk, twice.tfms[0])
    torch.cuda.synchronize()
    assert torch.equal(patches, before)


def test_raw_abi_rejects_bad_arguments(small):
    from ghost_amd import _lib
    lib = _lib.load()
    plan = small.solo
    Ph, Pw = plan.canvas
    st = _lib.stream_ptr(torch.device(DEV))
    canvas = torch.full((plan.n_patches, Ph, Pw, 3), 0xFF, dtype=torch.uint8, device=DEV)
    ptrs = np.array([f.ctypes.data for f in small.solo_frames][:plan.n_patches], np.uint64)

    def copy(rects, ph=Ph, pw=Pw, to_device=1):
        rects = np.ascontiguousarray(rects, np.int32)
        return lib.ghost_roi_copy_u8(canvas.data_ptr(), Ph * Pw * 3, plan.n_patches, ph, pw, rects.ctypes.data,
                                     ptrs.ctypes.data, C.H, C.W, to_device, st)

    for k, bad in enumerate([(100, 0, 40, 40), (0, 90, 10, 10), (-1, 0, 10, 10), (0, 0, 10, -3)]):
        rects = plan.rects.copy()
        rects[plan.n_patches - 1] = bad                     # the last one: every copy before it would have run
        assert copy(rects) == -1 and b"leaves the frame" in lib.ghost_last_error(), k           # GHOST_EINVAL
    assert copy(plan.rects, pw=Pw + 4) == -1 and b"bad sizes" in lib.ghost_last_error()        # beyond the stride
    little = np.tile(np.array([4, 4, 8, 8], np.int32), (plan.n_patches, 1))
    for ph, pw in [(8, 4), (4, 8)]:
        assert copy(little, ph=ph, pw=pw) == -1 and b"larger than the canvas" in lib.ghost_last_error()
    assert lib.ghost_roi_copy_u8(canvas.data_ptr(), Ph * Pw * 3, plan.n_patches, Ph, Pw, None, ptrs.ctypes.data, C.H,
                                 C.W, 1, st) == -1 and b"null" in lib.ghost_last_error()
    assert lib.ghost_roi_copy_u8(canvas.data_ptr(), Ph * Pw * 3, 0, Ph, Pw, None, None, C.H, C.W, 1, st) == 0
    torch.cuda.synchronize()
    assert (canvas == 0xFF).all()                           # nothing was copied by any refused call
    empty = plan.rects.copy()
    empty[0] = (5, 5, 0, 7)                                 # an empty rectangle is skipped, the others copied
    assert copy(empty) == 0
    got = canvas.cpu().numpy()
    assert (got[0] == 0xFF).all()
    x0, y0, w, h = plan.rects[1]
    assert np.array_equal(got[1, :h, :w], small.solo_frames[1][y0:y0 + h, x0:x0 + w])

    patches = _upload_prefilled(small.solo_frames, plan)
    maps, index = _solo_device_args(small)
    S, N = small.S, 7
    crops = torch.full((N, S, S, 3), 0xA5, dtype=torch.uint8, device=DEV)
    rz = torch.full((N, 64, 64, 3), 0x5A, dtype=torch.uint8, device=DEV)
    assert _raw_align(lib, patches, plan, index, maps, None, N, S, None, 0, None, 0, 0) == -1    # no output at all
    assert b"null" in lib.ghost_last_error()
    for s_, r_ in [(S, 60), (S, 56), (50, 57)]:                                                 # unsupported (S, R)
        assert _raw_align(lib, patches, plan, index, maps, None, N, s_, None, 0, rz, 64 * 64 * 3, r_) == -1
        assert b"fused resize" in lib.ghost_last_error()
    assert _raw_align(lib, patches, plan, index, maps, None, N, S, crops, S * S * 3 - 1, None, 0, 0) == -1
    assert b"bad sizes" in lib.ghost_last_error()
    assert _raw_align(lib, patches, plan, index, maps, None, 65536, S, crops, S * S * 3, None, 0, 0) == -1
    assert _raw_align(lib, patches, plan, index, maps, None, N, S, crops, S * S * 3, None, 0, 0, Np=0) == -1
    assert _raw_align(lib, patches, plan, index, maps, None, 0, S, crops, S * S * 3, None, 0, 0) == 0     # N == 0: OK

    def blend(N_, swaps, hs=S, np_=plan.n_patches):
        mats = torch.zeros(7, 6, device=DEV)
        masks = torch.ones(7, S, S, device=DEV)
        return lib.ghost_blend_swaps_roi_u8(patches.data_ptr(), Ph * Pw * 3, np_, Ph, Pw,
                                            plan.device("rects", patches.device).data_ptr(), index.data_ptr(), N_,
                                            None if swaps is None else swaps.data_ptr(), S * S * 3, hs, S,
                                            masks.data_ptr(), S * S, mats.data_ptr(), None, st)

    assert blend(7, None) == -1 and b"null" in lib.ghost_last_error()
    assert blend(7, crops, hs=S + 1) == -1 and b"bad sizes" in lib.ghost_last_error()
    assert blend(7, crops, np_=0) == -1 and blend(65536, crops) == -1
    assert blend(0, crops) == 0                                                                  # N == 0: OK
    torch.cuda.synchronize()
    assert (crops == 0xA5).all() and (rz == 0x5A).all()     # refused on the host: nothing was launched
    _check_canvas(patches, plan, small.solo_frames)
