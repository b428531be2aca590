"""The device mask polygons (ghost_mask_polygons_dev, ghost_amd/csrc/mask_poly.hip) on an MI355X against the host
path they replace.  The arithmetic is integer after one cast, so every comparison is exact (np.array_equal): poly
(the whole array, zeros past nv included) and nv against ``mask_polygons``, the derived parameters against
``mask_params``, masks against ``face_masks`` / ``identity_masks``.  tests/test_mask_poly_cpu.py shows that the host
path does on these sets what the oracle does.  F <= 64 everywhere."""
import numpy as np
import pytest
import torch

import landmark_ref
import mask_poly_cases as cases

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PATTERN = [0, 1, 1, 0, 0, 1, 0, 1, 1, 1]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _compare_polygons(lms, params):
    from ghost_amd.inference.masks import mask_polygons, mask_polygons_device
    poly, nv = mask_polygons(lms, params)
    d_poly, d_nv, d_pr = mask_polygons_device(_dev(lms), _dev(params))
    assert d_poly.dtype == torch.int32 and tuple(d_poly.shape) == poly.shape and d_nv.dtype == torch.int32
    got_nv, got_poly = d_nv.cpu().numpy(), d_poly.cpu().numpy()
    assert np.array_equal(got_nv, nv), (got_nv.tolist(), nv.tolist())
    bad = np.flatnonzero((got_poly != poly).any(axis=(1, 2)))
    assert np.array_equal(got_poly, poly), f"faces {bad.tolist()} differ"
    assert np.array_equal(d_pr.cpu().numpy(), params)
    return poly, nv


def test_face_like_sets():
    _compare_polygons(*cases.face_like())


def test_contraction():
    """A kernel that fuses the eyebrow expansion's multiply-add moves at least 20 of these sets' expanded points,
    each a vertex of the host's hull, by one."""
    lms, params, want, n_hazard = cases.contraction()
    assert n_hazard >= 20 and len(lms) <= 64
    poly, nv = _compare_polygons(lms, params)
    for f in range(len(lms)):
        verts = set(map(tuple, poly[f, :nv[f]].tolist()))
        assert all(tuple(w) in verts for w in want[f].tolist()), f


def test_degenerate_hulls():
    _, nv = _compare_polygons(*cases.degenerate())
    assert nv[:3].tolist() == [1, 2, 2] and nv[4] == 4


def test_large_hull():
    _, nv = _compare_polygons(*cases.large_hull())
    assert (nv >= 90).all()


def test_negative_and_large_coordinates():
    lms, params = cases.far_points()
    assert np.abs(lms).max() > 9e5
    _compare_polygons(lms, params)


def _quarter(a):
    return (np.round(np.asarray(a, np.float64) * 4) / 4).astype(np.float32)   # differences of these are exact


def test_derived_params():
    """(erode, sigmaX, sigmaY) from two landmark sets: each branch, each threshold hit exactly, rounded sums, and
    several faces sharing one reference."""
    from ghost_amd.inference.masks import mask_params, mask_polygons, mask_polygons_device
    t0 = _quarter(cases.landmarks(5))

    def pair(left, right):
        """a with left = sum over 1, 2, 13 of a.x - t.x and right = sum over 17, 18, 29 of t.x - a.x, exactly."""
        a = t0.copy()
        for i, w in zip((1, 2, 13), (0.25, 0.5, 0.25)):
            a[i, 0] += np.float32(left * w)
        for i, w in zip((17, 18, 29), (0.5, 0.25, 0.25)):
            a[i, 0] -= np.float32(right * w)
        return a
    exact = [(10, -2), (-2, 10), (4.5, 1), (1, 4.5), (-5, -6), (-6, -5), (0, 0), (2, -8),
             (6, -1), (-1, 6), (6, 6), (3, -1), (3, 3), (-3, -3.5), (-3.5, -3), (-3, -3), (-3.5, -4), (7, 8)]
    want_exact = [[15, 15, 10]] * 2 + [[10, 10, 8]] * 2 + [[-5, 5, 10]] * 2 + [[5, 5, 5]] * 2 + \
                 [[10, 10, 8]] * 3 + [[5, 5, 5]] * 5 + [[-5, 5, 10]] + [[15, 15, 10]]
    refs = [pair(l, r) for l, r in exact]
    tgts = [t0] * len(exact)
    for s in range(8):                                   # unrounded values: the order of the fp32 sums matters
        refs.append(cases.landmarks(s))
        tgts.append(cases.landmarks(s + 100, shift=(s - 4, 0)))
    n = len(refs)
    assert [mask_params(refs[i], tgts[i]) for i in range(len(exact))] == want_exact
    # face k uses reference k % n and target k % n: with 2 n > F > n some references are shared
    F = 40
    ref_index = np.array([k % n for k in range(F)], np.int32)
    tgt_index = ref_index.copy()
    # the faces' own landmarks are another set: the parameters come from the indexed sets alone
    lms = np.stack([cases.landmarks(50 + k % 5) for k in range(F)])
    want = np.array([mask_params(refs[i], tgts[i]) for i in ref_index], np.int32)
    assert len({tuple(w) for w in want.tolist()}) == 4
    d_poly, d_nv, d_pr = mask_polygons_device(_dev(lms), landmarks_ref=_dev(np.stack(refs)), ref_index=_dev(ref_index),
                                              landmarks_tgt=_dev(np.stack(tgts)), tgt_index=_dev(tgt_index))
    assert np.array_equal(d_pr.cpu().numpy(), want)
    poly, nv = mask_polygons(lms, want)
    assert np.array_equal(d_nv.cpu().numpy(), nv) and np.array_equal(d_poly.cpu().numpy(), poly)


def test_argument_forms():
    from ghost_amd.inference.masks import mask_polygons_device
    lms, params = cases.face_like()
    with pytest.raises(RuntimeError):
        mask_polygons_device(_dev(lms))
    with pytest.raises(RuntimeError):
        mask_polygons_device(_dev(lms), _dev(params), landmarks_ref=_dev(lms))
    with pytest.raises(RuntimeError):
        mask_polygons_device(torch.from_numpy(lms), torch.from_numpy(params))
    poly, nv, pr = mask_polygons_device(_dev(lms[:0]), _dev(params[:0]))
    assert tuple(poly.shape) == (0, 128, 2) and tuple(nv.shape) == (0,) and tuple(pr.shape) == (0, 3)


@pytest.mark.parametrize("H,W", [(224, 224), (160, 200)])
def test_face_masks_device_equals_face_masks(H, W):
    from ghost_amd.inference.masks import face_masks, face_masks_device
    lms, params = cases.face_like()
    want = face_masks(lms, params, H, W, DEV).cpu().numpy()
    got = face_masks_device(_dev(lms), _dev(params), H, W)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(lms), H, W)
    assert np.array_equal(got.cpu().numpy(), want)
    assert want.max() == 1.0


class _TableNet:
    """``landmarks_u8`` looks the landmarks up in a table by the first byte of each crop."""
    def __init__(self):
        base = cases.landmarks(3)
        wide = base.copy()
        wide[:, 0] = 112 + (base[:, 0] - 112) * 1.08
        narrow = base.copy()
        narrow[:, 0] = 112 + (base[:, 0] - 112) * 0.97
        variants = [base, base + np.float32([1.3, 0]), base + np.float32([2.6, 0]), wide, narrow, cases.landmarks(4)]
        self.table = _dev(np.stack([variants[k % 6] for k in range(256)]))

    def landmarks_u8(self, crops):
        return self.table[crops[:, 0, 0, 0].long()]


def _identity_inputs(present, swap_bytes, crop_bytes):
    F = len(present)
    swaps = torch.zeros(F, 256, 256, 3, dtype=torch.uint8, device=DEV)
    crops = torch.zeros(F, 224, 224, 3, dtype=torch.uint8, device=DEV)
    swaps += _dev(np.array(swap_bytes, np.uint8)).view(F, 1, 1, 1)       # constant images survive the resize
    crops += _dev(np.array(crop_bytes, np.uint8)).view(F, 1, 1, 1)
    return swaps, crops


def _compare_identity(net, swaps, crops, present, H=224, W=224):
    from ghost_amd.landmarks import identity_masks, identity_masks_device
    m0, s0, lm0, p0 = identity_masks(net, swaps, crops, present, H, W)
    m1, s1, lm1, p1 = identity_masks_device(net, swaps, crops, present, H, W)
    assert lm1.is_cuda and lm1.dtype == torch.float32 and p1.is_cuda and p1.dtype == torch.int32
    assert torch.equal(s0, s1)
    assert np.array_equal(lm1.cpu().numpy(), lm0)
    assert np.array_equal(p1.cpu().numpy(), p0)
    assert np.array_equal(m1.cpu().numpy(), m0.cpu().numpy())
    absent = ~np.asarray(present, bool)
    assert not m1.cpu().numpy()[absent].any() and not lm1.cpu().numpy()[absent].any()
    assert not p1.cpu().numpy()[absent].any()
    return m1, lm1, p1


# frames 1, 5 and 7 start the runs, with swap / crop table rows (0, 0): equal sets, (3, 4): wide against narrow,
# (1, 0): a shift of 1.3 px; the other bytes select rows that must not matter
SWAP_BYTES = [9, 0, 1, 9, 9, 3, 9, 1, 2, 0]
CROP_BYTES = [9, 0, 9, 9, 9, 4, 9, 0, 9, 9]


def test_identity_masks_device_equals_identity_masks():
    net = _TableNet()
    swaps, crops = _identity_inputs(PATTERN, SWAP_BYTES, CROP_BYTES)
    m, lm, p = _compare_identity(net, swaps, crops, PATTERN)
    runs = p.cpu().numpy()[[1, 5, 7]]
    assert len({tuple(r) for r in runs.tolist()}) == 3, runs.tolist()       # the runs differ in regime
    assert float(m[1].max()) == 1.0
    _compare_identity(net, swaps, crops, PATTERN, 160, 200)


def test_identity_masks_device_all_absent():
    from ghost_amd.landmarks import identity_masks_device
    swaps, crops = _identity_inputs([0] * 4, [1] * 4, [2] * 4)
    m, s, lm, p = identity_masks_device(_TableNet(), swaps, crops, [0] * 4)
    torch.cuda.synchronize()
    assert tuple(m.shape) == (4, 224, 224) and tuple(s.shape) == (4, 224, 224, 3)
    assert not m.any() and not lm.any() and not p.any()


def test_identity_masks_device_does_not_synchronise():
    """The call completes under torch's sync debug mode "error"; ``identity_masks``, which copies the landmarks to
    the host, must raise under the same mode (a mode that cannot see that copy would prove nothing)."""
    from ghost_amd.landmarks import identity_masks, identity_masks_device
    net = _TableNet()
    swaps, crops = _identity_inputs(PATTERN, SWAP_BYTES, CROP_BYTES)
    identity_masks_device(net, swaps, crops, PATTERN)          # library load, allocator warm-up
    torch.cuda.synchronize()
    try:
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
    except (AttributeError, NotImplementedError, RuntimeError) as e:
        pytest.skip(f"torch.cuda.set_sync_debug_mode is not implemented by this build: {e}")
    try:
        out = identity_masks_device(net, swaps, crops, PATTERN)
        with pytest.raises(RuntimeError):
            identity_masks(net, swaps, crops, PATTERN)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert float(out[0][1].max()) == 1.0


def test_identity_masks_device_real_network():
    from ghost_amd.landmarks import Landmark106
    net = Landmark106()
    net.load_state_dict(landmark_ref.make_weights(), strict=True)
    net = net.to(DEV)
    g = np.random.Generator(np.random.PCG64(11))
    swaps = _dev(g.integers(0, 256, (3, 256, 256, 3), dtype=np.uint8))
    crops = landmark_ref.make_input(3, 224).to(DEV)
    _compare_identity(net, swaps, crops, [1, 0, 1])
