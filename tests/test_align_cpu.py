"""Host geometry of ghost_amd.inference.align (numpy float64, no GPU): the similarity fit, the template choice,
landmark smoothing and the per-identity keypoint / present / tfm_array bookkeeping."""
import numpy as np
import pytest

from ghost_amd.inference import align

FRONTAL = np.array([[38.0, 52.0], [74.0, 51.0], [56.0, 72.0], [41.0, 92.0], [71.0, 91.0]])


def _similarity(scale, ang, tx, ty):
    c, s = scale * np.cos(ang), scale * np.sin(ang)
    return np.array([[c, -s, tx], [s, c, ty], [0.0, 0.0, 1.0]])


def _apply(M, pts):
    return pts @ M[:2, :2].T + M[:2, 2]


def _templates():
    shear = np.array([[1.0, 0.25], [0.0, 1.0]])
    return np.stack([FRONTAL, FRONTAL @ shear.T + np.array([9.0, -4.0]), FRONTAL @ shear + np.array([-7.0, 6.0])])


@pytest.mark.parametrize("seed", range(8))
def test_similarity_transform_recovers_known_similarity(seed):
    g = np.random.Generator(np.random.PCG64(seed))
    scale = g.uniform(0.2, 3.0)
    ang = g.uniform(-np.pi, np.pi)
    # source and destination coordinates both stay inside [0, 2000] (the bound's derivation assumes that)
    r = min(1000.0, 700.0 / scale)
    src = 1000.0 + g.uniform(-r, r, size=(5, 2))
    M = _similarity(scale, ang, 0.0, 0.0)
    M[:2, 2] = g.uniform(800, 1200, size=2) - M[:2, :2] @ np.array([1000.0, 1000.0])
    dst = _apply(M, src)
    assert 0 <= dst.min() and dst.max() <= 2000
    got = align.similarity_transform(src, dst)
    assert got.shape == (3, 3) and got.dtype == np.float64
    assert np.allclose(got, M, rtol=0, atol=1e-8), np.abs(got - M).max()


def test_similarity_transform_mirrored_points_give_a_rotation():
    g = np.random.Generator(np.random.PCG64(3))
    src = g.uniform(0, 200, size=(5, 2))
    dst = src * np.array([-1.0, 1.0]) + np.array([300.0, 5.0])          # a reflection
    got = align.similarity_transform(src, dst)
    assert np.isfinite(got).all()
    assert np.linalg.det(got[:2, :2]) > 0
    a, b = got[0, 0], got[1, 0]
    assert np.allclose(got[:2, :2], [[a, -b], [b, a]], atol=1e-12)      # still a similarity


def test_similarity_transform_collinear_points():
    src = np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0], [3.0, 3.0], [5.0, 5.0]])
    M = _similarity(1.7, 0.6, 4.0, -3.0)
    got = align.similarity_transform(src, _apply(M, src))
    assert np.linalg.det(got[:2, :2]) > 0
    assert np.allclose(_apply(got, src), _apply(M, src), atol=1e-9)


@pytest.mark.parametrize("seed", range(4))
def test_similarity_transform_is_the_least_squares_optimum(seed):
    from scipy.optimize import least_squares
    g = np.random.Generator(np.random.PCG64(100 + seed))
    src = g.uniform(0, 500, size=(5, 2))
    M = _similarity(g.uniform(0.2, 3.0), g.uniform(-np.pi, np.pi), g.uniform(-100, 100), g.uniform(-100, 100))
    dst = _apply(M, src) + g.normal(0, 3.0, size=(5, 2))

    def resid(p):
        a, b, tx, ty = p
        return (_apply(np.array([[a, -b, tx], [b, a, ty]]), src) - dst).ravel()

    ref = least_squares(resid, [M[0, 0], M[1, 0], M[0, 2], M[1, 2]], xtol=1e-15, ftol=1e-15, gtol=1e-15)
    got = align.similarity_transform(src, dst)
    mine = np.sum((_apply(got, src) - dst) ** 2)
    assert mine <= np.sum(ref.fun ** 2) * (1 + 1e-9)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_estimate_norm_picks_the_generating_template(which):
    T = _templates()
    g = np.random.Generator(np.random.PCG64(which))
    back = np.linalg.inv(_similarity(g.uniform(0.3, 0.8), g.uniform(-0.5, 0.5), g.uniform(-200, 0), g.uniform(-150, 0)))
    lmk = _apply(back, T[which])                                       # frame landmarks that map onto template `which`
    M, idx = align.estimate_norm(lmk, 112, T)
    assert idx == which and M.shape == (2, 3) and M.dtype == np.float64
    fits = [align.similarity_transform(lmk, t)[:2] for t in T]
    errs = [np.sum(np.linalg.norm(_apply(f, lmk) - t, axis=1)) for f, t in zip(fits, T)]
    assert np.array_equal(M, fits[which])
    assert errs[which] == min(errs) and errs[which] < 1e-9
    assert np.allclose(_apply(M, lmk), T[which], atol=1e-9)


def test_estimate_norm_tie_goes_to_the_first():
    T = np.stack([FRONTAL, FRONTAL])
    _, idx = align.estimate_norm(FRONTAL * 2.0 + 3.0, 112, T)
    assert idx == 0


def _track(n, step=1.0):
    return [FRONTAL + step * i for i in range(n)]


def test_smooth_landmarks_steady_track_windows():
    ka = _track(7)
    out = align.smooth_landmarks([ka], n=2)[0]
    assert len(out) == 7
    for i, q in enumerate([0, 1, 2, 2, 2, 1, 0]):
        assert np.allclose(out[i], np.mean(ka[i - q:i + q + 1], axis=0), atol=1e-12)
    # a linear track is its own centred mean
    assert np.allclose(np.stack(out), np.stack(ka), atol=1e-12)
    # a non-linear one is not: windows checked by hand
    kb = [FRONTAL + np.array([v, 0.0]) for v in (0.0, 1.0, 4.0, 5.0, 9.0)]
    ob = align.smooth_landmarks([kb], n=2)[0]
    assert np.allclose([o[0, 0] - FRONTAL[0, 0] for o in ob], [0.0, 5 / 3, 19 / 5, 6.0, 9.0], atol=1e-12)


def test_smooth_landmarks_jump_in_point_2_splits():
    ka = _track(6, step=0.5)
    for i in range(3, 6):
        ka[i] = ka[i].copy()
        ka[i][2] += np.array([6.0, 0.0])        # point 2 jumps 6.02 px between frames 2 and 3
    out = align.smooth_landmarks([ka], n=2)[0]
    # segments [0,1,2] and [3,4,5]: windows 0,1,0 each
    for i, (lo, hi) in enumerate([(0, 1), (0, 3), (2, 3), (3, 4), (3, 6), (5, 6)]):
        assert np.allclose(out[i], np.mean(ka[lo:hi], axis=0), atol=1e-12), i


def test_smooth_landmarks_jump_in_point_1_alone_does_not_split():
    ka = _track(5, step=0.5)
    for i in range(2, 5):
        ka[i] = ka[i].copy()
        ka[i][1] += np.array([40.0, 0.0])
    out = align.smooth_landmarks([ka], n=2)[0]
    for i, q in enumerate([0, 1, 2, 1, 0]):
        assert np.allclose(out[i], np.mean(ka[i - q:i + q + 1], axis=0), atol=1e-12)


def test_smooth_landmarks_empty_entry_passes_through_and_splits():
    ka = _track(6, step=0.5)
    ka[3] = []
    out = align.smooth_landmarks([ka, [[], FRONTAL]], n=2)
    a = out[0]
    assert len(a) == 6 and len(a[3]) == 0
    for i, (lo, hi) in {0: (0, 1), 1: (0, 3), 2: (2, 3), 4: (4, 5), 5: (5, 6)}.items():
        assert np.allclose(a[i], np.mean(ka[lo:hi], axis=0), atol=1e-12), i
    assert len(out[1][0]) == 0 and np.allclose(out[1][1], FRONTAL)


def _faces(*offsets):
    return np.stack([FRONTAL * 0.8 + np.array(o, float) for o in offsets])


def test_bookkeeping_single_target():
    T = _templates()
    kps = [_faces((10, 10)), None, _faces((11, 10)), _faces((12, 11), (200, 40)), _faces((13, 11))]
    assert align.frames_to_match(kps, set_target=False) == [3]
    matches = {3: (np.array([1]), np.array([True]))}
    ka = align.select_keypoints(kps, 1, False, matches)
    assert len(ka) == 1 and len(ka[0]) == 5
    assert np.array_equal(ka[0][0], kps[0][0]) and len(ka[0][1]) == 0 and np.array_equal(ka[0][3], kps[3][1])
    present, tfm = align.frame_transforms(ka, 112, T)
    assert present[0].dtype == np.float64 and present[0].tolist() == [1, 0, 1, 1, 1]
    assert len(tfm[0]) == 5 and len(tfm[0][1]) == 0
    # frame 0 stands alone (frame 1 is empty): unsmoothed keypoints; frame 3 jumped to another face: alone too
    assert np.array_equal(tfm[0][0], align.estimate_norm(kps[0][0], 112, T)[0])
    assert np.array_equal(tfm[0][2], align.estimate_norm(kps[2][0], 112, T)[0])
    assert np.array_equal(tfm[0][3], align.estimate_norm(kps[3][1], 112, T)[0])
    # with set_target every frame with a face is matched, and a rejected match leaves the frame absent
    assert align.frames_to_match(kps, set_target=True) == [0, 2, 3, 4]
    m = {i: (np.array([0]), np.array([i != 2])) for i in (0, 2, 3, 4)}
    ka = align.select_keypoints(kps, 1, True, m)
    present, _ = align.frame_transforms(ka, 112, T)
    assert present[0].tolist() == [1, 0, 0, 1, 1]


def test_bookkeeping_two_targets():
    T = _templates()
    kps = [_faces((10, 10), (200, 40)), _faces((10.5, 10)), None, _faces((201, 41), (11, 10))]
    assert align.frames_to_match(kps, set_target=False) == [0, 3]
    matches = {0: (np.array([0, 1]), np.array([True, True])), 3: (np.array([1, 0]), np.array([True, False]))}
    ka = align.select_keypoints(kps, 2, False, matches)
    assert [len(k) for k in ka] == [4, 4]                       # one entry per frame for every identity
    assert np.array_equal(ka[0][0], kps[0][0]) and np.array_equal(ka[1][0], kps[0][1])
    assert np.array_equal(ka[0][1], kps[1][0]) and len(ka[1][1]) == 0      # a single face goes to identity 0
    assert len(ka[0][2]) == 0 and len(ka[1][2]) == 0                       # faceless frame
    assert np.array_equal(ka[0][3], kps[3][1]) and len(ka[1][3]) == 0      # identity 1 rejected by the threshold
    present, tfm = align.frame_transforms(ka, 112, T)
    assert present[0].tolist() == [1, 1, 0, 1] and present[1].tolist() == [1, 0, 0, 0]
    assert [len(t) for t in tfm] == [4, 4]
    # identity 0, frames 0-1 form one segment of two: windows 0, 0 (q = min(i, len-1-i, 2))
    assert np.array_equal(tfm[0][1], align.estimate_norm(kps[1][0], 112, T)[0])
    assert len(tfm[1][1]) == 0 and len(tfm[0][2]) == 0 and tfm[1][0].shape == (2, 3)
