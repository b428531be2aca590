"""Host-side checks for the device mask polygons (ghost_mask_polygons_dev, ghost_amd/csrc/mask_poly.hip; no GPU):
the index arrays of identity_masks_device against present_runs, the new entry point in the ABI tables, and the host
yardstick (ghost_mask_polygons) against the oracle on the landmark sets of tests/mask_poly_cases.py, which
tests/test_mask_poly_gpu.py then holds the device path to bit for bit."""
import numpy as np
import pytest

import mask_poly_cases as cases
from oracle import mask_ref as M

PATTERN = [0, 1, 1, 0, 0, 1, 0, 1, 1, 1]


def _check_runs(present):
    from ghost_amd.landmarks import present_runs, run_indices
    idx, starts, ref_index, tgt_index = run_indices(present)
    runs = present_runs(present)
    assert idx.tolist() == [i for i, p in enumerate(present) if p]
    assert starts.tolist() == [a for a, _ in runs]
    assert ref_index.dtype == np.int32 and tgt_index.dtype == np.int32
    assert len(ref_index) == len(tgt_index) == len(idx)
    for k, frame in enumerate(idx.tolist()):
        r = [n for n, (a, b) in enumerate(runs) if a <= frame < b]
        assert len(r) == 1
        assert tgt_index[k] == r[0]                       # the run number: a row of the target-crop batch
        assert idx[ref_index[k]] == runs[r[0]][0]         # the run's first present frame: a row of the swap batch
    return idx, starts, ref_index, tgt_index


def test_run_indices_pattern():
    idx, starts, ref_index, tgt_index = _check_runs(PATTERN)
    assert idx.tolist() == [1, 2, 5, 7, 8, 9] and starts.tolist() == [1, 5, 7]
    assert ref_index.tolist() == [0, 0, 2, 3, 3, 3] and tgt_index.tolist() == [0, 0, 1, 2, 2, 2]


@pytest.mark.parametrize("present", [[0, 0, 0, 0], [1, 1, 1, 1, 1], [1, 0, 0, 0], [0, 0, 0, 1], [1], [0], [],
                                     [1, 0, 1, 0, 1], [True, True, False, True]])
def test_run_indices_edges(present):
    idx, starts, ref_index, tgt_index = _check_runs(present)
    if not any(present):
        assert len(idx) == len(starts) == len(ref_index) == len(tgt_index) == 0


def test_entry_point_in_abi_tables():
    from ghost_amd import _lib
    assert "ghost_mask_polygons_dev" in _lib._SIGS
    assert "ghost_mask_polygons_dev" in _lib.header_symbols()
    assert hasattr(_lib.load(), "ghost_mask_polygons_dev")
    import ghost_amd.landmarks as L
    from ghost_amd.inference.masks import face_masks_device, mask_polygons_device
    from ghost_amd.landmarks import identity_masks_device, run_indices
    assert "identity_masks_device" in L.__all__ and "run_indices" in L.__all__
    assert callable(face_masks_device) and callable(mask_polygons_device)
    assert callable(identity_masks_device) and callable(run_indices)


def test_entry_point_refuses_bad_argument_sets():
    """Exactly one of params_in / the four reference arguments; F = 0 is no launch.  (Host-side checks only: they
    return before anything touches a device.)"""
    from ghost_amd import _lib
    lib = _lib.load()
    p = 4096          # never dereferenced
    call = lib.ghost_mask_polygons_dev
    assert call(p, None, None, None, 0, None, None, 0, p, p, p, 4, None) != 0            # neither form
    assert b"ghost_mask_polygons_dev" in lib.ghost_last_error()
    assert call(p, p, p, p, 1, p, p, 1, p, p, p, 4, None) != 0                        # both forms
    assert call(p, None, p, p, 1, None, p, 1, p, p, p, 4, None) != 0                  # half a reference set
    assert call(p, None, p, p, 0, p, p, 1, p, p, p, 4, None) != 0                     # an empty reference set
    assert call(p, p, None, None, 0, None, None, 0, p, p, p, -1, None) != 0           # F < 0
    assert call(p, p, None, None, 0, None, None, 0, p, p, p, 0, None) == 0            # F = 0: nothing to do


@pytest.mark.parametrize("name", ["face_like", "contraction", "degenerate", "large_hull", "far_points"])
def test_host_yardstick_matches_oracle(name):
    """mask_polygons = the oracle's expand_eyebrows + convex_hull as vertex sets on every set the GPU test uses."""
    from ghost_amd.inference.masks import mask_polygons
    lms, params = cases.all_sets()[name]
    poly, nv = mask_polygons(lms, params)
    for f in range(len(lms)):
        hull = M.convex_hull(M.expand_eyebrows(lms[f], M.eyebrow_mod(params[f][0])))
        assert nv[f] == len(hull), (name, f)
        assert set(map(tuple, poly[f, :nv[f]].tolist())) == set(map(tuple, hull.tolist())), (name, f)
        assert not poly[f, nv[f]:].any()


def test_fixtures_are_what_they_claim():
    """The contraction sets hold at least 20 pairs that a fused multiply-add would move, each expanded point a vertex
    of the host's hull; the degenerate and large hulls have the stated sizes on the host path."""
    from ghost_amd.inference.masks import mask_polygons
    lms, params, want, n_hazard = cases.contraction()
    assert n_hazard >= 20
    assert cases.expand_exact(28, 48, 2.7, False) == 1 and cases.expand_exact(28, 48, 2.7, True) == 0
    poly, nv = mask_polygons(lms, params)
    for f in range(len(lms)):
        verts = set(map(tuple, poly[f, :nv[f]].tolist()))
        assert all(tuple(w) in verts for w in want[f].tolist()), f
    _, nv = mask_polygons(*cases.degenerate())
    assert nv[:3].tolist() == [1, 2, 2] and nv[4] == 4 and 3 <= nv[3] <= 8
    _, nv = mask_polygons(*cases.large_hull())
    assert (nv >= 90).all()
