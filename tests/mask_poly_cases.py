"""Landmark sets shared by tests/test_mask_poly_cpu.py and tests/test_mask_poly_gpu.py (seeded, built once per process).

Every function returns (landmarks float32 [F,106,2], params int32 [F,3]); F <= 64.  The CPU file checks that the host
path (ghost_mask_polygons) does on them what the oracle does, the GPU file compares the device path with the host path.
"""
import functools
from fractions import Fraction

import numpy as np

REGIMES = [[15, 15, 10], [10, 10, 8], [-5, 5, 10], [5, 5, 5]]
TOP = [43, 48, 49, 51, 50, 102, 103, 104, 105, 101]     # expand_eyebrows' tables (masks.py:9-16), left then right
BOT = [35, 41, 40, 42, 39, 89, 95, 94, 96, 93]
OTHER = [i for i in range(106) if i not in TOP and i not in BOT]


def landmarks(seed, shift=(0.0, 0.0), scale=1.0):
    """tests/test_masks.py's recipe: a 33-point jaw/forehead contour on an ellipse + 73 interior points."""
    g = np.random.Generator(np.random.PCG64(seed))
    t = np.linspace(0.15 * np.pi, 0.85 * np.pi, 33) + np.pi
    cx, cy = 112 + shift[0], 118 + shift[1]
    contour = np.stack([cx + 78 * scale * np.cos(-t), cy + 92 * scale * np.sin(-t)], 1)
    inner = np.stack([cx + g.uniform(-60, 60, 73) * scale, cy + g.uniform(-70, 60, 73) * scale], 1)
    pts = np.concatenate([contour, inner]) + g.normal(0, 1.5, (106, 2))
    return pts.astype(np.float32)


@functools.lru_cache(None)
def face_like():
    """The four regimes twice and the three off-image / small-face cases of test_face_masks_match_oracle."""
    cases = [(landmarks(s), REGIMES[s % 4]) for s in range(8)]
    cases += [(landmarks(20, shift=(-70, 0)), [10, 10, 8]), (landmarks(21, shift=(0, -80), scale=1.2), [-5, 5, 10]),
              (landmarks(22, scale=0.2), [5, 5, 5])]
    return np.stack([c[0] for c in cases]), np.array([c[1] for c in cases], np.int32)


def expand_exact(top: int, bot: int, mod: float, fused: bool) -> int:
    """(int32)((double)top + (mod * 0.5) * (double)(top - bot)) in exact rational arithmetic: the product rounded to
    double before the add (what the host computes), or kept exact into one rounding (a fused multiply-add)."""
    m = Fraction(mod * 0.5)                      # the double the code holds (halving is exact)
    prod = m * (top - bot)
    if not fused:
        prod = Fraction(float(prod))             # int / int true division: correctly rounded
    return int(float(Fraction(top) + prod))      # int(): truncation toward zero


SQUARE_LO, SQUARE_HI = -100, 320
PARABOLA_C = 200000
DY = -100001     # top.y - bot.y of the swept pairs: 1.35 * DY is far from an integer, so y has no hazard


def _square(n):
    """n points on the boundary of the fixed square, corners first."""
    lo, hi = SQUARE_LO, SQUARE_HI
    pts = [(lo, lo), (hi, lo), (hi, hi), (lo, hi)]
    k = 0
    while len(pts) < n:
        t = lo + 5 + 7 * (k // 4)
        pts.append([(t, lo), (hi, t), (t, hi), (lo, t)][k % 4])
        k += 1
    return np.array(pts, np.int64)


@functools.lru_cache(None)
def contraction():
    """Sets under erode = 15 (mod 2.7) whose ten (top, bot) pairs sweep, in x, top - bot over [-60, 60] and top over
    [0, 224): every pair where a fused multiply-add gives another integer than multiply-then-add (decided in exact
    arithmetic) and a grid of the rest.  Returns (landmarks, params, expected expanded tops int64 [F,10,2], the number
    of such pairs).

    The expanded point of a pair is (x', x'^2 - C) with x' the unfused result: the expanded points lie on a parabola
    far below the fixed square of the other points, each with every other point of its set strictly above its tangent
    (square: 2 * 305 * 320 < C; a pair's bot, 235002 above its expanded top, has x^2 <= 284^2 < 235002), so each is a
    hull vertex and another x' changes the hull.  In y the pairs have top - bot = DY, whose expansion is the same
    fused or not (asserted)."""
    hazard = [(t, d) for t in range(224) for d in range(-60, 61)
              if expand_exact(t, t - d, 2.7, False) != expand_exact(t, t - d, 2.7, True)]
    assert (28, -20) in hazard
    grid = [(t, d) for t in (0, 75, 150, 223) for d in range(-60, 61)]     # 10 pairs a set, 64 sets at the most
    samples = hazard + grid
    samples += [(0, 0)] * (-len(samples) % 10)
    F = len(samples) // 10
    assert F <= 64
    lm = np.zeros((F, 106, 2), np.int64)
    want = np.zeros((F, 10, 2), np.int64)
    lm[:, OTHER] = _square(len(OTHER))
    for f in range(F):
        for s, (t, d) in enumerate(samples[10 * f:10 * f + 10]):
            x1 = expand_exact(t, t - d, 2.7, False)
            y1 = x1 * x1 - PARABOLA_C
            ty = y1 + 135001
            assert expand_exact(ty, ty - DY, 2.7, False) == y1 == expand_exact(ty, ty - DY, 2.7, True)
            lm[f, TOP[s]] = (t, ty)
            lm[f, BOT[s]] = (t - d, ty - DY)
            want[f, s] = (x1, y1)
    # a fraction that truncation toward zero removes
    lmf = (lm + 0.4 * np.sign(lm)).astype(np.float32)
    assert np.array_equal(lmf.astype(np.int32), lm)
    return lmf, np.tile(np.array([[15, 15, 10]], np.int32), (F, 1)), want, len(hazard)


@functools.lru_cache(None)
def degenerate():
    """nv = 1, 2, 2, a few, 4: all points equal; all on one line; two distinct values; many duplicates; long collinear
    stretches on a square's edges.  erode = 5 (mod 2.0: the expansion is top + (top - bot), exact)."""
    g = np.random.Generator(np.random.PCG64(7))
    i = np.arange(106)
    same = np.full((106, 2), 7.9, np.float32)
    line = np.stack([3.0 * i - 100, 2 * (3.0 * i - 100) + 3], 1).astype(np.float32)
    two = np.where((i % 2 == 0)[:, None], np.array([5.2, 5.9]), np.array([50.5, 9.1])).astype(np.float32)
    two[TOP + BOT] = (5.2, 5.9)
    dup = np.array([[10, 10], [90, 14], [60, 80], [12, 70], [50, 40], [51, 41], [90, 14.5]])[g.integers(0, 7, 106)]
    t = 10 + (i % 27) * 7.0
    edges = np.stack([np.where(i < 27, t, np.where(i < 54, 199, np.where(i < 81, t, 10))),
                      np.where(i < 27, 10, np.where(i < 54, t, np.where(i < 81, 199, t)))], 1)
    edges[[0, 1, 2, 3]] = [(10, 10), (199, 10), (199, 199), (10, 199)]
    edges[TOP + BOT] = (10, 199)
    lms = np.stack([same, line, two, dup.astype(np.float32), edges.astype(np.float32)])
    return lms, np.tile(np.array([[5, 5, 5]], np.int32), (5, 1))


@functools.lru_cache(None)
def large_hull():
    """106 points on a parabola, the ten eye points on their eyebrow partners so that the expansion moves nothing:
    96 distinct points in strictly convex position.  One face per regime."""
    x = 3.0 * np.arange(106) - 150
    p = np.stack([x, x * x], 1)
    p[BOT] = p[TOP]
    return np.tile(p.astype(np.float32), (4, 1, 1)), np.array(REGIMES, np.int32)


@functools.lru_cache(None)
def far_points():
    """Coordinates up to +-1e6 (the cross products pass 2^31 by many bits), the four regimes twice."""
    g = np.random.Generator(np.random.PCG64(31))
    lms = g.uniform(-1e6, 1e6, (8, 106, 2))
    lms[4:] = np.round(lms[4:] / 50000) * 50000 + g.integers(-2, 3, (4, 106, 2))    # collinear and equal points too
    return lms.astype(np.float32), np.array(REGIMES * 2, np.int32)


def all_sets():
    c = contraction()
    return {"face_like": face_like(), "contraction": (c[0], c[1]), "degenerate": degenerate(),
            "large_hull": large_hull(), "far_points": far_points()}
