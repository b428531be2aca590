"""Polygons, parameter rows and oracle stages shared by tests/test_mask_raster_cpu.py and tests/test_mask_raster_gpu.py
(no GPU; built once per process).

The cases are polygons given directly as int32 [F,128,2] / nv (what ghost_face_masks reads), not landmarks, so that
a test controls every vertex.  ``frames(H, W)`` gives one launch's worth for a shape; ``stages`` is the oracle
(oracle/mask_ref.py) stage by stage: the fill, the erode / dilate with the fade, the row pass, the unrounded blur and
the final mask / 255.
"""
import functools
from typing import NamedTuple

import numpy as np

from oracle import mask_ref as M

MAX_V = 128
SMALL_SHAPES = [(64, 48), (37, 53)]          # odd, H != W, smaller than the largest blur radius (126)
LARGE_SHAPES = [(224, 256), (256, 224)]      # H * W == kMaxHW; H == kMaxRows
SHAPES = LARGE_SHAPES + SMALL_SHAPES
PARAMS = [[15, 15, 10], [10, 10, 8], [-5, 5, 10], [5, 5, 5],     # face_mask_static's four regimes
          [3, 1, 1], [-4, 2, 3],                                  # 7 taps; an even dilate
          [1, 42, 1], [2, 1, 42]]                                 # 253 taps, the most accepted, on one axis each
TIE_MARGIN = 1e-3      # a pixel whose unrounded blur is nearer than this to k + 0.5 may round either way
TIE_SHARE = 0.02       # the most such pixels a case may have


class Stages(NamedTuple):
    raw: np.ndarray          # uint8 [H,W] after fill_convex_poly
    u8: np.ndarray           # uint8 [H,W] after box_morph and the border fade
    blur_float: np.ndarray   # float32 [H,W] after both blur passes, before rounding
    final: np.ndarray        # float32 [H,W] rounded / 255
    row: np.ndarray          # float32 [H,W] after the row pass


def ellipse(cx, cy, rx, ry, n):
    """The convex hull of n integer points on an ellipse."""
    t = 2 * np.pi * np.arange(n) / n
    pts = np.stack([np.rint(cx + rx * np.cos(t)), np.rint(cy + ry * np.sin(t))], 1).astype(np.int64)
    return M.convex_hull(pts)


@functools.lru_cache(None)
def _large_hull():
    """One hull of at least 90 vertices: mask_poly_cases.large_hull() through the host polygon builder."""
    import mask_poly_cases
    from ghost_amd.inference.masks import mask_polygons
    lms, params = mask_poly_cases.large_hull()
    poly, nv = mask_polygons(lms[:1], params[:1])
    assert nv[0] >= 90
    return poly[0, :nv[0]].astype(np.int64)


@functools.lru_cache(None)
def polygons(H, W):
    """name -> int64 [n,2] vertices (x, y), in the order the kernel and the oracle are both given."""
    inside = ellipse(0.5 * W, 0.5 * H, 0.3 * W, 0.35 * H, 40)
    return {
        "inside": inside,
        "right_bottom": ellipse(0.9 * W, 0.85 * H, 0.4 * W, 0.4 * H, 40),
        "left_top": ellipse(0.05 * W, 0.1 * H, 0.4 * W, 0.4 * H, 40),
        "cover": np.array([(-30, -20), (W + 25, -10), (W + 40, H + 30), (-15, H + 20)], np.int64),
        "rect": np.array([(W // 4, H // 4), (3 * W // 4, H // 4), (3 * W // 4, 3 * H // 4), (W // 4, 3 * H // 4)],
                         np.int64),
        "outside": ellipse(-3 * W, -2 * H, 0.4 * W, 0.4 * H, 40),
        "point": np.array([(W // 2, H // 2)], np.int64),
        "segment": np.array([(2, 3), (W + 9, H - 4)], np.int64),
        "apex_above": np.array([(W // 2, -3 * H), (W - 2, H - 2), (1, H - 3)], np.int64),
        "sliver": np.array([(W // 3, -5), (W // 3 + 1, H + 5), (W // 3 + 2, -5)], np.int64),
        "wide": ellipse(0.5 * W, 0.5 * H, 2.5 * W, 0.2 * H, 60),
        "large_hull": _large_hull(),
        "inside_rotated": np.roll(inside, 7, axis=0),
        "inside_reversed": inside[::-1].copy(),
    }


@functools.lru_cache(None)
def raster(H, W, name):
    img = np.zeros((H, W), np.uint8)
    M.fill_convex_poly(img, polygons(H, W)[name], 255)
    img.setflags(write=False)
    return img


@functools.lru_cache(None)
def _morph(H, W, name, erode):
    return M.box_morph(raster(H, W, name), abs(erode), dilate=erode <= 0)


@functools.lru_cache(None)
def stages(H, W, name, params):
    """The oracle's stages of polygon ``name`` under ``params`` (a tuple), the fade as face_mask_static writes it."""
    erode, sx, sy = params
    m = _morph(H, W, name, erode).copy()
    c = sy * 2
    m[:c, :] = 0
    m[-c:, :] = 0
    m[:, :c] = 0
    m[:, -c:] = 0
    row, blur = M.gaussian_blur_planes(m, sx, sy)
    final = (M.round_u8(blur).astype(np.float64) / 255).astype(np.float32)
    for a in (m, row, blur, final):
        a.setflags(write=False)
    return Stages(raster(H, W, name), m, blur, final, row)


@functools.lru_cache(None)
def combos(H, W):
    """The (polygon, parameter row) pairs of a shape, in frame order: the full cross product at every shape (the
    oracle needs about 2 s for a large shape's 112 frames), the parameter row changing from each frame to the next."""
    return [(n, tuple(p)) for n in polygons(H, W) for p in PARAMS]


def pack(polys):
    """A list of [n,2] vertex arrays -> (poly int32 [F,128,2], nv int32 [F])."""
    poly = np.zeros((len(polys), MAX_V, 2), np.int32)
    nv = np.zeros(len(polys), np.int32)
    for f, p in enumerate(polys):
        nv[f] = len(p)
        poly[f, :len(p)] = p
    return poly, nv


@functools.lru_cache(None)
def frames(H, W):
    """One launch for a shape: (labels, poly int32 [F,128,2], nv int32 [F], params int32 [F,3], [Stages] * F)."""
    cs = combos(H, W)
    poly, nv = pack([polygons(H, W)[n] for n, _ in cs])
    labels = [f"{H}x{W} {n} {list(p)}" for n, p in cs]
    return labels, poly, nv, np.array([p for _, p in cs], np.int32), [stages(H, W, n, p) for n, p in cs]


def near_tie(blur_float):
    """Pixels whose unrounded blur lies within TIE_MARGIN of a rounding tie."""
    b = blur_float.astype(np.float64)
    return np.abs(b - np.floor(b) - 0.5) < TIE_MARGIN
