"""The cases of tests/mask_raster_cases.py are what they claim (no GPU): each polygon reaches the branch of the fill it
is named for, decided on the oracle (oracle/mask_ref.py) and on checks independent of it, and few enough pixels of
every case lie near a rounding tie for tests/test_mask_raster_gpu.py to compare the rest bit for bit.  A case that
stops meeting its claim fails here.  Also the host wrapper's refusal of parameters the device has no blur for.
"""
import numpy as np
import pytest

import mask_raster_cases as cases
from oracle import mask_ref as M


def _edges(pts):
    """(x1, y1, x2, y2) of every edge v[i-1] -> v[i], as FillConvexPoly draws them."""
    return [(*map(int, pts[i - 1]), *map(int, pts[i])) for i in range(len(pts))]


def _codes(H, W, pts):
    return [(M.outcode(W, H, e[0], e[1]), M.outcode(W, H, e[2], e[3])) for e in _edges(pts)]


def _clipped(H, W, pts, bit):
    """The edges with exactly one end outside in direction ``bit`` and the other inside, after clip_line."""
    out = []
    for e, (c1, c2) in zip(_edges(pts), _codes(H, W, pts)):
        if {c1, c2} == {0, bit}:
            out.append(M.clip_line(W, H, *e))
    return out


@pytest.mark.parametrize("H,W", cases.SHAPES)
def test_cover_and_outside(H, W):
    assert (cases.raster(H, W, "cover") == 255).all()
    assert not cases.raster(H, W, "outside").any()
    seen = 0
    for c1, c2 in _codes(H, W, cases.polygons(H, W)["cover"]):
        assert c1 & c2, "an edge of cover would be drawn"          # every pixel comes from the scanline fill
        seen |= c1 | c2
    assert seen == 15                                               # left, right, above and below all occur
    assert all(c1 & c2 for c1, c2 in _codes(H, W, cases.polygons(H, W)["outside"]))
    # n < 3: the edges are drawn, nothing is filled
    p = cases.raster(H, W, "point")
    assert p.sum() == 255 and p[H // 2, W // 2] == 255
    s = cases.raster(H, W, "segment")
    ok, x1, y1, x2, y2 = M.clip_line(W, H, 2, 3, W + 9, H - 4)
    assert ok and s[y1, x1] == 255 and s[y2, x2] == 255            # 8-connected: one pixel per step of the long axis
    assert (s > 0).sum() == max(x2 - x1, y2 - y1) + 1


@pytest.mark.parametrize("H,W", cases.SHAPES)
def test_clip_branches(H, W):
    """Each named case has edges that clipLine shortens on the border it is named for (and none it is not)."""
    right, bottom = W - 1, H - 1
    P = cases.polygons(H, W)
    flat = [c for cc in _codes(H, W, P["right_bottom"]) for c in cc]
    assert all(c & 5 == 0 for c in flat) and any(c == 10 for c in flat)      # a vertex beyond the corner as well
    r, b = _clipped(H, W, P["right_bottom"], 2), _clipped(H, W, P["right_bottom"], 8)
    assert r and all(ok and right in (x1, x2) for ok, x1, y1, x2, y2 in r)
    assert b and all(ok and bottom in (y1, y2) for ok, x1, y1, x2, y2 in b)
    flat = [c for cc in _codes(H, W, P["left_top"]) for c in cc]
    assert all(c & 10 == 0 for c in flat) and any(c == 5 for c in flat)
    le, t = _clipped(H, W, P["left_top"], 1), _clipped(H, W, P["left_top"], 4)
    assert le and all(ok and 0 in (x1, x2) for ok, x1, y1, x2, y2 in le)
    assert t and all(ok and 0 in (y1, y2) for ok, x1, y1, x2, y2 in t)
    # segment: one end inside, the other right of the image only: the second stage of clipLine
    assert sorted(_codes(H, W, P["segment"])[0]) == [0, 2]
    ok, x1, y1, x2, y2 = M.clip_line(W, H, 2, 3, W + 9, H - 4)
    assert ok and (x1, y1, x2) == (2, 3, right) and 3 < y2 < H - 4
    # apex_above: the apex above the image only, both its edges cut at y = 0 well inside the width
    apex = _clipped(H, W, P["apex_above"], 4)
    assert len(apex) == 2 and all(ok and 0 in (y1, y2) and 0 < min(x1, x2) and max(x1, x2) < right
                                  for ok, x1, y1, x2, y2 in apex)
    assert int(P["apex_above"][:, 1].min()) == -3 * H               # 3 H rows of the chain walk above the image
    # sliver: above and below, no more than 3 pixels wide
    assert sorted({c for cc in _codes(H, W, P["sliver"]) for c in cc}) == [4, 8]
    s = cases.raster(H, W, "sliver")
    assert s.any(axis=1).all() and (s > 0).sum(axis=1).max() <= 3
    # wide: vertices left and right of the image only, the top and the bottom edges crossing its whole width
    assert {c for cc in _codes(H, W, P["wide"]) for c in cc} - {0} == {1, 2}
    w = cases.raster(H, W, "wide")
    assert w[H // 2].all() and not w[0].any() and not w[H - 1].any()
    assert len(P["large_hull"]) >= 90


@pytest.mark.parametrize("H,W", cases.SHAPES)
def test_rect_is_the_slice(H, W):
    ref = np.zeros((H, W), np.uint8)
    ref[H // 4:3 * H // 4 + 1, W // 4:3 * W // 4 + 1] = 255
    assert np.array_equal(cases.raster(H, W, "rect"), ref)
    pts = cases.polygons(H, W)["rect"]
    assert (pts[:, 1] == pts[:, 1].min()).sum() == 2               # a horizontal top edge


@pytest.mark.parametrize("H,W", cases.SHAPES)
def test_inside_against_point_in_polygon(H, W):
    """Pixels more than 1 px inside every edge are set, pixels more than 1 px outside one are clear; the start
    vertex and the orientation do not matter."""
    pts = cases.polygons(H, W)["inside"].astype(np.float64)
    assert M.outcode(W, H, *map(int, pts.min(axis=0))) == 0 and M.outcode(W, H, *map(int, pts.max(axis=0))) == 0
    yy, xx = np.mgrid[:H, :W]
    n = len(pts)
    d = []
    for i in range(n):
        a, b = pts[i], pts[(i + 1) % n]
        d.append(((b[0] - a[0]) * (yy - a[1]) - (b[1] - a[1]) * (xx - a[0])) / np.hypot(*(b - a)))
    centre = np.array([s[H // 2, W // 2] for s in d])
    assert (centre > 0).all() or (centre < 0).all()
    inside = np.minimum.reduce([s * np.sign(c) for s, c in zip(d, centre)])
    img = cases.raster(H, W, "inside")
    assert (inside > 1.0).sum() > H * W // 8 and (inside < -1.0).sum() > H * W // 8
    assert (img[inside > 1.0] == 255).all() and (img[inside < -1.0] == 0).all()
    assert np.array_equal(cases.raster(H, W, "inside_rotated"), img)
    assert np.array_equal(cases.raster(H, W, "inside_reversed"), img)
    P = cases.polygons(H, W)
    assert not np.array_equal(P["inside_rotated"][0], P["inside"][0])
    assert np.array_equal(P["inside_reversed"][::-1], P["inside"])


@pytest.mark.parametrize("H,W", cases.SHAPES)
def test_near_tie_share(H, W):
    """At most 2 % of a case's pixels lie within 1e-3 of a rounding tie (measured on the oracle alone over every
    shape, polygon and parameter row: 0.88 % at the most); the GPU test may exclude only those from bit equality."""
    labels, poly, nv, params, st = cases.frames(H, W)
    assert len(labels) == len(cases.polygons(H, W)) * len(cases.PARAMS) == 112
    assert {tuple(p) for p in params.tolist()} == {tuple(p) for p in cases.PARAMS}
    assert (params[1:] != params[:-1]).any(axis=1).all()            # the row changes from every frame to the next
    worst = 0.0
    for label, p, s in zip(labels, params.tolist(), st):
        share = float(cases.near_tie(s.blur_float).mean())
        worst = max(worst, share)
        assert share <= cases.TIE_SHARE, (label, share)
        assert np.array_equal(s.final, (M.gaussian_blur(s.u8, p[1], p[2]) / 255.0).astype(np.float32)), label
    print(f"MASKFIG oracle {H}x{W}: {len(labels)} frames, largest near-tie share {worst:.4%}")


def test_stages_follow_face_mask_static():
    """The stage helper composes to oracle.face_mask_static: same hull, same fade, same rounding."""
    import mask_poly_cases
    lms, params = mask_poly_cases.face_like()
    H, W = 64, 48
    for f in (0, 2, 9):
        lm = lms[f] * np.float32(0.25)
        p = tuple(int(v) for v in params[f])
        want, _ = M.face_mask_static(H, W, lm, params=list(p))
        hull = M.convex_hull(M.expand_eyebrows(lm, M.eyebrow_mod(p[0])))
        img = np.zeros((H, W), np.uint8)
        M.fill_convex_poly(img, hull, 255)
        m = M.box_morph(img, abs(p[0]), dilate=p[0] <= 0)
        c = 2 * p[2]
        m[:c, :] = 0
        m[-c:, :] = 0
        m[:, :c] = 0
        m[:, -c:] = 0
        row, blur = M.gaussian_blur_planes(m, p[1], p[2])
        assert row.dtype == np.float32 and blur.dtype == np.float32
        assert np.array_equal((M.round_u8(blur).astype(np.float64) / 255).astype(np.float32), want)


@pytest.mark.parametrize("params", [[5, 0, 5], [5, 5, 0], [5, 0, 0], [0, 0, 0], [5, 43, 5], [5, 5, 43], [5, 50, 50],
                                    [5, -1, 5], [257, 5, 5], [-257, 5, 5]])
def test_wrapper_refuses_parameters_without_a_blur(params, monkeypatch):
    """face_masks and face_mask_static raise ValueError for a sigma outside 1..42 or |erode| > 256, before the native
    library or the device is touched (both are made to fail here)."""
    import torch

    from ghost_amd import _lib
    from ghost_amd.inference import masks

    def touched(*a, **k):
        raise AssertionError("the device or the native library was reached before the parameter check")
    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(torch.cuda, "current_device", touched)
    monkeypatch.setattr(torch.cuda, "device", touched)
    lm = np.zeros((106, 2), np.float32)
    with pytest.raises(ValueError):
        masks.face_masks(np.stack([lm, lm]), [[5, 5, 5], params], 64, 48)
    with pytest.raises(ValueError):
        masks.face_mask_static(np.zeros((64, 48, 3), np.uint8), lm, params=params)


def test_wrapper_accepts_every_case_row():
    from ghost_amd.inference.masks import check_params
    pr = check_params(cases.PARAMS + [[256, 1, 42], [-256, 42, 1]])
    assert pr.dtype == np.int32 and pr.shape == (len(cases.PARAMS) + 2, 3)
