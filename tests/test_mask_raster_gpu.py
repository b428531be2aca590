"""ghost_face_masks (ghost_amd/csrc/masks.hip) on an MI355X against the oracle stage by stage, through the raw ABI.

One launch per shape carries every polygon of tests/mask_raster_cases.py under every parameter row (the row changes
from each frame to the next).  Per frame, with the case named in the message:
* raster, erode / dilate and fade: the uint8 mask the call leaves at the start of the workspace equals the oracle's,
  every byte;
* row pass: the fp32 plane behind it is within 1e-4 of the oracle's.  Same arithmetic order on both sides and no FMA;
  only the taps can differ, by one float ulp each from the device's double exp, so a pass differs by at most
  255 * 2^-23 = 3e-5;
* final mask: every pixel whose unrounded oracle value is at least 1e-3 (15 times the 6e-5 of two passes) from a
  rounding tie equals the oracle's q / 255 bit for bit, the others differ by at most 1 / 255;
  tests/test_mask_raster_cpu.py caps those others at 2 % of a case;
* no NaN; the 24 words between two frames' masks (mask_stride = H*W + 24) keep their sentinel.
The tests print one MASKFIG line per launch.  Measured on an MI355X (112 frames a shape):
  224x256: 2205 pixels excluded near a tie, 7 pixels differ, row pass max|d| = 3.05e-05
  256x224: 1962 excluded, 2 differ, 3.05e-05;  64x48: 225 excluded, 0 differ, 1.53e-05;  37x53: 121, 0, 1.53e-05
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mask_raster_cases as cases

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GAP = 24
SENTINEL = np.float32(-12345.678)
EINVAL, ENOWS = -1, -3
ROW_TOL = 1e-4


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Launch:
    """The buffers of one ghost_face_masks call: the workspace filled with 0xFF bytes, the output [F, H*W + 24]
    filled with the sentinel."""

    def __init__(self, poly, nv, params, H, W):
        from ghost_amd import _lib
        self.lib = _lib.load()
        self.F, self.H, self.W = len(nv), H, W
        self.poly, self.nv, self.params = _dev(poly), _dev(nv), _dev(params)
        self.stride = H * W + GAP
        self.need = int(self.lib.ghost_face_masks_workspace_bytes(self.F, H, W))
        self.ws = torch.full((self.need,), 0xFF, dtype=torch.uint8, device=DEV)
        self.out = torch.full((self.F, self.stride), float(SENTINEL), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()

    def call(self, **over):
        a = dict(poly=self.poly.data_ptr(), nv=self.nv.data_ptr(), params=self.params.data_ptr(), F=self.F, H=self.H,
                 W=self.W, out=self.out.data_ptr(), stride=self.stride, ws=self.ws.data_ptr(), ws_bytes=self.need)
        a.update(over)
        rc = self.lib.ghost_face_masks(a["poly"], a["nv"], a["params"], a["F"], a["H"], a["W"], a["out"], a["stride"],
                                       a["ws"], a["ws_bytes"], torch.cuda.current_stream(DEV).cuda_stream)
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        out = self.out.cpu().numpy()
        return bool((self.ws.cpu().numpy() == 0xFF).all()) and \
            bool((out.view(np.int32) == SENTINEL.view(np.int32)).all())

    def results(self):
        """(u8 [F,H,W], row plane float32 [F,H,W], masks float32 [F,H,W], gap words int32 [F,24])."""
        F, H, W = self.F, self.H, self.W
        ws = self.ws.cpu().numpy()
        base = self.ws.data_ptr()
        off = ((base + F * H * W + 255) & ~255) - base
        u8 = ws[:F * H * W].reshape(F, H, W)
        row = ws[off:off + 4 * F * H * W].view(np.float32).reshape(F, H, W)
        out = self.out.cpu().numpy()
        return u8, row, out[:, :H * W].reshape(F, H, W), out[:, H * W:].view(np.int32)


def _check_frames(tag, labels, st, u8, row, got, gap, skip=()):
    """The stage assertions for every frame not in ``skip``; prints the MASKFIG line and returns its counts."""
    excluded = differ = 0
    row_err = 0.0
    assert (gap == SENTINEL.view(np.int32)).all(), f"{tag}: a gap word between two masks was written"
    assert not np.isnan(got).any() and not np.isnan(row).any(), f"{tag}: NaN"
    for f, (label, s) in enumerate(zip(labels, st)):
        if f in skip:
            continue
        bad = np.argwhere(u8[f] != s.u8)
        assert not len(bad), f"{label}: raster / erode / fade differs at {len(bad)} bytes, first (y, x) = " \
                             f"{bad[0].tolist()}: {u8[f][tuple(bad[0])]} for {s.u8[tuple(bad[0])]}"
        e = float(np.abs(row[f].astype(np.float64) - s.row).max())
        row_err = max(row_err, e)
        assert e <= ROW_TOL, f"{label}: row pass max|d| = {e:.3e}"
        tie = cases.near_tie(s.blur_float)
        ne = got[f].view(np.int32) != s.final.view(np.int32)
        excluded += int(tie.sum())
        differ += int(ne.sum())
        bad = np.argwhere(ne & ~tie)
        assert not len(bad), f"{label}: final mask differs at {len(bad)} pixels away from a tie, first (y, x) = " \
                             f"{bad[0].tolist()}: {got[f][tuple(bad[0])]!r} for {s.final[tuple(bad[0])]!r}"
        d = float(np.abs(got[f].astype(np.float64) - s.final).max())
        assert d <= 1.0 / 255 + 1e-7, f"{label}: a pixel near a tie differs by {d:.3e}"
    n = len(labels) - len(skip)
    print(f"MASKFIG {tag}: {n} frames, {excluded} pixels excluded near a tie, {differ} pixels differ, "
          f"row pass max|d| = {row_err:.2e}")
    return excluded, differ


@pytest.mark.parametrize("H,W", cases.SHAPES)
def test_stages_match_oracle(H, W):
    labels, poly, nv, params, st = cases.frames(H, W)
    la = Launch(poly, nv, params, H, W)
    assert la.call() == 0
    _check_frames(f"{H}x{W}", labels, st, *la.results())


def test_sigma_without_a_blur_gives_zero_mask():
    """sigma 0 (NaN taps before the guard) and sigma 43 (more taps than the kernel holds) on either axis: exactly
    zero masks, never NaN, and the frames between them unharmed."""
    H, W = 64, 48
    pts = cases.polygons(H, W)["inside"]
    rows = [(5, 5, 5), (5, 0, 0), (3, 1, 1), (5, 43, 5), (-4, 2, 3), (5, 5, 43), (10, 10, 8)]
    zero = (1, 3, 5)
    poly, nv = cases.pack([pts] * len(rows))
    labels = [f"{H}x{W} inside {list(r)}" for r in rows]
    st = [None if f in zero else cases.stages(H, W, "inside", r) for f, r in enumerate(rows)]
    la = Launch(poly, nv, np.array(rows, np.int32), H, W)
    assert la.call() == 0
    u8, row, got, gap = la.results()
    for f in zero:
        assert not np.isnan(got[f]).any(), f"{labels[f]}: NaN"
        assert (got[f].view(np.int32) == 0).all(), f"{labels[f]}: {int((got[f] != 0).sum())} pixels are not zero"
    _check_frames(f"{H}x{W} sigma 0 / 43 between", labels, st, u8, row, got, gap, skip=zero)
    assert all(float(st[f].final.max()) > 0.5 for f in range(len(rows)) if f not in zero)   # the neighbours are masks


@pytest.mark.parametrize("over,rc", [
    (dict(H=225, W=256), EINVAL),                    # H * W one row over the LDS plane
    (dict(H=257, W=100), EINVAL),                    # H over the row table
    (dict(stride=64 * 48 - 1), EINVAL),              # frames would overlap
    (dict(ws_bytes=-1), ENOWS),                      # (relative to the need) one byte short
    (dict(poly=None), EINVAL), (dict(nv=None), EINVAL), (dict(params=None), EINVAL), (dict(out=None), EINVAL),
    (dict(ws=None), EINVAL)],
    ids=["HW=225x256", "H=257", "stride=HW-1", "ws-1", "poly=NULL", "nv=NULL", "params=NULL", "out=NULL", "ws=NULL"])
def test_refusals(over, rc):
    """Every refusal returns its code and leaves the output and the workspace as they were.  The buffers are sized
    for the largest shape asked for, so a call that was not refused would still stay inside them."""
    H, W = 64, 48
    poly, nv = cases.pack([cases.polygons(H, W)["inside"]])
    big = Launch(poly, nv, np.array([[5, 5, 5]], np.int32), 257, 256)      # room for 225 x 256 and 257 x 100
    big.H, big.W, big.stride = H, W, H * W + GAP
    need = int(big.lib.ghost_face_masks_workspace_bytes(1, over.get("H", H), over.get("W", W)))
    over = dict(over)
    over["ws_bytes"] = need + over.get("ws_bytes", 0)
    if "H" in over:
        over["stride"] = over["H"] * over["W"] + GAP
    assert big.call(**over) == rc
    assert b"ghost_face_masks" in big.lib.ghost_last_error()
    assert big.untouched()
