"""The detector's single operators on an MI355X, each through its own C entry point.

  maxpool            [2,8,12,C] with every value negative (a zero padding would win): equal to F.max_pool2d
  upsample2x + add   3x2 -> 6x4: fp32 exact; 16-bit one rounding of the fp32 sum
  letterbox + stem   (96, 64) canvas of a 45 x 80 frame (new_h = 54: padding rows) and of an 80 x 45 frame (new_w = 36:
                     padding columns): the canvas bytes equal blend_ref.resize_linear_u8 + zeros, the stem is within the
                     project's fp32 bar 1e-3 of float64 (16-bit: half an ulp of the storage type on top)
  head               a level's cls / reg / kps convs as one fp32 conv 80 -> 30 on a 5 x 7 map (every border case), N = 2,
                     from each storage type: within the fp32 bar 1e-3 of float64 on the same stored input, fp32 outputs
  decode + NMS       synthetic maps fed directly: the kept anchor indices, their order and every float of det / kps are
                     bit-identical to the numpy float32 restatement (detector_ref.detect)

The scores of the exact cases are drawn without equal values among the candidates (the tie case aside), and every case
asserts on the restatement that no pair's overlap lies within 1e-6 of the NMS threshold: a seed that breaks either
fails, it does not skip.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detector_ref as R
from ghost_amd import _lib

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _lib.load()


def _stream():
    return _lib.stream_ptr(DEV)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("C_", [56, 4])
def test_maxpool_negative_values(lib, dt, C_):
    g = torch.Generator().manual_seed(5)
    x = (-torch.rand(2, 8, 12, C_, generator=g) - 0.25).to(dt)
    y = torch.empty(2, 4, 6, C_, dtype=dt, device=DEV)
    xd = x.to(DEV)
    _lib.check(lib.ghost_maxpool3x3s2_nhwc(_lib.gdtype(dt), xd.data_ptr(), 2, 8, 12, C_, y.data_ptr(), _stream()))
    want = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert float(want.max()) < 0 and torch.equal(y.cpu().float(), want)
    assert lib.ghost_maxpool3x3s2_nhwc(_lib.gdtype(dt), xd.data_ptr(), 2, 7, 12, C_, y.data_ptr(), _stream()) == -1
    assert lib.ghost_maxpool3x3s2_nhwc(_lib.gdtype(dt), xd.data_ptr(), 2, 8, 12, 6, y.data_ptr(), _stream()) == -1


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_upsample_add(lib, dt):
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 3, 2, 56, generator=g).to(dt)
    y = torch.randn(2, 6, 4, 56, generator=g).to(dt)
    yd = y.to(DEV)
    xd = x.to(DEV)
    _lib.check(lib.ghost_upsample2x_add_nhwc(_lib.gdtype(dt), xd.data_ptr(), 2, 3, 2, 56, yd.data_ptr(), _stream()))
    up = x.float().repeat_interleave(2, 1).repeat_interleave(2, 2)
    want = (y.float() + up).to(dt)                      # one rounding of the fp32 sum
    assert torch.equal(yd.cpu(), want)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("hw,seed", [((45, 80), 3), ((80, 45), 4)], ids=["pad_rows", "pad_cols"])
def test_letterbox_and_stem(lib, dt, hw, seed):
    det_size = (96, 64)
    frames = R.make_frames(2, hw[0], hw[1], seed)
    new_h, new_w, _ = R.geometry(hw[0], hw[1], det_size)
    assert (new_h, new_w) == ((54, 96) if hw == (45, 80) else (64, 36))
    fd = torch.from_numpy(frames).to(DEV)
    canvas = torch.full((2, 64, 96, 3), 7, dtype=torch.uint8, device=DEV)
    _lib.check(lib.ghost_det_letterbox_u8(fd.data_ptr(), hw[0] * hw[1] * 3, 2, hw[0], hw[1], new_h, new_w,
                                          canvas.data_ptr(), 64, 96, _stream()))
    want_canvas, _ = R.letterbox(frames, det_size)
    assert np.array_equal(canvas.cpu().numpy(), want_canvas)
    p = R.make_weights()
    w, b = p["backbone.stem.0.weight"], p["backbone.stem.0.bias"]
    wd = w.permute(2, 3, 1, 0).reshape(27, 28).contiguous().to(DEV)
    bd = b.to(DEV)
    y = torch.empty(2, 32, 48, 28, dtype=dt, device=DEV)
    _lib.check(lib.ghost_det_stem_u8(_lib.gdtype(dt), canvas.data_ptr(), 64 * 96 * 3, 1, 2, 64, 96, wd.data_ptr(),
                                     bd.data_ptr(), y.data_ptr(), _stream()))
    x = (torch.from_numpy(want_canvas).flip(-1).permute(0, 3, 1, 2).double() - 127.5) / 128.0
    assert float(x[0, 0, 63, 95]) == -0.99609375                        # the canvas padding is byte 0, not value 0
    want = F.relu(F.conv2d(x, w.double(), b.double(), stride=2, padding=1)).permute(0, 2, 3, 1)
    err = (y.cpu().double() - want).abs()
    # half an ulp relative to the value: 8 significand bits in bf16, 11 in fp16
    ulp_half = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dt]
    print(f"DETFIG stem {IDS[DTYPES.index(dt)]} {hw} max|d|={float(err.max()):.3e}")
    assert bool((err <= 1e-3 + ulp_half * want.abs()).all())


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_head(lib, dt):
    from ghost_amd.detection import pack
    p = R.make_weights()
    slots = {k: v.to(DEV) for k, v in pack.pack_detector(p, dt).items() if k.startswith("bbox_head.out.16")}
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 5, 7, 80, generator=g).to(dt)
    xd = x.to(DEV)
    cls = torch.empty(2, 5, 7, 2, device=DEV)
    reg = torch.empty(2, 5, 7, 8, device=DEV)
    kps = torch.empty(2, 5, 7, 20, device=DEV)
    _lib.check(lib.ghost_det_head_nhwc(_lib.gdtype(dt), xd.data_ptr(), 2, 5, 7, slots["bbox_head.out.16.w"].data_ptr(),
                                       slots["bbox_head.out.16.b"].data_ptr(), slots["bbox_head.out.16.m"].data_ptr(),
                                       cls.data_ptr(), reg.data_ptr(), kps.data_ptr(), _stream()))
    x64 = x.double().permute(0, 3, 1, 2)
    conv = lambda n: F.conv2d(x64, p[f"bbox_head.stride_{n}.16.weight"].double(), p[f"bbox_head.stride_{n}.16.bias"].double(),
                              padding=1).permute(0, 2, 3, 1)
    want = [torch.sigmoid(conv("cls")), conv("reg") * p["bbox_head.scales.1.scale"].double(), conv("kps")]
    for name, got, w in zip(("cls", "reg", "kps"), (cls, reg, kps), want):
        e = float((got.cpu().double() - w).abs().max())
        print(f"DETFIG head {IDS[DTYPES.index(dt)]} {name} max|d|={e:.3e}")
        assert e <= 1e-3, (name, e)


# ---- decode + NMS ----

def synth_maps(F_, det_size, clusters, seed, degenerate=0, thresh=0.5):
    """Nine NCHW float32 maps: background scores below thresh; per frame ``clusters[f]`` clusters of 3-6 neighbouring
    anchors above it with well-formed, strongly overlapping boxes; ``degenerate`` extra candidates per frame with
    x2 < x1.  Candidate scores are distinct."""
    Wd, Hd = det_size
    g = np.random.Generator(np.random.PCG64(seed))
    maps = []
    for ch in (2, 8, 20):
        for s in R.STRIDES:
            Hl, Wl = Hd // s, Wd // s
            if ch == 2:
                maps.append(g.uniform(0.01, 0.3, (F_, 2, Hl, Wl)).astype(np.float32))
            elif ch == 8:
                maps.append(g.uniform(1.0, 3.0, (F_, 8, Hl, Wl)).astype(np.float32))
            else:
                maps.append(g.uniform(-2.0, 2.0, (F_, 20, Hl, Wl)).astype(np.float32))
    for f in range(F_):
        for c in range(clusters[f]):
            l = (c + f) % 3
            Hl, Wl = maps[l].shape[2:]
            y, x = int(g.integers(0, Hl)), int(g.integers(0, Wl))
            for _ in range(int(g.integers(3, 7))):
                yy = min(Hl - 1, max(0, y + int(g.integers(-1, 2))))
                xx = min(Wl - 1, max(0, x + int(g.integers(-1, 2))))
                maps[l][f, int(g.integers(0, 2)), yy, xx] = g.uniform(thresh + 0.01, 0.99)
        for _ in range(degenerate):
            l = int(g.integers(0, 3))
            Hl, Wl = maps[l].shape[2:]
            a, yy, xx = int(g.integers(0, 2)), int(g.integers(0, Hl)), int(g.integers(0, Wl))
            maps[l][f, a, yy, xx] = g.uniform(thresh + 0.01, 0.99)
            maps[3 + l][f, a * 4:a * 4 + 4, yy, xx] = [-2.0, 1.0, -1.5, 1.0]        # x2 < x1
    return maps


def run_op(lib, maps, det_size, thresh, det_scale, cap=4096, max_faces=256):
    F_ = maps[0].shape[0]
    Wd, Hd = det_size
    dev = [torch.from_numpy(np.ascontiguousarray(m.transpose(0, 2, 3, 1))).to(DEV) for m in maps]
    arr = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
    det = torch.full((F_, max_faces, 5), 7.0, device=DEV)
    kps = torch.full((F_, max_faces, 5, 2), 7.0, device=DEV)
    anchor = torch.full((F_, max_faces), 7, dtype=torch.int32, device=DEV)
    count = torch.full((F_, 2), 7, dtype=torch.int32, device=DEV)
    nb = lib.ghost_det_decode_workspace_bytes(F_, cap)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.check(lib.ghost_det_decode_nms(arr(dev[:3]), arr(dev[3:6]), arr(dev[6:]), F_, Hd, Wd, thresh, det_scale,
                                        R.NMS_THRESH, cap, max_faces, det.data_ptr(), kps.data_ptr(), anchor.data_ptr(),
                                        count.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "decode_nms")
    torch.cuda.synchronize()
    return det.cpu().numpy(), kps.cpu().numpy(), anchor.cpu().numpy(), count.cpu().numpy()


def check_against_restatement(lib, maps, det_size, thresh, det_scale, cap=4096, max_faces=256, distinct=True):
    det, kps, anchor, count = run_op(lib, maps, det_size, thresh, det_scale, cap, max_faces)
    stats = []
    for f in range(maps[0].shape[0]):
        fm = R.frame_maps(maps, f)
        sc, box, _, _ = R.decode(fm, det_size, thresh, det_scale)
        sc, box = sc[:cap], box[:cap]
        if distinct:
            assert len(np.unique(sc)) == len(sc), "equal scores among the candidates: change the seed"
        assert R.min_ovr_margin(np.concatenate([box, sc[:, None]], axis=1)) > 1e-6, "an overlap at the threshold"
        d, k, a, n = R.detect(fm, det_size, thresh, det_scale, cap)
        assert count[f].tolist() == [len(a), n], (f, count[f], len(a), n)
        m = min(len(a), max_faces)
        assert anchor[f, :m].tolist() == a[:m].tolist(), f
        assert np.array_equal(det[f, :m].view(np.uint32), d[:m].view(np.uint32)), f            # every bit
        assert np.array_equal(kps[f, :m].view(np.uint32), k[:m].view(np.uint32)), f
        assert not det[f, m:].any() and not kps[f, m:].any() and bool((anchor[f, m:] == -1).all())
        stats.append((n, len(a)))
    return stats


def test_decode_no_candidate(lib):
    maps = synth_maps(2, (96, 64), [0, 0], 21)
    assert check_against_restatement(lib, maps, (96, 64), 0.5, 1.2) == [(0, 0), (0, 0)]


def test_decode_clusters_over_three_levels(lib):
    maps = synth_maps(2, (96, 64), [5, 7], 22)
    stats = check_against_restatement(lib, maps, (96, 64), 0.5, 1.2)
    assert all(n > k > 0 for n, k in stats)                  # something was suppressed, something kept
    stats = check_against_restatement(lib, maps, (96, 64), 0.5, 1.0 / 3.0)
    assert all(n > k > 0 for n, k in stats)


def test_decode_degenerate_boxes(lib):
    maps = synth_maps(1, (96, 64), [4], 23, degenerate=5)
    n, k = check_against_restatement(lib, maps, (96, 64), 0.5, 0.8)[0]
    assert n > k >= 5


def test_decode_640_multi_round_scan_and_large_sort(lib):
    maps = synth_maps(1, (640, 640), [70], 24)
    n, k = check_against_restatement(lib, maps, (640, 640), 0.5, 1.0 / 3.0)[0]
    print(f"DETFIG decode 640: {n} candidates, {k} kept")
    assert 256 < n <= 4096 and n > k > 30


def test_decode_tie_rule(lib):
    maps = synth_maps(1, (96, 64), [0], 25)
    # four candidates with one score on three levels, far apart, and one pair of equal scores that overlap: the lower
    # anchor index is kept
    for l, (a, y, x) in enumerate([(1, 2, 3), (0, 1, 4), (1, 1, 1)]):
        maps[l][0, a, y, x] = 0.75
    maps[0][0, 0, 6, 9] = 0.75
    maps[0][0, 0, 5, 2] = 0.625
    maps[0][0, 1, 5, 2] = 0.625                               # the same centre: overlaps anchor 0 of the pixel
    for c in range(4):
        maps[3][0, c, 5, 2] = 2.0
        maps[3][0, 4 + c, 5, 2] = 2.0
    det, kps, anchor, count = run_op(lib, maps, (96, 64), 0.5, 1.0)
    check_against_restatement(lib, maps, (96, 64), 0.5, 1.0, distinct=False)
    n8, n16 = 2 * 8 * 12, 2 * 4 * 6
    want = sorted([(2 * 12 + 3) * 2 + 1, (6 * 12 + 9) * 2, n8 + (1 * 6 + 4) * 2, n8 + n16 + (1 * 3 + 1) * 2 + 1])
    assert count[0].tolist() == [5, 6]
    assert anchor[0, :5].tolist() == want + [(5 * 12 + 2) * 2]


def test_decode_capacity(lib):
    maps = synth_maps(1, (96, 64), [0], 26)
    g = np.random.Generator(np.random.PCG64(27))
    flat = g.permutation(2 * 8 * 12)[:100]                     # 100 candidates on the stride-8 level
    vals = g.permutation(np.linspace(0.51, 0.98, 100)).astype(np.float32)
    for i, v in zip(flat, vals):
        a, pix = int(i) % 2, int(i) // 2
        maps[0][0, a, pix // 12, pix % 12] = v
    det, kps, anchor, count = run_op(lib, maps, (96, 64), 0.5, 1.2, cap=64)
    assert count[0, 1] == 100
    first64 = np.sort(flat)[:64]
    assert set(anchor[0, :count[0, 0]].tolist()) <= set(first64.tolist())
    check_against_restatement(lib, maps, (96, 64), 0.5, 1.2, cap=64)
    assert lib.ghost_det_decode_workspace_bytes(1, 100) == -1 and lib.ghost_det_decode_workspace_bytes(1, 8192) == -1


def test_decode_max_faces_overflow(lib):
    maps = synth_maps(1, (96, 64), [8], 28)
    n, k = check_against_restatement(lib, maps, (96, 64), 0.5, 1.2, max_faces=4)[0]
    assert k > 4


def test_decode_three_frames_different_counts(lib):
    maps = synth_maps(3, (96, 64), [6, 0, 2], 29)
    stats = check_against_restatement(lib, maps, (96, 64), 0.5, 0.8)
    assert stats[1] == (0, 0) and stats[0][0] > stats[2][0] > 0
