"""Host-side checks of ghost_amd.detection (no GPU): the graph table against the restatement's recorded spec list
(tests/golden/detector_scrfd.npz), the restatement against its recorded outputs, fold_bn, the slot pack, the letterbox
geometry, the host max_num rule, the restatement's NMS with its tie rule, and the dry-run plan of the runtime.

The graph and SCRFD.detect's arithmetic are recalled from the public sources, not verified: the
fixture pins the restatement against drift and nothing more.

The weight recipe (detector_ref.make_weights) was re-checked with the final names at det_size (96, 64) in float64:
|reg| <= 1.6, |kps| <= 2.3, scores spread over 0.38 - 0.78, 53 - 61 of the 252 anchors at or above 0.6 per image;
test_weight_recipe_keeps_outputs_moderate holds it to O(1) outputs and unsaturated scores.  (The plain sqrt(2 / fan_in)
everywhere drives the head outputs to +-800 and every score to 0 or 1.)
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import detector_ref as R
from ghost_amd import _lib
from ghost_amd.detection import SCRFD, Face_detect_crop, fold_bn, letterbox_geometry, pack, select_max_num

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detector_scrfd.npz")
DET_SIZE = (96, 64)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def weights():
    return R.make_weights()


@pytest.fixture(scope="module")
def ref_maps(weights):
    canvas, scale = R.letterbox(R.make_frames(2, 45, 80, R.E2E_SEED_45x80), DET_SIZE)
    return R.forward(weights, canvas, dtype=torch.float64)[0], scale


def test_table_matches_recorded_specs(golden):
    names = golden["spec_names"].tolist()
    shapes = [tuple(int(v) for v in s if v) for s in golden["spec_shapes"]]
    assert [(n, tuple(s)) for n, s in pack.param_specs()] == list(zip(names, shapes))
    assert [(n, tuple(s)) for n, s in R.param_specs()] == list(zip(names, shapes))
    # 58 conv units: 3 stem + 24 block + 3 avg-down + 10 PAFPN + 18 head
    assert len(pack.units()) == 58 and len(names) == 2 * 58 + 3
    sd = SCRFD().state_dict()
    assert sorted(sd) == sorted(names)          # state_dict groups by container, the table is in graph order
    for n, s in zip(names, shapes):
        assert tuple(sd[n].shape) == s, n


def test_restatement_matches_recorded_outputs(golden, ref_maps):
    maps, scale = ref_maps
    for i, m in enumerate(maps):
        assert float((m - torch.from_numpy(golden[f"map_{i}"]).double()).abs().max()) <= 2e-6, i
    scores = np.concatenate([m.numpy().reshape(2, -1) for m in maps[:3]], axis=1)
    thresh, gap = R.gap_threshold(scores)
    assert thresh == float(golden["e2e_thresh"]) and gap >= 4e-3
    dets, kpss, anchors, counts = [], [], [], []
    for f in range(2):
        d, k, a, n = R.detect(R.frame_maps(maps, f), DET_SIZE, thresh, scale)
        dets.append(d); kpss.append(k); anchors.append(a); counts.append([len(a), n])
    assert np.array_equal(np.concatenate(anchors), golden["e2e_anchor"])
    assert np.array_equal(np.array(counts), golden["e2e_count"])
    assert np.array_equal(np.concatenate(dets), golden["e2e_det"])
    assert np.array_equal(np.concatenate(kpss), golden["e2e_kps"])


def test_weight_recipe_keeps_outputs_moderate(ref_maps):
    maps, _ = ref_maps
    assert max(float(m.abs().max()) for m in maps[3:]) <= 5.0
    s = torch.cat([m.flatten() for m in maps[:3]])
    assert 0.05 < float(s.min()) and float(s.max()) < 0.95 and float(s.max() - s.min()) > 0.2
    # the storage emulation runs and moves the result
    canvas, _ = R.letterbox(R.make_frames(1, 45, 80, R.E2E_SEED_45x80), DET_SIZE)
    mh, _ = R.forward(R.make_weights(), canvas, dtype=torch.float32, store=torch.bfloat16)
    assert 0.0 < float((mh[0].double() - maps[0][:1]).abs().max()) < 0.1


def test_fold_bn():
    g = np.random.Generator(np.random.PCG64(3))
    w = g.normal(0, 1, (5, 4, 3, 3)).astype(np.float32)
    ga, be, mu = (g.normal(0, 1, 5).astype(np.float32) for _ in range(3))
    va = g.uniform(0.5, 2.0, 5).astype(np.float32)
    wf, bf = fold_bn(w, ga, be, mu, va)
    assert wf.dtype == np.float32 and bf.dtype == np.float32 and wf.shape == w.shape and bf.shape == (5,)
    s = ga.astype(np.float64) / np.sqrt(va.astype(np.float64) + 1e-5)
    assert np.array_equal(wf, (w.astype(np.float64) * s[:, None, None, None]).astype(np.float32))
    assert np.array_equal(bf, (be.astype(np.float64) - mu.astype(np.float64) * s).astype(np.float32))
    # the folded unit computes what conv + BatchNorm(eval) computes
    x = torch.from_numpy(g.normal(0, 1, (1, 4, 6, 6)))
    y = torch.nn.functional.conv2d(x, torch.from_numpy(w).double(), padding=1)
    y = (y - torch.from_numpy(mu).double().view(1, -1, 1, 1)) * torch.from_numpy(s).view(1, -1, 1, 1) + \
        torch.from_numpy(be).double().view(1, -1, 1, 1)
    yf = torch.nn.functional.conv2d(x, torch.from_numpy(wf).double(), torch.from_numpy(bf).double(), padding=1)
    assert float((y - yf).abs().max()) < 1e-5
    wf2, _ = fold_bn(torch.from_numpy(w), ga, be, mu, va, eps=1e-3)
    assert not np.array_equal(wf, wf2)


def test_pack_layouts(weights):
    s = pack.pack_detector(weights, torch.float32)
    assert sorted(s) == sorted(pack.slot_names())
    w = weights["backbone.stem.0.weight"]
    assert tuple(s["backbone.stem.0.w"].shape) == (27, 28)
    assert float(s["backbone.stem.0.w"][(1 * 3 + 2) * 3 + 0, 5]) == float(w[5, 0, 1, 2])
    # [Npad][Kpad], K = (ky*kw + kx)*Cin + c, zero padded
    w = weights["backbone.layer2.1.conv1.weight"]                       # 88 -> 88, 3x3
    p = s["backbone.layer2.1.conv1.w"]
    assert tuple(p.shape) == (128, 800) and float(p[17, (2 * 3 + 1) * 88 + 40]) == float(w[17, 40, 2, 1])
    assert float(p[88:].abs().max()) == 0.0 and float(p[:, 792:].abs().max()) == 0.0
    w = weights["bbox_head.cls_stride_convs.16.0.conv.weight"]           # 56 -> 80
    p = s["bbox_head.cls_stride_convs.16.0.conv.w"]
    assert tuple(p.shape) == (128, 512) and float(p[79, (0 * 3 + 2) * 56 + 55]) == float(w[79, 55, 0, 2])
    assert float(p[80:].abs().max()) == 0.0 and float(p[:, 504:].abs().max()) == 0.0
    # the three output convs of a level as one fp32 conv 80 -> 30: [720][30], columns cls | reg | kps
    p = s["bbox_head.out.16.w"]
    assert tuple(p.shape) == (720, 30) and p.dtype == torch.float32
    k = (1 * 3 + 2) * 80 + 33
    assert float(p[k, 1]) == float(weights["bbox_head.stride_cls.16.weight"][1, 33, 1, 2])
    assert float(p[k, 2 + 7]) == float(weights["bbox_head.stride_reg.16.weight"][7, 33, 1, 2])
    assert float(p[k, 10 + 19]) == float(weights["bbox_head.stride_kps.16.weight"][19, 33, 1, 2])
    # avg-down: AvgPool 2x2 then conv1x1 = conv 2x2/s2 with every tap w/4
    w = weights["backbone.layer3.0.downsample.1.weight"]
    p = s["backbone.layer3.0.downsample.1.w"]
    assert tuple(p.shape) == (128, 352)
    for tap in range(4):
        assert torch.equal(p[:88, tap * 88:(tap + 1) * 88], w[:, :, 0, 0] * 0.25)
    # Cin % 32 == 0 (the 224-channel units): pack_conv's blocked K order (channel block, tap, channel)
    w = weights["backbone.layer4.1.conv1.weight"]
    p = s["backbone.layer4.1.conv1.w"]
    assert tuple(p.shape) == (256, 2016) and float(p[3, (2 * 9 + 4) * 32 + 7]) == float(w[3, 2 * 32 + 7, 1, 1])
    # their biases, and bbox_scale as the multiplier of the reg columns only
    sc = weights["bbox_head.scales.0.scale"]
    m = s["bbox_head.out.8.m"]
    assert tuple(m.shape) == (32,) and torch.equal(m[2:10], sc.expand(8)) and torch.equal(m[:2], torch.ones(2)) and \
        torch.equal(m[10:], torch.ones(22))
    b = s["bbox_head.out.8.b"]
    assert torch.equal(b[2:10], weights["bbox_head.stride_reg.8.bias"]) and torch.equal(
        b[10:30], weights["bbox_head.stride_kps.8.bias"]) and float(b[30:].abs().max()) == 0
    assert torch.equal(s["neck.fpn_convs.1.conv.b"][:56], weights["neck.fpn_convs.1.conv.bias"])
    h = pack.pack_detector(weights, torch.bfloat16)
    assert h["backbone.stem.0.w"].dtype == torch.float32 and h["backbone.stem.3.w"].dtype == torch.bfloat16
    assert h["bbox_head.out.32.w"].dtype == torch.float32
    assert all(h[n].dtype == torch.float32 for n in h if n.endswith((".b", ".m")))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_pack_binds_every_declared_slot(weights, dt):
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.ghost_det_create(_lib.gdtype(dt), 96, 64, C.byref(h)), "create")
    try:
        slots = pack.pack_detector(weights, dt)
        assert lib.ghost_det_missing(h) == len(slots)
        assert lib.ghost_det_bind(h, b"no.such.slot", slots["backbone.stem.0.w"].data_ptr(), 1) == -1
        for name, t in slots.items():
            assert t.is_contiguous()
            _lib.check(lib.ghost_det_bind(h, name.encode(), t.data_ptr(), t.numel()), name)
        assert lib.ghost_det_missing(h) == 0
        assert lib.ghost_det_workspace_bytes(h, 0) > 0
        assert lib.ghost_det_workspace_bytes(h, 3) > lib.ghost_det_workspace_bytes(h, 1) > 64 * 96 * 3
        assert lib.ghost_det_forward_u8(h, None, 0, 0, 0, 0, 0, 0, None, None, 0, None) == 0     # F = 0
    finally:
        lib.ghost_det_destroy(h)
    bad = C.c_void_p()
    assert lib.ghost_det_create(_lib.U8, 96, 64, C.byref(bad)) == -1                           # not a storage type
    assert lib.ghost_det_create(_lib.gdtype(dt), 100, 64, C.byref(bad)) == -1                  # not a multiple of 32


class _Nd:
    def __init__(self, a):
        self.a = a

    def asnumpy(self):
        return self.a


def test_load_arrays(weights):
    net = SCRFD()
    names = list(weights)
    mixed = {k: (v if i % 3 == 0 else v.numpy() if i % 3 == 1 else _Nd(v.numpy())) for i, (k, v) in
             enumerate(weights.items())}
    net.load_arrays(mixed)
    for k, v in weights.items():
        assert torch.equal(net.state_dict()[k], v), k
    short = dict(weights)
    del short["neck.pafpn_convs.1.conv.bias"]
    with pytest.raises(KeyError, match="neck.pafpn_convs.1.conv.bias"):
        SCRFD().load_arrays(short)
    with pytest.raises(KeyError, match="bbox_head.stride_gn"):
        SCRFD().load_arrays(dict(weights, **{"bbox_head.stride_gn.weight": np.zeros(3)}))
    with pytest.raises(ValueError, match="backbone.stem.3.bias"):
        SCRFD().load_arrays(dict(weights, **{"backbone.stem.3.bias": np.zeros(3, np.float32)}))
    assert sorted(names) == sorted(SCRFD().state_dict())


@pytest.mark.parametrize("H,W,det_size,want", [
    (1080, 1920, (640, 640), (360, 640, 360 / 1080)),
    (1920, 1080, (640, 640), (640, 360, 640 / 1920)),
    (640, 640, (640, 640), (640, 640, 1.0)),
    (479, 641, (640, 640), (478, 640, 478 / 479)),
    (641, 479, (640, 640), (640, 478, 640 / 641)),
    (45, 80, (96, 64), (54, 96, 54 / 45)),
    (80, 45, (96, 64), (64, 36, 64 / 80)),
])
def test_letterbox_geometry(H, W, det_size, want):
    assert letterbox_geometry(H, W, det_size) == want
    assert R.geometry(H, W, det_size) == want


def test_max_num_selection():
    # centre (H // 2, W // 2) = (50, 100); rows: a large box far away, a small one at the centre, a medium one near it
    det = np.array([[150, 60, 190, 100, 0.9],      # area 1600, offset (70, 30): 1600 - 2 * 5800 = -10000
                    [95, 45, 105, 55, 0.8],        # area 100, offset 0: 100
                    [80, 30, 110, 60, 0.7],        # area 900, offset (-5, -5): 900 - 100 = 800
                    [0, 0, 20, 20, 0.6]], np.float32)   # area 400, offset (-90, -40): 400 - 2 * 9700 = -19000
    assert select_max_num(det, 0, 100, 200).tolist() == [0, 1, 2, 3]
    assert select_max_num(det, 4, 100, 200).tolist() == [0, 1, 2, 3]
    assert select_max_num(det, 2, 100, 200).tolist() == [2, 1]
    assert select_max_num(det, 1, 100, 200).tolist() == [2]
    assert select_max_num(det, 3, 100, 200).tolist() == [2, 1, 0]
    assert R.select_max_num(det, 2, 100, 200).tolist() == [2, 1]


def test_restatement_nms_and_tie_rule():
    d = np.array([[0, 0, 9, 9, 0.5],         # 0: tied with 2 and 4; first by index
                  [1, 1, 10, 10, 0.9],       # 1: the best; overlaps 0 (81 / 119 = 0.68) -> 0 goes
                  [20, 20, 29, 29, 0.5],     # 2: tied, apart from everything -> stays, before 4
                  [21, 20, 30, 29, 0.4],     # 3: overlaps 2 (90 / 110) -> goes
                  [40, 40, 49, 49, 0.5],     # 4: tied, stays
                  [40, 46, 49, 55, 0.3],     # 5: overlaps 4 by 40 / 160 = 0.25 <= 0.4 -> stays
                  [60, 60, 50, 50, 0.45]],   # 6: degenerate (x2 < x1): area 81, no overlap with anything -> stays
                 np.float32)
    keep = R.nms(d)
    assert keep == [1, 2, 4, 6, 5]
    order = np.argsort(-d[:, 4], kind="stable")
    assert order.tolist() == [1, 0, 2, 4, 6, 3, 5]
    # exactly at the threshold survives (ovr <= 0.4): two 10 x 10 boxes sharing 8 of 14 columns... 80 / 200 = 0.4
    e = np.array([[0, 0, 9, 9, 0.9], [0, 0, 9, 9, 0.8]], np.float32)
    e[1, [1, 3]] += 4.285                      # not exact: just below / above is what the margin assertion guards
    assert R.min_ovr_margin(e) < 0.05
    # a NaN overlap suppresses
    n = np.array([[0, 0, 9, 9, 0.9], [np.nan, 0, 9, 9, 0.8], [30, 30, 39, 39, 0.7]], np.float32)
    assert R.nms(n) == [0, 2]


def _expected_plan(dt_name):
    """The launches of one detect call at det_size (96, 64), walked from the table."""
    want = ["letterbox out=64x96", "stem backbone.stem.0 in=64x96 cin=3 cout=28"]
    H, W = 32, 48
    lvl = lambda i: (64 // (8 << i), 96 // (8 << i))
    for u in pack.units()[1:]:
        part = u.name.split(".")
        if u.name == "backbone.layer1.0.conv1":
            want.append("maxpool in=32x48 c=56")
            H, W = 16, 24
        if part[0] == "neck" and part[1] != "pafpn_convs":
            H, W = lvl(int(part[2]))
        if u.name == "neck.fpn_convs.0.conv":
            want += ["upadd in=2x3 c=56", "upadd in=4x6 c=56"]
        if part[1] == "pafpn_convs":
            H, W = lvl(int(part[2]) + 1)
        if part[0] == "bbox_head":
            H, W = 64 // int(part[2]), 96 // int(part[2])
        if u.role in ("reg", "kps"):
            continue                                   # one launch with cls
        if u.role == "cls":
            want.append(f"head bbox_head.out.{part[2]} k=3 in={H}x{W} cin=80 cout=30 out=f32")
            continue
        k, st = (2, 2) if u.role == "avgdown" else (u.k, u.stride)
        res = u.name.endswith(".conv2") or u.name.startswith("neck.downsample_convs")
        want.append(f"conv {u.name} k={k} s={st} in={H}x{W} cin={u.cin} cout={u.cout} relu={int(u.relu)} "
                    f"res={int(res)} out={dt_name}")
        if u.role == "avgdown":            # the block's conv2 runs on the halved map
            H, W = H // 2, W // 2
    return want + ["decode cap=4096", "nms cap=4096"]


@pytest.mark.parametrize("dt,name", [(None, "f32"), (torch.bfloat16, "bf16"), (torch.float16, "f16")])
def test_dry_run_plan_lists_the_launches(dt, name):
    lines = SCRFD(det_size=DET_SIZE, compute_dtype=dt).plan(2)
    assert lines == _expected_plan(name)
    assert len(lines) == 1 + 1 + 2 + 1 + 27 + 10 + 2 + 9 + 3 + 2
    with pytest.raises(TypeError, match="unsupported dtype"):
        SCRFD(det_size=DET_SIZE, compute_dtype=torch.float64).plan(1)


def test_check_counts_names_the_frame():
    SCRFD.check_counts(np.array([[3, 10], [0, 0], [256, 4096]]))
    with pytest.raises(RuntimeError, match="frame 1 has 4097"):
        SCRFD.check_counts(np.array([[3, 10], [9, 4097]]))


def test_cpu_input_raises():
    net = SCRFD(det_size=DET_SIZE)
    x = torch.zeros(1, 45, 80, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        net.forward(x)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        net.detect_frames(x, 0.5)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        Face_detect_crop(net)
    with pytest.raises(ValueError, match="multiples of 32"):
        SCRFD(det_size=(100, 64))
