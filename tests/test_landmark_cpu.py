"""Host-side checks of ghost_amd.landmarks (no GPU): the layer table and parameter names against what the reference's
symbol file says (tests/golden/landmark_2d106det.npz), the checkpoint loader, the slot pack against the runtime's
declared slots, the float64 restatement against its recorded outputs, and the run logic of identity_masks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import landmark_ref
from ghost_amd import _lib
from ghost_amd.landmarks import Landmark106, identity_landmarks, pack, present_runs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "landmark_2d106det.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_table_and_names_match_symbol_file(golden):
    sys.path.insert(0, os.path.dirname(GOLDEN))
    try:
        import make_golden_landmark
    finally:
        sys.path.pop(0)
    own = make_golden_landmark.own_graph()
    for k in make_golden_landmark.GRAPH_KEYS:
        assert golden[k].shape == own[k].shape and bool((golden[k] == own[k]).all()), k
    assert len(golden["param_names"]) == 28 * 6 + 2
    assert pack.BN_EPS == 1e-3 and landmark_ref.EPS == pack.BN_EPS


def test_state_dict_keys_are_checkpoint_names(golden):
    net = Landmark106()
    sd = net.state_dict()
    assert sorted(sd) == sorted(golden["param_names"].tolist())
    for n, kind, shape in zip(golden["param_names"], golden["param_kinds"], golden["param_shapes"]):
        assert tuple(sd[n].shape) == tuple(int(v) for v in shape if v), n
    bufs = {n for n, _ in net.named_buffers()}
    assert bufs == {n for n, k in zip(golden["param_names"], golden["param_kinds"]) if k == "aux"}
    net.load_state_dict(landmark_ref.make_weights(), strict=True)


class _Nd:
    """What mx.nd.load returns per tensor."""
    def __init__(self, a):
        self.a = a

    def asnumpy(self):
        return self.a


def test_load_mxnet_params(golden):
    p = landmark_ref.make_weights()
    kinds = dict(zip(golden["param_names"].tolist(), golden["param_kinds"].tolist()))
    arg = {k: _Nd(v.numpy()) for k, v in p.items() if kinds[k] == "arg"}
    aux = {k: v.numpy() for k, v in p.items() if kinds[k] == "aux"}
    a = Landmark106()
    a.load_mxnet_params(arg, aux)
    b = Landmark106()
    b.load_mxnet_params({f"{kinds[k]}:{k}": v for k, v in p.items()})          # mx.nd.load's prefixed keys
    for k, v in p.items():
        assert torch.equal(a.state_dict()[k], v) and torch.equal(b.state_dict()[k], v), k
    short = dict(arg)
    del short["conv_7_dw_relu_gamma"]
    with pytest.raises(KeyError, match="conv_7_dw_relu_gamma"):
        Landmark106().load_mxnet_params(short, aux)
    with pytest.raises(KeyError, match="fc2_weight"):
        Landmark106().load_mxnet_params(dict(arg, fc2_weight=np.zeros(3)), aux)
    with pytest.raises(ValueError, match="fc1_bias"):
        Landmark106().load_mxnet_params(dict(arg, fc1_bias=np.zeros(3, np.float32)), aux)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_pack_binds_every_declared_slot(dt):
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.ghost_lmk_create(_lib.gdtype(dt), C.byref(h)), "create")
    try:
        slots = pack.pack_landmark(landmark_ref.make_weights(), dt)
        assert sorted(slots) == sorted(pack.slot_names())
        assert lib.ghost_lmk_missing(h) == len(slots)
        assert lib.ghost_lmk_bind(h, b"no.such.slot", slots["fc.w"].data_ptr(), 1) == -1
        for name, t in slots.items():
            assert t.is_contiguous() and t.dtype == (dt if name.endswith((".pw.w", "c15.w")) else torch.float32), name
            _lib.check(lib.ghost_lmk_bind(h, name.encode(), t.data_ptr(), t.numel()), name)
        assert lib.ghost_lmk_missing(h) == 0
        assert lib.ghost_lmk_workspace_bytes(h, 0) > 0 and lib.ghost_lmk_workspace_bytes(h, 3) > 3 * 96 * 96 * 32 * 2
        # N = 0 is GHOST_OK before anything is looked at
        assert lib.ghost_lmk_forward(h, None, 0, 1, 0, None, None, 0, None) == 0
    finally:
        lib.ghost_lmk_destroy(h)


def test_pack_layouts():
    p = landmark_ref.make_weights()
    s = pack.pack_landmark(p, torch.float32)
    w = p["conv_1_conv2d_weight"]
    assert float(s["stem.w"][(1 * 3 + 2) * 3 + 0, 5]) == float(w[5, 0, 1, 2])
    assert float(s["c5.dw.w"][2 * 3 + 1, 17]) == float(p["conv_5_dw_conv2d_weight"][17, 0, 2, 1])
    assert tuple(s["c2.pw.w"].shape) == (128, 32) and float(s["c2.pw.w"][7, 9]) == float(p["conv_2_conv2d_weight"][7, 9, 0, 0])
    assert float(s["c2.pw.w"][:, 16:].abs().max()) == 0.0                    # the K padding of Cin = 16
    assert float(s["fc.w"][(2 * 3 + 1) * 64 + 11, 100]) == float(p["fc1_weight"][100, 11 * 9 + 2 * 3 + 1])
    sc = 1.0 / torch.sqrt(p["conv_3_batchnorm_moving_var"] + 1e-3)           # the stored gamma is not used
    assert torch.allclose(s["c3.pw.scale"][:64], sc, rtol=1e-6, atol=0)
    assert torch.allclose(s["c3.pw.shift"][:64], p["conv_3_batchnorm_beta"] - p["conv_3_batchnorm_moving_mean"] * sc,
                          rtol=1e-6, atol=1e-7)


def test_restatement_matches_recorded_outputs(golden):
    p = landmark_ref.make_weights()
    pred, taps = landmark_ref.forward(p, landmark_ref.make_input(2), bgr=True, dtype=torch.float64)
    assert float((pred - torch.from_numpy(golden["pred"])).abs().max()) <= 1e-9
    for n, t in taps.items():
        t = t[:, :, ::4, ::4] if n == "conv_2" else t
        assert float((t - torch.from_numpy(golden[f"tap_{n}"]).double()).abs().max()) <= 2e-6, n
    # float32 evaluation and the storage emulation run, and the emulation does move the result
    p32, _ = landmark_ref.forward(p, landmark_ref.make_input(1), dtype=torch.float32)
    ph, _ = landmark_ref.forward(p, landmark_ref.make_input(1), dtype=torch.float32, store=torch.float16)
    assert float((p32.double() - pred[:1]).abs().max()) < 1e-4
    assert 0.0 < float((ph.double() - pred[:1]).abs().max()) < 0.1
    lm = landmark_ref.landmarks_of(pred)
    assert tuple(lm.shape) == (2, 106, 2)
    assert float(lm[0, 0, 0]) == (float(pred[0, 0]) + 1.0) * 96.0 * 1.75 - 56.0


class _StubNet:
    """landmarks_u8 returns each crop's first byte as every coordinate and records the batches it was given."""
    def __init__(self):
        self.calls = []

    def landmarks_u8(self, crops):
        self.calls.append(crops[:, 0, 0, 0].tolist())
        return crops[:, 0, 0, 0].float().view(-1, 1, 1).expand(-1, 106, 2).contiguous()


def test_identity_landmarks_runs():
    present = [0, 1, 1, 1, 0, 0, 1, 1, 0, 1]
    assert present_runs(present) == [(1, 4), (6, 8), (9, 10)]
    assert present_runs([]) == [] and present_runs([0, 0]) == [] and present_runs([1, 1]) == [(0, 2)]
    F_ = len(present)
    swaps = torch.zeros(F_, 224, 224, 3, dtype=torch.uint8)
    crops = torch.zeros(F_, 224, 224, 3, dtype=torch.uint8)
    swaps[:, 0, 0, 0] = torch.arange(F_, dtype=torch.uint8) + 100
    crops[:, 0, 0, 0] = torch.arange(F_, dtype=torch.uint8) + 100
    crops[1, 0, 0, 0] = 90          # run 1: swap - target = +10 per point, offset 30 -> [15, 15, 10]
    crops[6, 0, 0, 0] = 107         # run 2: -1 per point on the left, +1 on the right -> offset 3 -> [5, 5, 5]
    crops[9, 0, 0, 0] = 111         # run 3: offset +6 (from the right side) -> [10, 10, 8]
    net = _StubNet()
    lm, params, idx = identity_landmarks(net, swaps, crops, np.array(present, bool))
    assert net.calls == [[101, 102, 103, 106, 107, 109], [90, 107, 111]]      # one swap batch, one batch of run starts
    assert idx.tolist() == [1, 2, 3, 6, 7, 9]
    assert lm[2, 50, 1] == 102.0 and not lm[0].any() and not lm[4].any()
    assert params.tolist() == [[0, 0, 0], [15, 15, 10], [15, 15, 10], [15, 15, 10], [0, 0, 0], [0, 0, 0], [5, 5, 5],
                               [5, 5, 5], [0, 0, 0], [10, 10, 8]]
    net = _StubNet()
    lm, params, idx = identity_landmarks(net, swaps, crops, np.zeros(F_, bool))
    assert net.calls == [] and len(idx) == 0 and not params.any()


def test_cpu_input_raises():
    net = Landmark106()
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        net.forward(torch.zeros(1, 192, 192, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        net.landmarks_u8(torch.zeros(1, 224, 224, 3, dtype=torch.uint8))
