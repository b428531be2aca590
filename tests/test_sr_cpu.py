"""use_sr face enhancer, checks that need no GPU: the restatement (tests/sr_ref.py) against the fixture that
tests/golden/make_golden_sr.py wrote by running the reference generator in train mode, the module's state_dict,
and face_enhancement's bookkeeping."""
import os

import numpy as np
import pytest
import torch

import sr_ref
from oracle import aei_ref, golden_io

GOLD = os.path.join(os.path.dirname(__file__), "golden")
PIN = 1e-5      # the project's oracle-pin level


@pytest.fixture(scope="module")
def gold():
    return golden_io.load(GOLD, "sr_lipspade_b2")


@pytest.fixture(scope="module")
def ref_run(gold):
    """Two consecutive restated forwards (shared, read-only): (Y1, taps of call 1, Y2)."""
    p = aei_ref.make_weights(sr_ref.param_specs())
    x = sr_ref.make_input(int(gold["batch"]), int(gold["seed"]))
    taps = {}
    y1 = sr_ref.sr_forward(p, x, taps=taps)
    y2 = sr_ref.sr_forward(p, x)
    return y1, taps, y2


def test_restatement_matches_reference_outputs(gold, ref_run):
    y1, _, y2 = ref_run
    d1 = float((y1 - torch.from_numpy(gold["Y1"])).abs().max())
    d2 = float((y2 - torch.from_numpy(gold["Y2"])).abs().max())
    print(f"SRFIG restatement max|dY1|={d1:.2e} max|dY2|={d2:.2e}")
    assert d1 <= PIN and d2 <= PIN, (d1, d2)
    # the per-call power iteration is modelled: the second call sees other spectral-norm vectors
    assert float((y2 - y1).abs().max()) > 1e-2
    assert float((torch.from_numpy(gold["Y2"]) - torch.from_numpy(gold["Y1"])).abs().max()) > 1e-2


def test_restatement_matches_reference_taps(gold, ref_run):
    _, taps, _ = ref_run
    assert float((taps["enc"] - torch.from_numpy(gold["enc"])).abs().max()) <= PIN
    for name in sr_ref.TAP_NAMES[1:]:
        n = name.replace(".", "_")
        a = taps[name]
        assert tuple(a.shape) == tuple(gold[f"{n}_shape"])
        flat = a.reshape(-1).double()
        np.testing.assert_allclose(flat[gold[f"{n}_idx"]].float().numpy(), gold[f"{n}_sample"], atol=PIN, rtol=PIN)
        np.testing.assert_allclose(float(flat.abs().sum()), float(gold[f"{n}_abssum"]), rtol=PIN)


def test_restatement_u8(gold, ref_run):
    u8 = sr_ref.postprocess_u8(ref_run[0])
    diff = np.abs(u8.astype(np.int16) - gold["U8"].astype(np.int16))
    assert u8.shape == (2, 256, 256, 3) and diff.max() <= 1 and (diff > 0).mean() < 1e-3


def test_store_float32_is_the_unrounded_forward(gold, ref_run):
    p = aei_ref.make_weights(sr_ref.param_specs())
    x = sr_ref.make_input(int(gold["batch"]), int(gold["seed"]))
    taps = {}
    y = sr_ref.sr_forward(p, x, store=torch.float32, taps=taps)
    assert torch.equal(y, ref_run[0]) and torch.equal(taps["enc"], ref_run[1]["enc"])


def test_store_bf16_rounds(gold):
    p = aei_ref.make_weights(sr_ref.param_specs())
    x = sr_ref.make_input(1, 7)
    taps = {}
    y = sr_ref.sr_forward(p, x, store=torch.bfloat16, taps=taps)
    for t in (y, taps["enc"], taps["head_0"], taps["ups.2"]):
        assert torch.equal(t, t.to(torch.bfloat16).float())
    assert torch.isfinite(y).all()


def test_module_state_dict_keys_shapes_and_load(gold):
    from ghost_amd.sr import LIPSPADEGenerator, TestOptions
    G = LIPSPADEGenerator(TestOptions())
    sd = G.state_dict()
    got = [(k, ",".join(str(d) for d in v.shape)) for k, v in sd.items()]
    want = list(zip(gold["keys"].tolist(), gold["shapes"].tolist()))
    assert got == want and len(got) == 230
    assert sum(v.numel() for k, v in sd.items() if v.is_floating_point()) == sum(
        int(np.prod(s)) for _, s, kind in sr_ref.param_specs() if kind != "bn_nbt")
    for k, v in sd.items():
        assert v.dtype == (torch.int64 if k.endswith("num_batches_tracked") else torch.float32), k
    w = aei_ref.make_weights(sr_ref.param_specs())
    res = G.load_state_dict(w, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(G.state_dict()["ups.3.conv_s.weight_u"], w["ups.3.conv_s.weight_u"])


def test_options_and_unsupported_geometry():
    from ghost_amd.sr import LIPSPADEGenerator, TestOptions
    o = TestOptions()
    assert (o.netG, o.ngf, o.semantic_nc, o.crop_size, o.num_upsampling_layers, o.norm_G, o.use_vae, o.is_test) == (
        "lipspade", 48, 3, 256, "normal", "spectralspadesyncbatch3x3", False, True)

    class Other(TestOptions):
        num_upsampling_layers = "more"
    with pytest.raises(NotImplementedError):
        LIPSPADEGenerator(Other())

    class Wide(TestOptions):
        ngf = 64
    with pytest.raises(NotImplementedError):
        LIPSPADEGenerator(Wide())


def test_cpu_tensors_raise():
    from ghost_amd.sr import LIPSPADEGenerator, Pix2PixModel, face_enhancement
    G = LIPSPADEGenerator()
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        G(torch.zeros(1, 3, 256, 256))
    m = Pix2PixModel()
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m({"label": torch.zeros(1, 3, 256, 256)}, mode="inference2")
    with pytest.raises(NotImplementedError):
        m({"label": torch.zeros(1, 3, 256, 256)}, mode="inference")
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        face_enhancement([[np.zeros((256, 256, 3), np.uint8)]], m)
    for name in ("head_0", "lip_encoder"):
        with pytest.raises(NotImplementedError):
            getattr(G, name)(torch.zeros(1))


class _StandIn:
    """A host model that records every call: returns 1 - x, so an input byte v comes back as 255 - v."""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def __call__(self, data, mode):
        assert mode == "inference2" and data["label"] is data["image"]
        x = data["label"]
        assert x.dtype == torch.float32 and tuple(x.shape[1:]) == (3, 256, 256)
        self.calls.append(x.clone())
        return 1.0 - x


def _crop(v):
    a = np.empty((256, 256, 3), np.uint8)
    a[..., 0], a[..., 1], a[..., 2] = v, (v + 1) % 256, (v + 2) % 256     # B, G, R
    return a


def test_face_enhancement_bookkeeping_and_chunks():
    from ghost_amd.sr import face_enhancement
    # target 0: 43 faces with blanks at 0, 5 and the end -> chunks of 20, 20, 3; target 1: no face; target 2: one
    t0 = [[]] + [_crop(i) for i in range(4)] + [[]] + [_crop(i) for i in range(4, 43)] + [[]]
    frames = [t0, [[], []], [_crop(200)]]
    m = _StandIn()
    out, dev = face_enhancement(frames, m, return_device=True)
    assert [c.shape[0] for c in m.calls] == [20, 20, 3, 1]
    assert len(out) == 3 and [len(o) for o in out] == [len(f) for f in frames]
    assert out[1] == [[], []] and dev[1] is None and out[0][0] == [] and out[0][5] == [] and out[0][-1] == []
    faces = [f for f in out[0] if not isinstance(f, list)]
    assert len(faces) == 43 and tuple(dev[0].shape) == (43, 256, 256, 3) and dev[0].dtype == torch.uint8
    for i, f in enumerate(faces):
        assert f.dtype == np.uint8 and f.shape == (256, 256, 3)
        # BGR in, BGR out, each byte v -> trunc(clamp((1 - v / 255) * 255))
        want = (1.0 - torch.from_numpy(_crop(i)).float() / 255.0).mul(255).clamp(0, 255).to(torch.uint8).numpy()
        assert np.array_equal(f, want), i
        assert np.array_equal(dev[0][i].numpy(), f)
    # the model saw RGB / 255, rows in face order: row 3 of the second chunk is face 23
    x = m.calls[1][3]
    assert torch.equal(x[:, 0, 0], torch.tensor([25.0, 24.0, 23.0]) / 255.0)
    # the input list is not modified; another batch size regroups the same rows
    assert t0[0] == [] and np.array_equal(t0[1], _crop(0))
    m2 = _StandIn()
    out2 = face_enhancement(frames, m2, batch_size=16)
    assert [c.shape[0] for c in m2.calls] == [16, 16, 11, 1]
    assert all(np.array_equal(a, b) for a, b in zip(out2[0], out[0]) if not isinstance(a, list))
    # a tensor of crops instead of a list
    out3 = face_enhancement([torch.from_numpy(np.stack([_crop(7), _crop(9)]))], _StandIn())
    assert np.array_equal(out3[0][1], out[0][11])
