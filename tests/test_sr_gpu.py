"""use_sr face enhancer on an MI355X: ghost_amd.sr.LIPSPADEGenerator against the fixture that
tests/golden/make_golden_sr.py wrote by running the reference generator (train mode, two consecutive forwards at
B = 2), and against the storage-emulating restatement tests/sr_ref.py for the 16-bit paths.

Measured on an MI355X (DESIGN.md §10 holds the same figures):
  fp32   max|dY1| 8.6e-6  max|dY2| 7.7e-6  encoder output 5.1e-5  u8: 21 of 393216 bytes differ, by 1
  bf16   mean|dY| 7.456e-3 (emulation 7.458e-3)  top 0.5 % 3.817e-2 (3.830e-2)
  fp16   mean|dY| 9.365e-4 (emulation 9.382e-4)  top 0.5 % 4.779e-3 (4.825e-3)
  frozen sigma against the restatement 8.4e-6; permuted batch 1.0e-6; row 0 alone against row 0 of B = 2: 4.3e-2
"""
import os

import numpy as np
import pytest
import torch

import sr_ref
from oracle import aei_ref, golden_io

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = torch.device("cuda:0")
Y_GATE = 1e-3        # the project's fp32 gate for AEI_Net, whose output has the same tanh range
ENC_GATE = 1e-4      # the attr-map gate


@pytest.fixture(scope="module")
def gold():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return golden_io.load(GOLD, "sr_lipspade_b2")


@pytest.fixture(scope="module")
def weights():
    """The recipe weights, shared and never modified (every user loads a copy)."""
    return aei_ref.make_weights(sr_ref.param_specs())


@pytest.fixture(scope="module")
def x2():
    return sr_ref.make_input(2, seed=7)


@pytest.fixture(scope="module")
def iterated(weights, x2):
    """The recipe weights after one reference-style power iteration: unit u, v (the recipe's are N(0, 0.02)
    vectors, whose eval-mode sigma is meaningless).  Shared, never modified."""
    p = dict(weights)
    sr_ref.sr_forward(p, x2[:1])
    return p


def _model(weights, **kw):
    from ghost_amd.sr import LIPSPADEGenerator
    G = LIPSPADEGenerator(**kw)
    G.load_state_dict(weights, strict=True)
    return G.to(DEV)


@pytest.fixture(scope="module")
def fp32_run(weights, x2):
    """Two consecutive fp32 forwards of one module: (Y1, encoder tap of call 1, Y2, module)."""
    G = _model(weights)
    y1, taps = G.forward_taps(x2.to(DEV))
    y1, enc = y1.float().cpu(), taps["enc"].float().cpu()
    y2 = G(x2.to(DEV)).float().cpu()
    return y1, enc, y2, G


def test_fp32_parity_with_the_reference(gold, fp32_run):
    y1, enc, y2, G = fp32_run
    assert y1.shape == (2, 3, 256, 256) and y1.dtype == torch.float32
    d1 = float((y1 - torch.from_numpy(gold["Y1"])).abs().max())
    d2 = float((y2 - torch.from_numpy(gold["Y2"])).abs().max())
    de = float((enc - torch.from_numpy(gold["enc"])).abs().max())
    u8 = sr_ref.postprocess_u8(y1)
    du = np.abs(u8.astype(np.int16) - gold["U8"].astype(np.int16))
    print(f"SRFIG fp32 max|dY1|={d1:.2e} max|dY2|={d2:.2e} enc={de:.2e} u8 max={du.max()} differing={(du > 0).sum()}"
          f" of {du.size}")
    assert d1 <= Y_GATE and d2 <= Y_GATE, (d1, d2)
    assert de <= ENC_GATE, de
    assert du.max() <= 1                      # truncation flips only
    # the second call ran another power iteration (weight_u / weight_v were updated in place)
    assert float((y2 - y1).abs().max()) > 1e-2
    u_ref = aei_ref.make_weights(sr_ref.param_specs())["head_0.conv_0.weight_u"]
    assert float((G.head_0.conv_0.weight_u.cpu() - u_ref).abs().max()) > 1e-3


@pytest.mark.parametrize("st", ["bf16", "fp16"])
def test_16bit_error_is_the_storage_error(gold, weights, x2, st):
    dt = torch.bfloat16 if st == "bf16" else torch.float16
    G = _model(weights, compute_dtype=dt)
    y = G(x2.to(DEV))
    assert y.dtype == dt
    y = y.float().cpu()
    emu = sr_ref.sr_forward(dict(weights), x2, store=dt)
    ref = torch.from_numpy(gold["Y1"])
    dg, de = (y - ref).abs().flatten(), (emu - ref).abs().flatten()
    k = max(1, dg.numel() // 200)
    tg, te = float(dg.topk(k).values.mean()), float(de.topk(k).values.mean())
    print(f"SRFIG {st} mean|dY| gpu={float(dg.mean()):.3e} emu={float(de.mean()):.3e} "
          f"top0.5% gpu={tg:.3e} emu={te:.3e}")
    assert torch.isfinite(y).all()
    assert float(dg.mean()) <= 1.25 * float(de.mean()), (float(dg.mean()), float(de.mean()))
    assert tg <= 1.3 * te, (tg, te)


def test_half_module_selects_fp16_storage(weights, x2):
    G = _model(weights).half()
    y = G(x2[:1].to(DEV))
    assert y.dtype == torch.float16 and bool(torch.isfinite(y).all())
    assert G.head_0.conv_0.weight_u.dtype == torch.float16


def test_frozen_sigma_is_deterministic_and_matches(iterated, x2):
    """power_iteration=False: sigma from the stored u, v (torch's eval-mode value); two calls give identical bytes
    and leave u, v alone."""
    p = iterated
    G = _model(p, power_iteration=False)
    a = G(x2.to(DEV))
    b = G(x2.to(DEV))
    assert torch.equal(a, b)
    assert torch.equal(G.head_0.conv_0.weight_u.cpu(), p["head_0.conv_0.weight_u"])
    ref = sr_ref.sr_forward(dict(p), x2, power_iteration_step=False)
    d = float((a.float().cpu() - ref).abs().max())
    print(f"SRFIG frozen-sigma max|dY|={d:.2e}")
    assert d <= Y_GATE, d


def test_batch_coupling(weights, x2, fp32_run):
    """BatchNorm statistics are the batch's: a permuted batch gives the permuted rows, and row 0 of B = 2 differs
    from the same image alone (an implementation on instance statistics would give the same row)."""
    y1 = fp32_run[0]
    G = _model(weights)
    yp = G(x2.flip(0).to(DEV)).float().cpu()
    d = float((yp.flip(0) - y1).abs().max())
    G1 = _model(weights)
    ya = G1(x2[:1].to(DEV)).float().cpu()
    da = float((ya[0] - y1[0]).abs().max())
    print(f"SRFIG permuted batch max|d|={d:.2e}; row 0 alone vs in B=2: {da:.3e}")
    assert d <= Y_GATE, d
    assert da > 5e-3, da


def test_face_enhancement_matches_direct_forward(iterated):
    from ghost_amd.sr import Pix2PixModel, face_enhancement
    g = np.random.Generator(np.random.PCG64(3))
    crops = g.integers(0, 256, size=(2, 256, 256, 3), dtype=np.uint8)
    model = Pix2PixModel(state_dict=iterated, power_iteration=False)
    model.netG.to(DEV)
    frames = [[crops[0], [], crops[1]]]
    out, dev = face_enhancement(frames, model, return_device=True)
    assert len(out) == 1 and len(out[0]) == 3 and out[0][1] == []
    x = torch.from_numpy(crops[..., ::-1].copy()).permute(0, 3, 1, 2).float().div(255.0).to(DEV)
    y = model({"label": x, "image": x}, mode="inference2")
    want = sr_ref.postprocess_u8(y.float().cpu())
    for j, n in ((0, 0), (2, 1)):
        assert out[0][j].dtype == np.uint8 and out[0][j].shape == (256, 256, 3)
        assert np.array_equal(out[0][j], want[n])
    assert dev[0].is_cuda and np.array_equal(dev[0].cpu().numpy(), want)
    # a device tensor of crops gives the same bytes
    out2 = face_enhancement([torch.from_numpy(crops).to(DEV)], model)
    assert np.array_equal(out2[0][0], want[0]) and np.array_equal(out2[0][1], want[1])
