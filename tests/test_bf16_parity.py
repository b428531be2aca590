"""16-bit storage paths against the storage-emulating oracle: bf16 (the throughput path, the bench
configuration, B = 64) and fp16 (a ``.half()`` module, the reference's own GPU precision,
inference.py:30).

The oracle (oracle/aei_ref.aei_forward_bf16_storage / aei_forward_fp16_storage) restates the
reference forward with every tensor the runtime stores rounded to the storage dtype at the same
point, fp32 in between.  What remains between it and the kernels is fp32 summation order, which
flips a rounding here and there; through 8 decoder blocks those flips grow (measured: two 16-bit
evaluations of the network differ from each other by about as much as each differs from fp32).  So
the gates are:

* per stage, isolated: every AADBlk_k recomputed by the oracle from the GPU's own stored inputs
  (AADBlk_{k-1} output, z_attr_k) must match the GPU's AADBlk_k within a couple of ulps of the
  storage dtype (max |d| <= 2 ulp(max |ref|), mean |d| <= 5e-3 of mean |ref|); Y and its uint8
  frame likewise;
* encoder maps z_attr1..8 against the oracle's: 2 ulps, rel mean <= 2e-3;
* end to end: the GPU's error against the fp32 oracle is no larger than the emulated 16-bit
  arithmetic's own (mean and 99.9th percentile within 1.25x) — the kernels add nothing to the
  intrinsic storage error.
The per-stage gates look at four of the 64 rows (the oracle is a CPU forward); every row of the
batch is covered by the batch-permutation property (test_swap_batch_permutation_is_exact).
Measured values are in DESIGN.md §2 (tools/bf16_bisect.py prints them).
"""
import numpy as np
import pytest
import torch

from oracle import aei_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROWS = [0, 21, 42, 63]
_CACHE = {}
STORE = {"bf16": torch.bfloat16, "fp16": torch.float16}
MANT = {"bf16": 7, "fp16": 10}   # explicit mantissa bits
# Y / uint8 gates per storage dtype (Y max, Y mean, u8 max LSB, fraction of u8 bytes off)
YGATE = {"bf16": (0.03, 5e-4, 3, 0.02), "fp16": (0.01, 1e-4, 2, 0.01)}


def ulp(x: float, st: str) -> float:
    return 2.0 ** (np.floor(np.log2(max(x, 1e-30))) - MANT[st])


def ulp_bf16(x: float) -> float:
    return ulp(x, "bf16")


def model(backbone, nb, st):
    """bf16: compute_dtype=torch.bfloat16 (fp32 parameters); fp16: the reference's own form, the module
    .half()'d after loading the checkpoint (inference.py:27-30)."""
    from ghost_amd.network import AEI_Net
    p = aei_ref.make_weights(aei_ref.param_specs(backbone, nb))
    if st == "bf16":
        G = AEI_Net(backbone, num_blocks=nb, c_id=512, compute_dtype=torch.bfloat16).eval()
        G.load_state_dict(p)
        G = G.to(DEV)
    else:
        G = AEI_Net(backbone, num_blocks=nb, c_id=512).eval()
        G.load_state_dict(p)
        G = G.to(DEV).half()
    return p, G


def run(backbone, nb, B=64, rows=ROWS, st="bf16"):
    key = (backbone, nb, B, st, tuple(rows))
    if key not in _CACHE:
        _CACHE[key] = compute(backbone, nb, B, rows, st)
    return _CACHE[key]


def compute(backbone, nb, B, rows, st, fp32=True):
    """One forward_taps of a batch of B on the GPU and the oracles' forwards of ``rows`` of it (not cached:
    tests/test_batch_sweep.py walks many batch sizes).  fp32=False skips the fp32 oracle."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    p, G = model(backbone, nb, st)
    xt, z = aei_ref.make_inputs(B, 11)
    u8 = torch.empty(B, 256, 256, 3, dtype=torch.uint8, device=DEV)
    xin = xt.to(DEV) if st == "bf16" else xt.to(DEV).half()   # core.py:20-21: fp16 inputs for a .half() G
    zin = z.to(DEV) if st == "bf16" else z.to(DEV).half()
    Y, attr, blocks = G.forward_taps(xin, zin, out_u8=u8)
    torch.cuda.synchronize()
    assert Y.dtype == STORE[st]
    ri = torch.tensor(rows)
    zr = z[ri] if st == "bf16" else z[ri].half().float()
    xr = xt[ri] if st == "bf16" else xt[ri].half().float()
    # a .half() module holds every parameter and buffer in float16 (fc1/fc2, conv_h, biases, BatchNorm
    # statistics included: torch's Module.half()): the emulation runs on those rounded values
    pe = p if st == "bf16" else {k: v.half().float() for k, v in p.items()}
    r = {"p": pe, "z": zr, "xt": xr, "Y": Y[ri].float().cpu(), "u8": u8[ri].cpu().numpy(),
         "attr": [a[ri].float().cpu() for a in attr], "blocks": [b[ri].float().cpu() for b in blocks]}
    r["emu"] = aei_ref.aei_forward_bf16_storage(pe, r["xt"], r["z"], backbone, nb, store=STORE[st])
    if fp32:
        r["fp32"], a32 = aei_ref.aei_forward(p, r["xt"], r["z"], backbone, nb)
        r["fp32_attr"] = [a.float() for a in a32]
    return r


CASES = [("unet", 2), ("linknet", 3)]


def check_blocks(r, backbone, nb, st="bf16"):
    p, z = r["p"], r["z"]
    ymax, ymean, u8max, u8frac = YGATE[st]
    with aei_ref.storage(STORE[st]):
        prev = aei_ref.up1_bf16_storage(z, p)
        for k in range(1, 9):
            yk = aei_ref.gen_block_bf16_storage(prev, r["attr"][k - 1], z, p, backbone, nb, k)
            if k < 8:
                g = r["blocks"][k - 1]
                d = (g - yk).abs()
                assert float(d.max()) <= 2 * ulp(float(yk.abs().max()), st), (k, float(d.max()))
                assert float(d.mean()) <= 5e-3 * float(yk.abs().mean()), (k, float(d.mean()))
                prev = g
            else:
                t8 = torch.tanh(yk)
                dY = (r["Y"] - aei_ref._q(t8)).abs()
                assert float(dY.max()) <= ymax and float(dY.mean()) <= ymean, (float(dY.max()), float(dY.mean()))
                du = np.abs(r["u8"].astype(np.int16) - aei_ref.y_to_u8_bgr(t8).astype(np.int16))
                assert du.max() <= u8max and (du > 0).mean() < u8frac, (du.max(), (du > 0).mean())


@pytest.mark.parametrize("st", ["bf16", "fp16"])
@pytest.mark.parametrize("backbone,nb", CASES)
def test_encoder_maps_match_emulation(backbone, nb, st):
    """The attribute encoder's eight maps (unet / linknet: conv4x4 + deconv4x4 chains) against the storage
    emulation."""
    check_encoder_maps(run(backbone, nb, st=st), st)


def check_encoder_maps(r, st="bf16"):
    for i, (g, e) in enumerate(zip(r["attr"], r["emu"][1]), 1):
        d = (g - e).abs()
        assert float(d.max()) <= 2 * ulp(float(e.abs().max()), st), (i, float(d.max()))
        assert float(d.mean()) <= 2e-3 * float(e.abs().mean()), (i, float(d.mean()))


@pytest.mark.parametrize("st", ["bf16", "fp16"])
def test_resnet_encoder_maps_within_storage_error(st):
    """MLAttrEncoderResnet (resnet.py:81-149): its deepest map z_attr1 sits behind two 7x7 convs and 12 Bottlenecks
    (36 convs, 12 residual adds), so a summation-order flip early in the chain reaches the maps a few ulps wide
    (measured: outside the 2-ulp gate the conv4x4 chains pass): its maps are
    gated end to end like Y — per map, the GPU's error against the fp32 oracle within 1.25x (mean) / 1.3x (top
    0.5 %) of the emulated 16-bit arithmetic's own error."""
    check_resnet_encoder_maps(run("resnet", 2, 4, list(range(4)), st=st), st)


def check_resnet_encoder_maps(r, st="bf16"):
    for i, (g, e, f) in enumerate(zip(r["attr"], r["emu"][1], r["fp32_attr"]), 1):
        dg, de = (g - f).abs().flatten(), (e.float() - f).abs().flatten()
        tol = ulp(float(f.abs().max()), st) / 64
        assert float(dg.mean()) <= 1.25 * float(de.mean()) + tol, (i, float(dg.mean()), float(de.mean()))
        k = max(1, dg.numel() // 200)
        tg, te = float(dg.topk(k).values.mean()), float(de.topk(k).values.mean())
        assert tg <= 1.3 * te + tol, (i, tg, te)


@pytest.mark.parametrize("st", ["bf16", "fp16"])
@pytest.mark.parametrize("backbone,nb", CASES)
def test_each_decoder_block_matches_emulation(backbone, nb, st):
    """Bisection by construction: each block from the GPU's own stored inputs."""
    check_blocks(run(backbone, nb, st=st), backbone, nb, st)


@pytest.mark.parametrize("st", ["bf16", "fp16"])
@pytest.mark.parametrize("backbone,nb,B", [("unet", 2, 1), ("linknet", 3, 2), ("unet", 1, 4), ("unet", 3, 2),
                                           ("resnet", 2, 4)])
def test_small_batch_blocks_match_emulation(backbone, nb, B, st):
    """Small batches take other kernels (split-K GEMMs, the generic AAD path): same per-stage gates."""
    check_blocks(run(backbone, nb, B, list(range(B)), st=st), backbone, nb, st)


@pytest.mark.parametrize("st", ["bf16", "fp16"])
@pytest.mark.parametrize("backbone,nb", CASES)
def test_end_to_end_error_is_the_intrinsic_storage_error(backbone, nb, st):
    r = run(backbone, nb, st=st)
    ref = r["fp32"]
    dg = (r["Y"] - ref).abs().flatten()
    de = (r["emu"][0] - ref).abs().flatten()
    assert float(dg.mean()) <= 1.25 * float(de.mean()), (float(dg.mean()), float(de.mean()))
    qg, qe = float(torch.quantile(dg[:1 << 22], 0.999)), float(torch.quantile(de[:1 << 22], 0.999))
    assert qg <= 1.25 * qe, (qg, qe)
    assert torch.isfinite(r["Y"]).all()


@pytest.mark.parametrize("backbone,nb", CASES)
def test_half_module_is_more_accurate_than_bf16(backbone, nb):
    """The point of the fp16 path: a .half() drop-in has the reference GPU precision, several times
    closer to the fp32 forward than bf16 storage (~4x in the mean)."""
    e16 = (run(backbone, nb, st="fp16")["Y"] - run(backbone, nb, st="fp16")["fp32"]).abs().mean()
    eb = (run(backbone, nb, st="bf16")["Y"] - run(backbone, nb, st="bf16")["fp32"]).abs().mean()
    assert float(e16) * 2.5 <= float(eb), (float(e16), float(eb))


@pytest.mark.parametrize("st", ["bf16", "fp16"])
def test_swap_batch_permutation_is_exact(st):
    """Every one of the 64 rows: swapping a permuted batch gives the permuted uint8 frames bit for bit
    (frames are independent inside G; a row-specific indexing error in any kernel — the 8x8 multi-image
    conv, XCD-ordered tile maps, per-sample statistics records — would break it)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _p, G = model("unet", 2, st)
    B = 64
    crops = torch.from_numpy(aei_ref.make_u8_crops(B, seed=31)).to(DEV)
    g = torch.Generator().manual_seed(5)
    z = torch.randn(B, 512, generator=g).to(DEV)
    z = z if st == "bf16" else z.half()
    perm = torch.randperm(B, generator=g).to(DEV)
    out = G.swap_u8(crops, z).clone()
    outp = G.swap_u8(crops[perm].contiguous(), z[perm].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(outp, out[perm])
    # and a batch of 1 reproduces its row of the batch of 64 up to 16-bit storage noise: B = 1 runs other
    # kernels (split-K GEMMs, the generic AAD path), whose different fp32 summation order flips 16-bit
    # roundings that compound through 8 InstanceNorm'd blocks (measured up to 34 LSB in
    # bf16).  Yardstick: the B = 64 row's own distance from the fp32 oracle.
    one = G.swap_u8(crops[7:8].contiguous(), z[7:8].contiguous())
    torch.cuda.synchronize()
    d = (one[0].int() - out[7].int()).abs().cpu().numpy()
    xt = aei_ref.transform_target(crops[7:8].cpu().numpy())
    ref = aei_ref.y_to_u8_bgr(aei_ref.aei_forward(_p, xt, z[7:8].float().cpu())[0])[0].astype(np.int16)
    d32 = np.abs(out[7].cpu().numpy().astype(np.int16) - ref)
    k = max(1, d.size // 200)
    assert d.mean() <= 1.25 * d32.mean() + 0.02, (float(d.mean()), float(d32.mean()))
    assert np.sort(d, axis=None)[-k:].mean() <= 1.3 * np.sort(d32, axis=None)[-k:].mean() + 1.0


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_tap_partial_modes_match_emulation(mode):
    """GHOST_AEI_OPT_TAP_PARTIALS 0 (AADBlk8's output conv on the concatenated channels), 1 (the h path's
    partials added into the narrow conv) and 2 (both paths' partials, the default): AADBlk8 against the
    emulation run with the same mode, from the GPU's own AADBlk7 output."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    p, G = model("unet", 2, "bf16")
    G.set_option("tap_partials", mode)
    xt, z = aei_ref.make_inputs(4, 13)
    u8 = torch.empty(4, 256, 256, 3, dtype=torch.uint8, device=DEV)
    Y, attr, blocks = G.forward_taps(xt.to(DEV), z.to(DEV), out_u8=u8)
    torch.cuda.synchronize()
    with aei_ref.storage(torch.bfloat16, tap_partials=mode):
        y8 = aei_ref.gen_block_bf16_storage(blocks[6].float().cpu(), attr[7].float().cpu(), z, p, "unet", 2, 8)
        t8 = torch.tanh(y8)
        dY = (Y.float().cpu() - aei_ref._q(t8)).abs()
    assert float(dY.max()) <= 0.03 and float(dY.mean()) <= 5e-4, (mode, float(dY.max()), float(dY.mean()))
    du = np.abs(u8.cpu().numpy().astype(np.int16) - aei_ref.y_to_u8_bgr(t8).astype(np.int16))
    assert du.max() <= 3 and (du > 0).mean() < 0.02, (mode, du.max(), (du > 0).mean())
