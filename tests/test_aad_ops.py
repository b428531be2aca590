"""Op tests of the AAD blend and mask kernels (MI355X): every production variant, pinned by its plan-log
signature, against a float64 reference of the same operation, per element.

Blend kernels (aad_v3.hip, aad_wide.hip, aad_fused.hip)
  reference  oracle/aei_ref.aad_layer on float64 tensors + leaky_relu(slope); inputs, z_attr and every parameter
             pre-rounded to the storage type; a through-upsample case reads F.interpolate(align_corners) of its
             source, evaluated in fp32 and rounded to the storage type.  The large cases evaluate the same plain
             torch expression on the device (aad_cases.aad_expr); test_reference_expression_matches_the_oracle
             holds the two evaluations together.
  gate       per element, den = max(1, |ref64|), ulp = 2^-7 (bf16) / 2^-10 (fp16):
               16-bit   |got - ref64| / den <= (0.5 + s + 32 e32) ulp
               fp32     |got - ref64| / den <= 32 e32
             0.5: the one rounding at the store.  e32: the error of the oracle's own fp32 evaluation of the case
             (computed in the test); the factor 32 covers the kernels' other fp32 summation order and their
             v_exp / v_rcp sigmoid.  s: only where the statistics of a through-upsample read take the closed
             form over the source (statistics of the unrounded fp32 upsample): the float64 reference re-evaluated
             with those statistics (computed in the test).
  ties       a through-upsample kernel rounds its own fp32 bilinear mix (up2x.h up2x_mix, FMA-contracted) to the
             storage type; F.interpolate's fp32 value differs in the last bits, so where that value lies within
             2^-21 sum |lambda v_tap| of a rounding midpoint the two may pick different neighbours (measured: 9 of
             1 M, 629 of 33 M elements of h_in, every one of them flagged).  For the elements such a tie reaches
             (the element itself, and its pixel's other channels through the mask) the gate adds the first-order
             effect of one storage step of h_in, derived in aad_cases.tie_allowance; every other element keeps
             the gate above.  The existing 4e-2 tests could not see this.
  also       the plan log holds exactly one AAD kernel, the expected one, with its parameters; outputs have
             ldo = C + 8 (the second layer C + 16) pre-filled with a sentinel that must survive bit for bit;
             h_in and z_attr have 8 NaN pad channels; B >= 2 with every sample and its z_id different.

Mask kernels (ops.hip aad_mask2 / stats_mask_small through ghost_aad_mask_nhwc)
  reference  sigmoid(sum_c wh_c (h_c - mean_c) rstd_c + bh) in float64;  gate |got - ref| <= 32 e32 with e32 the
             deviation of the same expression in torch fp32 (a C-term fp32 sum; sigmoid's slope is <= 1/4).
  uncentred  the register-table kernel (16-bit, C = 8 G or 16 G) and stats_mask_small form the logit as
             sum cf h - K, K = sum cf mean (documented in ops.hip: one FMA per channel), so their error follows the
             partial sums of cf h and cf mean, not of cf (h - mean).  With |mean| >> std they exceed 32 e32 (measured
             3.4e-6 against 1.2e-6), and at HW = 1, where rstd = 1 / sqrt(eps) = 316, by far (3.7e-5 against 1.2e-6).
             For these two kernels the gate adds the running error bound of both sums in the kernel's own order
             (aad_cases.uncentred_term); the centred LDS-table kernel keeps the gate above.

test_every_variant_was_launched closes the file: the signatures the cases above logged must cover every kernel,
type and parameter listed in REQUIRED.
"""
import pytest
import torch

import aad_cases as A

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32


@pytest.fixture(scope="module")
def lib():
    from ghost_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _lib.load()


SEEN = set()    # every AAD blend signature the cases of this module logged
RAN = set()     # ids of the blend cases that ran


# blend cases: aad_cases.CASES, the smallest shapes that select each variant of the planners aad_v3_plan and
# aad_wide_plan (tests/test_aad_plan_cpu.py checks the same signatures without a GPU)
CASES, _id, _tokens = A.CASES, A._id, A._tokens


def _gate(tag, got, ref, e32, s, dt, allow=None, tie=None):
    """The per-element gate of the module docstring; prints the figures it compares before it asserts.  ``allow``
    (aad_cases.tie_allowance) widens it for the elements behind an ambiguous storage rounding of the upsample."""
    assert bool(torch.isfinite(got).all()), tag
    den = ref.abs().clamp_min(1.0)
    err = (got.double().to(ref.device) - ref).abs() / den
    if dt == F32:
        print(f"AADFIG {tag} e32={e32:.3e} err={float(err.max()):.3e} bound={32 * e32:.3e}")
        assert float(err.max()) <= 32 * e32, (tag, float(err.max()), 32 * e32)
        return
    ulp = A.ULP[dt]
    bound = 0.5 + s / ulp + 32 * e32 / ulp
    if allow is None:
        print(f"AADFIG {tag} e32={e32 / ulp:.2e} s={s / ulp:.4f} err={float(err.max()) / ulp:.4f} bound={bound:.4f} (ulp)")
        assert float(err.max()) / ulp <= bound, (tag, float(err.max()) / ulp, bound)
        return
    clear = allow == 0        # elements no ambiguous rounding reaches: the plain gate
    over = err / ulp - allow / den / ulp
    print(f"AADFIG {tag} e32={e32 / ulp:.2e} s={s / ulp:.4f} err={float(err[clear].max()) / ulp:.4f} bound={bound:.4f} "
          f"(ulp); ties={int(tie.sum())} of {tie.numel()} reach {int((~clear).sum())} elements, worst there "
          f"err={float(err[~clear].max()) / ulp if bool((~clear).any()) else 0.0:.4f}, "
          f"err-allowance={float(over[~clear].max()) if bool((~clear).any()) else 0.0:.4f}")
    assert float(over.max()) <= bound, (tag, float(over.max()), bound)


# Measured on an MI355X, in ulp of the storage type, worst layer and case of each group.  e32 and s as the test
# computes them; err = the kernel's worst |got - ref64| / den over the elements no tie reaches; bound = the
# smallest 0.5 + s + 32 e32 of the group; tied = worst err of an element behind a tie, and what is left of it
# after its allowance (held to the same bound).  No variant needed a term of its own.
#   kernel        type  C     up  cases  e32      s      err     bound   tied (- allowance)
#   aad_v3        bf16  64    0   8      2.3e-4   -      0.4980  0.5051  -
#   aad_v3        f16   64    0   1      1.7e-3   -      0.4997  0.5449  -
#   aad_v3        f16   64    1   2      1.9e-3   0.064  0.5059  0.6048  1.251 (0.5099)
#   aad_v4        bf16  64    1   8      3.4e-4   0.062  0.5085  0.5403  0.839 (0.5024)
#   aad_v5        bf16  64    1   22     4.7e-4   0.037  0.5059  0.5248  1.739 (0.5008)
#   aad_v5        f16   64    1   1      2.9e-3   0.032  0.5045  0.6061  1.148 (0.5049)
#   aad_v3_wide   bf16  128   0   8      2.4e-4   -      0.4980  0.5049  -
#   aad_v3_wide   bf16  128   1   8      4.8e-4   0.084  0.5186  0.5774  0.749 (0.5129)
#   aad_v3_wide   f16   128   1   1      2.0e-3   0.086  0.5183  0.6201  0.909 (0.5145)
#   aad_v3_wide   bf16  256   0   4      2.8e-4   -      0.4980  0.5071  -
#   aad_v3_wide   f16   256   0   1      2.3e-3   -      0.4993  0.5746  -
#   aad_v5_wide   bf16  128   1   6      6.5e-4   0.154  0.5387  0.6124  2.009 (0.5212)
#   aad_v5_wide   f16   128   1   1      3.5e-3   0.085  0.5296  0.6984  1.465 (0.5235)
#   aad_wide      bf16  256   0   2      2.5e-4   -      0.4979  0.5080  -
#   aad_wide      bf16  512   0   2      2.0e-4   -      0.4977  0.5064  -
#   aad_wide      f16   256   0   1      2.0e-3   -      0.4988  0.5627  -
#   aad_wide_deep bf16  1024  0   2      6.4e-4   -      0.4980  0.5072  -
#   aad_wide_deep f16   1024  0   1      4.2e-3   -      0.4994  0.6358  -
#   aad_gemm      bf16  1024  0   2      8.5e-4   -      0.4980  0.5272  -
#   aad_gemm      f16   1024  0   1      1.0e-2   -      0.4992  0.8329  -
#   ghost_aad_layer_nhwc (test_aad_layer_vs_float64), fused 64 x 128 B = 4 / split 16 x 16 B = 2:
#     bf16  e32 1.8e-4 / 1.1e-4  err 0.4979 / 0.4967  bound 0.5055 / 0.5034
#     f16   e32 1.9e-3 / 1.0e-3  err 0.4995 / 0.4945  bound 0.5591 / 0.5299
#     f32   (absolute) e32 2.3e-6 / 1.4e-6  err 2.1e-6 / 9.9e-7  bound 7.3e-5 / 4.4e-5
# Ties: 1.0e-3 - 1.3e-3 of the bf16 and 6.3e-3 - 7.0e-3 of the fp16 elements of h_in are flagged; the project's
# upsample kernel rounds 9 of 1 M (bf16, 64 x 128), 629 of 33 M (bf16, v5_wide B = 64) and 515 of 8 M (fp16)
# elements differently from F.interpolate, all of them among the flagged.
@pytest.mark.parametrize("k", CASES, ids=_id)
def test_aad_layers_vs_float64(lib, k):
    data = A.make_case(k["c"], k["ca"], k["H"], k["W"], k["B"], k["L"], k["up"], k["dt"], DEV)
    outs, sigs = A.run_layers_v3(lib, data, k["slope"])
    SEEN.update(A.aad_sigs(sigs))
    RAN.add(_id(k))
    A.assert_plan(sigs, k["kernel"], _tokens(k))
    closed = k["up"] and A.closed_form_stats(k["dt"], k["H"] // 2, k["W"] // 2, k["c"], k["c"] + A.PAD)
    for l in range(k["L"]):
        assert outs[l].shape[-1] == k["c"] + A.PAD * (l + 1)
        assert A.pads_intact(outs[l], k["c"]), l
        ref, e32, s, allow, tie = A.reference(data, l, k["slope"], k["cpu"])
        _gate(f"{_id(k)} l={l}", outs[l][..., :k["c"]], ref, e32, s if closed else 0.0, k["dt"], allow, tie)


# ghost_aad_layer_nhwc (the AADLayer module's entry): the fused kernel where B * HW / 64 >= 512 workgroups, else
# the mask pass + the GEMM with the blend epilogue
LAYER_CASES = [(dt, H, W, B, slope, fused) for dt in (F32, BF, HF) for slope in (0.0, 1.0)
               for H, W, B, fused in ((64, 128, 4, True), (16, 16, 2, False))]


@pytest.mark.parametrize("dt,H,W,B,slope,fused", LAYER_CASES,
                         ids=[f"{A.TNAME[c[0]]}-{c[1]}x{c[2]}-B{c[3]}-slope{c[4]:g}" for c in LAYER_CASES])
def test_aad_layer_vs_float64(lib, dt, H, W, B, slope, fused):
    data = A.make_case(64, 64, H, W, B, 1, 0, dt, DEV, seed=3)
    outs, sigs = A.run_layer(lib, data, slope)
    SEEN.update(A.aad_sigs(sigs))
    if fused:
        A.assert_plan(sigs, "aad_fused", [f"t={A.TNAME[dt]}", "BM=64", "C=64", "Ca=64"])
    else:
        assert not A.aad_sigs(sigs), sigs
    assert A.pads_intact(outs[0], 64)
    ref, e32 = A.reference(data, 0, slope, True)[:2]
    _gate(f"aad_layer-{A.TNAME[dt]}-{H}x{W}-B{B}-slope{slope:g}", outs[0][..., :64], ref, e32, 0.0, dt)


def test_reference_expression_matches_the_oracle(lib):
    """The device evaluation of the large cases (aad_cases.aad_expr, float64) is the oracle's aad_layer: the two
    agree to 1e-12 relative on a through-upsample case, with the layer's own and with substituted statistics
    of the same tensor."""
    data = A.make_case(128, 64, 32, 128, 2, 1, 1, BF, DEV)
    p = data["layers"][0]
    for slope in (0.0, 1.0):
        on_dev = A.aad_expr(data["h"], data["za"].double(), data["zi"], p, slope).cpu()
        on_dev_stats = A.aad_expr(data["h"], data["za"].double(), data["zi"], p, slope, stats=A.stats_of(data["h"])).cpu()
        oracle = A.aad_oracle(data["h"].cpu(), data["za"].double().cpu(), data["zi"].cpu(),
                              {k: v.cpu() for k, v in p.items()}, slope, 32, 128)
        den = oracle.abs().clamp_min(1.0)
        assert float(((on_dev - oracle).abs() / den).max()) <= 1e-12
        assert float(((on_dev_stats - oracle).abs() / den).max()) <= 1e-12


# ----------------------------------------------------------------------------------------
# mask kernels
# ----------------------------------------------------------------------------------------
def _mask_inputs(dt, C, HW, B, L, offset):
    g = torch.Generator().manual_seed(C * 131 + HW * 7 + L)
    b = torch.arange(B, dtype=torch.float32).view(B, 1, 1)
    if offset:      # |mean| >> std: the register kernel's sum_c cf_c h_c - K form cancels
        h = torch.randn(B, HW, C, generator=g) * 0.3 + 5.0 + 0.5 * b
    else:
        h = torch.randn(B, HW, C, generator=g) * (1.25 + 0.25 * b) + 0.7 - 0.3 * b
    whs = [torch.randn(C, generator=g) * (2.0 / (C + 1)) ** 0.5 for _ in range(L)]
    bhs = [torch.randn(1, generator=g) * 0.7 for _ in range(L)]
    return h.to(dt), whs, bhs


def _mask_gate(tag, masks, h, mean, rstd, whs, bhs, kernel):
    """|got - ref64| <= 32 e32 per element, plus aad_cases.uncentred_term for the kernels that form the logit as
    sum cf h - K (``kernel`` "reg" / "small"; "lds": the centred LDS-table kernel); prints the figures first."""
    B, HW, _ = h.shape
    for l, m in enumerate(masks):
        assert float(m[-1]) == A.SENTINEL, (tag, l)       # the element after the last pixel
        got = m[:-1].view(B, HW).double()
        ref = A.mask_expr(h.double(), mean, rstd, whs[l].double(), bhs[l].double())
        m32 = A.mask_expr(h.float(), mean.float(), rstd.float(), whs[l], bhs[l])
        e32 = float((m32.double() - ref).abs().max())
        err = (got - ref).abs()
        term = torch.zeros_like(err) if kernel == "lds" else A.uncentred_term(
            h.double(), mean, rstd, whs[l].double(), bhs[l].double(), kernel, 4 if h.dtype == F32 else 8)
        print(f"AADFIG {tag} l={l} e32={e32:.3e} err={float(err.max()):.3e} 32e32={32 * e32:.3e} "
              f"uncentred={float(term.max()):.3e}")
        assert bool(torch.isfinite(got).all()) and bool((err <= 32 * e32 + term).all()), (tag, l, float(err.max()))


# dtype, C, offset: C = 64 lane groups smaller than a wave (16-bit: register kernel with G = 8); C = 512 / 1024 the
# register kernel with NCH = 1 / 2 (fp32: the LDS-table kernel); C = 32 in fp32 the LDS-table kernel with G = 8
MASK_CASES = [(dt, C, False) for dt in (F32, BF, HF) for C in (64, 512, 1024)] + [(F32, 32, False)] + \
             [(BF, 1024, True), (HF, 512, True), (F32, 512, True)]
# Measured on an MI355X (absolute, over the cases of each group; uncentred = the derived term, 0 for the LDS kernel):
#   kernel (small = 0)          e32              err      32 e32 (least)  uncentred
#   LDS, f32, every C           4.3e-8 - 1.3e-7  1.4e-7   1.4e-6          0
#   LDS, f32, C 512, offset     4.3e-8 - 1.3e-7  1.0e-7   1.4e-6          0
#   register, bf16 / f16        4.6e-8 - 1.7e-7  2.0e-7   1.5e-6          9.3e-7 - 6.4e-6
#   register, bf16 1024 offset  6.9e-8 - 1.2e-7  2.8e-6   2.2e-6          7.2e-5 - 1.4e-4
#   register, f16 512 offset    3.6e-8 - 1.7e-7  3.4e-6   1.2e-6          4.0e-5 - 8.4e-5
#   stats_mask_small (small = 1), every type
#   HW 4 / 16, C 64             3.4e-8 - 9.0e-8  2.6e-7   1.1e-6          1.2e-6 - 2.9e-6
#   HW 4 / 16, C 1024           5.0e-8 - 1.4e-7  1.7e-7   1.6e-6          3.7e-6 - 6.2e-6
#   HW 1, C 64                  6.7e-10 - 1.7e-8 9.6e-6   2.1e-8          4.4e-4 - 1.0e-3
#   HW 1, C 1024                2.1e-8 - 4.5e-8  3.7e-5   6.6e-7          1.7e-3 - 1.8e-3
# The offset and HW = 1 rows are the ones that need the uncentred term (module docstring); elsewhere the kernels
# sit a factor of ten inside 32 e32.


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("HW", [63, 4])    # 63 = 7 x 9: HW % ppb != 0 and no multiple of a pass; 4: ppb clamped to HW
@pytest.mark.parametrize("dt,C,offset", MASK_CASES,
                         ids=[f"{A.TNAME[c[0]]}-C{c[1]}{'-offset' if c[2] else ''}" for c in MASK_CASES])
def test_aad_mask_vs_float64(lib, dt, C, offset, HW, L):
    B = 3
    h, whs, bhs = _mask_inputs(dt, C, HW, B, L, offset)
    mean64, rstd64 = A.stats_of(h.double())
    stat = torch.stack([mean64.view(B, C), rstd64.view(B, C)], -1).float()      # the kernel's input, fp32
    rc, masks, _ = A.run_mask(lib, dt, h, stat, whs, bhs, small=0)
    assert rc == 0
    _mask_gate(f"mask-{A.TNAME[dt]}-C{C}-HW{HW}-L{L}{'-offset' if offset else ''}", masks, h,
               stat[..., 0].double().view(B, 1, C), stat[..., 1].double().view(B, 1, C), whs, bhs,
               "lds" if dt == F32 else "reg")      # 16-bit at these C: the register-table kernel


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("HW", [1, 4, 16])
@pytest.mark.parametrize("C", [64, 1024])
@pytest.mark.parametrize("dt", [F32, BF, HF], ids=lambda d: A.TNAME[d])
def test_stats_mask_small_vs_float64(lib, dt, C, HW, L):
    B = 3
    h, whs, bhs = _mask_inputs(dt, C, HW, B, L, False)
    rc, masks, stat = A.run_mask(lib, dt, h, None, whs, bhs, small=1)
    assert rc == 0
    mean, rstd = A.stats_of(h.double())
    st = stat.double()
    torch.testing.assert_close(st[..., 0], mean.view(B, C), atol=1e-5, rtol=1e-6)      # test_instnorm_stats' bounds
    torch.testing.assert_close(st[..., 1], rstd.view(B, C), atol=0, rtol=2e-4)
    # the masks against the statistics the kernel returned (held to float64 above), as the small = 0 gate feeds
    # fp32 statistics to kernel and reference alike
    _mask_gate(f"small-{A.TNAME[dt]}-C{C}-HW{HW}-L{L}", masks, h, st[..., 0].view(B, 1, C), st[..., 1].view(B, 1, C),
               whs, bhs, "small")


def test_stats_mask_small_rejects_an_8x8_image(lib):
    """HW = 64 is outside stats_mask_small_ok: GHOST_EINVAL and nothing launched (stat and mask untouched)."""
    h, whs, bhs = _mask_inputs(BF, 64, 64, 3, 1, False)
    rc, masks, stat = A.run_mask(lib, BF, h, None, whs, bhs, small=1)
    assert rc == -1
    assert bool((masks[0] == A.SENTINEL).all()) and bool(torch.isnan(stat).all())


# ----------------------------------------------------------------------------------------
# coverage: what the plan log has shown across this module
# ----------------------------------------------------------------------------------------
REQUIRED = [("aad_v3", "C=64", "up=0"), ("aad_v3", "C=64", "up=1"), ("aad_v3_wide", "C=128", "up=0"),
            ("aad_v3_wide", "C=128", "up=1"), ("aad_v3_wide", "C=256"), ("aad_v4",),
            ("aad_v5", "v5_ipw=1"), ("aad_v5", "v5_ipw=2"),
            ("aad_v5_wide", "v5_ipw=1"), ("aad_v5_wide", "v5_ipw=2"), ("aad_v5_wide", "v5_ipw=4"),
            ("aad_wide", "C=256"), ("aad_wide", "C=512"), ("aad_wide_deep",), ("aad_gemm",),
            ("aad_fused", "t=f32"), ("aad_fused", "t=bf16"), ("aad_fused", "t=f16")] + \
           [(name, "slope0=0") for name in ("aad_v3", "aad_v3_wide", "aad_v4", "aad_v5", "aad_v5_wide")] + \
           [(name, "slope0=1") for name in ("aad_v3", "aad_v3_wide", "aad_v4", "aad_v5", "aad_v5_wide")] + \
           [(name, f"L={L}") for name in ("aad_v3", "aad_v3_wide", "aad_v4", "aad_v5", "aad_v5_wide") for L in (1, 2)] + \
           [(name, "t=f16") for name in ("aad_v3", "aad_v3_wide", "aad_v5", "aad_v5_wide", "aad_wide", "aad_wide_deep",
                                         "aad_gemm")]


def test_every_variant_was_launched(lib):
    """A planner change that silently stops selecting a variant fails here.  Cases of this module that did not
    run in this session (a filtered run) are launched now, without their reference."""
    for k in CASES:
        if _id(k) not in RAN:
            data = A.make_case(k["c"], k["ca"], k["H"], k["W"], k["B"], k["L"], k["up"], k["dt"], DEV)
            SEEN.update(A.aad_sigs(A.run_layers_v3(lib, data, k["slope"])[1]))
    for dt in (F32, BF, HF):
        if not any(s.startswith("aad_fused") and f"t={A.TNAME[dt]}" in s.split() for s in SEEN):
            SEEN.update(A.aad_sigs(A.run_layer(lib, A.make_case(64, 64, 64, 128, 4, 1, 0, dt, DEV, seed=3), 0.0)[1]))
    missing = [r for r in REQUIRED if not any(s.split()[0] == r[0] and all(t in s.split() for t in r[1:]) for s in SEEN)]
    assert not missing, (missing, sorted(SEEN))
