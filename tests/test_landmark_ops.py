"""Op tests of ghost_dwsep_block_nhwc (csrc/lmk.hip) on an MI355X: the depthwise-separable block of the landmark
network against float64, per element, for fp32 / bf16 / fp16 storage.

Gate (the rule of tests/test_sr_ops.py), den = max(1, |ref64|), ulp = 2^-7 (bf16) / 2^-10 (fp16):
    16-bit   |got - ref64| / den <= (0.5 + 32 e32) ulp
    fp32     |got - ref64| / den <= 32 e32
0.5: the one rounding at the store.  e32: the error of the same expression evaluated by torch in fp32 on the same
inputs, computed in the test; the factor 32 covers the kernel's other association and FMA contraction.
* the depthwise stage (the Cout = 0 launch, and the tap of the fused launch) is gated against float64 of
  PReLU(BN(depthwise3x3(x))) on the storage-rounded x;
* the pointwise stage is gated against float64 evaluated on the kernel's own tap, so a rounding tie in the depthwise
  stage cannot be charged to the GEMM;
* the fused launch gives the same bytes with and without the tap; the plan log names the kernel.
The input has ldx = Cin + 8 with NaN in the pad channels; every output buffer has ld = C + 8 with a sentinel in the
pad channels that must survive bit for bit.  Shapes: Cin = 16 is half an MFMA K step; 36 and 35 pixels are no multiple
of the 16 / 32 row tile; Cout = 512 takes four column tiles, 32 and 64 fewer column tiles than waves.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
ULP = {BF: 2.0 ** -7, HF: 2.0 ** -10}
TNAME = {F32: "f32", BF: "bf16", HF: "f16"}
SENTINEL = -77.0
PAD = 8

# B, H, W, Cin, Cout, stride
CASES = [(1, 6, 6, 512, 512, 1), (3, 12, 12, 256, 512, 2), (2, 20, 20, 16, 32, 1), (1, 18, 22, 32, 64, 2),
         (2, 7, 5, 64, 64, 1), (2, 7, 5, 64, 64, 2)]


@pytest.fixture(scope="module")
def lib():
    from ghost_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _lib.load()


def _logged(call):
    from ghost_amd import _lib
    _lib.plan_log(True)
    try:
        call()
        torch.cuda.synchronize()
    finally:
        _lib.plan_log(False)
    return _lib.plan_log_read()


def _gate(tag, got, ref, e32, dt):
    assert bool(torch.isfinite(got).all()), tag
    den = ref.abs().clamp_min(1.0)
    err = float(((got.double() - ref).abs() / den).max())
    if dt == F32:
        print(f"LMKFIG {tag} e32={e32:.3e} err={err:.3e} bound={32 * e32:.3e}")
        assert err <= 32 * e32, (tag, err, 32 * e32)
    else:
        u = ULP[dt]
        print(f"LMKFIG {tag} e32={e32 / u:.2e} err={err / u:.4f} bound={0.5 + 32 * e32 / u:.4f} (ulp)")
        assert err / u <= 0.5 + 32 * e32 / u, (tag, err / u, 0.5 + 32 * e32 / u)


def _e32(o32, ref):
    return float(((o32.double() - ref).abs() / ref.abs().clamp_min(1.0)).max())


def _pads_intact(out, c):
    it = torch.int16 if out.element_size() == 2 else torch.int32
    want = torch.full((), SENTINEL, dtype=out.dtype).view(it)
    return bool((out[..., c:].contiguous().view(it).cpu() == want).all())


def _rup(v, m):
    return (v + m - 1) // m * m


def _bn_prelu(v, sc, sh, pr):
    """channels last"""
    v = v * sc + sh
    return torch.where(v > 0, v, v * pr)


def _dw_expr(x, w, sc, sh, pr, stride, t):
    """x [B,H,W,C], w [C,1,3,3] -> [B,Ho,Wo,C] in dtype t"""
    v = F.conv2d(x.to(t).permute(0, 3, 1, 2), w.to(t), stride=stride, padding=1, groups=x.shape[3]).permute(0, 2, 3, 1)
    return _bn_prelu(v, sc.to(t), sh.to(t), pr.to(t))


def _pw_expr(d, w, sc, sh, pr, t):
    return _bn_prelu(d.to(t) @ w.to(t).t(), sc.to(t), sh.to(t), pr.to(t))


@pytest.mark.parametrize("dt", [F32, BF, HF], ids=lambda d: TNAME[d])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "B{}_{}x{}_{}to{}_s{}".format(*c))
def test_dwsep_block_vs_float64(lib, case, dt):
    from ghost_amd import _lib
    B, H, W, Ci, Co, s = case
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    g = torch.Generator().manual_seed(1000 * Ci + 10 * H + W + s)
    x = (torch.randn(B, H, W, Ci, generator=g) * 1.2 + 0.1).to(dt)
    xb = torch.full((B, H, W, Ci + PAD), float("nan"), dtype=dt)
    xb[..., :Ci] = x
    dww = torch.randn(Ci, 1, 3, 3, generator=g) * (2.0 / 9.0) ** 0.5
    dsc, dsh, dpr = torch.rand(Ci, generator=g) * 0.6 + 0.7, torch.randn(Ci, generator=g) * 0.1, \
        torch.rand(Ci, generator=g) * 0.4 + 0.05
    pww = (torch.randn(Co, Ci, generator=g) * (2.0 / Ci) ** 0.5).to(dt)
    psc, psh, ppr = torch.rand(Co, generator=g) * 0.6 + 0.7, torch.randn(Co, generator=g) * 0.1, \
        torch.rand(Co, generator=g) * 0.4 + 0.05
    kpad = _rup(Ci, 32)
    wp = torch.zeros(_rup(Co, 128), kpad, dtype=dt)
    wp[:Co, :Ci] = pww
    d = {k: v.contiguous().to(DEV) for k, v in dict(
        x=xb, dww=dww.reshape(Ci, 9).t(), dsc=dsc, dsh=dsh, dpr=dpr, w=wp, psc=psc, psh=psh, ppr=ppr).items()}
    gd = _lib.gdtype(dt)
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def run(cout, tap):
        y = torch.full((B, Ho, Wo, (cout or Ci) + PAD), SENTINEL, dtype=dt, device=DEV)
        t = torch.full((B, Ho, Wo, Ci + PAD), SENTINEL, dtype=dt, device=DEV) if tap else None
        sigs = _logged(lambda: _lib.check(lib.ghost_dwsep_block_nhwc(
            gd, d["x"].data_ptr(), B, H, W, Ci, Ci + PAD, s, d["dww"].data_ptr(), d["dsc"].data_ptr(),
            d["dsh"].data_ptr(), d["dpr"].data_ptr(), d["w"].data_ptr() if cout else None, cout, kpad if cout else 0,
            d["psc"].data_ptr() if cout else None, d["psh"].data_ptr() if cout else None,
            d["ppr"].data_ptr() if cout else None, y.data_ptr(), y.shape[3], _lib.ptr(t), Ci + PAD if tap else 0,
            stream), "dwsep_block"))
        assert _pads_intact(y, cout or Ci) and (t is None or _pads_intact(t, Ci))
        return y, t, sigs

    bm = 16 if dt == F32 else 32
    mtail = int((B * Ho * Wo) % bm != 0)
    y_tap, tap, sig_tap = run(Co, True)
    y, _, sig = run(Co, False)
    ydw, _, sig_dw = run(0, False)
    want = f"dwsep_block t={TNAME[dt]} fused s={s} cin={Ci} cout={Co} bm={bm} bn={min(Co, 128)} kp={kpad} tap=%d mtail={mtail}"
    assert sig_tap == [want % 1] and sig == [want % 0], (sig_tap, sig)
    assert sig_dw == [f"dwsep_block t={TNAME[dt]} dw_only s={s} cin={Ci} bm={bm}"], sig_dw
    it = torch.int16 if dt != F32 else torch.int32
    assert torch.equal(y_tap.view(it), y.view(it)), "the tap changed the output"
    assert torch.equal(tap.view(it), ydw.view(it)), "the depthwise-only launch and the tap differ"

    tag = f"{case} {TNAME[dt]}"
    ref_dw = _dw_expr(x, dww, dsc, dsh, dpr, s, torch.float64)
    _gate(f"dw {tag}", tap[..., :Ci].cpu(), ref_dw, _e32(_dw_expr(x, dww, dsc, dsh, dpr, s, torch.float32), ref_dw), dt)
    own = tap[..., :Ci].cpu()
    ref_pw = _pw_expr(own, pww, psc, psh, ppr, torch.float64)
    _gate(f"pw {tag}", y[..., :Co].cpu(), ref_pw, _e32(_pw_expr(own, pww, psc, psh, ppr, torch.float32), ref_pw), dt)


def test_dwsep_block_einval(lib):
    from ghost_amd import _lib
    x = torch.zeros(1, 6, 6, 32, device=DEV)
    v = torch.ones(128, device=DEV)
    w9 = torch.zeros(9, 32, device=DEV)
    w = torch.zeros(128, 32, device=DEV)
    y = torch.zeros(1, 6, 6, 64, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def call(xx=x, Ci=32, Co=64, s=1, ldx=32, kpad=32, ldy=64, tap=None, pw=w):
        return lib.ghost_dwsep_block_nhwc(_lib.F32, _lib.ptr(xx), 1, 6, 6, Ci, ldx, s, w9.data_ptr(), v.data_ptr(),
                                          v.data_ptr(), v.data_ptr(), _lib.ptr(pw), Co, kpad, v.data_ptr(),
                                          v.data_ptr(), v.data_ptr(), y.data_ptr(), ldy, _lib.ptr(tap), 32, stream)
    assert call() == 0
    assert call(xx=None) == -1 and call(pw=None) == -1
    assert call(Ci=20) == -1 and call(Co=24) == -1           # Cin % 8, Cout % 16
    assert call(s=3) == -1 and call(ldx=30) == -1 and call(ldy=32) == -1
    assert call(kpad=16) == -1                                # Kpad % 32
    assert call(Co=0, tap=y) == -1                            # no tap without a pointwise stage
    assert "ghost_dwsep_block_nhwc" in lib.ghost_last_error().decode()
    torch.cuda.synchronize()
