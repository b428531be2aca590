"""Op tests of the use_sr kernels (csrc/sr.hip) on an MI355X: ghost_norm_modulate_nhwc and ghost_lip_pool_nhwc
against a float64 reference of the same expression, per element, for fp32 / bf16 / fp16 storage.

Gate (the rule of tests/test_aad_ops.py), den = max(1, |ref64|), ulp = 2^-7 (bf16) / 2^-10 (fp16):
    16-bit   |got - ref64| / den <= (0.5 + 32 e32) ulp
    fp32     |got - ref64| / den <= 32 e32
0.5: the one rounding at the store.  e32: the error of the same expression evaluated by torch in fp32 on the same
(storage-rounded) inputs, computed in the test; the factor 32 covers the kernel's other association / FMA
contraction and its expf / division.  Inputs, gamma / beta and the source are pre-rounded to the storage type;
statistics and the LIP affine are fp32 on both sides.
Every output buffer has ldo = C + 8 with a sentinel in the pad channels that must survive bit for bit.
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
        print(f"SRFIG {tag} e32={e32:.3e} err={err:.3e} bound={32 * e32:.3e}")
        assert err <= 32 * e32, (tag, err, 32 * e32)
    else:
        u = ULP[dt]
        print(f"SRFIG {tag} e32={e32 / u:.2e} err={err / u:.4f} bound={0.5 + 32 * e32 / u:.4f} (ulp)")
        assert err / u <= 0.5 + 32 * e32 / u, (tag, err / u, 0.5 + 32 * e32 / u)


def _e32(o32, ref):
    return float(((o32.double() - ref).abs() / ref.abs().clamp_min(1.0)).max())


def _pads_intact(out, c):
    it = torch.int16 if out.element_size() == 2 else torch.int32
    want = torch.full((), SENTINEL, dtype=out.dtype).view(it)
    return bool((out[..., c:].contiguous().view(it).cpu() == want).all())


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


# ---------------------------------------------------------------------------------------------------------
# ghost_norm_modulate_nhwc
# ---------------------------------------------------------------------------------------------------------
def _modulate_expr(src, mean, rstd, gamma, beta, slope):
    v = (src - mean) * rstd
    if gamma is not None:
        v = v * gamma + beta
    return F.leaky_relu(v, slope) if slope != 1.0 else v


def _run_modulate(lib, dt, B, H, W, Cn, bs, gb, slope, up2x, ldx_pad, seed):
    """-> (got [B,H,W,C] on the host, ref64, e32, signatures).  H, W: output size (the source is half with up2x)."""
    from ghost_amd import _lib
    g = torch.Generator().manual_seed(seed)
    hs, ws = (H // 2, W // 2) if up2x else (H, W)
    ldx = Cn + ldx_pad
    srcb = torch.full((B, hs, ws, ldx), float("nan"))
    srcb[..., :Cn] = torch.randn(B, hs, ws, Cn, generator=g) * 1.5 + 0.3
    srcb = srcb.to(dt)
    stat = torch.stack([torch.randn(bs, Cn, generator=g) * 0.5, torch.rand(bs, Cn, generator=g) * 2 + 0.25], -1)
    gbt = (torch.randn(B, H, W, 2 * Cn, generator=g) * 0.8).to(dt) if gb else None
    out = torch.full((B, H, W, Cn + PAD), SENTINEL, dtype=dt, device=DEV)
    sd, std, gbd = srcb.to(DEV), stat.contiguous().to(DEV), (gbt.to(DEV) if gb else None)
    sigs = _logged(lambda: _lib.check(lib.ghost_norm_modulate_nhwc(
        _lib.gdtype(dt), sd.data_ptr(), ldx, B, H, W, Cn, std.data_ptr(), bs, _lib.ptr(gbd), 2 * Cn, slope,
        1 if up2x else 0, out.data_ptr(), Cn + PAD, _stream()), "norm_modulate"))
    assert _pads_intact(out, Cn)

    def expr(t):
        s = srcb[..., :Cn].to(t)
        if up2x:
            s = s.repeat_interleave(2, 1).repeat_interleave(2, 2)       # nearest x2
        st = stat.to(t)
        idx = slice(None) if bs == B else slice(0, 1)
        mean, rstd = st[idx, :, 0].view(-1, 1, 1, Cn), st[idx, :, 1].view(-1, 1, 1, Cn)
        ga, be = (gbt[..., :Cn].to(t), gbt[..., Cn:].to(t)) if gb else (None, None)
        return _modulate_expr(s, mean, rstd, ga, be, slope)
    ref = expr(torch.float64)
    return out[..., :Cn].cpu(), ref, _e32(expr(torch.float32), ref), sigs


MOD_CASES = [
    # B, H, W, C, Bs ("b": batch record / "i": per sample), gb, slope, up2x, ldx pad
    (2, 4, 6, 48, "i", False, 0.0, False, 0),      # the encoder's InstanceNorm + ReLU
    (2, 4, 6, 48, "i", False, 1.0, False, 0),      # ... without ReLU (last encoder stage)
    (2, 4, 6, 48, "b", True, 0.2, False, 0),       # SPADE + leaky ReLU
    (2, 4, 6, 768, "b", True, 0.2, False, 0),
    (2, 4, 6, 768, "b", True, 1.0, False, 8),      # norm_s (no activation), ldx > C view
    (2, 4, 6, 768, "i", True, 0.0, False, 0),
    (2, 4, 6, 48, "b", False, 0.2, False, 8),
    (3, 5, 7, 48, "b", True, 0.2, False, 0),       # 105 pixels: no multiple of any tile
    (3, 5, 7, 48, "i", True, 1.0, False, 8),
    (2, 4, 6, 48, "b", True, 0.2, True, 0),        # nearest x2 folded into the read: [2,2,3,C] -> 4 x 6
    (2, 4, 6, 768, "b", True, 0.2, True, 8),
    (2, 4, 6, 768, "i", False, 0.0, True, 0),
]


@pytest.mark.parametrize("dt", [F32, BF, HF], ids=lambda d: TNAME[d])
@pytest.mark.parametrize("case", MOD_CASES, ids=lambda c: "B{}_{}x{}_C{}_{}_gb{:d}_s{}_up{:d}_pad{}".format(*c))
def test_norm_modulate_vs_float64(lib, case, dt):
    B, H, W, Cn, bsk, gb, slope, up2x, pad = case
    bs = B if bsk == "i" else 1
    got, ref, e32, sigs = _run_modulate(lib, dt, B, H, W, Cn, bs, gb, slope, up2x, pad, seed=Cn + H + 7 * W + bs)
    assert sigs == [f"norm_modulate t={TNAME[dt]} vec={4 if dt == F32 else 8} gb={int(gb)} up2x={int(up2x)} "
                    f"stat={'instance' if bs == B else 'batch'}"], sigs
    _gate(f"modulate {case} {TNAME[dt]}", got, ref, e32, dt)


def test_norm_modulate_einval(lib):
    from ghost_amd import _lib
    x = torch.zeros(2, 4, 6, 64, device=DEV)
    st = torch.ones(2, 64, 2, device=DEV)
    o = torch.zeros(2, 4, 6, 64, device=DEV)

    def call(src=x, C_=48, H=4, W=6, stat=st, out=o, up=0, bs=1, ldx=64):
        return lib.ghost_norm_modulate_nhwc(_lib.F32, _lib.ptr(src), ldx, 2, H, W, C_, _lib.ptr(stat), bs, None, 0, 1.0,
                                            up, _lib.ptr(out), 64, _stream())
    assert call() == 0
    assert call(C_=44) == -1                      # C not a multiple of 8
    assert call(H=3, up=1) == -1 and call(W=5, up=1) == -1      # odd H / W with up2x
    assert call(src=None) == -1 and call(stat=None) == -1 and call(out=None) == -1
    assert call(bs=3) == -1                       # Bs must be 1 or B
    assert call(ldx=50) == -1                     # rows not 16-byte aligned
    assert "norm_modulate" in lib.ghost_last_error().decode()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------
# ghost_lip_pool_nhwc
# ---------------------------------------------------------------------------------------------------------
def _lip_expr(x, lr, mean, rstd, w, b):
    """NHWC in, NHWC out; zero padding in both sums (the /9 of avg_pool cancels)."""
    logit = 12.0 * torch.sigmoid(((lr - mean) * rstd) * w + b)
    e = logit.exp().permute(0, 3, 1, 2)
    xe = x.permute(0, 3, 1, 2) * e
    num = F.avg_pool2d(xe, 3, 2, 1, divisor_override=1)
    den = F.avg_pool2d(e, 3, 2, 1, divisor_override=1)
    return (num / den).permute(0, 2, 3, 1)


LIP_CASES = [(2, 2, 2, 48), (1, 4, 6, 96), (2, 16, 16, 768)]      # [2,2,2,48]: every window touches padding


@pytest.mark.parametrize("dt", [F32, BF, HF], ids=lambda d: TNAME[d])
@pytest.mark.parametrize("case", LIP_CASES, ids=lambda c: "B{}_{}x{}_C{}".format(*c))
def test_lip_pool_vs_float64(lib, case, dt):
    from ghost_amd import _lib
    B, H, W, Cn = case
    g = torch.Generator().manual_seed(H * 31 + Cn)
    x = (torch.randn(B, H, W, Cn, generator=g) * 1.2 + 0.2).to(dt)
    # logits at both sigmoid extremes: normalised values of +-8 and more make l = 12 and l = 0, so windows mix
    # weights e^12 = 1.6e5 and 1
    lr = (torch.randn(B, H, W, Cn, generator=g) * 6.0).to(dt)
    stat = torch.stack([torch.randn(B, Cn, generator=g) * 0.3, torch.rand(B, Cn, generator=g) + 0.75], -1).contiguous()
    w = torch.rand(Cn, generator=g) + 0.5
    b = torch.randn(Cn, generator=g) * 0.2
    ldx, ldl = Cn + 8, Cn + 16
    xb = torch.full((B, H, W, ldx), float("nan"), dtype=dt)
    xb[..., :Cn] = x
    lb = torch.full((B, H, W, ldl), float("nan"), dtype=dt)
    lb[..., :Cn] = lr
    out = torch.full((B, H // 2, W // 2, Cn + PAD), SENTINEL, dtype=dt, device=DEV)
    xd, ld, sd, wd, bd = xb.to(DEV), lb.to(DEV), stat.to(DEV), w.to(DEV), b.to(DEV)
    sigs = _logged(lambda: _lib.check(lib.ghost_lip_pool_nhwc(
        _lib.gdtype(dt), xd.data_ptr(), ldx, ld.data_ptr(), ldl, B, H, W, Cn, sd.data_ptr(), wd.data_ptr(),
        bd.data_ptr(), out.data_ptr(), Cn + PAD, _stream()), "lip_pool"))
    assert sigs == [f"lip_pool t={TNAME[dt]} vec={4 if dt == F32 else 8} k=3 s=2"], sigs
    assert _pads_intact(out, Cn)

    def expr(t):
        return _lip_expr(x.to(t), lr.to(t), stat[:, :, 0].to(t).view(B, 1, 1, Cn), stat[:, :, 1].to(t).view(B, 1, 1, Cn),
                         w.to(t), b.to(t))
    ref = expr(torch.float64)
    lg = 12.0 * torch.sigmoid(((lr.double() - stat[:, :, 0].double().view(B, 1, 1, Cn))
                               * stat[:, :, 1].double().view(B, 1, 1, Cn)) * w.double() + b.double())
    assert float(lg.max()) > 11.99 and float(lg.min()) < 0.01        # both extremes occur
    _gate(f"lip_pool {case} {TNAME[dt]}", out[..., :Cn].cpu(), ref, _e32(expr(torch.float32), ref), dt)


def test_lip_pool_einval(lib):
    from ghost_amd import _lib
    x = torch.zeros(2, 4, 6, 64, device=DEV)
    st = torch.ones(2, 64, 2, device=DEV)
    wb = torch.ones(64, device=DEV)
    o = torch.zeros(2, 2, 3, 64, device=DEV)

    def call(xx=x, lg=x, H=4, W=6, C_=48, stat=st, w=wb, b=wb, out=o, ldx=64):
        return lib.ghost_lip_pool_nhwc(_lib.F32, _lib.ptr(xx), ldx, _lib.ptr(lg), 64, 2, H, W, C_, _lib.ptr(stat),
                                       _lib.ptr(w), _lib.ptr(b), _lib.ptr(out), 64, _stream())
    assert call() == 0
    assert call(H=3) == -1 and call(W=5) == -1    # odd H / W
    assert call(C_=44) == -1
    for k in ("xx", "lg", "stat", "w", "b", "out"):
        assert call(**{k: None}) == -1, k
    assert call(ldx=50) == -1
    assert "lip_pool" in lib.ghost_last_error().decode()
    torch.cuda.synchronize()
