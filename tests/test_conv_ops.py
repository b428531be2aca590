"""Op tests of the convolution kernels off the implicit GEMM (MI355X): halo, halo_pp, convT_halo, s2_patch, first and
stem3x3, every production variant pinned by its plan-log line, against a float64 reference of the same operation,
per element.  The cases are conv_cases.FAMILY_CASES (tests/test_conv_plan_cpu.py checks the same signatures without a
GPU); the implicit GEMM's own edge classes are gated in tests/test_gpu_parity.py, its split-K fix-up (arrival counters)
and its mixed-type instances in tests/test_fused_reduce_ops.py.

  reference  F.conv2d / F.conv_transpose2d and the epilogue of include/ghost_amd.h (ghost_conv_epi) in float64 on the
             CPU; x, w and the residual pre-rounded to the storage type, scale, shift, PReLU, scale2 and shift2 the
             fp32 values the kernel gets.
  gate       per element, den = max(1, |ref64|), ulp = 2^-7 (bf16) / 2^-10 (fp16):
               16-bit   |got - ref64| / den <= (0.5 + 32 e32 / ulp) ulp
               fp32     |got - ref64| / den <= 32 e32
             0.5: the one round-to-nearest at the store.  e32: the worst |ref32 - ref64| / den of the same expression
             in torch fp32 (computed in the test); the factor 32 is the one test_aad_ops.py allows another fp32
             summation order.  y2 goes through the same gate against ref64 * scale2 + shift2 with its own e32: the
             kernels form it from the unrounded fp32 value, and half an ulp of y carried into y2 would not pass.
             No variant needed a term of its own: the tanh_out case (tanhf on the fp32 value, a few fp32 ulp of a
             result below 1) sits inside the gate like the others.
  also       the plan log holds exactly one conv kernel line, the expected one with its tokens, and no
             splitk_reduce; y is pre-filled with NaN and has ldy > N with a sentinel in the pad channels and in the
             pixels after the last sample (where a tile overhanging the image of the last sample would write) that
             must survive bit for bit; y2 has its own ldy2 = N + 16 and sentinels; the residual its own
             ldres = N + 4; cases with ldx > Cin read a channel slice of a buffer whose other channels hold finite
             junk; every sample of a batch differs.
  STATS      ghost_conv2d_stats_nhwc (the persistent kernel with the InstanceNorm partials + in_stats_from_tiles, as
             the generator's conv3x3 runs it): y through the same gate, stat against the float64 mean and rstd of
             the kernel's own stored y (the kernel reads the rounded values back) within test_instnorm_stats' bounds.
  dead rows  halo_fn's table (conv_halo.hip) also instantiates tile=Img8 with NCB=6, with and without STATS;
             halo_plan takes Img8 at a power-of-two NCB only, so nothing selects those rows and no case can.

test_every_variant_was_launched closes the file: the signatures logged above must cover REQUIRED.
"""
import ctypes
import zlib

import pytest
import torch
import torch.nn.functional as F

import aad_cases as A
import conv_cases as K

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
CONV_KERNELS = ("halo", "halo_pp", "convT_halo", "s2_patch", "first", "stem3x3", "glds", "igemm")
LDY2_PAD, LDRES_PAD = 16, 4
IN_EPS = 1e-5       # ops.hip kInEps


@pytest.fixture(scope="module")
def lib():
    from ghost_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _lib.load()


SEEN = set()    # every conv signature the cases of this module logged
RAN = set()     # (case id, type) of the cases that ran

ROWS = [pytest.param(c, t, id=f"{K.case_id(c)}-{t}") for c in K.FAMILY_CASES for t in c["types"]]


def _out_hw(c):
    if c["kind"] == "T":
        return 2 * c["H"], 2 * c["W"]
    return (c["H"] + 2 * c["p"] - c["k"]) // c["s"] + 1, (c["W"] + 2 * c["p"] - c["k"]) // c["s"] + 1


def make_inputs(c, dt):
    """The case's operands on the CPU: x, w and the residual rounded to the storage type, the epilogue tables fp32.
    He-scaled weights and unit-variance inputs; randn gives every sample its own image, and sample b its own gain."""
    m = K.MODES[c["mode"]]
    B, cin, n, k = c["B"], c["cin"], c["n"], c["k"]
    # a STATS twin gets its plain case's operands
    g = torch.Generator().manual_seed(zlib.crc32(repr([c[f] for f in ("B", "H", "W", "cin", "n", "mode", "k", "s", "kind",
                                                                         "ldx", "ldy")]).encode()))
    gain = 1.0 + 0.25 * torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1) / B
    x = torch.randn(B, cin, c["H"], c["W"], generator=g) * gain
    if c["kind"] == "T":
        w = torch.randn(cin, n, 4, 4, generator=g) * (2.0 / (cin * 4)) ** 0.5      # four taps reach an output
    else:
        w = torch.randn(n, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    Ho, Wo = _out_hw(c)
    d = dict(x=x.to(dt), w=w.to(dt), w_raw=w)
    d["sc"], d["sh"] = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g) * 0.1
    d["pr"] = torch.rand(n, generator=g) * 0.5
    d["sc2"], d["sh2"] = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g) * 0.1
    d["res"] = torch.randn(B, n, Ho, Wo, generator=g).to(dt) if m.get("res") else None
    d["junk"] = torch.randn(B, c["H"], c["W"], c["ldx"] - cin, generator=g) * 3.0 if c["ldx"] > cin else None
    return d


def expression(c, d, P):
    """(y, y2 or None) of the case in precision P: the epilogue of ghost_conv_epi, in its order."""
    m = K.MODES[c["mode"]]

    def ch(t):
        return t.to(P).view(1, -1, 1, 1)
    x, w = d["x"].to(P), d["w"].to(P)
    v = F.conv_transpose2d(x, w, stride=2, padding=1) if c["kind"] == "T" else F.conv2d(x, w, stride=c["s"], padding=c["p"])
    if m["bn"]:
        v = v * ch(d["sc"]) + ch(d["sh"])
    r = d["res"].to(P) if m.get("res") else None
    if m.get("res_first"):
        v = v + r
    if m.get("prelu"):
        v = torch.where(v > 0, v, v * ch(d["pr"]))
    elif m["slope"] != 1.0:
        v = torch.where(v > 0, v, v * m["slope"])
    if m.get("res") and not m.get("res_first"):
        v = v + r
    if m.get("tanh"):
        v = torch.tanh(v)
    return v, (v * ch(d["sc2"]) + ch(d["sh2"]) if m.get("y2") else None)


def reference(c, d):
    """[(ref64, e32)] for y and, where the case has one, y2."""
    out = []
    for r64, r32 in zip(expression(c, d, torch.float64), expression(c, d, torch.float32)):
        if r64 is not None:
            out.append((r64, float(((r32.double() - r64).abs() / r64.abs().clamp_min(1.0)).max())))
    return out


def _padded_nhwc(t, ld, guard, fill, pad_fill, dt):
    """NCHW values (or None: ``fill`` everywhere) -> a flat [pixels + guard][ld] device buffer of type dt: the pad
    channels and the guard pixels after the last sample hold ``pad_fill``."""
    B, n, H, W = t if isinstance(t, tuple) else t.shape
    buf = torch.full((B * H * W + guard, ld), pad_fill, dtype=dt)
    buf[:B * H * W, :n] = fill if isinstance(t, tuple) else t.permute(0, 2, 3, 1).reshape(B * H * W, n)
    return buf.to(DEV)


def run(lib, c, dt, d):
    """Launch the case -> dict(sigs, y [B,N,Ho,Wo] on the CPU, y2, stat, intact)."""
    from ghost_amd import _lib
    from ghost_amd.network.pack import pack_conv, pack_convT4x4, rup
    m = K.MODES[c["mode"]]
    B, H, W, cin, n, ldx, ldy = c["B"], c["H"], c["W"], c["cin"], c["n"], c["ldx"], c["ldy"]
    Ho, Wo = _out_hw(c)
    M, guard = B * Ho * Wo, 64 * max(Wo, 16)
    xb = torch.empty(B, H, W, ldx, dtype=dt)
    xb[..., :cin] = d["x"].permute(0, 2, 3, 1)
    if ldx > cin:
        xb[..., cin:] = d["junk"].to(dt)
    xb = xb.to(DEV)
    wp = (pack_convT4x4 if c["kind"] == "T" else pack_conv)(d["w_raw"], dt).to(DEV)

    def table(t):
        o = torch.zeros(rup(n, 128), device=DEV)
        o[:n] = t.to(DEV)
        return o
    sc, sh, pr, sc2, sh2 = (table(d[k_]) for k_ in ("sc", "sh", "pr", "sc2", "sh2"))
    y = _padded_nhwc((B, n, Ho, Wo), ldy, guard, float("nan"), A.SENTINEL, dt)
    ldy2, ldres = n + LDY2_PAD, n + LDRES_PAD
    y2 = _padded_nhwc((B, n, Ho, Wo), ldy2, guard, float("nan"), A.SENTINEL, dt) if m.get("y2") else None
    res = _padded_nhwc(d["res"], ldres, guard, None, 3.0, dt) if m.get("res") else None
    stat = torch.full((B, n, 2), float("nan"), device=DEV) if c["stats"] else None
    ws = torch.empty(8 << 20, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    g = _lib.gdtype(dt)
    if c["kind"] == "T":
        assert not (m.get("prelu") or m.get("y2") or m.get("tanh") or m.get("res_first"))

        def call():
            return lib.ghost_conv_transpose4x4s2_nhwc(
                g, xb.data_ptr(), B, H, W, cin, ldx, wp.data_ptr(), n, wp.shape[1], wp.shape[2],
                sc.data_ptr() if m["bn"] else None, sh.data_ptr() if m["bn"] else None, m["slope"], _lib.ptr(res), ldres,
                y.data_ptr(), ldy, ws.data_ptr(), ws.numel(), s)
    else:
        e = _lib.ConvEpi()
        if m["bn"]:
            e.scale, e.shift = sc.data_ptr(), sh.data_ptr()
        e.slope = m["slope"]
        if m.get("prelu"):
            e.prelu = pr.data_ptr()
        if m.get("res"):
            e.res, e.ldres, e.res_first = res.data_ptr(), ldres, int(bool(m.get("res_first")))
        e.tanh_out = int(bool(m.get("tanh")))
        if m.get("y2"):
            e.y2, e.ldy2, e.scale2, e.shift2 = y2.data_ptr(), ldy2, sc2.data_ptr(), sh2.data_ptr()
        head = (g, xb.data_ptr(), B, H, W, cin, ldx, wp.data_ptr(), n, wp.shape[0], wp.shape[1], c["k"], c["k"], c["s"],
                c["p"], ctypes.byref(e), y.data_ptr(), ldy)

        def call():
            if c["stats"]:
                return lib.ghost_conv2d_stats_nhwc(*head, stat.data_ptr(), ws.data_ptr(), ws.numel(), s)
            return lib.ghost_conv2d_ex_nhwc(*head, ws.data_ptr(), ws.numel(), s)
    try:
        sigs = A.logged_call(lambda: _lib.check(call(), K.case_id(c)))
    except RuntimeError as ex:
        if str(ex).startswith("ghost_amd"):
            raise
        pytest.exit(f"device error in {K.case_id(c)}: {ex}", returncode=3)      # no further launch on a faulted device
    out = dict(sigs=sigs, stat=None if stat is None else stat.cpu())
    intact = True
    for name, buf in (("y", y), ("y2", y2)):
        if buf is None:
            out[name] = None
            continue
        host = buf.cpu()
        intact = intact and bool((host[:M, n:] == A.SENTINEL).all()) and bool((host[M:] == A.SENTINEL).all())
        out[name] = host[:M, :n].view(B, Ho, Wo, n).permute(0, 3, 1, 2)
    out["intact"] = intact
    return out


def conv_sigs(sigs):
    return [s for s in sigs if s.split()[0] in CONV_KERNELS]


def assert_plan(sigs, c, t):
    """Exactly one conv kernel ran, the case's, with its tokens, and nothing reduced split-K partials."""
    conv = conv_sigs(sigs)
    assert len(conv) == 1 and conv[0].split()[0] == c["tokens"][0], (c["tokens"], sigs)
    assert all(tok in conv[0].split() for tok in K.case_tokens(c, t)), (K.case_tokens(c, t), conv[0])
    assert not any(s.startswith("splitk_reduce") for s in sigs), sigs


def _gate(tag, got, ref, e32, dt):
    """The per-element gate of the module docstring; prints the figures it compares before it asserts."""
    assert bool(torch.isfinite(got).all()), tag
    err = float(((got.double() - ref).abs() / ref.abs().clamp_min(1.0)).max())
    if dt == torch.float32:
        print(f"CONVFIG {tag} e32={e32:.3e} err={err:.3e} bound={32 * e32:.3e}")
        assert err <= 32 * e32, (tag, err, 32 * e32)
        return
    ulp = A.ULP[dt]
    bound = 0.5 + 32 * e32 / ulp
    print(f"CONVFIG {tag} e32={e32 / ulp:.2e} err={err / ulp:.4f} bound={bound:.4f} (ulp)")
    assert err / ulp <= bound, (tag, err / ulp, bound)


# Measured on an MI355X, in ulp of the storage type (f32: absolute), worst case of each kernel and type: e32 as the
# test computes it, err = the kernel's worst |got - ref64| / den, bound = the smallest 0.5 + 32 e32 of the group.
#   kernel            STATS  out  type  cases  e32      err      bound
#   halo_pp Wide      0      y    bf16  8      2.0e-04  0.4981   0.5038
#   halo_pp Wide      0      y    f16   8      3.6e-03  0.5003   0.5630
#   halo_pp Img8      0      y    bf16  6      1.8e-04  0.4969   0.5024
#   halo_pp Img8      0      y    f16   6      2.1e-03  0.4988   0.5428
#   halo_pp Small     0      y    bf16  8      2.3e-04  0.4981   0.5035
#   halo_pp Small     0      y    f16   8      3.0e-03  0.4996   0.5698
#   halo_pp Small     0      y2   bf16  1      2.4e-04  0.4980   0.5077
#   halo_pp Small     0      y2   f16   1      3.4e-03  0.4997   0.6104
#   halo_pp Pair      0      y    bf16  8      2.5e-04  0.4982   0.5045
#   halo_pp Pair      0      y    f16   8      3.2e-03  0.5001   0.5803
#   halo_pp Pair      0      y2   bf16  2      2.5e-04  0.4981   0.5079
#   halo_pp Pair      0      y2   f16   2      3.8e-03  0.4998   0.6145
#   halo Wide         0      y    bf16  6      1.8e-04  0.4981   0.5047
#   halo Wide         0      y    f16   6      3.2e-03  0.4997   0.5899
#   halo Wide         0      y2   bf16  1      1.8e-04  0.4981   0.5056
#   halo Wide         0      y2   f16   1      3.7e-03  0.4987   0.6184
#   halo Small        0      y    bf16  3      1.8e-04  0.4981   0.5037
#   halo Small        0      y    f16   3      2.6e-03  0.4992   0.5770
#   convT_halo BN64   0      y    bf16  2      2.3e-04  0.4980   0.5048
#   convT_halo BN64   0      y    f16   2      3.6e-03  0.4996   0.5948
#   convT_halo BN32   0      y    bf16  2      1.3e-04  0.4980   0.5042
#   convT_halo BN32   0      y    f16   2      2.8e-03  0.4997   0.5754
#   s2_patch K4       0      y    bf16  2      1.7e-04  0.4980   0.5047
#   s2_patch K4       0      y    f16   2      4.0e-03  0.4994   0.5855
#   s2_patch K3       0      y    bf16  3      1.2e-04  0.4980   0.5032
#   s2_patch K3       0      y    f16   3      2.3e-03  0.4943   0.5475
#   s2_patch K3       0      y2   bf16  1      1.2e-04  0.4972   0.5040
#   s2_patch K3       0      y2   f16   1      2.8e-03  0.4961   0.5891
#   first mfma        0      y    bf16  2      4.1e-05  0.4971   0.5006
#   first mfma        0      y    f16   2      7.8e-04  0.4968   0.5138
#   first scalar      0      y    bf16  2      4.0e-05  0.4970   0.5006
#   first scalar      0      y    f16   2      8.1e-04  0.4906   0.5085
#   first scalar      0      y    f32   2      1.2e-06  1.2e-06  1.4e-05
#   stem3x3           0      y    bf16  3      3.9e-05  0.4976   0.5008
#   stem3x3           0      y2   bf16  2      2.8e-05  0.4966   0.5009
#   halo_pp Wide      1      y    bf16  8      2.0e-04  0.4981   0.5038
#   halo_pp Wide      1      y    f16   8      3.6e-03  0.5003   0.5630
#   halo_pp Img8      1      y    bf16  6      1.8e-04  0.4969   0.5024
#   halo_pp Img8      1      y    f16   6      2.1e-03  0.4988   0.5428
# stat of the STATS cases against the float64 statistics of the stored y (bounds: mean 1e-5 + 1e-6 |mean|, rstd 2e-4
# relative), worst case per tile and type:
#   halo_pp Wide  bf16  cases 8  mean abs 3.8e-08  rstd rel 8.2e-08
#   halo_pp Wide  f16   cases 8  mean abs 4.8e-08  rstd rel 8.5e-08
#   halo_pp Img8  bf16  cases 6  mean abs 3.7e-08  rstd rel 1.4e-07
#   halo_pp Img8  f16   cases 6  mean abs 6.0e-08  rstd rel 1.2e-07
@pytest.mark.parametrize("c,t", ROWS)
def test_conv_family_vs_float64(lib, c, t):
    dt = DT[t]
    d = make_inputs(c, dt)
    out = run(lib, c, dt, d)
    SEEN.update(conv_sigs(out["sigs"]))
    RAN.add((K.case_id(c), t))
    assert_plan(out["sigs"], c, t)
    assert out["intact"], "wrote outside its channel slice or past the last sample"
    refs = reference(c, d)
    tag = f"{K.case_id(c)}-{t}"
    _gate(tag, out["y"], refs[0][0], refs[0][1], dt)
    if out["y2"] is not None:
        _gate(tag + " y2", out["y2"], refs[1][0], refs[1][1], dt)
    if c["stats"]:
        var, mean = torch.var_mean(out["y"].double(), dim=(2, 3), unbiased=False)
        st, rstd = out["stat"].double(), 1.0 / torch.sqrt(var + IN_EPS)
        print(f"CONVFIG {tag} stat mean abs={float((st[..., 0] - mean).abs().max()):.2e} "
              f"rstd rel={float(((st[..., 1] - rstd).abs() / rstd).max()):.2e}")
        torch.testing.assert_close(st[..., 0], mean, atol=1e-5, rtol=1e-6)       # test_instnorm_stats' bounds
        torch.testing.assert_close(st[..., 1], rstd, atol=0, rtol=2e-4)


def test_stats_entry_refuses_a_plan_without_partials(lib):
    """A tile=Pair shape writes no InstanceNorm partials: ghost_conv2d_stats_nhwc returns GHOST_EINVAL and launches
    nothing (y and stat untouched); a workspace shorter than the partials is GHOST_ENOWS with the need named."""
    from ghost_amd import _lib
    from ghost_amd.network.pack import pack_conv
    dt = torch.bfloat16
    e = _lib.ConvEpi()
    e.slope = 1.0
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream

    def attempt(B, H, W, cin, n, ws_bytes):
        x = torch.zeros(B, H, W, cin, dtype=dt, device=DEV)
        wp = pack_conv(torch.zeros(n, cin, 3, 3), dt).to(DEV)
        y = torch.full((B, H, W, n), A.SENTINEL, dtype=dt, device=DEV)
        stat = torch.full((B, n, 2), float("nan"), device=DEV)
        sigs = []

        def call():
            sigs.append(lib.ghost_conv2d_stats_nhwc(_lib.BF16, x.data_ptr(), B, H, W, cin, cin, wp.data_ptr(), n, wp.shape[0],
                                                    wp.shape[1], 3, 3, 1, 1, ctypes.byref(e), y.data_ptr(), n, stat.data_ptr(),
                                                    ws.data_ptr(), ws_bytes, s))
        logged = A.logged_call(call)
        assert not logged, logged
        assert bool((y == A.SENTINEL).all()) and bool(torch.isnan(stat).all())
        return sigs[0], lib.ghost_last_error().decode()
    rc, _ = attempt(128, 14, 14, 64, 256, ws.numel())      # FAMILY_CASES' first tile=Pair shape
    assert rc == -1                                         # GHOST_EINVAL
    need = 32 * 8 * 128 * 2 * 4 + 256                       # the Wide sweep's shape: B x 8 records x N x (mean, M2)
    rc, msg = attempt(32, 16, 32, 64, 128, need - 1)
    assert rc == -3 and str(need) in msg, (rc, msg)         # GHOST_ENOWS


# ----------------------------------------------------------------------------------------
# coverage: what the plan log has shown across this module
# ----------------------------------------------------------------------------------------
_NCB = {"Wide": (2, 4, 6, 8, 16, 32), "Img8": (2, 4, 8, 16, 32), "Small": (2, 4, 6, 8, 16, 32), "Pair": (2, 4, 6, 8, 16, 32)}
REQUIRED = [r + (f"t={t}",) for t in K.T16 for r in
            [("halo_pp", f"tile={tile}", f"NCB={ncb}", "STATS=0") for tile, ncbs in _NCB.items() for ncb in ncbs] +
            [("halo_pp", f"tile={tile}", f"NCB={ncb}", "STATS=1") for tile in ("Wide", "Img8") for ncb in _NCB[tile]] +
            [("halo_pp", f"tile={tile}", "RESW=1", f"STATS={st}") for tile in ("Wide", "Img8") for st in (0, 1)] +
            [("halo_pp", "tile=Small", "RESW=1"), ("halo_pp", "tile=Small", "RESW=0"),
             ("halo_pp", "tile=Small", "overhang=0"), ("halo_pp", "tile=Small", "overhang=1"),
             ("halo_pp", "tile=Pair", "overhang=1"),
             ("halo_pp", "tile=Wide", "uneven=1", "STATS=0"), ("halo_pp", "tile=Wide", "uneven=1", "STATS=1"),
             ("halo_pp", "tile=Wide", "uneven=0"),
             ("halo", "tile=Wide", "overhang=0"), ("halo", "tile=Wide", "N=576"), ("halo", "tile=Wide", "Cin=96"),
             ("halo", "tile=Wide", "Cin=32"), ("halo", "tile=Small", "overhang=0"), ("halo", "tile=Small", "overhang=1"),
             ("halo", "tile=Small", "N=576"),
             ("convT_halo", "BN=64", "res=0"), ("convT_halo", "BN=64", "res=1"), ("convT_halo", "BN=32", "res=0"),
             ("convT_halo", "BN=32", "res=1"),
             ("s2_patch", "K=4", "ncb=1"), ("s2_patch", "K=4", "ncb=2"), ("s2_patch", "K=3", "overhang=0"),
             ("s2_patch", "K=3", "overhang=1"),
             ("first", "mfma", "chunktail=0"), ("first", "mfma", "chunktail=1"), ("first", "scalar", "mtail=0"),
             ("first", "scalar", "mtail=1")]] + \
           [("first", "scalar", "t=f32", "mtail=0"), ("first", "scalar", "t=f32", "mtail=1"),
            ("stem3x3", "y2=1", "mtail=1", "chunktail=1"), ("stem3x3", "y2=0", "mtail=0", "chunktail=0"),
            ("stem3x3", "y2=1", "mtail=0", "chunktail=1")]


def test_every_variant_was_launched(lib):
    """A planner change that silently stops selecting a variant fails here.  Cases of this module that did not
    run in this session (a filtered run) are launched now, without their reference."""
    for c in K.FAMILY_CASES:
        for t in c["types"]:
            if (K.case_id(c), t) not in RAN:
                SEEN.update(conv_sigs(run(lib, c, DT[t], make_inputs(c, DT[t]))["sigs"]))
    missing = [r for r in REQUIRED if not any(s.split()[0] == r[0] and all(t in s.split() for t in r[1:]) for s in SEEN)]
    assert not missing, (missing, sorted(SEEN))
