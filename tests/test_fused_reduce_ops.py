"""Op tests of the device code that only the network runtimes select (MI355X): the last-arriver reductions (the
split-K fix-up inside both GEMM kernels, standard and AAD form; the fused final pass of the InstanceNorm statistics) and
the GEMMs whose output type differs from their operand type.  They run through the test-support entries
ghost_conv_rt_nhwc, ghost_aad_layer_rt_nhwc and ghost_instnorm_stats_rt_nhwc, which take the arrival counters and the
second type that the public entries never pass.  The cases are conv_cases.FIXUP_CASES / FIXUP_AAD_CASES / LINEAR_CASES /
HEAD_CASES and stats_cases.CASES; tests/test_conv_plan_cpu.py and tests/test_stats_plan_cpu.py check the same plans
without a GPU.

  GEMMs      the layout of test_gpu_parity.test_igemm_edge_plans: operands rounded to storage, float64 reference, y
             pre-filled with NaN, ldy > N with sentinels that must survive, for kind=T4S2 the slice layout of
             test_convT_op.  The plan log holds exactly the expected GEMM line, no splitk_reduce* line when the plan
             fuses and the named one when not.  Gates, the project's own: test_gpu_parity._ulp_gate (1.01 ulp) for a
             16-bit GEMM of one type; test_conv_ops._gate for the rest ((0.5 + 32 e32 / ulp) ulp for fp32 -> 16-bit,
             32 e32 for an fp32 output, e32 the error of the same expression in torch fp32); test_aad_ops._gate for
             the AAD form.
  statistics the bounds of test_gpu_parity.test_instnorm_stats and test_instnorm_stats_of_virtual_upsample, inputs
             with |mean| >> std as there.  fp16 (not run there) takes the bf16 bounds with the storage step of fp16
             in place of bf16's: 2^-10 for 2^-7 at 2 <= |x| < 4.
  every case that has counters
             1. its bytes equal those of the same call with sem = NULL (the code claims the same sums in the same
                order), stat included;
             2. the counters are nsem zero words followed by guard words: after the call the first nsem are zero
                and the guards intact;
             3. a second call on the same counters and workspace, not zeroed again, gives the same bytes;
             4. every sample of a batch differs.
             The workspace is filled with 0xFF bytes (NaN partials) before the first call.

test_every_fused_signature_was_launched closes the file: the GEMM lines logged above must cover every fixup=std /
fixup=aad line of DESIGN.md section 2 (those lines hold batch-independent tokens only).

Classes that no accepted shape selects, read from the planners:
  * 16-bit operands -> fp32 from fp16: igemm_plan takes the pair for ti == bf16 only (f32_from16); the entry
    refuses fp16 -> fp32 and launches nothing (asserted below).
  * fixup=aad on the deep ring with a column tile beyond C_aad: the deep ring wants N = 2 C a multiple of 128, so
    every column tile is whole; the register-staged 64x128 tile at C = 32 covers the class.
  * several M tiles under a fix-up outside the 256x16 tile: a whole tile's partials of two splits must fit 32 KB
    (GHOST_SPLIT_FUSE_KB), 2 x BM x BN x 4 bytes: only BM x BN <= 4096, the 256x16 tile, admits M > BM.
  * short=1 with fp32 operands: the register-staged kernel's prologue is one K step, no split is shorter.
"""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import aad_cases as A
import conv_cases as K
import stats_cases as S
from test_aad_ops import _gate as aad_gate
from test_conv_ops import _gate as conv_gate
from test_gpu_parity import _logged_call, _ulp_gate

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
SENTINEL = 7.0
GUARD, PATTERN = 8, 0x5A5A5A5A          # guard words after the counters
WS_BYTES = 16 << 20
SLOPE = 0.2


@pytest.fixture(scope="module")
def lib():
    from ghost_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _lib.load()


SEEN = set()    # every GEMM line the cases of this module logged
RAN = set()     # ids of the GEMM cases that ran


def stream():
    return torch.cuda.current_stream().cuda_stream


def new_ws():
    return torch.full((WS_BYTES,), 0xFF, dtype=torch.uint8, device=DEV)


def new_counters(nsem):
    t = torch.zeros(nsem + GUARD, dtype=torch.int32, device=DEV)
    t[nsem:] = PATTERN
    return t


def counters_clean(t, nsem):
    return bool((t[:nsem] == 0).all()) and bool((t[nsem:] == PATTERN).all())


def raw(t):
    """The bytes of a tensor (NaN-safe equality)."""
    return t.contiguous().view(torch.uint8)


def gemm_lines(sigs):
    return [s for s in sigs if s.split()[0] in ("glds", "igemm")]


def reduce_lines(sigs):
    return [s for s in sigs if s.startswith("splitk_reduce")]


def has(sig, tokens):
    return all(t in sig.split() for t in tokens)


def fused_contract(run, nsem, tag):
    """run(sem, nsem, ws) -> ([output tensors], sigs).  Points 1-3 of the module docstring; returns the outputs and
    the plan log of the first call with counters."""
    base, _ = run(None, 0, new_ws())
    cnt, ws = new_counters(nsem), new_ws()
    outs, sigs = run(cnt, nsem, ws)
    assert counters_clean(cnt, nsem), f"{tag}: counters not left at zero, or a guard word written"
    for o, b in zip(outs, base):
        assert torch.equal(raw(o), raw(b)), f"{tag}: bytes differ from the call without counters"
    again, _ = run(cnt, nsem, ws)
    assert counters_clean(cnt, nsem), f"{tag}: counters after the second call"
    for o, b in zip(again, outs):
        assert torch.equal(raw(o), raw(b)), f"{tag}: the second call on the same counters differs"
    return outs, sigs


def samples_differ(ref):
    return all(not torch.equal(ref[0], ref[b]) for b in range(1, ref.shape[0]))


def e32_of(ref32, ref64):
    return float(((ref32.double() - ref64).abs() / ref64.abs().clamp_min(1.0)).max())


def gemm_gate(tag, got, ref, e32, ti, to):
    if ti == to and to != torch.float32:
        _ulp_gate(got.float().cpu(), ref, to)
    else:
        conv_gate(tag, got.float().cpu(), ref, e32, to)


# ----------------------------------------------------------------------------------------
# split-K fix-up, standard epilogue
# ----------------------------------------------------------------------------------------
def conv_data(c, dt):
    """Inputs of a FIXUP / HEAD case, every sample different, and (ref64 NCHW, e32) of conv + scale / shift / leaky."""
    from ghost_amd.network.pack import pack_conv, pack_convT4x4, rup
    B, H, W, cin, n, k = c["B"], c["H"], c["W"], c["cin"], c["n"], c["k"]
    T = c["kind"] == "T"
    g = torch.Generator().manual_seed(cin * 31 + n * 7 + H * 3 + W + c["split_k"])
    b = torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1)
    x = (torch.randn(B, cin, H, W, generator=g) * (1.0 + 0.25 * b) + 0.1 * b).to(dt)
    kk = 16 if T else k * k
    w = (torch.randn(*((cin, n, 4, 4) if T else (n, cin, k, k)), generator=g) * (2.0 / (cin * kk)) ** 0.5).to(dt)
    sc = torch.rand(n, generator=g) + 0.5
    sh = torch.randn(n, generator=g) * 0.1

    def expr(ft):
        y = F.conv_transpose2d(x.to(ft), w.to(ft), stride=2, padding=1) if T else \
            F.conv2d(x.to(ft), w.to(ft), stride=c["s"], padding=c["p"])
        return F.leaky_relu(y * sc.to(ft).view(1, -1, 1, 1) + sh.to(ft).view(1, -1, 1, 1), c.get("slope", SLOPE))
    ref = expr(torch.float64)
    scp = torch.zeros(rup(n, 128), device=DEV); scp[:n] = sc.to(DEV)
    shp = torch.zeros(rup(n, 128), device=DEV); shp[:n] = sh.to(DEV)
    wp = (pack_convT4x4(w.float(), dt) if T else pack_conv(w.float(), dt)).to(DEV)
    return dict(x=x.permute(0, 2, 3, 1).contiguous().to(DEV), wp=wp, sc=scp, sh=shp, ref=ref, e32=e32_of(expr(torch.float32), ref))


def conv_rt(lib, c, d, ti, to, ldy_pad):
    """run(sem, nsem, ws) of fused_contract for a conv case through ghost_conv_rt_nhwc."""
    from ghost_amd import _lib
    n, T = c["n"], c["kind"] == "T"
    Ho, Wo = d["ref"].shape[2:]
    wp = d["wp"]
    e = _lib.ConvEpi()
    e.scale, e.shift, e.slope, e.split_k = d["sc"].data_ptr(), d["sh"].data_ptr(), c.get("slope", SLOPE), c["split_k"]

    def run(sem, nsem, ws, rc=0):
        y = torch.full((c["B"], Ho, Wo, n + ldy_pad), float("nan"), dtype=to, device=DEV)
        y[..., n:] = SENTINEL

        def call():
            r = lib.ghost_conv_rt_nhwc(_lib.gdtype(ti), _lib.gdtype(to), 1 if T else 0, d["x"].data_ptr(), c["B"], c["H"],
                                       c["W"], c["cin"], c["cin"], wp.data_ptr(), n, wp.shape[-2], wp.shape[-1], c["k"],
                                       c["k"], c["s"], c["p"], ctypes.byref(e), y.data_ptr(), n + ldy_pad, ws.data_ptr(),
                                       ws.numel(), None if sem is None else sem.data_ptr(), nsem, stream())
            assert r == rc, (r, lib.ghost_last_error())
        return [y], _logged_call(call)
    return run


def run_fixup_case(lib, c, t, check):
    dt = DT[t]
    d = conv_data(c, dt)
    tag = f"fixup-{c['name']}-{t}"
    run = conv_rt(lib, c, d, dt, dt, K.CONVT_LDY_PAD if c["kind"] == "T" else K.IGEMM_LDY_PAD)
    (y,), sigs = fused_contract(run, c["nsem"], tag)
    SEEN.update(gemm_lines(sigs))
    RAN.add(("fix", c["name"], t))
    if not check:
        return
    want = c["tokens_f32"] if t == "f32" else K.gemm_tokens(c["tokens"], t)
    assert len(gemm_lines(sigs)) == 1 and has(gemm_lines(sigs)[0], want), (want, sigs)
    if "fixup=none" in c["tokens"]:
        assert reduce_lines(sigs) == [f"{c['reduce']} to={t} epi=STD"], sigs
    else:
        assert not reduce_lines(sigs), sigs
    # the same call without counters runs the same GEMM unfused and the case's reduction kernel
    _, plain = run(None, 0, new_ws())
    assert has(gemm_lines(plain)[0], ("fixup=none",)) and reduce_lines(plain) == [f"{c['reduce']} to={t} epi=STD"], plain
    got = y.float().cpu()
    assert torch.all(got[..., c["n"]:] == SENTINEL), "wrote outside its channel slice"
    assert c["B"] == 1 or samples_differ(d["ref"])
    gemm_gate(tag, y[..., :c["n"]].permute(0, 3, 1, 2), d["ref"], d["e32"], dt, dt)


FIXUP_ROWS = [pytest.param(c, t, id=f"{c['name']}-{t}") for c in K.FIXUP_CASES for t in c["types"]]


@pytest.mark.parametrize("c,t", FIXUP_ROWS)
def test_split_fixup_std(lib, c, t):
    run_fixup_case(lib, c, t, True)


# ----------------------------------------------------------------------------------------
# split-K fix-up, AAD epilogue (ghost_aad_layer_rt_nhwc: statistics, mask, GEMM, all with the counters)
# ----------------------------------------------------------------------------------------
def run_aad_case(lib, row, t, check):
    name, tokens, tokens_f32, B, H, W, c, ca, split_k, _ = row
    dt = DT[t]
    slope = 1.0 if H == 4 else 0.0      # AADLayer alone / with the ReLU that follows it
    data = A.make_case(c, ca, H, W, B, 1, 0, dt, DEV, seed=11)
    tag = f"fixup-aad-{name}-{t}"
    (out,), sigs = fused_contract(
        lambda sem, nsem, ws: A.run_layer(lib, data, slope, rt=dict(split_k=split_k, sem=sem, nsem=nsem, ws=ws)), K.NSEM, tag)
    SEEN.update(gemm_lines(sigs))
    RAN.add(("aad", name, t))
    if not check:
        return
    want = tokens_f32 if t == "f32" else K.gemm_tokens(tokens, t)
    assert len(gemm_lines(sigs)) == 1 and has(gemm_lines(sigs)[0], want), (want, sigs)
    assert not reduce_lines(sigs) and not A.aad_sigs(sigs), sigs
    assert A.pads_intact(out, c)
    assert B == 1 or samples_differ(data["h"])
    ref, e32 = A.reference(data, 0, slope, True)[:2]
    aad_gate(tag, out[..., :c], ref, e32, 0.0, dt)


AAD_ROWS = [pytest.param(r, t, id=f"{r[0]}-{t}") for r in K.FIXUP_AAD_CASES for t in r[9]]


@pytest.mark.parametrize("row,t", AAD_ROWS)
def test_split_fixup_aad(lib, row, t):
    run_aad_case(lib, row, t, True)


# ----------------------------------------------------------------------------------------
# mixed types: fp32 operands -> fp32 / bf16 / fp16 (ghost_linear_f32 and its split through the counters)
# ----------------------------------------------------------------------------------------
def run_linear_case(lib, row, to_name, check):
    from ghost_amd import _lib
    from ghost_amd.network.pack import pack_conv, rup
    name, B, Kc, N, split_k, nsem, tokens, reduce = row
    to = DT[to_name]
    tag = f"linear-{name}-{to_name}"
    g = torch.Generator().manual_seed(Kc * 13 + N + B)
    x = torch.randn(B, Kc, generator=g) * (1.0 + 0.25 * torch.arange(B).view(B, 1)) + 0.1
    w = torch.randn(N, Kc, generator=g) * (2.0 / Kc) ** 0.5
    bias = torch.randn(N, generator=g) * 0.3
    ref = x.double() @ w.double().t() + bias.double()
    e32 = e32_of(x @ w.t() + bias, ref)
    xd, wp = x.to(DEV), pack_conv(w.view(N, Kc, 1, 1), torch.float32).to(DEV)
    bp = torch.zeros(rup(N, 128), device=DEV); bp[:N] = bias.to(DEV)
    ldy = N + K.LINEAR_LDY_PAD
    e = _lib.ConvEpi()
    e.shift, e.slope, e.split_k = bp.data_ptr(), 1.0, split_k

    def run(sem, ns, ws, entry="rt"):
        y = torch.full((B, ldy), float("nan"), dtype=to, device=DEV)
        y[:, N:] = SENTINEL
        if entry == "linear":
            call = lambda: _lib.check(lib.ghost_linear_f32(xd.data_ptr(), B, Kc, wp.data_ptr(), N, wp.shape[0], wp.shape[1],  # noqa: E731
                                                           bp.data_ptr(), _lib.gdtype(to), y.data_ptr(), ldy, ws.data_ptr(),
                                                           ws.numel(), stream()))
        else:
            call = lambda: _lib.check(lib.ghost_conv_rt_nhwc(  # noqa: E731
                _lib.F32, _lib.gdtype(to), 0, xd.data_ptr(), B, 1, 1, Kc, Kc, wp.data_ptr(), N, wp.shape[0], wp.shape[1], 1,
                1, 1, 0, ctypes.byref(e), y.data_ptr(), ldy, ws.data_ptr(), ws.numel(),
                None if sem is None else sem.data_ptr(), ns, stream()))
        return [y], _logged_call(call)
    if nsem:
        (y,), sigs = fused_contract(run, nsem, tag)
    else:
        (y,), sigs = run(None, 0, new_ws(), "linear")
    SEEN.update(gemm_lines(sigs))
    RAN.add(("lin", name, to_name))
    if not check:
        return
    assert len(gemm_lines(sigs)) == 1 and has(gemm_lines(sigs)[0], ("to=" + to_name,) + tokens), (tokens, sigs)
    assert reduce_lines(sigs) == ([f"{reduce} to={to_name} epi=STD"] if reduce else []), sigs
    if split_k == 0:
        # ghost_linear_f32 is the same descriptor without counters: the same bytes
        (y_lin,), _ = run(None, 0, new_ws(), "linear")
        assert torch.equal(raw(y), raw(y_lin)), tag
    got = y.float().cpu()
    assert torch.all(got[:, N:] == SENTINEL), "wrote outside its channel slice"
    assert B == 1 or samples_differ(ref)
    gemm_gate(tag, y[:, :N], ref, e32, torch.float32, to)


LINEAR_ROWS = [pytest.param(r, to, id=f"{r[0]}-{to}") for r in K.LINEAR_CASES for to in ("f32", "bf16", "f16")]


@pytest.mark.parametrize("row,to", LINEAR_ROWS)
def test_linear_f32_mixed_output(lib, row, to):
    run_linear_case(lib, row, to, True)


# ----------------------------------------------------------------------------------------
# mixed types: 16-bit operands -> fp32 (the ArcFace head's form)
# ----------------------------------------------------------------------------------------
def head_case(n, B):
    return dict(name=f"head{n}", B=B, H=K.HEAD_HW, W=K.HEAD_HW, cin=K.HEAD_CIN, n=n, k=K.HEAD_HW, s=1, p=0, kind="fwd",
                split_k=0, slope=1.0)


@pytest.mark.parametrize("n,B,nsem", K.HEAD_CASES)
def test_bf16_gemm_with_fp32_output(lib, n, B, nsem):
    """splitk_reduce to=f32 from=bf16 applies the epilogue to the GEMM's fp32 partials; counters never fuse it and
    stay untouched."""
    c = head_case(n, B)
    d = conv_data(c, torch.bfloat16)
    run = conv_rt(lib, c, d, torch.bfloat16, torch.float32, K.IGEMM_LDY_PAD)
    tag = f"head-{n}-B{B}-nsem{nsem}"
    if nsem:
        (y,), sigs = fused_contract(run, nsem, tag)
    else:
        (y,), sigs = run(None, 0, new_ws())
    assert len(sigs) == 2 and has(sigs[0], K.HEAD_TOKENS + ("ntail=%d" % (n % 128 != 0),)) and sigs[1] == K.HEAD_REDUCE, sigs
    assert torch.all(y[..., n:].cpu() == SENTINEL), "wrote outside its channel slice"
    assert B == 1 or samples_differ(d["ref"])
    gemm_gate(tag, y[..., :n].permute(0, 3, 1, 2), d["ref"], d["e32"], torch.bfloat16, torch.float32)


def test_fp16_gemm_with_fp32_output_is_refused(lib):
    """No instance: GHOST_EINVAL, nothing launched, y untouched."""
    c = head_case(512, 1)
    d = conv_data(c, torch.float16)
    cnt = new_counters(K.NSEM)
    (y,), sigs = conv_rt(lib, c, d, torch.float16, torch.float32, K.IGEMM_LDY_PAD)(cnt, K.NSEM, new_ws(), rc=-1)
    assert sigs == [] and bool(torch.isnan(y[..., :512]).all()) and counters_clean(cnt, K.NSEM)


# ----------------------------------------------------------------------------------------
# InstanceNorm statistics
# ----------------------------------------------------------------------------------------
STEP = {"bf16": 2.0 ** -7, "f16": 2.0 ** -10}      # storage step at 2 <= |x| < 4
STATS_ROWS = [pytest.param(c, t, id=f"{c['name']}-{t}") for c in S.CASES for t in c["types"]]


@pytest.mark.parametrize("c,t", STATS_ROWS)
def test_instnorm_stats_forms(lib, c, t):
    from ghost_amd import _lib
    dt = DT[t]
    B, H, W, Cc, ldx, up = c["B"], c["H"], c["W"], c["C"], c["ldx"], c["up"]
    tag = f"stats-{c['name']}-{t}"
    g = torch.Generator().manual_seed(Cc + 3 * H + W)
    b = torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1)
    # |mean| >> std (the cancellation check of test_instnorm_stats); through the upsample 2 <= |x| < 4 as there
    x = (torch.randn(B, H, W, Cc, generator=g) * 0.3 + (2.4 + 0.25 * (b % 3) if up else 5.0 + 0.5 * (b % 4))).to(dt)
    off = 16 if ldx > Cc else 0
    buf = (torch.randn(B, H, W, ldx, generator=g) * 50.0).to(dt)
    buf[..., off:off + Cc] = x
    bufd = buf.to(DEV)
    xptr = bufd.data_ptr() + off * bufd.element_size()
    # the plan the launcher takes, with and without the counters (the statistics are not in the plan log)
    line = ctypes.create_string_buffer(256)
    for counters in (True, False):
        assert lib.ghost_instnorm_plan(_lib.gdtype(dt), B, H, W, Cc, ldx, up, c["nsem"] if counters else 0, None, line, 256) > 0
        assert line.value.decode() == S.plan_line(c, t, counters)

    def run(sem, nsem, ws):
        stat = torch.full((B * Cc * 2 + GUARD,), float("nan"), device=DEV)
        stat[B * Cc * 2:] = SENTINEL
        _lib.check(lib.ghost_instnorm_stats_rt_nhwc(_lib.gdtype(dt), xptr, B, H, W, Cc, ldx, up, stat.data_ptr(), ws.data_ptr(),
                                                    ws.numel(), None if sem is None else sem.data_ptr(), nsem, stream()))
        torch.cuda.synchronize()
        return [stat], []
    (stat,), _ = fused_contract(run, c["nsem"], tag)
    assert bool((stat[B * Cc * 2:] == SENTINEL).all()), "wrote past stat"
    st = stat[:B * Cc * 2].view(B, Cc, 2).cpu().double()
    assert samples_differ(st)
    if not up:
        # test_instnorm_stats' bounds, against float64 statistics of the stored values
        var, mean = torch.var_mean(x.double(), dim=(1, 2), unbiased=False)
        torch.testing.assert_close(st[..., 0], mean, atol=1e-5, rtol=1e-6)
        torch.testing.assert_close(st[..., 1], 1.0 / torch.sqrt(var + 1e-5), atol=0, rtol=2e-4)
        return
    # test_instnorm_stats_of_virtual_upsample's bounds.  First against the materialised upsample: the project's
    # upsample kernel, then the statistics of its output through the public entry
    xd = x.to(DEV)
    upd = torch.empty(B, 2 * H, 2 * W, Cc, dtype=dt, device=DEV)
    _lib.check(lib.ghost_upsample2x_nhwc(_lib.gdtype(dt), xd.data_ptr(), Cc, upd.data_ptr(), Cc, B, H, W, Cc, stream()))
    st_m = torch.empty(B, Cc, 2, device=DEV)
    ws = new_ws()
    _lib.check(lib.ghost_instnorm_stats_nhwc(_lib.gdtype(dt), upd.data_ptr(), B, 4 * H * W, Cc, Cc, st_m.data_ptr(),
                                             ws.data_ptr(), ws.numel(), stream()))
    st_m = st_m.cpu().double()
    quad = S.expected(c, t, True)[0] == "up_quad"
    n_out = 4 * H * W
    # quad: the materialised side carries the storage rounding (|e| <= half a step), whose mean over N outputs is
    # ~N(0, step / sqrt(3 N)): 5 sigma; otherwise the fp32 summation order only
    tol_m = 5 * STEP[t] / (3 * n_out) ** 0.5 if quad else 1e-5
    torch.testing.assert_close(st[..., 0], st_m[..., 0], atol=tol_m, rtol=1e-5)
    torch.testing.assert_close(st[..., 1], st_m[..., 1], atol=0, rtol=1e-3 + 0.1 / n_out ** 0.5 if quad else 1e-5)
    # and against float64 statistics of the unrounded PyTorch upsample: storage rounding only
    u = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True)
    var, mean = torch.var_mean(u, dim=(2, 3), unbiased=False)
    tol = 1e-5 if t == "f32" else 8e-3 * STEP[t] / STEP["bf16"]
    torch.testing.assert_close(st[..., 0], mean, atol=tol, rtol=0)
    torch.testing.assert_close(st[..., 1], 1.0 / torch.sqrt(var + 1e-5), atol=0, rtol=10 * tol)


# ----------------------------------------------------------------------------------------
# coverage: the fused signatures of production
# ----------------------------------------------------------------------------------------
def test_every_fused_signature_was_launched(lib):
    """Every fixup=std / fixup=aad line of DESIGN.md section 2 (the plans the networks select at small batch) was
    launched by an op test above.  Cases that did not run in this session (a filtered run) are launched now,
    without their reference."""
    with open(os.path.join(REPO, "DESIGN.md")) as f:
        required = set(re.findall(r"\| `([^`]*fixup=(?:std|aad)[^`]*)` \|", f.read()))
    assert len(required) >= 10, required
    for c in K.FIXUP_CASES:
        for t in c["types"]:
            if ("fix", c["name"], t) not in RAN:
                run_fixup_case(lib, c, t, False)
    for r in K.FIXUP_AAD_CASES:
        for t in r[9]:
            if ("aad", r[0], t) not in RAN:
                run_aad_case(lib, r, t, False)
    for r in K.LINEAR_CASES:
        for to in ("f32", "bf16", "f16"):
            if ("lin", r[0], to) not in RAN:
                run_linear_case(lib, r, to, False)
    missing = sorted(required - SEEN)
    assert not missing, (missing, sorted(SEEN))
