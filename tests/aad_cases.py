"""Shared helpers of tests/test_aad_ops.py: inputs, the float64 reference and the launch wrappers of the AAD
blend and mask kernels.  A plain module (not a conftest): it changes nothing about how the suite runs.

Layout conventions: activations are NHWC with a channel stride larger than the channel count; the pad channels
of the inputs hold NaN (a kernel that reads them poisons its output) and those of the outputs hold SENTINEL
(a kernel that writes them is caught bit-exactly).
"""
import ctypes as C

import torch
import torch.nn.functional as F

from oracle import aei_ref

SENTINEL = 7.0
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}      # one ulp of the storage type at |x| in [1, 2)
TNAME = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
BF, HF = torch.bfloat16, torch.float16
C_ID = 512
PAD = 8         # pad channels of h_in, z_attr and (first layer) out; the second layer's out pads 2 * PAD


def closed_form_stats(dt, Hs, Ws, C, ldx):
    """ops.hip in_stats_up2x_closed_form for an [Hs, Ws] source: the statistics of the through-upsample read are
    those of the unrounded fp32 upsample (the gate's term s), not of the stored, rounded one."""
    if dt == torch.float32 or Ws % 16 or C % 64 or ldx % 8 or Hs > 4096 or Ws > 4096:
        return False
    cpb = min(Ws, 128)
    return Ws % cpb == 0 and Hs % (512 // cpb) == 0


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def make_layer(g, c, ca, dt, dev):
    """One AADLayer's parameters, pre-rounded to the storage type ``dt``, as float64 tensors on ``dev``.  The mask
    bias and the identity path are of order 1 so that a dropped bias or a swapped layer moves the output by
    many ulps (the generator's own initialisation leaves both near 0.02)."""
    def rnd(*shape, std):
        return (torch.randn(*shape, generator=g, device=dev) * std).to(dt).double()
    return {"conv1.weight": rnd(c, ca, std=(2.0 / (c + ca)) ** 0.5), "conv1.bias": rnd(c, std=0.3),
            "conv2.weight": rnd(c, ca, std=(2.0 / (c + ca)) ** 0.5), "conv2.bias": rnd(c, std=0.3),
            "fc1.weight": rnd(c, C_ID, std=0.02), "fc1.bias": rnd(c, std=0.5),
            "fc2.weight": rnd(c, C_ID, std=0.02), "fc2.bias": rnd(c, std=0.5),
            "conv_h.weight": rnd(c, std=(2.0 / (c + 1)) ** 0.5), "conv_h.bias": rnd(1, std=0.7)}


def make_case(c, ca, H, W, B, L, up, dt, dev, seed=0):
    """Inputs of one blend case on ``dev``, every sample different (its own noise, offset, scale and z_id).

    hs  [B, Hs, Ws, c] storage-type source of h_in (Hs, Ws = H / 2, W / 2 for a through-upsample case)
    h   [B, H * W, c] float64: what the AADLayer reads (for up: F.interpolate of hs in fp32, rounded to dt)
    up32 [B, H * W, c] fp32: the unrounded upsample (up only)
    za  [B, H * W, ca] storage type, zi [B, 512] float64, layers: L parameter dicts (make_layer)
    """
    g = torch.Generator(device=dev).manual_seed(1000 * c + 10 * ca + 7 * L + H + seed)
    Hs, Ws = (H // 2, W // 2) if up else (H, W)
    b = torch.arange(B, device=dev, dtype=torch.float32).view(B, 1, 1, 1)
    hs = (torch.randn(B, Hs, Ws, c, generator=g, device=dev) * (1.25 + 0.25 * (b % 3)) + 0.7 - 0.3 * (b % 4)).to(dt)
    up32 = None
    if up:
        up32 = F.interpolate(hs.float().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True)
        up32 = up32.permute(0, 2, 3, 1).reshape(B, H * W, c)
        h = up32.to(dt).double()
    else:
        h = hs.double().reshape(B, H * W, c)
    za = torch.randn(B, H * W, ca, generator=g, device=dev).to(dt)
    zi = torch.randn(B, C_ID, generator=g, device=dev).double()
    return {"c": c, "ca": ca, "H": H, "W": W, "B": B, "L": L, "up": int(up), "dt": dt, "hs": hs, "h": h, "up32": up32,
            "za": za, "zi": zi, "layers": [make_layer(g, c, ca, dt, dev) for _ in range(L)]}


# ------------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------------
def stats_of(h):
    """(mean, rstd) over the pixels of an [B, HW, c] tensor, InstanceNorm2d's biased variance."""
    var, mean = torch.var_mean(h, dim=1, unbiased=False, keepdim=True)
    return mean, 1.0 / torch.sqrt(var + aei_ref.IN_EPS)


def aad_parts(h, za, zi, p, stats=None):
    """The terms of AADLayer.forward as plain torch expressions in the dtype and on the device of the arguments
    (NHWC, [B, HW, c]; the 1x1 convs are matmuls).  ``stats``: (mean, rstd) [B, 1, c] instead of h's own."""
    dt = h.dtype
    mean, rstd = stats_of(h) if stats is None else stats
    hn = (h - mean) * rstd
    ga = za @ p["conv1.weight"].to(dt).t() + p["conv1.bias"].to(dt)
    ba = za @ p["conv2.weight"].to(dt).t() + p["conv2.bias"].to(dt)
    gi = (zi @ p["fc1.weight"].to(dt).t() + p["fc1.bias"].to(dt)).unsqueeze(1)
    bi = (zi @ p["fc2.weight"].to(dt).t() + p["fc2.bias"].to(dt)).unsqueeze(1)
    M = torch.sigmoid(hn @ p["conv_h.weight"].to(dt).unsqueeze(1) + p["conv_h.bias"].to(dt))
    return {"rstd": rstd, "hn": hn, "ga": ga, "gi": gi, "M": M, "A": ga * hn + ba, "I": gi * hn + bi}


def aad_expr(h, za, zi, p, slope, stats=None):
    """AADLayer.forward + leaky_relu(slope), [B, HW, c], from aad_parts."""
    t = aad_parts(h, za, zi, p, stats)
    return F.leaky_relu((1 - t["M"]) * t["A"] + t["M"] * t["I"], slope)


def tie_allowance(case, l, dev):
    """Per-element allowance [B, HW, c] (absolute) for the storage rounding of an upsampled h_in, and the mask of
    the elements whose rounding is ambiguous.

    A through-upsample kernel evaluates the bilinear mix in fp32 with its own FMA contraction (up2x.h up2x_mix)
    and rounds it to the storage type; the reference rounds F.interpolate's fp32 value.  The interpolation
    weights are the same fp32 numbers in both (scale rounded once, lambda = src - floor(src)).  With or without
    contraction, the roundings of the two inner mixes sum to at most 2 u (ly0 |top| + ly1 |bot|) and those of the
    outer one to 2 u a, u = 2^-24, a = sum_taps lambda |v_tap|: each fp32 value is within 4 u a of the exact mix
    and the two within 2^-21 a of each other.  Where the fp32 value
    is that close to a midpoint of the storage grid both neighbours are correct roundings, and h_in may differ
    from the reference's by dh = one storage step + 2^-21 a.  To first order in dh (plus the dM dh cross term) that moves
    out = A + M (I - A), A = ga hn + ba, I = gi hn + bi, by
        |(1 - M) ga + M gi| rstd dh                                    (the element's own h)
      + dM (|I - A| + |gi - ga| rstd dh),  dM = 1/4 sum_c |wh_c| rstd_c dh_c   (the pixel's mask; sigmoid' <= 1/4)
    and leaky_relu (slope <= 1) does not enlarge it.  The statistics move by O(dh / HW): not counted.
    """
    dt = case["dt"]
    B, HW, c = case["h"].shape
    a = F.interpolate(case["hs"].float().abs().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear",
                      align_corners=True).permute(0, 2, 3, 1).reshape(B, HW, c).double().to(dev)
    v = case["up32"].double().to(dev)
    _, e = torch.frexp(v)                                     # |v| in [2^(e-1), 2^e)
    step = torch.ldexp(torch.ones_like(v), e - (8 if dt == torch.bfloat16 else 11))    # storage spacing at v
    frac = torch.remainder(v.abs() / step, 1.0)
    tie = ((frac - 0.5).abs() * step <= 2.0 ** -21 * a) & (v != 0)
    dh = torch.where(tie, step + 2.0 ** -21 * a, torch.zeros_like(step))   # (|v| << a: more than one step apart)
    p = {k: t.to(dev) for k, t in case["layers"][l].items()}
    t = aad_parts(case["h"].to(dev), case["za"].double().to(dev), case["zi"].to(dev), p)
    own = ((1 - t["M"]) * t["ga"] + t["M"] * t["gi"]).abs() * t["rstd"] * dh
    dM = 0.25 * (p["conv_h.weight"].abs() * t["rstd"] * dh).sum(-1, keepdim=True)
    return own + dM * ((t["I"] - t["A"]).abs() + (t["gi"] - t["ga"]).abs() * t["rstd"] * dh), tie


def aad_oracle(h, za, zi, p, slope, H, W):
    """The same through oracle/aei_ref.aad_layer (NCHW, F.instance_norm, F.conv2d), back in [B, HW, c]."""
    B, HW, c = h.shape
    dt = h.dtype
    nchw = lambda t: t.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()  # noqa: E731
    q = {"l." + k: v.to(dt) for k, v in p.items()}
    for k in ("conv1.weight", "conv2.weight"):
        q["l." + k] = q["l." + k].reshape(c, -1, 1, 1)
    q["l.conv_h.weight"] = q["l.conv_h.weight"].reshape(1, c, 1, 1)
    out = F.leaky_relu(aei_ref.aad_layer(nchw(h), nchw(za), zi, q, "l"), slope)
    return out.permute(0, 2, 3, 1).reshape(B, HW, c)


def reference(case, l, slope, on_cpu):
    """(ref64, e32, s, allow, tie) of layer ``l``: the float64 reference [B, HW, c], the max over elements of
    |fp32 evaluation - ref64| / max(1, |ref64|), the same for the float64 evaluation with the statistics of the
    unrounded upsample (0 for a case that is not read through the upsample), and tie_allowance's pair (None
    without the upsample)."""
    dev = torch.device("cpu") if on_cpu else case["h"].device
    h, za, zi = case["h"].to(dev), case["za"].double().to(dev), case["zi"].to(dev)
    p = {k: v.to(dev) for k, v in case["layers"][l].items()}
    if on_cpu:
        ref = aad_oracle(h, za, zi, p, slope, case["H"], case["W"])
        o32 = aad_oracle(h.float(), za.float(), zi.float(), p, slope, case["H"], case["W"])
    else:
        ref = aad_expr(h, za, zi, p, slope)
        o32 = aad_expr(h.float(), za.float(), zi.float(), p, slope)
    den = ref.abs().clamp_min(1.0)
    e32 = float(((o32.double() - ref).abs() / den).max())
    s, allow, tie = 0.0, None, None
    if case["up"]:
        alt = aad_expr(h, za, zi, p, slope, stats=stats_of(case["up32"].double().to(dev)))
        s = float(((alt - ref).abs() / den).max())
        allow, tie = tie_allowance(case, l, dev)
    return ref, e32, s, allow, tie


# ------------------------------------------------------------------------------------------------
# launches
# ------------------------------------------------------------------------------------------------
def logged_call(call):
    """call() with the plan log on -> the signatures it launched, in order."""
    from ghost_amd import _lib
    _lib.plan_log(True)
    try:
        call()
        torch.cuda.synchronize()
    finally:
        _lib.plan_log(False)
    return _lib.plan_log_read()


def aad_sigs(sigs):
    """The AAD blend kernels among the logged signatures."""
    return [s for s in sigs if s.split()[0].startswith("aad_")]


def assert_plan(sigs, name, tokens):
    """Exactly one AAD blend kernel ran, named ``name`` and holding every token."""
    aad = aad_sigs(sigs)
    assert len(aad) == 1 and aad[0].split()[0] == name, (name, sigs)
    assert all(t in aad[0].split() for t in tokens), (tokens, aad[0])


def padded(t, pad, fill):
    """[..., n] -> a [..., n + pad] buffer holding t with the pad channels set to ``fill``."""
    buf = torch.full(t.shape[:-1] + (t.shape[-1] + pad,), fill, dtype=t.dtype, device=t.device)
    buf[..., :t.shape[-1]] = t
    return buf


def id_table(case, l):
    """[B, 2c] fp32: gamma_id at c, beta_id at c + C (the fc1 / fc2 outputs the kernels take as an input)."""
    p, zi = case["layers"][l], case["zi"]
    return torch.cat([zi @ p["fc1.weight"].t() + p["fc1.bias"], zi @ p["fc2.weight"].t() + p["fc2.bias"]], 1) \
        .float().contiguous()


def run_layers_v3(lib, case, slope):
    """ghost_aad_layers_v3_dt_nhwc on the case -> ([out_l as [B, HW, ldo_l]], logged signatures)."""
    from ghost_amd import _lib
    from ghost_amd.network.pack import pack_aad_v3
    c, ca, H, W, B, L, dt = (case[k] for k in ("c", "ca", "H", "W", "B", "L", "dt"))
    dev = case["hs"].device
    hd = padded(case["hs"].reshape(B, -1, c), PAD, float("nan"))
    zad = padded(case["za"], PAD, float("nan"))
    keep, outs = [], []
    cols = {k: [] for k in ("w3", "b3", "wh", "bh", "id", "out")}
    for l in range(L):
        p = case["layers"][l]
        sd = {"l." + k: v.float() for k, v in p.items()}
        for k in ("l.conv1.weight", "l.conv2.weight"):
            sd[k] = sd[k].reshape(c, ca, 1, 1)
        pk = pack_aad_v3(sd, "l", dt)
        idgb = id_table(case, l)
        wh, bh = p["conv_h.weight"].float().contiguous(), p["conv_h.bias"].float().contiguous()
        out = torch.full((B, H * W, c + PAD * (l + 1)), SENTINEL, dtype=dt, device=dev)
        keep += [pk, idgb, wh, bh]
        outs.append(out)
        for k, t in zip(cols, (pk["w3"], pk["b3"], wh, bh, idgb, out)):
            cols[k].append(t.data_ptr())
    arr = lambda xs: (C.c_void_p * L)(*xs)  # noqa: E731
    ws = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    sigs = logged_call(lambda: _lib.check(lib.ghost_aad_layers_v3_dt_nhwc(
        _lib.gdtype(dt), hd.data_ptr(), c + PAD, case["up"], zad.data_ptr(), ca + PAD, B, H, W, c, ca, L, arr(cols["w3"]),
        arr(cols["b3"]), arr(cols["wh"]), arr(cols["bh"]), arr(cols["id"]), 2 * c, slope, arr(cols["out"]),
        (C.c_int * L)(*[o.shape[-1] for o in outs]), ws.data_ptr(), ws.numel(), s)))
    return outs, sigs


def run_layer(lib, case, slope, rt=None):
    """ghost_aad_layer_nhwc (the module path: fused kernel or mask + GEMM epilogue) on a one-layer case.
    rt = dict(split_k, sem, nsem, ws): through ghost_aad_layer_rt_nhwc instead, as the runtime calls the layer (sem:
    an int32 tensor of counters or None; ws: the workspace tensor to use, so that a second call can reuse it)."""
    from ghost_amd import _lib
    from ghost_amd.network.pack import pack_aad
    c, ca, H, W, B, dt = (case[k] for k in ("c", "ca", "H", "W", "B", "dt"))
    dev = case["hs"].device
    p = case["layers"][0]
    sd = {"l." + k: v.float() for k, v in p.items()}
    for k in ("l.conv1.weight", "l.conv2.weight"):
        sd[k] = sd[k].reshape(c, ca, 1, 1)
    pk = pack_aad(sd, "l", dt)
    idgb = id_table(case, 0)
    hd = padded(case["hs"].reshape(B, -1, c), PAD, float("nan"))
    zad = padded(case["za"], PAD, float("nan"))
    out = torch.full((B, H * W, c + PAD), SENTINEL, dtype=dt, device=dev)
    ws = rt["ws"] if rt else torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    args = (_lib.gdtype(dt), hd.data_ptr(), c + PAD, zad.data_ptr(), ca + PAD, B, H, W, c, ca, pk["gbw"].data_ptr(),
            pk["gbw"].shape[0], pk["gbw"].shape[1], pk["gbb"].data_ptr(), pk["wh"].data_ptr(), pk["bh"].data_ptr(),
            idgb.data_ptr(), 2 * c, slope, out.data_ptr(), c + PAD, ws.data_ptr(), ws.numel())
    if rt:
        sem = rt["sem"]
        sigs = logged_call(lambda: _lib.check(lib.ghost_aad_layer_rt_nhwc(
            *args, rt["split_k"], None if sem is None else sem.data_ptr(), rt["nsem"], s)))
    else:
        sigs = logged_call(lambda: _lib.check(lib.ghost_aad_layer_nhwc(*args, s)))
    return [out], sigs


def pads_intact(out, c):
    """The pad channels of an output buffer still hold SENTINEL, bit for bit."""
    want = torch.full((), SENTINEL, dtype=out.dtype).view(torch.int16 if out.element_size() == 2 else torch.int32)
    got = out[..., c:].contiguous().view(torch.int16 if out.element_size() == 2 else torch.int32)
    return bool((got == want.to(got.device)).all())


# ------------------------------------------------------------------------------------------------
# masks
# ------------------------------------------------------------------------------------------------
def mask_expr(h, mean, rstd, wh, bh):
    """sigmoid(sum_c wh_c (h_c - mean_c) rstd_c + bh) -> [B, HW], in the dtype of its arguments."""
    return torch.sigmoid((((h - mean) * rstd) * wh).sum(-1) + bh)


def _running_bound(t):
    """(sum, B) of a reduction of the terms t [..., lanes, n] in the order the mask kernels use: every lane adds its
    n terms one FMA at a time, then the lanes are summed by halving xor-shuffles (group_sum: lane i += lane
    i ^ o, o = lanes / 2 ... 1).  Every fp32 operation rounds its result r within u |r|, so to first order the
    computed sum is within u B of the exact one, B = the sum of |r| over every partial sum formed."""
    cs = t.cumsum(-1)
    bound = cs.abs().sum((-1, -2))
    x = cs[..., -1]
    while x.shape[-1] > 1:
        half = x.shape[-1] // 2
        x = x[..., :half] + x[..., half:]
        bound = bound + x.abs().sum(-1)
    return x[..., 0], bound


def _lanes(x, lanes, vec):
    """[..., C] -> [..., lanes, n]: lane i owns the vec-channel chunks i, i + lanes, ... in order (zero-padded)."""
    C = x.shape[-1]
    chunks = -(-C // (lanes * vec))
    x = F.pad(x, (0, chunks * lanes * vec - C))
    return x.reshape(x.shape[:-1] + (chunks, lanes, vec)).transpose(-3, -2).reshape(x.shape[:-1] + (lanes, chunks * vec))


def uncentred_term(h, mean, rstd, wh, bh, kernel, vec):
    """[B, HW]: what the uncentred logit of the register-table mask kernel (``kernel`` = "reg") and of
    stats_mask_small ("small") may add to the mask error.  Both evaluate sum_c cf_c h_c - K, cf = wh rstd,
    K = sum_c cf_c mean_c (ops.hip: "the logit is one FMA per channel"), not the centred sum the reference and
    the LDS-table kernel form, so their rounding errors scale with the partial sums of cf h and of cf mean, which
    are large where |mean| >> std or rstd is large (HW = 1: var = 0), not with those of cf (h - mean).  The bound
    is the running error bound (_running_bound) of the two sums in the kernels' own order, plus the rounding of
    cf (which perturbs the centred terms only), of the bias and of the final add, times sigmoid' <= 1/4.
      reg    lane gl of a G = min(64, C / 8)-lane group owns the 8-channel chunks gl, gl + G; K the same
      small  logit: lane i of a 64-lane wave owns the vec-channel chunks i, i + 64, ...; K: thread t of 256 owns
             chunks t, t + 256, ..., each wave sums its lanes, then ((w0 + w1) + w2) + w3 + bh
    It is 0 for the centred LDS-table kernel."""
    cf = wh * rstd
    th, tm = cf * h, cf * mean
    if kernel == "reg":
        G = min(64, h.shape[-1] // 8)
        sh, bnd_h = _running_bound(_lanes(th, G, 8))
        sm, bnd_m = _running_bound(_lanes(tm, G, 8))
        bias = bh - sm
    else:
        sh, bnd_h = _running_bound(_lanes(th, 64, vec))
        w = _lanes(tm, 256, vec)
        ws, bnd_m = _running_bound(w.reshape(w.shape[:-2] + (4, 64, w.shape[-1])))      # [..., 4] wave sums
        bnd_m = bnd_m.sum(-1)
        part = ws.cumsum(-1)
        bias = bh - part[..., -1]
        bnd_m = bnd_m + part[..., 1:].abs().sum(-1)
    total = bnd_h + bnd_m + bias.abs() + (sh + bias).abs() + (cf * (h - mean)).abs().sum(-1)
    return 0.25 * 2.0 ** -24 * total


def run_mask(lib, dt, h, stat, whs, bhs, small):
    """ghost_aad_mask_nhwc on h [B, HW, c] (dt, CPU) -> (rc, [mask_l incl. its sentinel element], stat)."""
    from ghost_amd import _lib
    dev = torch.device("cuda:0")
    B, HW, c = h.shape
    pad = 4 if dt == torch.float32 else 8
    hd = padded(h.to(dev), pad, float("nan"))
    std = torch.full((B, c, 2), float("nan"), device=dev) if stat is None else stat.float().to(dev).contiguous()
    whd = [w.float().to(dev).contiguous() for w in whs]
    bhd = [b.float().to(dev).contiguous() for b in bhs]
    masks = [torch.full((B * HW + 1,), SENTINEL, device=dev) for _ in whs]
    two = len(whs) == 2
    rc = lib.ghost_aad_mask_nhwc(_lib.gdtype(dt), hd.data_ptr(), c + pad, B, HW, c, std.data_ptr(), whd[0].data_ptr(),
                                 bhd[0].data_ptr(), masks[0].data_ptr(), whd[1].data_ptr() if two else None,
                                 bhd[1].data_ptr() if two else None, masks[1].data_ptr() if two else None,
                                 int(small), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, [m.cpu() for m in masks], std.cpu()


# ----------------------------------------------------------------------------------------
# blend cases (tests/test_aad_ops.py on the GPU, tests/test_aad_plan_cpu.py without one): the smallest shapes that
# select each variant, derived from the planners aad_v3_plan (aad_v3.hip) and aad_wide_plan (aad_wide.hip) behind
# aad_path (aad_path.h).  If a retuned heuristic moves a case to another kernel, test_aad_plan_cpu.py says so
# without a GPU: change the shape, not the kernel.
#   * a bf16 C = 64 through-upsample launch always runs aad_v5 or aad_v4 (v4 takes every such launch v5 leaves),
#     so no bf16 shape, with W / 2 % 4 != 0 or otherwise, reaches aad_v3's C = 64 UP form; fp16 has no v4, and the
#     fp16 launches at the v4 shape below are that form's cases (they must log aad_v3).
#   * cpu = True: the float64 reference is oracle/aei_ref.aad_layer on the CPU (at least the smallest case of
#     every kernel); otherwise the same expression on the device.  aad_v5_wide (33 M output elements at its
#     smallest) and aad_gemm (4 M elements behind 1024 x 512 weights) are device-only: their CPU evaluation
#     takes many seconds.
# ----------------------------------------------------------------------------------------
CASES = []


def _add(kernel, dt, c, ca, H, W, B, L, up, slope, ipw=0, ppw=None, cpu=False):
    CASES.append(dict(kernel=kernel, dt=dt, c=c, ca=ca, H=H, W=W, B=B, L=L, up=up, slope=slope, ipw=ipw, ppw=ppw,
                      cpu=cpu))


for _ca in (64, 32):
    for _L in (1, 2):
        for _s in (0.0, 1.0):
            _add("aad_v3", BF, 64, _ca, 64, 128, 2, _L, 0, _s, ppw=512, cpu=True)
            # v4: HW < 65536 keeps v5 away
            _add("aad_v4", BF, 64, _ca, 64, 128, 2, _L, 1, _s, ppw=512, cpu=True)
            # v5: HW = 65536 (1024-pixel work items); a wide image (one row tile per item) and a narrow one (four)
            _add("aad_v5", BF, 64, _ca, 128, 512, 2, _L, 1, _s, ipw=1, ppw=1024, cpu=(_ca, _L, _s) == (32, 1, 0.0))
            _add("aad_v5", BF, 64, _ca, 512, 128, 2, _L, 1, _s, ipw=1, ppw=1024)
        # two work items per workgroup need B * HW / 2048 >= 256
        _add("aad_v5", BF, 64, _ca, 256, 256, 8, _L, 1, 0.0, ipw=2, ppw=1024)
_add("aad_v5", BF, 64, 64, 256, 256, 8, 2, 1, 1.0, ipw=2, ppw=1024)
_add("aad_v5", BF, 64, 32, 256, 256, 8, 1, 1, 1.0, ipw=2, ppw=1024)
# C = 128: B * HW = 8192 is the least aad_v3_supported admits (32 workgroups of 256 pixels); neither v5_wide
# (needs 256 work items) nor v4 (C = 64) takes the through-upsample forms here
for _s in (0.0, 1.0):
    for _up in (0, 1):
        for _ca in (128, 64, 32):
            _add("aad_v3_wide", BF, 128, _ca, 32, 128, 2, 1, _up, _s, ppw=256, cpu=True)
        _add("aad_v3_wide", BF, 128, 64, 32, 128, 2, 2, _up, _s, ppw=256, cpu=True)
    for _ca in (128, 64):
        _add("aad_v3_wide", BF, 256, _ca, 32, 32, 8, 1, 0, _s, ppw=256, cpu=True)
# v5_wide: a 64 x 64 output is 4 work items; 256 / 512 / 1024 of them select 1 / 2 / 4 per workgroup
for _L in (1, 2):
    for _s in (0.0, 1.0):
        _add("aad_v5_wide", BF, 128, 64, 64, 64, 64, _L, 1, _s, ipw=1, ppw=1024)
_add("aad_v5_wide", BF, 128, 64, 64, 64, 128, 2, 1, 0.0, ipw=2, ppw=1024)
_add("aad_v5_wide", BF, 128, 64, 64, 64, 256, 1, 1, 0.0, ipw=4, ppw=1024)
for _s in (0.0, 1.0):
    _add("aad_wide", BF, 256, 128, 16, 16, 16, 1, 0, _s, ppw=32, cpu=True)
    _add("aad_wide", BF, 512, 64, 32, 32, 4, 1, 0, _s, ppw=64, cpu=True)
    _add("aad_wide_deep", BF, 1024, 512, 16, 16, 8, 1, 0, _s, ppw=128, cpu=_s == 0.0)
    _add("aad_gemm", BF, 1024, 512, 16, 16, 16, 1, 0, _s)
# fp16: one case per kernel family; v4 is bf16-only, so its shape must log aad_v3 (the C = 64 UP form)
_add("aad_v3", HF, 64, 64, 64, 128, 2, 2, 0, 0.0, ppw=512, cpu=True)
_add("aad_v3", HF, 64, 64, 64, 128, 2, 2, 1, 0.0, ppw=512, cpu=True)
_add("aad_v3", HF, 64, 32, 64, 128, 2, 1, 1, 1.0, ppw=512, cpu=True)
_add("aad_v5", HF, 64, 64, 128, 512, 2, 2, 1, 0.0, ipw=1, ppw=1024)
_add("aad_v3_wide", HF, 128, 64, 32, 128, 2, 2, 1, 0.0, ppw=256, cpu=True)
_add("aad_v3_wide", HF, 256, 128, 32, 32, 8, 1, 0, 0.0, ppw=256, cpu=True)
_add("aad_v5_wide", HF, 128, 64, 64, 64, 64, 1, 1, 0.0, ipw=1, ppw=1024)
_add("aad_wide", HF, 256, 128, 16, 16, 16, 1, 0, 0.0, ppw=32, cpu=True)
_add("aad_wide_deep", HF, 1024, 512, 16, 16, 8, 1, 0, 0.0, ppw=128)
_add("aad_gemm", HF, 1024, 512, 16, 16, 16, 1, 0, 0.0)


def _id(k):
    return (f"{k['kernel']}-{TNAME[k['dt']]}-C{k['c']}-Ca{k['ca']}-{k['H']}x{k['W']}-B{k['B']}-L{k['L']}-up{k['up']}"
            f"-slope{k['slope']:g}")


def _tokens(k):
    t = [f"t={TNAME[k['dt']]}", f"C={k['c']}", f"Ca={k['ca']}"]
    if k["kernel"] in ("aad_wide", "aad_wide_deep"):
        return t + [f"ppw={k['ppw']}"]
    if k["kernel"] == "aad_gemm":
        return t
    return t + [f"L={k['L']}", f"up={k['up']}", "zpm=0", f"slope0={int(k['slope'] == 0.0)}", f"v5_ipw={k['ipw']}",
                f"ppw={k['ppw']}"]
