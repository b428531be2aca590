"""Edge cases of the implicit GEMM shared by the GPU op tests (tests/test_gpu_parity.py: the kernels' results and the
plan log of the launch) and the CPU plan tests (tests/test_conv_plan_cpu.py: the same tokens from ghost_conv_plan).

Edge classes that no pipeline batch selects but the public conv entries accept: M and N tails, ragged / one-step /
clamped split-K, a last split shorter than the ring's prologue, both reduction forms, the non-FAST gather with 16-bit
operands.  split_k > 0 keeps a conv off the halo and patch kernels.  If a retuned heuristic moves a case to another
variant, change the shape, not the class.
"""

IGEMM_EDGES = [
    # cin, ldx, cout, k, s, p, B, H, W, split_k, plan tokens (GEMM launch), reduction kernel
    # glds 64x128, 3 stages, M = 120 (tail), non-square; nk = 27: splits 7,7,7,6 / one K step each / clamped to nk
    (96, 96, 128, 3, 1, 1, 2, 6, 10, 4, ("glds", "64x128", "stages=3", "split=1", "ragged=1", "short=0", "mtail=1"),
     "splitk_reduce4"),
    (96, 96, 128, 3, 1, 1, 2, 6, 10, 27, ("glds", "64x128", "stages=3", "split=1", "ragged=0", "short=1", "mtail=1"),
     "splitk_reduce4"),
    (96, 96, 128, 3, 1, 1, 2, 6, 10, 100, ("glds", "64x128", "stages=3", "split=1", "ragged=0", "short=1", "mtail=1"),
     "splitk_reduce4"),
    # N tail: Cout 200 reduces four channels at a time, Cout 130 one
    (64, 64, 200, 3, 1, 1, 3, 5, 7, 2, ("glds", "64x128", "split=1", "ntail=1", "mtail=1"), "splitk_reduce4"),
    (64, 64, 130, 3, 1, 1, 3, 5, 7, 2, ("glds", "64x128", "split=1", "ntail=1", "mtail=1"), "splitk_reduce"),
    # deep ring 128x128 x 8 stages; nk = 36: splits 8,8,8,8,4 (the last shorter than STAGES - 1) / one K step each
    (128, 128, 256, 3, 1, 1, 2, 8, 8, 5, ("glds", "128x128", "stages=8", "split=1", "ragged=1", "lastshort=1",
                                          "mtail=0"), "splitk_reduce4"),
    (128, 128, 256, 3, 1, 1, 3, 5, 7, 5, ("glds", "128x128", "stages=8", "split=1", "ragged=1", "lastshort=1",
                                          "mtail=1"), "splitk_reduce4"),
    (128, 128, 256, 3, 1, 1, 2, 8, 8, 36, ("glds", "128x128", "stages=8", "split=1", "short=1", "mtail=0"),
     "splitk_reduce4"),
    (128, 128, 256, 3, 1, 1, 3, 5, 7, 36, ("glds", "128x128", "stages=8", "split=1", "short=1", "mtail=1"),
     "splitk_reduce4"),
    # the encoder's 4x4/s2 tile on the ring
    (32, 32, 64, 4, 2, 1, 1, 12, 20, 2, ("glds", "128x64", "split=1", "mtail=1"), "splitk_reduce4"),
    # register-staged kernel, 256x32 tile, 16-bit split
    (64, 64, 24, 3, 1, 1, 2, 9, 5, 3, ("igemm", "256x32x32", "fast=1", "epi=SPLIT", "split=1", "ntail=1", "mtail=1"),
     "splitk_reduce4"),
    # 1x1/s2 (nk = 5): unsplit and one K step per split
    (160, 160, 96, 1, 2, 0, 2, 10, 6, 0, ("glds", "64x128", "split=0", "ntail=1", "mtail=1"), None),
    (160, 160, 96, 1, 2, 0, 2, 10, 6, 5, ("glds", "64x128", "split=1", "short=1", "ntail=1", "mtail=1"),
     "splitk_reduce4"),
    # the non-FAST gather (Cin % 32 != 0, padded input channels) with 16-bit operands
    (20, 24, 70, 3, 1, 1, 2, 7, 6, 0, ("igemm", "64x64x32", "fast=0", "split=0", "ntail=1", "mtail=1"), None),
]
IGEMM_LDY_PAD = 8       # test_igemm_edge_plans writes into ldy = cout + 8

# ConvT 4x4/s2 544 -> Cout at B = 1, 4 x 6 (M = 24 per parity class, nk = 68): the heuristic's 8 splits are seven of
# 9 K steps and a last of 5; every case reduces with splitk_reduce4
CONVT_CIN, CONVT_H, CONVT_W = 544, 4, 6
CONVT_LDY_PAD = 32      # test_convT_igemm_edge_plans writes into ldy = cout + 32
CONVT_EDGES = [
    (64, ("igemm", "256x64x32", "kind=T4S2", "split=1", "ragged=1", "mtail=1")),
    (128, ("glds", "64x128", "kind=T4S2", "split=1", "ragged=1", "mtail=1")),
]


def gemm_tokens(plan, t):
    """The tokens the GEMM line must hold for storage type name ``t`` ("bf16" / "f16")."""
    return plan + ("t=" + t,) if plan[0] == "glds" else plan


# ----------------------------------------------------------------------------------------
# The split-K fix-up (split_fixup, conv_igemm.hip) and the GEMMs whose output type differs from their operand type:
# what only the runtimes select, through ghost_conv_rt_nhwc / ghost_aad_layer_rt_nhwc (tests/test_fused_reduce_ops.py
# on the GPU, tests/test_conv_plan_cpu.py without one).  Each case: the smallest shape of its class, found by asking
# ghost_conv_plan; the tokens of its GEMM line with the case's counters, and the reduction kernel that follows where
# the plan does not fuse (`reduce`: also the line of the same call without counters).  The rule above holds.
# ----------------------------------------------------------------------------------------
NSEM = 4096             # the runtime's counter words (aei_runtime.hip kSemWords)
T16 = ("bf16", "f16")
T3 = T16 + ("f32",)
_FIX_M = ("split=1", "fixup=std", "fixrows=M", "mtail=1")


def _fix(name, tokens, B, H, W, cin, n, k=1, s=1, p=0, kind="fwd", split_k=0, types=("bf16", "f16"), nsem=NSEM,
         reduce="splitk_reduce4", tokens_f32=None):
    """tokens: the 16-bit GEMM line's (t=<type> is added for a glds line); tokens_f32: the fp32 line's, for a case
    whose types hold f32.  A case with "fixup=none" among its tokens must run `reduce`; the others nothing."""
    return dict(name=name, tokens=tuple(tokens), tokens_f32=tuple(tokens_f32 or ()), B=B, H=H, W=W, cin=cin, n=n, k=k, s=s,
                p=p, kind=kind, split_k=split_k, types=tuple(types), nsem=nsem, reduce=reduce)


_F32_M = ("igemm", "ti=f32", "to=f32", "64x128x32", "fast=1") + _FIX_M
FIXUP_CASES = [
    # glds 64x128, 15 rows of a 64-row tile: 4 x 15 x 128 x 4 = 30720 bytes of partials (test_igemm_thresholds' row)
    _fix("glds64-rowsM", ("glds", "64x128", "stages=3", "kind=FWD", "ntail=0") + _FIX_M, 1, 3, 5, 512, 128, split_k=4,
         types=T3, tokens_f32=_F32_M + ("kind=FWD",)),
    # the deep ring: 4 x 16 x 128 x 4 = 32768, exactly the bound
    _fix("deep-rowsM", ("glds", "128x128", "stages=8", "kind=FWD") + _FIX_M, 1, 4, 4, 1024, 256, split_k=4),
    # the register-staged kernel: 256x32 tile, N tail inside the only column tile
    _fix("igemm256x32", ("igemm", "256x32x32", "fast=1", "epi=SPLIT", "ntail=1") + _FIX_M, 1, 9, 5, 64, 24, 3, 1, 1,
         split_k=3),
    # two M tiles, the last of 67 rows: only the 256x16 tile holds a whole tile's partials of two splits in 32 KB
    _fix("mtiles-tail", ("igemm", "256x16x32", "fast=1", "split=1", "fixup=std", "fixrows=BM", "mtail=1"), 1, 17, 19,
         64, 16, 3, 1, 1, split_k=2),
    # N tail: 72 and 2 columns in the last tile
    _fix("ntail200", ("glds", "64x128", "ntail=1") + _FIX_M, 1, 3, 5, 64, 200, 3, 1, 1, split_k=2),
    _fix("ntail130", ("glds", "64x128", "ntail=1") + _FIX_M, 1, 3, 5, 64, 130, 3, 1, 1, split_k=2, reduce="splitk_reduce"),
    # nk = 27 in splits of 7, 7, 7, 6; nk = 5 in five splits of one K step (shorter than the ring's prologue)
    _fix("ragged", ("glds", "64x128", "ragged=1", "short=0") + _FIX_M, 1, 3, 5, 96, 128, 3, 1, 1, split_k=4),
    _fix("short", ("glds", "64x128", "ragged=0", "short=1", "ntail=1") + _FIX_M, 1, 3, 4, 160, 96, split_k=5),
    # ConvT 4x4/s2: the four parity classes share the counter array; the heuristic's own split (production: B = 1, 2)
    _fix("T4S2-deep", ("glds", "128x128", "stages=8", "kind=T4S2", "ntail=0") + _FIX_M, 2, 2, 2, 256, 256, kind="T",
         types=T3, tokens_f32=_F32_M + ("kind=T4S2",)),
    _fix("T4S2-ragged", ("glds", "64x128", "stages=3", "kind=T4S2", "ragged=1") + _FIX_M, 1, 2, 3, 544, 128, kind="T"),
    # a counter per (phase, tile): 4 phases x 1 tile fuse with 4 words; with 3 the reduction kernel runs
    _fix("T4S2-nsem4", ("glds", "64x128", "kind=T4S2") + _FIX_M, 1, 2, 3, 128, 128, kind="T", split_k=4, nsem=4),
    _fix("T4S2-nsem3", ("glds", "64x128", "kind=T4S2", "split=1", "fixup=none"), 1, 2, 3, 128, 128, kind="T", split_k=4,
         nsem=3),
    _fix("nsem2", ("glds", "64x128", "kind=FWD") + _FIX_M, 1, 3, 5, 512, 256, split_k=4, nsem=2),
    _fix("nsem1", ("glds", "64x128", "kind=FWD", "split=1", "fixup=none"), 1, 3, 5, 512, 256, split_k=4, nsem=1),
]

# fixup=aad through ghost_aad_layer_rt_nhwc: (name, tokens, tokens_f32, B, H, W, C, Ca, split_k, types).  The channel
# strides are aad_cases.PAD wider than the channel counts.  The production form is the deep ring's (N = 2 C >= 256,
# Ca >= 1024, the heuristic's four splits); no accepted C gives the deep ring a column tile beyond C_aad (it wants
# N % 128 == 0), the register-staged 64x128 tile at C = 32 has one (columns 64 .. 127 of its only tile: channels
# 32 .. 63).  The mask pass before the GEMM takes C / 8 (fp32: C / 4) a power of two only, so C = 80 is refused
_AAD_M = ("epi=SPLIT", "split=1", "fixup=aad", "mtail=1", "fixrows=M")
FIXUP_AAD_CASES = [
    ("deep-B1", ("glds", "128x128", "stages=8", "ntail=0") + _AAD_M, _F32_M[:5] + _AAD_M, 1, 2, 2, 128, 1024, 0, T3),
    ("deep-B3", ("glds", "128x128", "stages=8", "ntail=0") + _AAD_M, (), 3, 2, 2, 128, 1024, 0, T16),
    ("deep-4x4", ("glds", "128x128", "stages=8", "ntail=0") + _AAD_M, (), 1, 4, 4, 128, 1024, 0, T16),
    ("ntail-C32", ("igemm", "64x128x32", "fast=1", "ntail=1") + _AAD_M,
     ("igemm", "ti=f32", "to=f32", "64x128x32", "fast=1", "ntail=1") + _AAD_M, 2, 3, 5, 32, 512, 0, T3),
]

# ghost_linear_f32 (unsplit, or split without counters: the reduction kernel) and the same GEMM through
# ghost_conv_rt_nhwc with counters (the runtimes' "igemm ti=f32 ... fixup=std" line):
# (name, B, K, N, split_k, counters, tokens without to=<type>, reduction kernel or None)
LINEAR_LDY_PAD = 8
LINEAR_CASES = [
    ("tails-B1", 1, 100, 70, 0, 0, ("igemm", "ti=f32", "64x64x32", "fast=0", "epi=STD", "split=0", "ntail=1"), None),
    ("tails-B3", 3, 100, 70, 0, 0, ("igemm", "ti=f32", "64x64x32", "fast=0", "epi=STD", "split=0", "ntail=1"), None),
    ("split-nosem", 3, 512, 512, 0, 0, ("igemm", "ti=f32", "64x128x32", "fast=1", "split=1", "fixup=none"),
     "splitk_reduce4"),
    ("prod-B1", 1, 512, 512, 0, NSEM, ("igemm", "ti=f32", "64x128x32", "fast=1", "kind=FWD", "ntail=0") + _FIX_M, None),
    ("prod-B3", 3, 512, 512, 0, NSEM, ("igemm", "ti=f32", "64x128x32", "fast=1", "kind=FWD", "ntail=0") + _FIX_M, None),
    ("ntail130", 3, 1024, 130, 4, NSEM, ("igemm", "ti=f32", "64x128x32", "fast=1", "ntail=1") + _FIX_M, None),
    ("gather-ragged", 3, 520, 200, 4, NSEM, ("igemm", "ti=f32", "64x64x32", "fast=0", "ragged=1", "ntail=1") + _FIX_M,
     None),
]

# 16-bit operands with an fp32 output (the ArcFace head's form: a 7x7 valid conv on a 7x7 input, here 64 channels):
# the GEMM writes partials even unsplit and splitk_reduce to=f32 applies the epilogue; counters never fuse it.
# Only bf16 has instances (igemm_plan: f32_from16 wants ti == bf16): fp16 -> fp32 is refused, nothing launched.
HEAD_CIN, HEAD_HW = 64, 7
HEAD_TOKENS = ("igemm", "ti=bf16", "to=bf16", "64x128x32", "epi=SPLIT", "fixup=none")
HEAD_REDUCE = "splitk_reduce to=f32 epi=STD from=bf16"
HEAD_CASES = [(n, B, nsem) for n in (512, 200) for B in (1, 3) for nsem in (0, NSEM)]


# ----------------------------------------------------------------------------------------
# The convolution families off the implicit GEMM: halo, halo_pp, convT_halo, s2_patch, first, stem3x3.  One entry per
# variant, each at the smallest shape that selects it (halo_plan wants 64 work items, convT_halo 128 workgroups,
# s2_patch 32), with the tokens its plan-log line must hold.  tests/test_conv_ops.py runs them on the GPU against a
# float64 reference, tests/test_conv_plan_cpu.py asks ghost_conv_plan (ncu = 256) for the same tokens without one.
# The rule above holds here too: if a retuned heuristic moves a case, change the shape, not the class.
# ----------------------------------------------------------------------------------------
RES, RES_FIRST, PRELU, Y2, TANH, IN_PART = 1, 2, 4, 8, 32, 64      # GHOST_CONV_PLAN_* (include/ghost_amd.h)

# epilogues (include/ghost_amd.h ghost_conv_epi): bn = per-channel scale and shift; slope is the leaky slope where no
# PReLU table is given; res = a residual, added after the activation unless res_first
MODES = {
    "bn": dict(bn=1, slope=0.2),                                  # scale / shift / leaky
    "res": dict(bn=0, slope=1.0, res=1),                          # AAD_ResBlk's conv + residual: nothing else
    "none": dict(bn=0, slope=1.0),                                # ... and without it
    "y2": dict(bn=1, slope=0.2, y2=1),
    "prelu_y2": dict(bn=1, slope=1.0, prelu=1, y2=1),             # IBasicBlock conv1 + the next BN
    "prelu_res_y2": dict(bn=1, slope=1.0, prelu=1, res=1, y2=1),
    "resfirst": dict(bn=1, slope=0.0, res=1, res_first=1),        # Bottleneck tail relu(bn(conv) + residual)
    "resfirst_y2": dict(bn=1, slope=1.0, res=1, res_first=1, y2=1),   # IBasicBlock conv2 + residual + the next BN
    "tanh": dict(bn=1, slope=1.0, tanh=1),
    "bn_res": dict(bn=1, slope=0.2, res=1),                       # the linknet deconv: BN + leaky, then the skip
}


def mode_flags(mode):
    m = MODES[mode]
    return (RES if m.get("res") else 0) | (RES_FIRST if m.get("res_first") else 0) | (PRELU if m.get("prelu") else 0) | \
           (Y2 if m.get("y2") else 0) | (TANH if m.get("tanh") else 0)


LDY_PAD = 8


def _case(tokens, B, H, W, cin, n, mode="bn", k=3, s=1, p=1, kind="fwd", ldx=None, ldy=None, types=T16, stats=False):
    """tokens: the kernel's name first, then what its line must hold (t=<type> is added per type).  ldx > cin: the
    input is a channel slice of a wider buffer whose other channels hold finite junk (the 3-channel convs' 4-channel
    layout: the kernel reads channel 3 against zero weights).  stats: through ghost_conv2d_stats_nhwc."""
    return dict(tokens=tuple(tokens), B=B, H=H, W=W, cin=cin, n=n, mode=mode, k=k, s=s, p=p, kind=kind,
                ldx=cin if ldx is None else ldx, ldy=n + LDY_PAD if ldy is None else ldy, types=tuple(types),
                stats=stats)


def _pp(tile, resw, ncb, n, overhang, uneven=0):
    return ("halo_pp", f"tile={tile}", f"RESW={resw}", "STATS=0", f"NCB={ncb}", f"N={n}", f"overhang={overhang}",
            f"uneven={uneven}")


def _halo(tile, cin, n, overhang):
    return ("halo", f"tile={tile}", f"Cin={cin}", f"N={n}", f"overhang={overhang}")


_SWEEP = (64, 128, 192, 256, 512, 1024)        # the persistent kernels' Cin set: NCB 2, 4, 6, 8, 16, 32
_WIDE_MODE = {64: "bn", 128: "res", 192: "none", 256: "bn", 512: "res", 1024: "none"}

FAMILY_CASES = (
    # halo_pp tile=Wide: exact 16 x 32 tiles.  32 samples of one tile x 2 channel blocks = 64 work items; the three
    # epilogue forms of the kernel (scale / shift / leaky, residual alone, nothing) alternate over the NCB sweep
    [_case(_pp("Wide", 0, c // 32, 128, 0), 32, 16, 32, c, 128, _WIDE_MODE[c], ldx=c + 8 * (c == 128)) for c in _SWEEP] +
    [_case(_pp("Wide", 1, 2, 64, 0), 64, 16, 32, 64, 64, "bn"),
     # 33 x 8 tiles = 264 work items on 256 CUs
     _case(_pp("Wide", 1, 2, 64, 0, uneven=1), 33, 64, 64, 64, 64, "res")] +
    # halo_pp tile=Img8: four whole 8 x 8 images per tile
    [_case(_pp("Img8", 1, 2, 64, 0), 4, 8, 8, 64, 64, "res")] +
    [_case(_pp("Img8", 0, c // 32, 128, 0), 4, 8, 8, c, 128, "bn" if c in (64, 512) else "none" if c == 256 else "res")
     for c in (64, 128, 256, 512, 1024)] +
    # halo_pp tile=Small: 16 x 16 tiles over a 14 x 14 image; overhang=0 only through the epilogue rule
    [_case(_pp("Small", int(c == 64), c // 32, 64, 1), 64, 14, 14, c, 64, "bn" if c != 128 else "res") for c in _SWEEP] +
    [_case(_pp("Small", 1, 2, 64, 0), 8, 48, 48, 64, 64, "prelu_y2", ldx=72),
     _case(_pp("Small", 0, 4, 64, 0), 64, 16, 16, 128, 64, "resfirst")] +
    # halo_pp tile=Pair: a 16 x 16 window of two samples (64 pairs x 4 channel blocks = 256 work items)
    [_case(_pp("Pair", 0, c // 32, 256, 1), 128, 14, 14, c, 256, "bn" if c != 256 else "res") for c in _SWEEP] +
    [_case(_pp("Pair", 0, 4, 128, 1), 64, 28, 28, 128, 128, "prelu_y2"),
     _case(_pp("Pair", 0, 4, 128, 1), 64, 28, 28, 128, 128, "resfirst_y2")] +
    # halo (non-persistent)
    [_case(_halo("Wide", 96, 128, 0), 16, 32, 32, 96, 128, "bn"),
     _case(_halo("Wide", 32, 64, 0), 32, 32, 32, 32, 64, "res"),
     _case(_halo("Wide", 64, 64, 0), 32, 32, 32, 64, 64, "prelu_y2"),
     _case(_halo("Wide", 64, 64, 0), 32, 32, 32, 64, 64, "tanh"),
     _case(_halo("Wide", 64, 64, 0), 32, 32, 32, 64, 64, "bn", ldy=68),        # ldy % 8 != 0: the 8-byte stores
     _case(_halo("Wide", 64, 576, 0), 4, 32, 32, 64, 576, "bn", ldx=72),       # N > 512
     _case(_halo("Small", 64, 64, 0), 64, 16, 16, 64, 64, "bn"),
     _case(_halo("Small", 96, 128, 1), 8, 28, 28, 96, 128, "res"),
     _case(_halo("Small", 64, 576, 1), 8, 14, 14, 64, 576, "none")] +
    # convT_halo: 4x4/s2/p1 deconv on 8 x 16 input tiles, 128 workgroups
    [_case(("convT_halo", "BN=64", "Cin=64", "N=128", "res=0"), 64, 8, 16, 64, 128, "bn", kind="T", ldy=160),
     _case(("convT_halo", "BN=64", "Cin=96", "N=128", "res=1"), 32, 16, 16, 96, 128, "res", kind="T", ldx=104),
     _case(("convT_halo", "BN=32", "Cin=64", "N=32", "res=0"), 128, 8, 16, 64, 32, "none", kind="T"),
     _case(("convT_halo", "BN=32", "Cin=32", "N=32", "res=1"), 32, 16, 32, 32, 32, "bn_res", kind="T")] +
    # s2_patch: 4x4/s2 and 3x3/s2 on 8 x 16 output tiles
    [_case(("s2_patch", "K=4", "ncb=1", "N=64", "overhang=0"), 32, 16, 32, 32, 64, "bn", k=4, s=2, ldx=64),
     _case(("s2_patch", "K=4", "ncb=2", "N=128", "overhang=0"), 2, 64, 64, 64, 128, "none", k=4, s=2),
     _case(("s2_patch", "K=3", "ncb=2", "N=64", "overhang=0"), 4, 16, 32, 64, 64, "bn", s=2),
     _case(("s2_patch", "K=3", "ncb=1", "N=64", "overhang=1"), 1, 14, 28, 32, 64, "resfirst", s=2),
     _case(("s2_patch", "K=3", "ncb=2", "N=128", "overhang=1"), 2, 28, 28, 64, 128, "prelu_res_y2", s=2)] +
    # first: the encoder's 3 -> 32 4x4/s2; MFMA on the 4-channel layout where Wo % 64 == 0 (M = 64: one chunk of a
    # wave's share; M = 1024: whole shares), else the scalar kernel (also in fp32)
    [_case(("first", "mfma", "chunktail=1"), 1, 2, 128, 3, 32, "bn", k=4, s=2, ldx=4),
     _case(("first", "mfma", "chunktail=0"), 1, 32, 128, 3, 32, "bn", k=4, s=2, ldx=4),
     _case(("first", "scalar", "mtail=1"), 1, 6, 10, 3, 32, "bn", k=4, s=2, ldx=3, types=T16 + ("f32",)),
     _case(("first", "scalar", "mtail=0"), 2, 16, 64, 3, 32, "bn", k=4, s=2, ldx=4, types=T16 + ("f32",))] +
    # stem3x3: ArcFace's 3 -> 64 on the 4-channel layout (bf16 only)
    [_case(("stem3x3", "y2=1", "mtail=1", "chunktail=1"), 2, 9, 9, 3, 64, "prelu_y2", ldx=4, types=("bf16",)),
     _case(("stem3x3", "y2=0", "mtail=0", "chunktail=0"), 1, 32, 32, 3, 64, "bn", ldx=4, types=("bf16",)),
     _case(("stem3x3", "y2=1", "mtail=0", "chunktail=1"), 1, 8, 8, 3, 64, "y2", ldx=4, types=("bf16",))]
)
# every tile=Wide and tile=Img8 row again with the InstanceNorm partials (STATS=1)
FAMILY_CASES += [dict(c, stats=True, tokens=tuple("STATS=1" if t == "STATS=0" else t for t in c["tokens"]))
                 for c in FAMILY_CASES if c["tokens"][0] == "halo_pp" and c["tokens"][1] in ("tile=Wide", "tile=Img8")]


def case_id(c):
    return "-".join([c["tokens"][0], c["tokens"][1].replace("tile=", "").replace("=", "")] +
                    [f"B{c['B']}", f"{c['H']}x{c['W']}", f"{c['cin']}to{c['n']}", c["mode"]] +
                    ([f"ldy{c['ldy']}"] if c["ldy"] != c["n"] + LDY_PAD else []) + (["stats"] if c["stats"] else []))


def case_tokens(c, t):
    """The tokens of the case's line for storage type name ``t``."""
    return c["tokens"] + ("t=" + t,)
