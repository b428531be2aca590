"""CPU tests of convolution kernel selection: conv_path + igemm_plan / halo_plan through ghost_conv_plan (no device).

ghost_conv_plan returns the plan-log lines one conv launch of a descriptor would write (the kernel's, then a split-K
reduction's) and the workspace it needs, from the launch's own family rule, planners and formatters, so a retuned
threshold shows here, on a machine with no GPU, before tests/test_gpu_parity.py and tests/test_batch_sweep.py see it
on one.
"""
import ctypes as C
import os
import re

import pytest

import conv_cases as K
from ghost_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F16, F32 = _lib.BF16, _lib.F16, _lib.F32
FWD, T4S2 = 0, 1
RES, RES_FIRST, PRELU, Y2, U8, TANH, IN_PART = 1, 2, 4, 8, 16, 32, 64     # GHOST_CONV_PLAN_* (include/ghost_amd.h)
NSEM, NCU = 4096, 256                                                    # the runtime's counters, the MI355X


def rup(v, m):
    return (v + m - 1) // m * m


@pytest.fixture(scope="module")
def lib():
    from ghost_amd import build
    build.build(verbose=False)
    return _lib.load()


def plan(lib, dt, B, H, W, cin, n, k=3, s=1, p=1, kind=FWD, to=None, ldx=None, ldy=None, npad=None, kpad=None, epi=0,
         split_k=0, min_wgs=0, nsem=0, ncu=NCU, flags=0):
    """(the lines of the launch, its workspace bytes), or (None, None) where conv_launch would refuse the descriptor.
    Packed as pack.py packs: Npad = Cout up to 128, Kpad = K up to 32."""
    kk = 4 * cin if kind == T4S2 else k * k * cin
    ws = C.c_int64(-1)
    buf = C.create_string_buffer(512)
    r = lib.ghost_conv_plan(dt, dt if to is None else to, kind, B, H, W, cin, cin if ldx is None else ldx, n,
                            rup(n, 128) if npad is None else npad, rup(kk, 32) if kpad is None else kpad, k, k, s, p,
                            n if ldy is None else ldy, epi, split_k, min_wgs, nsem, ncu, flags, C.byref(ws), buf, 512)
    if r < 0:
        assert r == -1
        return None, None
    assert r == len(buf.value) + 1
    return buf.value.decode().split("\n"), ws.value


def line(lib, *a, **k):
    """The kernel's line alone."""
    lines, _ = plan(lib, *a, **k)
    return lines[0] if lines else None


def has(sig, *tokens):
    return sig is not None and all(t in sig.split() for t in tokens)


# ----------------------------------------------------------------------------------------
# the op tests' edge cases (tests/conv_cases.py), with test_gpu_parity's strides
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("cin,ldx,cout,k,s,p,B,H,W,split_k,tokens,reduce", K.IGEMM_EDGES)
def test_igemm_edge_signatures(lib, dt, cin, ldx, cout, k, s, p, B, H, W, split_k, tokens, reduce):
    """What test_igemm_edge_plans asserts of the plan log on the GPU."""
    lines, _ = plan(lib, BF16 if dt == "bf16" else F16, B, H, W, cin, cout, k, s, p, ldx=ldx, ldy=cout + K.IGEMM_LDY_PAD,
                    split_k=split_k)
    assert has(lines[0], *K.gemm_tokens(tokens, dt)), (tokens, lines)
    assert [l.split()[0] for l in lines[1:]] == ([reduce] if reduce else []), lines


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("cout,tokens", K.CONVT_EDGES)
def test_convT_edge_signatures(lib, dt, cout, tokens):
    """What test_convT_igemm_edge_plans asserts of the plan log on the GPU."""
    lines, _ = plan(lib, BF16 if dt == "bf16" else F16, 1, K.CONVT_H, K.CONVT_W, K.CONVT_CIN, cout, kind=T4S2,
                    ldy=cout + K.CONVT_LDY_PAD)
    assert has(lines[0], *tokens), (tokens, lines)
    assert [l.split()[0] for l in lines[1:]] == ["splitk_reduce4"], lines


def _family_rows():
    return [pytest.param(c, t, id=f"{K.case_id(c)}-{t}") for c in K.FAMILY_CASES for t in c["types"]]


@pytest.mark.parametrize("c,t", _family_rows())
def test_family_case_signatures(lib, c, t):
    """What test_conv_ops.py asserts of the plan log on the GPU: every case of the families off the implicit GEMM
    gives one line, its kernel's with its tokens, and needs no workspace (first: its 6 KB of fp32 weights).  The
    STATS twins ask with the InstanceNorm partials set, as ghost_conv2d_stats_nhwc launches them."""
    dt = {"bf16": BF16, "f16": F16, "f32": F32}[t]
    flags = K.mode_flags(c["mode"]) | (IN_PART if c["stats"] else 0)
    lines, ws = plan(lib, dt, c["B"], c["H"], c["W"], c["cin"], c["n"], c["k"], c["s"], c["p"],
                     kind=T4S2 if c["kind"] == "T" else FWD, ldx=c["ldx"], ldy=c["ldy"], flags=flags)
    assert lines and len(lines) == 1, lines
    assert lines[0].split()[0] == c["tokens"][0] and has(lines[0], *K.case_tokens(c, t)), (c["tokens"], lines)
    assert ws == (32 * 48 * 4 if c["tokens"][0] == "first" else 0), ws


def test_family_cases_cover_both_types_and_are_distinct():
    ids = [K.case_id(c) for c in K.FAMILY_CASES]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    for c in K.FAMILY_CASES:
        assert set(c["types"]) >= ({"bf16"} if c["tokens"][0] == "stem3x3" else {"bf16", "f16"}), c


# ----------------------------------------------------------------------------------------
# replay of DESIGN.md section 2a: the attribute encoder's 13 convolutions, as the parent launchers logged them on
# the MI355X
# ----------------------------------------------------------------------------------------
# aei_runtime.hip kEncDown, kEncUpUnet / kEncUpLink
ENC_DOWN = [(3, 32), (32, 64), (64, 128), (128, 256), (256, 512), (512, 1024), (1024, 1024)]
ENC_UP = {"unet2_bf16": [(1024, 1024), (2048, 512), (1024, 256), (512, 128), (256, 64), (128, 32)],
          "linknet3_bf16": [(1024, 1024), (1024, 512), (512, 256), (256, 128), (128, 64), (64, 32)]}


def _attr_channels(config, level):
    """aei_runtime.hip attr_geom: channels of z_attr_level (unet: the deconv's channels and the skip's)."""
    link = config.startswith("linknet")
    if level == 1:
        return 1024
    if level == 8:
        return 32 if link else 64
    return ENC_UP[config][level - 2][1] * (1 if link else 2)


def encoder_descs(config):
    """(args, kwargs) of plan() without the batch, for conv1..7 and deconv1..6 of MLAttrEncoder as encoder() builds
    them: unet writes feat_j into z_attr_{8-j} beside the deconv's channels, linknet adds the skip as a residual."""
    link = config.startswith("linknet")
    out, side, ldx = [], 256, 4
    for i, (ci, co) in enumerate(ENC_DOWN, 1):
        ldy = 1024 if i == 7 else co if link else _attr_channels(config, 8 - i)
        out.append(((side, side, ci, co, 4, 2, 1), dict(ldx=ldx, ldy=ldy)))
        side, ldx = side // 2, ldy
    for i, (_, co) in enumerate(ENC_UP[config], 1):
        cin = _attr_channels(config, i)
        out.append(((2 ** i, 2 ** i, cin, co), dict(kind=T4S2, ldy=_attr_channels(config, i + 1),
                                                    flags=RES if link else 0)))
    return out


def _sizes(spec):
    """'all' | '1-7' | '2, 3' | '4-64/4' | mixes -> the set of batch sizes (tools/plan_sweep.py's notation)."""
    out = set()
    for part in spec.split(","):
        part = part.strip()
        if part == "all":
            return set(range(1, 65))
        m = re.fullmatch(r"(\d+)(?:-(\d+)(?:/(\d+))?)?", part)
        a, b, d = int(m.group(1)), int(m.group(2) or m.group(1)), int(m.group(3) or 1)
        out.update(range(a, b + 1, d))
    return out


def _design_rows(config):
    """signature -> batch sizes, every row of DESIGN.md's table of ``config``."""
    with open(os.path.join(REPO, "DESIGN.md")) as f:
        lines = f.read().split("\n")
    i = next(i for i, l in enumerate(lines) if l.startswith(f"**{config}**"))
    rows = {}
    for l in lines[i + 1:]:
        if l.startswith("**"):
            break
        m = re.fullmatch(r"\| `([^`]*)` \| ([^|]*) \|", l)
        if m:
            rows[m.group(1)] = _sizes(m.group(2))
    return rows


def _encoder_only(sig):
    """Rows that only the encoder's convolutions produce: the deconvs' and the single-kernel families'."""
    return "kind=T4S2" in sig.split() or sig.split()[0] in ("convT_halo", "s2_patch", "first")


@pytest.mark.parametrize("config", sorted(ENC_UP))
def test_replay_of_the_design_tables(lib, config):
    """The encoder-only rows at exactly the table's batch sizes, none extra, none missing; every other line of the 13
    descriptors a row of the table at a batch size the row lists (generator launches share those rows)."""
    rows = _design_rows(config)
    got = {}
    for a, k in encoder_descs(config):
        for B in range(1, 65):
            lines, _ = plan(lib, BF16, B, *a, nsem=NSEM, ncu=NCU, **k)
            assert lines, (a, k, B)
            for sig in lines:
                got.setdefault(sig, set()).add(B)
    want = {s: b for s, b in rows.items() if _encoder_only(s)}
    assert len(want) >= 15, want
    mine = {s: b for s, b in got.items() if _encoder_only(s)}
    assert sorted(mine) == sorted(want), sorted(set(mine) ^ set(want))
    for sig in want:
        assert mine[sig] == want[sig], (sig, sorted(mine[sig] ^ want[sig]))
    for sig, sizes in got.items():
        assert sig in rows and sizes <= rows[sig], (sig, sorted(sizes - rows.get(sig, set())))


def test_replay_spot_values(lib):
    """The issue's spot values, spelled out (each a row of the unet2_bf16 table)."""
    every = range(1, 65)

    def where(a, *tokens, **k):
        return {B for B in every if has(line(lib, BF16, B, *a, nsem=NSEM, **k), *tokens)}
    assert where((16, 16, 1024, 1024), "halo", "tile=Small", "Cin=1024", "N=1024", "overhang=0") == set(range(4, 65))
    assert line(lib, BF16, 4, 16, 16, 1024, 1024) == "halo t=bf16 tile=Small Cin=1024 N=1024 overhang=0"
    assert where((16, 16, 2048, 512), "halo", "tile=Small", "Cin=2048", "N=512") == set(range(8, 65))
    assert where((8, 8, 1024, 1024), "halo_pp", "tile=Img8", "NCB=32", "N=1024") == set(range(4, 65, 4))
    blk8 = (256, 256, 64, 64)
    assert where(blk8, "halo_pp", "tile=Wide", "RESW=1", "uneven=0") == {1} | set(range(2, 65, 2))
    assert where(blk8, "halo_pp", "tile=Wide", "RESW=1", "uneven=1") == set(range(3, 65, 2))
    # the InstanceNorm partials change STATS alone
    assert line(lib, BF16, 2, *blk8, flags=IN_PART) == "halo_pp t=bf16 tile=Wide RESW=1 STATS=1 NCB=2 N=64 overhang=0 uneven=0"
    assert line(lib, BF16, 2, *blk8) == "halo_pp t=bf16 tile=Wide RESW=1 STATS=0 NCB=2 N=64 overhang=0 uneven=0"


# ----------------------------------------------------------------------------------------
# both sides of every threshold of the planners
# ----------------------------------------------------------------------------------------
def test_igemm_thresholds(lib):
    def g(B, H, W, cin, n, **k):        # a 1x1 conv: no other family takes it
        return line(lib, BF16, B, H, W, cin, n, 1, 1, 0, **k)
    # N > 64 outside the deep ring: 128-row tiles from 512 tiles of 128 x 128, else 64-row tiles
    assert has(g(1, 256, 256, 64, 128), "glds", "128x128", "stages=3")              # M = 65536: 512 tiles
    assert has(g(1, 256, 255, 64, 128), "glds", "64x128", "stages=3")               # 510
    # BK = 64 from Kpad 4096 (the ring kernel holds BK = 32 only)
    assert has(g(1, 16, 16, 4096, 128), "igemm", "64x128x64")
    assert has(g(1, 16, 16, 4032, 128), "glds", "64x128")
    # the deep ring (N >= 256, N % 128 == 0, Kpad >= 1024): M <= 8192 and fewer than 256 tiles of 128 x 128 ...
    assert has(g(8, 32, 32, 1024, 256), "glds", "stages=8")                         # M = 8192
    assert not has(g(1, 32, 257, 1024, 256), "stages=8")                            # M = 8224
    assert not has(g(8, 32, 32, 1024, 512), "stages=8")                             # 64 x 4 = 256 tiles
    assert has(g(1, 32, 252, 1024, 512), "glds", "stages=8")                        # 63 x 4 = 252
    assert not has(g(8, 32, 32, 992, 256), "stages=8") and not has(g(8, 32, 32, 1024, 128), "stages=8")
    # ... or deep_k: Kpad >= 4096 up to M = 16384 and 512 tiles
    assert has(g(16, 32, 32, 4096, 256), "glds", "stages=8")                        # M = 16384, 256 tiles
    assert not has(g(1, 32, 513, 4096, 256), "stages=8")                            # M = 16416
    assert not has(g(16, 32, 32, 4064, 256), "stages=8")                            # Kpad 4064
    assert not has(g(16, 32, 32, 4096, 512), "stages=8")                            # 128 x 4 = 512 tiles
    assert has(g(1, 32, 508, 4096, 512), "glds", "stages=8")                        # 127 x 4 = 508
    # the deep ring splits K below 256 tiles
    assert has(g(16, 32, 32, 4096, 256), "stages=8", "split=0")                     # 128 x 2 = 256 tiles
    assert has(g(1, 32, 508, 4096, 256), "stages=8", "split=1")                     # 127 x 2 = 254
    # the other tiles split below 256 tiles from 16 K steps
    assert has(g(1, 64, 64, 512, 128), "64x128", "split=1")                         # 64 tiles, nk = 16
    assert has(g(1, 64, 64, 480, 128), "64x128", "split=0")                         # nk = 15
    assert has(g(1, 64, 255, 512, 128), "64x128", "split=1")                        # 255 tiles
    assert has(g(4, 64, 64, 512, 128), "64x128", "split=0")                         # 256 tiles, nk = 16
    # exactly one round of 256 tiles splits from 64 K steps
    assert has(g(4, 64, 64, 2048, 128), "64x128", "split=1")                        # nk = 64
    assert has(g(4, 64, 64, 2016, 128), "64x128", "split=0")                        # nk = 63
    assert has(g(1, 64, 257, 2048, 128), "64x128", "split=0")                       # 257 tiles
    # min_wgs moves the bound and switches the one-round rule off
    assert has(g(1, 64, 64, 512, 128, min_wgs=65), "split=1") and has(g(1, 64, 64, 512, 128, min_wgs=64), "split=0")
    assert has(g(4, 64, 64, 2048, 128, min_wgs=256), "split=0")
    # the fix-up: a tile's partials within the kernel's LDS (64 x 128 tiles: 30720 B, fixrows=M below BM rows) ...
    assert has(g(1, 3, 5, 512, 128, split_k=4, nsem=NSEM), "64x128", "fixup=std", "fixrows=M")   # 4 x 15 x 128 x 4 = 30720
    assert has(g(1, 4, 4, 512, 128, split_k=4, nsem=NSEM), "64x128", "fixup=none")               # 4 x 16 x 128 x 4 = 32768
    # ... and within 32 KB (the deep ring's LDS holds 128 KB)
    assert has(g(1, 4, 4, 1024, 256, split_k=4, nsem=NSEM), "stages=8", "fixup=std", "fixrows=M")   # 32768
    assert has(g(1, 1, 17, 1024, 256, split_k=4, nsem=NSEM), "stages=8", "fixup=none")              # 34816
    # ... with a counter per tile
    assert has(g(1, 3, 5, 512, 256, split_k=4, nsem=2), "fixup=std") and has(g(1, 3, 5, 512, 256, split_k=4, nsem=1), "fixup=none")
    assert has(g(1, 3, 5, 512, 128, split_k=4), "fixup=none")
    # a fix-up leaves no reduction line; without it the reduction follows
    assert len(plan(lib, BF16, 1, 3, 5, 512, 128, 1, 1, 0, split_k=4, nsem=NSEM)[0]) == 1
    assert plan(lib, BF16, 1, 3, 5, 512, 128, 1, 1, 0, split_k=4)[0][1] == "splitk_reduce4 to=bf16 epi=STD"
    # 16-bit operands with an fp32 output: partials always, the reduction writes fp32
    lines, ws = plan(lib, BF16, 2, 1, 1, 512, 512, 1, 1, 0, to=F32)
    assert has(lines[0], "igemm", "ti=bf16", "to=bf16", "epi=SPLIT") and lines[1] == "splitk_reduce to=f32 epi=STD from=bf16"
    assert plan(lib, F16, 2, 1, 1, 512, 512, 1, 1, 0, to=F32)[0] is None      # no instance
    # weight rows the last tile reads must exist
    assert plan(lib, BF16, 1, 8, 8, 64, 130, 1, 1, 0, npad=130)[0] is None


def test_halo_thresholds(lib):
    def h(B, H, W, cin, n, **k):
        return line(lib, BF16, B, H, W, cin, n, **k)
    # 64 work items (tile x 64-channel block)
    assert has(h(4, 32, 32, 512, 512), "halo_pp", "tile=Wide") and h(3, 32, 32, 512, 512).split()[0] in ("glds", "igemm")
    # 16 x 16 tiles may overhang the image by a quarter of their pixels
    assert has(h(64, 14, 14, 64, 64), "halo_pp", "tile=Small", "overhang=1")        # 784 of 1024 >= 3/4
    assert h(64, 13, 13, 64, 64).split()[0] in ("glds", "igemm")                    # 676 of 1024
    # the Cin set of the persistent 16 x 32 form, and its N <= 512
    assert has(h(8, 64, 64, 192, 64), "halo_pp", "tile=Wide", "NCB=6") and has(h(8, 64, 64, 320, 64), "halo", "tile=Wide")
    assert has(h(1, 64, 64, 64, 512), "halo_pp", "tile=Wide") and has(h(1, 64, 64, 64, 576), "halo", "tile=Wide")
    # the pair rule: B even, N <= 256, a paired work item per CU
    assert has(h(64, 28, 28, 128, 128), "halo_pp", "tile=Pair")                     # 32 x 4 x 2 = 256 items
    assert has(h(62, 28, 28, 128, 128), "halo_pp", "tile=Small")                    # 248
    assert has(h(65, 28, 28, 128, 128), "halo_pp", "tile=Small")
    assert has(h(64, 28, 28, 128, 256), "halo_pp", "tile=Pair") and has(h(64, 28, 28, 128, 320), "halo_pp", "tile=Small")
    assert has(h(64, 28, 28, 128, 128, ncu=257), "halo_pp", "tile=Small")
    # in_part where the plan writes no partials is refused
    assert plan(lib, BF16, 64, 28, 28, 128, 128, flags=IN_PART)[0] is None


def test_conv_path_thresholds(lib):
    # convT_halo from 128 (input tile, channel block) workgroups
    assert line(lib, BF16, 16, 32, 32, 256, 64, kind=T4S2) == "convT_halo t=bf16 BN=64 Cin=256 N=64 res=0"
    assert has(line(lib, BF16, 15, 32, 32, 256, 64, kind=T4S2), "kind=T4S2")
    # the 4x4/s2 patch kernel from 32 workgroups
    assert line(lib, BF16, 2, 64, 64, 64, 128, 4, 2, 1) == "s2_patch t=bf16 K=4 ncb=2 N=128 overhang=0"
    assert line(lib, BF16, 1, 64, 64, 64, 128, 4, 2, 1).split()[0] in ("glds", "igemm")
    # a forced split sends everything to the GEMM
    for a, k in (((4, 32, 32, 512, 512), {}), ((16, 32, 32, 256, 64), dict(kind=T4S2)),
                 ((2, 64, 64, 64, 128, 4, 2, 1), {}), ((1, 256, 256, 3, 32, 4, 2, 1), dict(ldx=4))):
        assert line(lib, BF16, *a, **k).split()[0] not in ("glds", "igemm"), a
        assert has(line(lib, BF16, *a, split_k=2, **k), "split=1"), a


def test_workspace(lib):
    """npar * nsplit * M * NT * 4 exactly when the GEMM writes partials; 0 for every other path but first's 6 KB."""
    # nk = 27 in 4 splits (7, 7, 7, 6), M = 120, one 128-column tile
    assert plan(lib, BF16, 2, 6, 10, 96, 128, split_k=4)[1] == 1 * 4 * 120 * 128 * 4
    # the deconv edge case: nk = 68 in 8 splits of 9, M = 24 per phase, four phases, 64 / 128 columns
    assert plan(lib, BF16, 1, K.CONVT_H, K.CONVT_W, K.CONVT_CIN, 64, kind=T4S2)[1] == 4 * 8 * 24 * 64 * 4
    assert plan(lib, BF16, 1, K.CONVT_H, K.CONVT_W, K.CONVT_CIN, 128, kind=T4S2)[1] == 4 * 8 * 24 * 128 * 4
    # N tail: the tiles' padded extent, 2 x 128 columns for Cout 130
    assert plan(lib, BF16, 3, 5, 7, 64, 130, split_k=2)[1] == 1 * 2 * 105 * 256 * 4
    # fp32 from 16-bit: one slab of partials without a split
    assert plan(lib, BF16, 2, 1, 1, 512, 512, 1, 1, 0, to=F32, split_k=1)[1] == 1 * 1 * 2 * 512 * 4
    # an unsplit GEMM and the other families need none
    lines, ws = plan(lib, BF16, 2, 10, 6, 160, 96, 1, 2, 0)
    assert has(lines[0], "split=0") and ws == 0
    for a, k, name in (((4, 32, 32, 512, 512), {}, "halo_pp"), ((4, 16, 16, 1024, 1024), {}, "halo"),
                       ((16, 32, 32, 256, 64), dict(kind=T4S2), "convT_halo"),
                       ((2, 64, 64, 64, 128, 4, 2, 1), {}, "s2_patch"),
                       # IResNet's 3x3/s2 with the IBasicBlock epilogue: the patch kernel, sized as such
                       ((4, 56, 56, 64, 128, 3, 2, 1), dict(flags=PRELU | RES | Y2), "s2_patch"),
                       ((4, 112, 112, 3, 64), dict(ldx=4, flags=PRELU | Y2), "stem3x3")):
        lines, ws = plan(lib, BF16, *a, **k)
        assert lines[0].split()[0] == name and ws == 0, (lines, ws)
    lines, ws = plan(lib, BF16, 1, 256, 256, 3, 32, 4, 2, 1, ldx=4)
    assert lines == ["first mfma t=bf16 chunktail=0"] and ws == 32 * 48 * 4
    assert plan(lib, F32, 1, 256, 256, 3, 32, 4, 2, 1, ldx=3) == (["first scalar t=f32 mtail=0"], 32 * 48 * 4)


# ----------------------------------------------------------------------------------------
# what only the runtimes select (tests/test_fused_reduce_ops.py on the GPU): the split-K fix-up with arrival counters,
# the GEMMs whose output type differs from their operand type
# ----------------------------------------------------------------------------------------
DT = {"bf16": BF16, "f16": F16, "f32": F32}


def fixup_plan(lib, c, t, nsem):
    return plan(lib, DT[t], c["B"], c["H"], c["W"], c["cin"], c["n"], c["k"], c["s"], c["p"],
                kind=T4S2 if c["kind"] == "T" else FWD, ldy=c["n"] + K.IGEMM_LDY_PAD, split_k=c["split_k"], nsem=nsem)


def fixup_tokens(c, t):
    return c["tokens_f32"] if t == "f32" else K.gemm_tokens(c["tokens"], t)


@pytest.mark.parametrize("c,t", [pytest.param(c, t, id=f"{c['name']}-{t}") for c in K.FIXUP_CASES for t in c["types"]])
def test_fixup_case_signatures(lib, c, t):
    """With the case's counters: its GEMM line, and no reduction exactly when the line says fixup=std.  Without
    counters the same GEMM but fixup=none, followed by the case's reduction kernel; the workspace is the same."""
    lines, ws = fixup_plan(lib, c, t, c["nsem"])
    assert has(lines[0], *fixup_tokens(c, t)), (fixup_tokens(c, t), lines)
    fused = "fixup=none" not in c["tokens"]
    assert has(lines[0], "fixup=std" if fused else "fixup=none")
    assert [l.split()[0] for l in lines[1:]] == ([] if fused else [c["reduce"]]), lines
    plain, ws0 = fixup_plan(lib, c, t, 0)
    assert plain[0] == lines[0].replace("fixup=std", "fixup=none").replace(" fixrows=M", "").replace(" fixrows=BM", "")
    assert plain[1] == f"{c['reduce']} to={t} epi=STD" and len(plain) == 2 and ws0 == ws > 0


def test_fixup_counter_boundaries(lib):
    """A counter per (phase, tile): the cases at nsem == tiles fuse, their twins at nsem - 1 do not; both otherwise
    the same descriptor."""
    by = {c["name"]: c for c in K.FIXUP_CASES}
    for hi, lo in (("T4S2-nsem4", "T4S2-nsem3"), ("nsem2", "nsem1")):
        a, b = by[hi], by[lo]
        assert {k: v for k, v in a.items() if k not in ("name", "tokens", "nsem")} == \
               {k: v for k, v in b.items() if k not in ("name", "tokens", "nsem")}
        assert a["nsem"] == b["nsem"] + 1
        for t in a["types"]:
            assert has(fixup_plan(lib, a, t, a["nsem"])[0][0], "fixup=std")
            assert has(fixup_plan(lib, a, t, a["nsem"] - 1)[0][0], "fixup=none")
            assert has(fixup_plan(lib, a, t, a["nsem"] + 1)[0][0], "fixup=std")


@pytest.mark.parametrize("name,tokens,tokens_f32,B,H,W,c,ca,split_k,types", K.FIXUP_AAD_CASES,
                         ids=[r[0] for r in K.FIXUP_AAD_CASES])
def test_fixup_aad_case_signatures(lib, name, tokens, tokens_f32, B, H, W, c, ca, split_k, types):
    """The GEMM of ghost_aad_layer_rt_nhwc on aad_cases' strides (channel counts + 8)."""
    for t in types:
        lines, _ = plan(lib, DT[t], B, H, W, ca, 2 * c, 1, 1, 0, ldx=ca + 8, ldy=c + 8, epi=1, split_k=split_k, nsem=K.NSEM)
        want = tokens_f32 if t == "f32" else K.gemm_tokens(tokens, t)
        assert len(lines) == 1 and has(lines[0], *want), (want, lines)
        plain, _ = plan(lib, DT[t], B, H, W, ca, 2 * c, 1, 1, 0, ldx=ca + 8, ldy=c + 8, epi=1, split_k=split_k)
        assert has(plain[0], "fixup=none") and plain[1] == f"splitk_reduce4 to={t} epi=AAD", plain


@pytest.mark.parametrize("to", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("name,B,Kc,N,split_k,nsem,tokens,reduce", K.LINEAR_CASES, ids=[r[0] for r in K.LINEAR_CASES])
def test_linear_case_signatures(lib, to, name, B, Kc, N, split_k, nsem, tokens, reduce):
    lines, _ = plan(lib, F32, B, 1, 1, Kc, N, 1, 1, 0, to=DT[to], ldy=N + K.LINEAR_LDY_PAD, split_k=split_k, nsem=nsem)
    assert has(lines[0], "to=" + to, *tokens), (tokens, lines)
    assert lines[1:] == ([f"{reduce} to={to} epi=STD"] if reduce else []), lines


@pytest.mark.parametrize("n,B,nsem", K.HEAD_CASES)
def test_head_case_signatures(lib, n, B, nsem):
    """16-bit operands, fp32 output: partials and splitk_reduce to=f32 with or without counters; bf16 only."""
    a = (B, K.HEAD_HW, K.HEAD_HW, K.HEAD_CIN, n, K.HEAD_HW, 1, 0)
    lines, ws = plan(lib, BF16, *a, to=F32, ldy=n + K.IGEMM_LDY_PAD, nsem=nsem)
    assert has(lines[0], *K.HEAD_TOKENS) and has(lines[0], "ntail=%d" % (n % 128 != 0)), lines
    assert lines[1:] == [K.HEAD_REDUCE] and ws > 0, lines
    assert plan(lib, F16, *a, to=F32, nsem=nsem)[0] is None


def test_design_fused_signatures_are_covered_by_the_cases(lib):
    """Every fixup=std / fixup=aad line of DESIGN.md section 2 is the plan of a case above (what the closing test of
    tests/test_fused_reduce_ops.py asks of the plan log on the GPU)."""
    with open(os.path.join(REPO, "DESIGN.md")) as f:
        want = set(re.findall(r"\| `([^`]*fixup=(?:std|aad)[^`]*)` \|", f.read()))
    assert len(want) >= 10, want
    got = set()
    for c in K.FIXUP_CASES:
        got.update(fixup_plan(lib, c, t, c["nsem"])[0][0] for t in c["types"])
    for _, _, _, B, H, W, c, ca, split_k, types in K.FIXUP_AAD_CASES:
        got.update(plan(lib, DT[t], B, H, W, ca, 2 * c, 1, 1, 0, ldx=ca + 8, ldy=c + 8, epi=1, split_k=split_k,
                        nsem=K.NSEM)[0][0] for t in types)
    for _, B, Kc, N, split_k, nsem, _, _ in K.LINEAR_CASES:
        got.update(plan(lib, F32, B, 1, 1, Kc, N, 1, 1, 0, to=DT[to], split_k=split_k, nsem=nsem)[0][0] for to in DT)
    assert want <= got, sorted(want - got)


def test_rt_entries_reject_bad_arguments_without_launching(lib):
    """ghost_conv_rt_nhwc and ghost_aad_layer_rt_nhwc refuse before any launch: nothing reaches the plan log (host
    memory stands for every pointer: there is no device here)."""
    mem = (C.c_char * 4096)()
    a = C.addressof(mem)
    a += -a % 16
    e = _lib.ConvEpi()
    e.slope = 1.0

    def conv(ti=BF16, to=BF16, kind=FWD, x=a, epi=C.byref(e), npad=128, kpad=512, ws_bytes=1 << 20, sem=None, nsem=0):
        return lib.ghost_conv_rt_nhwc(ti, to, kind, x, 1, 3, 5, 512, 512, a, 128, npad, kpad, 1, 1, 1, 0, epi, a, 128, a,
                                      ws_bytes, sem, nsem, None)

    def aad(split_k=0, sem=None, nsem=0, h=a, ws_bytes=1 << 20):
        return lib.ghost_aad_layer_rt_nhwc(BF16, h, 128, a, 1024, 1, 2, 2, 128, 1024, a, 256, 1024, a, a, a, a, 256, 1.0,
                                           a, 128, a, ws_bytes, split_k, sem, nsem, None)
    _lib.plan_log(True)
    try:
        assert conv(epi=None) == -1 and conv(kind=2) == -1 and conv(x=None) == -1 and conv(ws_bytes=-1) == -1
        assert conv(sem=None, nsem=4) == -1 and conv(sem=a, nsem=0) == -1 and conv(sem=a, nsem=-1) == -1
        assert conv(npad=64) == -1 and conv(kpad=500) == -1 and conv(kpad=256) == -1      # packing the tiles overrun
        # type pairs without an instance: fp16 -> fp32, 16-bit -> the other 16-bit type, bf16 -> fp32 with a residual
        assert conv(ti=F16, to=F32) == -1 and conv(ti=BF16, to=F16) == -1 and conv(ti=F16, to=BF16) == -1
        e.res, e.ldres = a, 128
        assert conv(ti=BF16, to=F32) == -1
        e.res, e.split_k = None, -1
        assert conv() == -1
        e.split_k = 0
        assert b"ghost_conv_rt_nhwc" in lib.ghost_last_error()
        assert aad(split_k=-1) == -1 and aad(sem=None, nsem=1) == -1 and aad(sem=a, nsem=0) == -1 and aad(h=None) == -1
        assert aad(ws_bytes=-1) == -1 and aad(ws_bytes=64) == -3
    finally:
        _lib.plan_log(False)
    assert _lib.plan_log_read() == []
