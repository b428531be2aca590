"""CPU tests of AAD kernel selection: aad_path + aad_v3_plan / aad_wide_plan through ghost_aad_plan (no device).

ghost_aad_plan returns the plan-log signature a launch of a shape would write, from the launch's own path rule,
planner and formatter, so a retuned heuristic shows here, on a machine with no GPU, before tests/test_aad_ops.py and
tests/test_batch_sweep.py see it on one.
"""
import ctypes as C
import os
import re

import pytest

import aad_cases as A
from ghost_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = _lib.BF16


@pytest.fixture(scope="module")
def lib():
    from ghost_amd import build
    build.build(verbose=False)
    return _lib.load()


def plan(lib, dt, B, H, W, c, ca, L=1, up=0, zpm=0, slope=0.0, lda=None, ldh=None, ldo=None):
    """The signature of the launch, or None where ghost_aad_plan answers GHOST_EINVAL (no aad_v3 / aad_wide kernel)."""
    ldo = ldo or [c] * L
    buf = C.create_string_buffer(256)
    n = lib.ghost_aad_plan(dt, B, H, W, c, ca, L, up, zpm, slope, ca if lda is None else lda, c if ldh is None else ldh,
                           (C.c_int * L)(*ldo[:L]), buf, 256)
    if n < 0:
        assert n == -1
        return None
    assert n == len(buf.value) + 1
    return buf.value.decode()


@pytest.mark.parametrize("k", A.CASES, ids=A._id)
def test_case_signatures(lib, k):
    """What assert_plan checks on the GPU for every case of tests/test_aad_ops.py, with that test's strides."""
    c, ca = k["c"], k["ca"]
    sig = plan(lib, _lib.gdtype(k["dt"]), k["B"], k["H"], k["W"], c, ca, k["L"], k["up"], 0, k["slope"], ca + A.PAD,
               c + A.PAD, [c + A.PAD, c + 2 * A.PAD])
    assert sig is not None and sig.split()[0] == k["kernel"], sig
    assert all(t in sig.split() for t in A._tokens(k)), (A._tokens(k), sig)


# ----------------------------------------------------------------------------------------
# replay of DESIGN.md section 2a: the aad_* rows of two tables, as the parent launchers logged them on the MI355X
# ----------------------------------------------------------------------------------------
# One entry per AAD launch of a generator pass: (C, Ca, image side, L, up, zp_mask, ldo), with the pipeline's strides
# (lda = Ca, ldh = C; ldo = C, 2 C for an output inside the concatenation, 32 for a tap-partial buffer) and the first
# DESIGN.md line of the table that holds its rows.  A block's first group is its layer 0 with last_add_block (L = 2
# where one launch takes both), the others one layer each; a C = 256 / C = 128, Ca = 32 pair launches one layer at a
# time.  The 2 x 2 .. 8 x 8 stages (Ca >= 1024, or too few pixels) have no aad_v3 / aad_wide kernel.
STAGES = {
    "unet2_bf16": [                                        # DESIGN.md:120 (its aad_* rows: 124-204)
        (1024, 1024, 2, 1, 0, 0, [1024]), (1024, 2048, 4, 1, 0, 0, [1024]), (1024, 1024, 8, 1, 0, 0, [1024]),
        (1024, 512, 16, 1, 0, 0, [1024]), (1024, 512, 16, 1, 0, 0, [2048]),     # :130, :152, :162, :177, :183
        (512, 256, 32, 1, 0, 0, [512]), (512, 256, 32, 1, 0, 0, [1024]),        # :129, :151, :161, :176, :186 ...
        (256, 128, 64, 1, 0, 0, [256]), (256, 128, 64, 1, 0, 0, [512]),         # :128, :150, :184, :192
        (128, 64, 128, 2, 1, 0, [128, 256]), (128, 64, 128, 1, 0, 0, [256]),    # :125, :160, :185, :193, :203; :124, :159
        (64, 64, 256, 2, 1, 2, [64, 32]), (64, 64, 256, 1, 0, 1, [32]),         # :127, :175; :126
    ],
    "linknet3_bf16": [                                     # DESIGN.md:337 (its aad_* rows: 341-417)
        (1024, 1024, 2, 1, 0, 0, [1024]), (1024, 1024, 4, 1, 0, 0, [1024]),
        (1024, 512, 8, 1, 0, 0, [1024]),                                        # :379, :392, :405
        (1024, 256, 16, 1, 0, 0, [1024]), (1024, 256, 16, 1, 0, 0, [2048]),     # :345, :377, :390, :403, :411
        (512, 128, 32, 1, 0, 0, [512]), (512, 128, 32, 1, 0, 0, [1024]),        # :347, :369, :378, :391, :404 ...
        (256, 64, 64, 1, 0, 0, [256]), (256, 64, 64, 1, 0, 0, [512]),           # :346, :368, :402, :410
        (128, 32, 128, 1, 0, 0, [128]), (128, 32, 128, 1, 0, 0, [256]),         # :342, :376
        (64, 32, 256, 2, 1, 2, [64, 32]), (64, 32, 256, 1, 0, 0, [64]), (64, 32, 256, 1, 0, 1, [32]),   # :344, :389; :341; :343
    ],
}


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
    """signature -> batch sizes of the aad_v3 / aad_wide family rows of DESIGN.md's table of ``config``."""
    with open(os.path.join(REPO, "DESIGN.md")) as f:
        lines = f.read().split("\n")
    i = next(i for i, l in enumerate(lines) if l.startswith(f"**{config}**"))
    rows = {}
    for l in lines[i + 1:]:
        if l.startswith("**"):
            break
        m = re.fullmatch(r"\| `(aad_(?!fused)[^`]*)` \| ([^|]*) \|", l)
        if m:
            rows[m.group(1)] = _sizes(m.group(2))
    return rows


@pytest.mark.parametrize("config", sorted(STAGES))
def test_replay_of_the_design_tables(lib, config):
    """Every signature of the table at exactly the table's batch sizes, and no signature the table does not hold."""
    want = _design_rows(config)
    assert len(want) >= 20, want
    got = {}
    for c, ca, n, L, up, zpm, ldo in STAGES[config]:
        for B in range(1, 65):
            sig = plan(lib, BF16, B, n, n, c, ca, L, up, zpm, 0.0, ca, c, ldo)
            if sig is not None:
                got.setdefault(sig, set()).add(B)
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want)))
    for sig in want:
        assert got[sig] == want[sig], (sig, sorted(got[sig] ^ want[sig]))


def test_replay_spot_values(lib):
    """The issue's spot values, spelled out (each also a row of the tables above)."""
    def where(c, ca, n, L, up, zpm, ldo, name, token):
        return {B for B in range(1, 65)
                if (lambda s: s and s.split()[0] == name and token in s.split())(plan(lib, BF16, B, n, n, c, ca, L, up, zpm,
                                                                                       0.0, ca, c, ldo))}
    blk8 = (64, 64, 256, 2, 1, 2, [64, 32])
    assert where(*blk8, "aad_v5z_asm", "v5_ipw=1") == set(range(1, 8))
    assert where(*blk8, "aad_v5z_asm", "v5_ipw=2") == set(range(8, 65))
    blk7 = (128, 64, 128, 2, 1, 0, [128, 256])
    assert where(*blk7, "aad_v3_wide", "ppw=256") == {1, 2, 3}
    assert where(*blk7, "aad_v3_wide", "ppw=512") == set(range(4, 16))
    assert where(*blk7, "aad_v5_wide", "v5_ipw=1") == set(range(16, 32))
    assert where(*blk7, "aad_v5_wide", "v5_ipw=2") == set(range(32, 64))
    assert where(*blk7, "aad_v5_wide", "v5_ipw=4") == {64}
    blk4 = (1024, 512, 16, 1, 0, 0, [1024])
    for ppw, sizes in ((16, {1}), (32, {2, 3}), (64, set(range(4, 8))), (128, set(range(8, 16)))):
        assert where(*blk4, "aad_wide_deep", f"ppw={ppw}") == sizes
    assert where(*blk4, "aad_gemm", "Ca=512") == set(range(16, 65))


# ----------------------------------------------------------------------------------------
# both sides of every threshold of the planners
# ----------------------------------------------------------------------------------------
def test_thresholds(lib):
    def p(*a, **k):
        return plan(lib, BF16, *a, **k)
    # aad_v3 takes a launch from B * HW / ppw >= 32 workgroups (C = 64: 512 pixels each below 256 x 256)
    assert p(2, 64, 128, 64, 64).startswith("aad_v3 ") and p(1, 64, 128, 64, 64) is None
    assert p(8, 32, 32, 256, 128).startswith("aad_v3_wide ") and "ppw=256" in p(8, 32, 32, 256, 128)      # 32 of them
    assert p(7, 32, 32, 256, 128).startswith("aad_wide ")                                                   # 28: aad_wide
    # C = 128 / 256 halve their workgroups while B * HW / ppw < 128
    assert "ppw=512" in p(4, 128, 128, 128, 64) and "ppw=256" in p(3, 128, 128, 128, 64)
    assert "ppw=1024" in p(32, 64, 64, 256, 128) and "ppw=512" in p(31, 64, 64, 256, 128)
    # v5: two work items per workgroup from 256 workgroups of them; v5_wide from 256 work items
    up64 = dict(L=2, up=1, ldo=[64, 64])
    assert "v5_ipw=2" in p(8, 256, 256, 64, 64, **up64) and "v5_ipw=1" in p(7, 256, 256, 64, 64, **up64)
    up128 = dict(L=2, up=1, ldo=[128, 128])
    assert p(16, 128, 128, 128, 64, **up128).startswith("aad_v5_wide ")
    assert p(15, 128, 128, 128, 64, **up128).startswith("aad_v3_wide ")
    assert "v5_ipw=2" in p(32, 128, 128, 128, 64, **up128) and "v5_ipw=1" in p(31, 128, 128, 128, 64, **up128)
    assert "v5_ipw=4" in p(64, 128, 128, 128, 64, **up128) and "v5_ipw=2" in p(63, 128, 128, 128, 64, **up128)
    # aad_wide takes a launch from 256 workgroups at its smallest (16 pixels x one 64-channel tile)
    assert p(4, 8, 8, 1024, 512) == "aad_wide_deep t=bf16 C=1024 Ca=512 ppw=16" and p(3, 8, 8, 1024, 512) is None
    # aad_gemm from 128 of its 256 x 256 tiles
    assert p(16, 16, 16, 1024, 512) == "aad_gemm t=bf16 C=1024 Ca=512"
    assert p(15, 16, 16, 1024, 512) == "aad_wide_deep t=bf16 C=1024 Ca=512 ppw=128"
    assert p(32, 16, 16, 512, 512) == "aad_gemm t=bf16 C=512 Ca=512" and p(31, 16, 16, 512, 512).startswith("aad_wide_deep ")
    # HW % ppw: 64 x 132 is no multiple of the 512-pixel workgroup
    assert p(4, 64, 128, 64, 64) is not None and p(4, 64, 132, 64, 64) is None
    assert p(64, 16, 24, 1024, 512).startswith("aad_wide_deep ")      # HW % 256 != 0 keeps aad_gemm away
    # every leading dimension must be a multiple of 8 (16 bytes)
    ok = dict(lda=72, ldh=72, ldo=[72, 80])
    assert p(4, 64, 128, 64, 64, L=2, **ok) is not None
    for bad in (dict(ok, lda=68), dict(ok, ldh=68), dict(ok, ldo=[68, 80]), dict(ok, ldo=[72, 76])):
        assert p(4, 64, 128, 64, 64, L=2, **bad) is None, bad
    assert p(16, 16, 16, 1024, 512, lda=516) is None and p(16, 16, 16, 1024, 512, ldo=[1028]) is None
    # f32 has no register-epilogue kernel
    assert plan(lib, _lib.F32, 4, 64, 128, 64, 64) is None
