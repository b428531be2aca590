"""CPU tests of the InstanceNorm statistics' kernel selection: in_stats_plan through ghost_instnorm_plan (no device).

ghost_instnorm_plan returns the one line of the plan that in_stats / in_stats_up2x launch for a shape (kernel, chunk,
records per sample, ending), from the launcher's own planner, so a retuned chunk rule or a changed ending shows here,
on a machine with no GPU, before tests/test_fused_reduce_ops.py sees it on one.  The cases are stats_cases.CASES.
"""
import ctypes as C

import pytest

import stats_cases as S
from ghost_amd import _lib

DT = {"bf16": _lib.BF16, "f16": _lib.F16, "f32": _lib.F32}
EINVAL, ENOWS = -1, -3


@pytest.fixture(scope="module")
def lib():
    from ghost_amd import build
    build.build(verbose=False)
    return _lib.load()


def plan(lib, t, B, H, W, Cc, ldx=None, up=0, nsem=0):
    """(the plan's line, the workspace the entries ask for), or (None, None) where in_stats refuses the shape."""
    ws = C.c_int64(-1)
    buf = C.create_string_buffer(256)
    r = lib.ghost_instnorm_plan(DT[t], B, H, W, Cc, Cc if ldx is None else ldx, up, nsem, C.byref(ws), buf, 256)
    if r < 0:
        assert r == EINVAL
        return None, None
    assert r == len(buf.value) + 1
    return buf.value.decode(), ws.value


def fields(line):
    return dict(tok.split("=") for tok in line.split()[1:])


ROWS = [pytest.param(c, t, counters, id=S.case_id(c, t, counters))
        for c in S.CASES for t in c["types"] for counters in (True, False)]


@pytest.mark.parametrize("c,t,counters", ROWS)
def test_case_plans(lib, c, t, counters):
    """What test_fused_reduce_ops.py relies on: every case selects its kernel, chunk, record count and ending."""
    line, ws = plan(lib, t, c["B"], c["H"], c["W"], c["C"], c["ldx"], c["up"], c["nsem"] if counters else 0)
    assert line == S.plan_line(c, t, counters), (line, S.plan_line(c, t, counters))
    assert ws >= c["B"] * S.expected(c, t, counters)[2] * c["C"] * 8


def test_cases_cover_the_classes():
    """Every form of the launcher, each type with and without counters, and distinct names."""
    names = [c["name"] for c in S.CASES]
    assert len(set(names)) == len(names)
    for t in S.T3:
        got = {S.expected(c, t, k)[::3] for c in S.CASES if t in c["types"] for k in (True, False)}
        want = {("partial", "self"), ("partial", "final_kernel"), ("partial", "fused"), ("partial_up", "final_kernel"),
                ("partial_up", "fused")} | ({("up_quad", "final_kernel"), ("up_quad", "fused")} if t != "f32" else set())
        assert got == want, (t, got ^ want)
    assert {S.expected(c, "bf16", True)[2] for c in S.CASES} >= {1, 2, 3, 16, 20}


def test_counter_boundary(lib):
    """One counter per (sample, 64-channel group): B * ceil(C / 64) words fuse, one fewer runs the final kernel."""
    for B, Cc in ((3, 80), (1, 64), (2, 1024), (5, 16)):
        need = B * ((Cc + 63) // 64)
        assert fields(plan(lib, "bf16", B, 16, 16, Cc, nsem=need)[0])["end"] == "fused", (B, Cc)
        assert fields(plan(lib, "bf16", B, 16, 16, Cc, nsem=need - 1)[0])["end"] == "final_kernel", (B, Cc)
    # one chunk finishes itself with or without counters; the closed form has no such ending
    assert fields(plan(lib, "f32", 2, 5, 5, 32, nsem=S.NSEM)[0])["end"] == "self"
    assert plan(lib, "bf16", 1, 32, 16, 64, up=1)[0] == "in_stats t=bf16 kernel=up_quad chunk=512 nchunk=1 end=final_kernel"
    assert plan(lib, "bf16", 1, 32, 16, 64, up=1, nsem=1)[0] == "in_stats t=bf16 kernel=up_quad chunk=512 nchunk=1 end=fused"


def test_plan_invariants(lib):
    """Over a sweep of shapes: the chunks cover the pixels, the halving rule never leaves more than 16 chunks, the
    closed form's records are whole workgroups of 512 source pixels, and the workspace covers the records."""
    n = 0
    for t in S.T3:
        for B in (1, 2, 3, 7, 64):
            for Cc in (16, 32, 64, 80, 128, 1024):
                for H, W, up in ((1, 1, 0), (2, 2, 0), (5, 5, 0), (16, 16, 0), (9, 13, 0), (64, 64, 0), (128, 160, 0),
                                 (256, 256, 0), (1031, 1, 0), (4100, 5, 0), (7, 5, 1), (32, 16, 1), (8, 128, 1),
                                 (4, 256, 1), (64, 64, 1), (128, 128, 1), (6, 16, 1)):
                    for nsem in (0, S.NSEM):
                        line, ws = plan(lib, t, B, H, W, Cc, up=up, nsem=nsem)
                        f = fields(line)
                        chunk, nchunk, HW = int(f["chunk"]), int(f["nchunk"]), H * W * (4 if up else 1)
                        if f["kernel"] == "up_quad":
                            assert up and t != "f32" and Cc % 64 == 0 and chunk == 512 and nchunk * 512 == H * W, line
                            assert f["end"] == ("fused" if nsem else "final_kernel"), line
                        else:
                            assert f["kernel"] == ("partial_up" if up else "partial"), line
                            assert nchunk * chunk >= HW > (nchunk - 1) * chunk and 1 <= chunk <= 1024, (line, HW)
                            if chunk < min(HW, 1024):           # the halving rule fired
                                assert nchunk <= 16, (line, HW)
                            assert f["end"] == ("self" if nchunk == 1 else "fused" if nsem else "final_kernel"), line
                        assert ws >= B * nchunk * Cc * 8, (line, ws)
                        n += 1
    assert n == 3 * 5 * 6 * 17 * 2


def test_plan_rejects_what_the_launcher_rejects(lib):
    assert plan(lib, "bf16", 2, 8, 8, 24)[0] is None                # C % 16
    assert plan(lib, "bf16", 2, 8, 8, 64, ldx=68)[0] is None        # ldx % 8
    assert plan(lib, "bf16", 0, 8, 8, 64)[0] is None and plan(lib, "bf16", 2, 0, 8, 64)[0] is None
    buf = C.create_string_buffer(64)
    assert lib.ghost_instnorm_plan(_lib.U8, 2, 8, 8, 64, 64, 0, 0, None, buf, 64) == EINVAL      # no such type
    assert lib.ghost_instnorm_plan(_lib.BF16, 2, 8, 8, 64, 64, 2, 0, None, buf, 64) == EINVAL    # up2x is 0 or 1
    assert lib.ghost_instnorm_plan(_lib.BF16, 2, 8, 8, 64, 64, 0, -1, None, buf, 64) == EINVAL
    assert lib.ghost_instnorm_plan(_lib.BF16, 2, 8, 8, 64, 64, 0, 0, None, None, 64) == EINVAL
    # the size query
    assert lib.ghost_instnorm_plan(_lib.BF16, 2, 8, 8, 64, 64, 0, 0, None, None, 0) == \
        len("in_stats t=bf16 kernel=partial chunk=64 nchunk=1 end=self") + 1


def test_stats_entry_rejects_bad_arguments_without_launching(lib):
    """ghost_instnorm_stats_rt_nhwc refuses before any launch (host memory stands for every pointer: a launch would
    fail otherwise, there is no device here)."""
    mem = (C.c_char * 4096)()
    a = C.addressof(mem)
    a += -a % 16

    def call(dt=_lib.BF16, x=a, B=2, H=8, W=8, Cc=64, ldx=64, up=0, stat=a, ws=a, ws_bytes=1 << 20, sem=None, nsem=0):
        return lib.ghost_instnorm_stats_rt_nhwc(dt, x, B, H, W, Cc, ldx, up, stat, ws, ws_bytes, sem, nsem, None)
    assert call(x=None) == EINVAL and call(stat=None) == EINVAL and call(up=2) == EINVAL and call(ws_bytes=-1) == EINVAL
    assert call(sem=None, nsem=4) == EINVAL and call(sem=a, nsem=0) == EINVAL and call(sem=a, nsem=-1) == EINVAL
    assert call(Cc=24, ldx=24) == EINVAL and call(ldx=68) == EINVAL and call(x=a + 8) == EINVAL and call(dt=_lib.U8) == EINVAL
    assert call(ws=None) == ENOWS and call(ws_bytes=64) == ENOWS
    assert b"workspace" in lib.ghost_last_error()
