"""What the ArcFace, landmark and detector runtimes share on the host (plan_ctx.h: the handle base, the dry-run sizing
and the run bracket), on every path that reaches no device.

The workspace sizes are pinned to the values the three separate runtimes gave before they were folded into the shared
code (re-read from a build of that commit).  They are not proportional to N, because the scratch term follows the
split-K plan, so a changed allocation order or a dropped region shows.  A forward call with every slot bound to a dummy
aligned address and no workspace stops at the workspace check, before the first device call; its message must name
exactly the pinned size.
"""
import ctypes as C

import pytest

from ghost_amd import _lib

F32, BF16, F16 = _lib.F32, _lib.BF16, _lib.F16
EINVAL, ENOTREADY, ENOWS = -1, -2, -3
R100, R1 = (3, 13, 30, 3), (1, 1, 1, 1)

ARC_N = (1, 2, 3, 8, 33)
ARC_F32 = (24285696, 48570880, 72856064, 162169344, 609337856)
ARC_BF16 = (15354368, 25088512, 37632512, 85901824, 311292416)
ARC_BYTES = {(F32, R100): ARC_F32, (F32, R1): ARC_F32, (BF16, R100): ARC_BF16,
             (BF16, R1): ARC_BF16[:3] + (84296192,) + ARC_BF16[4:]}

LMK_N = (0, 1, 2, 3, 8, 33)
LMK_16 = (256, 1627392, 3254016, 4880640, 13014016, 53680896)
LMK_BYTES = {F32: (256, 3101952, 6203136, 9304320, 24810496, 102341376), BF16: LMK_16, F16: LMK_16}

DET_N = (0, 1, 2, 3, 8)
DET_SMALL_16 = (256, 1073920, 2145280, 3217408, 8574720)
DET_BIG_16 = (256, 50960384, 88812800, 131990272, 348696064)
DET_BYTES = {((96, 64), F32): (256, 1652992, 3303936, 4955136, 13210368),
             ((96, 64), BF16): DET_SMALL_16, ((96, 64), F16): DET_SMALL_16,
             ((640, 640), F32): (256, 89590784, 166073600, 247881472, 657739264),
             ((640, 640), BF16): DET_BIG_16, ((640, 640), F16): DET_BIG_16}
# ghost_det_forward_u8 at 96 x 64, N = 1 and 3: below the detect size, since the nine maps are the caller's and there
# is no decode workspace
DET_FORWARD_NEED = {F32: {1: 1374976, 3: 4122368}, BF16: {1: 795904, 3: 2384640}, F16: {1: 795904, 3: 2384640}}

DUMMY = 0x10000          # never dereferenced: every call below returns before the first device call
STEM = {"arc": "stem.w", "lmk": "stem.w", "det": "backbone.stem.0.w"}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def last_error(lib):
    return lib.ghost_last_error().decode()


class Handle:
    """A native handle of one runtime (arc with layers (1,1,1,1) and det at 96 x 64 unless told otherwise)."""

    def __init__(self, lib, kind, dt, layers=R1, det_size=(96, 64)):
        self.lib, self.kind = lib, kind
        self.h = C.c_void_p()
        if kind == "arc":
            rc = lib.ghost_arc_create((C.c_int * 4)(*layers), 512, dt, C.byref(self.h))
        elif kind == "lmk":
            rc = lib.ghost_lmk_create(dt, C.byref(self.h))
        else:
            rc = lib.ghost_det_create(dt, det_size[0], det_size[1], C.byref(self.h))
        assert rc == 0, last_error(lib)

    def fn(self, name):
        return getattr(self.lib, f"ghost_{self.kind}_{name}")

    def bind_all(self, skip=None):
        """Bind every slot but ``skip`` to a dummy aligned address; the names come from asking which slot is unbound
        (the first in name order), on a handle of the same kind that is bound as it answers."""
        names = []
        probe = self if skip is None else Handle(self.lib, self.kind, F32)
        while probe.fn("missing")(probe.h):
            msg = last_error(self.lib)
            assert msg.startswith("unbound weight slot "), msg
            names.append(msg[len("unbound weight slot "):])
            assert probe.fn("bind")(probe.h, names[-1].encode(), DUMMY, 1) == 0, last_error(self.lib)
        if probe is not self:
            probe.close()
            for name in names:
                if name != skip:
                    assert self.fn("bind")(self.h, name.encode(), DUMMY, 1) == 0, last_error(self.lib)
        return self

    def bytes(self, N):
        return self.fn("workspace_bytes")(self.h, N)

    def pinned(self, dt, N):
        """The pinned workspace size of the default handle of this kind."""
        if self.kind == "arc":
            return ARC_BYTES[dt, R1][ARC_N.index(N)]
        return LMK_BYTES[dt][LMK_N.index(N)] if self.kind == "lmk" else DET_BYTES[(96, 64), dt][DET_N.index(N)]

    def forwards(self, N, h="own", ws=None, ws_bytes=0):
        """Every forward entry point of the runtime with valid arguments and the given workspace (none): (name, rc,
        last error)."""
        lib, p = self.lib, DUMMY
        h = self.h if h == "own" else h
        out = []

        def call(name, *args):
            rc = getattr(lib, name)(h, *args)
            out.append((name, rc, last_error(lib)))
        if self.kind == "arc":
            st = (C.c_int64 * 4)(3 * 112 * 112, 112 * 112, 112, 1)
            call("ghost_arc_forward", p, F32, st, N, p, ws, ws_bytes, None)
            call("ghost_arc_embed_u8", p, 224 * 224 * 3, N, 224, 224, p, ws, ws_bytes, None)
        elif self.kind == "lmk":
            call("ghost_lmk_forward", p, 192 * 192 * 3, 1, N, p, ws, ws_bytes, None)
            call("ghost_lmk_landmarks_u8", p, 224 * 224 * 3, N, p, p, ws, ws_bytes, None)
        else:
            maps = (C.c_void_p * 9)(*[p] * 9)
            call("ghost_det_forward_u8", p, 45 * 80 * 3, N, 45, 80, 54, 96, maps, ws, ws_bytes, None)
            call("ghost_det_detect_u8", p, 45 * 80 * 3, N, 45, 80, 54, 96, 1.2, 0.5, 0.4, 16, p, p, p, p, ws, ws_bytes, None)
        return out

    def close(self):
        self.fn("destroy")(self.h)


@pytest.fixture
def make(lib):
    made = []

    def _make(*args, **kw):
        made.append(Handle(lib, *args, **kw))
        return made[-1]
    yield _make
    for h in made:
        h.close()


KINDS = [("arc", F32), ("arc", BF16), ("lmk", F32), ("lmk", BF16), ("lmk", F16), ("det", F32), ("det", BF16),
         ("det", F16)]


@pytest.mark.parametrize("dt,layers", sorted(ARC_BYTES))
def test_arc_workspace_bytes(make, dt, layers):
    h = make("arc", dt, layers=layers)
    assert tuple(h.bytes(n) for n in ARC_N) == ARC_BYTES[dt, layers]
    assert tuple(h.bytes(n) for n in ARC_N) == ARC_BYTES[dt, layers]      # run to run
    assert h.bytes(0) == -1


@pytest.mark.parametrize("dt", sorted(LMK_BYTES))
def test_lmk_workspace_bytes(make, dt):
    h = make("lmk", dt)
    assert tuple(h.bytes(n) for n in LMK_N) == LMK_BYTES[dt]
    assert tuple(h.bytes(n) for n in LMK_N) == LMK_BYTES[dt]
    assert h.bytes(65536) == -1


@pytest.mark.parametrize("size,dt", sorted(DET_BYTES))
def test_det_workspace_bytes(make, size, dt):
    h = make("det", dt, det_size=size)
    assert tuple(h.bytes(n) for n in DET_N) == DET_BYTES[size, dt]
    assert tuple(h.bytes(n) for n in DET_N) == DET_BYTES[size, dt]        # the second round is the handle's memo
    assert h.bytes(4097) == -1


@pytest.mark.parametrize("kind,dt", KINDS)
def test_no_workspace_names_the_need(make, kind, dt):
    h = make(kind, dt).bind_all()
    assert h.fn("missing")(h.h) == 0
    for N in (1, 3):
        need = h.pinned(dt, N)
        for name, rc, msg in h.forwards(N):
            want = DET_FORWARD_NEED[dt][N] if name == "ghost_det_forward_u8" else need
            assert (rc, msg) == (ENOWS, f"workspace too small: need {want}"), name
        # a workspace one byte short is refused the same way (the pointer is not touched)
        for name, rc, msg in h.forwards(N, ws=DUMMY, ws_bytes=DET_FORWARD_NEED[dt][N] - 1 if kind == "det" else need - 1):
            assert rc == ENOWS and msg.startswith("workspace too small: need "), name
        assert h.bytes(N) == need


@pytest.mark.parametrize("kind,dt", KINDS)
def test_unbound_slot_is_named(make, kind, dt):
    h = make(kind, dt).bind_all(skip=STEM[kind])
    assert h.fn("missing")(h.h) == 1
    for name, rc, msg in h.forwards(2):
        assert (rc, msg) == (ENOTREADY, "unbound weight slot " + STEM[kind]), name
    assert h.bytes(2) > 256       # sizing needs no weights


@pytest.mark.parametrize("kind,dt", [("arc", F32), ("lmk", F16), ("det", BF16)])
def test_bad_arguments(make, kind, dt):
    h = make(kind, dt).bind_all()
    lo, hi = {"arc": (1, 65535), "lmk": (0, 65535), "det": (0, 4096)}[kind]
    for name, rc, msg in h.forwards(2, h=None):
        assert (rc, msg) == (EINVAL, "null handle"), name
    for name, rc, msg in h.forwards(hi + 1):
        assert (rc, msg) == (EINVAL, f"batch must be in {lo}..{hi}"), name
    for name, rc, msg in h.forwards(-1):
        assert (rc, msg) == (EINVAL, f"batch must be in {lo}..{hi}"), name
    for name, rc, msg in h.forwards(0):
        assert rc == (EINVAL if kind == "arc" else 0), name
    ptrs = (C.c_void_p * 4)(*[DUMMY] * 4)
    set_taps = h.fn("set_taps")
    assert set_taps(h.h, ptrs, 4) == 0 and set_taps(h.h, None, 0) == 0
    if kind == "arc":
        assert set_taps(h.h, ptrs, 3) == 0 and set_taps(h.h, None, 0) == 0       # any number
        assert set_taps(h.h, None, 2) == EINVAL and last_error(h.lib) == "bad argument"
    else:
        assert set_taps(h.h, ptrs, 3) == EINVAL and last_error(h.lib) == "bad argument (0 or 4 taps)"
        assert set_taps(h.h, None, 4) == EINVAL and last_error(h.lib) == "bad argument (0 or 4 taps)"
    assert set_taps(None, ptrs, 4) == EINVAL
    assert h.fn("bind")(h.h, b"no.such.slot", DUMMY, 1) == EINVAL
    assert last_error(h.lib) == "unknown weight slot no.such.slot"
    assert h.fn("bind")(h.h, STEM[kind].encode(), None, 1) == EINVAL
    assert last_error(h.lib) == "empty tensor for " + STEM[kind]
    # arc's bind does not ask for alignment; the other two do
    rc = h.fn("bind")(h.h, STEM[kind].encode(), DUMMY + 4, 1)
    assert rc == (0 if kind == "arc" else EINVAL)
    if kind != "arc":
        assert last_error(h.lib) == "slot not 16-byte aligned: " + STEM[kind]
    assert h.fn("bind")(None, STEM[kind].encode(), DUMMY, 1) == EINVAL and last_error(h.lib) == "null argument"
    assert h.fn("missing")(None) == EINVAL and last_error(h.lib) == "null handle"
