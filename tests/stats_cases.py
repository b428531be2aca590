"""Cases of the InstanceNorm statistics launcher (ops.hip in_stats_plan / in_stats_launch), shared by the GPU op tests
(tests/test_fused_reduce_ops.py, through ghost_instnorm_stats_rt_nhwc) and the CPU plan tests
(tests/test_stats_plan_cpu.py, the same tokens from ghost_instnorm_plan).

The launcher chooses among five forms by shape: one chunk whose workgroup finishes the statistics itself (end=self),
partial records + in_stats_final_kernel (end=final_kernel), partial records merged by the last arriver (end=fused,
only with arrival counters, one per (sample, 64-channel group)), and for the statistics of a virtual x2 upsample the
closed form over the source (kernel=up_quad, 16-bit types) with either ending or the per-pixel kernel
(kernel=partial_up).  Each case is the smallest shape of its class, found by asking ghost_instnorm_plan.  If a retuned
heuristic moves a case, change the shape, not the class.
"""
NSEM = 4096             # the runtime's counter words (aei_runtime.hip kSemWords)
T3 = ("bf16", "f16", "f32")
T16 = ("bf16", "f16")


def _st(name, B, H, W, C, plan16, plan32=None, ldx=None, up=0, nsem=NSEM, fused=True, types=T3):
    """plan16 / plan32: (kernel, chunk, nchunk) of the 16-bit types and of fp32 (None: the same).  fused: what the
    case's counters give (a plan of one chunk ends in "self" either way); without counters the ending is
    "final_kernel".  ldx > C: x is a 16-byte aligned channel slice of a wider buffer."""
    return dict(name=name, B=B, H=H, W=W, C=C, ldx=C if ldx is None else ldx, up=up, nsem=nsem, fused=fused,
                plan16=plan16, plan32=plan32 or plan16, types=tuple(types))


CASES = [
    # one chunk; C % 64 != 0: the threads of the last channel group beyond C load nothing (cok), its merge stops at C
    _st("self-C32", 2, 5, 5, 32, ("partial", 25, 1)),
    _st("self-C80", 2, 5, 5, 80, ("partial", 25, 1)),
    # HW = 2 * 512 + 7: a last chunk of 7 pixels, fewer than one pass of the workgroup (88 groups x 3 chunks stop the
    # halving at 512)
    _st("tail7", 22, 1031, 1, 256, ("partial", 512, 3)),
    # exactly 16 chunks: one full batch of the fix-up's clamped loads; 20: a second batch, clamped from its 5th load
    _st("chunks16", 1, 64, 64, 64, ("partial", 256, 16)),
    _st("chunks20", 1, 128, 160, 80, ("partial", 1024, 20)),
    # 3 samples x 2 channel groups: 6 counters fuse, 5 fall back to the final kernel
    _st("groups6-nsem6", 3, 16, 16, 80, ("partial", 64, 4), nsem=6),
    _st("groups6-nsem5", 3, 16, 16, 80, ("partial", 64, 4), nsem=5, fused=False),
    # a channel slice (channels 16 .. 79 of 96) of a buffer whose other channels hold finite junk
    _st("slice", 2, 9, 13, 64, ("partial", 58, 3), ldx=96),
    # the statistics of the x2 upsample: the closed form over the source with 1 record and with 2 records in each of
    # its three workgroup shapes (32 x 16, 4 x 128, 4 x 128 of a 256-wide row); fp32 walks the upsampled pixels
    _st("up-1rec", 2, 32, 16, 64, ("up_quad", 512, 1), ("partial_up", 128, 16), up=1),
    _st("up-64x16", 2, 64, 16, 64, ("up_quad", 512, 2), ("partial_up", 256, 16), up=1),
    _st("up-8x128", 2, 8, 128, 64, ("up_quad", 512, 2), ("partial_up", 256, 16), up=1),
    _st("up-4x256", 2, 4, 256, 64, ("up_quad", 512, 2), ("partial_up", 256, 16), up=1),
    # the per-pixel kernel, fused: W % 16 != 0 keeps the 16-bit types off the closed form
    _st("up-pix-7x5", 2, 7, 5, 80, ("partial_up", 35, 4), up=1),
    _st("up-pix-8x16", 2, 8, 16, 64, ("partial_up", 64, 8), up=1, types=("f32",)),
]


def case_id(c, t, counters):
    return f"{c['name']}-{t}-{'sem' if counters else 'nosem'}"


def expected(c, t, counters):
    """(kernel, chunk, nchunk, end) of the case for storage type name ``t``, with its counters or without any."""
    kernel, chunk, nchunk = c["plan32"] if t == "f32" else c["plan16"]
    end = "self" if nchunk == 1 and kernel != "up_quad" else "fused" if counters and c["fused"] else "final_kernel"
    return kernel, chunk, nchunk, end


def plan_line(c, t, counters):
    kernel, chunk, nchunk, end = expected(c, t, counters)
    return f"in_stats t={t} kernel={kernel} chunk={chunk} nchunk={nchunk} end={end}"
