"""Timings of the use_sr face enhancer (ghost_amd.sr) on the MI355X.

    python tools/bench_sr.py [--batch 20] [--calls 10] [--repeats 5] [--out profiles/sr_ab.txt]

1. crops/s of LIPSPADEGenerator.forward at B = batch (face_enhancement's chunk), bf16 and fp32 storage, with the
   per-call power iteration (the default) and with frozen sigma; host clock around `calls` forwards that end in a
   device synchronise, after a warm-up of every shape.
2. the two kernels of csrc/sr.hip at their 256 x 256 shapes: device events around `launches` back-to-back calls;
   achieved bytes/s against the minimum bytes the pass must move (each input and output once), computed from the
   shapes below.
3. A/B of the nearest x2 upsample folded into ghost_norm_modulate_nhwc's read (up2x = 1) against a materialised
   upsample followed by the plain pass, both forms in one process, alternated; outputs compared bit for bit first.
   The spread is the range of a form's repeats.
Weights are the key-hashed test recipe; inputs are seeded.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from ghost_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
TN = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}


def timed(fn, launches, repeats):
    """us per call, one figure per repeat (device events around `launches` back-to-back calls)."""
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / launches)
    return out


def line(name, ts, extra=""):
    return (f"{name:<34s} us/call: median {np.median(ts):9.2f}  min {min(ts):9.2f}  max {max(ts):9.2f}  "
            f"spread {max(ts) - min(ts):7.2f}{extra}")


def modulate(lib, dt, src, stat, gb, out, up2x, slope=0.2):
    B, H, W, Cn = out.shape
    _lib.check(lib.ghost_norm_modulate_nhwc(_lib.gdtype(dt), src.data_ptr(), Cn, B, H, W, Cn, stat.data_ptr(),
                                            stat.shape[0], _lib.ptr(gb), 2 * Cn, slope, 1 if up2x else 0,
                                            out.data_ptr(), Cn, torch.cuda.current_stream(DEV).cuda_stream), "modulate")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sr_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sr: no GPU (timings are taken on the MI355X only)")
    import sr_ref
    from ghost_amd.sr import LIPSPADEGenerator
    from oracle import aei_ref
    lib = _lib.load()
    B = a.batch
    rep = [f"use_sr enhancer on {torch.cuda.get_device_name(0)}: B={B}, {a.calls} forwards x {a.repeats} repeats (host clock "
           f"to synchronise); kernels {a.launches} launches x {a.repeats} repeats (device events)"]

    # ---- 1. whole forward
    w = aei_ref.make_weights(sr_ref.param_specs())
    x = sr_ref.make_input(B, seed=11).to(DEV)
    for dt in (torch.bfloat16, torch.float32):
        for pi in (True, False):
            G = LIPSPADEGenerator(compute_dtype=dt, power_iteration=pi)
            G.load_state_dict(w)
            G = G.to(DEV)
            for _ in range(2):
                G(x)
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    G(x)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) / a.calls)
            med = float(np.median(ts))
            rep.append(f"forward {TN[dt]} power_iteration={int(pi)}: {med * 1e3:8.2f} ms/call  {B / med:8.1f} crops/s  "
                       f"(repeats ms: {' '.join(f'{t * 1e3:.2f}' for t in ts)})")
            del G
            torch.cuda.empty_cache()

    # ---- 2. the two kernels at their 256 x 256 shapes
    gen = torch.Generator(device=DEV).manual_seed(5)

    def rnd(*shape, dt):
        return torch.randn(*shape, device=DEV, generator=gen).to(dt)
    for dt in (torch.bfloat16, torch.float32):
        es = 2 if dt != torch.float32 else 4
        # SPADE modulate of ups.3.norm_1: C = 48 at 256 x 256, gamma / beta from one [.., 96] tensor
        Cn = 48
        src, gb = rnd(B, 256, 256, Cn, dt=dt), rnd(B, 256, 256, 2 * Cn, dt=dt)
        stat = torch.rand(1, Cn, 2, device=DEV, generator=gen) + 0.5
        out = torch.empty_like(src)
        ts = timed(lambda: modulate(lib, dt, src, stat, gb, out, False), a.launches, a.repeats)
        nbytes = B * 65536 * Cn * es * 4              # src + gamma + beta + out
        rep.append(line(f"norm_modulate {TN[dt]} C=48 gb", ts,
                        f"  min bytes {nbytes / 1e6:.1f} MB -> {nbytes / np.median(ts) / 1e6:.2f} TB/s"))
        # the encoder's InstanceNorm + ReLU at 256 x 256 (no gamma / beta)
        sti = torch.rand(B, Cn, 2, device=DEV, generator=gen) + 0.5
        ts = timed(lambda: modulate(lib, dt, src, sti, None, out, False, 0.0), a.launches, a.repeats)
        nbytes = B * 65536 * Cn * es * 2
        rep.append(line(f"norm_modulate {TN[dt]} C=48 instance", ts,
                        f"  min bytes {nbytes / 1e6:.1f} MB -> {nbytes / np.median(ts) / 1e6:.2f} TB/s"))
        # LIP pooling of the first encoder stage: 256 x 256 x 48 -> 128 x 128 x 48
        lg = rnd(B, 256, 256, Cn, dt=dt)
        wv, bv = torch.rand(Cn, device=DEV, generator=gen) + 0.5, torch.randn(Cn, device=DEV, generator=gen) * 0.1
        po = torch.empty(B, 128, 128, Cn, dtype=dt, device=DEV)
        st = torch.cuda.current_stream(DEV).cuda_stream

        def pool():
            _lib.check(lib.ghost_lip_pool_nhwc(_lib.gdtype(dt), src.data_ptr(), Cn, lg.data_ptr(), Cn, B, 256, 256, Cn,
                                               sti.data_ptr(), wv.data_ptr(), bv.data_ptr(), po.data_ptr(), Cn, st),
                       "lip_pool")
        ts = timed(pool, a.launches, a.repeats)
        nbytes = B * 65536 * Cn * es * 2 + B * 16384 * Cn * es      # x + logit + out
        rep.append(line(f"lip_pool {TN[dt]} C=48 256->128", ts,
                        f"  min bytes {nbytes / 1e6:.1f} MB -> {nbytes / np.median(ts) / 1e6:.2f} TB/s"))

    # ---- 3. A/B: nearest x2 folded into the read against a materialised upsample + the plain pass
    for dt in (torch.bfloat16, torch.float32):
        for (hs, Cn, what) in ((128, 96, "ups.3 norm_0/norm_s 128->256 C=96"), (32, 384, "ups.1 32->64 C=384")):
            small = rnd(B, hs, hs, Cn, dt=dt)
            gb = rnd(B, 2 * hs, 2 * hs, 2 * Cn, dt=dt)
            stat = torch.rand(1, Cn, 2, device=DEV, generator=gen) + 0.5
            o = [torch.empty(B, 2 * hs, 2 * hs, Cn, dtype=dt, device=DEV) for _ in range(2)]

            def fold():
                modulate(lib, dt, small, stat, gb, o[0], True)

            def mat():
                big = small[:, :, None, :, None, :].expand(B, hs, 2, hs, 2, Cn).reshape(B, 2 * hs, 2 * hs, Cn)
                modulate(lib, dt, big, stat, gb, o[1], False)
            fold(), mat()
            torch.cuda.synchronize()
            same = torch.equal(o[0], o[1])
            tf, tm = [], []
            for _ in range(a.repeats):                # alternated
                tf += timed(fold, a.launches, 1)
                tm += timed(mat, a.launches, 1)
            rep.append(f"A/B {TN[dt]} {what}: outputs identical: {same}")
            rep.append(line("  up2x folded into the read", tf))
            rep.append(line("  materialised x2 + plain pass", tm))
            d, sp = float(np.median(tm) - np.median(tf)), max(max(tf) - min(tf), max(tm) - min(tm))
            rep.append(f"  materialised - folded (medians): {d:.2f} us; largest spread {sp:.2f} us; "
                       f"{'folded is faster by more than the spread' if d > sp else 'materialised is faster by more than the spread' if -d > sp else 'within the spread'}")
    text = "\n".join(rep) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
