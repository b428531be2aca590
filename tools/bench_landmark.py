"""Timings of the 106-point landmark network (ghost_amd.landmarks) on the MI355X.

    python tools/bench_landmark.py [--batch 64] [--calls 20] [--launches 50] [--repeats 5] [--out profiles/landmark_ab.txt]

1. Landmark106.landmarks_u8 (warp + network + transform) at N = batch for fp32, fp16 and bf16 storage: device events
   around `calls` back-to-back calls after a warm-up, one figure per repeat; per-call time, faces/s, the spread
   (range of the repeats) and the launches the plan log records for one call.
2. For each conv_k (k = 2 .. 14) at the network's shape, fp32 and fp16: A/B of the fused ghost_dwsep_block_nhwc
   against the unfused form (its depthwise-only launch + ghost_conv2d_ex_nhwc 1x1 with the prelu epilogue), both in
   one process, alternated, device events around `launches` back-to-back calls; outputs compared first.  The spread
   is the larger range of the two forms' repeats; a form wins where the medians differ by more than that.
3. VGPRs, scratch and static LDS of the kernels of csrc/lmk.hip as hipcc reports them (when hipcc is present); the
   fused block's LDS image is dynamic: BM x (rup(Cin, 32) + 16 bytes) rows, BM = 32 (16-bit) or 16 (fp32).
Weights are the key-hashed test recipe; inputs are seeded.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import re
import subprocess
import sys

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
    return (f"{name:<30s} us/call: median {np.median(ts):9.2f}  min {min(ts):9.2f}  max {max(ts):9.2f}  "
            f"spread {max(ts) - min(ts):7.2f}{extra}")


def resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(REPO, "ghost_amd", "csrc", "lmk.hip")
    if not os.path.exists(hipcc):
        return ["(hipcc not found: no resource figures)"]
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.dirname(src),
           "-I" + os.path.join(REPO, "include"), "--cuda-device-only", "-c", src, "-o", os.devnull,
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    rows, cur = [], {}
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            rows.append(cur)
        else:
            cur[m.group(1).split()[0]] = m.group(2)
    out = []
    for row in rows:
        # the mangled name's kernel and storage type (c++filt does not know DF16b)
        m = re.search(r"\d+([a-z_]+_kernel)(I(f|DF16b|DF16_))?", row["name"])
        name = row["name"] if not m else m.group(1) + (
            "<" + {"f": "float", "DF16b": "bf16", "DF16_": "f16"}[m.group(3)] + ">" if m.group(3) else "")
        out.append(f"  {name:<44s} VGPRs {row.get('VGPRs', '?'):>4s}  scratch {row.get('ScratchSize', '?'):>2s} B/lane  "
                   f"static LDS {row.get('LDS', '?'):>5s} B")
    return out or ["(hipcc printed no resource remarks)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "landmark_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_landmark: no GPU (timings are taken on the MI355X only)")
    import landmark_ref
    from ghost_amd.landmarks import Landmark106, pack
    lib = _lib.load()
    N = a.batch
    rep = [f"2d106det landmark network on {torch.cuda.get_device_name(0)}: N={N}; whole call {a.calls} calls x {a.repeats} "
           f"repeats, kernels {a.launches} launches x {a.repeats} repeats (device events)"]
    w = landmark_ref.make_weights()
    crops = landmark_ref.make_input(N, 224).to(DEV)

    # ---- 1. the whole call
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        net = Landmark106(compute_dtype=dt)
        net.load_state_dict(w)
        net = net.to(DEV)
        for _ in range(3):
            net.landmarks_u8(crops)
        torch.cuda.synchronize()
        _lib.plan_log(True)
        net.landmarks_u8(crops)
        torch.cuda.synchronize()
        _lib.plan_log(False)
        sigs = _lib.plan_log_read()
        ts = timed(lambda: net.landmarks_u8(crops), a.calls, a.repeats)
        med = float(np.median(ts))
        rep.append(line(f"landmarks_u8 {TN[dt]} N={N}", ts, f"  {N / med * 1e6:9.0f} faces/s  plan-log launches {len(sigs)}"))
        if dt == torch.float32:
            rep += [f"    {s}" for s in sigs]
        del net
        torch.cuda.empty_cache()

    # ---- 2. fused block against depthwise-only + 1x1 conv, per layer
    st = torch.cuda.current_stream(DEV).cuda_stream
    ws = torch.empty(256 << 20, dtype=torch.uint8, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(5)
    wins = {}
    for dt in (torch.float32, torch.float16):
        gd = _lib.gdtype(dt)
        slots = {k: v.to(DEV) for k, v in pack.pack_landmark(w, dt).items()}
        rep.append(f"A/B per layer, {TN[dt]} storage, N={N} (us/call medians; d = unfused - fused)")
        for k, ci, co, s, hin in pack.DWSEP:
            ho = hin // s
            x = (torch.randn(N, hin, hin, ci, device=DEV, generator=gen) * 1.2).to(dt)
            yf = torch.empty(N, ho, ho, co, dtype=dt, device=DEV)
            yu = torch.empty_like(yf)
            d = torch.empty(N, ho, ho, ci, dtype=dt, device=DEV)
            P = lambda n: slots[f"c{k}.{n}"].data_ptr()
            epi = _lib.ConvEpi(scale=P("pw.scale"), shift=P("pw.shift"), slope=1.0, prelu=P("pw.prelu"))
            npad, kpad = slots[f"c{k}.pw.w"].shape

            def block(cout, y):
                _lib.check(lib.ghost_dwsep_block_nhwc(gd, x.data_ptr(), N, hin, hin, ci, ci, s, P("dw.w"), P("dw.scale"),
                                                      P("dw.shift"), P("dw.prelu"), P("pw.w") if cout else None, cout,
                                                      kpad if cout else 0, P("pw.scale") if cout else None,
                                                      P("pw.shift") if cout else None, P("pw.prelu") if cout else None,
                                                      y.data_ptr(), cout or ci, None, 0, st), "dwsep")

            def fused():
                block(co, yf)

            def unfused():
                block(0, d)
                _lib.check(lib.ghost_conv2d_ex_nhwc(gd, d.data_ptr(), N, ho, ho, ci, ci, P("pw.w"), co, npad, kpad, 1, 1,
                                                    1, 0, C.byref(epi), yu.data_ptr(), co, ws.data_ptr(), ws.numel(),
                                                    st), "conv 1x1")
            fused()
            try:
                unfused()
            except RuntimeError as e:
                torch.cuda.synchronize()
                ts = timed(fused, a.launches, a.repeats)
                rep.append(line(f"  conv_{k} {ci}->{co} s{s} @{hin} fused", ts, f"  unfused form refused: {e}"))
                wins[(dt, k)] = "fused (no unfused form)"
                continue
            torch.cuda.synchronize()
            diff = float((yf.float() - yu.float()).abs().max())
            tf, tu = [], []
            for _ in range(a.repeats):                # alternated
                tf += timed(fused, a.launches, 1)
                tu += timed(unfused, a.launches, 1)
            dd, sp = float(np.median(tu) - np.median(tf)), max(max(tf) - min(tf), max(tu) - min(tu))
            verdict = "fused" if dd > sp else "unfused" if -dd > sp else "within the spread"
            wins[(dt, k)] = verdict
            rep.append(f"  conv_{k:<2d} {ci:>3d}->{co:<3d} s{s} @{hin:<2d} fused {np.median(tf):8.2f} [{min(tf):.2f}, {max(tf):.2f}]  "
                       f"unfused {np.median(tu):8.2f} [{min(tu):.2f}, {max(tu):.2f}]  d {dd:8.2f}  spread {sp:6.2f}  "
                       f"max|dy| {diff:.2e}  -> {verdict}")
        rep.append(f"  {TN[dt]}: fused wins by more than the spread at conv_k, k in "
                   f"{[k for (t, k), v in wins.items() if t == dt and v.startswith('fused')]}; unfused at "
                   f"{[k for (t, k), v in wins.items() if t == dt and v == 'unfused']}")

    # ---- 3. resources
    rep.append("kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):")
    rep += resources()
    text = "\n".join(rep) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
