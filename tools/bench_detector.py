"""Timings of the SCRFD face detector (ghost_amd.detection) on the MI355X.

    python tools/bench_detector.py [--frames 16] [--size 640] [--calls 10] [--launches 50] [--repeats 5]
                                   [--out profiles/detector.txt]

1. SCRFD.detect_frames (letterbox + network + decode + NMS) and SCRFD.forward (without the post-processing) on F
   frames of size x size for fp32, fp16 and bf16 storage: device events around `calls` back-to-back calls after a warm-up, one figure per
   repeat; per-call time, frames/s, the spread (range of the repeats), the workspace and the launches of one call.
   detect_frames is timed at a threshold that leaves about 300 candidates per frame and at one that puts every frame
   over the capacity of 4096 (seeded noise frames suppress nothing: the worst case of the greedy pass).
2. Channel padding, one layer: the 56 -> 56 3x3 conv at 160 x 160, N = 8, as the network runs it (Cin = 56, the
   implicit GEMM's scalar gather) against activations and packed weights padded to 64 channels (its fast gather), both
   in one process, alternated; fp32 and bf16.  And the head's three output convs (80 -> 2, 8, 20) through the implicit
   GEMM against the merged fp32 kernel the network runs (ghost_det_head_nhwc) at 80 x 80, N = 8, fp32.  A form wins
   where the medians differ by more than the spread.
3. VGPRs, scratch and static LDS of the kernels of csrc/det.hip as hipcc reports them (when hipcc is present).
There is no pass / fail on these times: there is nothing earlier to compare with, so they are recorded, not gated.
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
from ghost_amd.network.pack import pack_conv  # noqa: E402

DEV = torch.device("cuda:0")
TN = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}


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
    return (f"{name:<34s} us/call: median {np.median(ts):10.2f}  min {min(ts):10.2f}  max {max(ts):10.2f}  "
            f"spread {max(ts) - min(ts):8.2f}{extra}")


def resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(REPO, "ghost_amd", "csrc", "det.hip")
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
        m = re.search(r"\d+([a-z_]+_kernel)(I(f|DF16b|DF16_))?", row["name"])
        name = row["name"] if not m else m.group(1) + (
            "<" + {"f": "float", "DF16b": "bf16", "DF16_": "f16"}[m.group(3)] + ">" if m.group(3) else "")
        out.append(f"  {name:<32s} VGPRs {row.get('VGPRs', '?'):>4s}  scratch {row.get('ScratchSize', '?'):>2s} B/lane  "
                   f"static LDS {row.get('LDS', '?'):>5s} B")
    return out or ["(hipcc printed no resource remarks)"]


def ab(rep, name, fa, fb, na, nb, launches, repeats):
    ta, tb = [], []
    for _ in range(repeats):                # alternated
        ta += timed(fa, launches, 1)
        tb += timed(fb, launches, 1)
    d, sp = float(np.median(ta) - np.median(tb)), max(max(ta) - min(ta), max(tb) - min(tb))
    verdict = nb if d > sp else na if -d > sp else "within the spread"
    rep.append(f"  {name:<34s} {na} {np.median(ta):8.2f} [{min(ta):.2f}, {max(ta):.2f}]  {nb} {np.median(tb):8.2f} "
               f"[{min(tb):.2f}, {max(tb):.2f}]  d {d:8.2f}  spread {sp:6.2f}  -> {verdict}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "detector.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detector: no GPU (timings are taken on the MI355X only)")
    import detector_ref
    from ghost_amd.detection import SCRFD
    lib = _lib.load()
    F_, S = a.frames, a.size
    rep = [f"scrfd_10g_bnkps detector on {torch.cuda.get_device_name(0)}: F={F_} frames of {S}x{S}, det_size (640, 640); "
           f"whole call {a.calls} calls x {a.repeats} repeats, kernels {a.launches} launches x {a.repeats} repeats "
           f"(device events)"]
    w = detector_ref.make_weights()
    g = torch.Generator().manual_seed(3)
    frames = torch.randint(0, 256, (F_, S, S, 3), dtype=torch.uint8, generator=g).to(DEV)

    # ---- 1. the whole call
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        net = SCRFD(compute_dtype=dt)
        net.load_arrays(w)
        net = net.to(DEV)
        # two thresholds from the scores themselves: about 300 candidates per frame (a crowded frame), and one that
        # puts every frame over the capacity of 4096 with nothing suppressed (noise frames: the greedy pass's worst case)
        maps = net.forward(frames[:1])
        sc = torch.cat([m.flatten() for m in maps[:3]])
        typical = float(torch.topk(sc, 300).values[-1])
        over = float(torch.topk(sc, 5000).values[-1])
        _lib.plan_log(True)
        net.detect_frames(frames[:net.chunk_frames()], typical)
        torch.cuda.synchronize()
        _lib.plan_log(False)
        sigs = _lib.plan_log_read()
        rt = net._runtime(DEV)
        wsb = lib.ghost_det_workspace_bytes(rt.h, min(F_, net.chunk_frames()))
        nch = min(F_, net.chunk_frames())
        for name, n, fn in ((f"detect_frames ~300 cand.", F_, lambda: net.detect_frames(frames, typical)),
                            (f"detect_frames > capacity", F_, lambda: net.detect_frames(frames, over)),
                            ("forward (one chunk)", nch, lambda: net.forward(frames[:nch]))):
            out = fn()
            torch.cuda.synchronize()
            ts = timed(fn, a.calls, a.repeats)
            med = float(np.median(ts))
            extra = f"  {n / med * 1e6:8.0f} frames/s"
            if name.startswith("detect"):
                cnt = out[2].cpu().numpy()
                extra += (f"  candidates {int(cnt[:, 1].min())}..{int(cnt[:, 1].max())} kept {int(cnt[:, 0].min())}.."
                          f"{int(cnt[:, 0].max())}")
            rep.append(line(f"{name} {TN[dt]} F={n}", ts, extra))
        rep.append(f"    chunk {net.chunk_frames()} frames, workspace {wsb / 2 ** 20:.0f} MiB, plan-log launches per chunk "
                   f"{len(sigs)}")
        if dt == torch.float32:
            seen = []
            for s in sigs:
                if s not in seen:
                    seen.append(s)
            rep += [f"    {sigs.count(s):3d} x {s}" for s in seen]
        del net
        torch.cuda.empty_cache()

    # ---- 2. A/B: channel padding of one layer, and the merged head conv
    st = torch.cuda.current_stream(DEV).cuda_stream
    ws = torch.empty(256 << 20, dtype=torch.uint8, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(5)
    rep.append("A/B (us/call medians, alternated; d = first - second)")

    def conv_fn(dt, x, wt, cin, cout, y, H, W, N):
        wp = pack_conv(wt.to(DEV), dt)
        bias = torch.zeros(wp.shape[0], device=DEV)
        epi = _lib.ConvEpi(scale=None, shift=bias.data_ptr(), slope=0.0)
        keep = (wp, bias, epi)

        def fn(_keep=keep):
            _lib.check(lib.ghost_conv2d_ex_nhwc(_lib.gdtype(dt), x.data_ptr(), N, H, W, cin, cin, wp.data_ptr(), cout,
                                                wp.shape[0], wp.shape[1], 3, 3, 1, 1, C.byref(epi), y.data_ptr(), cout,
                                                ws.data_ptr(), ws.numel(), st), "conv")
        return fn

    N, H = 8, 160
    w56 = w["backbone.layer1.1.conv1.weight"]
    w64 = torch.zeros(64, 64, 3, 3)
    w64[:56, :56] = w56
    for dt in (torch.float32, torch.bfloat16):
        x56 = torch.randn(N, H, H, 56, device=DEV, generator=gen).to(dt)
        x64 = torch.zeros(N, H, H, 64, dtype=dt, device=DEV)
        x64[..., :56] = x56
        y56 = torch.empty(N, H, H, 56, dtype=dt, device=DEV)
        y64 = torch.empty(N, H, H, 64, dtype=dt, device=DEV)
        f56, f64 = conv_fn(dt, x56, w56, 56, 56, y56, H, H, N), conv_fn(dt, x64, w64, 64, 64, y64, H, H, N)
        f56(); f64()
        torch.cuda.synchronize()
        diff = float((y56.float() - y64[..., :56].float()).abs().max())
        ab(rep, f"3x3 56->56 @160 N=8 {TN[dt]} (max|dy| {diff:.1e})", f56, f64, "unpadded", "padded-64", a.launches,
           a.repeats)
    H = 80
    x80 = torch.randn(N, H, H, 80, device=DEV, generator=gen)
    parts = [w[f"bbox_head.stride_{k}.8.weight"] for k in ("cls", "reg", "kps")]
    ys = [torch.empty(N, H, H, p.shape[0], device=DEV) for p in parts]
    fns = [conv_fn(torch.float32, x80, p, 80, p.shape[0], y, H, H, N) for p, y in zip(parts, ys)]
    from ghost_amd.detection import pack
    hs = {k: v.to(DEV) for k, v in pack.pack_detector(w, torch.float32).items() if k.startswith("bbox_head.out.8")}

    def merged():
        _lib.check(lib.ghost_det_head_nhwc(_lib.gdtype(torch.float32), x80.data_ptr(), N, H, H,
                                           hs["bbox_head.out.8.w"].data_ptr(), hs["bbox_head.out.8.b"].data_ptr(),
                                           hs["bbox_head.out.8.m"].data_ptr(), ys[0].data_ptr(), ys[1].data_ptr(),
                                           ys[2].data_ptr(), st), "head")
    ab(rep, "head 80->2,8,20 @80 N=8 fp32", lambda: [f() for f in fns], merged, "three convs", "det_head", a.launches,
       a.repeats)

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
