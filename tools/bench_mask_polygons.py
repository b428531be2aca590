"""A/B of the mask step of one identity: ``identity_masks`` (landmarks to the host, parameters and convex hull there,
polygons back up) against ``identity_masks_device`` (ghost_mask_polygons_dev, no host copy), on the MI355X.

    python tools/bench_mask_polygons.py [--frames 64 900] [--calls 10] [--repeats 5] [--out profiles/mask_polygons_ab.txt]

Both paths run in one process, alternated repeat by repeat, after a warm-up.  The network is a stub whose
``landmarks_u8`` gathers face-like landmarks from a device table by a byte of each crop (one launch), and the swaps are
224 x 224 already, so what is timed is the mask step: index uploads, the gathers, parameters + hull, raster, erode,
blur, and the scatter into the [F,224,224] result.  ``present`` has three runs of present frames (about 5/6 of F).
Per repeat: wall clock around `calls` back-to-back calls and a final synchronise (both paths; the host path also waits
inside every call), and device events around the same calls (the time the stream was busy or waiting between the first
and the last launch).  Figures are per call; spread = max - min of the repeats.  The kernel's resources are hipcc's
report when hipcc is present.
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

DEV = torch.device("cuda:0")


class TableNet:
    def __init__(self):
        import mask_poly_cases as cases
        sets = [cases.landmarks(s, shift=(s % 5 - 2.0, 0.0), scale=1.0 + 0.02 * (s % 4)) for s in range(16)]
        self.table = torch.from_numpy(np.stack([sets[k % 16] for k in range(256)])).to(DEV)

    def landmarks_u8(self, crops):
        return self.table[crops[:, 0, 0, 0].long()]


def present_three_runs(F):
    p = np.ones(F, bool)
    a, b = F // 3, 2 * F // 3
    p[:F // 24] = False
    p[a:a + F // 16] = False
    p[b:b + F // 16] = False
    return p


def measure(fn, calls):
    """(wall us per call, device-event us per call) of `calls` back-to-back calls and a final synchronise."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return (t1 - t0) * 1e6 / calls, e0.elapsed_time(e1) * 1e3 / calls


def line(name, ts):
    return (f"  {name:<38s} us/call: median {np.median(ts):10.1f}  min {min(ts):10.1f}  max {max(ts):10.1f}  "
            f"spread {max(ts) - min(ts):9.1f}")


def resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(REPO, "ghost_amd", "csrc", "mask_poly.hip")
    if not os.path.exists(hipcc):
        return ["  (hipcc not found: no resource figures)"]
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.dirname(src),
           "-I" + os.path.join(REPO, "include"), "--cuda-device-only", "-c", src, "-o", os.devnull,
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    keys = ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    got = {}
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:.*?\s{2,}([A-Za-z][^:]*): (\S+)", ln)
        if m and m.group(1) in keys:
            got[m.group(1)] = m.group(2)
    return ["  mask_poly_kernel  " + "  ".join(f"{k} {got[k]}" for k in keys if k in got)] if got else \
        ["  (hipcc printed no resource remarks)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[64, 900])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mask_polygons_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_polygons: no GPU (timings are taken on the MI355X only)")
    from ghost_amd.landmarks import identity_masks, identity_masks_device
    net = TableNet()
    rep = [f"mask step of one identity on {torch.cuda.get_device_name(0)}: identity_masks (host parameters + hull) against "
           f"identity_masks_device; stub network, 224 x 224 swaps, three runs of present frames; {a.calls} calls x "
           f"{a.repeats} repeats, alternated"]
    g = np.random.Generator(np.random.PCG64(3))
    for F in a.frames:
        present = present_three_runs(F)
        fill = torch.from_numpy(g.integers(0, 256, (2, F), dtype=np.uint8)).to(DEV)
        swaps = torch.zeros(F, 224, 224, 3, dtype=torch.uint8, device=DEV) + fill[0].view(F, 1, 1, 1)
        crops = torch.zeros(F, 224, 224, 3, dtype=torch.uint8, device=DEV) + fill[1].view(F, 1, 1, 1)
        host = lambda: identity_masks(net, swaps, crops, present)
        dev = lambda: identity_masks_device(net, swaps, crops, present)
        m0, _, lm0, p0 = host()
        m1, _, lm1, p1 = dev()
        same = bool(torch.equal(m0, m1)) and np.array_equal(lm1.cpu().numpy(), lm0) and \
            np.array_equal(p1.cpu().numpy(), p0)
        del m0, m1
        for _ in range(2):
            host()
            dev()
        wh, eh, wd, ed = [], [], [], []
        for _ in range(a.repeats):
            w, e = measure(host, a.calls)
            wh.append(w)
            eh.append(e)
            w, e = measure(dev, a.calls)
            wd.append(w)
            ed.append(e)
        rep.append(f"F = {F} ({int(present.sum())} present frames); outputs {'identical' if same else 'DIFFER'}")
        rep += [line("identity_masks         wall", wh), line("identity_masks_device  wall", wd),
                line("identity_masks         device events", eh), line("identity_masks_device  device events", ed)]
        d, sp = float(np.median(wh) - np.median(wd)), max(max(wh) - min(wh), max(wd) - min(wd))
        verdict = "device path faster" if d > sp else "device path slower" if -d > sp else "within the spread"
        rep.append(f"  wall: host - device = {d:.1f} us, larger spread {sp:.1f} us -> {verdict}")
        del swaps, crops
        torch.cuda.empty_cache()
    rep.append("kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):")
    rep += resources()
    text = "\n".join(rep) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
