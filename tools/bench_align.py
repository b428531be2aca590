"""A/B of the two ways to make the 224 crop and its 256 resize from device-resident frames.

    python tools/bench_align.py [--n 64] [--launches 200] [--repeats 7] [--out profiles/align_ab.txt]

fused:  one ghost_align_crops_u8 launch writes the crops and resizes them out of LDS;
split:  ghost_align_crops_u8 with resized = NULL, then ghost_resize_u8_linear of the crops it wrote.

N crops from 1920x1080 frames (seeded similarity transforms: scale 0.3-1.2, +-0.4 rad, centre inside the frame), both
forms in one process, alternated; each repeat times `launches` back-to-back calls with device events after a
warm-up, so the figures are enqueue-to-finish per call on an otherwise idle stream.  The outputs of the two forms are
compared byte for byte before timing.  The spread is the range of a form's repeats.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from ghost_amd import _lib  # noqa: E402
from ghost_amd.inference.blend import _invert_affine_cv  # noqa: E402

DEV = torch.device("cuda:0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "align_ab.txt"))
    a = ap.parse_args()
    N, F_, H, W, S, R = a.n, a.frames, 1080, 1920, 224, 256
    g = np.random.Generator(np.random.PCG64(1))
    gen = torch.Generator(device=DEV).manual_seed(1)
    frames = torch.randint(0, 256, (F_, H, W, 3), dtype=torch.uint8, device=DEV, generator=gen)
    maps = []
    for _ in range(N):
        sc, ang = g.uniform(0.3, 1.2), g.uniform(-0.4, 0.4)
        cx, cy = g.uniform(0.2 * W, 0.8 * W), g.uniform(0.2 * H, 0.8 * H)
        c, s = sc * np.cos(ang), sc * np.sin(ang)
        maps.append(_invert_affine_cv(np.array([[c, -s, S / 2 - (c * cx - s * cy)], [s, c, S / 2 - (s * cx + c * cy)]])))
    maps = torch.from_numpy(np.stack(maps).reshape(N, 6)).to(DEV)
    index = torch.from_numpy(g.integers(0, F_, size=N).astype(np.int32)).to(DEV)
    lib, st = _lib.load(), torch.cuda.current_stream(DEV).cuda_stream
    crops = [torch.zeros(N, S, S, 3, dtype=torch.uint8, device=DEV) for _ in range(2)]
    rz = [torch.zeros(N, R, R, 3, dtype=torch.uint8, device=DEV) for _ in range(2)]

    def align(k, fused):
        _lib.check(lib.ghost_align_crops_u8(frames.data_ptr(), H * W * 3, F_, H, W, index.data_ptr(), maps.data_ptr(),
                                            None, N, S, crops[k].data_ptr(), S * S * 3,
                                            rz[k].data_ptr() if fused else None, R * R * 3 if fused else 0,
                                            R if fused else 0, st), "align")

    def fused():
        align(0, True)

    def split():
        align(1, False)
        _lib.check(lib.ghost_resize_u8_linear(crops[1].data_ptr(), S * S * 3, N, S, S, rz[1].data_ptr(), R * R * 3,
                                              R, R, st), "resize")

    fused(), split()
    torch.cuda.synchronize()
    same = torch.equal(crops[0], crops[1]) and torch.equal(rz[0], rz[1])

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.launches):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.launches * 1e3   # us per call

    for fn in (fused, split):
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    t = {"fused": [], "split": []}
    for _ in range(a.repeats):
        t["fused"].append(timed(fused))
        t["split"].append(timed(split))
    lines = [f"align A/B on {torch.cuda.get_device_name(0)}: N={N} crops {S}->{R} from {F_} frames {W}x{H}, "
             f"{a.launches} launches x {a.repeats} repeats, alternated, device events",
             f"outputs identical: {same}"]
    for k, v in t.items():
        lines.append(f"{k:6s} us/call: median {np.median(v):8.2f}  min {min(v):8.2f}  max {max(v):8.2f}  "
                     f"spread {max(v) - min(v):6.2f}   repeats: " + " ".join(f"{x:.2f}" for x in v))
    d = np.median(t["split"]) - np.median(t["fused"])
    spread = max(max(v) - min(v) for v in t.values())
    lines.append(f"split - fused (medians): {d:.2f} us; largest repeat-to-repeat spread: {spread:.2f} us; "
                 f"fused is {'faster by more than the spread' if d > spread else 'NOT faster by more than the spread'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    if not same:
        raise SystemExit("the two forms disagree")


if __name__ == "__main__":
    main()
