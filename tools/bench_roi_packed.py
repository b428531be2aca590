"""A/B of the two ways to move the face rectangles of a video that lives on the host: one 2-D copy per rectangle
(upload_rois / download_rois) against packed transfers (upload_rois_packed / download_rois_packed: the host packs the
rectangles into a pinned staging buffer, one copy per chunk, one kernel spreads them over the canvas).

    python tools/bench_roi_packed.py [--frames 900] [--repeats 7] [--out profiles/roi_packed_ab.txt]

Both chains are  plan_rois -> upload -> align_crops_roi -> blend_swaps_roi -> download  on the workload of
tools/bench_roi.py (bench.py's video leg: 1920x1080 frames, 5 % faceless, the swap left out).  They run in one process,
alternated, after a warm-up; a repeat is timed with a host clock around work that ends with the host frames written
(the per-patch chain ends in a device synchronise, the packed chain returns with them written).  Both run from pinned
and from pageable frames; the frames of the two chains are compared byte for byte.  The staging buffer is allocated
once, outside the timed region, as a video pipeline would.  Also: the host time of packing alone, the device time of
the unpack / pack kernels against the link time of the same bytes, and a sweep of threads x chunk_bytes.
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
sys.path.insert(0, os.path.join(REPO, "tools"))
from bench_roi import DEV, H, S, W, fill, workload  # noqa: E402
from ghost_amd.inference import (RoiStaging, align_crops_roi, blend_swaps_roi, download_rois,  # noqa: E402
                                 download_rois_packed, packed_layout, plan_rois, upload_rois, upload_rois_packed)
from ghost_amd.inference import roi_pack  # noqa: E402
from ghost_amd.inference.masks import face_masks  # noqa: E402
from ghost_amd.inference.roi import _frame_pointers  # noqa: E402

STAGES = ("upload", "align", "blend", "download")
MIB = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=900)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sweep-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "roi_packed_ab.txt"))
    a = ap.parse_args()
    n = a.frames
    present, tile, mats, lms, params = workload(n)
    mats64 = mats.astype(np.float64)
    tfm_array = [[mats64[i] if present[i] else [] for i in range(n)]]
    face = np.nonzero(present)[0]
    masks = face_masks(lms, params, S, S, DEV)
    valid_d = torch.from_numpy(present.astype(np.int32)).to(DEV)
    slot = torch.from_numpy(np.maximum(np.cumsum(present) - 1, 0)).to(DEV)
    cur = torch.cuda.current_stream(DEV)
    plan0 = plan_rois(tfm_array, S, (H, W))
    total = packed_layout(plan0)[1]
    staging = RoiStaging(total, DEV)
    stage_ev = []

    def mark():
        e = torch.cuda.Event(enable_timing=True)
        e.record(cur)
        stage_ev.append(e)

    def chain(fr, packed, threads=0, chunk_bytes=None, host_s=None):
        """One video through one chain; returns with the host frames written."""
        stage_ev.clear()
        plan = plan_rois(tfm_array, S, (H, W))
        mark()
        t0 = time.perf_counter()
        if packed:
            patches = upload_rois_packed(fr, plan, DEV, staging=staging, chunk_bytes=chunk_bytes, threads=threads)
        else:
            patches = upload_rois(fr, plan, DEV)
        t1 = time.perf_counter()
        mark()
        _, crops256 = align_crops_roi(patches, plan, 0, mats64[face], S, resize_to=256, want_crops=False)
        swaps = crops256.index_select(0, slot)
        mark()
        blend_swaps_roi(patches, plan, 0, swaps, masks, mats, valid=valid_d, resize_to=S)
        mark()
        t2 = time.perf_counter()
        if packed:
            download_rois_packed(patches, plan, fr, staging=staging, chunk_bytes=chunk_bytes, threads=threads)
        else:
            download_rois(patches, plan, fr)
        t3 = time.perf_counter()
        mark()
        if not packed:
            torch.cuda.synchronize()
        if host_s is not None:
            host_s["upload call"].append(t1 - t0)
            host_s["download call"].append(t3 - t2)
        return plan

    def timed(*args, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        chain(*args, **kw)
        el = time.perf_counter() - t0
        torch.cuda.synchronize()
        return el, [stage_ev[i].elapsed_time(stage_ev[i + 1]) for i in range(len(STAGES))]

    def ab(make, label):
        """1 warm-up + repeats of both chains, alternated, each on frames of its own."""
        fr = {False: make(), True: make()}
        t, st = {False: [], True: []}, {False: [], True: []}
        hs = {k: {"upload call": [], "download call": []} for k in (False, True)}
        for k in (False, True):
            chain(fr[k], k)
        torch.cuda.synchronize()
        same = torch.equal(fr[False], fr[True])
        changed = not torch.equal(fr[True][int(face[0])], tile[int(face[0]) % 16])
        for _ in range(a.repeats):
            for k in (False, True):
                el, ms = timed(fr[k], k, host_s=hs[k])
                t[k].append(el)
                st[k].append(ms)
        same = same and torch.equal(fr[False], fr[True])
        out = [f"--- {label} frames: 1 warm-up + {a.repeats} repeats per chain, alternated; host frames identical after "
               f"both chains: {same} (faces pasted: {changed})"]
        for k, name in ((False, "per-patch"), (True, "packed   ")):
            v = t[k]
            out.append(f"{name} s/video: median {np.median(v):.4f}  min {min(v):.4f}  max {max(v):.4f}  spread "
                       f"{max(v) - min(v):.4f}  ({n / np.median(v):.0f} frames/s)   repeats: " +
                       " ".join(f"{x:.4f}" for x in v))
            out.append(f"{name} stream time between events, ms per video (medians): " +
                       "  ".join(f"{s} {np.median([m[i] for m in st[k]]):.2f}" for i, s in enumerate(STAGES)) +
                       "   host time of the calls, ms: " +
                       "  ".join(f"{s} {1e3 * np.median(x):.2f}" for s, x in hs[k].items()))
        d = np.median(t[False]) - np.median(t[True])
        spread = max(max(v) - min(v) for v in t.values())
        verdict = "packed is faster by more than the spread" if d > spread else (
            "per-patch is faster by more than the spread" if -d > spread else "the difference is within the spread")
        out.append(f"per-patch - packed (medians): {d:.4f} s; largest repeat-to-repeat spread: {spread:.4f} s; "
                   f"{verdict}; ratio per-patch / packed = {np.median(t[False]) / np.median(t[True]):.2f}")
        return out, same, fr[True]

    lines = [f"packed roi A/B on {torch.cuda.get_device_name(0)}: {n} frames {W}x{H}, {len(face)} with a face, crop {S} "
             "-> 256 -> blend; host clock around work that ends with the host frames written",
             f"patches: {plan0.n_patches} on a canvas of {plan0.canvas[0]} x {plan0.canvas[1]}; rectangle bytes "
             f"{plan0.link_bytes() / 1e9:.4f} GB, packed {total / 1e9:.4f} GB per direction; defaults: threads "
             f"{roi_pack.DEFAULT_THREADS}, chunk_bytes {roi_pack.DEFAULT_CHUNK_BYTES // MIB} MiB; one RoiStaging, "
             "allocated once outside the timed region"]
    out, same_pin, pinned = ab(lambda: fill(torch.empty(n, H, W, 3, dtype=torch.uint8, pin_memory=True), tile), "pinned")
    lines += out

    # ---- the sweep (pinned frames, the packed chain) ----
    lines.append(f"--- sweep of the packed chain from pinned frames, s/video (median of {a.sweep_repeats}, after one "
                 "warm-up each): rows threads, columns chunk_bytes")
    chunk_sets = [("8 MiB", 8 * MIB), ("32 MiB", 32 * MIB), ("128 MiB", 128 * MIB), ("whole", 1 << 40)]
    lines.append("threads  " + "  ".join(f"{c[0]:>8s}" for c in chunk_sets))
    best = None
    for threads in (1, 4, 8, 16):
        row = []
        for cname, cb in chunk_sets:
            chain(pinned, True, threads, cb)
            v = [timed(pinned, True, threads, cb)[0] for _ in range(a.sweep_repeats)]
            row.append(float(np.median(v)))
            if best is None or row[-1] < best[0]:
                best = (row[-1], threads, cname)
        lines.append(f"{threads:7d}  " + "  ".join(f"{x:8.4f}" for x in row))
    lines.append(f"fastest cell: threads {best[1]}, chunk_bytes {best[2]}: {best[0]:.4f} s/video")

    # ---- the parts alone: host packing, the kernels, the link ----
    plan = plan0
    call = roi_pack._Call(torch.empty(plan.n_patches, plan.canvas[0], plan.canvas[1], 3, dtype=torch.uint8, device=DEV),
                          plan, _frame_pointers(pinned, plan, "bench", True), staging)
    Np = plan.n_patches

    def host_ms(to_staging, threads):
        v = []
        for _ in range(5):
            t0 = time.perf_counter()
            call.host(0, Np, to_staging, threads, "bench")
            v.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(v))

    def dev_ms(fn):
        v = []
        for _ in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(cur)
            fn()
            e1.record(cur)
            e1.synchronize()
            v.append(e0.elapsed_time(e1))
        return float(np.median(v[1:]))

    torch.cuda.synchronize()
    lines.append("--- the parts alone, whole video in one call (pinned frames; medians of 5)")
    for threads in (1, 4, 8, 16):
        lines.append(f"host packing, {threads:2d} threads: frames -> staging {host_ms(True, threads):7.2f} ms   "
                     f"staging -> frames {host_ms(False, threads):7.2f} ms")
    up = dev_ms(lambda: staging.dev.copy_(staging.host, non_blocking=True))
    down = dev_ms(lambda: staging.host.copy_(staging.dev, non_blocking=True))
    k_un = dev_ms(lambda: call.kernel(0, Np, True, "bench"))
    k_pk = dev_ms(lambda: call.kernel(0, Np, False, "bench"))
    gb = total / 1e9
    lines.append(f"link, {gb:.4f} GB in one copy: host to device {up:.2f} ms ({gb / up * 1e3:.1f} GB/s)   device to "
                 f"host {down:.2f} ms ({gb / down * 1e3:.1f} GB/s)")
    lines.append(f"kernels, {gb:.4f} GB packed + {plan.link_bytes() / 1e9:.4f} GB canvas each: unpack (to the canvas) "
                 f"{k_un:.3f} ms ({2 * gb / k_un * 1e3:.0f} GB/s read + written)   pack (from the canvas) {k_pk:.3f} "
                 f"ms ({2 * gb / k_pk * 1e3:.0f} GB/s)")
    below = "the kernels are below the link time" if k_un < up and k_pk < down else \
        "a kernel is NOT below the link time: it is the bottleneck"
    lines.append(f"unpack kernel / link time of the same bytes: {k_un / up:.3f}; pack kernel / link: "
                 f"{k_pk / down:.3f} ({below})")
    del call, pinned
    torch.cuda.synchronize()

    out, same_page, _ = ab(lambda: fill(torch.empty(n, H, W, 3, dtype=torch.uint8), tile), "pageable")
    lines += out
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    if not (same_pin and same_page):
        raise SystemExit("the two chains disagree")


if __name__ == "__main__":
    main()
