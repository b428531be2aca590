"""A/B of the two ways to take the crops from, and paste the swaps into, the frames of a video that lives on the host.

    python tools/bench_roi.py [--frames 900] [--repeats 7] [--pageable-repeats 3] [--out profiles/roi_ab.txt]

full: the frames go up whole in chunks of 32 (two device buffers, copy streams as bench.py's video leg) ->
      align_crops(resize_to=256) -> blend_swaps(resize_to=224) -> the frames come down whole;
roi:  plan_rois on the host (timed, reported separately) -> upload_rois (one 2-D copy per face rectangle) ->
      align_crops_roi -> blend_swaps_roi -> download_rois (one 2-D copy per rectangle back).

The workload is the video leg's (bench.py, config3_video): 1920x1080 frames in pinned memory, 5 % faceless, its
transforms (scale 0.7-0.9, +-0.3 rad) and face_mask_static masks from its synthetic landmarks.  The swap itself is the
same in both chains and is left out: the swaps are the 256 x 256 crops themselves.  Both chains run in one process,
alternated, after a warm-up; a repeat is timed with a host clock around work that ends in a device synchronise.  The
host frames of the two chains are compared byte for byte.  The roi chain also runs from pageable frames.
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
from ghost_amd.inference import (align_crops, align_crops_roi, blend_swaps_roi, download_rois, plan_rois,  # noqa: E402
                                 upload_rois)
from ghost_amd.inference.blend import blend_swaps  # noqa: E402
from ghost_amd.inference.masks import face_masks, mask_params  # noqa: E402
from ghost_amd.inference.streams import stream_set  # noqa: E402

DEV = torch.device("cuda:0")
H, W, S, CH = 1080, 1920, 224, 32


def workload(n):
    """bench.py video_leg's presence, transforms and landmarks (same generator, same order of draws)."""
    rng = np.random.Generator(np.random.PCG64(9))
    present = (rng.random(n) > 0.05).astype(np.int64)
    rng.integers(0, 256, size=(int(present.sum()), 256, 256, 3), dtype=np.uint8)        # the leg's crops: unused here
    tile = torch.from_numpy(rng.integers(0, 256, size=(16, H, W, 3), dtype=np.uint8))
    ang, sc = rng.uniform(-0.3, 0.3, n), rng.uniform(0.7, 0.9, n)
    tx, ty = rng.uniform(600, 1300, n), rng.uniform(200, 700, n)
    mats = np.zeros((n, 2, 3), np.float32)
    mats[:, 0, 0], mats[:, 0, 1] = sc * np.cos(ang), -sc * np.sin(ang)
    mats[:, 1, 0], mats[:, 1, 1] = sc * np.sin(ang), sc * np.cos(ang)
    mats[:, 0, 2] = -(mats[:, 0, 0] * tx + mats[:, 0, 1] * ty)
    mats[:, 1, 2] = -(mats[:, 1, 0] * tx + mats[:, 1, 1] * ty)
    t_ = np.linspace(0.15 * np.pi, 0.85 * np.pi, 33) + np.pi
    base = np.concatenate([np.stack([112 + 78 * np.cos(-t_), 118 + 92 * np.sin(-t_)], 1),
                           np.stack([112 + rng.uniform(-60, 60, 73), 118 + rng.uniform(-70, 60, 73)], 1)])
    lms = (base[None] + rng.normal(0, 1.5, (n, 106, 2))).astype(np.float32)
    lm_tgt = (base + rng.normal(0, 1.5, (106, 2))).astype(np.float32)
    params = np.tile(np.array(mask_params(lms[0], lm_tgt), np.int32), (n, 1))
    return present, tile, mats, lms, params


def fill(dst, tile):
    for i in range(0, dst.shape[0], 16):
        dst[i:i + 16] = tile[:min(16, dst.shape[0] - i)]
    return dst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=900)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pageable-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "roi_ab.txt"))
    a = ap.parse_args()
    n = a.frames
    present, tile, mats, lms, params = workload(n)
    mats64 = mats.astype(np.float64)
    tfm_array = [[mats64[i] if present[i] else [] for i in range(n)]]
    face = np.nonzero(present)[0]
    masks = face_masks(lms, params, S, S, DEV)
    valid_d = torch.from_numpy(present.astype(np.int32)).to(DEV)
    mats_d = torch.from_numpy(mats).to(DEV)
    slot = torch.from_numpy(np.maximum(np.cumsum(present) - 1, 0)).to(DEV)      # frame -> row of the identity's crops
    frames = {"full": fill(torch.empty(n, H, W, 3, dtype=torch.uint8, pin_memory=True), tile),
              "roi": fill(torch.empty(n, H, W, 3, dtype=torch.uint8, pin_memory=True), tile)}
    bufs = [torch.empty(CH, H, W, 3, dtype=torch.uint8, device=DEV) for _ in range(2)]
    s_in, s_out = stream_set(DEV).h2d, stream_set(DEV).d2h
    cur = torch.cuda.current_stream(DEV)
    blend_ev = {"full": [], "roi": []}
    host_s = {"plan": [], "upload_calls": [], "download_calls": []}
    stage_ev, stage_ms = [], {"upload": [], "align": [], "blend": [], "download": []}

    def mark():
        e = torch.cuda.Event(enable_timing=True)
        e.record(cur)
        stage_ev.append(e)

    def bracket(kind):
        e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        blend_ev[kind].append(e)
        return e

    def full():
        fr = frames["full"]
        blend_ev["full"].clear()
        freed = [None, None]
        for c, f0 in enumerate(range(0, n, CH)):
            f1 = min(n, f0 + CH)
            b = bufs[c % 2][:f1 - f0]
            with torch.cuda.stream(s_in):
                if freed[c % 2] is not None:
                    s_in.wait_event(freed[c % 2])
                b.copy_(fr[f0:f1], non_blocking=True)
                loaded = torch.cuda.Event()
                loaded.record(s_in)
            cur.wait_event(loaded)
            _, swaps = align_crops(b, mats64[f0:f1], np.arange(f1 - f0), S, resize_to=256, want_crops=False,
                                   valid=valid_d[f0:f1])
            e0, e1 = bracket("full")
            e0.record(cur)
            blend_swaps(b, swaps, masks[f0:f1], mats_d[f0:f1], valid_d[f0:f1], resize_to=S)
            e1.record(cur)
            blended = torch.cuda.Event()
            blended.record(cur)
            with torch.cuda.stream(s_out):
                s_out.wait_event(blended)
                fr[f0:f1].copy_(b, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(s_out)
                freed[c % 2] = ev
        s_out.synchronize()

    def roi(fr=None, record=True):
        fr = frames["roi"] if fr is None else fr
        blend_ev["roi"].clear()
        stage_ev.clear()
        t0 = time.perf_counter()
        plan = plan_rois(tfm_array, S, (H, W))
        t1 = time.perf_counter()
        mark()
        patches = upload_rois(fr, plan, DEV)
        t2 = time.perf_counter()
        mark()
        _, crops256 = align_crops_roi(patches, plan, 0, mats64[face], S, resize_to=256, want_crops=False)
        swaps = crops256.index_select(0, slot)
        mark()
        e0, e1 = bracket("roi")
        e0.record(cur)
        blend_swaps_roi(patches, plan, 0, swaps, masks, mats, valid=valid_d, resize_to=S)
        e1.record(cur)
        mark()
        t3 = time.perf_counter()
        download_rois(patches, plan, fr)
        t4 = time.perf_counter()
        mark()
        if record:
            host_s["plan"].append(t1 - t0)
            host_s["upload_calls"].append(t2 - t1)
            host_s["download_calls"].append(t4 - t3)
        return plan

    def timed(fn, *args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*args)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    full()
    plan = roi(record=False)
    torch.cuda.synchronize()
    same = torch.equal(frames["full"], frames["roi"])
    changed = not torch.equal(frames["roi"][int(face[0])], tile[int(face[0]) % 16])
    t = {"full": [], "roi": []}
    dev_ms = {"full": [], "roi": []}
    for _ in range(a.repeats):
        for k, fn in (("full", full), ("roi", roi)):
            t[k].append(timed(fn)[0])
            dev_ms[k].append(sum(e0.elapsed_time(e1) for e0, e1 in blend_ev[k]))
            if k == "roi":
                for i, name in enumerate(stage_ms):
                    stage_ms[name].append(stage_ev[i].elapsed_time(stage_ev[i + 1]))
    same = same and torch.equal(frames["full"], frames["roi"])
    # the roi chain from pageable frames (the composites go on top of fresh frames: timing only)
    pageable = fill(torch.empty(n, H, W, 3, dtype=torch.uint8), tile) if a.pageable_repeats else None
    t_page = []
    for i in range(a.pageable_repeats + 1 if a.pageable_repeats else 0):
        el = timed(roi, pageable, False)[0]
        if i:
            t_page.append(el)

    link = {"full": 2 * n * H * W * 3, "roi": 2 * plan.link_bytes()}
    lines = [f"roi A/B on {torch.cuda.get_device_name(0)}: {n} frames {W}x{H} in pinned memory, {len(face)} with a "
             f"face, crop {S} -> 256 -> blend; 1 warm-up + {a.repeats} repeats per chain, alternated, host clock around "
             "work that ends in a device synchronise",
             f"host frames identical after both chains: {same} (faces pasted: {changed})",
             f"patches: {plan.n_patches} on a canvas of {plan.canvas[0]} x {plan.canvas[1]}; mean rectangle "
             f"{plan.rects[:, 2].mean():.0f} x {plan.rects[:, 3].mean():.0f} = "
             f"{100.0 * plan.link_bytes() / (3.0 * H * W * max(plan.n_patches, 1)):.2f} % of a frame"]
    for k in ("full", "roi"):
        v = t[k]
        lines.append(f"{k:5s} link bytes {link[k] / 1e9:7.3f} GB   s/video: median {np.median(v):.4f}  min {min(v):.4f}  "
                     f"max {max(v):.4f}  spread {max(v) - min(v):.4f}  ({n / np.median(v):.0f} frames/s)   repeats: " +
                     " ".join(f"{x:.4f}" for x in v))
        lines.append(f"{k:5s} device time of the blend (events, incl. the 256 -> 224 resize): median "
                     f"{np.median(dev_ms[k]):.3f} ms per video")
    for k, v in host_s.items():
        lines.append(f"roi   host time of {k:14s}: median {1e3 * np.median(v):.2f} ms  min {1e3 * min(v):.2f}  "
                     f"max {1e3 * max(v):.2f}   (inside the roi chain's time)")
    lines.append("roi   stream time between events, ms per video (medians): " +
                 "  ".join(f"{k} {np.median(v):.2f}" for k, v in stage_ms.items()) +
                 f"   ({plan.n_patches} 2-D copies in each direction)")
    if t_page:
        lines.append(f"roi   from pageable frames, s/video: median {np.median(t_page):.4f}  min {min(t_page):.4f}  "
                     f"max {max(t_page):.4f}   repeats: " + " ".join(f"{x:.4f}" for x in t_page))
    d = np.median(t["full"]) - np.median(t["roi"])
    spread = max(max(v) - min(v) for v in t.values())
    verdict = "roi is faster by more than the spread" if d > spread else (
        "full is faster by more than the spread" if -d > spread else "the difference is within the spread")
    lines.append(f"full - roi (medians): {d:.4f} s; largest repeat-to-repeat spread: {spread:.4f} s; {verdict}; "
                 f"ratio full / roi = {np.median(t['full']) / np.median(t['roi']):.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    if not same:
        raise SystemExit("the two chains disagree")


if __name__ == "__main__":
    main()
