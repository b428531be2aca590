"""Writes tests/golden/detector_scrfd.npz from the restatement tests/detector_ref.py.

    python tests/golden/make_golden_detector.py

  spec_names / spec_shapes   every parameter of the restatement in graph order (shape padded with zeros to 4)
  map_<i>                    the nine maps (float32 of the float64 evaluation) for N = 2 at det_size (96, 64): two
                             45 x 80 frames, key-hashed weights
  e2e_thresh, e2e_det, e2e_kps, e2e_anchor, e2e_count
                             the restatement's detections of those two frames (the threshold chosen as
                             tests/test_detector_gpu.py chooses it)
They pin the restatement against drift and nothing more: the graph and SCRFD.detect's arithmetic are recalled from
the public sources, not verified, and nothing here is a reference run.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "detector_scrfd.npz")
DET_SIZE = (96, 64)


def build():
    import detector_ref as R
    p = R.make_weights()
    frames = R.make_frames(2, 45, 80, R.E2E_SEED_45x80)
    canvas, scale = R.letterbox(frames, DET_SIZE)
    maps, _ = R.forward(p, canvas, dtype=torch.float64)
    out = {"spec_names": np.array([n for n, _ in R.param_specs()]),
           "spec_shapes": np.array([list(s) + [0] * (4 - len(s)) for _, s in R.param_specs()], np.int32)}
    for i, m in enumerate(maps):
        out[f"map_{i}"] = m.numpy().astype(np.float32)
    scores = np.concatenate([m.numpy().reshape(2, -1) for m in maps[:3]], axis=1)
    thresh, _ = R.gap_threshold(scores)
    dets, kpss, anchors, counts = [], [], [], []
    for f in range(2):
        d, k, a, n = R.detect(R.frame_maps(maps, f), DET_SIZE, thresh, scale)
        dets.append(d); kpss.append(k); anchors.append(a); counts.append([len(a), n])
    out.update(e2e_thresh=np.float64(thresh), e2e_det=np.concatenate(dets), e2e_kps=np.concatenate(kpss),
               e2e_anchor=np.concatenate(anchors), e2e_count=np.array(counts, np.int32))
    return out


if __name__ == "__main__":
    np.savez_compressed(OUT, **build())
    print(OUT, os.path.getsize(OUT))
