"""ghost_amd.detection on an MI355X against the restatement tests/detector_ref.py (key-hashed weights, N <= 3, det_size
(96, 64) and once (160, 128)).

There is no reference run to compare with (no ONNX file, no onnxruntime, no insightface): the restatement is written
from a description of the graph and of SCRFD.detect recalled from the public sources, and parity against onnxruntime stays unpinned.

Gates
  fp32      the nine maps and the four taps against float64: max abs <= 1e-3 (the project's fp32 bar; the outputs are
            O(1) under the weight recipe)
  16-bit    fp16 and bf16: mean and top 0.5 % of |x - x64| over the nine maps, and over the stage-4 tap, <= 1.25 x the
            same figure of detector_ref.forward(store=dt), which rounds exactly at the kernels' rounding points
  rows      a row of an N = 3 call equals the frame alone within the fp32 bar
  e2e fp32  detect_frames on two 45 x 80 frames and one 80 x 45 frame (two calls): the threshold is the midpoint of
            the widest gap between ranks 8 and 20 of the restatement's sorted float64 scores (asserted >= 4e-3) and no
            restated pair's overlap lies within 1e-2 of 0.4; then the kept anchors and their order equal the
            restatement's and the coordinates agree within 1e-3 * 32 / det_scale px
  Face_detect_crop.get_frames  None for a frame without a candidate; its output feeds crop_frames_and_get_transforms

Measured on an MI355X (DESIGN.md §12 holds the same figures; the tests print them as DETFIG lines):
  fp32   maps cls 2.6e-7 / 1.4e-7 / 5.0e-8, reg 1.4e-6 / 3.8e-7 / 1.0e-7, kps 2.1e-6 / 5.0e-7 / 1.7e-7 (strides 8 / 16 /
         32); taps stem 1.8e-6, layer1 2.4e-6, layer4 7.6e-7, p3 1.4e-6; (160, 128) maps 1.9e-6
  fp16   maps mean 2.157e-4 (emulation 2.151e-4) top 0.5 % 1.026e-3 (1.019e-3); layer4 1.689e-4 (1.659e-4) / 1.164e-3
         (1.017e-3); keypoint error mean 0.0020, max 0.014 canvas px
  bf16   maps mean 1.845e-3 (emulation 1.844e-3) top 0.5 % 9.04e-3 (8.95e-3); layer4 1.268e-3 (1.277e-3) / 8.26e-3
         (8.28e-3); keypoint error mean 0.017, max 0.092 canvas px
  row 1 of an N = 3 call against the frame alone: identical
  e2e    45 x 80: thresh 0.713815, gap 8.1e-3, kept [3, 13], max coordinate error 9.5e-6 px (bar 2.7e-2)
         80 x 45: thresh 0.721375, gap 9.8e-3, kept [12], max coordinate error 2.3e-5 px (bar 4.0e-2)
"""
import numpy as np
import pytest
import torch

import detector_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FP32_BAR = 1e-3
DET_SIZE = (96, 64)


@pytest.fixture(scope="module")
def weights():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return R.make_weights()


def _net(weights, det_size=DET_SIZE, compute_dtype=None):
    from ghost_amd.detection import SCRFD
    net = SCRFD(det_size=det_size, compute_dtype=compute_dtype)
    net.load_arrays(weights)
    return net.to(DEV)


@pytest.fixture(scope="module")
def net32(weights):
    return _net(weights)


@pytest.fixture(scope="module")
def frames3():
    return R.make_frames(3, 45, 80, R.E2E_SEED_45x80)       # the first two are the e2e frames


@pytest.fixture(scope="module")
def ref64(weights, frames3):
    """float64 maps and taps of frames3, computed once; and det_scale."""
    canvas, scale = R.letterbox(frames3, DET_SIZE)
    maps, taps = R.forward(weights, canvas, dtype=torch.float64)
    return maps, taps, scale, canvas


def _errs(got, want):
    return [float((g.cpu().double() - w).abs().max()) for g, w in zip(got, want)]


def test_fp32_maps_and_taps(net32, frames3, ref64):
    maps, taps = net32.forward_taps(torch.from_numpy(frames3).to(DEV))
    torch.cuda.synchronize()
    for name, e, m in zip(["cls8", "cls16", "cls32", "reg8", "reg16", "reg32", "kps8", "kps16", "kps32"],
                          _errs(maps, ref64[0]), maps):
        print(f"DETFIG fp32 map {name} max|d|={e:.3e}")
        assert m.dtype == torch.float32 and e <= FP32_BAR, (name, e)
    for name, t in zip(R.TAP_NAMES, taps):
        e = float((t.cpu().double() - ref64[1][name]).abs().max())
        print(f"DETFIG fp32 tap {name} max|d|={e:.3e}")
        assert t.dtype == torch.float32 and e <= FP32_BAR, (name, e)


def test_fp32_second_det_size(weights):
    det_size = (160, 128)
    frames = R.make_frames(1, 100, 150, 41)
    canvas, _ = R.letterbox(frames, det_size)
    want, _ = R.forward(weights, canvas, dtype=torch.float64)
    maps = _net(weights, det_size).forward(torch.from_numpy(frames).to(DEV))
    torch.cuda.synchronize()
    e = max(_errs(maps, want))
    print(f"DETFIG fp32 (160,128) maps max|d|={e:.3e}")
    assert tuple(maps[0].shape) == (1, 2, 16, 20) and tuple(maps[8].shape) == (1, 20, 4, 5) and e <= FP32_BAR


def _figs(x, x64):
    d = (x.double() - x64).abs().flatten()
    k = max(1, int(round(d.numel() * 0.005)))
    return float(d.mean()), float(d.topk(k).values.min())


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_16bit_against_storage_emulation(weights, frames3, ref64, dt):
    tn = "f16" if dt == torch.float16 else "bf16"
    maps, taps = _net(weights, compute_dtype=dt).forward_taps(torch.from_numpy(frames3).to(DEV))
    torch.cuda.synchronize()
    emaps, etaps = R.forward(weights, ref64[3], dtype=torch.float32, store=dt)
    cat = lambda ms: torch.cat([m.cpu().double().flatten() for m in ms])
    assert all(m.dtype == torch.float32 for m in maps) and taps[2].dtype == dt
    for name, got, emu, want in (("maps", cat(maps), cat(emaps), cat(ref64[0])),
                                 ("layer4", cat([taps[2]]), cat([etaps["layer4"]]), cat([ref64[1]["layer4"]]))):
        (gm, gt), (em, et) = _figs(got, want), _figs(emu, want)
        print(f"DETFIG {tn} {name} mean {gm:.3e} (emulation {em:.3e}) top0.5% {gt:.3e} ({et:.3e})")
        assert gm <= 1.25 * em and gt <= 1.25 * et, (name, gm, em, gt, et)
    # keypoint error in canvas pixels (the scale of a 640 x 640 input): |d kps| * stride per level
    errs = torch.cat([((g.cpu().double() - w).abs() * s).flatten() for g, w, s in zip(maps[6:], ref64[0][6:], R.STRIDES)])
    print(f"DETFIG {tn} keypoint error mean {float(errs.mean()):.4f} max {float(errs.max()):.4f} px (canvas pixels)")


def test_row_independence(net32, frames3):
    fd = torch.from_numpy(frames3).to(DEV)
    all3 = net32.forward(fd)
    one = net32.forward(fd[1:2].clone())
    torch.cuda.synchronize()
    e = max(float((a[1:2] - b).abs().max()) for a, b in zip(all3, one))
    print(f"DETFIG row 1 of N=3 against the frame alone max|d|={e:.3e}")
    assert e <= FP32_BAR


def _e2e_call(weights, net, frames):
    canvas, scale = R.letterbox(frames, DET_SIZE)
    maps, _ = R.forward(weights, canvas, dtype=torch.float64)
    n = frames.shape[0]
    scores = np.concatenate([m.numpy().reshape(n, -1) for m in maps[:3]], axis=1)
    thresh, gap = R.gap_threshold(scores)
    assert gap >= 4e-3, f"score gap {gap}: change the seed (detector_ref.E2E_SEED_*)"
    det, kps, count, anchor = net.detect_frames(torch.from_numpy(frames).to(DEV), thresh, return_anchor=True)
    torch.cuda.synchronize()
    det, kps, count, anchor = (t.cpu().numpy() for t in (det, kps, count, anchor))
    tol = FP32_BAR * 32 / scale
    worst = 0.0
    for f in range(n):
        fm = R.frame_maps(maps, f)
        sc, box, _, _ = R.decode(fm, DET_SIZE, thresh, scale)
        assert R.min_ovr_margin(np.concatenate([box, sc[:, None]], axis=1)) >= 1e-2, "change the seed"
        d, k, a, nc = R.detect(fm, DET_SIZE, thresh, scale)
        assert count[f].tolist() == [len(a), nc]
        assert anchor[f, :len(a)].tolist() == a.tolist()
        if len(a):
            worst = max(worst, float(np.abs(det[f, :len(a), :4] - d[:, :4]).max()),
                        float(np.abs(kps[f, :len(a)] - k).max()))
            assert float(np.abs(det[f, :len(a), 4] - d[:, 4]).max()) <= FP32_BAR
    print(f"DETFIG e2e {frames.shape[1]}x{frames.shape[2]} thresh {thresh:.6f} gap {gap:.2e} kept "
          f"{count[:, 0].tolist()} max coordinate error {worst:.3e} px (bar {tol:.3e})")
    assert worst <= tol
    return count


def test_e2e_fp32(weights, net32):
    c = _e2e_call(weights, net32, R.make_frames(2, 45, 80, R.E2E_SEED_45x80))
    assert (c[:, 0] > 0).all()
    c = _e2e_call(weights, net32, R.make_frames(1, 80, 45, R.E2E_SEED_80x45))
    assert c[0, 0] >= 8


def test_face_detect_crop_feeds_the_aligner(weights, net32):
    from ghost_amd.detection import Face_detect_crop
    from ghost_amd.inference import align_crops, crop_frames_and_get_transforms
    frames = R.make_frames(2, 45, 80, R.NOFACE_SEED_45x80)
    canvas, _ = R.letterbox(frames, DET_SIZE)
    maps, _ = R.forward(weights, canvas, dtype=torch.float64)
    scores = np.concatenate([m.numpy().reshape(2, -1) for m in maps[:3]], axis=1)
    thresh, gap = R.gap_threshold(scores)
    assert gap >= 4e-3 and scores[1].max() < thresh - 2e-3 and scores[0].max() > thresh + 2e-3
    app = Face_detect_crop(net32)
    app.prepare(ctx_id=0, det_thresh=thresh, det_size=DET_SIZE)
    fd = torch.from_numpy(frames).to(DEV)
    kps = app.get_frames(fd, max_num=1)
    assert kps[1] is None and kps[0].dtype == np.float32 and kps[0].shape == (1, 5, 2)
    many = app.get_frames(fd)
    assert many[1] is None and many[0].shape[0] > 1 and many[0].shape[1:] == (5, 2)
    one = app.get(frames[0], 224)
    assert isinstance(one, list) and len(one) == many[0].shape[0] and np.array_equal(one[0], many[0][0])
    assert app.get(fd[1], 224) is None
    templates = np.array([[[38.0, 52.0], [74.0, 51.0], [56.0, 72.0], [41.0, 92.0], [71.0, 91.0]]]) * 2.0
    target = torch.zeros(1, 512, device=DEV)
    crops, rz, present, tfm = crop_frames_and_get_transforms(fd, kps, target, None, 224, False, 0.15, templates)
    assert present[0].tolist() == [1, 0] and tuple(crops[0].shape) == (1, 224, 224, 3)
    M = np.asarray(tfm[0][0], np.float64)
    assert M.shape == (2, 3)
    c, _ = align_crops(fd, M[None], [0], 224)
    assert torch.equal(c, crops[0])
