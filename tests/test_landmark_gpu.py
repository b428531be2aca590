"""ghost_amd.landmarks on an MI355X against the float64 restatement tests/landmark_ref.py (key-hashed weights, N <= 3).

There is no reference run to compare with (no mxnet, no checkpoint): the restatement is written from the symbol
file's records and image_infer.py, and numerics against mxnet stay unpinned.

Gates
  fp32     max |pred - pred64| and max |tap - tap64| <= 1e-3 (the project's fp32 bar); landmarks are pred scaled by
           96 * 1.75 = 168, so max |landmarks - landmarks64| <= 0.168 px is the same bar
  16-bit   mean and top-0.5 % of |x - x64| for x = pred and x = the conv_14 tap <= 1.25 x the same figure of the
           storage emulation (landmark_ref.forward(store=dt), fp32 in between)
  the landmark transform is within 2 fp32 ulps of its float64 value on the kernel's own pred
  a row of an N = 3 call agrees with the same crop alone within the fp32 bar

Measured on an MI355X (DESIGN.md §11 holds the same figures; the tests print them as LMKFIG lines):
  fp32   max|dpred| 1.0e-6; taps conv_2 1.9e-6, conv_7 4.6e-6, conv_14 2.5e-5, conv_15 1.5e-5
         through the warp: max|dpred| 1.3e-6, max|dlandmark| 2.2e-4 px; the transform 0.5 ulp
  fp16   pred mean 3.37e-4 (emulation 3.19e-4) top 0.5 % 1.36e-3 (1.34e-3); conv_14 2.45e-3 (2.49e-3) / 1.75e-2 (1.81e-2)
  bf16   pred mean 2.30e-3 (emulation 2.50e-3) top 0.5 % 8.62e-3 (8.53e-3); conv_14 1.92e-2 (1.96e-2) / 1.32e-1 (1.38e-1)
  landmarks against float64: fp16 mean 0.057 px, max 0.26 px; bf16 mean 0.39 px, max 1.5 px
  row 1 of an N = 3 call against the crop alone: identical
"""
import numpy as np
import pytest
import torch

import landmark_ref
from oracle import blend_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FP32_BAR = 1e-3


@pytest.fixture(scope="module")
def weights():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return landmark_ref.make_weights()


def _net(weights, compute_dtype=None):
    from ghost_amd.landmarks import Landmark106
    net = Landmark106(compute_dtype=compute_dtype)
    net.load_state_dict(weights, strict=True)
    return net.to(DEV)


@pytest.fixture(scope="module")
def net32(weights):
    return _net(weights)


@pytest.fixture(scope="module")
def x3():
    return landmark_ref.make_input(3)


@pytest.fixture(scope="module")
def ref64(weights, x3):
    """float64 pred and taps of x3, computed once."""
    return landmark_ref.forward(weights, x3, bgr=True, dtype=torch.float64)


@pytest.fixture(scope="module")
def crops3():
    return landmark_ref.make_input(3, 224)


def test_fp32_pred_and_taps(net32, x3, ref64):
    pred, taps = net32.forward_taps(x3.to(DEV))
    torch.cuda.synchronize()
    err = float((pred.cpu().double() - ref64[0]).abs().max())
    print(f"LMKFIG fp32 max|dpred|={err:.3e}")
    assert err <= FP32_BAR
    for name, t in zip(landmark_ref.TAP_NAMES, taps):
        e = float((t.cpu().double() - ref64[1][name]).abs().max())
        print(f"LMKFIG fp32 tap {name} max|d|={e:.3e}")
        assert t.dtype == torch.float32 and e <= FP32_BAR, (name, e)
    # R,G,B input order: the same bytes flipped give the same result
    p_rgb = net32.forward(x3.flip(-1).contiguous().to(DEV), bgr=False)
    assert torch.equal(p_rgb, pred)
    assert torch.equal(net32.forward(x3.to(DEV)), pred)          # taps do not change the result


def test_landmarks_u8_against_cv_warp(net32, weights, crops3):
    lm, pred = net32.landmarks_u8(crops3.to(DEV), return_pred=True)
    torch.cuda.synchronize()
    x192 = np.stack([blend_ref.warp_affine_cv(c, landmark_ref.M, (192, 192), "constant") for c in crops3.numpy()])
    assert x192[:, :50].any() and not x192[:, 190:].any()        # the crop fills [32, 160): borders are constant 0
    p64, _ = landmark_ref.forward(weights, torch.from_numpy(x192), bgr=True, dtype=torch.float64)
    e = float((pred.cpu().double() - p64).abs().max())
    el = float((lm.cpu().double() - landmark_ref.landmarks_of(p64)).abs().max())
    print(f"LMKFIG landmarks_u8 max|dpred|={e:.3e} max|dlandmark|={el:.3e} px")
    assert lm.dtype == torch.float32 and tuple(lm.shape) == (3, 106, 2)
    assert e <= FP32_BAR and el <= FP32_BAR * 168.0
    # the transform alone, on the kernel's own pred: 2 ulps of the float64 value
    want = landmark_ref.landmarks_of(pred.cpu().double())
    ulp = torch.from_numpy(np.spacing(want.abs().numpy().astype(np.float32))).double()
    worst = float(((lm.cpu().double() - want).abs() / ulp).max())
    print(f"LMKFIG landmark transform: {worst:.3f} ulp")
    assert worst <= 2.0


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_16bit_against_storage_emulation(weights, x3, ref64, dt):
    net = _net(weights, dt)
    pred, taps = net.forward_taps(x3.to(DEV))
    torch.cuda.synchronize()
    assert taps[2].dtype == dt and bool(torch.isfinite(pred).all())
    pe, te = landmark_ref.forward(weights, x3, bgr=True, dtype=torch.float32, store=dt)
    for what, got, emu, ref in (("pred", pred.cpu(), pe, ref64[0]),
                                ("conv_14", taps[2].cpu(), te["conv_14"], ref64[1]["conv_14"])):
        dg, de = (got.double() - ref).abs().flatten(), (emu.double() - ref).abs().flatten()
        k = max(1, dg.numel() // 200)
        tg, tm = float(dg.topk(k).values.mean()), float(de.topk(k).values.mean())
        print(f"LMKFIG {dt} {what} mean|d| gpu={float(dg.mean()):.3e} emu={float(de.mean()):.3e} "
              f"top0.5% gpu={tg:.3e} emu={tm:.3e}")
        assert float(dg.mean()) <= 1.25 * float(de.mean()), (what, float(dg.mean()), float(de.mean()))
        assert tg <= 1.25 * tm, (what, tg, tm)
    lm_err = (landmark_ref.landmarks_of(pred.cpu().double()) - landmark_ref.landmarks_of(ref64[0])).abs()
    print(f"LMKFIG {dt} landmarks mean|d|={float(lm_err.mean()):.3e} max={float(lm_err.max()):.3e} px")


def test_half_module_selects_fp16_storage(weights, x3):
    net = _net(weights).half()
    _, taps = net.forward_taps(x3[:1].to(DEV))
    assert taps[0].dtype == torch.float16


def test_batch_row_alone_empty_and_strided(net32, x3, crops3):
    xd = x3.to(DEV)
    p3 = net32.forward(xd)
    p1 = net32.forward(xd[1:2])
    e = float((p3[1:2] - p1).abs().max())
    print(f"LMKFIG row 1 of N=3 against the crop alone: {e:.3e}")
    assert e <= FP32_BAR
    assert tuple(net32.forward(xd[:0]).shape) == (0, 212)
    assert tuple(net32.landmarks_u8(crops3[:0].to(DEV)).shape) == (0, 106, 2)
    wide = torch.zeros(6, 192, 192, 3, dtype=torch.uint8, device=DEV)
    wide[::2] = xd
    assert torch.equal(net32.forward(wide[::2]), p3)
    cw = torch.zeros(6, 224, 224, 3, dtype=torch.uint8, device=DEV)
    cw[1::2] = crops3.to(DEV)
    assert torch.equal(net32.landmarks_u8(cw[1::2]), net32.landmarks_u8(crops3.to(DEV)))


def test_handler_returns_landmarks_u8(net32, crops3):
    from ghost_amd.landmarks import Handler
    h = Handler(net32)
    want = net32.landmarks_u8(crops3[:1].to(DEV))[0].cpu().numpy()
    a = h.get_without_detection_without_transform(crops3[0].numpy())
    b = h.get_without_detection_without_transform(crops3[0].to(DEV))
    assert a.dtype == np.float32 and a.shape == (106, 2)
    assert np.array_equal(a, want) and np.array_equal(b, want)
    with pytest.raises(RuntimeError):
        h.get_without_detection_without_transform(np.zeros((192, 192, 3), np.uint8))


def test_identity_masks_equals_hand_computed(net32):
    from ghost_amd.inference.blend import resize_u8
    from ghost_amd.inference.masks import face_masks, mask_params
    from ghost_amd.landmarks import identity_masks
    g = np.random.Generator(np.random.PCG64(11))
    present = [1, 1, 0, 1, 1]
    swaps = torch.from_numpy(g.integers(0, 256, (5, 256, 256, 3), dtype=np.uint8)).to(DEV)
    crops = torch.from_numpy(g.integers(0, 256, (5, 224, 224, 3), dtype=np.uint8)).to(DEV)
    masks, s224, lm, params = identity_masks(net32, swaps, crops, present)
    # by hand, with the same batches: all present swaps, then the first crop of each run (frames 0 and 3)
    want224 = resize_u8(swaps, (224, 224))
    idx = torch.tensor([0, 1, 3, 4], device=DEV)
    lms = net32.landmarks_u8(want224[idx]).cpu().numpy()
    lmt = net32.landmarks_u8(crops[torch.tensor([0, 3], device=DEV)]).cpu().numpy()
    pr = np.array([mask_params(lms[0], lmt[0])] * 2 + [mask_params(lms[2], lmt[1])] * 2, np.int32)
    want = face_masks(lms, pr, 224, 224, DEV)
    assert torch.equal(s224, want224)
    assert np.array_equal(lm[[0, 1, 3, 4]], lms) and not lm[2].any()
    assert np.array_equal(params[[0, 1, 3, 4]], pr)
    assert torch.equal(masks[idx], want) and not bool(masks[2].any())
    assert float(want.max()) > 0.5                                # the masks are not empty


def test_cpu_input_raises(net32):
    with pytest.raises(RuntimeError):
        net32.forward(torch.zeros(1, 192, 192, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        net32.forward(torch.zeros(1, 3, 192, 192, dtype=torch.uint8, device=DEV))
