"""ghost_align_crops_u8 / ghost_amd.inference.align on the GPU: byte-exact against the OpenCV restatement
oracle.blend_ref.warp_affine_cv(frame, M, (S, S), "constant") and resize_linear_u8 of it."""
import numpy as np
import pytest
import torch

from oracle import blend_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FRONTAL = np.array([[38.0, 52.0], [74.0, 51.0], [56.0, 72.0], [41.0, 92.0], [71.0, 91.0]])


def _tfm(scale, ang, cx, cy, S):
    """frame -> crop: crop = scale * Rot(ang) (frame - centre) + S/2, float64 as estimate_norm returns it."""
    c, s = scale * np.cos(ang), scale * np.sin(ang)
    return np.array([[c, -s, S / 2 - (c * cx - s * cy)], [s, c, S / 2 - (s * cx + c * cy)]], np.float64)


def _oracle(frames, tfms, index, S, Rz=None):
    crops = np.stack([R.warp_affine_cv(frames[f], M, (S, S), "constant") for f, M in zip(index, tfms)])
    rz = None if Rz is None else np.stack([R.resize_linear_u8(c, (Rz, Rz)) for c in crops])
    return crops, rz


class _Small:
    S, Rz, INDEX = 56, 64, [2, 0, 0, 1, 2, 1, 0]

    def __init__(self):
        g = np.random.Generator(np.random.PCG64(2024))
        self.frames = g.integers(0, 256, size=(3, 96, 128, 3), dtype=np.uint8)
        S = self.S
        self.tfms = np.stack([
            _tfm(0.9, 0.0, 64.0, 48.0, S),         # well inside the frame
            _tfm(2.7, 0.2, 50.3, 40.6, S),         # upsampling
            _tfm(0.35, -0.1, 60.0, 50.0, S),       # minification: the crop sees more than the frame
            _tfm(1.0, 0.4, 70.2, 50.1, S),
            _tfm(1.0, -0.4, 55.7, 44.4, S),
            _tfm(1.0, 0.0, 118.0, 10.0, S),        # about half the crop is border
            _tfm(1.0, 0.1, -200.0, -300.0, S),     # wholly outside: all zeros
        ])
        self.crops, self.rz = _oracle(self.frames, self.tfms, self.INDEX, S, self.Rz)
        self.dev_frames = torch.from_numpy(self.frames).to(DEV)


@pytest.fixture(scope="module")
def small():
    return _Small()


def test_align_crops_small_case(small):
    from ghost_amd.inference import align_crops
    # the oracle's zero-pixel fractions: no border, about half border, all border
    zero = [(c.reshape(-1, 3) == 0).all(axis=1).mean() for c in small.crops]
    assert zero[0] == 0.0 and zero[6] == 1.0 and 0.3 < zero[5] < 0.7 and zero[2] > 0.2
    crops, rz = align_crops(small.dev_frames, small.tfms, small.INDEX, small.S, resize_to=small.Rz)
    assert crops.shape == (7, 56, 56, 3) and rz.shape == (7, 64, 64, 3) and crops.dtype == rz.dtype == torch.uint8
    assert np.array_equal(crops.cpu().numpy(), small.crops)
    assert np.array_equal(rz.cpu().numpy(), small.rz)
    assert not crops[6].any() and not rz[6].any()


def test_align_crops_one_output_each(small):
    from ghost_amd.inference import align_crops
    crops, rz = align_crops(small.dev_frames, small.tfms, small.INDEX, small.S)
    assert rz is None and np.array_equal(crops.cpu().numpy(), small.crops)
    crops, rz = align_crops(small.dev_frames, small.tfms, small.INDEX, small.S, resize_to=small.Rz, want_crops=False)
    assert crops is None and np.array_equal(rz.cpu().numpy(), small.rz)


def test_align_crops_unfused_ratio_goes_through_the_resize_kernel(small):
    from ghost_amd.inference import align_crops
    crops, rz = align_crops(small.dev_frames, small.tfms, small.INDEX, small.S, resize_to=48, want_crops=False)
    assert crops is None
    ref = np.stack([R.resize_linear_u8(c, (48, 48)) for c in small.crops])
    assert np.array_equal(rz.cpu().numpy(), ref)


def _raw(lib, frames, index, maps, valid, N, S, crops, cstride, rz, rstride, Rz):
    from ghost_amd import _lib
    F_, H, W = frames.shape[:3]
    return lib.ghost_align_crops_u8(frames.data_ptr(), H * W * 3, F_, H, W, index.data_ptr(), maps.data_ptr(),
                                    None if valid is None else valid.data_ptr(), N, S,
                                    None if crops is None else crops.data_ptr(), cstride,
                                    None if rz is None else rz.data_ptr(), rstride, Rz,
                                    _lib.stream_ptr(frames.device))


def _device_args(small):
    from ghost_amd.inference.blend import _invert_affine_cv
    maps = torch.from_numpy(np.stack([_invert_affine_cv(m) for m in small.tfms]).reshape(-1, 6)).to(DEV)
    index = torch.tensor(small.INDEX, dtype=torch.int32, device=DEV)
    return maps, index


@pytest.mark.parametrize("pad", [40, 13])      # dword-aligned rows (packed stores) and odd ones (byte stores)
def test_strided_outputs_and_valid_rows(small, pad):
    from ghost_amd import _lib
    lib = _lib.load()
    maps, index = _device_args(small)
    S, Rz, N = small.S, small.Rz, 7
    valid = torch.tensor([1, 0, 1, 1, 0, 1, 1], dtype=torch.int32, device=DEV)
    cs, rs = S * S * 3 + pad, Rz * Rz * 3 + pad
    cbuf = torch.full((N, cs), 0xA5, dtype=torch.uint8, device=DEV)
    rbuf = torch.full((N, rs), 0x5A, dtype=torch.uint8, device=DEV)
    assert _raw(lib, small.dev_frames, index, maps, valid, N, S, cbuf, cs, rbuf, rs, Rz) == 0
    c, r = cbuf.cpu().numpy(), rbuf.cpu().numpy()
    assert (c[:, S * S * 3:] == 0xA5).all() and (r[:, Rz * Rz * 3:] == 0x5A).all()      # the gaps of the view
    for n in range(N):
        if valid[n]:
            assert np.array_equal(c[n, :S * S * 3].reshape(S, S, 3), small.crops[n]), n
            assert np.array_equal(r[n, :Rz * Rz * 3].reshape(Rz, Rz, 3), small.rz[n]), n
        else:
            assert (c[n] == 0xA5).all() and (r[n] == 0x5A).all(), n


def test_align_crops_valid_argument(small):
    from ghost_amd.inference import align_crops
    valid = np.array([0, 1, 1, 0, 1, 1, 1])
    crops, _ = align_crops(small.dev_frames, small.tfms, small.INDEX, small.S, valid=valid)
    got = crops.cpu().numpy()
    assert np.array_equal(got[valid == 1], small.crops[valid == 1])


def test_workload_shape_224_to_256():
    from ghost_amd.inference import align_crops
    cases = [R.make_case(s) for s in (21, 22)]
    frames = np.stack([c[0] for c in cases])                        # [2,270,480,3]
    index = [1, 0, 1]
    tfms = np.stack([cases[1][3], cases[0][3], R.make_case(23)[3]]).astype(np.float64)
    ref_c, ref_r = _oracle(frames, tfms, index, 224, 256)
    crops, rz = align_crops(torch.from_numpy(frames).to(DEV), tfms, index, 224, resize_to=256)
    assert np.array_equal(crops.cpu().numpy(), ref_c)
    assert np.array_equal(rz.cpu().numpy(), ref_r)


def test_resize_matches_core_resize_frames():
    from ghost_amd.inference import align_crops
    from ghost_amd.inference.core import resize_frames
    f, _, _, M = R.make_case(31)
    M2 = R.make_case(32)[3]
    tfms = np.stack([M, M2]).astype(np.float64)
    host_crops = [R.warp_affine_cv(f, m, (224, 224), "constant") for m in tfms]
    want, present = resize_frames(host_crops, (256, 256), device=DEV)
    _, rz = align_crops(torch.from_numpy(f[None]).to(DEV), tfms, [0, 0], 224, resize_to=256, want_crops=False)
    assert present.tolist() == [1, 1] and torch.equal(rz, want)


def test_frame_offset_past_2_31():
    from ghost_amd.inference import align_crops
    frames = torch.empty(350, 1080, 1920, 3, dtype=torch.uint8, device=DEV)      # 2.18 GB, not initialised
    g = torch.Generator(device=DEV).manual_seed(5)
    frames[349] = torch.randint(0, 256, (1080, 1920, 3), dtype=torch.uint8, device=DEV, generator=g)
    last = frames[349].cpu().numpy()
    tfms = np.stack([_tfm(0.45, 0.15, 960.0, 540.0, 224), _tfm(1.3, -0.3, 1850.0, 1040.0, 224)])
    ref_c, ref_r = _oracle([last, last], tfms, [0, 1], 224, 256)
    crops, rz = align_crops(frames, tfms, [349, 349], 224, resize_to=256)
    assert np.array_equal(crops.cpu().numpy(), ref_c)
    assert np.array_equal(rz.cpu().numpy(), ref_r)


def test_crop_frames_and_get_transforms_single_target():
    from ghost_amd.inference import align, crop_frames_and_get_transforms
    g = np.random.Generator(np.random.PCG64(77))
    frames = g.integers(0, 256, size=(6, 96, 128, 3), dtype=np.uint8)
    templates = np.stack([FRONTAL * 2.0, FRONTAL * 2.0 + np.array([6.0, 0.0])])      # 224-sized, two poses
    base = FRONTAL * 0.4 + np.array([30.0, 15.0])
    drift = [0.0, 0.7, 1.1, None, 2.0, 9.5]          # frame 3 faceless; frame 5 jumps more than 5 px
    kps = [None if d is None else (base + d + g.normal(0, 0.2, size=(5, 2)))[None] for d in drift]
    target = torch.zeros(1, 512, device=DEV)
    target[0, 0] = 1.0
    crops, rz, present, tfm = crop_frames_and_get_transforms(torch.from_numpy(frames).to(DEV), kps, target, None, 224,
                                                             False, 0.15, templates)
    assert len(crops) == len(rz) == len(present) == len(tfm) == 1
    assert present[0].dtype == np.float64 and present[0].tolist() == [1, 1, 1, 0, 1, 1]
    smooth = align.smooth_landmarks([[[] if k is None else k[0] for k in kps]], n=2)[0]
    assert np.allclose(smooth[1], np.mean([kps[i][0] for i in range(3)], axis=0))     # frames 0-2 are one segment
    want_c, want_r, n = [], [], 0
    for i in range(6):
        if drift[i] is None:
            assert len(tfm[0][i]) == 0
            continue
        M = align.estimate_norm(smooth[i], 224, templates)[0]
        assert np.array_equal(tfm[0][i], M)
        c = R.warp_affine_cv(frames[i], M, (224, 224), "constant")
        want_c.append(c)
        want_r.append(R.resize_linear_u8(c, (256, 256)))
        n += 1
    assert crops[0].shape == (n, 224, 224, 3) and rz[0].shape == (n, 256, 256, 3)
    assert np.array_equal(crops[0].cpu().numpy(), np.stack(want_c))
    assert np.array_equal(rz[0].cpu().numpy(), np.stack(want_r))


def test_crop_face_is_the_first_face(small):
    from ghost_amd.inference import align, crop_face
    templates = FRONTAL[None] * 0.5
    kps = np.stack([FRONTAL * 0.6 + 20.0, FRONTAL * 0.3 + 5.0])
    out = crop_face(small.dev_frames[1], kps, 56, templates)
    M = align.estimate_norm(kps[0], 56, templates)[0]
    assert len(out) == 1
    assert np.array_equal(out[0].cpu().numpy(), R.warp_affine_cv(small.frames[1], M, (56, 56), "constant"))
    with pytest.raises(TypeError):
        crop_face(small.dev_frames[1], None, 56, templates)


def test_refused_before_any_launch(small):
    from ghost_amd.inference import align_crops
    with pytest.raises(IndexError):
        align_crops(small.dev_frames, small.tfms[:2], [0, 3], small.S)
    with pytest.raises(IndexError):
        align_crops(small.dev_frames, small.tfms[:2], [-1, 0], small.S)
    with pytest.raises(RuntimeError):
        align_crops(torch.from_numpy(small.frames), small.tfms[:1], [0], small.S)            # a CPU tensor
    with pytest.raises(RuntimeError):
        align_crops(small.dev_frames[:, :, ::2], small.tfms[:1], [0], small.S)               # not contiguous
    with pytest.raises(RuntimeError):
        align_crops(small.dev_frames.float(), small.tfms[:1], [0], small.S)                  # float frames


def test_raw_abi_rejects_bad_arguments(small):
    from ghost_amd import _lib
    lib = _lib.load()
    maps, index = _device_args(small)
    S, N = small.S, 7
    crops = torch.empty(N, S, S, 3, dtype=torch.uint8, device=DEV)
    rz = torch.empty(N, 64, 64, 3, dtype=torch.uint8, device=DEV)
    F_, H, W = small.frames.shape[:3]
    st = _lib.stream_ptr(torch.device(DEV))
    rc = lib.ghost_align_crops_u8(None, H * W * 3, F_, H, W, index.data_ptr(), maps.data_ptr(), None, N, S,
                                  crops.data_ptr(), S * S * 3, None, 0, 0, st)
    assert rc == -1 and b"null" in lib.ghost_last_error()                                    # GHOST_EINVAL
    assert _raw(lib, small.dev_frames, index, maps, None, N, S, None, 0, None, 0, 0) == -1   # no output at all
    assert b"null" in lib.ghost_last_error()
    for s_, r_ in [(S, 60), (S, 56), (50, 57)]:                                              # unsupported (S, R)
        assert _raw(lib, small.dev_frames, index, maps, None, N, s_, None, 0, rz, 64 * 64 * 3, r_) == -1
        assert b"fused resize" in lib.ghost_last_error()
    assert _raw(lib, small.dev_frames, index, maps, None, N, S, crops, S * S * 3 - 1, None, 0, 0) == -1
    assert b"bad sizes" in lib.ghost_last_error()
    assert _raw(lib, small.dev_frames, index, maps, None, 65536, S, crops, S * S * 3, None, 0, 0) == -1
    assert _raw(lib, small.dev_frames, index, maps, None, 0, S, crops, S * S * 3, None, 0, 0) == 0     # N == 0: OK


class _PixelArc:
    """Stands in for netArc: a crop's embedding is an 8 x 8 grid of its pixels, so equal crops match with cosine 1
    and crops of independent textures with about 0."""

    def embed_u8(self, crops):
        return crops[:, 14::28, 14::28, :].reshape(crops.shape[0], -1).float() - 127.5


def test_crop_frames_and_get_transforms_two_targets_matched_on_the_device():
    from ghost_amd.inference import align, crop_frames_and_get_transforms
    g = np.random.Generator(np.random.PCG64(91))
    tex = g.integers(0, 256, size=(2, 48, 48, 3), dtype=np.uint8)          # the two "faces"
    templates = FRONTAL[None] * 2.0                                         # crop = 5 (frame - offset)
    # per frame: top-left corner of each face's texture, in the order the detector lists them (None: faceless)
    layout = [[(0, (5, 10)), (1, (70, 30))], [(1, (72, 31)), (0, (6, 10))], [(0, (7, 11))], None,
              [(1, (71, 33)), (0, (8, 12))]]
    frames = np.zeros((len(layout), 96, 128, 3), np.uint8)
    kps = []
    for i, faces in enumerate(layout):
        if faces is None:
            kps.append(None)
            continue
        for who, (x, y) in faces:
            frames[i, y:y + 48, x:x + 48] = tex[who]
        kps.append(np.stack([FRONTAL * 0.4 + np.array([x + 1.0, y + 1.0]) for _, (x, y) in faces]))
    arc = _PixelArc()
    first = [R.warp_affine_cv(frames[0], align.estimate_norm(k, 224, templates)[0], (224, 224), "constant")
             for k in kps[0]]
    target = arc.embed_u8(torch.from_numpy(np.stack(first))).to(DEV)       # identity 0 = face 0, identity 1 = face 1
    crops, rz, present, tfm = crop_frames_and_get_transforms(torch.from_numpy(frames).to(DEV), kps, target, arc, 224,
                                                             False, 0.5, templates, embed_batch=4)
    # what the matching has to find: the position of each identity's face in the detector's list
    matches = {i: (np.array([[w for w, _ in layout[i]].index(q) for q in range(2)]), np.array([True, True]))
               for i in (0, 1, 4)}
    want_present, want_tfm = align.frame_transforms(align.select_keypoints(kps, 2, False, matches), 224, templates)
    assert want_present[0].tolist() == [1, 1, 1, 0, 1] and want_present[1].tolist() == [1, 1, 0, 0, 1]
    for q in range(2):
        assert present[q].tolist() == want_present[q].tolist()
        idx = [i for i in range(len(layout)) if want_present[q][i]]
        for i in range(len(layout)):
            assert np.array_equal(np.asarray(tfm[q][i]), np.asarray(want_tfm[q][i])), (q, i)
        ref_c, ref_r = _oracle(frames, [want_tfm[q][i] for i in idx], idx, 224, 256)
        assert np.array_equal(crops[q].cpu().numpy(), ref_c)
        assert np.array_equal(rz[q].cpu().numpy(), ref_r)
