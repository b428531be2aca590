"""Shared inputs of test_roi_cpu.py and test_roi_gpu.py (not a test module)."""
import numpy as np

S, H, W = 56, 96, 128

# (scale, angle, centre x, centre y): the seven transforms of tests/test_align_gpu.py::_Small
SMALL = [(0.9, 0.0, 64.0, 48.0),         # well inside the frame
         (2.7, 0.2, 50.3, 40.6),         # upsampling
         (0.35, -0.1, 60.0, 50.0),       # minification: the rectangle is the whole frame
         (1.0, 0.4, 70.2, 50.1),
         (1.0, -0.4, 55.7, 44.4),
         (1.0, 0.0, 118.0, 10.0),        # about half the crop is border
         (1.0, 0.1, -200.0, -300.0)]     # wholly outside: no rectangle
SMALL_FRAME = [2, 0, 0, 1, 2, 1, 0]


def tfm(scale, ang, cx, cy, size=S):
    """frame -> crop: crop = scale * Rot(ang) (frame - centre) + size/2, float64 as estimate_norm returns it."""
    c, s = scale * np.cos(ang), scale * np.sin(ang)
    return np.array([[c, -s, size / 2 - (c * cx - s * cy)], [s, c, size / 2 - (s * cx + c * cy)]], np.float64)


def small_tfms():
    return np.stack([tfm(*p) for p in SMALL])


def random_tfms(n=60, seed=7):
    """Scale 0.3-3, angle +-0.8, centres up to 20 px outside the 96 x 128 frame."""
    g = np.random.Generator(np.random.PCG64(seed))
    return np.stack([tfm(g.uniform(0.3, 3.0), g.uniform(-0.8, 0.8), g.uniform(-20.0, W + 20.0),
                         g.uniform(-20.0, H + 20.0)) for _ in range(n)])


def tfm_lists(per_identity, n_frames):
    """{frame: M} per identity -> the lists of M or [] that align.frame_transforms returns."""
    return [[d.get(i, []) for i in range(n_frames)] for d in per_identity]
