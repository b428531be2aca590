"""Shared inputs of test_roi_packed_cpu.py and test_roi_packed_gpu.py (not a test module): hand-made rectangles on
3 frames of 96 x 128 and the packed layout restated in numpy."""
import numpy as np

H, W = 96, 128
WIDTHS = {1, 2, 3, 4, 5, 6, 7, 16, 21, 43, 128}
HEIGHTS = {1, 2, 5, 96}

# (x0, y0, w, h, frame): every width and height of the sets above, odd and even x0, edges touching x0 + w = W and
# y0 + h = H, two empty rectangles in the middle; the rectangles of one frame are disjoint
HAND = [(0, 0, 128, 96, 0),
        (0, 0, 1, 1, 1), (3, 0, 2, 2, 1), (8, 1, 3, 5, 1), (13, 0, 4, 1, 1), (20, 3, 5, 2, 1), (27, 0, 6, 5, 1),
        (0, 0, 1, 96, 2), (5, 0, 3, 96, 2),
        (36, 2, 7, 1, 1), (45, 0, 16, 2, 1), (63, 1, 21, 5, 1), (85, 0, 43, 5, 1),
        (10, 10, 0, 7, 1),                                         # empty: takes no bytes
        (0, 91, 43, 5, 1), (50, 94, 21, 2, 1), (107, 50, 21, 5, 1), (5, 20, 16, 5, 1), (31, 21, 4, 2, 1),
        (121, 0, 7, 96, 2), (9, 91, 5, 5, 2), (16, 94, 16, 2, 2),
        (4, 4, 5, 0, 2),                                           # empty
        (40, 10, 43, 5, 2), (85, 1, 21, 2, 2), (33, 95, 2, 1, 2), (100, 7, 6, 1, 2)]


def hand_rects():
    a = np.array(HAND, np.int32)
    return np.ascontiguousarray(a[:, :4]), np.ascontiguousarray(a[:, 4])


def frames(seed=77, n=3):
    """n frames of 96 x 128 without a 0xEE or 0xFF byte."""
    g = np.random.Generator(np.random.PCG64(seed))
    return g.integers(0, 0xEE, size=(n, H, W, 3), dtype=np.uint8)


def pitch(w):
    return (3 * int(w) + 15) & ~15


def layout_ref(rects):
    """The layout rule, restated: offsets int64 [Np] and the total."""
    offsets, off = [], 0
    for _, _, w, h in np.asarray(rects).tolist():
        offsets.append(off)
        if w > 0 and h > 0:
            off += pitch(w) * h
        off = (off + 255) & ~255
    return np.array(offsets, np.int64).reshape(-1), off


def packed_ref(rects, frame_of, offsets, total, src, fill=0xEE):
    """The packed buffer a pack of every rectangle leaves in a staging buffer prefilled with ``fill``."""
    out = np.full(total, fill, np.uint8)
    for (x0, y0, w, h), f, off in zip(np.asarray(rects).tolist(), frame_of, offsets):
        for y in range(h if w > 0 else 0):
            out[off + y * pitch(w):off + y * pitch(w) + 3 * w] = src[f][y0 + y, x0:x0 + w].reshape(-1)
    return out


def hand_plan():
    """A RoiPlan over the hand-made rectangles with the whole frame as canvas (nothing but the transfers uses it)."""
    from ghost_amd.inference.roi import RoiPlan
    rects, frame_of = hand_rects()
    return RoiPlan(rects, frame_of, np.full((1, 3), -1, np.int32), (H, W), np.zeros((1, 3, 2, 3)),
                   np.zeros((1, 3), bool), 56, (H, W), 2)
