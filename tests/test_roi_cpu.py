"""Host geometry of the ROI video path (ghost_amd.inference.roi): the rectangle of a face covers everything
cv2.warpAffine reads and everything the paste-back may write, is tight, and plan_rois gives intersecting faces of one
frame one shared patch.  No GPU."""
import numpy as np
import pytest
import torch

import roi_cases as C
from oracle import blend_ref as R

MARGIN = 2


@pytest.fixture(scope="module")
def cases():
    from ghost_amd.inference import face_rois
    tfms = np.concatenate([C.small_tfms(), C.random_tfms()])
    return tfms, face_rois(tfms, C.S, (C.H, C.W), MARGIN)


def _outside(rect):
    x0, y0, w, h = (int(v) for v in rect)
    out = np.ones((C.H, C.W), bool)
    out[y0:y0 + h, x0:x0 + w] = False
    return out


def test_rectangle_covers_the_warp_and_the_paste_back(cases):
    tfms, rects = cases
    assert rects.dtype == np.int32 and rects.shape == (67, 4)
    frame = np.random.Generator(np.random.PCG64(5)).integers(1, 256, size=(C.H, C.W, 3), dtype=np.uint8)
    ones = np.ones((C.S, C.S), np.float32)
    swap = np.full((C.S, C.S, 3), 255, np.uint8)
    blank = np.zeros((C.H, C.W, 3), np.uint8)
    for n, (M, rect) in enumerate(zip(tfms, rects)):
        x0, y0, w, h = (int(v) for v in rect)
        assert 0 <= x0 and 0 <= y0 and x0 + w <= C.W and y0 + h <= C.H, n
        out = _outside(rect)
        cut = frame.copy()
        cut[out] = 0                                       # the warp reads nothing outside the rectangle
        assert np.array_equal(R.warp_affine_cv(cut, M, (C.S, C.S), "constant"),
                              R.warp_affine_cv(frame, M, (C.S, C.S), "constant")), n
        pasted = R.paste_back(blank, swap, ones, M.astype(np.float32))
        assert not pasted[out].any(), n                    # and the paste-back changes nothing outside it


def test_rectangle_is_tight(cases):
    from ghost_amd.inference.blend import _invert_affine_cv
    tfms, rects = cases
    corners = np.array([[-1.0, -1.0, 1.0], [C.S, -1.0, 1.0], [-1.0, C.S, 1.0], [C.S, C.S, 1.0]])
    slack = MARGIN + 2
    areas = []
    for n, (M, rect) in enumerate(zip(tfms, rects)):
        x0, y0, w, h = (int(v) for v in rect)
        if w == 0:
            continue
        p = corners @ _invert_affine_cv(M).T               # the real-valued preimage of [-1, S]^2
        bx0, by0 = np.clip(p.min(axis=0), [0, 0], [C.W - 1, C.H - 1])
        bx1, by1 = np.clip(p.max(axis=0), [0, 0], [C.W - 1, C.H - 1])
        assert x0 >= bx0 - slack and y0 >= by0 - slack and x0 + w - 1 <= bx1 + slack and y0 + h - 1 <= by1 + slack, n
        areas.append(w * h / (C.H * C.W))
    assert rects[2].tolist() == [0, 0, C.W, C.H]           # the minified face sees the whole frame
    assert np.mean(areas) < 0.5                            # and the others a fraction of it


def test_face_outside_the_frame_has_no_rectangle(cases):
    from ghost_amd.inference import face_rois
    assert cases[1][6].tolist() == [0, 0, 0, 0]
    far = np.stack([C.tfm(1.0, 0.3, 500.0, 48.0), C.tfm(1.5, -0.2, 64.0, -90.0)])
    assert face_rois(far, C.S, (C.H, C.W)).tolist() == [[0, 0, 0, 0]] * 2
    assert face_rois(np.zeros((0, 2, 3)), C.S, (C.H, C.W)).shape == (0, 4)
    # a transform that cannot be inverted tells nothing about where the face is: the whole frame
    assert face_rois(np.zeros((1, 2, 3)), C.S, (C.H, C.W)).tolist() == [[0, 0, C.W, C.H]]


def test_plan_rois_patches_and_merging():
    from ghost_amd.inference import face_rois, plan_rois
    a, b = C.tfm(2.0, 0.0, 25.0, 25.0), C.tfm(2.0, 0.1, 100.0, 70.0)           # two small faces far apart
    near = C.tfm(2.0, 0.0, 40.0, 30.0)                                          # overlaps a
    chain = [C.tfm(2.5, 0.0, 20.0 + 22.0 * k, 48.0) for k in range(3)]          # 0-1 and 1-2 overlap, 0-2 do not
    outside = C.tfm(1.0, 0.1, -200.0, -300.0)
    ra, rb, rn, ro = face_rois(np.stack([a, b, near, outside]), C.S, (C.H, C.W))
    rc = face_rois(np.stack(chain), C.S, (C.H, C.W))
    assert rc[0][0] + rc[0][2] <= rc[2][0] and rc[0][0] + rc[0][2] > rc[1][0] and rc[1][0] + rc[1][2] > rc[2][0]
    # frames: 0 disjoint pair, 1 overlapping pair, 2 the chain, 3 nobody, 4 only identity 1, 5 a face off the frame
    lists = C.tfm_lists([{0: a, 1: a, 2: chain[0], 5: outside}, {0: b, 1: near, 2: chain[2], 4: b}, {2: chain[1]}], 6)
    plan = plan_rois(lists, C.S, (C.H, C.W))
    po = plan.patch_of
    assert po.dtype == np.int32 and po.shape == (3, 6) and plan.rects.dtype == np.int32
    assert po[0, 0] >= 0 and po[1, 0] >= 0 and po[0, 0] != po[1, 0] and po[2, 0] == -1        # two patches
    assert plan.rects[po[0, 0]].tolist() == ra.tolist() and plan.rects[po[1, 0]].tolist() == rb.tolist()
    assert po[0, 1] == po[1, 1] >= 0                                                          # one shared union
    u = plan.rects[po[0, 1]]
    assert u[0] == min(ra[0], rn[0]) and u[1] == min(ra[1], rn[1])
    assert u[0] + u[2] == max(ra[0] + ra[2], rn[0] + rn[2]) and u[1] + u[3] == max(ra[1] + ra[3], rn[1] + rn[3])
    assert po[0, 2] == po[1, 2] == po[2, 2] >= 0                                              # transitively
    u = plan.rects[po[0, 2]]
    assert u[0] == rc[:, 0].min() and u[0] + u[2] == (rc[:, 0] + rc[:, 2]).max()
    assert (po[:, 3] == -1).all() and po[:, 4].tolist() == [-1, po[1, 4], -1] and po[1, 4] >= 0
    assert (po[:, 5] == -1).all() and plan.has_face[0, 5] and ro.tolist() == [0, 0, 0, 0]     # empty rectangle
    assert plan.n_patches == 5 and plan.frame.tolist() == [0, 0, 1, 2, 4] and plan.frame.dtype == np.int32
    Ph, Pw = plan.canvas
    assert Pw % 4 == 0 and Ph == plan.rects[:, 3].max() and Pw - 4 < plan.rects[:, 2].max() <= Pw
    # the patches of one frame are disjoint
    for i in range(6):
        rs = plan.rects[plan.frame == i]
        for j in range(len(rs)):
            for k in range(j + 1, len(rs)):
                p, q = rs[j], rs[k]
                assert p[0] + p[2] <= q[0] or q[0] + q[2] <= p[0] or p[1] + p[3] <= q[1] or q[1] + q[3] <= p[1]
    assert plan.frames_of(0).tolist() == [0, 1, 2, 5] and plan.link_bytes() == int((plan.rects[:, 2] * plan.rects[:, 3]).sum()) * 3
    empty = plan_rois([[[], []]], C.S, (C.H, C.W))
    assert empty.n_patches == 0 and empty.canvas == (0, 0) and empty.patch_of.tolist() == [[-1, -1]]


def test_refused_without_a_device():
    from ghost_amd.inference import (align_crops_roi, blend_swaps_roi, crop_frames_and_get_transforms_roi,
                                     download_rois, face_rois, plan_rois, upload_rois)
    M = C.tfm(2.0, 0.0, 25.0, 25.0)
    plan = plan_rois(C.tfm_lists([{0: M, 1: M}], 2), C.S, (C.H, C.W))
    frames = np.zeros((2, C.H, C.W, 3), np.uint8)
    for bad in (frames.astype(np.float32),                     # dtype
                frames[:, :, ::-1],                            # layout
                frames[:1],                                    # not the plan's frame count
                [frames[0], np.zeros((C.H + 2, C.W, 3), np.uint8)],        # frames of differing size
                [frames[0], frames[1, :, :, ::-1]],
                torch.zeros(2, C.H, C.W, 3),                   # a float tensor
                np.zeros((2, C.H, C.W, 4), np.uint8)):
        with pytest.raises(RuntimeError):
            upload_rois(bad, plan, "cuda:0")
    with pytest.raises(RuntimeError):
        upload_rois(frames, plan, "cpu")
    patches = torch.zeros(plan.n_patches, plan.canvas[0], plan.canvas[1], 3, dtype=torch.uint8)   # on the host
    with pytest.raises(RuntimeError):
        download_rois(patches, plan, frames)
    with pytest.raises(RuntimeError):
        align_crops_roi(patches, plan, 0, plan.tfms[0], C.S)
    with pytest.raises(RuntimeError):
        blend_swaps_roi(patches, plan, 0, torch.zeros(2, C.S, C.S, 3, dtype=torch.uint8), torch.zeros(2, C.S, C.S),
                        plan.tfms[0])
    with pytest.raises(RuntimeError):
        plan_rois([[M, []], [M]], C.S, (C.H, C.W))             # ragged
    with pytest.raises(RuntimeError):
        face_rois(np.zeros((3, 3, 3)), C.S, (C.H, C.W))
    with pytest.raises(RuntimeError):                          # one keypoint entry per frame
        crop_frames_and_get_transforms_roi(frames, [None], torch.zeros(1, 512), None, C.S, False, 0.15, None, "cuda:0")
