"""CPU restatement of the SCRFD face detector (test infrastructure only; the product never imports it).

Written from a description of ``scrfd_10g_bnkps`` and of ``SCRFD.detect`` (insightface ``detection/scrfd`` on mmdet
2.x and ``insightface/model_zoo/scrfd.py``), which are recalled from the public sources, not verified: no ONNX file,
no onnxruntime and no insightface are available offline, so nothing here is a reference run.  torch for the network,
evaluated in float64; numpy float32 for ``detect``'s post-processing, which is float32 in insightface.

Network (NCHW; every conv has a bias; BatchNorm folded):
    stem    conv3x3/s2 3->28 +R, conv3x3 28->28 +R, conv3x3 28->56 +R, MaxPool 3x3/s2/p1
    stages  BasicBlocks, planes 56/88/88/224, 3/4/2/3 blocks, the first of stages 2-4 with stride 2:
            y = conv3x3(stride)+R -> conv3x3; out = ReLU(y + identity); identity at stride 2: AvgPool 2x2/s2 -> conv1x1
    PAFPN   56 channels on C3..C5: laterals 1x1, top-down nearest-x2 adds, 3x3 convs, bottom-up 3x3/s2 adds
            (sequential), P3 = inter_0, P4 = conv3x3(inter_1), P5 = conv3x3(inter_2); no activation
    heads   per stride 8/16/32: three conv3x3 +R to 80 channels, then cls 80->2 (sigmoid), reg 80->8 (times the
            level's bbox_scale), kps 80->20; 2 anchors per pixel, channel a*K + k belongs to anchor a

``store=`` emulates the 16-bit device path: every tensor the GPU path materialises in the storage type — each conv's
output (after bias, identity and ReLU), the pooled stem, the top-down sums — and every conv weight but the first stem
conv's and the cls / reg / kps convs' (the avg-down weight after its exact scaling) are rounded to that dtype; the
input, the biases, bbox_scale, the arithmetic in between and the nine output maps stay in the evaluation dtype.
"""
from __future__ import annotations

import zlib
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import blend_ref

PLANES = (56, 88, 88, 224)
BLOCKS = (3, 4, 2, 3)
STRIDES = (8, 16, 32)
TAP_NAMES = ["stem", "layer1", "layer4", "p3"]
NMS_THRESH = 0.4
# frame seeds of the end-to-end cases (make_frames): chosen on the CPU so that the restatement's sorted scores have a
# gap >= 4e-3 between ranks 8 and 20 (45 x 80, two frames: 8.1e-3; 80 x 45, one frame: 9.8e-3) and no pair's overlap
# lies within 1e-2 of the NMS threshold; seed 34 gives a second 45 x 80 frame without any candidate
E2E_SEED_45x80, E2E_SEED_80x45, NOFACE_SEED_45x80 = 26, 12, 34


def conv_units() -> List[Tuple[str, Tuple[int, int, int, int], bool]]:
    """(name, weight shape, followed directly by ReLU) of every conv unit in graph order."""
    u = [("backbone.stem.0", (28, 3, 3, 3), True), ("backbone.stem.3", (28, 28, 3, 3), True),
         ("backbone.stem.6", (56, 28, 3, 3), True)]
    cin = 56
    for st, (pl, nb) in enumerate(zip(PLANES, BLOCKS)):
        for b in range(nb):
            nm = f"backbone.layer{st + 1}.{b}"
            u.append((f"{nm}.conv1", (pl, cin, 3, 3), True))
            if st > 0 and b == 0:
                u.append((f"{nm}.downsample.1", (pl, cin, 1, 1), False))
            u.append((f"{nm}.conv2", (pl, pl, 3, 3), False))
            cin = pl
    u += [(f"neck.lateral_convs.{i}.conv", (56, PLANES[i + 1], 1, 1), False) for i in range(3)]
    u += [(f"neck.fpn_convs.{i}.conv", (56, 56, 3, 3), False) for i in range(3)]
    u += [(f"neck.downsample_convs.{i}.conv", (56, 56, 3, 3), False) for i in range(2)]
    u += [(f"neck.pafpn_convs.{i}.conv", (56, 56, 3, 3), False) for i in range(2)]
    for s in STRIDES:
        u += [(f"bbox_head.cls_stride_convs.{s}.{j}.conv", (80, 56 if j == 0 else 80, 3, 3), True) for j in range(3)]
        u += [(f"bbox_head.stride_cls.{s}", (2, 80, 3, 3), False), (f"bbox_head.stride_reg.{s}", (8, 80, 3, 3), False),
              (f"bbox_head.stride_kps.{s}", (20, 80, 3, 3), False)]
    return u


def param_specs() -> List[Tuple[str, Tuple[int, ...]]]:
    s: List[Tuple[str, Tuple[int, ...]]] = []
    for name, shape, _ in conv_units():
        s += [(f"{name}.weight", shape), (f"{name}.bias", (shape[0],))]
    return s + [(f"bbox_head.scales.{i}.scale", ()) for i in range(3)]


def _rng(name: str) -> np.random.Generator:
    return np.random.Generator(np.random.PCG64(zlib.crc32(name.encode())))


def make_weights() -> Dict[str, torch.Tensor]:
    """Every tensor from PCG64(crc32(name)), float32: convs followed by ReLU N(0, sqrt(2 / fan_in)), every other conv
    N(0, sqrt(0.5 / fan_in)), biases N(0, 0.1), bbox_scale U(0.5, 1.5)."""
    p: Dict[str, np.ndarray] = {}
    for name, shape, relu in conv_units():
        fan_in = shape[1] * shape[2] * shape[3]
        n = f"{name}.weight"
        p[n] = _rng(n).normal(0.0, np.sqrt((2.0 if relu else 0.5) / fan_in), shape)
        n = f"{name}.bias"
        p[n] = _rng(n).normal(0.0, 0.1, shape[0])
    for i in range(3):
        n = f"bbox_head.scales.{i}.scale"
        p[n] = _rng(n).uniform(0.5, 1.5, ())
    return {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in p.items()}


def make_frames(n: int, H: int, W: int, seed: int = 11) -> np.ndarray:
    """uint8 BGR [n,H,W,3]: smooth blobs over noise, so the resize has something to interpolate."""
    g = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n, H, W, 3), np.uint8)
    for i in range(n):
        img = g.uniform(0, 60, (H, W, 3))
        for _ in range(6):
            cy, cx, r = g.uniform(0, H), g.uniform(0, W), g.uniform(3, 12)
            img += g.uniform(40, 190, 3) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))[..., None]
        out[i] = np.clip(img, 0, 255).astype(np.uint8)
    return out


def gap_threshold(scores, lo: int = 8, hi: int = 20):
    """The midpoint of the widest gap between consecutive scores of ranks lo..hi (sorted descending, float64), and
    the gap."""
    s = np.sort(np.asarray(scores, np.float64).reshape(-1))[::-1]
    gaps = s[lo - 1:hi - 1] - s[lo:hi]
    k = int(np.argmax(gaps))
    return float((s[lo - 1 + k] + s[lo + k]) / 2), float(gaps[k])


def geometry(H: int, W: int, det_size) -> Tuple[int, int, float]:
    """SCRFD.detect's letterbox: (new_h, new_w, det_scale), Python floats truncated."""
    Wd, Hd = det_size
    im_ratio = float(H) / W
    model_ratio = float(Hd) / Wd
    if im_ratio > model_ratio:
        new_h = Hd
        new_w = int(new_h / im_ratio)
    else:
        new_w = Wd
        new_h = int(new_w * im_ratio)
    return new_h, new_w, float(new_h) / H


def letterbox(frames: np.ndarray, det_size) -> Tuple[np.ndarray, float]:
    """uint8 [n,H,W,3] -> the zero canvas [n,Hd,Wd,3] with cv2.resize's bytes top-left, and det_scale."""
    Wd, Hd = det_size
    new_h, new_w, scale = geometry(frames.shape[1], frames.shape[2], det_size)
    canvas = np.zeros((frames.shape[0], Hd, Wd, 3), np.uint8)
    for i, f in enumerate(frames):
        canvas[i, :new_h, :new_w] = blend_ref.resize_linear_u8(f, (new_w, new_h))
    return canvas, scale


def forward(p: Dict[str, torch.Tensor], canvas_u8, dtype=torch.float64, store: Optional[torch.dtype] = None):
    """canvas_u8 uint8 BGR [N,Hd,Wd,3] -> (the nine maps NCHW: cls x 3, reg x 3, kps x 3; {tap name: NCHW})."""
    rnd = (lambda t: t.to(store).to(dtype)) if store is not None else (lambda t: t)
    x = torch.as_tensor(canvas_u8).flip(-1).permute(0, 3, 1, 2).to(dtype)
    x = (x - 127.5) / 128.0

    def conv(name, x, stride=1, pad=1, relu=False, res=None, round_w=True, out_round=True):
        w = p[f"{name}.weight"].to(dtype)
        y = F.conv2d(x, rnd(w) if round_w else w, p[f"{name}.bias"].to(dtype), stride=stride, padding=pad)
        if res is not None:
            y = y + res
        if relu:
            y = F.relu(y)
        return rnd(y) if out_round else y

    taps = {}
    x = conv("backbone.stem.0", x, stride=2, relu=True, round_w=False)
    x = conv("backbone.stem.3", x, relu=True)
    x = conv("backbone.stem.6", x, relu=True)
    x = F.max_pool2d(x, 3, 2, 1)
    taps["stem"] = x
    feats = []
    for st, (pl, nb) in enumerate(zip(PLANES, BLOCKS)):
        for b in range(nb):
            nm = f"backbone.layer{st + 1}.{b}"
            s = 2 if st > 0 and b == 0 else 1
            y = conv(f"{nm}.conv1", x, stride=s, relu=True)
            idn = x
            if s == 2:
                idn = conv(f"{nm}.downsample.1", F.avg_pool2d(x, 2, 2), pad=0)
            x = conv(f"{nm}.conv2", y, relu=True, res=idn)
        if st == 0:
            taps["layer1"] = x
        else:
            feats.append(x)
    taps["layer4"] = x
    lat = [conv(f"neck.lateral_convs.{i}.conv", feats[i], pad=0) for i in range(3)]
    for i in (2, 1):
        lat[i - 1] = rnd(lat[i - 1] + F.interpolate(lat[i], scale_factor=2, mode="nearest"))
    inter = [conv(f"neck.fpn_convs.{i}.conv", lat[i]) for i in range(3)]
    for i in range(2):
        inter[i + 1] = conv(f"neck.downsample_convs.{i}.conv", inter[i], stride=2, res=inter[i + 1])
    P = [inter[0], conv("neck.pafpn_convs.0.conv", inter[1]), conv("neck.pafpn_convs.1.conv", inter[2])]
    taps["p3"] = P[0]
    cls, reg, kps = [], [], []
    for l, s in enumerate(STRIDES):
        t = P[l]
        for j in range(3):
            t = conv(f"bbox_head.cls_stride_convs.{s}.{j}.conv", t, relu=True)
        out = lambda name: conv(name, t, round_w=False, out_round=False)      # fp32 weights, fp32 maps
        cls.append(torch.sigmoid(out(f"bbox_head.stride_cls.{s}")))
        reg.append(out(f"bbox_head.stride_reg.{s}") * p[f"bbox_head.scales.{l}.scale"].to(dtype))
        kps.append(out(f"bbox_head.stride_kps.{s}"))
    return cls + reg + kps, taps


# ---- SCRFD.detect's post-processing, numpy float32 ----

def frame_maps(maps, f: int) -> List[np.ndarray]:
    """The nine NCHW maps of frame f as float32 anchor-major arrays: scores [A], boxes [A,4], keypoints [A,10] per
    level, anchor (y*Wl + x)*2 + a."""
    out = []
    for i, m in enumerate(maps):
        m = np.asarray(m[f].detach().cpu() if torch.is_tensor(m) else m[f]).astype(np.float32)
        K = m.shape[0] // 2
        out.append(np.ascontiguousarray(m.reshape(2, K, -1).transpose(2, 0, 1)).reshape(-1, K))
    return out


def nms(dets: np.ndarray, thresh: float = NMS_THRESH) -> List[int]:
    """insightface's SCRFD.nms on float32 dets [n,5] with the tie rule: equal scores by ascending index."""
    t = np.float32(thresh)
    x1, y1, x2, y2, scores = (dets[:, i] for i in range(5))
    one = np.float32(1.0)
    areas = (x2 - x1 + one) * (y2 - y1 + one)
    order = np.argsort(-scores, kind="stable")
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(int(i))
        xx1 = np.maximum(x1[i], x1[order[1:]])
        yy1 = np.maximum(y1[i], y1[order[1:]])
        xx2 = np.minimum(x2[i], x2[order[1:]])
        yy2 = np.minimum(y2[i], y2[order[1:]])
        w = np.maximum(np.float32(0.0), xx2 - xx1 + one)
        h = np.maximum(np.float32(0.0), yy2 - yy1 + one)
        inter = w * h
        with np.errstate(invalid="ignore", divide="ignore"):
            ovr = inter / (areas[i] + areas[order[1:]] - inter)
        inds = np.where(ovr <= t)[0]
        order = order[inds + 1]
    return keep


def min_ovr_margin(dets: np.ndarray, thresh: float = NMS_THRESH) -> float:
    """min |ovr - thresh| over all pairs of dets (float64 of the float32 arithmetic's inputs)."""
    d = dets.astype(np.float64)
    n = d.shape[0]
    if n < 2:
        return np.inf
    area = (d[:, 2] - d[:, 0] + 1) * (d[:, 3] - d[:, 1] + 1)
    w = np.maximum(0, np.minimum(d[:, None, 2], d[None, :, 2]) - np.maximum(d[:, None, 0], d[None, :, 0]) + 1)
    h = np.maximum(0, np.minimum(d[:, None, 3], d[None, :, 3]) - np.maximum(d[:, None, 1], d[None, :, 1]) + 1)
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        ovr = inter / (area[:, None] + area[None, :] - inter)
    m = np.abs(ovr - thresh)[~np.eye(n, dtype=bool)]
    m = m[np.isfinite(m)]
    return float(m.min()) if m.size else np.inf


def decode(fm: List[np.ndarray], det_size, thresh: float, det_scale: float):
    """Candidates of one frame in concatenated anchor order: (scores [n], boxes [n,4], kps [n,10], anchor index [n]),
    boxes and keypoints divided by float32(det_scale)."""
    Wd, Hd = det_size
    t = np.float32(thresh)
    S, B, K, I = [], [], [], []
    base = 0
    for l, s in enumerate(STRIDES):
        sc, rg, kp = fm[l][:, 0], fm[3 + l] * np.float32(s), fm[6 + l] * np.float32(s)
        Hl, Wl = Hd // s, Wd // s
        ac = np.stack(np.mgrid[:Hl, :Wl][::-1], axis=-1).astype(np.float32)
        ac = (ac * s).reshape(-1, 2)
        ac = np.stack([ac] * 2, axis=1).reshape(-1, 2)
        box = np.stack([ac[:, 0] - rg[:, 0], ac[:, 1] - rg[:, 1], ac[:, 0] + rg[:, 2], ac[:, 1] + rg[:, 3]], axis=-1)
        pts = np.stack([ac[:, i % 2] + kp[:, i] for i in range(10)], axis=-1)
        pos = np.where(sc >= t)[0]
        S.append(sc[pos]); B.append(box[pos]); K.append(pts[pos]); I.append(pos + base)
        base += sc.shape[0]
    ds = np.float32(det_scale)
    return (np.concatenate(S), (np.concatenate(B) / ds).astype(np.float32), (np.concatenate(K) / ds).astype(np.float32),
            np.concatenate(I).astype(np.int64))


def detect(fm: List[np.ndarray], det_size, thresh: float, det_scale: float, cap: int = 4096):
    """(det [k,5], kps [k,5,2], anchor index [k], number of candidates) of one frame, in kept order; past ``cap``
    candidates the first ``cap`` in anchor order are used."""
    sc, box, kp, idx = decode(fm, det_size, thresh, det_scale)
    n = sc.shape[0]
    sc, box, kp, idx = sc[:cap], box[:cap], kp[:cap], idx[:cap]
    dets = np.concatenate([box, sc[:, None]], axis=1).astype(np.float32)
    keep = nms(dets)
    return dets[keep], kp[keep].reshape(-1, 5, 2), idx[keep], n


def select_max_num(det: np.ndarray, max_num: int, H: int, W: int) -> np.ndarray:
    """SCRFD.detect's max_num rule: indices of the rows kept."""
    if max_num <= 0 or det.shape[0] <= max_num:
        return np.arange(det.shape[0])
    area = (det[:, 2] - det[:, 0]) * (det[:, 3] - det[:, 1])
    center = H // 2, W // 2
    offsets = np.vstack([(det[:, 0] + det[:, 2]) / 2 - center[1], (det[:, 1] + det[:, 3]) / 2 - center[0]])
    values = area - np.sum(np.power(offsets, 2.0), 0) * 2.0
    return np.argsort(values)[::-1][:max_num]
