"""CPU restatement of the use_sr face enhancer (test infrastructure only; the product never imports it).

The network is the reference's ``LIPSPADEGenerator(TestOptions())`` (models/networks/generator.py:390,
models/config_sr.py: netG 'lipspade', ngf 48, semantic_nc 3, crop 256, 'normal' upsampling,
norm_G 'spectralspadesyncbatch3x3') as ``inference.py:48`` runs it: in train mode.  Written with
``torch.nn.functional`` from the network's description; parity is pinned by ``tests/golden/make_golden_sr.py``,
which runs the reference itself and stores its outputs (``tests/test_sr_cpu.py`` compares).

Train mode means
* every SPADE normalises with the statistics of the call's own batch (mean and biased variance per channel over
  B*H*W, eps 1e-5); running statistics are never read;
* every forward runs one spectral-norm power iteration on conv_0 / conv_1 / conv_s, also under no_grad:
  v <- normalize(W^T u), u <- normalize(W v) (eps 1e-12), sigma = u . W v; the conv uses W / sigma and u, v are
  updated in place.

``store=`` emulates the 16-bit device path: every tensor the GPU path materialises (conv outputs after their
epilogue, modulate and pool outputs, 16-bit weights) is rounded to that dtype, arithmetic in between stays fp32.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

NGF = 48
EPS = 1e-5
SN_EPS = 1e-12
LIP_COEFF = 12.0
ENC_CH = [NGF, 2 * NGF, 4 * NGF, 8 * NGF, 16 * NGF, 16 * NGF]          # 48 .. 768, 768
# (name, fin, fout, nearest x2 in front of it)
BLOCKS = [("head_0", 768, 768, False), ("G_middle_0", 768, 768, True), ("G_middle_1", 768, 768, False),
          ("ups.0", 768, 384, True), ("ups.1", 384, 192, True), ("ups.2", 192, 96, True), ("ups.3", 96, 48, True)]
TAP_NAMES = ["enc"] + [b[0] for b in BLOCKS]


def nhidden(c: int) -> int:
    return 128 if c > 128 else c


def param_specs() -> List[Tuple[str, Tuple[int, ...], str]]:
    """Ordered (key, shape, kind) of the generator's state_dict; kind is the ``oracle.aei_ref.make_weights`` recipe:
    conv for 4-D tensors, BN kinds for the LIP affine and the BatchNorm buffers, bias for biases and weight_u/_v."""
    s: List[Tuple[str, Tuple[int, ...], str]] = [("fc.weight", (16 * NGF, 3, 3, 3), "conv"), ("fc.bias", (16 * NGF,), "bias")]

    def sn_conv(pre, co, ci, k, bias):
        if bias:
            s.append((f"{pre}.bias", (co,), "bias"))
        s.extend([(f"{pre}.weight_orig", (co, ci, k, k), "conv"), (f"{pre}.weight_u", (co,), "bias"),
                  (f"{pre}.weight_v", (ci * k * k,), "bias")])

    def spade(pre, c):
        nh = nhidden(c)
        s.extend([(f"{pre}.param_free_norm.running_mean", (c,), "bn_rm"),
                  (f"{pre}.param_free_norm.running_var", (c,), "bn_rv"),
                  (f"{pre}.param_free_norm.num_batches_tracked", (), "bn_nbt"),
                  (f"{pre}.mlp_shared.0.weight", (nh, 3, 3, 3), "conv"), (f"{pre}.mlp_shared.0.bias", (nh,), "bias"),
                  (f"{pre}.mlp_gamma.weight", (c, nh, 3, 3), "conv"), (f"{pre}.mlp_beta.weight", (c, nh, 3, 3), "conv")])

    for name, fin, fout, _ in BLOCKS:
        fm = min(fin, fout)
        sn_conv(f"{name}.conv_0", fm, fin, 3, True)
        sn_conv(f"{name}.conv_1", fout, fm, 3, True)
        if fin != fout:
            sn_conv(f"{name}.conv_s", fout, fin, 1, False)
        spade(f"{name}.norm_0", fin)
        spade(f"{name}.norm_1", fm)
        if fin != fout:
            spade(f"{name}.norm_s", fin)
    for i, c in enumerate([8 * NGF, 4 * NGF, 2 * NGF, NGF]):
        s.extend([(f"to_rgbs.{i}.weight", (3, c, 3, 3), "conv"), (f"to_rgbs.{i}.bias", (3,), "bias")])
    s.append(("lip_encoder.model.0.weight", (NGF, 3, 3, 3), "conv"))
    for i in range(5):
        c, cn = ENC_CH[i], ENC_CH[i + 1]
        s.extend([(f"lip_encoder.model.{3 + 4 * i}.logit.0.weight", (c, c, 3, 3), "conv"),
                  (f"lip_encoder.model.{3 + 4 * i}.logit.1.weight", (c,), "bn_w"),
                  (f"lip_encoder.model.{3 + 4 * i}.logit.1.bias", (c,), "bn_b"),
                  (f"lip_encoder.model.{4 + 4 * i}.weight", (cn, c, 3, 3), "conv"),
                  (f"lip_encoder.model.{4 + 4 * i}.bias", (cn,), "bias")])
    return s


def make_input(batch: int, seed: int = 7) -> torch.Tensor:
    """x ~ U(0,1) [B,3,256,256] from PCG64(seed)."""
    import numpy as np
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(g.uniform(0.0, 1.0, size=(batch, 3, 256, 256)).astype(np.float32))


def power_iteration(w: torch.Tensor, u: torch.Tensor, v: torch.Tensor, iterate: bool = True):
    """One spectral-norm step on W = w.reshape(Cout, -1) -> (sigma, u', v'); iterate=False: sigma from the stored u, v."""
    m = w.reshape(w.shape[0], -1)
    if iterate:
        v = F.normalize(torch.mv(m.t(), u), dim=0, eps=SN_EPS)
        u = F.normalize(torch.mv(m, v), dim=0, eps=SN_EPS)
    return torch.dot(u, torch.mv(m, v)), u, v


def batch_stats(x: torch.Tensor):
    var, mean = torch.var_mean(x, dim=(0, 2, 3), unbiased=False, keepdim=True)
    return mean, torch.rsqrt(var + EPS)


def lip_pool(x: torch.Tensor, logit: torch.Tensor) -> torch.Tensor:
    """sum3x3 x e^l / sum3x3 e^l at stride 2, pad 1 (padding taps are zero in both sums, so avg_pool's /9 cancels)."""
    w = logit.exp()
    return F.avg_pool2d(x * w, 3, 2, 1) / F.avg_pool2d(w, 3, 2, 1)


def postprocess_u8(y: torch.Tensor):
    """face_enhancement's output step: clamp(Y * 255, 0, 255) truncated to uint8, RGB -> BGR, NHWC."""
    t = (y.permute(0, 2, 3, 1) * 255.0).clamp(0, 255)
    return t[..., [2, 1, 0]].to(torch.uint8).numpy()


@torch.no_grad()
def sr_forward(p: Dict[str, torch.Tensor], x: torch.Tensor, power_iteration_step: bool = True,
               store: Optional[torch.dtype] = None, taps: Optional[dict] = None) -> torch.Tensor:
    """LIPSPADEGenerator.forward(x) (seg = x) in train mode.  ``p`` is the state_dict; with power_iteration_step its
    weight_u / weight_v entries are replaced by the iterated vectors (the reference updates them in place).
    taps (optional dict) receives the encoder output and every block output by TAP_NAMES."""
    q = (lambda t: t) if store is None else (lambda t: t.to(store).float())
    x = q(x.float())
    seg = x

    def sn_conv(h, pre, pad, res=None, slope=1.0):
        w = p[f"{pre}.weight_orig"].float()
        sigma, u, v = power_iteration(w, p[f"{pre}.weight_u"].float(), p[f"{pre}.weight_v"].float(),
                                      power_iteration_step)
        if power_iteration_step:
            p[f"{pre}.weight_u"], p[f"{pre}.weight_v"] = u, v
        y = F.conv2d(h, q(w), None, padding=pad) * (1.0 / sigma)
        if f"{pre}.bias" in p:
            y = y + p[f"{pre}.bias"].float().view(1, -1, 1, 1)
        if res is not None:
            y = y + res
        return q(F.leaky_relu(y, slope) if slope != 1.0 else y), y

    def spade(h, pre, slope):
        s = seg.shape[-1] // h.shape[-1]
        sg = seg[:, :, ::s, ::s]
        actv = q(F.relu(F.conv2d(sg, q(p[f"{pre}.mlp_shared.0.weight"].float()),
                                 p[f"{pre}.mlp_shared.0.bias"].float(), padding=1)))
        wgb = torch.cat([p[f"{pre}.mlp_gamma.weight"], p[f"{pre}.mlp_beta.weight"]], 0).float()
        gb = q(F.conv2d(actv, q(wgb), None, padding=1))
        c = h.shape[1]
        mean, rstd = batch_stats(h)
        out = (h - mean) * rstd * gb[:, :c] + gb[:, c:]
        return q(F.leaky_relu(out, slope) if slope != 1.0 else out)

    # ---- encoder
    e = "lip_encoder.model"
    h = q(F.conv2d(x, q(p[f"{e}.0.weight"].float()), None, padding=1))
    h = q(F.relu(F.instance_norm(h, eps=EPS)))
    for i in range(5):
        lr = q(F.conv2d(h, q(p[f"{e}.{3 + 4 * i}.logit.0.weight"].float()), None, padding=1))
        logit = LIP_COEFF * torch.sigmoid(F.instance_norm(lr, weight=p[f"{e}.{3 + 4 * i}.logit.1.weight"].float(),
                                                          bias=p[f"{e}.{3 + 4 * i}.logit.1.bias"].float(), eps=EPS))
        h = q(lip_pool(h, logit))
        h = q(F.conv2d(h, q(p[f"{e}.{4 + 4 * i}.weight"].float()), p[f"{e}.{4 + 4 * i}.bias"].float(), padding=1))
        h = F.instance_norm(h, eps=EPS)      # biased variance, per sample and channel
        h = q(F.relu(h) if i < 4 else h)
    if taps is not None:
        taps["enc"] = h
    # ---- decoder
    for name, fin, fout, up in BLOCKS:
        if up:
            h = F.interpolate(h, scale_factor=2, mode="nearest")
        xs = h
        if fin != fout:
            xs = sn_conv(spade(h, f"{name}.norm_s", 1.0), f"{name}.conv_s", 0)[0]
        dx = sn_conv(spade(h, f"{name}.norm_0", 0.2), f"{name}.conv_0", 1)[0]
        # the last block's conv_1 stores lrelu(x_s + dx): only to_rgbs[3] reads it (the tap is the block output
        # x_s + dx itself, unrounded there)
        last = name == "ups.3"
        h, pre = sn_conv(spade(dx, f"{name}.norm_1", 0.2), f"{name}.conv_1", 1, res=xs, slope=0.2 if last else 1.0)
        if taps is not None:
            taps[name] = pre if last else h
    y = F.conv2d(h, q(p["to_rgbs.3.weight"].float()), p["to_rgbs.3.bias"].float(), padding=1)
    return q(torch.tanh(y))
