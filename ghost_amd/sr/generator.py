"""Drop-in for the reference's ``LIPSPADEGenerator`` (models/networks/generator.py:390), the network behind
``--use_sr`` (inference.py:42-50, utils/inference/video_processing.py:263-285), on MI355X.

``LIPSPADEGenerator(opt)`` keeps the reference's 230 ``state_dict`` keys, shapes and dtypes — the spectral-norm
``weight_orig / weight_u / weight_v`` triples, the never-called ``fc`` conv and the BatchNorm buffers (accepted,
never read) included — so ``load_state_dict(torch.load(path), strict=True)`` works.  Sub-modules only hold
parameters; their ``forward`` raises.

Execution (``forward``): every conv is ``ghost_conv2d_ex_nhwc`` on weights packed once per (device, dtype) by
``network/pack.py pack_conv``; the spectral norm's 1/sigma and the conv bias ride in that conv's epilogue
``scale`` / ``shift`` (no weight is re-packed per call), ``x_s + dx`` is its residual.  InstanceNorm / BatchNorm
statistics come from ``ghost_instnorm_stats_nhwc`` (batch statistics: the same entry with B = 1, HW = B*H*W), the
normalise-modulate-activate pass (with the nearest x2 upsample folded into its read) and the LIP pooling are the
two kernels of ``csrc/sr.hip``.

The reference runs this network in TRAIN mode (inference.py:48), and so does this module, whatever
``.train()`` / ``.eval()`` say:
* SPADE's BatchNorm uses the statistics of the call's own batch, so a row's output depends on the other rows of
  its batch (``face_enhancement``'s chunks of 20 are part of the semantics);
* ``power_iteration=True`` (default) runs one spectral-norm power iteration per conv_0 / conv_1 / conv_s per
  forward and updates ``weight_u / weight_v`` in place, as the reference does even under ``no_grad``.
  ``power_iteration=False`` computes sigma from the stored ``u``, ``v`` (torch's eval-mode value): the fast choice
  for a converged checkpoint, whose ``u`` is at its fixed point, and it makes repeated calls bit-identical.

fp32 parameters run the exact-fp32 path; ``compute_dtype=torch.bfloat16`` (or ``.half()`` / ``.bfloat16()``)
stores activations and weights in 16 bits with fp32 accumulation and fp32 statistics, as ``AEI_Net`` does.
There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from .._packed import _VERSION, PackedModule, WorkspaceCache
from ..network.pack import pack_conv, rup
from .config_sr import SUPPORTED

SN_EPS = 1e-12
# (attribute path, fin, fout, nearest x2 in front of the block)
_BLOCKS = [("head_0", 768, 768, False), ("G_middle_0", 768, 768, True), ("G_middle_1", 768, 768, False),
           ("ups.0", 768, 384, True), ("ups.1", 384, 192, True), ("ups.2", 192, 96, True), ("ups.3", 96, 48, True)]
_WS_BYTES = 64 << 20   # split-K partials of the low-resolution convs (<= 50 MB by the planner's bounds) / statistics


def _no_forward(name):
    def forward(self, *a, **k):
        raise NotImplementedError(f"ghost_amd: {name} runs inside LIPSPADEGenerator.forward on the MI355X path")
    return forward


class _Holder(nn.Sequential):
    forward = _no_forward("this container")


class _SNConv(nn.Module):
    """A spectral-normalised Conv2d as ``torch.nn.utils.spectral_norm`` leaves it in a state_dict."""

    def __init__(self, cin, cout, k, bias):
        super().__init__()
        if bias:
            self.bias = nn.Parameter(torch.zeros(cout))
        self.weight_orig = nn.Parameter(torch.empty(cout, cin, k, k))
        nn.init.xavier_normal_(self.weight_orig, gain=0.02)
        self.register_buffer("weight_u", F.normalize(torch.randn(cout), dim=0, eps=SN_EPS))
        self.register_buffer("weight_v", F.normalize(torch.randn(cin * k * k), dim=0, eps=SN_EPS))

    forward = _no_forward("a spectral-norm conv")


class SPADE(nn.Module):
    """models/networks/normalization.py:63-107: BN(x) * gamma(seg) + beta(seg)."""

    def __init__(self, norm_nc, label_nc=3):
        super().__init__()
        nh = 128 if norm_nc > 128 else norm_nc
        self.param_free_norm = nn.BatchNorm2d(norm_nc, affine=False)     # buffers kept for the keys; never read
        self.mlp_shared = _Holder(nn.Conv2d(label_nc, nh, 3, padding=1), nn.ReLU())
        self.mlp_gamma = nn.Conv2d(nh, norm_nc, 3, padding=1, bias=False)
        self.mlp_beta = nn.Conv2d(nh, norm_nc, 3, padding=1, bias=False)

    forward = _no_forward("SPADE")


class SPADEResnetBlock(nn.Module):
    """models/networks/architecture.py:21-70."""

    def __init__(self, fin, fout):
        super().__init__()
        self.learned_shortcut = fin != fout
        fmiddle = min(fin, fout)
        self.conv_0 = _SNConv(fin, fmiddle, 3, True)
        self.conv_1 = _SNConv(fmiddle, fout, 3, True)
        if self.learned_shortcut:
            self.conv_s = _SNConv(fin, fout, 1, False)
        self.norm_0 = SPADE(fin)
        self.norm_1 = SPADE(fmiddle)
        if self.learned_shortcut:
            self.norm_s = SPADE(fin)

    forward = _no_forward("SPADEResnetBlock")


class SimplifiedLIP(nn.Module):
    """models/networks/generator.py:327-351: logit = 12 sigmoid(IN_affine(conv3x3(x))), local-importance pooling."""

    def __init__(self, channels):
        super().__init__()
        self.logit = _Holder(nn.Conv2d(channels, channels, 3, padding=1, bias=False),
                             nn.InstanceNorm2d(channels, affine=True), nn.Sigmoid())

    forward = _no_forward("SimplifiedLIP")


class LIPEncoder(nn.Module):
    """models/networks/generator.py:353-388."""

    def __init__(self, ngf=48, n_2xdown=5):
        super().__init__()
        model = [nn.Conv2d(3, ngf, 3, padding=1, bias=False), nn.InstanceNorm2d(ngf), nn.ReLU()]
        cur = 1
        for i in range(n_2xdown):
            nxt = min(cur * 2, 16)
            model += [SimplifiedLIP(ngf * cur), nn.Conv2d(ngf * cur, ngf * nxt, 3, padding=1),
                      nn.InstanceNorm2d(ngf * nxt)]
            cur = nxt
            if i < n_2xdown - 1:
                model += [nn.ReLU(inplace=True)]
        self.model = _Holder(*model)

    forward = _no_forward("LIPEncoder")


class _ConvW:
    """One conv's packed weight and epilogue vectors."""

    def __init__(self, w, dt, bias=None):
        self.cout, self.cin, self.k = w.shape[0], w.shape[1], w.shape[2]
        self.w = pack_conv(w, dt).contiguous()
        self.npad, self.kpad = self.w.shape
        self.shift = None
        if bias is not None:
            self.shift = torch.zeros(self.npad, dtype=torch.float32, device=w.device)
            self.shift[:self.cout] = bias.float()
        self.scale = None      # spectral-norm convs: 1 / sigma, refreshed per call
        self.wmat = None       # fp32 [cout, cin k k] for the power iteration
        self.key = None


class _Runtime:
    """Packed weights of one (device, dtype)."""

    def __init__(self, sd, dt):
        self.dt = dt
        self.lib = _lib.load()
        c = self.convs = {}
        dev = sd["fc.weight"].device
        self.sn = []
        for name, fin, fout, _ in _BLOCKS:
            for cv in ("conv_0", "conv_1", "conv_s"):
                pre = f"{name}.{cv}"
                if f"{pre}.weight_orig" not in sd:
                    continue
                w = sd[f"{pre}.weight_orig"]
                cw = _ConvW(w, dt, sd.get(f"{pre}.bias"))
                cw.wmat = w.float().reshape(w.shape[0], -1).contiguous()
                cw.scale = torch.ones(cw.npad, dtype=torch.float32, device=dev)
                cw.key = pre
                c[pre] = cw
                self.sn.append(cw)
            for nm in ("norm_0", "norm_1", "norm_s"):
                pre = f"{name}.{nm}"
                if f"{pre}.mlp_gamma.weight" not in sd:
                    continue
                c[f"{pre}.shared"] = _ConvW(sd[f"{pre}.mlp_shared.0.weight"], dt, sd[f"{pre}.mlp_shared.0.bias"])
                # one conv whose rows are mlp_gamma then mlp_beta: gamma at channel c, beta at C + c
                c[f"{pre}.gb"] = _ConvW(torch.cat([sd[f"{pre}.mlp_gamma.weight"], sd[f"{pre}.mlp_beta.weight"]], 0), dt)
        c["rgb"] = _ConvW(sd["to_rgbs.3.weight"], dt, sd["to_rgbs.3.bias"])
        e = "lip_encoder.model"
        c["enc.0"] = _ConvW(sd[f"{e}.0.weight"], dt)
        self.lip_affine = []
        for i in range(5):
            c[f"enc.logit{i}"] = _ConvW(sd[f"{e}.{3 + 4 * i}.logit.0.weight"], dt)
            c[f"enc.conv{i}"] = _ConvW(sd[f"{e}.{4 + 4 * i}.weight"], dt, sd[f"{e}.{4 + 4 * i}.bias"])
            self.lip_affine.append((sd[f"{e}.{3 + 4 * i}.logit.1.weight"].float().contiguous(),
                                    sd[f"{e}.{3 + 4 * i}.logit.1.bias"].float().contiguous()))
        self.wsc = WorkspaceCache()   # stream -> workspace (stream-ordered reuse)
        self.ws = None
        self.frozen_sigma = False    # scale vectors hold the sigma of the stored u, v (power_iteration=False)


class LIPSPADEGenerator(PackedModule):
    """LIPSPADEGenerator(opt)  (models/networks/generator.py:27-63, 390-400)."""

    def __init__(self, opt=None, *, compute_dtype: Optional[torch.dtype] = None, power_iteration: bool = True):
        super().__init__()
        if opt is None:
            from .config_sr import TestOptions
            opt = TestOptions()
        for k, v in SUPPORTED.items():
            if getattr(opt, k, v) != v:
                raise NotImplementedError(f"ghost_amd: LIPSPADEGenerator supports only opt.{k} = {v!r} "
                                          f"(models/config_sr.py), got {getattr(opt, k)!r}")
        self.opt = opt
        self.compute_dtype = compute_dtype
        self.power_iteration = power_iteration
        nf = opt.ngf
        self.sw = self.sh = opt.crop_size // 32
        self.scale_ratio = 5
        self.fc = nn.Conv2d(opt.semantic_nc, 16 * nf, 3, padding=1)        # in the state_dict, never called
        self.head_0 = SPADEResnetBlock(16 * nf, 16 * nf)
        self.G_middle_0 = SPADEResnetBlock(16 * nf, 16 * nf)
        self.G_middle_1 = SPADEResnetBlock(16 * nf, 16 * nf)
        self.ups = nn.ModuleList([SPADEResnetBlock(16 * nf, 8 * nf), SPADEResnetBlock(8 * nf, 4 * nf),
                                  SPADEResnetBlock(4 * nf, 2 * nf), SPADEResnetBlock(2 * nf, 1 * nf)])
        self.to_rgbs = nn.ModuleList([nn.Conv2d(8 * nf, 3, 3, padding=1), nn.Conv2d(4 * nf, 3, 3, padding=1),
                                      nn.Conv2d(2 * nf, 3, 3, padding=1), nn.Conv2d(1 * nf, 3, 3, padding=1)])
        self.lip_encoder = LIPEncoder(nf, self.scale_ratio)
        self._init_packed()

    # -- weights -------------------------------------------------------------------
    def _dtype(self) -> torch.dtype:
        if self.compute_dtype is not None:
            if self.compute_dtype not in (torch.float32, torch.bfloat16, torch.float16):
                raise TypeError(f"ghost_amd: unsupported compute_dtype {self.compute_dtype}")
            return self.compute_dtype
        dt = self.to_rgbs[3].weight.dtype
        return dt if dt in (torch.float32, torch.float16) else torch.bfloat16

    def _runtime(self, device) -> _Runtime:
        dt = self._dtype()
        return self._cached_runtime(device, dt, lambda sd: _Runtime(sd, dt))

    def _sn_module(self, key) -> _SNConv:
        m = self
        for part in key.split("."):
            m = m[int(part)] if part.isdigit() else getattr(m, part)
        return m

    def _refresh_sigma(self, rt: _Runtime):
        """scale = 1 / sigma of every spectral-norm conv: a handful of device matrix-vector products, no host
        synchronisation.  With power_iteration one step v <- normalize(W^T u), u <- normalize(W v) first, written
        back to weight_u / weight_v (their version bump is absorbed: the pack does not depend on them)."""
        if not self.power_iteration and rt.frozen_sigma:
            return
        for cw in rt.sn:
            m = self._sn_module(cw.key)
            u, v = m.weight_u.detach().float(), m.weight_v.detach().float()
            if self.power_iteration:
                v = F.normalize(torch.mv(cw.wmat.t(), u), dim=0, eps=SN_EPS)
                u = F.normalize(torch.mv(cw.wmat, v), dim=0, eps=SN_EPS)
                m.weight_u.copy_(u)
                m.weight_v.copy_(v)
            sigma = torch.dot(u, torch.mv(cw.wmat, v))
            cw.scale[:cw.cout] = (1.0 / sigma).expand(cw.cout)
        rt.frozen_sigma = not self.power_iteration
        if self.power_iteration:
            self._rt_versions = tuple(map(_VERSION, self._rt_tensors))

    # -- launches ------------------------------------------------------------------
    @staticmethod
    def _conv(rt, x, cw, *, ldx=None, slope=1.0, res=None, res_first=0, tanh_out=0):
        B, H, W = x.shape[:3]
        y = torch.empty(B, H, W, cw.cout, dtype=rt.dt, device=x.device)
        e = _lib.ConvEpi()
        e.scale, e.shift, e.slope = _lib.ptr(cw.scale), _lib.ptr(cw.shift), slope
        if res is not None:
            e.res, e.ldres, e.res_first = res.data_ptr(), res.shape[-1], res_first
        e.tanh_out = tanh_out
        _lib.check(rt.lib.ghost_conv2d_ex_nhwc(_lib.gdtype(rt.dt), x.data_ptr(), B, H, W, cw.cin,
                                               ldx or x.shape[-1], cw.w.data_ptr(), cw.cout, cw.npad, cw.kpad, cw.k,
                                               cw.k, 1, cw.k // 2, C.byref(e), y.data_ptr(), cw.cout,
                                               rt.ws.data_ptr(), rt.ws.numel(), _lib.stream_ptr(x.device)),
                   "LIPSPADEGenerator conv")
        return y

    @staticmethod
    def _stats(rt, x, batch: bool):
        """[Bs][C][2] (mean, rstd): per sample, or (batch) one record over B*H*W — the same entry with B = 1."""
        B, H, W, Cn = x.shape
        bs, hw = (1, B * H * W) if batch else (B, H * W)
        stat = torch.empty(bs, Cn, 2, dtype=torch.float32, device=x.device)
        _lib.check(rt.lib.ghost_instnorm_stats_nhwc(_lib.gdtype(rt.dt), x.data_ptr(), bs, hw, Cn, Cn, stat.data_ptr(),
                                                    rt.ws.data_ptr(), rt.ws.numel(), _lib.stream_ptr(x.device)),
                   "LIPSPADEGenerator statistics")
        return stat

    @staticmethod
    def _modulate(rt, src, stat, gb, slope, up2x=False):
        B, H, W, Cn = src.shape
        if up2x:
            H, W = 2 * H, 2 * W
        out = torch.empty(B, H, W, Cn, dtype=rt.dt, device=src.device)
        _lib.check(rt.lib.ghost_norm_modulate_nhwc(_lib.gdtype(rt.dt), src.data_ptr(), Cn, B, H, W, Cn, stat.data_ptr(),
                                                   stat.shape[0], _lib.ptr(gb), 2 * Cn, slope, 1 if up2x else 0,
                                                   out.data_ptr(), Cn, _lib.stream_ptr(src.device)),
                   "LIPSPADEGenerator modulate")
        return out

    @staticmethod
    def _lip_pool(rt, x, logit, stat, w, b):
        B, H, W, Cn = x.shape
        out = torch.empty(B, H // 2, W // 2, Cn, dtype=rt.dt, device=x.device)
        _lib.check(rt.lib.ghost_lip_pool_nhwc(_lib.gdtype(rt.dt), x.data_ptr(), Cn, logit.data_ptr(), Cn, B, H, W, Cn,
                                              stat.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), Cn,
                                              _lib.stream_ptr(x.device)), "LIPSPADEGenerator lip_pool")
        return out

    def _spade(self, rt, pre, src, stat, seg, slope, up2x):
        actv = self._conv(rt, seg, rt.convs[f"{pre}.shared"], slope=0.0)
        gb = self._conv(rt, actv, rt.convs[f"{pre}.gb"])
        return self._modulate(rt, src, stat, gb, slope, up2x)

    # -- execution -----------------------------------------------------------------
    @torch.no_grad()
    def forward(self, input, seg=None):
        return self._forward(input, seg)[0]

    @torch.no_grad()
    def forward_taps(self, input, seg=None):
        """forward + {'enc': encoder output [B,768,8,8]} (NCHW view), the tap the parity tests gate."""
        return self._forward(input, seg)

    def _forward(self, x, seg):
        _lib.require_gpu(x, "LIPSPADEGenerator.forward")
        if x.ndim != 4 or tuple(x.shape[1:]) != (3, 256, 256):
            raise RuntimeError(f"ghost_amd: LIPSPADEGenerator expects [B,3,256,256], got {tuple(x.shape)}")
        if seg is None:
            seg = x
        _lib.require_same_device(seg, x.device, "seg")
        if tuple(seg.shape) != tuple(x.shape):
            raise RuntimeError(f"ghost_amd: seg must have the input's shape, got {tuple(seg.shape)}")
        rt = self._runtime(x.device)
        rt.ws = rt.wsc.get(_lib.stream_ptr(x.device), lambda: _WS_BYTES, x.device)
        self._refresh_sigma(rt)
        dt = rt.dt
        xin = x.permute(0, 2, 3, 1).to(dt).contiguous()
        sg = xin if seg is x else seg.permute(0, 2, 3, 1).to(dt).contiguous()
        # F.interpolate(seg, size, 'nearest') at these sizes is a strided slice
        segs = {256 // s: (sg if s == 1 else sg[:, ::s, ::s, :].contiguous()) for s in (1, 2, 4, 8, 16, 32)}
        cv = rt.convs
        # ---- LIP encoder: 256 -> 8, 48 -> 768
        h = self._conv(rt, xin, cv["enc.0"])
        h = self._modulate(rt, h, self._stats(rt, h, False), None, 0.0)
        for i in range(5):
            logit = self._conv(rt, h, cv[f"enc.logit{i}"])
            h = self._lip_pool(rt, h, logit, self._stats(rt, logit, False), *rt.lip_affine[i])
            h = self._conv(rt, h, cv[f"enc.conv{i}"])
            h = self._modulate(rt, h, self._stats(rt, h, False), None, 0.0 if i < 4 else 1.0)
        taps = {"enc": h.permute(0, 3, 1, 2)}
        # ---- SPADE decoder: 8 -> 256, 768 -> 48
        for name, fin, fout, up in _BLOCKS:
            if up and fin == fout:
                # G_middle_0's identity shortcut needs the upsampled tensor as the residual: the one materialised x2
                B, H, W, Cn = h.shape
                h = h[:, :, None, :, None, :].expand(B, H, 2, W, 2, Cn).reshape(B, 2 * H, 2 * W, Cn)
                up = False
            res = (2 * h.shape[1]) if up else h.shape[1]
            stat = self._stats(rt, h, True)       # of the source: a nearest x2 upsample has the same statistics
            if fin != fout:
                xs = self._conv(rt, self._spade(rt, f"{name}.norm_s", h, stat, segs[res], 1.0, up), cv[f"{name}.conv_s"])
            else:
                xs = h
            dx = self._conv(rt, self._spade(rt, f"{name}.norm_0", h, stat, segs[res], 0.2, up), cv[f"{name}.conv_0"])
            a1 = self._spade(rt, f"{name}.norm_1", dx, self._stats(rt, dx, True), segs[res], 0.2, False)
            if name == "ups.3":
                # to_rgbs[3] reads leaky_relu(x, 0.2): stored by this conv's epilogue, lrelu(x_s + dx)
                h = self._conv(rt, a1, cv[f"{name}.conv_1"], res=xs, res_first=1, slope=0.2)
            else:
                h = self._conv(rt, a1, cv[f"{name}.conv_1"], res=xs)
        y = self._conv(rt, h, cv["rgb"], tanh_out=1)
        return y.permute(0, 3, 1, 2), taps
