"""Generate tests/golden/sr_lipspade_b2*.npz by running the REFERENCE face enhancer itself.

Runs only where /root/reference exists (the build container):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sr.py

What it does
* registers an empty stub module under the name ``torchvision`` (models/networks/architecture.py imports it for a
  VGG class the generator never builds) and imports ``LIPSPADEGenerator`` / ``TestOptions`` from the read-only
  reference; nothing is copied, only outputs are stored;
* puts the generator in train mode, as inference.py:48 does;
* checks its state_dict keys and shapes against ``tests/sr_ref.param_specs`` and loads the deterministic
  ``oracle.aei_ref.make_weights`` recipe (strict);
* runs TWO consecutive forwards on PCG64(7) U(0,1) input at B = 2 (the second sees the spectral-norm vectors the
  first one updated) and stores Y1, Y2, the u8 bytes of the restated post-processing, the full 8 x 8 encoder
  output, 4096-point samples + sums of every block output of the first call, and the key / shape list;
* asserts the run is non-degenerate.
"""
from __future__ import annotations

import os
import sys
import time
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from oracle import aei_ref, golden_io  # noqa: E402
import sr_ref  # noqa: E402

NAME = "sr_lipspade_b2"
SAMPLE = 4096


def tap_summary(name, a):
    a = a.detach().double()
    flat = a.reshape(-1)
    idx = np.linspace(0, flat.numel() - 1, SAMPLE).astype(np.int64)
    return {f"{name}_shape": np.array(a.shape, dtype=np.int64), f"{name}_sum": np.array(float(flat.sum())),
            f"{name}_abssum": np.array(float(flat.abs().sum())), f"{name}_idx": idx,
            f"{name}_sample": flat[idx].float().numpy()}


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference not present: golden vectors are regenerated only in the build container")
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))
    from models.config_sr import TestOptions
    from models.networks.generator import LIPSPADEGenerator
    torch.set_num_threads(min(os.cpu_count() or 8, 16))
    G = LIPSPADEGenerator(TestOptions())
    G.train()                                            # inference.py:48
    specs = sr_ref.param_specs()
    sd = G.state_dict()
    ref_keys = [(k, tuple(v.shape), str(v.dtype)) for k, v in sd.items()]
    mine = [(k, tuple(s), "torch.int64" if kind == "bn_nbt" else "torch.float32") for k, s, kind in specs]
    assert ref_keys == mine, "sr_ref.param_specs disagrees with the reference state_dict"
    G.load_state_dict(aei_ref.make_weights(specs), strict=True)

    taps = {}
    mods = {"enc": G.lip_encoder, "head_0": G.head_0, "G_middle_0": G.G_middle_0, "G_middle_1": G.G_middle_1}
    mods.update({f"ups.{i}": G.ups[i] for i in range(4)})
    def tap(n):
        def hook(_m, _i, o):                             # first call only; returns None (a value would replace o)
            if n not in taps:
                taps[n] = o.detach().clone()
        return hook
    hooks = [m.register_forward_hook(tap(n)) for n, m in mods.items()]
    x = sr_ref.make_input(2, seed=7)
    t0 = time.time()
    with torch.no_grad():
        y1 = G(x)
        y2 = G(x)
    dt = time.time() - t0
    for h in hooks:
        h.remove()

    assert float(y1.std()) > 0.05, float(y1.std())
    rec = {"batch": np.array(2), "seed": np.array(7), "Y1": y1.numpy().astype(np.float32),
           "Y2": y2.numpy().astype(np.float32), "U8": sr_ref.postprocess_u8(y1),
           "enc": taps["enc"].numpy().astype(np.float32),
           "keys": np.array([k for k, _, _ in specs]),
           "shapes": np.array([",".join(str(d) for d in s) for _, s, _ in specs])}
    for n in sr_ref.TAP_NAMES:
        assert float(taps[n].std()) > 0.01, (n, float(taps[n].std()))
        if n != "enc":
            rec.update(tap_summary(n.replace(".", "_"), taps[n]))
    files = golden_io.save(HERE, NAME, rec)
    print(f"{NAME}: 2 forwards {dt:.2f}s  std(Y1)={float(y1.std()):.4f}  max|Y1|={float(y1.abs().max()):.3f}  "
          f"max|Y2-Y1|={float((y2 - y1).abs().max()):.4f}  "
          f"tap std {min(float(t.std()) for t in taps.values()):.3f}..{max(float(t.std()) for t in taps.values()):.3f}  "
          f"-> {len(files)} files")


if __name__ == "__main__":
    main()
