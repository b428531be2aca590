"""Which kernel plans does each batch size select?  (the plan log: include/ghost_amd.h ghost_plan_log)

    python tools/plan_sweep.py                      # every configuration
    python tools/plan_sweep.py unet2_bf16 iresnet100_bf16
    python tools/plan_sweep.py --markdown           # the tables as DESIGN.md §2 holds them

For each configuration one ``swap_u8`` (ArcFace: ``embed_u8``) per batch size runs with the plan log on.  Printed:
the table signature -> batch sizes that select it, and a minimal set of batch sizes whose union covers every
signature (greedy set cover; the AEI sets always keep 1, 60 and 64: the smallest batch, ``swap_identity_frames``'
default and the benchmark's).  tests/test_batch_sweep.py holds the sets as CHECKED_B / CHECKED_N and fails when a
retuned heuristic makes a batch outside them select a plan none of them selects; rerun this tool then and update
both the constants and DESIGN.md.

The same sweep checks row independence on the way: swapping a permuted batch must give the permuted frames bit
for bit at every batch size (``sweep`` yields the verdict; the tests assert it).
"""
from __future__ import annotations

import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

# configuration -> (backbone, num_blocks, storage); storage "fp16" is a .half() module (inference.py:30)
AEI_CONFIGS = {
    "unet2_bf16": ("unet", 2, "bf16"),
    "unet2_fp16": ("unet", 2, "fp16"),
    "unet2_fp32": ("unet", 2, "fp32"),
    "linknet3_bf16": ("linknet", 3, "bf16"),
    "resnet2_bf16": ("resnet", 2, "bf16"),
}
ARC_CONFIG = "iresnet100_bf16"
AEI_SIZES = range(1, 65)
ARC_SIZES = range(1, 257)
AEI_KEEP = (1, 60, 64)


def aei_model(config: str, dev):
    from ghost_amd.network import AEI_Net
    from oracle import aei_ref
    backbone, nb, st = AEI_CONFIGS[config]
    p = aei_ref.make_weights(aei_ref.param_specs(backbone, nb))
    G = AEI_Net(backbone, num_blocks=nb, c_id=512, compute_dtype=torch.bfloat16 if st == "bf16" else None).eval()
    G.load_state_dict(p)
    G = G.to(dev)
    return G.half() if st == "fp16" else G


def arc_model(dev):
    from ghost_amd import arcface
    from oracle import arcface_ref as A
    m = arcface.iresnet100(fp16=False, compute_dtype=torch.bfloat16).eval()
    m.load_state_dict(A.make_weights(A.param_specs(A.LAYERS["iresnet100"])))
    return m.to(dev)


def _logged(fn):
    """fn() with the plan log on -> (result, the set of signatures it launched)."""
    from ghost_amd import _lib
    _lib.plan_log(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        _lib.plan_log(False)
    return out, frozenset(_lib.plan_log_read())


_RUNNERS = {}


def runner(config: str, dev):
    """f(idx) = the configuration's swap / embedding of rows ``idx`` of its fixed inputs (model and inputs built
    once per process)."""
    if (config, str(dev)) in _RUNNERS:
        return _RUNNERS[(config, str(dev))]
    top = max(ARC_SIZES if config == ARC_CONFIG else AEI_SIZES)
    if config == ARC_CONFIG:
        m = arc_model(dev)
        crops = torch.from_numpy(np.random.Generator(np.random.PCG64(12)).integers(
            0, 256, (top, 224, 224, 3), dtype=np.uint8)).to(dev)

        def f(idx):
            return m.embed_u8(crops[idx].contiguous())
    else:
        from oracle import aei_ref
        G = aei_model(config, dev)
        crops = torch.from_numpy(aei_ref.make_u8_crops(top, seed=31)).to(dev)
        z = torch.randn(top, 512, generator=torch.Generator().manual_seed(5)).to(dev)
        if AEI_CONFIGS[config][2] == "fp16":
            z = z.half()

        def f(idx):
            return G.swap_u8(crops[idx].contiguous(), z[idx].contiguous()).clone()
    _RUNNERS[(config, str(dev))] = f
    return f


def sweep(config: str, sizes, dev=None):
    """Yield (batch, signatures, rows_independent, finite) for each batch size of ``sizes``.
    rows_independent: f(x[perm]) == f(x)[perm] bit for bit, perm a fixed seeded permutation of the batch."""
    dev = torch.device(dev or "cuda:0")
    f = runner(config, dev)
    for n in sizes:
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(1000 + n)).to(dev)
        out, sigs = _logged(lambda: f(torch.arange(n, device=dev)))
        outp = f(perm)
        torch.cuda.synchronize()
        finite = bool(torch.isfinite(out).all()) if out.is_floating_point() else True
        yield n, sigs, bool(torch.equal(outp, out[perm])), finite


def table(by_batch: dict) -> dict:
    """{batch: signatures} -> {signature: sorted batches that select it}."""
    t = {}
    for n in sorted(by_batch):
        for s in by_batch[n]:
            t.setdefault(s, []).append(n)
    return t


def cover(by_batch: dict, keep=()) -> list:
    """Greedy set cover: batch sizes whose signatures together are every signature of the sweep.  ``keep`` first;
    then the batch adding the most uncovered signatures, the smallest such batch on a tie."""
    chosen = [n for n in keep if n in by_batch]
    covered = set().union(*[by_batch[n] for n in chosen]) if chosen else set()
    every = set().union(*by_batch.values())
    while covered != every:
        n = max(sorted(by_batch), key=lambda b: len(by_batch[b] - covered))
        chosen.append(n)
        covered |= by_batch[n]
    return sorted(chosen)


def ranges(ns) -> str:
    """[1, 2, 3, 7] -> '1-3, 7'; a run of three or more with another step d is 'a-b/d': [9, 11, 13] -> '9-13/2'."""
    out, i = [], 0
    while i < len(ns):
        j = i
        if i + 1 < len(ns):
            d = ns[i + 1] - ns[i]
            while j + 1 < len(ns) and ns[j + 1] - ns[j] == d:
                j += 1
        if j - i >= 2:
            out.append(f"{ns[i]}-{ns[j]}" + ("" if d == 1 else f"/{d}"))
            i = j + 1
        else:
            out.append(str(ns[i]))
            i += 1
    return ", ".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("configs", nargs="*", default=list(AEI_CONFIGS) + [ARC_CONFIG])
    ap.add_argument("--markdown", action="store_true", help="print the tables as DESIGN.md holds them")
    args = ap.parse_args()
    bad = 0
    for config in args.configs:
        arc = config == ARC_CONFIG
        by_batch = {}
        for n, sigs, indep, finite in sweep(config, ARC_SIZES if arc else AEI_SIZES):
            by_batch[n] = sigs
            if not (indep and finite):
                bad += 1
                print(f"!! {config} batch {n}: rows_independent={indep} finite={finite}", flush=True)
        report(config, by_batch, args.markdown)
    return 1 if bad else 0


def report(config: str, by_batch: dict, markdown: bool = False):
    """Print the table signature -> batch sizes and the chosen set of one configuration."""
    t = table(by_batch)
    chosen = cover(by_batch, () if config == ARC_CONFIG else AEI_KEEP)
    every = sorted(by_batch)
    n_all = sum(1 for ns in t.values() if ns == every)
    order = sorted(t, key=lambda s: (t[s][0], s))
    if markdown:
        print(f"\n**{config}** — {len(t)} signatures, {n_all} of them at every batch size; checked: `{chosen}`\n")
        print("| signature | batch sizes |\n|---|---|")
        for s in order:
            print(f"| `{s}` | {'all' if t[s] == every else ranges(t[s])} |")
    else:
        print(f"== {config}: {len(t)} signatures ({n_all} at every batch size)")
        for s in order:
            print(f"  {s}  <-  {'all' if t[s] == every else ranges(t[s])}")
        print(f"CHECKED {config} = {chosen}", flush=True)


if __name__ == "__main__":
    sys.exit(main())
