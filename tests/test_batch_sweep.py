"""Batch size is a free parameter of the product and nearly every launcher picks its kernel from it: the last batch
of a video is ``n mod BS``, the multi-identity and ROI paths batch whatever a chunk holds.  These tests walk every
batch size (AEI networks 1..64, ArcFace 1..256) with the native plan log on (include/ghost_amd.h ghost_plan_log:
one signature per launch naming the kernel variant and its edge classes, never the batch itself) and pin three
things:

* closure — the batch sizes of CHECKED_B / CHECKED_N select, between them, every plan any batch size selects.
  A retuned threshold that gives some other batch a plan of its own fails here, naming the signature and the
  smallest batch that shows it: rerun tools/plan_sweep.py and update the constants and DESIGN.md §2.
* row independence at every batch size — f(x[perm]) == f(x)[perm] bit for bit (same sums in the same order for a
  row wherever it sits in the batch): tails, short splits, paired and four-image tiles at odd batches.
* numerics at each checked batch size, with the gates the suite already has (tests/test_bf16_parity.py,
  tests/test_arcface.py, the fp32 bound of tests/test_gpu_parity.py) on rows [0, B // 2, B - 1]: the last row sits
  in the M tail.

The sets come from tools/plan_sweep.py (greedy set cover; 1, 60 and 64 always kept for the AEI networks).
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import aei_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

_spec = importlib.util.spec_from_file_location(
    "plan_sweep", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "plan_sweep.py"))
plan_sweep = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(plan_sweep)

CHECKED_B = {
    "unet2_bf16": [1, 2, 4, 11, 22, 60, 63, 64],
    "unet2_fp16": [1, 2, 4, 11, 22, 60, 63, 64],
    "unet2_fp32": [1, 11, 60, 63, 64],
    "linknet3_bf16": [1, 2, 4, 9, 10, 11, 22, 60, 63, 64],
    "resnet2_bf16": [1, 2, 5, 8, 16, 42, 60, 63, 64],
}
CHECKED_N = [1, 4, 12, 34, 96, 128, 165, 192, 256]
ARC_CHUNK = 32
ARC_CHUNKS = [range(a, a + ARC_CHUNK) for a in range(1, 257, ARC_CHUNK)]

_SWEPT = {}   # (config, batch) -> (signatures, rows_independent, finite)


def swept(config, sizes):
    """The sweep's records for ``sizes`` (each batch size runs once per session)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    todo = [n for n in sizes if (config, n) not in _SWEPT]
    for n, sigs, indep, finite in plan_sweep.sweep(config, todo, DEV):
        _SWEPT[(config, n)] = (sigs, indep, finite)
    return {n: _SWEPT[(config, n)] for n in sizes}


def assert_rows_independent(config, sizes):
    rec = swept(config, sizes)
    mixed = [n for n in sizes if not rec[n][1]]
    assert not mixed, f"{config}: a permuted batch does not give the permuted rows at batch sizes {mixed}"
    assert all(rec[n][2] for n in sizes), [n for n in sizes if not rec[n][2]]


def assert_closed(config, sizes, checked):
    rec = swept(config, sizes)
    assert set(checked) <= set(sizes)
    have = set().union(*[rec[n][0] for n in checked])
    missing = {}
    for n in sizes:                      # ascending: the smallest batch that shows a signature names it
        for s in rec[n][0] - have:
            missing.setdefault(s, n)
    assert not missing, (f"{config}: plans that no checked batch size {sorted(checked)} selects (signature: smallest "
                         f"batch): {missing}; rerun tools/plan_sweep.py")


# ------------------------------------------------------------------------------ AEI networks, B = 1..64
AEI_CHUNKS = [range(a, a + 8) for a in range(1, 65, 8)]


@pytest.mark.parametrize("chunk", AEI_CHUNKS, ids=lambda c: f"{c[0]}-{c[-1]}")
@pytest.mark.parametrize("config", list(plan_sweep.AEI_CONFIGS))
def test_aei_rows_independent_at_every_batch_size(config, chunk):
    assert_rows_independent(config, chunk)


@pytest.mark.parametrize("config", list(plan_sweep.AEI_CONFIGS))
def test_aei_checked_batches_select_every_plan(config):
    assert_closed(config, plan_sweep.AEI_SIZES, CHECKED_B[config])


# ------------------------------------------------------------------------------ ArcFace, N = 1..256
@pytest.mark.parametrize("chunk", ARC_CHUNKS, ids=lambda c: f"{c[0]}-{c[-1]}")
def test_arcface_rows_independent_at_every_batch_size(chunk):
    assert_rows_independent(plan_sweep.ARC_CONFIG, chunk)


def test_arcface_checked_batches_select_every_plan():
    assert_closed(plan_sweep.ARC_CONFIG, plan_sweep.ARC_SIZES, CHECKED_N)


# ------------------------------------------------------------------------------ numerics at the checked sizes
def _rows(B):
    return sorted({0, B // 2, B - 1})


def _cases16():
    for config, (backbone, nb, st) in plan_sweep.AEI_CONFIGS.items():
        if st != "fp32":
            for B in CHECKED_B[config]:
                yield pytest.param(backbone, nb, st, B, id=f"{config}-{B}")


@pytest.mark.parametrize("backbone,nb,st,B", list(_cases16()))
def test_aei_16bit_blocks_and_maps_at_checked_batches(backbone, nb, st, B):
    """Every decoder block, Y and its uint8 frame recomputed by the storage emulation from the GPU's own stored
    inputs (check_blocks), and the encoder maps against the emulation's (resnet: the relative gate)."""
    import test_bf16_parity as T
    r = T.compute(backbone, nb, B, _rows(B), st, fp32=backbone == "resnet")
    assert torch.isfinite(r["Y"]).all()
    T.check_blocks(r, backbone, nb, st)
    if backbone == "resnet":
        T.check_resnet_encoder_maps(r, st)
    else:
        T.check_encoder_maps(r, st)


@pytest.mark.parametrize("B", CHECKED_B["unet2_fp32"])
def test_aei_fp32_rows_at_checked_batches(B):
    """fp32: Y and the eight attribute maps of rows [0, B // 2, B - 1] against the oracle within 1e-3 (the bound of
    test_full_batch64_bf16_properties_and_fp32_rows)."""
    import test_gpu_parity as P
    G = P.model("unet", 2)
    xt, z = aei_ref.make_inputs(B, 11)
    Y, attr = G(xt.to(DEV), z.to(DEV))
    torch.cuda.synchronize()
    ri = torch.tensor(_rows(B))
    yr, ar = aei_ref.aei_forward(P.weights("unet", 2), xt[ri], z[ri])
    Yc = Y.cpu()
    assert torch.isfinite(Yc).all()
    err = (Yc[ri] - yr).abs().amax(dim=(1, 2, 3))
    assert float(err.max()) <= 1e-3, (ri[int(err.argmax())], float(err.max()))
    for k, (a, b) in enumerate(zip(attr, ar)):
        assert float((a[ri.to(DEV)].cpu() - b).abs().max()) <= 1e-3, k


@pytest.mark.parametrize("N", CHECKED_N)
def test_arcface_bf16_stages_at_checked_batches(N):
    """The per-stage teacher-forced gate of test_bf16_each_stage_matches_storage_emulation on rows [0, N - 1]."""
    import test_arcface as TA
    m = TA.net("iresnet100", compute_dtype=torch.bfloat16)
    TA.check_bf16_stages(m, "iresnet100", N, sorted({0, N - 1}))


# ------------------------------------------------------------------------------ the default batching end to end
def test_swap_identity_frames_default_batching_is_60_then_the_rest():
    """61 present frames with no BS argument: byte for byte G.swap_u8 of frames [0:60] and of [60:61]."""
    from ghost_amd.inference.core import swap_identity_frames
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    G = plan_sweep.aei_model("unet2_bf16", DEV)
    n = 61
    crops = aei_ref.make_u8_crops(n, seed=17)
    z = torch.randn(1, 512, generator=torch.Generator().manual_seed(9))
    final = swap_identity_frames(crops, [1] * n, z, G, device=DEV)
    cd, zd = torch.from_numpy(crops).to(DEV), z.to(DEV)
    want = torch.cat([G.swap_u8(cd[0:60], zd), G.swap_u8(cd[60:61], zd)]).cpu().numpy()
    assert len(final) == n
    got = np.stack([np.asarray(f) for f in final])
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want)
