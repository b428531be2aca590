"""Edge cases of the implicit GEMM shared by the GPU op tests (tests/test_gpu_parity.py: the kernels' results and the
plan log of the launch) and the CPU plan tests (tests/test_conv_plan_cpu.py: the same tokens from ghost_conv_plan).

Edge classes that no pipeline batch selects but the public conv entries accept: M and N tails, ragged / one-step /
clamped split-K, a last split shorter than the ring's prologue, both reduction forms, the non-FAST gather with 16-bit
operands.  split_k > 0 keeps a conv off the halo and patch kernels.  If a retuned heuristic moves a case to another
variant, change the shape, not the class.
"""

IGEMM_EDGES = [
    # cin, ldx, cout, k, s, p, B, H, W, split_k, plan tokens (GEMM launch), reduction kernel
    # glds 64x128, 3 stages, M = 120 (tail), non-square; nk = 27: splits 7,7,7,6 / one K step each / clamped to nk
    (96, 96, 128, 3, 1, 1, 2, 6, 10, 4, ("glds", "64x128", "stages=3", "split=1", "ragged=1", "short=0", "mtail=1"),
     "splitk_reduce4"),
    (96, 96, 128, 3, 1, 1, 2, 6, 10, 27, ("glds", "64x128", "stages=3", "split=1", "ragged=0", "short=1", "mtail=1"),
     "splitk_reduce4"),
    (96, 96, 128, 3, 1, 1, 2, 6, 10, 100, ("glds", "64x128", "stages=3", "split=1", "ragged=0", "short=1", "mtail=1"),
     "splitk_reduce4"),
    # N tail: Cout 200 reduces four channels at a time, Cout 130 one
    (64, 64, 200, 3, 1, 1, 3, 5, 7, 2, ("glds", "64x128", "split=1", "ntail=1", "mtail=1"), "splitk_reduce4"),
    (64, 64, 130, 3, 1, 1, 3, 5, 7, 2, ("glds", "64x128", "split=1", "ntail=1", "mtail=1"), "splitk_reduce"),
    # deep ring 128x128 x 8 stages; nk = 36: splits 8,8,8,8,4 (the last shorter than STAGES - 1) / one K step each
    (128, 128, 256, 3, 1, 1, 2, 8, 8, 5, ("glds", "128x128", "stages=8", "split=1", "ragged=1", "lastshort=1",
                                          "mtail=0"), "splitk_reduce4"),
    (128, 128, 256, 3, 1, 1, 3, 5, 7, 5, ("glds", "128x128", "stages=8", "split=1", "ragged=1", "lastshort=1",
                                          "mtail=1"), "splitk_reduce4"),
    (128, 128, 256, 3, 1, 1, 2, 8, 8, 36, ("glds", "128x128", "stages=8", "split=1", "short=1", "mtail=0"),
     "splitk_reduce4"),
    (128, 128, 256, 3, 1, 1, 3, 5, 7, 36, ("glds", "128x128", "stages=8", "split=1", "short=1", "mtail=1"),
     "splitk_reduce4"),
    # the encoder's 4x4/s2 tile on the ring
    (32, 32, 64, 4, 2, 1, 1, 12, 20, 2, ("glds", "128x64", "split=1", "mtail=1"), "splitk_reduce4"),
    # register-staged kernel, 256x32 tile, 16-bit split
    (64, 64, 24, 3, 1, 1, 2, 9, 5, 3, ("igemm", "256x32x32", "fast=1", "epi=SPLIT", "split=1", "ntail=1", "mtail=1"),
     "splitk_reduce4"),
    # 1x1/s2 (nk = 5): unsplit and one K step per split
    (160, 160, 96, 1, 2, 0, 2, 10, 6, 0, ("glds", "64x128", "split=0", "ntail=1", "mtail=1"), None),
    (160, 160, 96, 1, 2, 0, 2, 10, 6, 5, ("glds", "64x128", "split=1", "short=1", "ntail=1", "mtail=1"),
     "splitk_reduce4"),
    # the non-FAST gather (Cin % 32 != 0, padded input channels) with 16-bit operands
    (20, 24, 70, 3, 1, 1, 2, 7, 6, 0, ("igemm", "64x64x32", "fast=0", "split=0", "ntail=1", "mtail=1"), None),
]
IGEMM_LDY_PAD = 8       # test_igemm_edge_plans writes into ldy = cout + 8

# ConvT 4x4/s2 544 -> Cout at B = 1, 4 x 6 (M = 24 per parity class, nk = 68): the heuristic's 8 splits are seven of
# 9 K steps and a last of 5; every case reduces with splitk_reduce4
CONVT_CIN, CONVT_H, CONVT_W = 544, 4, 6
CONVT_LDY_PAD = 32      # test_convT_igemm_edge_plans writes into ldy = cout + 32
CONVT_EDGES = [
    (64, ("igemm", "256x64x32", "kind=T4S2", "split=1", "ragged=1", "mtail=1")),
    (128, ("glds", "64x128", "kind=T4S2", "split=1", "ragged=1", "mtail=1")),
]


def gemm_tokens(plan, t):
    """The tokens the GEMM line must hold for storage type name ``t`` ("bf16" / "f16")."""
    return plan + ("t=" + t,) if plan[0] == "glds" else plan
