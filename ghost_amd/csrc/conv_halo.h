// ghost_amd — halo-tiled 3x3/s1/p1 convolution (bf16, Cin % 32 == 0, N % 64 == 0).
#pragma once
#include <hip/hip_runtime.h>

#include "conv_igemm.h"

namespace ghost {

// ---- the 3x3 halo family's plan: everything conv3x3_halo launches, decided once from the descriptor ----
enum class HaloKernel { None, Halo, HaloPP };        // conv3x3_halo_kernel, the persistent conv3x3_halo_pp_kernel
// Wide: exact 16 x 32 tiles.  Small: 16 x 16 tiles that may overhang the image by up to a quarter of their pixels.
// Img8: four whole 8 x 8 images per tile.  Pair: a 16 x 16 window of two samples.
enum class HaloTile { Wide, Small, Img8, Pair };

struct HaloPlan {
  HaloKernel kernel = HaloKernel::None;   // None: conv3x3_halo does not take the descriptor
  HaloTile tile = HaloTile::Wide;
  bool resw = false, stats = false;       // HaloPP: weights resident (64 -> 64), InstanceNorm partials (d.in_part)
  int ncb = 0;                            // HaloPP: 32-channel blocks of the reduction
  int tiles_x = 0, tiles_y = 0, ntiles = 0;   // ntiles: work items, (tile, 64-channel block)
  unsigned grid = 0, block = 0;
  int nrec = 0;   // InstanceNorm-partial records per (sample, channel) the kernel can write (0: it writes none)
};

// pure: reads the descriptor's integers and flags, which pointers are set and their alignment; no HIP call.
// ncu (the device's compute units) sizes the persistent grid and decides Small against Pair, nothing else; kernel,
// tile and nrec do not depend on d.in_part, so a caller may ask before it allocates the partials.
HaloPlan halo_plan(const ConvDesc& d, int ncu);
PlanSig halo_signature(const HaloPlan& p, const ConvDesc& d);   // the plan-log line of (plan, desc)

// true when conv3x3_halo takes this descriptor (3x3/s1/p1, bf16, standard epilogue without the
// uint8 copy — PReLU / residual-first / second BN'd output allowed —, K ordered (channel block, tap,
// channel) as pack.py packs it, and either exact 16 x 32 tiles or 16 x 16 tiles that overhang the
// image by at most a quarter of their pixels)
bool conv3x3_halo_supported(const ConvDesc& d);
// true when conv3x3_halo runs a persistent kernel for d that can also emit InstanceNorm partials of its output
// (d.in_part): count of partial records per (sample, channel) in *nrec
// (the persistent 16 x 16 forms for overhanging tiles / the IBasicBlock epilogue write no partials)
bool conv3x3_pp_takes(const ConvDesc& d, int* nrec);
int conv3x3_halo(const ConvDesc& d, hipStream_t s);

// ConvTranspose2d 4x4/s2/p1 on 8 x 16 input tiles (bf16, Cin % 32 == 0, N % 64 == 0 or N == 32,
// H % 8 == 0, W % 16 == 0; weights as pack.py pack_convT4x4 lays them out)
bool convT_halo_supported(const ConvDesc& d);
PlanSig convT_halo_signature(const ConvDesc& d);
int convT_halo(const ConvDesc& d, hipStream_t s);

}  // namespace ghost
