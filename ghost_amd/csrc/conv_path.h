// ghost_amd — which kernel family runs one convolution: conv_launch, conv_workspace_bytes and ghost_conv_plan ask
// here; the families' own *_supported predicates say what each takes, their planners (conv_halo.h, conv_igemm.h)
// decide the rest.
#pragma once
#include "conv_first.h"
#include "conv_halo.h"
#include "conv_igemm.h"
#include "conv_s2.h"

namespace ghost {

// Halo3x3: conv3x3_halo (halo_plan).  First / Stem3x3: the 3-channel input convs (conv_first.h).  ConvTHalo: the
// 4x4/s2 deconv on input tiles.  S2Patch: the 4x4/s2 and 3x3/s2 LDS-patch kernel.  Igemm: the implicit GEMM
// (igemm_plan), which takes everything else — a forced split (d.force_split) among it.
enum class ConvPath { Halo3x3, First, Stem3x3, ConvTHalo, S2Patch, Igemm };

inline ConvPath conv_path(const ConvDesc& d) {
  if (conv3x3_halo_supported(d)) return ConvPath::Halo3x3;
  if (conv_first_supported(d)) return ConvPath::First;
  if (conv_stem3x3_supported(d)) return ConvPath::Stem3x3;
  if (convT_halo_supported(d)) return ConvPath::ConvTHalo;
  if (conv4x4s2_patch_supported(d) || conv3x3s2_patch_supported(d)) return ConvPath::S2Patch;
  return ConvPath::Igemm;
}

}  // namespace ghost
