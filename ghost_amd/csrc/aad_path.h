// ghost_amd — which kernel family blends the AADLayers of one group (same h_in / z_attr, one output each):
// the runtime's layer groups and the op entry points ask here, the families' planners (aad_v3.h, aad_wide.h)
// decide the rest.
#pragma once
#include "aad_fused.h"
#include "aad_v3.h"
#include "aad_wide.h"
#include "ghost_common.h"

namespace ghost {

// V3: aad_v3, up to aad_v3_max_layers per launch.  Wide: the masks from one aad_mask2 pass, one aad_wide launch
// per layer.  Fused: aad_fused per layer.  Split: aad_mask + the GEMM with the blend epilogue per layer.
enum class AadPath { V3, Wide, Fused, Split };

// reg_layout: the layers carry the w3 / b3 slots (aad_reg_layout); without them only Fused and Split remain
inline AadPath aad_path(int dt, int B, int HW, int C, int Ca, int lda, int ldh, const int ldo[], int L,
                        bool reg_layout = true) {
  auto every = [&](bool (*ok)(int, int, int, int, int, int, int, int)) {
    for (int l = 0; l < L; ++l)
      if (!ok(dt, B, HW, C, Ca, lda, ldh, ldo[l])) return false;
    return true;
  };
  if (reg_layout && every(aad_v3_supported)) return AadPath::V3;
  if (reg_layout && L <= 2 && every(aad_wide_supported)) return AadPath::Wide;
  return every(aad_fused_supported) ? AadPath::Fused : AadPath::Split;
}

// the AADLayers packed in the permuted register-epilogue layout as well (w3 / b3: pack.py pack_aad_v3, v3_layout):
// every (C, Ca) one of the two planners has a kernel for
inline bool aad_reg_layout(int dt, int C, int Ca) {
  return is16(dt) && (aad_v3_max_layers(C, Ca) > 0 || aad_wide_shape(C, Ca));
}

}  // namespace ghost
