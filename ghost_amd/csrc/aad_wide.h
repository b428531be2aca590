// ghost_amd — AADLayer kernel for the wide stages (bf16, C in {256, 512, 1024}, Ca <= 512):
// one workgroup per (pixel block, 64-channel tile), weights in the pack_aad_v3 layout.
#pragma once
#include <hip/hip_runtime.h>

#include "plan_log.h"

namespace ghost {

struct AadWideDesc {
  const void* za = nullptr;  int lda = 0, Ca = 0;
  const void* hin = nullptr; int ldh = 0;
  const float* stat = nullptr;                 // [B][C][2] mean, rstd of h_in
  int B = 0, HW = 0, C = 0, id_ld = 0;
  float slope = 0.f;
  const void* w3 = nullptr;                    // [C/64][128][Ca] permuted (pack.py pack_aad_v3)
  const float* b3 = nullptr;                   // [C/64][128]
  const float* wh = nullptr;                   // conv_h weight [C]
  const float* bh = nullptr;                   // conv_h bias [1]
  const float* idgb = nullptr;                 // [B][id_ld]: gamma_id at c, beta_id at C + c
  const float* mask = nullptr;                 // [B*HW] sigmoid mask of this layer (aad_mask)
  void* out = nullptr;       int ldo = 0;
  int dt = 1;                                  // storage type: GHOST_BF16 (1) or GHOST_F16 (2)
};

// the inputs of a launch, then its one layer (the same pair as aad_v3.h's)
inline AadWideDesc aad_wide_desc(int dt, const void* za, int lda, int Ca, const void* hin, int ldh, const float* stat,
                                 int B, int HW, int C, int id_ld, float slope) {
  AadWideDesc d;
  d.dt = dt;
  d.za = za; d.lda = lda; d.Ca = Ca; d.hin = hin; d.ldh = ldh; d.stat = stat;
  d.B = B; d.HW = HW; d.C = C; d.id_ld = id_ld; d.slope = slope;
  return d;
}
inline void aad_wide_set_layer(AadWideDesc& d, const void* w3, const float* b3, const float* wh, const float* bh,
                               const float* idgb, const float* mask, void* out, int ldo) {
  d.w3 = w3; d.b3 = b3; d.wh = wh; d.bh = bh; d.idgb = idgb; d.mask = mask;
  d.out = out; d.ldo = ldo;
}

// What a launch of a descriptor runs, decided from its integers (dt, B, HW, C, Ca, the leading dimensions) and
// from whether za and w3 are 16-byte aligned (aad_gemm's DMA needs it; without it the launch takes aad_wide)
enum class AadWideKernel { None, Gemm, Wide, WideDeep };
struct AadWidePlan {
  AadWideKernel kernel = AadWideKernel::None;   // None: no kernel takes this descriptor
  int ppw = 0;                                  // pixels per workgroup (aad_wide, aad_wide_deep)
  unsigned grid = 0, block = 0;
};
AadWidePlan aad_wide_plan(const AadWideDesc& d, bool ptrs_aligned16);
PlanSig aad_wide_signature(const AadWidePlan& p, const AadWideDesc& d);   // the plan-log line of (plan, desc)

bool aad_wide_shape(int C, int Ca);   // the (C, Ca) with a kernel here
// true when a launch of this shape has a plan (whatever its pointers' alignment)
bool aad_wide_supported(int dt, int B, int HW, int C, int Ca, int lda, int ldh, int ldo);
int aad_wide(const AadWideDesc& d, hipStream_t s);

}  // namespace ghost
