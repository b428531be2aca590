// ghost_amd — register-epilogue AADLayer kernel for the 64/128-channel stages (bf16).
#pragma once
#include <hip/hip_runtime.h>

#include "plan_log.h"

namespace ghost {

struct AadV3Desc {
  int dt = 1;                                        // storage type: GHOST_BF16 (1) or GHOST_F16 (2)
  const void* za = nullptr;  int lda = 0, Ca = 0;   // z_attr NHWC
  const void* hin = nullptr; int ldh = 0;           // h_in NHWC (shared by the L layers)
  // up_H > 0: h_in = upsample2x(hin) (bilinear x2, align_corners) with hin the [B, up_H, up_W]
  // source, sampled on the fly (values rounded to bf16 as upsample2x stores them)
  int up_H = 0, up_W = 0;
  const float* stat = nullptr;                       // [B][C][2] mean, rstd of h_in
  int B = 0, HW = 0, C = 0, L = 1, id_ld = 0;
  float slope = 0.f;
  // per layer (L <= 2): permuted weights [C/64][128][Ca], biases [C/64][128], conv_h, id table, output
  const void* w3[2] = {nullptr, nullptr};
  const float* b3[2] = {nullptr, nullptr};
  const float* wh[2] = {nullptr, nullptr};
  const float* bh[2] = {nullptr, nullptr};
  const float* idgb[2] = {nullptr, nullptr};
  void* out[2] = {nullptr, nullptr};
  int ldo[2] = {0, 0};
  // tap partials (C = 64 only): a layer with zw[l] set writes, instead of its 64 channels, its share of
  // the 3x3 conv to 3 channels that is its only consumer, per-tap sums Z_t[o] = sum_c zw[l][t*3 + o][c] *
  // out_c (t = ky*3 + kx) pre-summed along 8-column row segments (tap_rows.h: 15 fp16 per pixel; zw: bf16
  // rows of stride zwld, the narrow layout's K slice of this layer's channels); out[l] is then that buffer,
  // zr_image(HW) fp16 per sample, and the image width must be a multiple of 8
  const void* zw[2] = {nullptr, nullptr};
  int zwld = 0;
  // in-kernel clock of the launch (profiling; v4 / v5): AadV3Plan::clock_words words of per-workgroup start
  // and per-wave end stamps
  unsigned long long* tclk = nullptr;
};

// what the L layers of a launch share, for an H x W image (up2x: hin is its [B, H/2, W/2] source); the caller
// sets L, then each layer
inline AadV3Desc aad_v3_desc(int dt, const void* za, int lda, int Ca, const void* hin, int ldh, const float* stat, int B,
                             int H, int W, int C, int id_ld, float slope, bool up2x) {
  AadV3Desc d;
  d.dt = dt;
  d.za = za; d.lda = lda; d.Ca = Ca; d.hin = hin; d.ldh = ldh; d.stat = stat;
  d.B = B; d.HW = H * W; d.C = C; d.id_ld = id_ld; d.slope = slope;
  if (up2x) { d.up_H = H / 2; d.up_W = W / 2; }
  return d;
}
inline void aad_v3_set_layer(AadV3Desc& d, int l, const void* w3, const float* b3, const float* wh, const float* bh,
                             const float* idgb, void* out, int ldo) {
  d.w3[l] = w3; d.b3[l] = b3; d.wh[l] = wh; d.bh[l] = bh; d.idgb[l] = idgb;
  d.out[l] = out; d.ldo[l] = ldo;
}

// What a launch of a descriptor runs, decided from its integers and flags alone (dt, B, HW, C, Ca, L, the leading
// dimensions, up_H / up_W, zwld, slope == 0, which zw[l] are set): no pointer is read through, no HIP call made.
enum class AadV3Kernel { None, V3, V3Wide, V3Zp1, V3Z, V4, V4Z, V5, V5Z, V5ZAsm, V5Wide };
struct AadV3Plan {
  AadV3Kernel kernel = AadV3Kernel::None;   // None: no kernel takes this descriptor
  int version = 0;                          // kernel generation: 3, 4 or 5
  int ppw = 0, ipw = 0, zpm = 0;            // pixels per workgroup / work item, v5 work items per workgroup, zw mask
  unsigned grid = 0, block = 0, dyn_lds = 0;
  int clock_words = 0;                      // words a launch with tclk set stamps (0: generation 3 stamps none)
};
AadV3Plan aad_v3_plan(const AadV3Desc& d);
PlanSig aad_v3_signature(const AadV3Plan& p, const AadV3Desc& d);   // the plan-log line of (plan, desc)

// the 3x3 / pad 1 conv to 3 channels from two tap-partial buffers (AADBlk8's output conv over
// cat(h, x'), AADLayer.py:71,79): y = tanh(sum_t (zh + zx)[p + off_t][t*3 + o]) -> bf16 y (ldy) + BGR uint8
int tap_sum3x3(int dt, const void* zh, const void* zx, int B, int H, int W, void* y, int ldy, uint8_t* u8,
               hipStream_t s);

// the (C, Ca) with a kernel here, and how many AADLayers one launch of it blends (1 or 2; 0: none)
int aad_v3_max_layers(int C, int Ca);
// true when a one-layer launch of this shape has a plan
bool aad_v3_supported(int dt, int B, int HW, int C, int Ca, int lda, int ldh, int ldo);
// launches p = aad_v3_plan(d) (the second form plans itself); -1 when the plan is None or a zw[l] is misaligned
int aad_v3(const AadV3Desc& d, const AadV3Plan& p, hipStream_t s);
int aad_v3(const AadV3Desc& d, hipStream_t s);

}  // namespace ghost
