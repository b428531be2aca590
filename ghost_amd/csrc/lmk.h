// ghost_amd — kernels of the 106-point landmark network (2d106det: MobileNet-v1 at width 0.5), lmk.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plan_log.h"

namespace ghost {

// depthwise 3x3 (stride 1 | 2, pad 1) + BN + PReLU, rounded once to the storage type, then (Cout > 0) the pointwise
// 1x1 over Cout on the matrix cores + BN + PReLU.  Cout == 0: depthwise only, written to y.
struct DwsepDesc {
  int dt = 0;                          // storage type of x, w, y and dw_tap
  const void* x = nullptr;             // [B,H,W,ldx]
  int B = 0, H = 0, W = 0, Cin = 0, ldx = 0, stride = 1;
  const float* dw_w = nullptr;         // [9][Cin] fp32, tap ky*3 + kx
  const float* dw_scale = nullptr;     // [Cin] each
  const float* dw_shift = nullptr;
  const float* dw_prelu = nullptr;
  const void* w = nullptr;             // pointwise [>= Cout][Kpad] in dt, K = input channel, zero beyond Cin
  int Cout = 0, Kpad = 0;
  const float* scale = nullptr;        // [Cout] each
  const float* shift = nullptr;
  const float* prelu = nullptr;
  void* y = nullptr;                   // [B,Ho,Wo,ldy]
  int ldy = 0;
  void* dw_tap = nullptr;              // optional [B,Ho,Wo,ldt]: the rounded depthwise activations
  int ldt = 0;
};

struct DwsepPlan {
  bool ok = false;
  int Ho = 0, Wo = 0, BM = 0, BN = 0, Kp = 0, lda = 0;   // row tile, column tile, padded K, LDS row stride (elements)
  long M = 0;
  unsigned grid[2] = {0, 0};
  size_t lds_bytes = 0;
};

DwsepPlan dwsep_plan(const DwsepDesc& d);                       // pure
PlanSig dwsep_signature(const DwsepPlan& p, const DwsepDesc& d);
int dwsep_launch(const DwsepDesc& d, hipStream_t s);            // 0, a hipError_t, or -1 (bad descriptor)

// stem: uint8 [N,Hi,Wi,3] (bgr != 0: B,G,R order) -> (x - 127.5) * 0.0078125 in RGB order -> conv 3x3 s2 p1 3 -> 16
// (w [27][16] fp32, K = (ky*3 + kx)*3 + rgb channel) + BN + PReLU -> [N,Hi/2,Wi/2,16] in dt
int lmk_stem(int dt, const uint8_t* x, int64_t bstride, int bgr, int N, int Hi, int Wi, const float* w,
             const float* scale, const float* shift, const float* prelu, void* y, hipStream_t s);
// head: pred[n][j] = bias[j] + sum_k x[n][k] w[k][j] over the K = 576 stored values of conv_15 in NHWC order
// (w [K][J] fp32); landmarks[n][j] = (pred + 1) * 96 * 1.75 - 56.  pred or landmarks may be NULL, not both.
int lmk_head(int dt, const void* x, int N, int K, int J, const float* w, const float* bias, float* pred,
             float* landmarks, hipStream_t s);
// frame_index[n] = n and maps[n] = m6 for ghost_align_crops_u8 over a batch of crops
int lmk_fill_maps(int32_t* frame_index, double* maps, int N, const double m6[6], hipStream_t s);

}  // namespace ghost
