// ghost_amd — the two bandwidth-bound passes of the use_sr face enhancer (LIPSPADEGenerator,
// models/networks/generator.py:353-388 and normalization.py:63-107 of the reference).  Both are NHWC, one thread
// per 16-byte channel vector, fp32 arithmetic, 64-bit addressing, no LDS and no scratch.
//
//   norm_modulate: out = act((src - mean) * rstd * gamma + beta)   InstanceNorm (+ReLU) of the LIP encoder and the
//                  SPADE modulation of the decoder, optionally reading src through a nearest x2 upsample
//   lip_pool:      out = sum3x3 x e^l / sum3x3 e^l, l = 12 sigmoid(IN_affine(logit))   SimplifiedLIP, stride 2
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ghost_amd.h"
#include "ghost_common.h"
#include "plan_log.h"

namespace ghost {
int set_last_error(int rc, const std::string& msg);   // aei_runtime.hip (ghost_last_error)
}
using namespace ghost;

namespace {

int sr_fail(const char* msg) { return ghost::set_last_error(GHOST_EINVAL, std::string(msg)); }

constexpr int kMaxBlocks = 256 * 32;   // grid-stride: 32 workgroups of 256 threads per CU

struct NmArgs {
  const void* src;
  const void* gb;    // optional: gamma at channel c, beta at C + c of one [.., ldgb] tensor
  const float* stat;   // [Bs][C][2] mean, rstd
  void* out;
  long total;   // B * H * W * (C / VEC) vectors
  int H, W, C, ldx, ldgb, ldo, bstat, up2x;
  float slope;
};

template <typename T>
__global__ void __launch_bounds__(256) norm_modulate_kernel(const NmArgs a) {
  constexpr int VEC = Vec16<T>::N;
  const int cv = a.C / VEC;
  const T* __restrict__ src = reinterpret_cast<const T*>(a.src);
  const T* __restrict__ gb = reinterpret_cast<const T*>(a.gb);
  T* __restrict__ out = reinterpret_cast<T*>(a.out);
  const long hw = (long)a.H * a.W;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (long)gridDim.x * 256) {
    const long p = i / cv;
    const int c = (int)(i - p * cv) * VEC;
    const long b = p / hw;
    long ps = p;
    if (a.up2x) {   // nearest x2: pixel (y, x) of the output reads (y >> 1, x >> 1) of the [B, H/2, W/2, C] source
      const long r = p - b * hw;
      const int y = (int)(r / a.W), x = (int)(r - (long)y * a.W);
      ps = (b * (a.H >> 1) + (y >> 1)) * (a.W >> 1) + (x >> 1);
    }
    float v[VEC];
    load16_f(src + ps * a.ldx + c, v);
    // (mean, rstd) pairs of the vector's channels: 2 VEC floats, 32-byte aligned (c % VEC == 0)
    const f32x4* sp = reinterpret_cast<const f32x4*>(a.stat + ((a.bstat ? b : 0) * a.C + c) * 2);
#pragma unroll
    for (int e = 0; e < VEC; e += 2) {
      const f32x4 st = sp[e >> 1];
      v[e] = (v[e] - st[0]) * st[1];
      v[e + 1] = (v[e + 1] - st[2]) * st[3];
    }
    if (gb) {
      float g[VEC], bt[VEC];
      load16_f(gb + p * a.ldgb + c, g);
      load16_f(gb + p * a.ldgb + a.C + c, bt);
#pragma unroll
      for (int e = 0; e < VEC; ++e) v[e] = v[e] * g[e] + bt[e];
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * a.slope;
    store16_f(out + p * a.ldo + c, v);
  }
}

struct LipArgs {
  const void* x;
  const void* logit;
  const float* stat;   // [B][C][2] mean, rstd of logit
  const float* w;      // [C] InstanceNorm affine
  const float* b;
  void* out;
  long total;   // B * (H/2) * (W/2) * (C / VEC)
  int H, W, C, ldx, ldl, ldo;
};

template <typename T>
__global__ void __launch_bounds__(256) lip_pool_kernel(const LipArgs a) {
  constexpr int VEC = Vec16<T>::N;
  const int cv = a.C / VEC;
  const T* __restrict__ xin = reinterpret_cast<const T*>(a.x);
  const T* __restrict__ lg = reinterpret_cast<const T*>(a.logit);
  T* __restrict__ out = reinterpret_cast<T*>(a.out);
  const int Ho = a.H >> 1, Wo = a.W >> 1;
  const long hwo = (long)Ho * Wo;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (long)gridDim.x * 256) {
    const long p = i / cv;
    const int c = (int)(i - p * cv) * VEC;
    const long b = p / hwo;
    const long r = p - b * hwo;
    const int oy = (int)(r / Wo), ox = (int)(r - (long)oy * Wo);
    float mean[VEC], rstd[VEC], w[VEC], bb[VEC], num[VEC], den[VEC];
    const float* sp = a.stat + (b * a.C + c) * 2;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      mean[e] = sp[2 * e];
      rstd[e] = sp[2 * e + 1];
      w[e] = a.w[c + e];
      bb[e] = a.b[c + e];
      num[e] = 0.f;
      den[e] = 0.f;
    }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = 2 * oy - 1 + ky;
      if (iy < 0 || iy >= a.H) continue;   // padding taps are zero in both sums
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = 2 * ox - 1 + kx;
        if (ix < 0 || ix >= a.W) continue;
        const long q = (b * a.H + iy) * a.W + ix;
        float xv[VEC], lv[VEC];
        load16_f(xin + q * a.ldx + c, xv);
        load16_f(lg + q * a.ldl + c, lv);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float l = 12.f * sigmoidf_ref(((lv[e] - mean[e]) * rstd[e]) * w[e] + bb[e]);
          const float ex = expf(l);
          num[e] = fmaf(xv[e], ex, num[e]);
          den[e] += ex;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) num[e] = num[e] / den[e];
    store16_f(out + p * a.ldo + c, num);
  }
}

unsigned grid_for(long total) {
  const long nb = (total + 255) / 256;
  return (unsigned)(nb < kMaxBlocks ? nb : kMaxBlocks);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int ghost_norm_modulate_nhwc(int dtype, const void* src, int ldx, int B, int H, int W, int C,
                                        const float* stat, int Bs, const void* gb, int ldgb, float slope, int up2x,
                                        void* out, int ldo, void* stream) {
  if (!src || !stat || !out) return sr_fail("norm_modulate: null pointer");
  if (dtype != GHOST_F32 && dtype != GHOST_BF16 && dtype != GHOST_F16) return sr_fail("norm_modulate: bad dtype");
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8) return sr_fail("norm_modulate: C must be a multiple of 8");
  if (Bs != 1 && Bs != B) return sr_fail("norm_modulate: Bs must be 1 or B");
  if (up2x && (H % 2 || W % 2)) return sr_fail("norm_modulate: up2x needs even H and W");
  const int vec = dtype == GHOST_F32 ? 4 : 8;
  if (ldx < C || ldo < C || ldx % vec || ldo % vec || !aligned16(src) || !aligned16(out) || !aligned16(stat))
    return sr_fail("norm_modulate: leading dimensions / pointers must be 16-byte aligned and >= C");
  if (gb && (ldgb < 2 * C || ldgb % vec || !aligned16(gb))) return sr_fail("norm_modulate: bad gamma/beta layout");
  NmArgs a{src, gb, stat, out, (long)B * H * W * (C / vec), H, W, C, ldx, ldgb, ldo, Bs == B && B > 1 ? 1 : 0,
           up2x ? 1 : 0, slope};
  // Bs == B == 1: instance and batch statistics are the same record
  GHOST_PLAN_LOG("norm_modulate t=%s vec=%d gb=%d up2x=%d stat=%s", plan_dt(dtype), vec, gb ? 1 : 0, a.up2x,
                 Bs == 1 ? "batch" : "instance");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == GHOST_F32) hipLaunchKernelGGL(norm_modulate_kernel<float>, dim3(grid_for(a.total)), dim3(256), 0, s, a);
  else if (dtype == GHOST_BF16) hipLaunchKernelGGL(norm_modulate_kernel<bf16>, dim3(grid_for(a.total)), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(norm_modulate_kernel<_Float16>, dim3(grid_for(a.total)), dim3(256), 0, s, a);
  const int rc = (int)hipGetLastError();
  return rc ? ghost::set_last_error(rc, std::string("norm_modulate: launch failed")) : 0;
}

extern "C" int ghost_lip_pool_nhwc(int dtype, const void* x, int ldx, const void* logit_raw, int ldl, int B, int H, int W,
                                   int C, const float* stat, const float* w, const float* b, void* out, int ldo,
                                   void* stream) {
  if (!x || !logit_raw || !stat || !w || !b || !out) return sr_fail("lip_pool: null pointer");
  if (dtype != GHOST_F32 && dtype != GHOST_BF16 && dtype != GHOST_F16) return sr_fail("lip_pool: bad dtype");
  if (B <= 0 || H <= 0 || W <= 0 || H % 2 || W % 2) return sr_fail("lip_pool: H and W must be even");
  if (C <= 0 || C % 8) return sr_fail("lip_pool: C must be a multiple of 8");
  const int vec = dtype == GHOST_F32 ? 4 : 8;
  if (ldx < C || ldl < C || ldo < C || ldx % vec || ldl % vec || ldo % vec || !aligned16(x) || !aligned16(logit_raw) ||
      !aligned16(out))
    return sr_fail("lip_pool: leading dimensions / pointers must be 16-byte aligned and >= C");
  LipArgs a{x, logit_raw, stat, w, b, out, (long)B * (H / 2) * (W / 2) * (C / vec), H, W, C, ldx, ldl, ldo};
  GHOST_PLAN_LOG("lip_pool t=%s vec=%d k=3 s=2", plan_dt(dtype), vec);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == GHOST_F32) hipLaunchKernelGGL(lip_pool_kernel<float>, dim3(grid_for(a.total)), dim3(256), 0, s, a);
  else if (dtype == GHOST_BF16) hipLaunchKernelGGL(lip_pool_kernel<bf16>, dim3(grid_for(a.total)), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(lip_pool_kernel<_Float16>, dim3(grid_for(a.total)), dim3(256), 0, s, a);
  const int rc = (int)hipGetLastError();
  return rc ? ghost::set_last_error(rc, std::string("lip_pool: launch failed")) : 0;
}
