// ghost_amd — kernels of the 106-point landmark network (coordinate_reg/model/2d106det-symbol.json of the
// reference: MobileNet-v1 at width 0.5 on a 192x192 crop).  NHWC, fp32 arithmetic, 64-bit addressing, no scratch.
//
//   lmk_stem_kernel    uint8 crop -> normalise, RGB order, conv 3x3 s2 3 -> 16 + BN + PReLU, all in fp32 VALU
//   dwsep_kernel       one depthwise-separable block: a workgroup owns BM output pixels across all of Cin; it
//                      evaluates the depthwise 3x3 + BN + PReLU in fp32 VALU, rounds once to the storage type into LDS
//                      and runs the pointwise 1x1 on the matrix cores with the weights as the A operand and the LDS
//                      image as B, so a lane's four accumulators are four consecutive channels of one pixel
//   lmk_head_kernel    fc over the 576 stored values of conv_15 in fp32 + the landmark transform
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>

#include "../../include/ghost_amd.h"
#include "ghost_common.h"
#include "lmk.h"

namespace ghost {
int set_last_error(int rc, const std::string& msg);   // aei_runtime.hip (ghost_last_error)
}
using namespace ghost;

namespace {

// eight consecutive elements <-> fp32
template <typename T> GHOST_DEV void load8_f(const T* p, float* v) { load16_f(p, v); }
template <> GHOST_DEV void load8_f<float>(const float* p, float* v) {
  load16_f(p, v);
  load16_f(p + 4, v + 4);
}
template <typename T> GHOST_DEV void store8_f(T* p, const float* v) { store16_f(p, v); }
template <> GHOST_DEV void store8_f<float>(float* p, const float* v) {
  store16_f(p, v);
  store16_f(p + 4, v + 4);
}
template <typename T> GHOST_DEV void store4_f(T* p, const float* v) {
  typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
  *reinterpret_cast<u32x2*>(p) = u32x2{pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3])};
}
template <> GHOST_DEV void store4_f<float>(float* p, const float* v) { store16_f(p, v); }

// the MFMA operand of one lane: 8 consecutive K of one row (16x16x32 for 16-bit; fp32 runs eight 16x16x4 steps, step j
// taking element j of every lane group, a permutation of K that both operands share)
template <typename T> struct Frag { v8_t<T> v; };
template <> struct Frag<float> { float v[8]; };

template <typename T> GHOST_DEV Frag<T> frag_load(const T* p) {
  Frag<T> f;
  f.v = *reinterpret_cast<const v8_t<T>*>(p);
  return f;
}
template <> GHOST_DEV Frag<float> frag_load<float>(const float* p) {
  Frag<float> f;
  load8_f(p, f.v);
  return f;
}
template <typename T> GHOST_DEV f32x4 frag_mma(const Frag<T>& a, const Frag<T>& b, f32x4 c) {
  return mfma16x16x32<T>(a.v, b.v, c);
}
template <> GHOST_DEV f32x4 frag_mma<float>(const Frag<float>& a, const Frag<float>& b, f32x4 c) {
#pragma unroll
  for (int j = 0; j < 8; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[j], b.v[j], c, 0, 0, 0);
  return c;
}

struct DwsepArgs {
  const void* x;
  const float* dww;
  const float* dsc;
  const float* dsh;
  const float* dpr;
  const void* w;
  const float* psc;
  const float* psh;
  const float* ppr;
  void* y;
  void* tap;
  long M;
  int H, W, Ho, Wo, Cin, Cout, stride, ldx, ldy, ldt, ldw, Kp, BN, lda;
};

// MT: 16-pixel row tiles per workgroup (BM = 16 MT).  256 threads; wave w takes the 16-channel column tiles w and w + 4
// of the workgroup's BN <= 128 columns.
template <typename T, int MT>
__global__ void __launch_bounds__(256) dwsep_kernel(const DwsepArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lmk_smem[];
  T* As = reinterpret_cast<T*>(lmk_smem);
  constexpr int BM = 16 * MT;
  const int tid = threadIdx.x;
  const long m0 = (long)blockIdx.x * BM;
  const bool gemm = a.Cout > 0;
  const T* __restrict__ x = reinterpret_cast<const T*>(a.x);
  // the rounded depthwise activations leave through the tap (or y when there is no pointwise stage), written by the
  // first column tile only
  T* dst = gemm ? reinterpret_cast<T*>(a.tap) : reinterpret_cast<T*>(a.y);
  const int ldd = gemm ? a.ldt : a.ldy;
  if (blockIdx.y != 0) dst = nullptr;
  const int cvp = a.Kp >> 3;
  const long hwo = (long)a.Ho * a.Wo;
  for (int i = tid; i < BM * cvp; i += 256) {
    const int r = i / cvp, c = (i - r * cvp) << 3;
    const long p = m0 + r;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bool live = p < a.M && c < a.Cin;   // padded rows and the K padding of Cin = 16 are zeros
    if (live) {
      const long b = p / hwo;
      const long rem = p - b * hwo;
      const int oy = (int)(rem / a.Wo), ox = (int)(rem - (long)oy * a.Wo);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * a.stride - 1 + ky;
        if (iy < 0 || iy >= a.H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int ix = ox * a.stride - 1 + kx;
          if (ix < 0 || ix >= a.W) continue;
          float xv[8], wv[8];
          load8_f(x + ((b * a.H + iy) * a.W + ix) * a.ldx + c, xv);
          load8_f(a.dww + (ky * 3 + kx) * a.Cin + c, wv);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = fmaf(xv[e], wv[e], v[e]);
        }
      }
      float sc[8], sh[8], pr[8];
      load8_f(a.dsc + c, sc);
      load8_f(a.dsh + c, sh);
      load8_f(a.dpr + c, pr);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float t = v[e] * sc[e] + sh[e];
        v[e] = t > 0.f ? t : t * pr[e];
      }
      if (dst) store8_f(dst + p * ldd + c, v);
    }
    if (gemm) store8_f(As + r * a.lda + c, v);
  }
  if (!gemm) return;
  __syncthreads();

  const int lane = tid & 63, wv = tid >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const int NT = a.BN >> 4;
  const int n_base = blockIdx.y * a.BN;
  const T* __restrict__ w = reinterpret_cast<const T*>(a.w);
  f32x4 acc[2][MT];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[j][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < a.Kp; k0 += 32) {
    Frag<T> xb[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) xb[mt] = frag_load<T>(As + (mt * 16 + l16) * a.lda + k0 + 8 * g);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int nt = wv + 4 * j;
      if (nt < NT) {   // wave-uniform
        const Frag<T> wa = frag_load<T>(w + (long)(n_base + nt * 16 + l16) * a.ldw + k0 + 8 * g);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[j][mt] = frag_mma<T>(wa, xb[mt], acc[j][mt]);
      }
    }
  }
  // D[channel 4 g + r of the tile][pixel l16]
  T* __restrict__ y = reinterpret_cast<T*>(a.y);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int nt = wv + 4 * j;
    if (nt >= NT) continue;
    const int n = n_base + nt * 16 + 4 * g;
    const f32x4 sc = *reinterpret_cast<const f32x4*>(a.psc + n);
    const f32x4 sh = *reinterpret_cast<const f32x4*>(a.psh + n);
    const f32x4 pr = *reinterpret_cast<const f32x4*>(a.ppr + n);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const long p = m0 + mt * 16 + l16;
      if (p >= a.M) continue;   // padded rows are never stored
      float o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float t = acc[j][mt][r] * sc[r] + sh[r];
        o[r] = t > 0.f ? t : t * pr[r];
      }
      store4_f(y + p * a.ldy + n, o);
    }
  }
}

struct StemArgs {
  const uint8_t* x;
  long bstride;
  const float* w;
  const float* sc;
  const float* sh;
  const float* pr;
  void* y;
  long total;   // N * Ho * Wo
  int Hi, Wi, Ho, Wo, bgr;
};

template <typename T>
__global__ void __launch_bounds__(256) lmk_stem_kernel(const StemArgs a) {
  __shared__ float ws[27 * 16 + 48];
  for (int i = threadIdx.x; i < 27 * 16; i += 256) ws[i] = a.w[i];
  if (threadIdx.x < 16) {
    ws[432 + threadIdx.x] = a.sc[threadIdx.x];
    ws[448 + threadIdx.x] = a.sh[threadIdx.x];
    ws[464 + threadIdx.x] = a.pr[threadIdx.x];
  }
  __syncthreads();
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;   // one output pixel, 16 channels
  if (idx >= a.total) return;
  const long hwo = (long)a.Ho * a.Wo;
  const long n = idx / hwo;
  const long rem = idx - n * hwo;
  const int oy = (int)(rem / a.Wo), ox = (int)(rem - (long)oy * a.Wo);
  const uint8_t* __restrict__ src = a.x + n * a.bstride;
  float acc[16];
#pragma unroll
  for (int o = 0; o < 16; ++o) acc[o] = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = 2 * oy - 1 + ky;
    if (iy < 0 || iy >= a.Hi) continue;   // the zero padding is of the normalised image
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = 2 * ox - 1 + kx;
      if (ix < 0 || ix >= a.Wi) continue;
      const uint8_t* px = src + ((long)iy * a.Wi + ix) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = ((float)px[a.bgr ? 2 - c : c] - 127.5f) * 0.0078125f;   // exact in fp32
        const float* wr = ws + ((ky * 3 + kx) * 3 + c) * 16;
#pragma unroll
        for (int o = 0; o < 16; ++o) acc[o] = fmaf(v, wr[o], acc[o]);
      }
    }
  }
#pragma unroll
  for (int o = 0; o < 16; ++o) {
    const float t = acc[o] * ws[432 + o] + ws[448 + o];
    acc[o] = t > 0.f ? t : t * ws[464 + o];
  }
  T* y = reinterpret_cast<T*>(a.y) + idx * 16;
  store8_f(y, acc);
  store8_f(y + 8, acc + 8);
}

constexpr int kHeadMaxK = 1024;

template <typename T>
__global__ void __launch_bounds__(256) lmk_head_kernel(const T* __restrict__ x, int K, int J,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* pred, float* lmk) {
  __shared__ float xs[kHeadMaxK];
  const long n = blockIdx.x;
  for (int k = threadIdx.x; k < K; k += 256) xs[k] = to_f(x[n * K + k]);
  __syncthreads();
  for (int j = threadIdx.x; j < J; j += 256) {
    float acc = bias[j];
    for (int k = 0; k < K; ++k) acc = fmaf(xs[k], w[(long)k * J + j], acc);
    if (pred) pred[n * J + j] = acc;
    // (pred + 1) * (192 / 2), then IM = [[1.75, 0, -56], [0, 1.75, -56]]: one rounding, of the exact value
    if (lmk) lmk[n * J + j] = (float)(((double)acc + 1.0) * 96.0 * 1.75 - 56.0);
  }
}

__global__ void __launch_bounds__(256) lmk_fill_maps_kernel(int32_t* fi, double* maps, int N, double m0, double m1,
                                                             double m2, double m3, double m4, double m5) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  fi[n] = n;
  double* m = maps + (long)n * 6;
  m[0] = m0; m[1] = m1; m[2] = m2; m[3] = m3; m[4] = m4; m[5] = m5;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename T>
int dwsep_run(const DwsepDesc& d, const DwsepPlan& p, hipStream_t s) {
  DwsepArgs a{d.x, d.dw_w, d.dw_scale, d.dw_shift, d.dw_prelu, d.w, d.scale, d.shift, d.prelu, d.y, d.dw_tap, p.M,
              d.H, d.W, p.Ho, p.Wo, d.Cin, d.Cout, d.stride, d.ldx, d.ldy, d.ldt, d.Kpad, p.Kp, p.BN, p.lda};
  constexpr int MT = sizeof(T) == 4 ? 1 : 2;
  hipLaunchKernelGGL((dwsep_kernel<T, MT>), dim3(p.grid[0], p.grid[1]), dim3(256), p.lds_bytes, s, a);
  return (int)hipGetLastError();
}

}  // namespace

namespace ghost {

DwsepPlan dwsep_plan(const DwsepDesc& d) {
  DwsepPlan p;
  if (d.dt != GHOST_F32 && d.dt != GHOST_BF16 && d.dt != GHOST_F16) return p;
  const int vec = d.dt == GHOST_F32 ? 4 : 8;   // elements per 16 bytes
  if (!d.x || !d.dw_w || !d.dw_scale || !d.dw_shift || !d.dw_prelu || !d.y) return p;
  if (d.B <= 0 || d.H <= 0 || d.W <= 0 || d.Cin <= 0 || d.Cin % 8 || (d.stride != 1 && d.stride != 2)) return p;
  if (d.ldx < d.Cin || d.ldx % vec || !aligned16(d.x) || !aligned16(d.dw_w) || !aligned16(d.dw_scale) ||
      !aligned16(d.dw_shift) || !aligned16(d.dw_prelu))
    return p;
  const int Cy = d.Cout > 0 ? d.Cout : d.Cin;
  if (d.ldy < Cy || d.ldy % vec || !aligned16(d.y)) return p;
  if (d.Cout < 0) return p;
  if (d.Cout > 0) {
    if (d.Cout % 16 || (d.Cout > 128 && d.Cout % 128)) return p;
    if (!d.w || !d.scale || !d.shift || !d.prelu || !aligned16(d.w) || !aligned16(d.scale) || !aligned16(d.shift) ||
        !aligned16(d.prelu))
      return p;
    if (d.Kpad < d.Cin || d.Kpad % 32) return p;
    if (d.dw_tap && (d.ldt < d.Cin || d.ldt % vec || !aligned16(d.dw_tap))) return p;
  } else if (d.dw_tap) {
    return p;   // depthwise only writes y
  }
  p.Ho = (d.H - 1) / d.stride + 1;   // (H + 2 - 3) / stride + 1
  p.Wo = (d.W - 1) / d.stride + 1;
  p.M = (long)d.B * p.Ho * p.Wo;
  p.BM = d.dt == GHOST_F32 ? 16 : 32;
  p.Kp = (d.Cin + 31) / 32 * 32;
  p.lda = p.Kp + vec;   // 16 bytes of row padding: the 16 rows of an operand read start in different banks
  p.BN = d.Cout > 128 ? 128 : d.Cout;
  p.lds_bytes = d.Cout > 0 ? (size_t)p.BM * p.lda * (d.dt == GHOST_F32 ? 4 : 2) : 0;
  if (p.lds_bytes > 65536) return p;
  const long gx = (p.M + p.BM - 1) / p.BM;
  if (gx > 0x7fffffffL) return p;
  p.grid[0] = (unsigned)gx;
  p.grid[1] = d.Cout > 0 ? (unsigned)(d.Cout / p.BN) : 1u;
  p.ok = true;
  return p;
}

PlanSig dwsep_signature(const DwsepPlan& p, const DwsepDesc& d) {
  PlanSig sig;
  if (d.Cout > 0)
    snprintf(sig.s, sizeof sig.s, "dwsep_block t=%s fused s=%d cin=%d cout=%d bm=%d bn=%d kp=%d tap=%d mtail=%d",
             plan_dt(d.dt), d.stride, d.Cin, d.Cout, p.BM, p.BN, p.Kp, d.dw_tap ? 1 : 0, p.M % p.BM ? 1 : 0);
  else
    snprintf(sig.s, sizeof sig.s, "dwsep_block t=%s dw_only s=%d cin=%d bm=%d", plan_dt(d.dt), d.stride, d.Cin, p.BM);
  return sig;
}

int dwsep_launch(const DwsepDesc& d, hipStream_t s) {
  const DwsepPlan p = dwsep_plan(d);
  if (!p.ok) return -1;
  if (g_plan_log_on.load(std::memory_order_relaxed)) plan_log_append("%s", dwsep_signature(p, d).s);
  if (d.dt == GHOST_F32) return dwsep_run<float>(d, p, s);
  if (d.dt == GHOST_BF16) return dwsep_run<bf16>(d, p, s);
  return dwsep_run<_Float16>(d, p, s);
}

int lmk_stem(int dt, const uint8_t* x, int64_t bstride, int bgr, int N, int Hi, int Wi, const float* w,
             const float* scale, const float* shift, const float* prelu, void* y, hipStream_t s) {
  if (!x || !w || !scale || !shift || !prelu || !y || N <= 0 || Hi <= 0 || Wi <= 0 || Hi % 2 || Wi % 2 ||
      !aligned16(y))
    return -1;
  StemArgs a{x, (long)bstride, w, scale, shift, prelu, y, (long)N * (Hi / 2) * (Wi / 2), Hi, Wi, Hi / 2, Wi / 2,
             bgr ? 1 : 0};
  const long nb = (a.total + 255) / 256;
  if (nb > 0x7fffffffL) return -1;
  GHOST_PLAN_LOG("lmk_stem t=%s k=3 s=2 bgr=%d", plan_dt(dt), a.bgr);
  if (dt == GHOST_F32) hipLaunchKernelGGL(lmk_stem_kernel<float>, dim3((unsigned)nb), dim3(256), 0, s, a);
  else if (dt == GHOST_BF16) hipLaunchKernelGGL(lmk_stem_kernel<bf16>, dim3((unsigned)nb), dim3(256), 0, s, a);
  else if (dt == GHOST_F16) hipLaunchKernelGGL(lmk_stem_kernel<_Float16>, dim3((unsigned)nb), dim3(256), 0, s, a);
  else return -1;
  return (int)hipGetLastError();
}

int lmk_head(int dt, const void* x, int N, int K, int J, const float* w, const float* bias, float* pred,
             float* landmarks, hipStream_t s) {
  if (!x || !w || !bias || (!pred && !landmarks) || N <= 0 || K <= 0 || K > kHeadMaxK || J <= 0) return -1;
  GHOST_PLAN_LOG("lmk_head t=%s k=%d j=%d lmk=%d", plan_dt(dt), K, J, landmarks ? 1 : 0);
  const dim3 grid((unsigned)N);
  if (dt == GHOST_F32)
    hipLaunchKernelGGL(lmk_head_kernel<float>, grid, dim3(256), 0, s, (const float*)x, K, J, w, bias, pred, landmarks);
  else if (dt == GHOST_BF16)
    hipLaunchKernelGGL(lmk_head_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)x, K, J, w, bias, pred, landmarks);
  else if (dt == GHOST_F16)
    hipLaunchKernelGGL(lmk_head_kernel<_Float16>, grid, dim3(256), 0, s, (const _Float16*)x, K, J, w, bias, pred,
                       landmarks);
  else return -1;
  return (int)hipGetLastError();
}

int lmk_fill_maps(int32_t* frame_index, double* maps, int N, const double m6[6], hipStream_t s) {
  if (!frame_index || !maps || N <= 0) return -1;
  hipLaunchKernelGGL(lmk_fill_maps_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, frame_index, maps, N,
                     m6[0], m6[1], m6[2], m6[3], m6[4], m6[5]);
  return (int)hipGetLastError();
}

}  // namespace ghost

extern "C" int ghost_dwsep_block_nhwc(int dtype, const void* x, int B, int H, int W, int Cin, int ldx, int stride,
                                      const float* dw_w, const float* dw_scale, const float* dw_shift,
                                      const float* dw_prelu, const void* w_packed, int Cout, int Kpad,
                                      const float* scale, const float* shift, const float* prelu, void* y, int ldy,
                                      void* dw_tap, int ld_tap, void* stream) {
  DwsepDesc d;
  d.dt = dtype; d.x = x; d.B = B; d.H = H; d.W = W; d.Cin = Cin; d.ldx = ldx; d.stride = stride;
  d.dw_w = dw_w; d.dw_scale = dw_scale; d.dw_shift = dw_shift; d.dw_prelu = dw_prelu;
  d.w = w_packed; d.Cout = Cout; d.Kpad = Kpad; d.scale = scale; d.shift = shift; d.prelu = prelu;
  d.y = y; d.ldy = ldy; d.dw_tap = dw_tap; d.ldt = ld_tap;
  const int rc = dwsep_launch(d, (hipStream_t)stream);
  if (rc == -1)
    return ghost::set_last_error(GHOST_EINVAL, std::string(
        "ghost_dwsep_block_nhwc: bad descriptor (f32 / bf16 / f16; Cin % 8; Cout % 16, and % 128 above 128; stride 1 "
        "or 2; Kpad % 32 >= Cin; 16-byte aligned pointers and leading dimensions >= C; no tap without Cout)"));
  return rc ? ghost::set_last_error(rc, std::string("ghost_dwsep_block_nhwc: launch failed")) : 0;
}
