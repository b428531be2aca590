// ghost_amd — kernels of the SCRFD face detector (insightface scrfd_10g_bnkps) outside the convolutions.  NHWC, fp32
// arithmetic, 64-bit addressing, no scratch.
//
//   det_letterbox_kernel  cv2.resize of the frame (OpenCV's fixed point, cv_warp.h) into the top-left of a zero canvas
//   det_stem_kernel       uint8 canvas -> normalise, R,G,B order, conv 3x3 s2 3 -> 28 + bias + ReLU, all in fp32 VALU
//   det_maxpool_kernel    MaxPool 3x3 s2 p1
//   det_upadd_kernel      PAFPN's top-down step: y += nearest-x2(x), one rounding of the fp32 sum
//   det_head_kernel       the three output convs of one level as one 3x3 conv 80 -> 30 (cls 2 | reg 8 | kps 20) in fp32
//                         VALU from fp32 weights: bias, reg's bbox_scale, the sigmoid of cls, fp32 stores whatever the
//                         storage type of its input
//   det_decode_kernel     one workgroup per frame walks the anchors of the three levels in order: threshold, decode,
//                         and an ordered compaction by ballot + prefix counts (no atomics: slot k is the k-th candidate
//                         in anchor order, whatever the schedule)
//   det_nms_kernel        one workgroup per frame: bitonic sort of 64-bit keys (inverted score bits, slot) in LDS, then
//                         the greedy pass of insightface's nms(): for each surviving box in order, all threads clear
//                         the boxes it suppresses
// The float32 arithmetic of decode and NMS is insightface's numpy arithmetic operation by operation, with fp
// contraction off (a fused cx - d*s or area_i + area_j - w*h changes bits).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ghost_amd.h"
#include "cv_warp.h"
#include "det.h"
#include "ghost_common.h"

namespace ghost {
int set_last_error(int rc, const std::string& msg);   // aei_runtime.hip (ghost_last_error)
}
using namespace ghost;

namespace {

// four consecutive elements <-> fp32 (16 bytes of fp32, 8 bytes of a 16-bit type)
template <typename T> GHOST_DEV void load4_f(const T* p, float* v) {
  typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
  const u32x2 raw = *reinterpret_cast<const u32x2*>(p);
  const f32x2 a = unpack2<T>(raw.x), b = unpack2<T>(raw.y);
  v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
}
template <> GHOST_DEV void load4_f<float>(const float* p, float* v) { load16_f(p, v); }
template <typename T> GHOST_DEV void store4_f(T* p, const float* v) {
  typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
  *reinterpret_cast<u32x2*>(p) = u32x2{pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3])};
}
template <> GHOST_DEV void store4_f<float>(float* p, const float* v) { store16_f(p, v); }

__global__ void __launch_bounds__(256) det_letterbox_kernel(const uint8_t* __restrict__ src, long sstride, int H, int W,
                                                            int new_h, int new_w, uint8_t* __restrict__ dst, int Hd,
                                                            int Wd) {
  const long f = blockIdx.y;
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long)Hd * Wd) return;
  const int dy = (int)(p / Wd), dx = (int)(p - (long)dy * Wd);
  uint8_t* o = dst + (f * Hd * Wd + p) * 3;
  if (dy >= new_h || dx >= new_w) {   // the canvas padding is byte 0
    o[0] = o[1] = o[2] = 0;
    return;
  }
  const RzTap tx = rz_tap(dx, W, new_w), ty = rz_tap(dy, H, new_h);
  const uint8_t* sb = src + f * sstride;
  const uint8_t* r0 = sb + (long)ty.s0 * W * 3;
  const uint8_t* r1 = sb + (long)ty.s1 * W * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int D0 = (int)r0[tx.s0 * 3 + c] * tx.w0 + (int)r0[tx.s1 * 3 + c] * tx.w1;
    const int D1 = (int)r1[tx.s0 * 3 + c] * tx.w0 + (int)r1[tx.s1 * 3 + c] * tx.w1;
    int v = ((((D0 >> 4) * ty.w0) >> 16) + (((D1 >> 4) * ty.w1) >> 16) + 2) >> 2;
    o[c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
}

struct StemArgs {
  const uint8_t* x;
  long bstride;
  const float* w;
  const float* bias;
  void* y;
  long total;   // N * Ho * Wo
  int Hi, Wi, Ho, Wo, bgr;
};

constexpr int kSC = kDetStemC;

template <typename T>
__global__ void __launch_bounds__(256) det_stem_kernel(const StemArgs a) {
  __shared__ float ws[27 * kSC + kSC];
  for (int i = threadIdx.x; i < 27 * kSC; i += 256) ws[i] = a.w[i];
  if (threadIdx.x < kSC) ws[27 * kSC + threadIdx.x] = a.bias[threadIdx.x];
  __syncthreads();
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;   // one output pixel, 28 channels
  if (idx >= a.total) return;
  const long hwo = (long)a.Ho * a.Wo;
  const long n = idx / hwo;
  const long rem = idx - n * hwo;
  const int oy = (int)(rem / a.Wo), ox = (int)(rem - (long)oy * a.Wo);
  const uint8_t* __restrict__ src = a.x + n * a.bstride;
  float acc[kSC];
#pragma unroll
  for (int o = 0; o < kSC; ++o) acc[o] = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = 2 * oy - 1 + ky;
    if (iy < 0 || iy >= a.Hi) continue;   // the conv's zero padding lies beyond the canvas, and is of the normalised image
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = 2 * ox - 1 + kx;
      if (ix < 0 || ix >= a.Wi) continue;
      const uint8_t* px = src + ((long)iy * a.Wi + ix) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = ((float)px[a.bgr ? 2 - c : c] - 127.5f) * 0.0078125f;   // exact in fp32
        const float* wr = ws + ((ky * 3 + kx) * 3 + c) * kSC;
#pragma unroll
        for (int o = 0; o < kSC; ++o) acc[o] = fmaf(v, wr[o], acc[o]);
      }
    }
  }
#pragma unroll
  for (int o = 0; o < kSC; ++o) {
    const float t = acc[o] + ws[27 * kSC + o];
    acc[o] = t > 0.f ? t : 0.f;
  }
  T* y = reinterpret_cast<T*>(a.y) + idx * kSC;
#pragma unroll
  for (int o = 0; o < kSC; o += 4) store4_f(y + o, acc + o);
}

template <typename T>
__global__ void __launch_bounds__(256) det_maxpool_kernel(const T* __restrict__ x, T* __restrict__ y, long total, int H,
                                                          int W, int Ho, int Wo, int C) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;   // four channels of one output pixel
  if (idx >= total) return;
  const int c4 = C >> 2;
  const long p = idx / c4;
  const int c = (int)(idx - p * c4) << 2;
  const long hwo = (long)Ho * Wo;
  const long n = p / hwo;
  const long rem = p - n * hwo;
  const int oy = (int)(rem / Wo), ox = (int)(rem - (long)oy * Wo);
  float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = 2 * oy - 1 + ky;
    if (iy < 0 || iy >= H) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = 2 * ox - 1 + kx;
      if (ix < 0 || ix >= W) continue;
      float v[4];
      load4_f(x + ((n * H + iy) * W + ix) * C + c, v);
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
    }
  }
  store4_f(y + p * C + c, m);
}

template <typename T>
__global__ void __launch_bounds__(256) det_upadd_kernel(const T* __restrict__ x, T* __restrict__ y, long total, int h,
                                                        int w, int C) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;   // four channels of one pixel of y
  if (idx >= total) return;
  const int c4 = C >> 2;
  const long p = idx / c4;
  const int c = (int)(idx - p * c4) << 2;
  const long hw2 = 4L * h * w;
  const long n = p / hw2;
  const long rem = p - n * hw2;
  const int oy = (int)(rem / (2 * w)), ox = (int)(rem - (long)oy * (2 * w));
  float a[4], b[4];
  load4_f(y + p * C + c, a);
  load4_f(x + ((n * h + (oy >> 1)) * w + (ox >> 1)) * C + c, b);
#pragma unroll
  for (int e = 0; e < 4; ++e) a[e] += b[e];
  store4_f(y + p * C + c, a);
}

struct HeadArgs {
  const void* x;      // [N,H,W,80] in the storage type
  const float* w;     // [9*80][30], K = (ky*3 + kx)*80 + c; columns cls 0-1, reg 2-9, kps 10-29
  const float* b;     // [30] bias
  const float* m;     // [30] multiplier after the bias: bbox_scale on the reg columns, 1 elsewhere
  float* cls;         // [N,H,W,2] scores
  float* reg;         // [N,H,W,8]
  float* kps;         // [N,H,W,20]
  long total;         // N * H * W
  int H, W;
};

constexpr int kHC = kDetTowerC, kHO = kDetHeadOut;

// one thread per pixel, 30 accumulators; the weight index is the same for every lane, so the weights come through
// the scalar cache
template <typename T>
__global__ void __launch_bounds__(256) det_head_kernel(const HeadArgs a) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.total) return;
  const long hw = (long)a.H * a.W;
  const long n = idx / hw;
  const long rem = idx - n * hw;
  const int oy = (int)(rem / a.W), ox = (int)(rem - (long)oy * a.W);
  const T* __restrict__ x = reinterpret_cast<const T*>(a.x);
  const float* __restrict__ w = a.w;
  float acc[kHO];
#pragma unroll
  for (int o = 0; o < kHO; ++o) acc[o] = 0.f;
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = oy - 1 + ky;
    if (iy < 0 || iy >= a.H) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = ox - 1 + kx;
      if (ix < 0 || ix >= a.W) continue;
      const T* px = x + ((n * a.H + iy) * a.W + ix) * kHC;
      const float* wt = w + (ky * 3 + kx) * kHC * kHO;
      for (int c = 0; c < kHC; c += 4) {
        float v[4];
        load4_f(px + c, v);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int o = 0; o < kHO; ++o) acc[o] = fmaf(v[e], wt[(c + e) * kHO + o], acc[o]);
      }
    }
  }
#pragma unroll
  for (int o = 0; o < kHO; ++o) acc[o] = (acc[o] + a.b[o]) * a.m[o];
  a.cls[idx * 2] = sigmoidf_ref(acc[0]);
  a.cls[idx * 2 + 1] = sigmoidf_ref(acc[1]);
  store16_f(a.reg + idx * 8, acc + 2);
  store16_f(a.reg + idx * 8 + 4, acc + 6);
#pragma unroll
  for (int o = 0; o < 20; o += 4) store16_f(a.kps + idx * 20 + o, acc + 10 + o);
}

struct DecodeArgs {
  const float *cls0, *cls1, *cls2, *reg0, *reg1, *reg2, *kps0, *kps1, *kps2;
  int Hd, Wd, cap;
  float thresh, det_scale;
  float* c_score;     // [F][cap]
  int32_t* c_idx;     // [F][cap] concatenated anchor index
  float* c_box;       // [F][cap][4]
  float* c_kps;       // [F][cap][10]
  int32_t* count;     // [F][2]: (kept, candidates)
};

__global__ void __launch_bounds__(256) det_decode_kernel(const DecodeArgs a) {
  __shared__ int wsum[4];
  const long f = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int W0 = a.Wd >> 3, W1 = a.Wd >> 4, W2 = a.Wd >> 5;
  const int n0 = (a.Hd >> 3) * W0 * 2, n1 = (a.Hd >> 4) * W1 * 2, n2 = (a.Hd >> 5) * W2 * 2;
  const int A = n0 + n1 + n2;
  int base = 0;
  for (int start = 0; start < A; start += 256) {
    const int ai = start + tid;
    int l = 0, r = ai;
    if (r >= n0) { r -= n0; l = 1; }
    if (l == 1 && r >= n1) { r -= n1; l = 2; }
    const int nl = l == 0 ? n0 : l == 1 ? n1 : n2;
    const float* cls = l == 0 ? a.cls0 : l == 1 ? a.cls1 : a.cls2;
    float sc = 0.f;
    bool flag = false;
    if (ai < A) {
      sc = cls[f * nl + r];
      flag = sc >= a.thresh;   // false for a NaN, as numpy's comparison
    }
    const unsigned long long bal = __ballot(flag);
    const int pre = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wv] = __popcll(bal);
    __syncthreads();
    int off = base + pre, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = wsum[w];
      if (w < wv) off += c;
      tot += c;
    }
    if (flag && off < a.cap) {   // past capacity the first cap candidates in anchor order stand
      const int Wl = l == 0 ? W0 : l == 1 ? W1 : W2;
      const float* reg = l == 0 ? a.reg0 : l == 1 ? a.reg1 : a.reg2;
      const float* kps = l == 0 ? a.kps0 : l == 1 ? a.kps1 : a.kps2;
      const int pix = r >> 1, an = r & 1;
      const int y = pix / Wl, x = pix - y * Wl;
      const int s = 8 << l;
      const float fs = (float)s, cx = (float)(x * s), cy = (float)(y * s);
      const long pl = f * (nl >> 1) + pix;
      const float* rg = reg + pl * 8 + an * 4;
      const float* kp = kps + pl * 20 + an * 10;
      const long slot = f * a.cap + off;
      a.c_score[slot] = sc;
      a.c_idx[slot] = ai;
      float* bo = a.c_box + slot * 4;
      bo[0] = f_sub(cx, f_mul(rg[0], fs)) / a.det_scale;
      bo[1] = f_sub(cy, f_mul(rg[1], fs)) / a.det_scale;
      bo[2] = f_add(cx, f_mul(rg[2], fs)) / a.det_scale;
      bo[3] = f_add(cy, f_mul(rg[3], fs)) / a.det_scale;
      float* ko = a.c_kps + slot * 10;
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        ko[2 * i] = f_add(cx, f_mul(kp[2 * i], fs)) / a.det_scale;
        ko[2 * i + 1] = f_add(cy, f_mul(kp[2 * i + 1], fs)) / a.det_scale;
      }
    }
    base += tot;
    __syncthreads();   // wsum is rewritten by the next round
  }
  if (tid == 0) a.count[2 * f + 1] = base;
}

struct NmsArgs {
  const float* c_score;
  const int32_t* c_idx;
  const float* c_box;
  const float* c_kps;
  int cap, max_faces;
  float nms_thresh;
  float* det;         // [F][max_faces][5]
  float* kps;         // [F][max_faces][10]
  int32_t* anchor;    // [F][max_faces]
  int32_t* count;     // [F][2]
};

constexpr int kNmsThreads = 1024;
constexpr int kNmsPer = kDetMaxCap / kNmsThreads;   // boxes a thread keeps in registers

// np.maximum / np.minimum: a NaN operand is the result
GHOST_DEV float np_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
GHOST_DEV float np_min(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }

GHOST_DEV float box_area(const float* b) {
#pragma clang fp contract(off)
  const float w = (b[2] - b[0]) + 1.f;
  const float h = (b[3] - b[1]) + 1.f;
  return w * h;
}

// insightface's nms(): inter / (area_i + area_j - inter), every operation rounded on its own
GHOST_DEV float box_ovr(const float* bi, float ai, const float* bj, float aj) {
#pragma clang fp contract(off)
  const float xx1 = np_max(bi[0], bj[0]), yy1 = np_max(bi[1], bj[1]);
  const float xx2 = np_min(bi[2], bj[2]), yy2 = np_min(bi[3], bj[3]);
  const float w = np_max(0.f, (xx2 - xx1) + 1.f);
  const float h = np_max(0.f, (yy2 - yy1) + 1.f);
  const float inter = w * h;
  const float uni = (ai + aj) - inter;
  return inter / uni;
}

__global__ void __launch_bounds__(kNmsThreads) det_nms_kernel(const NmsArgs a) {
  __shared__ unsigned long long key[kDetMaxCap];
  __shared__ unsigned char alive[kDetMaxCap];
  const long f = blockIdx.x;
  const int tid = threadIdx.x;
  int n = a.count[2 * f + 1];
  if (n > a.cap) n = a.cap;
  int np = 2;
  while (np < n) np <<= 1;   // n <= cap, a power of two <= kDetMaxCap
  const long cb = f * a.cap;
  for (int i = tid; i < np; i += kNmsThreads) {
    unsigned long long k = ~0ull;
    if (i < n) {
      unsigned u = __float_as_uint(a.c_score[cb + i]);
      u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // unsigned order = float order
      k = ((unsigned long long)(~u) << 32) | (unsigned)i;   // score descending, then slot (= anchor index) ascending
    }
    key[i] = k;
  }
  __syncthreads();
  for (int size = 2; size <= np; size <<= 1)
    for (int j = size >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < np; t += kNmsThreads) {
        const int p = t ^ j;
        if (p > t) {
          const unsigned long long u = key[t], v = key[p];
          if ((u > v) == ((t & size) == 0)) {
            key[t] = v;
            key[p] = u;
          }
        }
      }
      __syncthreads();
    }
  float bx[kNmsPer][4], ar[kNmsPer];
#pragma unroll
  for (int k = 0; k < kNmsPer; ++k) {
    const int j = tid + k * kNmsThreads;
    bx[k][0] = bx[k][1] = bx[k][2] = bx[k][3] = ar[k] = 0.f;
    if (j < n) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(a.c_box + (cb + (unsigned)key[j]) * 4);
      bx[k][0] = b[0]; bx[k][1] = b[1]; bx[k][2] = b[2]; bx[k][3] = b[3];
      ar[k] = box_area(bx[k]);
      alive[j] = 1;
    }
  }
  __syncthreads();
  int kept = 0;
  for (int i = 0; i < n; ++i) {
    if (alive[i]) {   // the same byte for every thread: uniform
      const long si = cb + (unsigned)key[i];
      const f32x4 b = *reinterpret_cast<const f32x4*>(a.c_box + si * 4);
      const float bi[4] = {b[0], b[1], b[2], b[3]};
      const float ai = box_area(bi);
      if (kept < a.max_faces) {   // kept boxes past max_faces are dropped, and counted
        const long o = f * a.max_faces + kept;
        if (tid < 4) a.det[o * 5 + tid] = tid == 0 ? bi[0] : tid == 1 ? bi[1] : tid == 2 ? bi[2] : bi[3];
        else if (tid == 4) a.det[o * 5 + 4] = a.c_score[si];
        else if (tid < 15) a.kps[o * 10 + (tid - 5)] = a.c_kps[si * 10 + (tid - 5)];
        else if (tid == 15) a.anchor[o] = a.c_idx[si];
      }
      ++kept;
#pragma unroll
      for (int k = 0; k < kNmsPer; ++k) {
        const int j = tid + k * kNmsThreads;
        if (j > i && j < n && alive[j] && !(box_ovr(bi, ai, bx[k], ar[k]) <= a.nms_thresh)) alive[j] = 0;
      }
    }
    __syncthreads();
  }
  const int from = kept < a.max_faces ? kept : a.max_faces;
  for (int o = from + (tid >> 4); o < a.max_faces; o += kNmsThreads >> 4) {   // rows that hold no face are zero
    const long r = f * a.max_faces + o;
    const int e = tid & 15;
    if (e < 5) a.det[r * 5 + e] = 0.f;
    else if (e < 15) a.kps[r * 10 + (e - 5)] = 0.f;
    else a.anchor[r] = -1;
  }
  if (tid == 0) a.count[2 * f] = kept;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool dt_ok(int dt) { return dt == GHOST_F32 || dt == GHOST_BF16 || dt == GHOST_F16; }
bool size_ok(int Hd, int Wd) { return Hd > 0 && Wd > 0 && Hd % 32 == 0 && Wd % 32 == 0 && Hd <= 8192 && Wd <= 8192; }
size_t up256(size_t v) { return (v + 255) & ~size_t(255); }

#define DET_DISPATCH(dt, kernel, grid, ...)                                                             \
  do {                                                                                                  \
    if (dt == GHOST_F32) hipLaunchKernelGGL(kernel<float>, grid, dim3(256), 0, s, __VA_ARGS__);         \
    else if (dt == GHOST_BF16) hipLaunchKernelGGL(kernel<bf16>, grid, dim3(256), 0, s, __VA_ARGS__);    \
    else hipLaunchKernelGGL(kernel<_Float16>, grid, dim3(256), 0, s, __VA_ARGS__);                      \
  } while (0)

}  // namespace

namespace ghost {

int det_letterbox(const uint8_t* frames, int64_t fstride, int F, int H, int W, int new_h, int new_w, uint8_t* canvas,
                  int Hd, int Wd, hipStream_t s) {
  if (!frames || !canvas || F <= 0 || F > 65535 || H <= 0 || W <= 0 || new_h <= 0 || new_w <= 0 || new_h > Hd ||
      new_w > Wd || fstride < (int64_t)H * W * 3)
    return -1;
  GHOST_PLAN_LOG("det_letterbox");
  const dim3 grid((unsigned)(((long)Hd * Wd + 255) / 256), (unsigned)F);
  hipLaunchKernelGGL(det_letterbox_kernel, grid, dim3(256), 0, s, frames, (long)fstride, H, W, new_h, new_w, canvas, Hd,
                     Wd);
  return (int)hipGetLastError();
}

int det_stem(int dt, const uint8_t* canvas, int64_t bstride, int bgr, int N, int Hd, int Wd, const float* w,
             const float* bias, void* y, hipStream_t s) {
  if (!dt_ok(dt) || !canvas || !w || !bias || !y || N <= 0 || Hd <= 0 || Wd <= 0 || Hd % 2 || Wd % 2 || !aligned16(y) ||
      bstride < (int64_t)Hd * Wd * 3)
    return -1;
  StemArgs a{canvas, (long)bstride, w, bias, y, (long)N * (Hd / 2) * (Wd / 2), Hd, Wd, Hd / 2, Wd / 2, bgr ? 1 : 0};
  const long nb = (a.total + 255) / 256;
  if (nb > 0x7fffffffL) return -1;
  GHOST_PLAN_LOG("det_stem t=%s k=3 s=2 bgr=%d", plan_dt(dt), a.bgr);
  DET_DISPATCH(dt, det_stem_kernel, dim3((unsigned)nb), a);
  return (int)hipGetLastError();
}

int det_maxpool(int dt, const void* x, int N, int H, int W, int C, void* y, hipStream_t s) {
  if (!dt_ok(dt) || !x || !y || N <= 0 || H <= 0 || W <= 0 || H % 2 || W % 2 || C <= 0 || C % 4 || !aligned16(x) ||
      !aligned16(y))
    return -1;
  const long total = (long)N * (H / 2) * (W / 2) * (C / 4);
  const long nb = (total + 255) / 256;
  if (nb > 0x7fffffffL) return -1;
  GHOST_PLAN_LOG("det_maxpool t=%s k=3 s=2", plan_dt(dt));
  if (dt == GHOST_F32)
    hipLaunchKernelGGL(det_maxpool_kernel<float>, dim3((unsigned)nb), dim3(256), 0, s, (const float*)x, (float*)y, total,
                       H, W, H / 2, W / 2, C);
  else if (dt == GHOST_BF16)
    hipLaunchKernelGGL(det_maxpool_kernel<bf16>, dim3((unsigned)nb), dim3(256), 0, s, (const bf16*)x, (bf16*)y, total, H,
                       W, H / 2, W / 2, C);
  else
    hipLaunchKernelGGL(det_maxpool_kernel<_Float16>, dim3((unsigned)nb), dim3(256), 0, s, (const _Float16*)x,
                       (_Float16*)y, total, H, W, H / 2, W / 2, C);
  return (int)hipGetLastError();
}

int det_upadd(int dt, const void* x, int N, int h, int w, int C, void* y, hipStream_t s) {
  if (!dt_ok(dt) || !x || !y || N <= 0 || h <= 0 || w <= 0 || C <= 0 || C % 4 || !aligned16(x) || !aligned16(y))
    return -1;
  const long total = (long)N * 4 * h * w * (C / 4);
  const long nb = (total + 255) / 256;
  if (nb > 0x7fffffffL) return -1;
  GHOST_PLAN_LOG("det_upadd t=%s", plan_dt(dt));
  if (dt == GHOST_F32)
    hipLaunchKernelGGL(det_upadd_kernel<float>, dim3((unsigned)nb), dim3(256), 0, s, (const float*)x, (float*)y, total, h,
                       w, C);
  else if (dt == GHOST_BF16)
    hipLaunchKernelGGL(det_upadd_kernel<bf16>, dim3((unsigned)nb), dim3(256), 0, s, (const bf16*)x, (bf16*)y, total, h, w,
                       C);
  else
    hipLaunchKernelGGL(det_upadd_kernel<_Float16>, dim3((unsigned)nb), dim3(256), 0, s, (const _Float16*)x, (_Float16*)y,
                       total, h, w, C);
  return (int)hipGetLastError();
}

int det_head(int dt, const void* x, int N, int H, int W, const float* w, const float* bias, const float* mul, float* cls,
             float* reg, float* kps, hipStream_t s) {
  if (!dt_ok(dt) || !x || !w || !bias || !mul || !cls || !reg || !kps || N <= 0 || H <= 0 || W <= 0 || !aligned16(x) ||
      !aligned16(reg) || !aligned16(kps))
    return -1;
  HeadArgs a{x, w, bias, mul, cls, reg, kps, (long)N * H * W, H, W};
  const long nb = (a.total + 255) / 256;
  if (nb > 0x7fffffffL) return -1;
  GHOST_PLAN_LOG("det_head t=%s k=3 cout=30", plan_dt(dt));
  DET_DISPATCH(dt, det_head_kernel, dim3((unsigned)nb), a);
  return (int)hipGetLastError();
}

size_t det_decode_workspace_bytes(int F, int cap) {
  const size_t n = (size_t)F * cap;
  return up256(n * 4) * 2 + up256(n * 16) + up256(n * 40) + 256;
}

int det_decode_nms(const DetMaps& m, int F, int Hd, int Wd, float thresh, float det_scale, float nms_thresh, int cap,
                   int max_faces, float* det, float* kps, int32_t* anchor, int32_t* count, void* ws, size_t ws_bytes,
                   hipStream_t s) {
  if (F <= 0 || F > 65535 || !size_ok(Hd, Wd) || cap < 2 || cap > kDetMaxCap || (cap & (cap - 1)) || max_faces <= 0 ||
      !(det_scale > 0.f) || !det || !kps || !anchor || !count || !ws || ws_bytes < det_decode_workspace_bytes(F, cap))
    return -1;
  for (int l = 0; l < kDetLevels; ++l)
    if (!m.cls[l] || !m.reg[l] || !m.kps[l]) return -1;
  const size_t n = (size_t)F * cap;
  char* p = (char*)up256((size_t)(uintptr_t)ws);
  float* c_score = (float*)p;      p += up256(n * 4);
  int32_t* c_idx = (int32_t*)p;    p += up256(n * 4);
  float* c_box = (float*)p;        p += up256(n * 16);
  float* c_kps = (float*)p;
  GHOST_PLAN_LOG("det_decode cap=%d", cap);
  const DecodeArgs d{m.cls[0], m.cls[1], m.cls[2], m.reg[0], m.reg[1], m.reg[2], m.kps[0], m.kps[1], m.kps[2],
                     Hd, Wd, cap, thresh, det_scale, c_score, c_idx, c_box, c_kps, count};
  hipLaunchKernelGGL(det_decode_kernel, dim3((unsigned)F), dim3(256), 0, s, d);
  GHOST_PLAN_LOG("det_nms cap=%d", cap);
  const NmsArgs q{c_score, c_idx, c_box, c_kps, cap, max_faces, nms_thresh, det, kps, anchor, count};
  hipLaunchKernelGGL(det_nms_kernel, dim3((unsigned)F), dim3(kNmsThreads), 0, s, q);
  return (int)hipGetLastError();
}

}  // namespace ghost

static int det_op(int rc, const char* what, const char* contract) {
  if (rc == -1) return ghost::set_last_error(GHOST_EINVAL, std::string(what) + ": bad argument (" + contract + ")");
  return rc ? ghost::set_last_error(rc, std::string(what) + ": launch failed") : 0;
}

extern "C" int ghost_det_letterbox_u8(const uint8_t* frames, int64_t frame_stride, int F, int H, int W, int new_h,
                                      int new_w, uint8_t* canvas, int Hd, int Wd, void* stream) {
  return det_op(det_letterbox(frames, frame_stride, F, H, W, new_h, new_w, canvas, Hd, Wd, (hipStream_t)stream),
                "ghost_det_letterbox_u8", "F in 1..65535, 0 < new_h <= Hd, 0 < new_w <= Wd, frame_stride >= H*W*3");
}

extern "C" int ghost_det_stem_u8(int dtype, const uint8_t* canvas, int64_t batch_stride, int bgr, int N, int Hd, int Wd,
                                 const float* w, const float* bias, void* y, void* stream) {
  return det_op(det_stem(dtype, canvas, batch_stride, bgr, N, Hd, Wd, w, bias, y, (hipStream_t)stream),
                "ghost_det_stem_u8", "f32 / bf16 / f16; even Hd, Wd; batch_stride >= Hd*Wd*3; y 16-byte aligned");
}

extern "C" int ghost_maxpool3x3s2_nhwc(int dtype, const void* x, int N, int H, int W, int C, void* y, void* stream) {
  return det_op(det_maxpool(dtype, x, N, H, W, C, y, (hipStream_t)stream), "ghost_maxpool3x3s2_nhwc",
                "f32 / bf16 / f16; even H, W; C % 4 == 0; 16-byte aligned pointers");
}

extern "C" int ghost_upsample2x_add_nhwc(int dtype, const void* x, int N, int h, int w, int C, void* y, void* stream) {
  return det_op(det_upadd(dtype, x, N, h, w, C, y, (hipStream_t)stream), "ghost_upsample2x_add_nhwc",
                "f32 / bf16 / f16; C % 4 == 0; 16-byte aligned pointers");
}

extern "C" int ghost_det_head_nhwc(int dtype, const void* x, int N, int H, int W, const float* w, const float* bias,
                                   const float* mul, float* cls, float* reg, float* kps, void* stream) {
  return det_op(det_head(dtype, x, N, H, W, w, bias, mul, cls, reg, kps, (hipStream_t)stream), "ghost_det_head_nhwc",
                "f32 / bf16 / f16 input of 80 channels; 16-byte aligned x, reg and kps");
}

extern "C" int64_t ghost_det_decode_workspace_bytes(int F, int cap) {
  if (F < 0 || F > 65535 || cap < 2 || cap > kDetMaxCap || (cap & (cap - 1)))
    return ghost::set_last_error(GHOST_EINVAL, std::string("ghost_det_decode_workspace_bytes: bad argument"));
  return (int64_t)det_decode_workspace_bytes(F, cap);
}

extern "C" int ghost_det_decode_nms(const float* const* cls, const float* const* reg, const float* const* kps_maps, int F,
                                    int Hd, int Wd, float thresh, float det_scale, float nms_thresh, int cap,
                                    int max_faces, float* det, float* kps, int32_t* anchor, int32_t* count, void* ws,
                                    int64_t ws_bytes, void* stream) {
  if (F == 0) return 0;
  if (!cls || !reg || !kps_maps || ws_bytes < 0)
    return ghost::set_last_error(GHOST_EINVAL, std::string("ghost_det_decode_nms: null argument"));
  DetMaps m;
  for (int l = 0; l < kDetLevels; ++l) { m.cls[l] = cls[l]; m.reg[l] = reg[l]; m.kps[l] = kps_maps[l]; }
  return det_op(det_decode_nms(m, F, Hd, Wd, thresh, det_scale, nms_thresh, cap, max_faces, det, kps, anchor, count, ws,
                               (size_t)ws_bytes, (hipStream_t)stream),
                "ghost_det_decode_nms",
                "F in 1..65535; Hd, Wd multiples of 32; cap a power of two in 2..4096; max_faces > 0; det_scale > 0; "
                "workspace of ghost_det_decode_workspace_bytes");
}
