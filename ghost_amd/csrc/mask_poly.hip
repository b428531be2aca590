// ghost_amd — the mask polygons on the device: face_mask_static's parameter choice (masks.py:43-65), expand_eyebrows
// (masks.py:5-20) and cv2.convexHull of the 106 landmarks (masks.py:31) for F faces in one launch, so that the chain
// landmarks -> masks -> blend needs no device -> host copy.  The yardstick is the host path of masks.hip
// (ghost_mask_polygons) and ghost_amd.inference.masks.mask_params: every output here is equal to theirs bit for bit.
//
// mask_poly_kernel, one workgroup of 128 threads (two waves) per face, everything in LDS:
//   1. thread p < 106 casts landmark p to int32 by truncation; thread 0 takes (erode, sigmaX, sigmaY) from params_in
//      or derives them from the x of six landmarks of two sets: fp32 subtractions and additions in numpy's order
//      (((d1 + d2) + d13), no multiply, so nothing to fuse), offset = right > left ? right : left (Python's max);
//   2. thread p expands its point if it is an eyebrow point: (int32)((double)top + (mod * 0.5) * (double)(top - bot))
//      with the product rounded before the add (fp contraction is off for that expression: hipcc contracts by default,
//      and the fused form gives another integer for about 0.3 % of the pairs a face produces), top and bot from the
//      un-expanded copy; the point becomes a 64-bit key (x, y), each half with its sign bit flipped so that unsigned
//      order is the signed lexicographic order; threads 106 .. 127 hold the largest key as padding;
//   3. bitonic sort of the 128 keys;
//   4. Andrew's monotone chain as the host walks it: thread 0 the lower chain over the ascending keys, thread 64 (the
//      other wave, so both run at once) the upper chain over the descending keys, each skipping equal neighbours and
//      popping while cross <= 0 (int64); two or fewer distinct points are emitted as they are;
//   5. thread v writes vertex v (lower chain without its last point, then the upper chain without its last), zeros
//      from nv on.
// Contract: landmarks finite with |v| <= 2^20 (beyond it the host's cast is undefined as well).  No index depends
// on a landmark's value, so values outside the contract give an unspecified polygon and no access outside the arrays.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ghost_amd.h"
#include "ghost_common.h"

namespace ghost {
int set_last_error(int rc, const char* msg);
}

namespace {

constexpr int kPts = 106;
constexpr int kMaxV = 128;   // masks.hip's kMaxV: vertices per face in poly
constexpr int kThreads = 128;
constexpr unsigned long long kPad = ~0ull;

// masks.hip's tables (expand_eyebrows, masks.py:9-16): top[s] moves away from bot[s], left brow then right brow
__constant__ int c_top[10] = {43, 48, 49, 51, 50, 102, 103, 104, 105, 101};
__constant__ int c_bot[10] = {35, 41, 40, 42, 39, 89, 95, 94, 96, 93};

struct PolyArgs {
  const float* lm;            // [F][106][2]
  const int32_t* params_in;   // [F][3] or null
  const float* ref;           // [n_ref][106][2] or null
  const int32_t* ref_index;   // [F]
  const float* tgt;           // [n_tgt][106][2] or null
  const int32_t* tgt_index;   // [F]
  int n_ref, n_tgt;
  int32_t* params_out;        // [F][3]
  int32_t* poly;              // [F][kMaxV][2]
  int32_t* nv;                // [F]
};

// top + m (top - bot) as the host evaluates it: a rounded product, then a rounded sum, truncated
__device__ __forceinline__ int expand(int top, int bot, double m) {
#pragma clang fp contract(off)
  const double prod = m * (double)(top - bot);
  const double sum = (double)top + prod;
  return (int)sum;
}

__device__ __forceinline__ unsigned long long pack_key(int x, int y) {
  return ((unsigned long long)((unsigned)x ^ 0x80000000u) << 32) | ((unsigned)y ^ 0x80000000u);
}
__device__ __forceinline__ int2 unpack_key(unsigned long long k) {
  return make_int2((int)((unsigned)(k >> 32) ^ 0x80000000u), (int)((unsigned)k ^ 0x80000000u));
}

__device__ __forceinline__ long long cross(int2 o, int2 a, int2 b) {
  return ((long long)a.x - o.x) * ((long long)b.y - o.y) - ((long long)a.y - o.y) * ((long long)b.x - o.x);
}

// one chain over the sorted keys from index i0 in steps of di (kThreads keys): the distinct points seen and the
// chain's length
__device__ int walk_chain(const unsigned long long* key, int i0, int di, int2* st, int* distinct) {
  int n = 0, m = 0;
  unsigned long long prev = kPad;
  for (int c = 0, i = i0; c < kThreads; ++c, i += di) {
    const unsigned long long k = key[i];
    if (k == kPad || k == prev) continue;
    prev = k;
    ++m;
    const int2 p = unpack_key(k);
    while (n >= 2 && cross(st[n - 2], st[n - 1], p) <= 0) --n;
    st[n++] = p;
  }
  *distinct = m;
  return n;
}

__global__ void __launch_bounds__(kThreads) mask_poly_kernel(const PolyArgs a) {
  __shared__ int li[kThreads][2];
  __shared__ unsigned long long key[kThreads];
  __shared__ int2 lower[kThreads], upper[kThreads];
  __shared__ int s_erode, s_m, s_nl, s_nu;
  const int f = blockIdx.x, tid = threadIdx.x;
  if (tid < kPts) {
    const float2 L = reinterpret_cast<const float2*>(a.lm)[(long)f * kPts + tid];
    li[tid][0] = (int)L.x;
    li[tid][1] = (int)L.y;
  }
  if (tid == 0) {
    int e = 0, sx = 0, sy = 0;
    if (a.params_in) {
      e = a.params_in[f * 3L];
      sx = a.params_in[f * 3L + 1];
      sy = a.params_in[f * 3L + 2];
    } else {
      const int ri = a.ref_index[f], ti = a.tgt_index[f];
      if (ri >= 0 && ri < a.n_ref && ti >= 0 && ti < a.n_tgt) {
        const float* A = a.ref + (long)ri * kPts * 2;
        const float* T = a.tgt + (long)ti * kPts * 2;
        const float left = ((A[2 * 1] - T[2 * 1]) + (A[2 * 2] - T[2 * 2])) + (A[2 * 13] - T[2 * 13]);
        const float right = ((T[2 * 17] - A[2 * 17]) + (T[2 * 18] - A[2 * 18])) + (T[2 * 29] - A[2 * 29]);
        const float off = right > left ? right : left;
        if (off > 6.f) { e = 15; sx = 15; sy = 10; }
        else if (off > 3.f) { e = 10; sx = 10; sy = 8; }
        else if (off < -3.f) { e = -5; sx = 5; sy = 10; }
        else { e = 5; sx = 5; sy = 5; }
      }   // an index outside its set: params stay 0 (no blur taps, an empty erode window)
    }
    a.params_out[f * 3L] = e;
    a.params_out[f * 3L + 1] = sx;
    a.params_out[f * 3L + 2] = sy;
    s_erode = e;
  }
  __syncthreads();
  unsigned long long k = kPad;
  if (tid < kPts) {
    const int erode = s_erode;
    const double m = (erode == 15 ? 2.7 : erode == -5 ? 0.5 : 2.0) * 0.5;
    int x = li[tid][0], y = li[tid][1];
#pragma unroll
    for (int s = 0; s < 10; ++s)
      if (c_top[s] == tid) {
        x = expand(x, li[c_bot[s]][0], m);
        y = expand(y, li[c_bot[s]][1], m);
      }
    k = pack_key(x, y);
  }
  key[tid] = k;
  __syncthreads();
  for (int size = 2; size <= kThreads; size <<= 1)
    for (int j = size >> 1; j > 0; j >>= 1) {
      const int p = tid ^ j;
      if (p > tid) {
        const unsigned long long u = key[tid], v = key[p];
        if ((u > v) == ((tid & size) == 0)) {
          key[tid] = v;
          key[p] = u;
        }
      }
      __syncthreads();
    }
  if (tid == 0) s_nl = walk_chain(key, 0, 1, lower, &s_m);
  if (tid == 64) {
    int m;
    s_nu = walk_chain(key, kThreads - 1, -1, upper, &m);
  }
  __syncthreads();
  const int m = s_m;
  const int nl = m <= 2 ? m : s_nl - 1, nu = m <= 2 ? 0 : s_nu - 1;
  int2 v = make_int2(0, 0);
  if (tid < nl) v = lower[tid];
  else if (tid < nl + nu) v = upper[tid - nl];
  reinterpret_cast<int2*>(a.poly)[(long)f * kMaxV + tid] = v;
  if (tid == 0) a.nv[f] = nl + nu;
}

}  // namespace

extern "C" int ghost_mask_polygons_dev(const float* landmarks, const int32_t* params_in, const float* landmarks_ref,
                                       const int32_t* ref_index, int n_ref, const float* landmarks_tgt,
                                       const int32_t* tgt_index, int n_tgt, int32_t* params_out, int32_t* poly,
                                       int32_t* nv, int F, void* stream) {
  if (F < 0) return ghost::set_last_error(GHOST_EINVAL, "ghost_mask_polygons_dev: F < 0");
  const bool any_ref = landmarks_ref || ref_index || landmarks_tgt || tgt_index;
  const bool all_ref = landmarks_ref && ref_index && landmarks_tgt && tgt_index;
  if ((params_in != nullptr) == any_ref || any_ref != all_ref)
    return ghost::set_last_error(GHOST_EINVAL, "ghost_mask_polygons_dev: give either params_in or all of landmarks_ref, "
                                               "ref_index, landmarks_tgt, tgt_index");
  if (all_ref && (n_ref <= 0 || n_tgt <= 0) && F > 0)
    return ghost::set_last_error(GHOST_EINVAL, "ghost_mask_polygons_dev: n_ref and n_tgt must be positive");
  if (F == 0) return 0;
  if (!landmarks || !params_out || !poly || !nv)
    return ghost::set_last_error(GHOST_EINVAL, "ghost_mask_polygons_dev: null argument");
  const PolyArgs a{landmarks, params_in, landmarks_ref, ref_index, landmarks_tgt, tgt_index, n_ref, n_tgt,
                   params_out, poly, nv};
  hipLaunchKernelGGL(mask_poly_kernel, dim3((unsigned)F), dim3(kThreads), 0, (hipStream_t)stream, a);
  const int rc = (int)hipGetLastError();
  return rc ? ghost::set_last_error(rc, "ghost_mask_polygons_dev launch failed") : 0;
}
