// ghost_amd — OpenCV's fixed point for warpAffine and resize on uint8 images, shared by the paste-back
// (blend.hip) and the forward alignment crop (align.hip).  Restated from OpenCV's published imgproc
// algorithms (imgwarp.cpp, resize.cpp); the CPU oracle is oracle/blend_ref.py.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// One rounding per operation, never fused: HIP's __fmul_rn / __dadd_rn ... are plain operators compiled with the
// translation unit's contraction mode, so after inlining the compiler fuses a*b + c into an FMA.  These carry no
// contract flag (the pragma applies to the operations written in their bodies).
__device__ __forceinline__ float f_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float f_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float f_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
__device__ __forceinline__ double d_mul(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ double d_add(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ double d_sub(double a, double b) {
#pragma clang fp contract(off)
  return a - b;
}

// cv2.resize INTER_LINEAR (resize.cpp): per axis the source index and two 11-bit weights,
// fx = (float)((d + 0.5) * scale - 0.5), clamped at the borders with the weight on the edge pixel.
struct RzTap {
  int s0, s1, w0, w1;
};
__device__ RzTap rz_tap(int d, int src_n, int dst_n) {
  const double scale = 1.0 / ((double)dst_n / (double)src_n);
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s0 = (int)floorf(f);
  f = f_sub(f, (float)s0);
  if (s0 < 0) { f = 0.f; s0 = 0; }
  if (s0 >= src_n - 1) { f = 0.f; s0 = src_n - 1; }
  RzTap t;
  t.s0 = s0;
  t.s1 = min(s0 + 1, src_n - 1);
  t.w0 = (int)rintf(f_mul(f_sub(1.f, f), 2048.f));
  t.w1 = (int)rintf(f_mul(f, 2048.f));
  return t;
}

// warpAffine's fixed point (imgwarp.cpp): the map A (the double inverse of the given matrix, host-side) sampled at
// X = (rint((A1 y + A2) 1024) + 16 + rint(A0 x 1024)) >> 5: pixel X >> 5, sub-pixel X & 31.  OpenCV keeps the
// x terms (adelta, bdelta) per destination column and the y terms (X0, Y0) per destination row.
struct CvWarp {
  int sx, sy;            // top-left source pixel
  float wx1, wy1;        // sub-pixel weights (multiples of 1/32)
};
__device__ __forceinline__ void cv_warp_col(const double* A, int x, long* adelta, long* bdelta) {
  *adelta = __double2ll_rn(d_mul(d_mul(A[0], (double)x), 1024.0));
  *bdelta = __double2ll_rn(d_mul(d_mul(A[3], (double)x), 1024.0));
}
__device__ __forceinline__ void cv_warp_row(const double* A, int y, long* X0, long* Y0) {
  *X0 = __double2ll_rn(d_mul(d_add(d_mul(A[1], (double)y), A[2]), 1024.0)) + 16;
  *Y0 = __double2ll_rn(d_mul(d_add(d_mul(A[4], (double)y), A[5]), 1024.0)) + 16;
}
__device__ CvWarp cv_warp_pos(const double* A, int x, int y) {
  long adelta, bdelta, X0, Y0;
  cv_warp_col(A, x, &adelta, &bdelta);
  cv_warp_row(A, y, &X0, &Y0);
  const long X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
  CvWarp w;
  w.sx = (int)(X >> 5);
  w.sy = (int)(Y >> 5);
  w.wx1 = (float)(X & 31) * (1.f / 32.f);
  w.wy1 = (float)(Y & 31) * (1.f / 32.f);
  return w;
}
// The 15-bit integer weight of one bilinear tap for uint8 sources: the float 32 x 32 table entry wy * wx,
// scaled by 2^15 and rounded (the four of a pixel sum to 2^15; the result is (sum + 2^14) >> 15).
__device__ __forceinline__ int cv_warp_weight_u8(float wy, float wx) {
  return (int)rintf(f_mul(f_mul(wy, wx), 32768.f));
}

}  // namespace
