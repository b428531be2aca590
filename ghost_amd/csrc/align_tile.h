// ghost_amd — one 28 x 28 tile of cv2.warpAffine(src, M, (S, S), borderValue=0.0) and of the cv2.resize that follows,
// shared by the two sources the crops are taken from: whole device-resident frames (align.hip) and the per-face
// rectangles of the ROI path (roi.hip).  The arithmetic is the same code for both; only the tap lookup differs.
//
// A workgroup owns a 28 x 28 tile of the S x S crop: it gathers the tile (plus a one-pixel halo when a resize follows)
// from the source into LDS, stores it, and resizes out of LDS.  For R = 8 S / 7 output rows [8k, 8k+8) read crop rows
// [7k-1, 7k+7] (clamped at the image edges), so the 30 x 30 LDS tile yields a 32 x 32 output tile and the crop never
// makes a round trip through memory.  OpenCV's per-column (adelta, bdelta) and per-row (X0, Y0) terms and the resize
// taps are tables per tile; the per-pixel work is integer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cv_warp.h"

namespace {

constexpr int kTile = 28;              // crop pixels per tile side
constexpr int kSide = kTile + 2;       // with the halo
constexpr int kOut = 32;               // resized pixels per tile side (kTile * 8 / 7)
// LDS row: tile column c in [-1, 28] at byte 4 + 3c, so the interior starts dword-aligned
constexpr int kRow = 92;

struct AlignOut {
  int S;
  uint8_t* crops; int64_t cstride;
  uint8_t* resized; int64_t rstride; int R;
  int tiles;                           // per side
};

struct LocalTap {
  int o0, o1, w0, w1;                  // LDS offsets of the two taps (bytes for columns, rows for rows), weights
};

// Source::tap(tx, ty): the three bytes of source pixel (tx, ty), or nullptr where the constant 0 border applies.
// A = the double map of crop n, blockIdx.x = the tile; 256 threads.
template <class Source>
__device__ __forceinline__ void align_tile(const Source& src, const double* A, int n, const AlignOut& a) {
  __shared__ __align__(16) uint8_t tile[kSide * kRow];
  __shared__ long colA[kSide], colB[kSide], rowX[kSide], rowY[kSide];
  __shared__ LocalTap rzc[kOut], rzr[kOut];

  const int tid = threadIdx.x;
  const int tyi = blockIdx.x / a.tiles, txi = blockIdx.x - tyi * a.tiles;
  const int ox = txi * kTile, oy = tyi * kTile;          // crop coordinates of the tile's interior
  const int S = a.S;
  const int halo = a.resized ? 1 : 0;

  // ---- tables (one wave each) ----
  if (tid < kSide) {
    cv_warp_col(A, ox + tid - 1, &colA[tid], &colB[tid]);
  } else if (tid >= 64 && tid < 64 + kSide) {
    cv_warp_row(A, oy + tid - 64 - 1, &rowX[tid - 64], &rowY[tid - 64]);
  } else if (a.resized && tid >= 128 && tid < 128 + kOut) {
    const int d = min(txi * kOut + tid - 128, a.R - 1);
    const RzTap t = rz_tap(d, S, a.R);
    LocalTap l;
    l.o0 = 4 + 3 * min(max(t.s0 - ox, -1), kTile);
    l.o1 = 4 + 3 * min(max(t.s1 - ox, -1), kTile);
    l.w0 = t.w0;
    l.w1 = t.w1;
    rzc[tid - 128] = l;
  } else if (a.resized && tid >= 192 && tid < 192 + kOut) {
    const int d = min(tyi * kOut + tid - 192, a.R - 1);
    const RzTap t = rz_tap(d, S, a.R);
    LocalTap l;
    l.o0 = (min(max(t.s0 - oy, -1), kTile) + 1) * kRow;
    l.o1 = (min(max(t.s1 - oy, -1), kTile) + 1) * kRow;
    l.w0 = t.w0;
    l.w1 = t.w1;
    rzr[tid - 192] = l;
  }
  __syncthreads();

  // ---- gather: the warpAffine of the tile (and its halo) into LDS ----
  const int side = kTile + 2 * halo;
  for (int p = tid; p < side * side; p += 256) {
    const int r = p / side - halo, c = p - (p / side) * side - halo;   // tile coordinates in [-1, 28]
    const int cx = ox + c, cy = oy + r;
    if (cx < 0 || cx >= S || cy < 0 || cy >= S) continue;              // outside the crop: never read back
    const long X = (rowX[r + 1] + colA[c + 1]) >> 5, Y = (rowY[r + 1] + colB[c + 1]) >> 5;
    const long sx = X >> 5, sy = Y >> 5;
    const float fx = (float)(X & 31) * (1.f / 32.f), fy = (float)(Y & 31) * (1.f / 32.f);
    const float wx[2] = {f_sub(1.f, fx), fx}, wy[2] = {f_sub(1.f, fy), fy};
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int ky = 0; ky < 2; ++ky)
#pragma unroll
      for (int kx = 0; kx < 2; ++kx) {
        const uint8_t* s = src.tap(sx + kx, sy + ky);
        if (!s) continue;                                              // constant 0 border
        const int wi = cv_warp_weight_u8(wy[ky], wx[kx]);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) acc[ch] += (int)s[ch] * wi;
      }
    uint8_t* t = tile + (r + 1) * kRow + 4 + 3 * c;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int v = (acc[ch] + (1 << 14)) >> 15;
      t[ch] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
  }
  __syncthreads();

  // ---- the crop tile: packed dword stores where the rows allow it ----
  if (a.crops) {
    const int tw = min(kTile, S - ox), th = min(kTile, S - oy);
    uint8_t* dst = a.crops + (int64_t)n * a.cstride + ((int64_t)oy * S + ox) * 3;
    const int64_t pitch = (int64_t)S * 3;
    const bool packed = (((uintptr_t)a.crops | (uint64_t)a.cstride | (uint64_t)pitch | (uint64_t)(tw * 3)) & 3) == 0;
    if (packed) {
      const int ndw = tw * 3 / 4;
      for (int i = tid; i < th * ndw; i += 256) {
        const int r = i / ndw, j = i - r * ndw;
        *(uint32_t*)(dst + r * pitch + 4 * j) = *(const uint32_t*)(tile + (r + 1) * kRow + 4 + 4 * j);
      }
    } else {
      const int nb = tw * 3;
      for (int i = tid; i < th * nb; i += 256) {
        const int r = i / nb, j = i - r * nb;
        dst[r * pitch + j] = tile[(r + 1) * kRow + 4 + j];
      }
    }
  }

  // ---- cv2.resize out of LDS: one thread makes 4 pixels = 3 dwords ----
  if (a.resized) {
    const int R = a.R;
    const int ow = min(kOut, R - txi * kOut), oh = min(kOut, R - tyi * kOut);   // multiples of 8
    const int row = tid >> 3, q = (tid & 7) * 4;
    if (row < oh && q < ow) {
      const LocalTap ty = rzr[row];
      union { uint8_t b[12]; uint32_t d[3]; } o;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const LocalTap tx = rzc[q + k];
        const uint8_t* r0 = tile + ty.o0;
        const uint8_t* r1 = tile + ty.o1;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int D0 = (int)r0[tx.o0 + ch] * tx.w0 + (int)r0[tx.o1 + ch] * tx.w1;
          const int D1 = (int)r1[tx.o0 + ch] * tx.w0 + (int)r1[tx.o1 + ch] * tx.w1;
          int v = ((((D0 >> 4) * ty.w0) >> 16) + (((D1 >> 4) * ty.w1) >> 16) + 2) >> 2;
          o.b[k * 3 + ch] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
      }
      uint8_t* dst = a.resized + (int64_t)n * a.rstride + ((int64_t)(tyi * kOut + row) * R + txi * kOut + q) * 3;
      if ((((uintptr_t)a.resized | (uint64_t)a.rstride) & 3) == 0) {   // R is a multiple of 8: rows are dword-aligned
#pragma unroll
        for (int k = 0; k < 3; ++k) ((uint32_t*)dst)[k] = o.d[k];
      } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) dst[k] = o.b[k];
      }
    }
  }
}

}  // namespace
