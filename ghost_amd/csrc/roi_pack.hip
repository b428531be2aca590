// ghost_amd — packed ROI transfer: the rectangles of a plan cross the host link as one contiguous byte range per
// chunk, not as one 2-D copy per rectangle.
//
// roi.hip moves every rectangle with its own hipMemcpy2DAsync; 866 of them per direction run at 5-11 GB/s and are what
// bounds the ROI chain.  Here the host packs the rows of the rectangles [p0, p1) into a staging buffer
// (ghost_roi_pack_host, worker threads, no device pointer), one plain copy moves the chunk, and one kernel
// (ghost_roi_unpack_u8) spreads the packed rows over the canvas patches; the way back is the mirror image.  The layout
// is stated once, below, and used by all three entries.  The per-patch path of roi.hip is untouched.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <functional>
#include <thread>
#include <vector>

#include "ghost_amd.h"

namespace ghost {
int set_last_error(int rc, const char* msg);
}

namespace {

// ---- the packed layout -------------------------------------------------------------------------------------------
// Rectangle p = (x0, y0, w, h) holds h rows of pitch (3 w + 15) & ~15 bytes from byte offset_p; offset_0 = 0 and
// offset_{p+1} = offset_p + pitch_p h_p rounded up to 256; an empty rectangle takes no bytes.
constexpr int64_t kRowAlign = 16, kPatchAlign = 256;
__host__ __device__ __forceinline__ int64_t packed_pitch(int64_t w) {
  return (3 * w + (kRowAlign - 1)) & ~(kRowAlign - 1);
}
__host__ __device__ __forceinline__ int64_t packed_bytes_of(int64_t w, int64_t h) {
  return (w <= 0 || h <= 0) ? 0 : packed_pitch(w) * h;
}
inline int64_t next_offset(int64_t off, int64_t w, int64_t h) {
  return (off + packed_bytes_of(w, h) + (kPatchAlign - 1)) & ~(kPatchAlign - 1);
}

// ---- device ------------------------------------------------------------------------------------------------------
struct UnpackArgs {
  uint8_t* patches; int64_t stride; int Ph, Pw;
  const int32_t* rects;       // [Np][4]
  const int64_t* offsets;     // [Np]
  uint8_t* packed; int64_t packed_bytes;
  int p0;
  int dwords;                 // the canvas rows are dword-aligned
};

// One thread per 16-byte piece of a packed row: the packed side is one 16-byte access, the canvas side up to four
// dword accesses and the 1-3 bytes of a row's odd tail.  blockIdx.y = the patch, blockIdx.x covers the pieces of the
// largest rectangle the canvas can hold.
template <bool kToCanvas>
__global__ void __launch_bounds__(256) roi_unpack_kernel(const UnpackArgs a) {
  const int p = a.p0 + (int)blockIdx.y;
  const int32_t* r = a.rects + (int64_t)p * 4;
  const int64_t w_plan = r[2], h_plan = r[3];
  if (w_plan <= 0 || h_plan <= 0) return;
  const int64_t off = a.offsets[p], pitch = packed_pitch(w_plan);
  // the whole packed range of the patch, by the plan's own size, before any access
  if (off < 0 || (off & (kRowAlign - 1)) || off > a.packed_bytes || h_plan > (a.packed_bytes - off) / pitch)
    return;
  const int64_t w = min(w_plan, (int64_t)a.Pw), h = min(h_plan, (int64_t)a.Ph);     // never leave the patch
  const int64_t rowb = 3 * w, pieces = (rowb + 15) >> 4;
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= pieces * h) return;
  const int64_t py = q / pieces, b0 = (q - py * pieces) << 4;
  uint8_t* row = a.patches + (int64_t)p * a.stride + py * ((int64_t)a.Pw * 3) + b0;
  uint4* pk = reinterpret_cast<uint4*>(a.packed + off + py * pitch + b0);
  const int64_t left = rowb - b0;                      // bytes of the rectangle from here on, > 0
  if (kToCanvas) {
    const uint4 v = *pk;
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t n = left - 4 * j;
      if (n >= 4 && a.dwords) {
        reinterpret_cast<uint32_t*>(row)[j] = d[j];
      } else {
        for (int k = 0; k < 4 && k < n; ++k) row[4 * j + k] = (uint8_t)(d[j] >> (8 * k));
      }
    }
  } else {
    uint32_t d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t n = left - 4 * j;
      if (n >= 4 && a.dwords) {
        d[j] = reinterpret_cast<const uint32_t*>(row)[j];
      } else {
        d[j] = 0;                                      // row padding: unspecified, zero here
        for (int k = 0; k < 4 && k < n; ++k) d[j] |= (uint32_t)row[4 * j + k] << (8 * k);
      }
    }
    *pk = make_uint4(d[0], d[1], d[2], d[3]);          // inside the row's pitch
  }
}

// ---- host packer -------------------------------------------------------------------------------------------------
struct PackJob {
  uint8_t* staging;
  const int32_t* rects;
  const int64_t* offsets;
  uint8_t* const* frames;
  int p0, p1, W, to_staging;
  const int64_t* cum;          // [p1 - p0 + 1] bytes of the rectangles before patch p0 + i
};

// The rows whose first byte, counted over the rows of the range laid end to end, lies in [lo, hi).
void pack_rows(const PackJob& j, int64_t lo, int64_t hi) {
  const int n = j.p1 - j.p0;
  int i = 0;
  {                                                    // the patch that holds byte lo
    int a = 0, b = n;
    while (a < b) {
      const int m = (a + b) / 2;
      if (j.cum[m + 1] <= lo) a = m + 1; else b = m;
    }
    i = a;
  }
  for (; i < n && j.cum[i] < hi; ++i) {
    const int32_t* r = j.rects + (int64_t)(j.p0 + i) * 4;
    const int64_t w = r[2], h = r[3];
    if (w == 0 || h == 0) continue;
    const int64_t rowb = 3 * w, pitch = packed_pitch(w);
    const int64_t first = lo > j.cum[i] ? (lo - j.cum[i] + rowb - 1) / rowb : 0;
    const int64_t last = hi < j.cum[i + 1] ? (hi - j.cum[i] + rowb - 1) / rowb : h;
    uint8_t* f = j.frames[j.p0 + i] + ((int64_t)r[1] * j.W + r[0]) * 3;
    uint8_t* s = j.staging + j.offsets[j.p0 + i];
    for (int64_t y = first; y < last; ++y) {
      if (j.to_staging) memcpy(s + y * pitch, f + y * (int64_t)j.W * 3, (size_t)rowb);
      else memcpy(f + y * (int64_t)j.W * 3, s + y * pitch, (size_t)rowb);
    }
  }
}

constexpr int64_t kMinBytesPerWorker = 64 << 10;       // below this a thread costs more than it copies

}  // namespace

extern "C" int ghost_roi_packed_layout(const int32_t* rects_host, int Np, int64_t* offsets_host,
                                       int64_t* total_bytes) {
  if (Np < 0 || !total_bytes || (Np > 0 && (!rects_host || !offsets_host)))
    return ghost::set_last_error(GHOST_EINVAL, "ghost_roi_packed_layout: null argument");
  for (int p = 0; p < Np; ++p)
    if (rects_host[(int64_t)p * 4 + 2] < 0 || rects_host[(int64_t)p * 4 + 3] < 0)
      return ghost::set_last_error(GHOST_EINVAL, "ghost_roi_packed_layout: a rectangle has a negative size");
  int64_t off = 0;
  for (int p = 0; p < Np; ++p) {
    offsets_host[p] = off;
    off = next_offset(off, rects_host[(int64_t)p * 4 + 2], rects_host[(int64_t)p * 4 + 3]);
  }
  *total_bytes = off;
  return GHOST_OK;
}

extern "C" int ghost_roi_pack_host(uint8_t* staging, int64_t staging_bytes, const int32_t* rects_host,
                                   const int64_t* offsets_host, uint8_t* const* frame_ptrs_host, int Np, int p0, int p1,
                                   int H, int W, int to_staging, int threads) {
  if (Np < 0 || p0 < 0 || p1 < p0 || p1 > Np || H <= 0 || W <= 0 || staging_bytes < 0)
    return ghost::set_last_error(GHOST_EINVAL, "ghost_roi_pack_host: bad sizes");
  if (p0 == p1) return GHOST_OK;
  if (!staging || !rects_host || !offsets_host || !frame_ptrs_host)
    return ghost::set_last_error(GHOST_EINVAL, "ghost_roi_pack_host: null argument");
  const int n = p1 - p0;
  std::vector<int64_t> cum((size_t)n + 1, 0);
  int64_t rows = 0;
  for (int p = p0; p < p1; ++p) {          // every rectangle of the range before the first byte moves
    const int32_t* r = rects_host + (int64_t)p * 4;
    const int64_t x0 = r[0], y0 = r[1], w = r[2], h = r[3];
    cum[p - p0 + 1] = cum[p - p0];
    if (w == 0 || h == 0) continue;
    if (w < 0 || h < 0 || x0 < 0 || y0 < 0 || x0 + w > W || y0 + h > H)
      return ghost::set_last_error(GHOST_EINVAL, "ghost_roi_pack_host: a rectangle leaves the frame");
    if (!frame_ptrs_host[p]) return ghost::set_last_error(GHOST_EINVAL, "ghost_roi_pack_host: null argument");
    const int64_t off = offsets_host[p], bytes = packed_bytes_of(w, h);
    if (off < 0 || (off & (kRowAlign - 1)) || bytes > staging_bytes - off)
      return ghost::set_last_error(GHOST_EINVAL,
                                   "ghost_roi_pack_host: an offset is negative, not a multiple of 16 or leaves the "
                                   "staging buffer");
    if (p + 1 < Np && bytes > offsets_host[p + 1] - off)
      return ghost::set_last_error(GHOST_EINVAL, "ghost_roi_pack_host: the offsets overlap or descend");
    cum[p - p0 + 1] += 3 * w * h;
    rows += h;
  }
  const int64_t total = cum[n];
  if (total == 0) return GHOST_OK;
  int nt = threads == 0 ? 8 : (threads < 1 ? 1 : (threads > 16 ? 16 : threads));
  if ((int64_t)nt > total / kMinBytesPerWorker) nt = (int)(total / kMinBytesPerWorker);
  if ((int64_t)nt > rows) nt = (int)rows;
  if (nt < 1) nt = 1;
  const PackJob job{staging, rects_host, offsets_host, frame_ptrs_host, p0, p1, W, to_staging, cum.data()};
  if (nt == 1) {
    pack_rows(job, 0, total);
    return GHOST_OK;
  }
  // split by bytes, not by patch: one large face does not serialise the call.  Joined before the return.
  std::vector<std::thread> workers;
  workers.reserve((size_t)nt - 1);
  for (int t = 1; t < nt; ++t) {
    const int64_t lo = total * t / nt, hi = total * (t + 1) / nt;
    try {
      workers.emplace_back(pack_rows, std::cref(job), lo, hi);
    } catch (...) {                        // no thread to be had: this share is copied here
      pack_rows(job, lo, hi);
    }
  }
  pack_rows(job, 0, total / nt);
  for (std::thread& t : workers) t.join();
  return GHOST_OK;
}

extern "C" int ghost_roi_unpack_u8(uint8_t* patches, int64_t patch_stride, int Np, int Ph, int Pw, const int32_t* rects,
                                   const int64_t* offsets, uint8_t* packed, int64_t packed_bytes, int p0, int p1,
                                   int to_canvas, void* stream) {
  if (p0 == p1 && p0 >= 0 && p1 <= Np) return GHOST_OK;
  if (!patches || !rects || !offsets || !packed)
    return ghost::set_last_error(GHOST_EINVAL, "ghost_roi_unpack_u8: null argument");
  if (Np <= 0 || Ph <= 0 || Pw <= 0 || patch_stride < (int64_t)Ph * Pw * 3 || packed_bytes < 0 || p0 < 0 || p1 < p0 ||
      p1 > Np || p1 - p0 > 65535 || ((uintptr_t)packed & (kRowAlign - 1)))
    return ghost::set_last_error(GHOST_EINVAL, "ghost_roi_unpack_u8: bad sizes");
  const int64_t pieces = (packed_pitch(Pw) >> 4) * Ph;
  if ((pieces + 255) / 256 > 0x7fffffffLL) return ghost::set_last_error(GHOST_EINVAL, "ghost_roi_unpack_u8: bad sizes");
  const int dwords = !(((uintptr_t)patches | (uint64_t)patch_stride | (uint64_t)((int64_t)Pw * 3)) & 3);
  const UnpackArgs a{patches, patch_stride, Ph, Pw, rects, offsets, packed, packed_bytes, p0, dwords};
  const dim3 grid((unsigned)((pieces + 255) / 256), (unsigned)(p1 - p0));
  if (to_canvas) hipLaunchKernelGGL(roi_unpack_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(roi_unpack_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
  const int rc = (int)hipGetLastError();
  return rc ? ghost::set_last_error(rc, "ghost_roi_unpack_u8 launch failed") : GHOST_OK;
}
