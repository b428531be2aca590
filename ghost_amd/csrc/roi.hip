// ghost_amd — the ROI (region of interest) video path: the frames stay on the host and only each face's rectangle
// crosses the host link.
//
// cv2.warpAffine(frame, M, (S, S)) reads only the preimage of the S x S crop, and the paste-back composite
// uint8(mask_t*swap_t + (1-mask_t)*frame) (get_final_video, utils/inference/video_processing.py:218-227) returns the
// frame's own byte wherever mask_t == 0, so nothing outside the preimage of the crop square can change.  Per
// (identity, frame) that rectangle (ghost_amd/inference/roi.py: face_rois, plan_rois) is uploaded into one patch of
// a [Np,Ph,Pw,3] canvas; the crops are taken from the patches (the tile code of align.hip, align_tile.h), the swaps
// are composited into the patches (the pixel code of blend.hip, blend_pixel.h) and the rectangles are copied back.
// The results are the bytes of the full-frame path.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "align_tile.h"
#include "blend_pixel.h"
#include "ghost_amd.h"
#include "ghost_common.h"

namespace ghost {
int set_last_error(int rc, const char* msg);
}

namespace {

struct Patches {
  uint8_t* base; int64_t stride; int Np, Ph, Pw;
  const int32_t* rects;          // [Np][4] x0, y0, w, h in frame coordinates
  const int32_t* patch_index;    // [N]
};

// The rectangle of one patch, its extent clamped to the canvas: no read or write can leave the patch.
struct Rect {
  int x0, y0, w, h;
};
__device__ __forceinline__ Rect load_rect(const Patches& p, int pi) {
  const int32_t* r = p.rects + (int64_t)pi * 4;
  return Rect{r[0], r[1], min(max(r[2], 0), p.Pw), min(max(r[3], 0), p.Ph)};
}

struct RectSource {
  const uint8_t* base; int64_t pitch;    // the patch, bytes per canvas row
  Rect r;
  __device__ __forceinline__ const uint8_t* tap(long tx, long ty) const {
    tx -= r.x0;
    ty -= r.y0;
    if (tx < 0 || tx >= r.w || ty < 0 || ty >= r.h) return nullptr;   // the rectangle covers every in-frame tap
    return base + ty * pitch + tx * 3;
  }
};

struct AlignRoiArgs {
  Patches p;
  const double* maps;
  const int32_t* valid;
  AlignOut out;
};

__global__ void __launch_bounds__(256) align_crops_roi_kernel(const AlignRoiArgs a) {
  const int n = blockIdx.y;
  if (a.valid && !a.valid[n]) return;
  const int pi = a.p.patch_index[n];
  if (pi < 0 || pi >= a.p.Np) return;    // never read through a bad index
  const RectSource src{a.p.base + (int64_t)pi * a.p.stride, (int64_t)a.p.Pw * 3, load_rect(a.p, pi)};
  align_tile(src, a.maps + (int64_t)n * 6, n, a.out);
}

struct BlendRoiArgs {
  Patches p;
  const uint8_t* swaps; int64_t sstride; int Hs, Ws;
  const float* masks; int64_t mstride;
  const float* mats;      // [N][6] crop <- frame, in frame coordinates
  const int32_t* valid;   // [N] or null
};

__global__ void __launch_bounds__(256) blend_roi_kernel(const BlendRoiArgs a) {
  const int n = blockIdx.y;
  if (a.valid && !a.valid[n]) return;
  const int pi = a.p.patch_index[n];
  if (pi < 0 || pi >= a.p.Np) return;
  const Rect r = load_rect(a.p, pi);
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (int64_t)r.w * r.h) return;
  const int py = (int)(q / r.w), px = (int)(q - (int64_t)py * r.w);
  blend_pixel(r.x0 + px, r.y0 + py, a.mats + (int64_t)n * 6, a.swaps + n * a.sstride, a.Hs, a.Ws,
              a.masks + n * a.mstride, a.p.base + pi * a.p.stride + ((int64_t)py * a.p.Pw + px) * 3);
}

bool bad_canvas(const void* patches, int64_t patch_stride, int Np, int Ph, int Pw) {
  return !patches || Np <= 0 || Ph <= 0 || Pw <= 0 || patch_stride < (int64_t)Ph * Pw * 3;
}

}  // namespace

extern "C" int ghost_roi_copy_u8(uint8_t* patches, int64_t patch_stride, int Np, int Ph, int Pw,
                                 const int32_t* rects_host, uint8_t* const* frame_ptrs_host, int H, int W,
                                 int to_device, void* stream) {
  if (Np == 0) return 0;
  if (!rects_host || !frame_ptrs_host || !patches)
    return ghost::set_last_error(GHOST_EINVAL, "ghost_roi_copy_u8: null argument");
  if (bad_canvas(patches, patch_stride, Np, Ph, Pw) || H <= 0 || W <= 0)
    return ghost::set_last_error(GHOST_EINVAL, "ghost_roi_copy_u8: bad sizes");
  for (int p = 0; p < Np; ++p) {           // every rectangle before the first copy
    const int32_t* r = rects_host + (int64_t)p * 4;
    const int64_t x0 = r[0], y0 = r[1], w = r[2], h = r[3];
    if (w == 0 || h == 0) continue;
    if (w < 0 || h < 0 || x0 < 0 || y0 < 0 || x0 + w > W || y0 + h > H)
      return ghost::set_last_error(GHOST_EINVAL, "ghost_roi_copy_u8: a rectangle leaves the frame");
    if (w > Pw || h > Ph)
      return ghost::set_last_error(GHOST_EINVAL, "ghost_roi_copy_u8: a rectangle is larger than the canvas");
    if (!frame_ptrs_host[p]) return ghost::set_last_error(GHOST_EINVAL, "ghost_roi_copy_u8: null argument");
  }
  const size_t fpitch = (size_t)W * 3, ppitch = (size_t)Pw * 3;
  for (int p = 0; p < Np; ++p) {
    const int32_t* r = rects_host + (int64_t)p * 4;
    if (r[2] == 0 || r[3] == 0) continue;
    uint8_t* host = frame_ptrs_host[p] + ((int64_t)r[1] * W + r[0]) * 3;
    uint8_t* dev = patches + (int64_t)p * patch_stride;
    const size_t wb = (size_t)r[2] * 3, rows = (size_t)r[3];
    const hipError_t rc = to_device ? hipMemcpy2DAsync(dev, ppitch, host, fpitch, wb, rows, hipMemcpyHostToDevice,
                                                       (hipStream_t)stream)
                                    : hipMemcpy2DAsync(host, fpitch, dev, ppitch, wb, rows, hipMemcpyDeviceToHost,
                                                       (hipStream_t)stream);
    if (rc != hipSuccess) return ghost::set_last_error((int)rc, "ghost_roi_copy_u8: hipMemcpy2DAsync failed");
  }
  return 0;
}

extern "C" int ghost_align_crops_roi_u8(const uint8_t* patches, int64_t patch_stride, int Np, int Ph, int Pw,
                                        const int32_t* rects, const int32_t* patch_index, const double* maps,
                                        const int32_t* valid, int N, int S, uint8_t* crops, int64_t crop_stride,
                                        uint8_t* resized, int64_t resized_stride, int R, void* stream) {
  if (N == 0) return 0;
  if (!patches || !rects || !patch_index || !maps || (!crops && !resized))
    return ghost::set_last_error(GHOST_EINVAL, "ghost_align_crops_roi_u8: null argument");
  if (N < 0 || N > 65535 || bad_canvas(patches, patch_stride, Np, Ph, Pw) || S <= 0 ||
      (crops && crop_stride < (int64_t)S * S * 3))
    return ghost::set_last_error(GHOST_EINVAL, "ghost_align_crops_roi_u8: bad sizes");
  if (resized) {
    if (R <= 0 || resized_stride < (int64_t)R * R * 3)
      return ghost::set_last_error(GHOST_EINVAL, "ghost_align_crops_roi_u8: bad sizes");
    if (S % 7 != 0 || R != S / 7 * 8)
      return ghost::set_last_error(GHOST_EINVAL,
                                   "ghost_align_crops_roi_u8: the fused resize needs S % 7 == 0 and R == S / 7 * 8 "
                                   "(crop without it and call ghost_resize_u8_linear)");
  }
  const int tiles = (S + kTile - 1) / kTile;
  if ((int64_t)tiles * tiles > 0x7fffffffLL)
    return ghost::set_last_error(GHOST_EINVAL, "ghost_align_crops_roi_u8: bad sizes");
  AlignRoiArgs a{{const_cast<uint8_t*>(patches), patch_stride, Np, Ph, Pw, rects, patch_index}, maps, valid,
                 {S, crops, crop_stride, resized, resized_stride, resized ? R : 0, tiles}};
  dim3 grid((unsigned)(tiles * tiles), (unsigned)N);
  hipLaunchKernelGGL(align_crops_roi_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  const int rc = (int)hipGetLastError();
  return rc ? ghost::set_last_error(rc, "ghost_align_crops_roi_u8 launch failed") : 0;
}

extern "C" int ghost_blend_swaps_roi_u8(uint8_t* patches, int64_t patch_stride, int Np, int Ph, int Pw,
                                        const int32_t* rects, const int32_t* patch_index, int N, const uint8_t* swaps,
                                        int64_t swap_stride, int Hs, int Ws, const float* masks, int64_t mask_stride,
                                        const float* mats, const int32_t* valid, void* stream) {
  if (N == 0) return 0;
  if (!patches || !rects || !patch_index || !swaps || !masks || !mats)
    return ghost::set_last_error(GHOST_EINVAL, "ghost_blend_swaps_roi_u8: null argument");
  if (N < 0 || N > 65535 || bad_canvas(patches, patch_stride, Np, Ph, Pw) || Hs <= 0 || Ws <= 0 ||
      swap_stride < (int64_t)Hs * Ws * 3 || mask_stride < (int64_t)Hs * Ws || (int64_t)Ph * Pw > 0x7fffffffLL)
    return ghost::set_last_error(GHOST_EINVAL, "ghost_blend_swaps_roi_u8: bad sizes");
  BlendRoiArgs a{{patches, patch_stride, Np, Ph, Pw, rects, patch_index}, swaps, swap_stride, Hs, Ws, masks,
                 mask_stride, mats, valid};
  dim3 grid((unsigned)(((int64_t)Ph * Pw + 255) / 256), (unsigned)N);      // w h <= Ph Pw threads do the work
  hipLaunchKernelGGL(blend_roi_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  const int rc = (int)hipGetLastError();
  return rc ? ghost::set_last_error(rc, "ghost_blend_swaps_roi_u8 launch failed") : 0;
}
