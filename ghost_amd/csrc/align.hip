// ghost_amd — aligned face crops taken from device-resident frames (the step in front of the swap).
//
// crop_face (utils/inference/image_processing.py:18-19) and crop_frames_and_get_transforms
// (utils/inference/video_processing.py:134,163): align_img = cv2.warpAffine(frame, M, (S, S), borderValue=0.0),
// then resize_frames (video_processing.py:184): cv2.resize(align_img, (256, 256)).  Both restated from OpenCV's
// fixed point (cv_warp.h): bit-exact against oracle/blend_ref.warp_affine_cv(..., "constant") and
// resize_linear_u8 of it.
//
// One launch makes both outputs: a workgroup owns a 28 x 28 tile of the S x S crop (align_tile.h, which the ROI path's
// ghost_align_crops_roi_u8 shares); here a tap is a pixel of a whole frame.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "align_tile.h"
#include "cv_warp.h"
#include "ghost_amd.h"
#include "ghost_common.h"

namespace ghost {
int set_last_error(int rc, const char* msg);
}

namespace {

struct AlignArgs {
  const uint8_t* frames; int64_t fstride; int F, H, W;
  const int32_t* frame_index;
  const double* maps;
  const int32_t* valid;
  AlignOut out;
};

struct FrameSource {
  const uint8_t* base; int H, W;
  __device__ __forceinline__ const uint8_t* tap(long tx, long ty) const {
    if (tx < 0 || tx >= W || ty < 0 || ty >= H) return nullptr;
    return base + (ty * (int64_t)W + tx) * 3;
  }
};

__global__ void __launch_bounds__(256) align_crops_kernel(const AlignArgs a) {
  const int n = blockIdx.y;
  if (a.valid && !a.valid[n]) return;
  const int fi = a.frame_index[n];
  if (fi < 0 || fi >= a.F) return;     // never read through a bad index
  const FrameSource src{a.frames + (int64_t)fi * a.fstride, a.H, a.W};
  align_tile(src, a.maps + (int64_t)n * 6, n, a.out);
}

}  // namespace

extern "C" int ghost_align_crops_u8(const uint8_t* frames, int64_t frame_stride, int F, int H, int W,
                                    const int32_t* frame_index, const double* maps, const int32_t* valid, int N, int S,
                                    uint8_t* crops, int64_t crop_stride, uint8_t* resized, int64_t resized_stride, int R,
                                    void* stream) {
  if (N == 0) return 0;
  if (!frames || !frame_index || !maps || (!crops && !resized))
    return ghost::set_last_error(GHOST_EINVAL, "ghost_align_crops_u8: null argument");
  if (N < 0 || N > 65535 || F <= 0 || H <= 0 || W <= 0 || S <= 0 || frame_stride < (int64_t)H * W * 3 ||
      (crops && crop_stride < (int64_t)S * S * 3))
    return ghost::set_last_error(GHOST_EINVAL, "ghost_align_crops_u8: bad sizes");
  if (resized) {
    if (R <= 0 || resized_stride < (int64_t)R * R * 3)
      return ghost::set_last_error(GHOST_EINVAL, "ghost_align_crops_u8: bad sizes");
    if (S % 7 != 0 || R != S / 7 * 8)
      return ghost::set_last_error(GHOST_EINVAL,
                                   "ghost_align_crops_u8: the fused resize needs S % 7 == 0 and R == S / 7 * 8 "
                                   "(crop without it and call ghost_resize_u8_linear)");
  }
  const int tiles = (S + kTile - 1) / kTile;
  if ((int64_t)tiles * tiles > 0x7fffffffLL)
    return ghost::set_last_error(GHOST_EINVAL, "ghost_align_crops_u8: bad sizes");
  AlignArgs a{frames, frame_stride, F, H, W, frame_index, maps, valid,
              {S, crops, crop_stride, resized, resized_stride, resized ? R : 0, tiles}};
  dim3 grid((unsigned)(tiles * tiles), (unsigned)N);
  hipLaunchKernelGGL(align_crops_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  const int rc = (int)hipGetLastError();
  return rc ? ghost::set_last_error(rc, "ghost_align_crops_u8 launch failed") : 0;
}
