// ghost_amd — the paste-back composite of one frame pixel (get_final_video, video_processing.py:218-227), shared by
// the full-frame kernel (blend.hip) and the ROI kernel that visits only a face's rectangle (roi.hip): one body, so the
// two write the same bytes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// Frame pixel (x, y), whose three bytes are at fr, sampled at m (x, y, 1) in the crop-space swap [Hs,Ws,3] and mask
// [Hs,Ws]: kornia.warp_affine (bilinear, zeros, align_corners=True) and frame = uint8(mask_t*swap_t + (1-mask_t)*frame).
// A pixel whose sample position has all four taps outside the crop keeps its value and is not written.
__device__ __forceinline__ void blend_pixel(int x, int y, const float* m, const uint8_t* sw8, int Hs, int Ws,
                                            const float* mk, uint8_t* fr) {
  const float ix = fmaf(m[0], (float)x, fmaf(m[1], (float)y, m[2]));
  const float iy = fmaf(m[3], (float)x, fmaf(m[4], (float)y, m[5]));
  if (!(ix > -1.f && ix < (float)Ws && iy > -1.f && iy < (float)Hs)) return;   // every tap outside
  // grid_sampler_2d bilinear (zeros padding): corner weights as PyTorch forms them
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy;
  const float nw = (fx + 1.f - ix) * (fy + 1.f - iy), ne = (ix - fx) * (fy + 1.f - iy);
  const float sw = (fx + 1.f - ix) * (iy - fy), se = (ix - fx) * (iy - fy);
  const int tx[4] = {x0, x0 + 1, x0, x0 + 1}, ty[4] = {y0, y0, y0 + 1, y0 + 1};
  const float tw[4] = {nw, ne, sw, se};
  float ms = 0.f, sv[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (tx[t] < 0 || tx[t] >= Ws || ty[t] < 0 || ty[t] >= Hs) continue;
    const long o = (long)ty[t] * Ws + tx[t];
    ms += mk[o] * tw[t];
#pragma unroll
    for (int c = 0; c < 3; ++c) sv[c] += (float)sw8[o * 3 + c] * tw[t];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = ms * sv[c] + (1.f - ms) * (float)fr[c];
    fr[c] = (uint8_t)(int)fminf(fmaxf(v, 0.f), 255.f);   // .type(torch.uint8) of a value in [0, 255]
  }
}

}  // namespace
