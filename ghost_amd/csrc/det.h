// ghost_amd — kernels of the SCRFD face detector (scrfd_10g_bnkps) outside the convolutions, det.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plan_log.h"

namespace ghost {

constexpr int kDetMaxCap = 4096;   // candidates per frame the sort holds (32 KiB of 64-bit keys in LDS)
constexpr int kDetLevels = 3;      // strides 8, 16, 32
constexpr int kDetStemC = 28;      // output channels of the first stem conv
constexpr int kDetTowerC = 80;     // channels of a head's tower
constexpr int kDetHeadOut = 30;    // a level's outputs per pixel: cls 2 | reg 8 | kps 20

// the three score / box / keypoint maps of one call, NHWC fp32: cls [F,Hl,Wl,2] (scores, after the sigmoid),
// reg [F,Hl,Wl,8], kps [F,Hl,Wl,20]; channel a*K + k belongs to anchor a.  Level l has stride 8 << l and
// Hl = Hd / stride, Wl = Wd / stride.
struct DetMaps {
  const float* cls[kDetLevels];
  const float* reg[kDetLevels];
  const float* kps[kDetLevels];
};

// cv2.resize(frame, (new_w, new_h)) INTER_LINEAR (ghost_resize_u8_linear's bytes) into the top-left of a zero canvas
// [F,Hd,Wd,3]
int det_letterbox(const uint8_t* frames, int64_t fstride, int F, int H, int W, int new_h, int new_w, uint8_t* canvas,
                  int Hd, int Wd, hipStream_t s);
// canvas uint8 [N,Hd,Wd,3] (bgr != 0: B,G,R order) -> (x - 127.5) / 128 in R,G,B order -> conv 3x3 s2 p1 3 -> 28
// (w [27][28] fp32, K = (ky*3 + kx)*3 + rgb channel) + bias + ReLU -> [N,Hd/2,Wd/2,28] in dt, rounded once
int det_stem(int dt, const uint8_t* canvas, int64_t bstride, int bgr, int N, int Hd, int Wd, const float* w,
             const float* bias, void* y, hipStream_t s);
// MaxPool 3x3 s2 p1 over [N,H,W,C] -> [N,H/2,W/2,C] (H, W even, C % 4 == 0); the padding never wins
int det_maxpool(int dt, const void* x, int N, int H, int W, int C, void* y, hipStream_t s);
// y [N,2h,2w,C] = round(y + nearest-x2(x [N,h,w,C])), in place, the sum in fp32
int det_upadd(int dt, const void* x, int N, int h, int w, int C, void* y, hipStream_t s);
// a level's three output convs as one 3x3 p1 conv 80 -> 30 in fp32 from fp32 weights w [720][30] (K = (ky*3 + kx)*80 +
// c; columns cls | reg | kps): v = (acc + bias[o]) * mul[o]; cls = sigmoid(v) [N,H,W,2], reg [N,H,W,8], kps [N,H,W,20],
// fp32 whatever dt, the storage type of x [N,H,W,80]
int det_head(int dt, const void* x, int N, int H, int W, const float* w, const float* bias, const float* mul, float* cls,
             float* reg, float* kps, hipStream_t s);
// bytes of det_decode_nms's workspace
size_t det_decode_workspace_bytes(int F, int cap);
// threshold + decode + ordered compaction (det_decode_kernel), then sort + greedy NMS (det_nms_kernel)
int det_decode_nms(const DetMaps& m, int F, int Hd, int Wd, float thresh, float det_scale, float nms_thresh, int cap,
                   int max_faces, float* det, float* kps, int32_t* anchor, int32_t* count, void* ws, size_t ws_bytes,
                   hipStream_t s);

}  // namespace ghost
