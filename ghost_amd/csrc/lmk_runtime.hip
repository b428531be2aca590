// ghost_amd — the 106-point face landmark network (insightface 2d106det) on gfx950, C ABI in include/ghost_amd.h.
//
// GHOST calls it as handler.get_without_detection_without_transform(crop224) for every swapped face and for the
// first target crop of each run of frames (utils/inference/video_processing.py:218-223, coordinate_reg/
// image_infer.py:141-157).  The network is coordinate_reg/model/2d106det-symbol.json: (x - 127.5) / 128 on a 192 x 192
// RGB crop, conv_1 3x3/s2 3 -> 16, thirteen depthwise-separable blocks conv_2 .. conv_14, conv_15 3x3/s2 512 -> 64,
// Flatten (NCHW order) and FullyConnected(212); every Convolution is followed by BatchNorm(fix_gamma) and a
// per-channel PReLU.  No checkpoint and no mxnet are available offline: parity against mxnet is unpinned.
//
// Plan (NHWC, one stream):
//   warp   ghost_align_crops_u8 of the N crops as N frames, M = [[0.57142857, 0, 32], [0, 0.57142857, 32]], S = 192
//   stem   lmk_stem (uint8 -> fp32 normalise -> conv + BN + PReLU)
//   k      ghost_dwsep_block (fused) | depthwise-only launch + the implicit-GEMM 1x1 conv (unfused_mask())
//   c15    the implicit-GEMM 3x3/s2 conv, BN + PReLU epilogue
//   head   lmk_head: fc in fp32 over the stored conv_15 values + the landmark transform
#include <string>
#include <vector>

#include "ghost_amd.h"
#include "ghost_common.h"
#include "conv_igemm.h"
#include "lmk.h"
#include "plan_ctx.h"

using namespace ghost;

static int lmk_fail(int rc, const std::string& msg) { return ghost::set_last_error(rc, msg); }

// diagnostic taps (ghost_lmk_set_taps): the stored outputs of conv_2, conv_7, conv_14 and conv_15
struct ghost_lmk : Handle {
  static constexpr int kTaps = 4;
  static constexpr bool kAligned16 = true;
};

namespace {

struct Block { int k, cin, cout, stride, hin; };
const Block kBlocks[13] = {{2, 16, 32, 1, 96},    {3, 32, 64, 2, 96},    {4, 64, 64, 1, 48},   {5, 64, 128, 2, 48},
                           {6, 128, 128, 1, 24},  {7, 128, 256, 2, 24},  {8, 256, 256, 1, 12}, {9, 256, 256, 1, 12},
                           {10, 256, 256, 1, 12}, {11, 256, 256, 1, 12}, {12, 256, 256, 1, 12}, {13, 256, 512, 2, 12},
                           {14, 512, 512, 1, 6}};
constexpr int kIn = 192, kCrop = 224, kOut = 212;
// image_infer.py:13: the module constant the 224 crop is warped with
const double kM[6] = {0.57142857, 0.0, 32.0, 0.0, 0.57142857, 32.0};

// bit k set: conv_k runs as the depthwise-only launch + the implicit-GEMM 1x1 instead of the fused block
// (profiles/landmark_ab.txt: the fused block is chosen wherever it wins by more than the spread)
static int unfused_mask() {
  static const int v = GHOST_KNOB("GHOST_LMK_UNFUSED", 0);
  return v;
}

typedef HandleCtx<ghost_lmk> LmkCtx;

std::string cname(int k) { return "c" + std::to_string(k); }

// x192: uint8 [N,192,192,3], bstride bytes apart
void lmk_plan(LmkCtx& c, const uint8_t* x192, int64_t bstride, int bgr, int N, float* pred, float* lmk) {
  ghost_lmk* h = c.h;
  const int es = h->esz, dt = h->dt;
  const size_t big = (size_t)N * 96 * 96 * 32 * es;   // conv_2's output, the largest activation
  void* X[2] = {c.alloc(big), c.alloc(big)};
  void* D = c.alloc(big / 2);                         // depthwise output of an unfused block (at most 96 x 96 x 16)
  int cur = 0;
  {
    const float* w = c.F("stem.w");
    const float *sc = c.F("stem.scale"), *sh = c.F("stem.shift"), *pr = c.F("stem.prelu");
    if (c.ok() && !c.dry) c.check(lmk_stem(dt, x192, bstride, bgr, N, kIn, kIn, w, sc, sh, pr, X[0], c.s), "stem");
  }
  for (const Block& b : kBlocks) {
    const std::string nm = cname(b.k);
    DwsepDesc d;
    d.dt = dt; d.x = X[cur]; d.B = N; d.H = d.W = b.hin; d.Cin = d.ldx = b.cin; d.stride = b.stride;
    d.dw_w = c.F(nm + ".dw.w"); d.dw_scale = c.F(nm + ".dw.scale"); d.dw_shift = c.F(nm + ".dw.shift");
    d.dw_prelu = c.F(nm + ".dw.prelu");
    const void* pw = c.W(nm + ".pw.w");
    const float *sc = c.F(nm + ".pw.scale"), *sh = c.F(nm + ".pw.shift"), *pr = c.F(nm + ".pw.prelu");
    const int ho = b.hin / b.stride;
    if (unfused_mask() >> b.k & 1) {
      d.y = D; d.ldy = b.cin;
      ConvDesc g = conv_desc(dt, dt, D, N, ho, b.cin, b.cin, pw, b.cout, CONV_FWD, 1, 1, 0, X[cur ^ 1], b.cout);
      g.scale = sc; g.shift = sh; g.slope = 1.f; g.prelu = pr;
      if (c.dry) c.need_scratch(conv_workspace_bytes(g));
      else if (c.ok()) {
        c.check(dwsep_launch(d, c.s), nm + " depthwise");
        if (c.ok()) c.check(conv_launch(g, c.scratch, c.scratch_cap, c.s), nm + " pointwise");
      }
    } else {
      d.w = pw; d.Cout = b.cout; d.Kpad = rup(b.cin, 32); d.scale = sc; d.shift = sh; d.prelu = pr;
      d.y = X[cur ^ 1]; d.ldy = b.cout;
      if (!c.dry && c.ok()) c.check(dwsep_launch(d, c.s), nm);
    }
    cur ^= 1;
    const size_t bytes = (size_t)N * ho * ho * b.cout * es;
    if (b.k == 2) c.tap(0, X[cur], bytes);
    if (b.k == 7) c.tap(1, X[cur], bytes);
    if (b.k == 14) c.tap(2, X[cur], bytes);
  }
  {
    ConvDesc g = conv_desc(dt, dt, X[cur], N, 6, 512, 512, c.W("c15.w"), 64, CONV_FWD, 3, 2, 1, X[cur ^ 1], 64);
    g.scale = c.F("c15.scale"); g.shift = c.F("c15.shift"); g.slope = 1.f; g.prelu = c.F("c15.prelu");
    if (c.dry) c.need_scratch(conv_workspace_bytes(g));
    else if (c.ok()) c.check(conv_launch(g, c.scratch, c.scratch_cap, c.s), "c15");
    cur ^= 1;
    c.tap(3, X[cur], (size_t)N * 9 * 64 * es);
  }
  const float *fw = c.F("fc.w"), *fb = c.F("fc.bias");
  if (!c.dry && c.ok()) c.check(lmk_head(dt, X[cur], N, 576, kOut, fw, fb, pred, lmk, c.s), "head");
}

void declare(ghost_lmk* h) {
  auto add = [&](const std::string& s) { h->slots[s] = nullptr; };
  auto bnp = [&](const std::string& s) { add(s + ".scale"); add(s + ".shift"); add(s + ".prelu"); };
  add("stem.w"); bnp("stem");
  for (const Block& b : kBlocks) {
    add(cname(b.k) + ".dw.w"); bnp(cname(b.k) + ".dw");
    add(cname(b.k) + ".pw.w"); bnp(cname(b.k) + ".pw");
  }
  add("c15.w"); bnp("c15");
  add("fc.w"); add("fc.bias");
}

// the regions in front of the plan's: the warped crops, frame_index and maps of the warp
struct Front { uint8_t* x192; int32_t* fi; double* maps; };
Front front(LmkCtx& c, int N) {
  Front f;
  f.x192 = (uint8_t*)c.alloc((size_t)N * kIn * kIn * 3);
  f.fi = (int32_t*)c.alloc((size_t)N * sizeof(int32_t));
  f.maps = (double*)c.alloc((size_t)N * 6 * sizeof(double));
  return f;
}

PlanSize lmk_bytes(ghost_lmk* h, int N) {
  return size_plan<LmkCtx>(h, [&](LmkCtx& c) {
    const Front f = front(c, N);
    lmk_plan(c, f.x192, (int64_t)kIn * kIn * 3, 1, N, (float*)uintptr_t(0x30000000), nullptr);
  });
}

int run_lmk(ghost_lmk* h, const uint8_t* x192, int64_t xstride, int bgr, const uint8_t* crops, int64_t crop_bs, int N,
            float* pred, float* lmk, void* ws, int64_t ws_bytes, void* stream) {
  if (const int rc = check_batch(h, N, 0, 65535)) return rc;
  if (N == 0) return GHOST_OK;
  if (count_missing(h->slots)) return GHOST_ENOTREADY;
  return run_plan<LmkCtx>(h, lmk_bytes(h, N), ws, ws_bytes, stream, "landmark forward", [&](LmkCtx& c) {
    const Front f = front(c, N);
    if (crops) {
      // cv2.warpAffine(crop, M, (192, 192), borderValue=0.0): the maps are cv2.invertAffineTransform(M) in double
      const double Dv = 1.0 / (kM[0] * kM[4] - kM[1] * kM[3]);
      const double a11 = kM[4] * Dv, a22 = kM[0] * Dv, a12 = -kM[1] * Dv, a21 = -kM[3] * Dv;
      const double inv[6] = {a11, a12, -a11 * kM[2] - a12 * kM[5], a21, a22, -a21 * kM[2] - a22 * kM[5]};
      c.check(lmk_fill_maps(f.fi, f.maps, N, inv, c.s), "fill maps");
      if (c.ok() && ghost_align_crops_u8(crops, crop_bs, N, kCrop, kCrop, f.fi, f.maps, nullptr, N, kIn, f.x192,
                                         (int64_t)kIn * kIn * 3, nullptr, 0, 0, stream) != 0)
        return (int)GHOST_EINVAL;   // the last error is ghost_align_crops_u8's
      x192 = f.x192;
      xstride = (int64_t)kIn * kIn * 3;
      bgr = 1;
    }
    lmk_plan(c, x192, xstride, bgr, N, pred, lmk);
    return 0;
  });
}

}  // namespace

extern "C" int ghost_lmk_create(int dtype, ghost_lmk** out) {
  if (!out) return lmk_fail(GHOST_EINVAL, "null argument");
  if (!storage_esz(dtype)) return lmk_fail(GHOST_EINVAL, "dtype must be f32, bf16 or f16");
  ghost_lmk* h = new ghost_lmk();
  h->set_storage(dtype);
  declare(h);
  *out = h;
  return 0;
}

extern "C" void ghost_lmk_destroy(ghost_lmk* h) { delete h; }

extern "C" int ghost_lmk_bind(ghost_lmk* h, const char* name, const void* p, int64_t numel) {
  return handle_bind(h, name, p, numel);
}

extern "C" int ghost_lmk_missing(ghost_lmk* h) { return handle_missing(h); }

extern "C" int64_t ghost_lmk_workspace_bytes(ghost_lmk* h, int N) {
  if (!h || N < 0 || N > 65535) return lmk_fail(GHOST_EINVAL, "bad argument");
  if (N == 0) return 256;
  return lmk_bytes(h, N).need();
}

extern "C" int ghost_lmk_forward(ghost_lmk* h, const uint8_t* x192, int64_t x_batch_stride, int bgr, int N,
                                 float* pred, void* ws, int64_t ws_bytes, void* stream) {
  if (N != 0 && (!x192 || !pred)) return lmk_fail(GHOST_EINVAL, "null argument");
  if (N != 0 && x_batch_stride < (int64_t)kIn * kIn * 3) return lmk_fail(GHOST_EINVAL, "batch stride below 192*192*3");
  return run_lmk(h, x192, x_batch_stride, bgr, nullptr, 0, N, pred, nullptr, ws, ws_bytes, stream);
}

extern "C" int ghost_lmk_landmarks_u8(ghost_lmk* h, const uint8_t* crops224_bgr, int64_t crop_batch_stride, int N,
                                      float* landmarks, float* pred, void* ws, int64_t ws_bytes, void* stream) {
  if (N != 0 && (!crops224_bgr || !landmarks)) return lmk_fail(GHOST_EINVAL, "null argument");
  if (N != 0 && crop_batch_stride < (int64_t)kCrop * kCrop * 3)
    return lmk_fail(GHOST_EINVAL, "batch stride below 224*224*3");
  return run_lmk(h, nullptr, 0, 1, crops224_bgr, crop_batch_stride, N, pred, landmarks, ws, ws_bytes, stream);
}

extern "C" int ghost_lmk_set_taps(ghost_lmk* h, void* const* taps, int ntaps) {
  return handle_set_taps(h, taps, ntaps);
}
