// ghost_amd — the SCRFD face detector (insightface scrfd_10g_bnkps) on gfx950, C ABI in include/ghost_amd.h.
//
// GHOST calls it once per video frame as Face_detect_crop.get -> SCRFD.detect on one 640 x 640 letterboxed image
// (insightface_func/face_detect_crop_multi.py:54-93).  The graph (ResNet-style backbone with a deep stem and
// avg-down shortcuts, PAFPN, three shared-tower heads; BatchNorm folded) is recalled from the public sources, not
// verified against the ONNX file: DESIGN.md §12 lists what to check first.  ghost_amd/detection/pack.py holds the same
// graph as one table; the names here are that table's.
//
// Plan (NHWC, one stream):
//   canvas  det_letterbox: cv2.resize into the top-left of a zero uint8 canvas [N,Hd,Wd,3]
//   stem    det_stem (uint8 -> fp32 normalise -> conv 3 -> 28 + bias + ReLU), two 3x3 convs, det_maxpool
//   stages  BasicBlocks: conv3x3 + ReLU, conv3x3 + identity + ReLU (res_first); a stride-2 block's identity is one
//           conv 2x2/s2 whose taps are w/4 (AvgPool 2x2 then conv1x1, exactly)
//   neck    laterals 1x1, det_upadd top-down, 3x3 convs, 3x3/s2 bottom-up with the add as the conv's residual
//   heads   three 3x3 + ReLU, then det_head: cls / reg / kps as one fp32 conv 80 -> 30 with the sigmoid, fp32 outputs
//   detect  det_decode_nms over the nine maps
// Every convolution but the first and the last goes through conv_launch (conv_igemm.h): bias as shift, slope 0 for
// ReLU.  The last is a kernel of its own because the maps are fp32 whatever the storage type, and the implicit GEMM
// has a 16-bit -> fp32 instance for bf16 only.
#include <cstdarg>
#include <cstdio>
#include <map>
#include <string>
#include <utility>

#include "ghost_amd.h"
#include "ghost_common.h"
#include "conv_igemm.h"
#include "conv_path.h"
#include "det.h"
#include "plan_ctx.h"

using namespace ghost;

static int det_fail(int rc, const std::string& msg) { return ghost::set_last_error(rc, msg); }

// diagnostic taps (ghost_det_set_taps): the stored outputs of the stem (after the pool), stage 1, stage 4 and P3
struct ghost_det : Handle {
  static constexpr int kTaps = 4;
  static constexpr bool kAligned16 = true;
  int Hd = 640, Wd = 640;
  // (N, detect) -> the dry run's result, kept so that a call does not repeat it
  std::map<std::pair<int, bool>, PlanSize> sized;
};

namespace {

const int kPlanes[4] = {56, 88, 88, 224};
const int kNBlocks[4] = {3, 4, 2, 3};
constexpr int kNeck = 56, kTower = 80;
constexpr int kMaxBatch = 4096;

struct DetCtx : HandleCtx<ghost_det> {
  std::string* list = nullptr;   // ghost_det_plan: one line per launch of the dry run
  void line(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
    if (!list) return;
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    *list += buf;
    *list += "\n";
  }
};

struct Outs { float* cls[3]; float* reg[3]; float* kps[3]; };

// one conv unit of the table: y = act(conv(x) + bias + res)
void conv(DetCtx& c, const std::string& name, const void* x, int N, int H, int W, int cin, int cout, int k, int stride,
          int pad, bool relu, const void* res, void* y, int to) {
  const int dt = c.h->dt;
  ConvDesc g = conv_desc(dt, to, x, N, H, W, cin, cin, c.W(name + ".w"), cout, rup(cout, 128), rup(k * k * cin, 32),
                         CONV_FWD, k, k, stride, pad, y, cout);
  g.shift = c.F(name + ".b");
  g.slope = relu ? 0.f : 1.f;
  if (res) { g.res = res; g.ldres = cout; g.res_first = 1; }
  c.line("conv %s k=%d s=%d in=%dx%d cin=%d cout=%d relu=%d res=%d out=%s", name.c_str(), k, stride, H, W, cin, cout,
         relu ? 1 : 0, res ? 1 : 0, plan_dt(to));
  if (!c.ok()) return;
  if (c.dry) {
    if (!conv_desc_ok(g) || (conv_path(g) == ConvPath::Igemm && igemm_plan(g).kernel == IgemmKernel::None))
      c.check(GHOST_EINVAL, "no conv kernel takes " + name);
    else
      c.need_scratch(conv_workspace_bytes(g));
  } else {
    c.check(conv_launch(g, c.scratch, c.scratch_cap, c.s), name);
  }
}

// canvas: uint8 [N,Hd,Wd,3] B,G,R, bstride bytes apart
void det_plan(DetCtx& c, const uint8_t* canvas, int64_t bstride, int N, const Outs& o) {
  ghost_det* h = c.h;
  const int es = h->esz, dt = h->dt, Hd = h->Hd, Wd = h->Wd;
  const int H2 = Hd / 2, W2 = Wd / 2, H4 = Hd / 4, W4 = Wd / 4;
  const size_t px2 = (size_t)N * H2 * W2, px4 = (size_t)N * H4 * W4, px8 = px4 / 4;
  void* S0 = c.alloc(px2 * kDetStemC * es);
  void* S1 = c.alloc(px2 * kDetStemC * es);
  void* S2 = c.alloc(px2 * 56 * es);
  void* P[2] = {c.alloc(px4 * 56 * es), c.alloc(px4 * 56 * es)};
  void* T = c.alloc(px4 * 56 * es);        // a block's first conv
  void* I = c.alloc(px8 * 88 * es);        // a stride-2 block's identity (at most H/8 x W/8 x 88)
  void* C[4] = {nullptr, c.alloc(px8 * 88 * es), c.alloc(px8 / 4 * 88 * es), c.alloc(px8 / 16 * 224 * es)};
  {
    const float *w = c.F("backbone.stem.0.w"), *b = c.F("backbone.stem.0.b");
    c.line("stem backbone.stem.0 in=%dx%d cin=3 cout=%d", Hd, Wd, kDetStemC);
    if (c.ok() && !c.dry) c.check(det_stem(dt, canvas, bstride, 1, N, Hd, Wd, w, b, S0, c.s), "stem");
  }
  conv(c, "backbone.stem.3", S0, N, H2, W2, kDetStemC, kDetStemC, 3, 1, 1, true, nullptr, S1, dt);
  conv(c, "backbone.stem.6", S1, N, H2, W2, kDetStemC, 56, 3, 1, 1, true, nullptr, S2, dt);
  c.line("maxpool in=%dx%d c=56", H2, W2);
  if (c.ok() && !c.dry) c.check(det_maxpool(dt, S2, N, H2, W2, 56, P[0], c.s), "maxpool");
  c.tap(0, P[0], px4 * 56 * es);
  void* cur = P[0];
  int cin = 56, H = H4, W = W4;
  for (int st = 0; st < 4; ++st) {
    const int pl = kPlanes[st];
    for (int b = 0; b < kNBlocks[st]; ++b) {
      const int stride = st > 0 && b == 0 ? 2 : 1;
      const int Ho = H / stride, Wo = W / stride;
      const std::string nm = "backbone.layer" + std::to_string(st + 1) + "." + std::to_string(b);
      void* out = b == kNBlocks[st] - 1 && st > 0 ? C[st] : (cur == P[0] ? P[1] : P[0]);
      conv(c, nm + ".conv1", cur, N, H, W, cin, pl, 3, stride, 1, true, nullptr, T, dt);
      const void* idn = cur;
      if (stride == 2) {
        conv(c, nm + ".downsample.1", cur, N, H, W, cin, pl, 2, 2, 0, false, nullptr, I, dt);
        idn = I;
      }
      conv(c, nm + ".conv2", T, N, Ho, Wo, pl, pl, 3, 1, 1, true, idn, out, dt);
      cur = out; cin = pl; H = Ho; W = Wo;
    }
    if (st == 0) c.tap(1, cur, px4 * 56 * es);
    if (st == 3) c.tap(2, cur, px8 / 16 * 224 * es);
  }
  // ---- PAFPN ----
  const int Hl[3] = {Hd / 8, Hd / 16, Hd / 32}, Wl[3] = {Wd / 8, Wd / 16, Wd / 32};
  const size_t pxl[3] = {px8, px8 / 4, px8 / 16};
  void *L[3], *In[3], *J[3], *Pm[3];
  for (int i = 0; i < 3; ++i) {
    L[i] = c.alloc(pxl[i] * kNeck * es);
    conv(c, "neck.lateral_convs." + std::to_string(i) + ".conv", C[i + 1], N, Hl[i], Wl[i], kPlanes[i + 1], kNeck, 1, 1,
         0, false, nullptr, L[i], dt);
  }
  for (int i = 2; i > 0; --i) {
    c.line("upadd in=%dx%d c=%d", Hl[i], Wl[i], kNeck);
    if (c.ok() && !c.dry) c.check(det_upadd(dt, L[i], N, Hl[i], Wl[i], kNeck, L[i - 1], c.s), "upadd");
  }
  for (int i = 0; i < 3; ++i) {
    In[i] = c.alloc(pxl[i] * kNeck * es);
    conv(c, "neck.fpn_convs." + std::to_string(i) + ".conv", L[i], N, Hl[i], Wl[i], kNeck, kNeck, 3, 1, 1, false,
         nullptr, In[i], dt);
  }
  J[0] = In[0];
  for (int i = 0; i < 2; ++i) {
    J[i + 1] = c.alloc(pxl[i + 1] * kNeck * es);
    conv(c, "neck.downsample_convs." + std::to_string(i) + ".conv", J[i], N, Hl[i], Wl[i], kNeck, kNeck, 3, 2, 1, false,
         In[i + 1], J[i + 1], dt);
  }
  Pm[0] = In[0];
  for (int i = 0; i < 2; ++i) {
    Pm[i + 1] = c.alloc(pxl[i + 1] * kNeck * es);
    conv(c, "neck.pafpn_convs." + std::to_string(i) + ".conv", J[i + 1], N, Hl[i + 1], Wl[i + 1], kNeck, kNeck, 3, 1, 1,
         false, nullptr, Pm[i + 1], dt);
  }
  c.tap(3, Pm[0], px8 * kNeck * es);
  // ---- heads ----
  void* U[2] = {c.alloc(px8 * kTower * es), c.alloc(px8 * kTower * es)};
  for (int l = 0; l < 3; ++l) {
    const std::string s = std::to_string(8 << l);
    const void* x = Pm[l];
    int ci = kNeck;
    for (int j = 0; j < 3; ++j) {
      conv(c, "bbox_head.cls_stride_convs." + s + "." + std::to_string(j) + ".conv", x, N, Hl[l], Wl[l], ci, kTower, 3,
           1, 1, true, nullptr, U[j & 1], dt);
      x = U[j & 1];
      ci = kTower;
    }
    const std::string hn = "bbox_head.out." + s;
    const float *hw = c.F(hn + ".w"), *hb = c.F(hn + ".b"), *hm = c.F(hn + ".m");
    c.line("head %s k=3 in=%dx%d cin=%d cout=%d out=f32", hn.c_str(), Hl[l], Wl[l], kTower, kDetHeadOut);
    if (c.ok() && !c.dry)
      c.check(det_head(dt, x, N, Hl[l], Wl[l], hw, hb, hm, o.cls[l], o.reg[l], o.kps[l], c.s), hn);
  }
}

void declare(ghost_det* h) {
  auto unit = [&](const std::string& s) { h->slots[s + ".w"] = nullptr; h->slots[s + ".b"] = nullptr; };
  unit("backbone.stem.0"); unit("backbone.stem.3"); unit("backbone.stem.6");
  for (int st = 0; st < 4; ++st)
    for (int b = 0; b < kNBlocks[st]; ++b) {
      const std::string nm = "backbone.layer" + std::to_string(st + 1) + "." + std::to_string(b);
      unit(nm + ".conv1"); unit(nm + ".conv2");
      if (st > 0 && b == 0) unit(nm + ".downsample.1");
    }
  for (int i = 0; i < 3; ++i) {
    unit("neck.lateral_convs." + std::to_string(i) + ".conv");
    unit("neck.fpn_convs." + std::to_string(i) + ".conv");
    if (i < 2) {
      unit("neck.downsample_convs." + std::to_string(i) + ".conv");
      unit("neck.pafpn_convs." + std::to_string(i) + ".conv");
    }
    const std::string s = std::to_string(8 << i);
    for (int j = 0; j < 3; ++j) unit("bbox_head.cls_stride_convs." + s + "." + std::to_string(j) + ".conv");
    unit("bbox_head.out." + s);
    h->slots["bbox_head.out." + s + ".m"] = nullptr;
  }
}

// the regions in front of the plan's: the canvas and, for detect, the nine maps and the decode workspace
struct Front { uint8_t* canvas; Outs maps; void* dws; size_t dws_bytes; };
Front front(DetCtx& c, int N, bool detect) {
  ghost_det* h = c.h;
  Front f{};
  f.canvas = (uint8_t*)c.alloc((size_t)N * h->Hd * h->Wd * 3);
  if (detect) {
    for (int l = 0; l < 3; ++l) {
      const size_t px = (size_t)N * (h->Hd >> (3 + l)) * (h->Wd >> (3 + l));
      f.maps.cls[l] = (float*)c.alloc(px * 2 * 4);
      f.maps.reg[l] = (float*)c.alloc(px * 8 * 4);
      f.maps.kps[l] = (float*)c.alloc(px * 20 * 4);
    }
    f.dws_bytes = det_decode_workspace_bytes(N, kDetMaxCap);
    f.dws = c.alloc(f.dws_bytes);
  }
  return f;
}

// detect: with the nine maps and the decode workspace in the workspace (forward's maps are the caller's)
// A failure (rc set) has set the last error.
PlanSize det_bytes(ghost_det* h, int N, bool detect, std::string* list = nullptr) {
  PlanSize z;
  if ((int64_t)N * (h->Hd / 2) * (h->Wd / 2) > 0x7fffffffLL) {
    z.rc = det_fail(GHOST_EINVAL, "batch x det_size too large for one call (N * Hd/2 * Wd/2 must fit 31 bits)");
    return z;
  }
  const auto key = std::make_pair(N, detect);
  const auto it = h->sized.find(key);
  if (it != h->sized.end() && !list) return it->second;
  z = size_plan<DetCtx>(h, [&](DetCtx& c) {
    c.list = list;
    c.line("letterbox out=%dx%d", h->Hd, h->Wd);
    const Front f = front(c, N, detect);
    det_plan(c, f.canvas, (int64_t)h->Hd * h->Wd * 3, N, f.maps);
    if (detect) {
      c.line("decode cap=%d", kDetMaxCap);
      c.line("nms cap=%d", kDetMaxCap);
    }
  });
  if (z.rc) {
    det_fail(z.rc, "detector plan: " + z.where);
    return z;
  }
  if (h->sized.size() >= 64) h->sized.clear();
  h->sized[key] = z;
  return z;
}

struct DetectArgs {
  float det_scale, thresh, nms_thresh;
  int max_faces;
  float* det; float* kps; int32_t* anchor; int32_t* count;
};

int run_det(ghost_det* h, const uint8_t* frames, int64_t fstride, int N, int H, int W, int new_h, int new_w,
            float* const* maps, const DetectArgs* da, void* ws, int64_t ws_bytes, void* stream) {
  if (const int rc = check_batch(h, N, 0, kMaxBatch)) return rc;
  if (N == 0) return GHOST_OK;
  if (!frames || H <= 0 || W <= 0 || fstride < (int64_t)H * W * 3) return det_fail(GHOST_EINVAL, "bad frames");
  if (new_h <= 0 || new_w <= 0 || new_h > h->Hd || new_w > h->Wd)
    return det_fail(GHOST_EINVAL, "the resized frame must fit det_size");
  if (count_missing(h->slots)) return GHOST_ENOTREADY;
  const PlanSize z = det_bytes(h, N, da != nullptr);
  if (z.rc) return z.rc;
  return run_plan<DetCtx>(h, z, ws, ws_bytes, stream, "detector", [&](DetCtx& c) {
    Front f = front(c, N, da != nullptr);
    if (maps)
      for (int l = 0; l < 3; ++l) { f.maps.cls[l] = maps[l]; f.maps.reg[l] = maps[3 + l]; f.maps.kps[l] = maps[6 + l]; }
    c.check(det_letterbox(frames, fstride, N, H, W, new_h, new_w, f.canvas, h->Hd, h->Wd, c.s), "letterbox");
    det_plan(c, f.canvas, (int64_t)h->Hd * h->Wd * 3, N, f.maps);
    if (c.ok() && da) {
      DetMaps m;
      for (int l = 0; l < 3; ++l) { m.cls[l] = f.maps.cls[l]; m.reg[l] = f.maps.reg[l]; m.kps[l] = f.maps.kps[l]; }
      c.check(det_decode_nms(m, N, h->Hd, h->Wd, da->thresh, da->det_scale, da->nms_thresh, kDetMaxCap, da->max_faces,
                             da->det, da->kps, da->anchor, da->count, f.dws, f.dws_bytes, c.s), "decode + nms");
    }
    return 0;
  });
}

}  // namespace

extern "C" int ghost_det_create(int dtype, int det_w, int det_h, ghost_det** out) {
  if (!out) return det_fail(GHOST_EINVAL, "null argument");
  if (!storage_esz(dtype)) return det_fail(GHOST_EINVAL, "dtype must be f32, bf16 or f16");
  if (det_w <= 0 || det_h <= 0 || det_w % 32 || det_h % 32 || det_w > 8192 || det_h > 8192)
    return det_fail(GHOST_EINVAL, "det_size must be positive multiples of 32, at most 8192");
  ghost_det* h = new ghost_det();
  h->set_storage(dtype);
  h->Wd = det_w;
  h->Hd = det_h;
  declare(h);
  *out = h;
  return 0;
}

extern "C" void ghost_det_destroy(ghost_det* h) { delete h; }

extern "C" int ghost_det_bind(ghost_det* h, const char* name, const void* p, int64_t numel) {
  return handle_bind(h, name, p, numel);
}

extern "C" int ghost_det_missing(ghost_det* h) { return handle_missing(h); }

extern "C" int64_t ghost_det_workspace_bytes(ghost_det* h, int N) {
  if (!h || N < 0 || N > kMaxBatch) return det_fail(GHOST_EINVAL, "bad argument");
  if (N == 0) return 256;
  return det_bytes(h, N, true).need();
}

extern "C" int64_t ghost_det_plan(ghost_det* h, int N, char* buf, int64_t cap) {
  if (!h || N <= 0 || N > kMaxBatch || cap < 0 || (cap > 0 && !buf)) return det_fail(GHOST_EINVAL, "bad argument");
  std::string text;
  const PlanSize z = det_bytes(h, N, true, &text);
  if (z.rc) return z.rc;
  if (cap > 0) snprintf(buf, (size_t)cap, "%s", text.c_str());
  return (int64_t)text.size() + 1;
}

extern "C" int ghost_det_forward_u8(ghost_det* h, const uint8_t* frames_bgr, int64_t frame_stride, int F, int H, int W,
                                    int new_h, int new_w, float* const* maps, void* ws, int64_t ws_bytes, void* stream) {
  if (F != 0) {
    if (!maps) return det_fail(GHOST_EINVAL, "null argument");
    for (int i = 0; i < 9; ++i)
      if (!maps[i] || ((uintptr_t)maps[i] & 15)) return det_fail(GHOST_EINVAL, "maps must be nine 16-byte aligned pointers");
  }
  return run_det(h, frames_bgr, frame_stride, F, H, W, new_h, new_w, maps, nullptr, ws, ws_bytes, stream);
}

extern "C" int ghost_det_detect_u8(ghost_det* h, const uint8_t* frames_bgr, int64_t frame_stride, int F, int H, int W,
                                   int new_h, int new_w, float det_scale, float thresh, float nms_thresh, int max_faces,
                                   float* det, float* kps, int32_t* anchor, int32_t* count, void* ws, int64_t ws_bytes,
                                   void* stream) {
  if (F != 0 && (!det || !kps || !anchor || !count || max_faces <= 0 || !(det_scale > 0.f)))
    return det_fail(GHOST_EINVAL, "null output, max_faces <= 0 or det_scale <= 0");
  const DetectArgs da{det_scale, thresh, nms_thresh, max_faces, det, kps, anchor, count};
  return run_det(h, frames_bgr, frame_stride, F, H, W, new_h, new_w, nullptr, &da, ws, ws_bytes, stream);
}

extern "C" int ghost_det_set_taps(ghost_det* h, void* const* taps, int ntaps) {
  return handle_set_taps(h, taps, ntaps);
}
