// ghost_amd — C ABI of the single operators (include/ghost_amd.h): one kernel family per entry point, no handle.
// The descriptors come from the builders the network's schedule uses (conv_igemm.h, aad_v3.h, aad_wide.h).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/ghost_amd.h"
#include "aad_fused.h"
#include "aad_path.h"
#include "aad_v3.h"
#include "aad_wide.h"
#include "conv_halo.h"
#include "conv_igemm.h"
#include "conv_narrow.h"
#include "conv_path.h"
#include "ghost_common.h"
#include "ops.h"
#include "plan_ctx.h"

using namespace ghost;

static int fail(int rc, const std::string& msg) { return set_last_error(rc, msg); }

static int conv_op(ConvDesc& d, void* ws, int64_t ws_bytes, void* stream, const char* what) {
  const size_t need = conv_workspace_bytes(d);
  if (need > 0 && (!ws || (size_t)ws_bytes < need))
    return fail(GHOST_ENOWS, std::string(what) + ": workspace too small, need " + std::to_string(need));
  int rc = conv_launch(d, ws, (size_t)ws_bytes, (hipStream_t)stream);
  if (rc) return fail(rc, std::string(what) + " failed");
  return 0;
}

extern "C" int ghost_conv2d_nhwc(int dtype, const void* x, int B, int H, int W, int Cin, int ldx, const void* w_packed,
                                 int Cout, int Npad, int Kpad, int kh, int kw, int stride, int pad, const float* scale,
                                 const float* shift, float slope, const void* res, int ldres, int tanh_out, void* y,
                                 int ldy, void* ws, int64_t ws_bytes, void* stream) {
  ConvDesc d = conv_desc(dtype, dtype, x, B, H, W, Cin, ldx, w_packed, Cout, Npad, Kpad, CONV_FWD, kh, kw, stride, pad,
                         y, ldy);
  d.scale = scale; d.shift = shift; d.slope = slope; d.res = res; d.ldres = ldres; d.tanh_out = tanh_out;
  return conv_op(d, ws, ws_bytes, stream, "ghost_conv2d_nhwc");
}

static void set_epi(ConvDesc& d, const ghost_conv_epi* epi) {
  d.scale = epi->scale; d.shift = epi->shift; d.slope = epi->slope; d.prelu = epi->prelu;
  d.res = epi->res; d.ldres = epi->ldres; d.res_first = epi->res_first; d.tanh_out = epi->tanh_out;
  d.y2 = epi->y2; d.ldy2 = epi->ldy2; d.scale2 = epi->scale2; d.shift2 = epi->shift2;
  d.force_split = epi->split_k;
}

extern "C" int ghost_conv2d_ex_nhwc(int dtype, const void* x, int B, int H, int W, int Cin, int ldx,
                                    const void* w_packed, int Cout, int Npad, int Kpad, int kh, int kw, int stride,
                                    int pad, const ghost_conv_epi* epi, void* y, int ldy, void* ws, int64_t ws_bytes,
                                    void* stream) {
  if (!epi) return fail(GHOST_EINVAL, "ghost_conv2d_ex_nhwc: null epilogue");
  ConvDesc d = conv_desc(dtype, dtype, x, B, H, W, Cin, ldx, w_packed, Cout, Npad, Kpad, CONV_FWD, kh, kw, stride, pad,
                         y, ldy);
  if (epi->split_k < 0) return fail(GHOST_EINVAL, "ghost_conv2d_ex_nhwc: split_k must be >= 0");
  set_epi(d, epi);
  return conv_op(d, ws, ws_bytes, stream, "ghost_conv2d_ex_nhwc");
}

// what aei_runtime.hip conv3x3() does with its stat argument: the conv writes per-(tile, wave) partials of its
// output into the workspace, in_stats_from_tiles merges them
extern "C" int ghost_conv2d_stats_nhwc(int dtype, const void* x, int B, int H, int W, int Cin, int ldx,
                                       const void* w_packed, int Cout, int Npad, int Kpad, int kh, int kw, int stride,
                                       int pad, const ghost_conv_epi* epi, void* y, int ldy, float* stat, void* ws,
                                       int64_t ws_bytes, void* stream) {
  if (!epi || !stat) return fail(GHOST_EINVAL, "ghost_conv2d_stats_nhwc: null epilogue or stat");
  if (epi->split_k < 0) return fail(GHOST_EINVAL, "ghost_conv2d_stats_nhwc: split_k must be >= 0");
  ConvDesc d = conv_desc(dtype, dtype, x, B, H, W, Cin, ldx, w_packed, Cout, Npad, Kpad, CONV_FWD, kh, kw, stride, pad,
                         y, ldy);
  set_epi(d, epi);
  int nrec = 0;
  if (!conv_desc_ok(d) || conv_path(d) != ConvPath::Halo3x3 || !conv3x3_pp_takes(d, &nrec))
    return fail(GHOST_EINVAL, "ghost_conv2d_stats_nhwc: the kernel of this conv writes no InstanceNorm partials");
  const size_t need = (size_t)B * nrec * Cout * 2 * sizeof(float) + 256;
  if (!ws || ws_bytes < 0 || (size_t)ws_bytes < need)
    return fail(GHOST_ENOWS, "ghost_conv2d_stats_nhwc: workspace too small, need " + std::to_string(need));
  d.in_part = (float*)align_up(ws);
  int rc = conv_launch(d, nullptr, 0, (hipStream_t)stream);
  if (rc) return fail(rc, "ghost_conv2d_stats_nhwc failed");
  rc = in_stats_from_tiles(d.in_part, B, nrec, Cout, stat, (hipStream_t)stream);
  return rc ? fail(rc, "ghost_conv2d_stats_nhwc: in_stats_from_tiles failed") : 0;
}

extern "C" int ghost_conv_transpose4x4s2_nhwc(int dtype, const void* x, int B, int H, int W, int Cin, int ldx,
                                              const void* w_packed, int Cout, int Npad, int Kpad, const float* scale,
                                              const float* shift, float slope, const void* res, int ldres, void* y,
                                              int ldy, void* ws, int64_t ws_bytes, void* stream) {
  ConvDesc d = conv_desc(dtype, dtype, x, B, H, W, Cin, ldx, w_packed, Cout, Npad, Kpad, CONV_T4S2, 1, 1, 1, 0, y, ldy);
  d.scale = scale; d.shift = shift; d.slope = slope; d.res = res; d.ldres = ldres;
  return conv_op(d, ws, ws_bytes, stream, "ghost_conv_transpose4x4s2_nhwc");
}

extern "C" int ghost_linear_f32(const float* x, int B, int K, const float* w_packed, int N, int Npad, int Kpad,
                                const float* bias, int out_dtype, void* y, int ldy, void* ws, int64_t ws_bytes,
                                void* stream) {
  ConvDesc d = conv_desc(GHOST_F32, out_dtype, x, B, 1, 1, K, K, w_packed, N, Npad, Kpad, CONV_FWD, 1, 1, 1, 0, y, ldy);
  d.shift = bias;
  return conv_op(d, ws, ws_bytes, stream, "ghost_linear_f32");
}

extern "C" int ghost_instnorm_stats_nhwc(int dtype, const void* x, int B, int HW, int C, int ldx, float* stat, void* ws,
                                         int64_t ws_bytes, void* stream) {
  if ((size_t)ws_bytes < in_stats_workspace_bytes(B, HW, C)) return fail(GHOST_ENOWS, "in_stats: workspace too small");
  int rc = in_stats(dtype, x, ldx, B, HW, C, stat, ws, (size_t)ws_bytes, (hipStream_t)stream);
  return rc ? fail(rc, "in_stats failed") : 0;
}

extern "C" int ghost_instnorm_stats_up2x_nhwc(int dtype, const void* x, int B, int H, int W, int C, int ldx,
                                              float* stat, void* ws, int64_t ws_bytes, void* stream) {
  if ((size_t)ws_bytes < in_stats_workspace_bytes(B, 4 * H * W, C))
    return fail(GHOST_ENOWS, "in_stats_up2x: workspace too small");
  int rc = in_stats_up2x(dtype, x, ldx, B, H, W, C, stat, ws, (size_t)ws_bytes, (hipStream_t)stream);
  return rc ? fail(rc, "in_stats_up2x failed") : 0;
}

static bool sem_ok(const unsigned* sem, int nsem);

// Test support: the statistics as the runtimes call them (aei_runtime.hip run_stats / run_stats_up), with the arrival
// counters of the fused final pass.  up2x = 1: x is the [B, H, W, C] source of the virtual upsample
extern "C" int ghost_instnorm_stats_rt_nhwc(int dtype, const void* x, int B, int H, int W, int C, int ldx, int up2x,
                                            float* stat, void* ws, int64_t ws_bytes, unsigned* sem, int nsem,
                                            void* stream) {
  if (!x || !stat || (up2x & ~1) || ws_bytes < 0) return fail(GHOST_EINVAL, "ghost_instnorm_stats_rt_nhwc: bad argument");
  if (!sem_ok(sem, nsem)) return fail(GHOST_EINVAL, "ghost_instnorm_stats_rt_nhwc: sem / nsem must be (NULL, 0) or nsem > 0 words");
  const InStatsPlan p = in_stats_plan(dtype, B, H, W, C, ldx, up2x != 0, nsem);
  if (p.kernel == InStatsKernel::None || (uintptr_t)x % 16)
    return fail(GHOST_EINVAL, "ghost_instnorm_stats_rt_nhwc: unsupported shape (C % 16, ldx % 8, a 16-byte aligned x)");
  if (!ws || (size_t)ws_bytes < in_stats_workspace_bytes(B, p.HW, C))
    return fail(GHOST_ENOWS, "ghost_instnorm_stats_rt_nhwc: workspace too small");
  int rc = up2x ? in_stats_up2x(dtype, x, ldx, B, H, W, C, stat, ws, (size_t)ws_bytes, (hipStream_t)stream, sem, nsem)
                : in_stats(dtype, x, ldx, B, H * W, C, stat, ws, (size_t)ws_bytes, (hipStream_t)stream, sem, nsem);
  return rc ? fail(rc, "ghost_instnorm_stats_rt_nhwc failed") : 0;
}

extern "C" int64_t ghost_instnorm_plan(int dtype, int B, int H, int W, int C, int ldx, int up2x, int nsem,
                                       int64_t* ws_bytes, char* buf, int64_t cap) {
  if ((up2x & ~1) || nsem < 0 || cap < 0 || (cap > 0 && !buf)) return fail(GHOST_EINVAL, "instnorm_plan: bad argument");
  const InStatsPlan p = in_stats_plan(dtype, B, H, W, C, ldx, up2x != 0, nsem);
  if (p.kernel == InStatsKernel::None) return fail(GHOST_EINVAL, "instnorm_plan: in_stats rejects this shape");
  char text[160];
  const int n = in_stats_plan_text(dtype, p, text, sizeof(text));
  if (ws_bytes) *ws_bytes = (int64_t)in_stats_workspace_bytes(B, p.HW, C);
  if (cap > 0) snprintf(buf, (size_t)cap, "%s", text);
  return (int64_t)n + 1;
}

// the arrival counters of a test-support entry: none (NULL, 0) or nsem > 0 words at sem
static bool sem_ok(const unsigned* sem, int nsem) { return nsem >= 0 && (nsem > 0) == (sem != nullptr) && (uintptr_t)sem % 4 == 0; }

// Test support: one convolution as the runtimes launch it (aei_runtime.hip run_conv, arc_runtime.hip's head): the
// output type apart from the operand type, and the arrival counters of the split-K fix-up
extern "C" int ghost_conv_rt_nhwc(int in_dtype, int out_dtype, int kind, const void* x, int B, int H, int W, int Cin,
                                  int ldx, const void* w_packed, int Cout, int Npad, int Kpad, int kh, int kw,
                                  int stride, int pad, const ghost_conv_epi* epi, void* y, int ldy, void* ws,
                                  int64_t ws_bytes, unsigned* sem, int nsem, void* stream) {
  if (!epi) return fail(GHOST_EINVAL, "ghost_conv_rt_nhwc: null epilogue");
  if (kind != CONV_FWD && kind != CONV_T4S2) return fail(GHOST_EINVAL, "ghost_conv_rt_nhwc: kind must be 0 (FWD) or 1 (T4S2)");
  if (epi->split_k < 0 || ws_bytes < 0) return fail(GHOST_EINVAL, "ghost_conv_rt_nhwc: split_k and ws_bytes must be >= 0");
  if (!sem_ok(sem, nsem)) return fail(GHOST_EINVAL, "ghost_conv_rt_nhwc: sem / nsem must be (NULL, 0) or nsem > 0 words");
  ConvDesc d = kind == CONV_T4S2
                   ? conv_desc(in_dtype, out_dtype, x, B, H, W, Cin, ldx, w_packed, Cout, Npad, Kpad, CONV_T4S2, 1, 1, 1, 0, y, ldy)
                   : conv_desc(in_dtype, out_dtype, x, B, H, W, Cin, ldx, w_packed, Cout, Npad, Kpad, CONV_FWD, kh, kw, stride,
                               pad, y, ldy);
  set_epi(d, epi);
  d.sem = sem; d.nsem = nsem;
  if (!conv_desc_ok(d)) return fail(GHOST_EINVAL, "ghost_conv_rt_nhwc: conv_launch rejects this descriptor");
  // only the implicit GEMM has instances whose output type differs from the operand type, and not for every pair
  if (conv_path(d) != ConvPath::Igemm ? in_dtype != out_dtype : igemm_plan(d).kernel == IgemmKernel::None)
    return fail(GHOST_EINVAL, "ghost_conv_rt_nhwc: no kernel instance takes this descriptor (type pair, packing)");
  return conv_op(d, ws, ws_bytes, stream, "ghost_conv_rt_nhwc");
}

static int aad_layer(int dtype, const void* h_in, int ldh, const void* z_attr, int lda, int B, int H, int W, int C, int Ca,
                     const void* gbw_packed, int Npad, int Kpad, const float* gbb, const float* wh, const float* bh,
                     const float* idgb, int id_ld, float slope, void* out, int ldo, void* ws, int64_t ws_bytes,
                     int split_k, unsigned* sem, int nsem, void* stream);

extern "C" int ghost_aad_layer_nhwc(int dtype, const void* h_in, int ldh, const void* z_attr, int lda, int B, int H,
                                    int W, int C, int Ca, const void* gbw_packed, int Npad, int Kpad, const float* gbb,
                                    const float* wh, const float* bh, const float* idgb, int id_ld, float slope,
                                    void* out, int ldo, void* ws, int64_t ws_bytes, void* stream) {
  return aad_layer(dtype, h_in, ldh, z_attr, lda, B, H, W, C, Ca, gbw_packed, Npad, Kpad, gbb, wh, bh, idgb, id_ld, slope,
                   out, ldo, ws, ws_bytes, 0, nullptr, 0, stream);
}

// Test support: ghost_aad_layer_nhwc as the runtime runs the layer at low resolution: a split of the GEMM's K, and
// the arrival counters given to both the statistics and the GEMM (launches on one stream share the words)
extern "C" int ghost_aad_layer_rt_nhwc(int dtype, const void* h_in, int ldh, const void* z_attr, int lda, int B, int H,
                                       int W, int C, int Ca, const void* gbw_packed, int Npad, int Kpad,
                                       const float* gbb, const float* wh, const float* bh, const float* idgb, int id_ld,
                                       float slope, void* out, int ldo, void* ws, int64_t ws_bytes, int split_k,
                                       unsigned* sem, int nsem, void* stream) {
  if (split_k < 0 || ws_bytes < 0) return fail(GHOST_EINVAL, "ghost_aad_layer_rt_nhwc: split_k and ws_bytes must be >= 0");
  if (!sem_ok(sem, nsem)) return fail(GHOST_EINVAL, "ghost_aad_layer_rt_nhwc: sem / nsem must be (NULL, 0) or nsem > 0 words");
  if (!h_in || !z_attr || !gbw_packed || !gbb || !wh || !bh || !idgb || !out || B < 1 || H < 1 || W < 1 || C < 1 || Ca < 1)
    return fail(GHOST_EINVAL, "ghost_aad_layer_rt_nhwc: null argument or empty shape");
  return aad_layer(dtype, h_in, ldh, z_attr, lda, B, H, W, C, Ca, gbw_packed, Npad, Kpad, gbb, wh, bh, idgb, id_ld, slope,
                   out, ldo, ws, ws_bytes, split_k, sem, nsem, stream);
}

static int aad_layer(int dtype, const void* h_in, int ldh, const void* z_attr, int lda, int B, int H, int W, int C, int Ca,
                     const void* gbw_packed, int Npad, int Kpad, const float* gbb, const float* wh, const float* bh,
                     const float* idgb, int id_ld, float slope, void* out, int ldo, void* ws, int64_t ws_bytes,
                     int split_k, unsigned* sem, int nsem, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int HW = H * W;
  // workspace: stat [B][C][2] | mask [B*HW] | scratch (max of IN partials and split-K partials)
  const size_t stat_b = align_up((size_t)B * C * 2 * sizeof(float));
  const size_t mask_b = align_up((size_t)B * HW * sizeof(float));
  ConvDesc d = conv_desc(dtype, dtype, z_attr, B, H, W, Ca, lda, gbw_packed, 2 * C, Npad, Kpad, CONV_FWD, 1, 1, 1, 0,
                         out, ldo);
  d.shift = gbb; d.slope = slope; d.epi = EPI_AAD;
  d.hin = h_in; d.ldh = ldh; d.idgb = idgb; d.id_ld = id_ld; d.C_aad = C;
  d.force_split = split_k; d.sem = sem; d.nsem = nsem;
  size_t sc = conv_workspace_bytes(d);
  const size_t st = in_stats_workspace_bytes(B, HW, C);
  if (st > sc) sc = st;
  char* base = align_up(ws);
  if (!ws || (size_t)ws_bytes < stat_b + mask_b + sc + 256) return fail(GHOST_ENOWS, "aad_layer: workspace too small");
  float* stat = (float*)base;
  float* mask = (float*)(base + stat_b);
  char* scratch = base + stat_b + mask_b;
  int rc = in_stats(dtype, h_in, ldh, B, HW, C, stat, scratch, sc, s, sem, nsem);
  if (rc) return fail(rc, "aad_layer: in_stats failed");
  // this entry takes gbw, not the w3 / b3 layout: Fused or Split
  if (aad_path(dtype, B, HW, C, Ca, lda, ldh, &ldo, 1, false) == AadPath::Fused) {
    rc = aad_fused(dtype, z_attr, lda, Ca, gbw_packed, Kpad, gbb, h_in, ldh, stat, wh, bh, idgb, id_ld, out, ldo, B, HW, C,
                   slope, s);
    return rc ? fail(rc, "aad_layer: fused kernel failed") : 0;
  }
  rc = aad_mask(dtype, h_in, ldh, B, HW, C, stat, wh, bh, mask, s);
  if (rc) return fail(rc, "aad_layer: mask failed");
  d.stat = stat; d.mask = mask;
  rc = conv_launch(d, scratch, sc, s);
  if (rc) return fail(rc, "aad_layer: gemm failed");
  return 0;
}

extern "C" int ghost_upsample2x_nhwc(int dtype, const void* x, int ldx, void* y, int ldy, int B, int H, int W, int C,
                                     void* stream) {
  int rc = upsample2x(dtype, x, ldx, y, ldy, B, H, W, C, (hipStream_t)stream);
  return rc ? fail(rc, "upsample2x failed") : 0;
}

extern "C" int ghost_nhwc_to_nchw(int dtype, const void* x, int ldx, int B, int H, int W, int C, void* y, void* stream) {
  int rc = nhwc_to_nchw(dtype, x, ldx, B, H, W, C, y, (hipStream_t)stream);
  return rc ? fail(rc, "nhwc_to_nchw failed") : 0;
}

extern "C" int ghost_crops_to_input_nhwc(const uint8_t* crops, int64_t crop_batch_stride, int B, int H, int W, int dtype,
                                         void* y, void* stream) {
  int rc = crops_u8_to_input(crops, crop_batch_stride, B, H, W, dtype, y, (hipStream_t)stream, 3);
  return rc ? fail(rc, "crops_to_input failed") : 0;
}

extern "C" int ghost_conv3x3_narrow_nhwc(int dtype, const void* x, int B, int H, int W, int Cin, int ldx,
                                         const void* w_narrow, int Kpad, int Cout, const void* res, int ldres,
                                         int tanh_out, void* y, int ldy, uint8_t* u8, void* stream) {
  int rc = conv3x3_narrow(dtype, x, B, H, W, Cin, ldx, w_narrow, Kpad, Cout, res, ldres, tanh_out, y, ldy, u8,
                          (hipStream_t)stream);
  return rc ? fail(rc, "conv3x3_narrow failed (H % 8, W % 32, Cin % 32 and Cout <= 3 required)") : 0;
}

extern "C" int ghost_aad_layers_v3_dt_nhwc(int dtype, const void* h_in, int ldh, int up2x, const void* z_attr, int lda,
                                           int B, int H, int W, int C, int Ca, int L, const void* const w3[],
                                           const float* const b3[], const float* const wh[], const float* const bh[],
                                           const float* const idgb[], int id_ld, float slope, void* const out[],
                                           const int ldo[], void* ws, int64_t ws_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int HW = H * W;
  if (L < 1 || L > 2) return fail(GHOST_EINVAL, "aad_v3: L must be 1 or 2");
  if (up2x & ~1) return fail(GHOST_EINVAL, "aad_v3: up2x must be 0 or 1");
  if (up2x && (H % 2 || W % 2 || (C != 64 && C != 128)))
    return fail(GHOST_EINVAL, "aad_v3: up2x needs even H, W and C in {64, 128}");
  // aad_wide: one layer, C in {256, 512, 1024}, Ca <= 512, where the all-channel kernel does not fit
  const AadPath path = aad_path(dtype, B, HW, C, Ca, lda, ldh, ldo, L);
  const bool wide = path == AadPath::Wide;
  if (wide ? (L != 1 || up2x) : path != AadPath::V3)
    return fail(GHOST_EINVAL, "aad_v3 / aad_wide: unsupported shape (bf16 / fp16, a planner's (C, Ca), enough pixels; "
                              "aad_wide: one layer, no upsample)");
  const size_t stat_b = align_up((size_t)B * C * 2 * sizeof(float));
  const size_t sc = in_stats_workspace_bytes(B, HW, C);
  char* base = align_up(ws);
  if (!ws || (size_t)ws_bytes < stat_b + sc + 256) return fail(GHOST_ENOWS, "aad_v3: workspace too small");
  float* stat = (float*)base;
  int rc = up2x ? in_stats_up2x(dtype, h_in, ldh, B, H / 2, W / 2, C, stat, base + stat_b, sc, s)
                : in_stats(dtype, h_in, ldh, B, HW, C, stat, base + stat_b, sc, s);
  if (rc) return fail(rc, "aad_v3: in_stats failed");
  if (wide) {
    const size_t mask_b = align_up((size_t)B * HW * sizeof(float));
    if ((size_t)ws_bytes < stat_b + sc + mask_b + 256) return fail(GHOST_ENOWS, "aad_wide: workspace too small");
    float* mask = (float*)(base + stat_b + sc);
    rc = aad_mask(dtype, h_in, ldh, B, HW, C, stat, wh[0], bh[0], mask, s);
    if (rc) return fail(rc, "aad_wide: aad_mask failed");
    AadWideDesc w = aad_wide_desc(dtype, z_attr, lda, Ca, h_in, ldh, stat, B, HW, C, id_ld, slope);
    aad_wide_set_layer(w, w3[0], b3[0], wh[0], bh[0], idgb[0], mask, out[0], ldo[0]);
    rc = aad_wide(w, s);
    return rc ? fail(rc, "aad_wide launch failed") : 0;
  }
  AadV3Desc d = aad_v3_desc(dtype, z_attr, lda, Ca, h_in, ldh, stat, B, H, W, C, id_ld, slope, up2x != 0);
  d.L = L;
  for (int l = 0; l < L; ++l) aad_v3_set_layer(d, l, w3[l], b3[l], wh[l], bh[l], idgb[l], out[l], ldo[l]);
  rc = aad_v3(d, s);
  return rc ? fail(rc, "aad_v3 launch failed") : 0;
}

extern "C" int ghost_aad_layers_v3_nhwc(const void* h_in, int ldh, int up2x, const void* z_attr, int lda, int B, int H,
                                        int W, int C, int Ca, int L, const void* const w3[], const float* const b3[],
                                        const float* const wh[], const float* const bh[], const float* const idgb[],
                                        int id_ld, float slope, void* const out[], const int ldo[], void* ws,
                                        int64_t ws_bytes, void* stream) {
  return ghost_aad_layers_v3_dt_nhwc(GHOST_BF16, h_in, ldh, up2x, z_attr, lda, B, H, W, C, Ca, L, w3, b3, wh, bh, idgb,
                                     id_ld, slope, out, ldo, ws, ws_bytes, stream);
}

extern "C" int64_t ghost_aad_plan(int dtype, int B, int H, int W, int C, int Ca, int L, int up2x, int zp_mask,
                                  float slope, int lda, int ldh, const int ldo[], char* buf, int64_t cap) {
  if (L < 1 || L > 2 || !ldo || (up2x & ~1) || (zp_mask & ~3) || cap < 0 || (cap > 0 && !buf))
    return fail(GHOST_EINVAL, "aad_plan: bad argument");
  const int HW = H * W;
  PlanSig sig;
  sig.s[0] = 0;
  const AadPath path = aad_path(dtype, B, HW, C, Ca, lda, ldh, ldo, L);
  // the planners read no pointer but zw[l], and of that only whether it is set
  if (path == AadPath::V3) {
    AadV3Desc d = aad_v3_desc(dtype, nullptr, lda, Ca, nullptr, ldh, nullptr, B, H, W, C, 0, slope, up2x != 0);
    d.L = L;
    for (int l = 0; l < L; ++l) {
      aad_v3_set_layer(d, l, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ldo[l]);
      if (zp_mask >> l & 1) d.zw[l] = &sig;
    }
    d.zwld = 2 * C;   // the narrow conv layout's row of both K halves
    const AadV3Plan p = aad_v3_plan(d);
    if (p.kernel != AadV3Kernel::None) sig = aad_v3_signature(p, d);
  } else if (path == AadPath::Wide && !up2x && !zp_mask) {
    AadWideDesc d = aad_wide_desc(dtype, nullptr, lda, Ca, nullptr, ldh, nullptr, B, HW, C, 0, slope);
    aad_wide_set_layer(d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ldo[0]);
    const AadWidePlan p = aad_wide_plan(d, true);
    if (p.kernel != AadWideKernel::None) sig = aad_wide_signature(p, d);
  }
  if (!sig.s[0]) return fail(GHOST_EINVAL, "aad_plan: no aad_v3 / aad_wide kernel takes this shape");
  if (cap > 0) snprintf(buf, (size_t)cap, "%s", sig.s);
  return (int64_t)strlen(sig.s) + 1;
}

extern "C" int64_t ghost_conv_plan(int ti, int to, int kind, int B, int H, int W, int Cin, int ldx, int N, int Npad,
                                   int Kpad, int kh, int kw, int stride, int pad, int ldy, int epi, int split_k,
                                   int min_wgs, int nsem, int ncu, int flags, int64_t* ws_bytes, char* buf, int64_t cap) {
  if ((kind != CONV_FWD && kind != CONV_T4S2) || (epi != EPI_STD && epi != EPI_AAD) || split_k < 0 || nsem < 0 ||
      ncu < 1 || (flags & ~GHOST_CONV_PLAN_FLAGS) || cap < 0 || (cap > 0 && !buf))
    return fail(GHOST_EINVAL, "conv_plan: bad argument");
  alignas(16) static char mem[16];   // stands for every pointer: the planners ask only whether one is set and aligned
  float* const fp = reinterpret_cast<float*>(mem);
  ConvDesc d = conv_desc(ti, to, mem, B, H, W, Cin, ldx, mem, N, Npad, Kpad, kind, kh, kw, stride, pad, mem, ldy);
  d.scale = fp; d.shift = fp;
  d.epi = epi; d.force_split = split_k; d.min_wgs = min_wgs;
  if (nsem) { d.sem = reinterpret_cast<unsigned*>(mem); d.nsem = nsem; }
  if (epi == EPI_AAD) { d.C_aad = N / 2; d.hin = mem; d.ldh = N / 2; d.stat = d.idgb = d.mask = fp; d.id_ld = N; }
  if (flags & GHOST_CONV_PLAN_RES) { d.res = mem; d.ldres = ldy; }
  d.res_first = (flags & GHOST_CONV_PLAN_RES_FIRST) != 0;
  if (flags & GHOST_CONV_PLAN_PRELU) d.prelu = fp;
  if (flags & GHOST_CONV_PLAN_Y2) { d.y2 = mem; d.ldy2 = ldy; d.scale2 = d.shift2 = fp; }
  if (flags & GHOST_CONV_PLAN_U8) d.u8 = reinterpret_cast<uint8_t*>(mem);
  d.tanh_out = (flags & GHOST_CONV_PLAN_TANH) != 0;
  if (flags & GHOST_CONV_PLAN_IN_PART) d.in_part = fp;
  if (!conv_desc_ok(d)) return fail(GHOST_EINVAL, "conv_plan: conv_launch rejects this descriptor");
  std::string text;
  switch (conv_path(d)) {
    case ConvPath::Halo3x3: {
      const HaloPlan p = halo_plan(d, ncu);
      if (d.in_part && !p.stats) return fail(GHOST_EINVAL, "conv_plan: this halo plan writes no InstanceNorm partials");
      text = halo_signature(p, d).s;
      break;
    }
    case ConvPath::First: text = conv_first_signature(d).s; break;
    case ConvPath::Stem3x3: text = conv_stem3x3_signature(d).s; break;
    case ConvPath::ConvTHalo: text = convT_halo_signature(d).s; break;
    case ConvPath::S2Patch: text = conv_s2_patch_signature(d).s; break;
    case ConvPath::Igemm: {
      const IgemmPlan p = igemm_plan(d);
      if (p.kernel == IgemmKernel::None) return fail(GHOST_EINVAL, "conv_plan: no implicit-GEMM instance takes this descriptor");
      text = igemm_signature(p, d).s;
      if (p.reduce != IgemmReduce::None) text += std::string("\n") + igemm_reduce_signature(p, d).s;
      break;
    }
  }
  if (ws_bytes) *ws_bytes = (int64_t)conv_workspace_bytes(d);
  if (cap > 0) snprintf(buf, (size_t)cap, "%s", text.c_str());
  return (int64_t)text.size() + 1;
}

extern "C" int ghost_aad_mask_nhwc(int dtype, const void* h, int ldh, int B, int HW, int C, float* stat, const float* wh0,
                                   const float* bh0, float* mask0, const float* wh1, const float* bh1, float* mask1,
                                   int small, void* stream) {
  if (!h || !stat || !wh0 || !bh0 || !mask0 || (wh1 && (!bh1 || !mask1)))
    return fail(GHOST_EINVAL, "aad_mask: null argument");
  if (B < 1 || HW < 1 || C < 1) return fail(GHOST_EINVAL, "aad_mask: empty shape");
  if (small) {
    if (!stats_mask_small_ok(dtype, HW, C, ldh))
      return fail(GHOST_EINVAL, "aad_mask: small form needs HW <= 16, C <= 1024, C and ldh multiples of the vector");
    int rc = stats_mask_small(dtype, h, ldh, B, HW, C, stat, wh0, bh0, mask0, wh1, bh1, mask1, (hipStream_t)stream);
    return rc ? fail(rc, "stats_mask_small failed") : 0;
  }
  int rc = aad_mask2(dtype, h, ldh, B, HW, C, stat, wh0, bh0, mask0, wh1, bh1, mask1, (hipStream_t)stream);
  return rc ? fail(rc, "aad_mask2 failed") : 0;
}
