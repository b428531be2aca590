/* ghost_amd — C ABI of the MI355X-native GHOST swap forward path.
 *
 * This is the drop-in boundary for the per-frame face-swap hot path of GHOST
 * (postworthy/ghost, a fork of sber-swap): the AEI_Net generator = attribute
 * encoder + AAD ResBlk decoder.  Every entry point takes plain device pointers,
 * sizes and an hipStream_t (passed as void*), returns an int status
 * (0 = success, <0 = invalid argument / state, >0 = hipError_t), never throws,
 * and never allocates device memory on the hot path (the caller supplies the
 * workspace).  ghost_last_error() describes the last failure of the calling thread.
 *
 * Reference interfaces replaced (paths under the reference repository):
 *   network/AEI_Net.py:143-151   AEI_Net(backbone, num_blocks, c_id)        -> ghost_aei_create
 *   inference.py:27-30           G.load_state_dict(...); .cuda(); .half()   -> ghost_aei_bind (prepacked)
 *   network/AEI_Net.py:153-156   AEI_Net.forward(Xt, z_id) -> (Y, attr)     -> ghost_aei_forward
 *   network/AEI_Net.py:158-159   AEI_Net.get_attr(X)                       -> ghost_aei_get_attr
 *   utils/inference/faceshifter_run.py:5-22 + utils/inference/core.py:13-26
 *                                faceshifter_batch(transform_target_to_torch(crops)) -> ghost_aei_swap_u8
 *   network/AADLayer.py:28-29 + utils/inference/faceshifter_run.py:15-16
 *                                fc1/fc2(z_id) per AADLayer, once per source identity -> ghost_aei_identity_table,
 *                                                                          ghost_aei_swap_u8_indexed
 *   network/AADLayer.py:20-38    AADLayer.forward(h_in, z_attr, z_id)       -> ghost_aad_layer_nhwc
 *   network/AEI_Net.py:19-24     conv4x4 (Conv 4x4/s2 + BN + LReLU)         -> ghost_conv2d_nhwc
 *   network/AEI_Net.py:27-41     deconv4x4 (ConvT 4x4/s2 + BN + LReLU + skip) -> ghost_conv_transpose4x4s2_nhwc
 *   network/AADLayer.py:64,71    Conv2d 3x3 of AAD_ResBlk (+ residual)     -> ghost_conv2d_nhwc
 *   network/AADLayer.py:16,24    InstanceNorm2d statistics                 -> ghost_instnorm_stats_nhwc
 *   network/AEI_Net.py:94,125    F.interpolate(x2, bilinear, align_corners) -> ghost_upsample2x_nhwc
 *   utils/inference/video_processing.py:134,163,184 + utils/inference/image_processing.py:18-19
 *                                cv2.warpAffine(frame, M, (224, 224)) + cv2.resize(crop, (256, 256)) -> ghost_align_crops_u8
 *   models/networks/normalization.py:93-107  SPADE: BN(x) * gamma + beta (+ InstanceNorm / activation / nearest x2)
 *                                                                          -> ghost_norm_modulate_nhwc
 *   models/networks/generator.py:313-351     SimplifiedLIP / lip2d         -> ghost_lip_pool_nhwc
 *
 * Activations crossing this ABI are NHWC with an explicit channel stride `ld`
 * (elements between consecutive pixels).  Packed weight layouts are documented
 * in INTEGRATION.md and produced by ghost_amd/network/pack.py.
 */
#ifndef GHOST_AMD_H
#define GHOST_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { GHOST_DTYPE_F32 = 0, GHOST_DTYPE_BF16 = 1, GHOST_DTYPE_F16 = 2, GHOST_DTYPE_U8 = 3 };
enum { GHOST_OK = 0, GHOST_EINVAL = -1, GHOST_ENOTREADY = -2, GHOST_ENOWS = -3 };

typedef struct ghost_aei ghost_aei;

const char* ghost_version(void);
const char* ghost_last_error(void);

/* ---- whole-network handle (one per device) ---------------------------------------- */
/* backbone: "unet" | "linknet" | "resnet" (MLAttrEncoderResnet, network/resnet.py:147-149); dtype: compute/storage dtype of activations and
 * conv weights (GHOST_DTYPE_F32 = parity path, GHOST_DTYPE_BF16 = throughput path). */
int ghost_aei_create(const char* backbone, int num_blocks, int c_id, int dtype, ghost_aei** out);
void ghost_aei_destroy(ghost_aei* h);
/* bind one prepacked weight tensor (device pointer, numel elements) under its slot name */
int ghost_aei_bind(ghost_aei* h, const char* name, const void* dev_ptr, int64_t numel);
/* number of slots still unbound (0 = ready); name of the first missing one in ghost_last_error() */
int ghost_aei_missing(ghost_aei* h);
/* geometry of z_attr_k (k = 1..8): channels, height, width (NHWC contiguous) */
int ghost_aei_attr_geometry(ghost_aei* h, int level, int* C, int* H, int* W);
/* device workspace needed by one forward of batch B (attr buffers supplied by the caller) */
int64_t ghost_aei_workspace_bytes(ghost_aei* h, int B);

/* AEI_Net.forward.  xt: [B,3,256,256] addressed with element strides xt_strides (any
 * layout, e.g. the permuted NHWC view of core.py:24), dtype f32/f16/bf16.  z_id: [B, c_id]
 * rows with row stride zid_row_stride.  y_nhwc: [B,256,256,3] in the handle dtype (tanh
 * output).  y_u8_bgr (optional): [B,256,256,3] uint8 BGR.  attr_nhwc: 8 device buffers
 * with the geometry above in the handle dtype (all required). */
int ghost_aei_forward(ghost_aei* h, const void* xt, int xt_dtype, const int64_t xt_strides[4], int B,
                      const void* z_id, int zid_dtype, int64_t zid_row_stride, void* y_nhwc, uint8_t* y_u8_bgr,
                      void* const attr_nhwc[8], void* ws, int64_t ws_bytes, void* stream);
/* AEI_Net.get_attr: the encoder only */
int ghost_aei_get_attr(ghost_aei* h, const void* xt, int xt_dtype, const int64_t xt_strides[4], int B,
                       void* const attr_nhwc[8], void* ws, int64_t ws_bytes, void* stream);
/* faceshifter_batch on uint8 BGR crops [B,256,256,3] (crop_batch_stride bytes apart):
 * normalise -> AEI_Net -> ((Y*0.5+0.5)*255)[...,BGR].uint8 into out_u8 [B,256,256,3].
 * y_nhwc and attr buffers come from the workspace. */
int64_t ghost_aei_swap_workspace_bytes(ghost_aei* h, int B);
int ghost_aei_swap_u8(ghost_aei* h, const uint8_t* crops, int64_t crop_batch_stride, int B, const void* z_id,
                      int zid_dtype, int64_t zid_row_stride, uint8_t* out_u8, void* ws, int64_t ws_bytes,
                      void* stream);

/* Per-identity projection table (AADLayer.py:28-29 fc1/fc2 of every AADLayer, AEI_Net.py:101 up1; a source
 * embedding's gamma_id / beta_id / m1 rows do not depend on the target frame, faceshifter_run.py:15-16 repeats one
 * z_id over the batch): computed once per (identity, weight version) and gathered per sample by identity_index.
 * ghost_aei_identity_table writes the rows of n_ident z_id rows (any float dtype, row stride zid_row_stride) into
 * table (device, 256-byte aligned, ghost_aei_identity_table_bytes(h, n_ident) bytes; workspace
 * ghost_aei_identity_table_workspace_bytes).  The table holds results of the handle's bound weights: rebuild it after
 * re-binding.  Rows are bit-identical to the projections a ghost_aei_swap_u8 of up to 64 frames computes.
 * ghost_aei_swap_u8_indexed = ghost_aei_swap_u8 with sample b's identity rows taken from table row
 * identity_index[b] (device int32 [B], values in [0, n_ident); an out-of-range value is clamped to that range, not
 * reported: validate on the host).  table_bytes: the table's size, checked against
 * ghost_aei_identity_table_bytes(h, n_ident) (GHOST_EINVAL if smaller), so the clamped gather stays inside the table.
 * Workspace: ghost_aei_swap_workspace_bytes. */
int64_t ghost_aei_identity_table_bytes(ghost_aei* h, int n_ident);
int64_t ghost_aei_identity_table_workspace_bytes(ghost_aei* h, int n_ident);
int ghost_aei_identity_table(ghost_aei* h, const void* z_id, int zid_dtype, int64_t zid_row_stride, int n_ident,
                             void* table, int64_t table_bytes, void* ws, int64_t ws_bytes, void* stream);
int ghost_aei_swap_u8_indexed(ghost_aei* h, const uint8_t* crops, int64_t crop_batch_stride, int B, const void* table,
                              int n_ident, int64_t table_bytes, const int32_t* identity_index, uint8_t* out_u8, void* ws,
                              int64_t ws_bytes, void* stream);

/* Per-handle plan options (defaults are the measured choices; every forward of the handle uses them):
 *   GHOST_AEI_OPT_FUSE_UPSAMPLE (1): AADBlk8's first AADLayer pair samples upsample2x(AADBlk7 output) on the fly
 *                                    instead of reading a materialised upsample (0 materialises it)
 *   GHOST_AEI_OPT_FUSE_STATS (1):    the persistent 3x3 conv emits the InstanceNorm partials of its output
 *                                    (0: a separate statistics pass)
 *   GHOST_AEI_OPT_TWO_STREAMS (1):   forward / swap run the attribute encoder's up path (deconv1..6 and the
 *                                    z_attr8 upsample) on a second, handle-owned HIP stream, overlapped with
 *                                    the generator's AADBlk k, which waits only for z_attr_k; the caller's
 *                                    stream waits for that stream before the call's last launch, so the
 *                                    ordering seen by the caller is unchanged (0: one stream; batches of
 *                                    fewer than 8 frames always run on one stream).  Same results.
 *   GHOST_AEI_OPT_TAP_PARTIALS (2):  bf16, C = 64 output block (AADBlk8): the 3x3 conv to 3 channels is
 *                                    contracted in its producers: each AADLayer that feeds it writes the
 *                                    per-tap partial sums of its channels, pre-summed along 8-pixel row
 *                                    segments (fp16, 15 per pixel) instead of its 64 bf16 channels, and a
 *                                    gather kernel sums three rows of them (+ tanh, uint8).
 *                                    2: both the h path and last_add_block's x'; 1: the h path only (x' is
 *                                    written and the narrow conv contracts it); 0: neither.  The partials
 *                                    are rounded to fp16 once per row sum (the extra rounding the
 *                                    bf16-storage emulation of oracle/aei_ref.py models).
 *   GHOST_AEI_OPT_FUSE_REDUCE (1):   split-K GEMMs with small partial tiles and the InstanceNorm statistics
 *                                    passes reduce their partials in the last workgroup to finish (arrival
 *                                    counters in the workspace, zeroed once per call) instead of a second
 *                                    kernel: the same sums in the same order, the same bytes, fewer launches
 *                                    (0: the separate reduction kernels).
 * value is 0 or 1 (TAP_PARTIALS: 0..2).  A handle is not shared across threads without external
 * synchronisation.  Two-stream calls of ALL handles on one device share one up-path stream (below): while one
 * call is being captured into a HIP graph (stream capture of the caller's stream), no other handle on that device
 * may run a two-stream call from another thread — its up-path work would join the capture — so capture with
 * GHOST_AEI_OPT_TWO_STREAMS = 0 (ghost_amd.inference.GraphedSwap's default) or serialise the calls. */
enum {
  GHOST_AEI_OPT_FUSE_UPSAMPLE = 0,
  GHOST_AEI_OPT_FUSE_STATS = 1,
  GHOST_AEI_OPT_TWO_STREAMS = 2,
  GHOST_AEI_OPT_TAP_PARTIALS = 3,
  GHOST_AEI_OPT_FUSE_REDUCE = 4,
  GHOST_AEI_NOPT = 5
};
int ghost_aei_set_option(ghost_aei* h, int option, int value);
int ghost_aei_get_option(ghost_aei* h, int option, int* value);
/* Diagnostic taps (parity bisection): while set, every forward / swap of the handle copies the stored
 * output of AADBlk k (k = 1..7, NHWC [B, 2^k, 2^k, cout_k] in the handle dtype, before the x2 upsample)
 * into taps[k-1] when that pointer is non-NULL (taps[7] is unused: AADBlk8's output is Y).
 * NULL taps clears them. */
int ghost_aei_set_taps(ghost_aei* h, void* const taps[8]);

/* the up-path stream on `device` as this handle uses it: ONE low-priority stream per device for the whole process,
 * shared by every handle on that device, created by the first two-stream forward / swap there and never destroyed
 * (valid until the process exits; NULL before this handle's first two-stream call there, or when stream creation
 * failed and the handle runs on one stream).  Diagnostics of hardware-queue sharing (tools/leg_probe.py). */
int ghost_aei_up_stream(ghost_aei* h, int device, void** stream);

/* per-kernel-class device timing with HIP events (bench instrumentation).
 * class_mask bit i enables class i; classes: 0 AAD kernels (all stages), 1 the block-input AAD
 * kernel at 256x256 (through-upsample: aad_v5, aad_v3.hip), 2 conv3x3 (all), 3 conv3x3 at 256x256, 4 IN stats + mask,
 * 5 encoder, 6 upsample, 7 identity projections. */
int ghost_aei_profile(ghost_aei* h, int class_mask);
/* after the stream is synchronised: total ms, launches, algorithmic bytes and flops of class i */
int ghost_aei_profile_read(ghost_aei* h, int cls, double* ms, int64_t* launches, double* bytes, double* flops);
/* class 1's in-kernel clock (armed by ghost_aei_profile with bit 1 set, on the current device): the sum over
 * its launches since then of (latest wave end - earliest workgroup start), in microseconds, read from the
 * kernel's own wall-clock stamps (hipDeviceAttributeWallClockRate) — the kernel's execution span, which
 * unlike a HIP-event bracket does not include queueing behind other streams' kernels.  After a sync.
 * kernel_version (may be NULL): generation of the class-1 AAD kernel that ran last (4: aad_v4, 5: aad_v5). */
int ghost_aei_profile_clock(ghost_aei* h, double* us_total, int64_t* launches, int* kernel_version);

/* ---- single operators (NHWC, per-op parity tests and callers of single layers) ------ */
/* Conv2d kh x kw / stride / pad (+ per-channel scale/shift, leaky slope, residual, tanh).
 * w_packed: [Npad][Kpad] with K index (ky*kw + kx)*Cin + c. */
int ghost_conv2d_nhwc(int dtype, const void* x, int B, int H, int W, int Cin, int ldx, const void* w_packed, int Cout,
                      int Npad, int Kpad, int kh, int kw, int stride, int pad, const float* scale, const float* shift,
                      float slope, const void* res, int ldres, int tanh_out, void* y, int ldy, void* ws,
                      int64_t ws_bytes, void* stream);
/* Epilogue of ghost_conv2d_ex_nhwc, applied per output (pixel, channel n):
 *   v = acc*scale[n] + shift[n];  if res_first: v += res;  v = v > 0 ? v : v*(prelu ? prelu[n] : slope);
 *   if !res_first: v += res;  if tanh_out: v = tanh(v);  y = v;  if y2: y2 = v*scale2[n] + shift2[n]
 * Covers Conv+BN+LeakyReLU (AEI_Net.py:19-24), the ResNet Bottleneck tail relu(bn3(conv3) + residual)
 * (network/resnet.py:72-78), and the ArcFace IBasicBlock (conv + BN + PReLU; BN of the next block's
 * input written as the second output).  Pointers may be NULL (scale/shift default 1/0). */
typedef struct ghost_conv_epi {
  const float* scale;
  const float* shift;
  float slope;
  const float* prelu;
  const void* res;
  int ldres;
  int res_first;
  int tanh_out;
  void* y2;
  int ldy2;
  const float* scale2;
  const float* shift2;
  int split_k;   /* 0 = the planner's choice; n > 0 forces n K-splits (tests of the split-K reduction) */
} ghost_conv_epi;
int ghost_conv2d_ex_nhwc(int dtype, const void* x, int B, int H, int W, int Cin, int ldx, const void* w_packed,
                         int Cout, int Npad, int Kpad, int kh, int kw, int stride, int pad, const ghost_conv_epi* epi,
                         void* y, int ldy, void* ws, int64_t ws_bytes, void* stream);
/* ghost_conv2d_ex_nhwc whose kernel also writes the InstanceNorm partials of its output, merged into
 * stat [B][Cout][2] (mean, rstd of the stored y per (sample, channel)) as the generator's 3x3 convs do it.  Only the
 * persistent 3x3 kernels on exact 16 x 32 tiles or whole 8 x 8 images write partials: for any other descriptor
 * GHOST_EINVAL, nothing launched.  Workspace: B * nrec * Cout * 2 floats + 256 bytes, nrec = H/16 * W/32 * 8 records
 * per (sample, channel) (8 x 8 images: 1); GHOST_ENOWS names the need. */
int ghost_conv2d_stats_nhwc(int dtype, const void* x, int B, int H, int W, int Cin, int ldx, const void* w_packed,
                            int Cout, int Npad, int Kpad, int kh, int kw, int stride, int pad,
                            const ghost_conv_epi* epi, void* y, int ldy, float* stat, void* ws, int64_t ws_bytes,
                            void* stream);
/* Conv2d 3x3/p1 to Cout <= 3 channels (the generator's RGB output): halo-tiled per-tap partial
 * sums; w_narrow [32][Kpad], row (ky*3+kx)*Cout + o; optional residual, tanh and BGR uint8 copy. */
int ghost_conv3x3_narrow_nhwc(int dtype, const void* x, int B, int H, int W, int Cin, int ldx, const void* w_narrow,
                              int Kpad, int Cout, const void* res, int ldres, int tanh_out, void* y, int ldy,
                              uint8_t* u8, void* stream);
/* ConvTranspose2d 4x4/s2/p1 as four 2x2 sub-pixel phases; w_packed: [4][Npad][Kpad],
 * phase = 2*py + px, K index (ty*2 + tx)*Cin + c. */
int ghost_conv_transpose4x4s2_nhwc(int dtype, const void* x, int B, int H, int W, int Cin, int ldx,
                                   const void* w_packed, int Cout, int Npad, int Kpad, const float* scale,
                                   const float* shift, float slope, const void* res, int ldres, void* y, int ldy,
                                   void* ws, int64_t ws_bytes, void* stream);
/* fp32 GEMM y[B, N] = x[B, K] * W^T + bias (Linear / ConvT-on-1x1); out dtype f32 or bf16 */
int ghost_linear_f32(const float* x, int B, int K, const float* w_packed, int N, int Npad, int Kpad,
                     const float* bias, int out_dtype, void* y, int ldy, void* ws, int64_t ws_bytes, void* stream);
/* InstanceNorm statistics: stat[b][c] = (mean, 1/sqrt(var+1e-5)) */
int ghost_instnorm_stats_nhwc(int dtype, const void* x, int B, int HW, int C, int ldx, float* stat, void* ws,
                              int64_t ws_bytes, void* stream);
/* the same statistics of upsample2x(x) (bilinear x2, align_corners, values rounded to dtype as the
 * upsample kernel stores them) for an [B, H, W, C] source, without materialising the upsample
 * (AEI_Net.py:137 feeding AADLayer.py:16's InstanceNorm) */
int ghost_instnorm_stats_up2x_nhwc(int dtype, const void* x, int B, int H, int W, int C, int ldx, float* stat,
                                   void* ws, int64_t ws_bytes, void* stream);
/* AADLayer.forward: gbw_packed [Npad][Kpad] rows interleaved per 16 channels
 * (gamma c0..15, beta c0..15, gamma c16..31, ...), gbb the matching biases (fp32);
 * wh [C] / bh [1] the conv_h weights; idgb [B][id_ld] holds gamma_id at c and beta_id
 * at C + c (fp32).  slope = 1: plain AADLayer; slope = 0: fused following ReLU. */
int ghost_aad_layer_nhwc(int dtype, const void* h_in, int ldh, const void* z_attr, int lda, int B, int H, int W, int C,
                         int Ca, const void* gbw_packed, int Npad, int Kpad, const float* gbb, const float* wh,
                         const float* bh, const float* idgb, int id_ld, float slope, void* out, int ldo, void* ws,
                         int64_t ws_bytes, void* stream);
/* One or two AADLayers (bf16, C in {64,128}) that read the same h_in and z_attr, in one pass:
 * w3/b3 per layer in the permuted layout of pack.py pack_aad_v3; InstanceNorm statistics of h_in
 * are computed into the workspace first.  up2x = 1: h_in is upsample2x of the [B, H/2, W/2, C]
 * tensor passed as h_in (F.interpolate of AEI_Net.py:135-137 fused into the AADLayer read; C in {64, 128}).
 * C = 256 (L = 1, Ca in {64, 128}) keeps all channels in one workgroup; C in {256, 512, 1024} otherwise
 * (L = 1, Ca <= 512) runs the per-channel-tile kernel of aad_wide.hip. */
int ghost_aad_layers_v3_nhwc(const void* h_in, int ldh, int up2x, const void* z_attr, int lda, int B, int H, int W,
                             int C, int Ca, int L, const void* const w3[], const float* const b3[],
                             const float* const wh[], const float* const bh[], const float* const idgb[], int id_ld,
                             float slope, void* const out[], const int ldo[], void* ws, int64_t ws_bytes,
                             void* stream);
/* Test support: ghost_aad_layers_v3_nhwc with the 16-bit storage type (GHOST_BF16 or GHOST_F16) as an argument;
 * ghost_aad_layers_v3_nhwc is this with GHOST_BF16. */
int ghost_aad_layers_v3_dt_nhwc(int dtype, const void* h_in, int ldh, int up2x, const void* z_attr, int lda, int B,
                                int H, int W, int C, int Ca, int L, const void* const w3[], const float* const b3[],
                                const float* const wh[], const float* const bh[], const float* const idgb[],
                                int id_ld, float slope, void* const out[], const int ldo[], void* ws, int64_t ws_bytes,
                                void* stream);
/* Test support: the AAD mask kernels alone.  mask_l[b*HW + p] = sigmoid(sum_c wh_l[c] (h[p,c] - mean[b,c]) rstd[b,c]
 * + bh_l) in fp32 for one (wh1 == NULL) or two layers reading the same h [B, HW, C] (ldh).  small = 0: stat
 * ([B][C][2] mean, rstd) is an input; small = 1: the one-launch statistics + mask kernel of the HW <= 16 stages,
 * which also writes stat (GHOST_EINVAL unless HW <= 16 and C <= 1024). */
int ghost_aad_mask_nhwc(int dtype, const void* h, int ldh, int B, int HW, int C, float* stat, const float* wh0,
                        const float* bh0, float* mask0, const float* wh1, const float* bh1, float* mask1, int small,
                        void* stream);
int ghost_upsample2x_nhwc(int dtype, const void* x, int ldx, void* y, int ldy, int B, int H, int W, int C,
                          void* stream);
int ghost_nhwc_to_nchw(int dtype, const void* x, int ldx, int B, int H, int W, int C, void* y, void* stream);
/* transform_target_to_torch (core.py:13-26): uint8 BGR NHWC crops -> RGB NHWC in [-1,1] (dtype f32/bf16) */
int ghost_crops_to_input_nhwc(const uint8_t* crops, int64_t crop_batch_stride, int B, int H, int W, int dtype, void* y,
                              void* stream);
/* ---- use_sr face enhancer (LIPSPADEGenerator; inference.py:42-50, models/networks/generator.py:353-388,
 *      models/networks/normalization.py:63-107): the two passes its convs do not cover ---------------------
 * out[b,y,x,c] = act((src - mean) * rstd * gamma + beta), act(v) = v > 0 ? v : v * slope (0: ReLU, 1: none).
 * stat = [Bs][C][2] (mean, rstd) in ghost_instnorm_stats_nhwc's layout: Bs = B per-sample (InstanceNorm), Bs = 1
 * one record for the whole batch (train-mode BatchNorm: ghost_instnorm_stats_nhwc with B = 1, HW = B*H*W).
 * gb (optional, NULL: gamma = 1, beta = 0): one [B,H,W,ldgb] tensor of dtype holding gamma at channel c and beta
 * at C + c.  up2x = 1: src is [B,H/2,W/2,C] and is read at (y >> 1, x >> 1) (nearest x2 folded into the read; stat
 * is that of the small tensor).  GHOST_EINVAL: C % 8 != 0, odd H or W with up2x, a null src / stat / out, Bs not in
 * {1, B}, or a leading dimension / pointer that is not 16-byte aligned. */
int ghost_norm_modulate_nhwc(int dtype, const void* src, int ldx, int B, int H, int W, int C, const float* stat, int Bs,
                             const void* gb, int ldgb, float slope, int up2x, void* out, int ldo, void* stream);
/* SimplifiedLIP pooling: out[B,H/2,W/2,C] = sum3x3 x e^l / sum3x3 e^l over the 3x3 / stride 2 / pad 1 window
 * (out-of-image taps skipped), l = 12 sigmoid(((logit_raw - mean) * rstd) * w[c] + b[c]); stat = [B][C][2] instance
 * statistics of logit_raw.  GHOST_EINVAL: odd H or W, C % 8 != 0, null pointers, misaligned leading dimensions. */
int ghost_lip_pool_nhwc(int dtype, const void* x, int ldx, const void* logit_raw, int ldl, int B, int H, int W, int C,
                        const float* stat, const float* w, const float* b, void* out, int ldo, void* stream);
/* ---- ArcFace identity encoder (IResNet, the netArc GHOST loads) ------------------------
 * Replaces: inference.py:33-36 iresnet100(fp16=False) + load_state_dict + .cuda().eval();
 *   core.py:43-54 / video_processing.py:136-140 netArc(F.interpolate(normalize_and_torch_batch(crops),
 *   scale_factor=0.5, bilinear, align_corners=True)); video_processing.py:126,139-148 face matching.
 * The IResNet definition itself is not in the reference tree (download_models.sh:3): parity unpinned. */
typedef struct ghost_arc ghost_arc;
/* layers: blocks per stage ({3,13,30,3} = iresnet100); num_features: embedding size (512) */
int ghost_arc_create(const int layers[4], int num_features, int dtype, ghost_arc** out);
void ghost_arc_destroy(ghost_arc* h);
int ghost_arc_bind(ghost_arc* h, const char* name, const void* dev_ptr, int64_t numel);
int ghost_arc_missing(ghost_arc* h);
int64_t ghost_arc_workspace_bytes(ghost_arc* h, int N);
/* x: [N,3,112,112] with element strides (f32/f16/bf16/u8) -> emb fp32 [N, num_features] */
int ghost_arc_forward(ghost_arc* h, const void* x, int x_dtype, const int64_t x_strides[4], int N, float* emb,
                      void* ws, int64_t ws_bytes, void* stream);
/* uint8 aligned crops [N,H,W,3] (H = W = 224, channel order as given): normalize_and_torch_batch
 * (divide by 255 only if the batch max > 1) -> bilinear 0.5x align_corners -> IResNet -> emb */
int ghost_arc_embed_u8(ghost_arc* h, const uint8_t* crops, int64_t crop_batch_stride, int N, int H, int W,
                       float* emb, void* ws, int64_t ws_bytes, void* stream);
/* per target j: best_idx[j] = argmax_i cos(face_i, target_j) (first on ties), best_sim[j] = that
 * cosine, accepted[j] = best_sim[j] > similarity_th */
/* Diagnostic taps (parity bisection): while set, every forward copies, for stage i (0 = the stem, i >= 1 =
 * the i-th IBasicBlock in forward order), the stored residual stream X_i into taps[2i] and the next
 * BatchNorm's output BN(X_i) (the producer's second output, what the next block's conv reads) into
 * taps[2i+1], NHWC [N, H_i, W_i, C_i] in the handle dtype, where those pointers are non-NULL.
 * ntaps = 0 clears them. */
int ghost_arc_set_taps(ghost_arc* h, void* const* taps, int ntaps);
int ghost_arc_match(const float* face_emb, int F, const float* target_emb, int T, int dim, float similarity_th,
                    int32_t* best_idx, float* best_sim, int32_t* accepted, void* stream);

/* ---- 106-point face landmarks (insightface 2d106det, the `handler` GHOST builds its masks from) --------
 * Replaces: coordinate_reg/image_infer.py:141-157 Handler.get_without_detection_without_transform, called per face by
 *   utils/inference/video_processing.py:218-223.  The network is coordinate_reg/model/2d106det-symbol.json
 *   (MobileNet-v1 at width 0.5 on a 192 x 192 RGB crop, BatchNorm(fix_gamma) + per-channel PReLU after every conv).
 *   No checkpoint and no mxnet offline: parity against mxnet is unpinned.
 * dtype: storage of activations and of the pointwise / conv_15 weights (f32, bf16 or f16); the stem, every depthwise
 * conv, every BatchNorm / PReLU and the fc are fp32 arithmetic on fp32 parameters in all three.
 * Slots (ghost_amd/landmarks/pack.py): stem.w [27][16] f32; cK.dw.w [9][Cin] f32 and cK.pw.w [rup(Cout,128)][rup(Cin,32)]
 * dtype for K = 2..14; c15.w as every conv here; X.scale / X.shift / X.prelu f32 for X in {stem, cK.dw, cK.pw, c15};
 * fc.w [576][212] f32 with K = (y*3 + x)*64 + c; fc.bias [212] f32.  Every slot must be 16-byte aligned. */
typedef struct ghost_lmk ghost_lmk;
int ghost_lmk_create(int dtype, ghost_lmk** out);
void ghost_lmk_destroy(ghost_lmk* h);
int ghost_lmk_bind(ghost_lmk* h, const char* name, const void* dev_ptr, int64_t numel);
int ghost_lmk_missing(ghost_lmk* h);
int64_t ghost_lmk_workspace_bytes(ghost_lmk* h, int N);
/* the network alone: x192 uint8 [N,192,192,3], x_batch_stride bytes apart, channel order B,G,R (bgr != 0) or R,G,B
 * -> pred fp32 [N,212] (fc1's output).  N == 0 returns GHOST_OK without a launch; N <= 65535. */
int ghost_lmk_forward(ghost_lmk* h, const uint8_t* x192, int64_t x_batch_stride, int bgr, int N, float* pred, void* ws,
                      int64_t ws_bytes, void* stream);
/* get_without_detection_without_transform over a batch: crops224_bgr uint8 [N,224,224,3] -> cv2.warpAffine(crop, M,
 * (192, 192), borderValue=0.0) with M = [[0.57142857, 0, 32], [0, 0.57142857, 32]] (ghost_align_crops_u8's bytes) ->
 * BGR to RGB -> the network -> landmarks fp32 [N,106,2] = ((pred + 1) * 96) * 1.75 - 56 in the crop's pixel
 * coordinates.  pred (optional) receives fc1's output [N,212]. */
int ghost_lmk_landmarks_u8(ghost_lmk* h, const uint8_t* crops224_bgr, int64_t crop_batch_stride, int N, float* landmarks,
                           float* pred, void* ws, int64_t ws_bytes, void* stream);
/* Diagnostic taps: while set (ntaps = 4), every forward copies the stored outputs of conv_2 [N,96,96,32], conv_7
 * [N,12,12,256], conv_14 [N,6,6,512] and conv_15 [N,3,3,64] (NHWC, handle dtype) into the non-NULL taps[i].
 * ntaps = 0 clears them. */
int ghost_lmk_set_taps(ghost_lmk* h, void* const* taps, int ntaps);
/* One depthwise-separable block: d = PReLU(BN(depthwise3x3(x, stride 1 | 2, pad 1))) in fp32 from fp32 weights dw_w
 * [9][Cin] (tap ky*3 + kx), rounded once to dtype; y = PReLU(BN(d * w^T)) with the 1x1 on the matrix cores, fp32
 * accumulation and epilogue.  BN is v*scale[c] + shift[c], PReLU v > 0 ? v : v*prelu[c]; dw_* have Cin entries, scale /
 * shift / prelu Cout.  w_packed: [>= Cout][Kpad] of dtype, K = input channel, zero beyond Cin (Kpad % 32 == 0: pack_conv
 * of the 1x1 weight).  x [B,H,W,ldx], y [B,Ho,Wo,ldy], Ho = (H - 1) / stride + 1.
 * dw_tap (optional, [B,Ho,Wo,ld_tap]): also receives d; y is bit-identical with and without it.
 * Cout == 0: depthwise only, d is written to y (w_packed / scale / shift / prelu / dw_tap unused, dw_tap must be NULL).
 * GHOST_EINVAL: Cin % 8, Cout % 16 (Cout % 128 above 128), Cin > 992 with Cout > 0 (the LDS image), a pointer or
 * leading dimension that is not 16-byte aligned or is below its channel count. */
int ghost_dwsep_block_nhwc(int dtype, const void* x, int B, int H, int W, int Cin, int ldx, int stride,
                           const float* dw_w, const float* dw_scale, const float* dw_shift, const float* dw_prelu,
                           const void* w_packed, int Cout, int Kpad, const float* scale, const float* shift,
                           const float* prelu, void* y, int ldy, void* dw_tap, int ld_tap, void* stream);

/* ---- paste-back blend (get_final_video, utils/inference/video_processing.py:218-227) ----
 * For each frame f with valid[f] != 0 (valid may be NULL): warp the crop-space swap [Hs,Ws,3] u8 and
 * mask [Hs,Ws] f32 back into the frame with kornia.warp_affine semantics (bilinear, zeros,
 * align_corners=True, destination pixel sampled at mats[f] (x, y, 1), mats = the crop <- frame tfm
 * [F][2][3] fp32) and composite in place: frame = uint8(mask_t*swap_t + (1-mask_t)*frame).
 * Several identities on one frame: call once per identity, in the reference's order. */
int ghost_blend_swaps_u8(uint8_t* frames, int64_t frame_stride, int F, int H, int W, const uint8_t* swaps,
                         int64_t swap_stride, int Hs, int Ws, const float* masks, int64_t mask_stride,
                         const float* mats, const int32_t* valid, void* stream);
/* cv2.resize(src, (Wd, Hd)) INTER_LINEAR for F uint8 [Hs,Ws,3] images (OpenCV's fixed point): the
 * resize of the 256x256 swap to the 224x224 crop size that precedes the warp (video_processing.py:212,
 * image_processing.py:63). */
int ghost_resize_u8_linear(const uint8_t* src, int64_t src_stride, int F, int Hs, int Ws, uint8_t* dst,
                           int64_t dst_stride, int Hd, int Wd, void* stream);
/* get_final_image (utils/inference/image_processing.py:51-76) for one full frame [H,W,3] u8, in place: for
 * each identity j in order, swap_t = cv2.warpAffine(swaps[j] (S x S, already resized), invertAffineTransform
 * (tfm_j), BORDER_REPLICATE), mask_t = the same warp of masks[j] with the constant 0 border, final =
 * mask_t*swap_t + (1-mask_t)*final; one uint8 cast at the end.  masks are float64 [J][S][S] (face_mask_static
 * returns mask/255 of a uint8 array, masks.py:83-85: numpy float64), so the mask warp (float table weights, double
 * accumulation, as cv2 does for CV_64F) and the composite run in double as numpy does.  maps[j] = the [2][3] double
 * matrix warpAffine samples with (the inverse of invertAffineTransform(tfm_j), computed on the host as
 * OpenCV does: ghost_amd.inference.blend.cv_warp_map). */
int ghost_blend_image_u8(uint8_t* frame, int H, int W, const uint8_t* swaps, int64_t swap_stride, int J, int S,
                         const double* masks, int64_t mask_stride, const double* maps, void* stream);

/* ---- aligned crops from device-resident frames ----
 * utils/inference/image_processing.py:18-19 (crop_face) and utils/inference/video_processing.py:134,163
 * (crop_frames_and_get_transforms): cv2.warpAffine(frame, M, (S, S), borderValue=0.0) per face, and
 * video_processing.py:184 (resize_frames): cv2.resize(crop, (R, R)), from the uint8 frames [F,H,W,3] that
 * ghost_blend_swaps_u8 later composites into.  For crop n: crops[n] = warpAffine(frames[frame_index[n]], M_n, (S, S))
 * INTER_LINEAR, constant 0 border, in OpenCV's fixed point; maps[n] = the [2][3] double matrix warpAffine samples
 * with, cv2.invertAffineTransform(M_n) computed on the host in double; resized[n] = cv2.resize(crops[n], (R, R))
 * INTER_LINEAR as ghost_resize_u8_linear computes it, made in the same launch from the tile held in LDS.
 * frame_index, maps and valid are device arrays of N; valid may be NULL, valid[n] == 0 leaves row n of both outputs
 * untouched, and so does a frame_index[n] outside [0, F).  crops or resized may be NULL, not both.  The fused resize
 * covers S % 7 == 0 with R == S / 7 * 8 (224 -> 256); any other (S, R) with resized != NULL is GHOST_EINVAL: crop
 * with resized = NULL and call ghost_resize_u8_linear.  N <= 65535; N == 0 returns GHOST_OK without a launch. */
int ghost_align_crops_u8(const uint8_t* frames, int64_t frame_stride, int F, int H, int W, const int32_t* frame_index,
                         const double* maps, const int32_t* valid, int N, int S, uint8_t* crops, int64_t crop_stride,
                         uint8_t* resized, int64_t resized_stride, int R, void* stream);

/* ---- ROI video path: only each face's rectangle crosses the host link ----
 * The frames stay on the host.  Per (identity, frame) the rectangle (x0, y0, w, h) of the frame that
 * cv2.warpAffine(frame, M, (S, S)) reads and the paste-back can write (ghost_amd.inference.roi.face_rois) lives in
 * patch p of a device canvas patches [Np,Ph,Pw,3] u8 (patch_stride bytes apart, w <= Pw, h <= Ph), rectangle pixel
 * (px, py) at patches + p patch_stride + (py Pw + px) 3.
 * ghost_roi_copy_u8 issues one hipMemcpy2DAsync per patch on the stream between frame_ptrs_host[p] + (y0 W + x0) 3
 * (pitch 3 W; frame_ptrs_host[p] = the [H,W,3] host frame patch p belongs to, pinned for an asynchronous copy) and
 * the patch (pitch 3 Pw), 3 w bytes by h rows: host to device with to_device != 0, back otherwise.  rects_host is
 * the host int32 [Np][4] array; every rectangle is checked before the first copy (inside the frame, no larger than
 * the canvas: GHOST_EINVAL, nothing copied); an empty rectangle (w or h 0) is skipped.  Np == 0 returns GHOST_OK.
 * ghost_align_crops_roi_u8 = ghost_align_crops_u8 with crop n taken from patch patch_index[n]: a tap at frame pixel
 * (tx, ty) is read at (tx - x0, ty - y0) of the patch when it lies inside the rectangle and is 0 otherwise, which is
 * cv2's constant border because the rectangle lies inside the frame and covers every in-frame tap.  rects
 * (int32 [Np][4]) and patch_index (int32 [N]) are device arrays, maps the same double frame-coordinate maps; w and h
 * are clamped to the canvas, and a row with patch_index[n] outside [0, Np) or valid[n] == 0 is left untouched.  The
 * outputs, the (S, R) rule, N <= 65535 and N == 0 are those of ghost_align_crops_u8; the crops are its bytes.
 * ghost_blend_swaps_roi_u8 = ghost_blend_swaps_u8 over the rectangles only: entry n composites swaps[n] / masks[n]
 * through mats[n] (fp32 [N][2][3], frame coordinates) into patch patch_index[n], one thread per rectangle pixel,
 * writing the bytes the full-frame kernel writes.  The composite is an in-place read-modify-write: the entries of
 * one call must reference distinct patches (several identities on one patch: one call each, in the reference's
 * order).  N <= 65535; N == 0 returns GHOST_OK without a launch.  No call allocates or synchronises. */
int ghost_roi_copy_u8(uint8_t* patches, int64_t patch_stride, int Np, int Ph, int Pw, const int32_t* rects_host,
                      uint8_t* const* frame_ptrs_host, int H, int W, int to_device, void* stream);
int ghost_align_crops_roi_u8(const uint8_t* patches, int64_t patch_stride, int Np, int Ph, int Pw,
                             const int32_t* rects, const int32_t* patch_index, const double* maps,
                             const int32_t* valid, int N, int S, uint8_t* crops, int64_t crop_stride, uint8_t* resized,
                             int64_t resized_stride, int R, void* stream);
int ghost_blend_swaps_roi_u8(uint8_t* patches, int64_t patch_stride, int Np, int Ph, int Pw, const int32_t* rects,
                             const int32_t* patch_index, int N, const uint8_t* swaps, int64_t swap_stride, int Hs,
                             int Ws, const float* masks, int64_t mask_stride, const float* mats, const int32_t* valid,
                             void* stream);

/* ---- packed ROI transfer: one host-link copy per chunk of patches, not one per rectangle ----
 * The per-patch copies of ghost_roi_copy_u8 run at 5-11 GB/s and need pinned frames to be asynchronous.  Here the
 * rectangles of a plan are packed into one buffer: rectangle p = (x0, y0, w, h) occupies h rows of pitch
 * pitch_p = (3 w + 15) & ~15 bytes from byte offset_p, offset_0 = 0, offset_{p+1} = offset_p + pitch_p h_p rounded up
 * to a multiple of 256; an empty rectangle (w or h 0) takes no bytes; total = the offset after the last rectangle.
 * Offsets ascend in patch order, so the patches [p0, p1) are one contiguous byte range (one hipMemcpyAsync moves the
 * chunk), and every packed row starts 16-byte aligned.
 * ghost_roi_packed_layout (host only) writes offsets_host [Np] and *total_bytes for rects_host int32 [Np][4]; a
 * negative w or h is GHOST_EINVAL; Np == 0 gives total 0.
 * ghost_roi_pack_host (host only, no device pointer) copies the 3 w bytes of every row of every rectangle in [p0, p1)
 * between frame_ptrs_host[p] + (y0 W + x0) 3 (pitch 3 W; indexed by patch as for ghost_roi_copy_u8, any host memory)
 * and staging + offset_p (pitch pitch_p): into the staging buffer with to_staging != 0, back otherwise.  Row padding
 * and the gaps between rectangles are never written; on the way back exactly the rectangles' bytes of a frame are.
 * Before the first byte moves every rectangle of the range is checked: inside the H x W frame, a non-null frame,
 * offset_p >= 0 and a multiple of 16, offset_p + pitch_p h_p <= staging_bytes and <= offset_{p+1} (GHOST_EINVAL,
 * nothing copied).  Empty rectangles are skipped; p0 == p1 returns GHOST_OK.  The rows are split by bytes, not by
 * patch, over `threads` worker threads (0 = 8, clamped to 1..16; a short range uses fewer) that are joined before the
 * call returns; the result does not depend on threads.  Back into the frames, two rectangles of one frame that
 * overlap are the caller's error (plan_rois' merge rule makes them disjoint).
 * ghost_roi_unpack_u8 (device; rects, offsets, packed are device arrays, packed 16-byte aligned) copies the packed
 * rows of the patches [p0, p1) into the canvas of the ROI block above with to_canvas != 0 and the canvas rectangles
 * into the packed rows otherwise.  w and h are clamped to the canvas (the packed pitch stays that of the plan's w); a
 * patch whose offset is negative, not a multiple of 16, or whose offset + pitch h exceeds packed_bytes is skipped
 * before any access.  Toward the canvas only the rectangle's bytes are written; toward the packed buffer a row may be
 * written up to its pitch (padding content unspecified) and nothing past offset + pitch h; no canvas access leaves
 * the patch's Ph Pw 3 bytes.  p1 - p0 <= 65535; a null pointer or a bad canvas is GHOST_EINVAL; p0 == p1 returns
 * GHOST_OK without a launch.  No call allocates or synchronises. */
int ghost_roi_packed_layout(const int32_t* rects_host, int Np, int64_t* offsets_host, int64_t* total_bytes);
int ghost_roi_pack_host(uint8_t* staging, int64_t staging_bytes, const int32_t* rects_host,
                        const int64_t* offsets_host, uint8_t* const* frame_ptrs_host, int Np, int p0, int p1, int H,
                        int W, int to_staging, int threads);
int ghost_roi_unpack_u8(uint8_t* patches, int64_t patch_stride, int Np, int Ph, int Pw, const int32_t* rects,
                        const int64_t* offsets, uint8_t* packed, int64_t packed_bytes, int p0, int p1, int to_canvas,
                        void* stream);

/* ---- face masks (face_mask_static, utils/inference/masks.py:38-107) ----
 * Host, CPU only (no device pointers): for F frames of 106 float32 landmarks [F][106][2] and their
 * (erode, sigmaX, sigmaY) params [F][3] (face_mask_static's, masks.py:43-65), expand_eyebrows on the int32
 * landmarks (masks.py:5-20) and the convex hull (masks.py:31): poly [F][128][2] int32 vertices, nv[F] counts. */
int ghost_mask_polygons(const float* landmarks, int F, int npts, const int32_t* params, int32_t* poly, int32_t* nv);
/* Device: poly / nv / params as above (device copies) -> masks [F][H][W] f32 (frame f at f*mask_stride floats):
 * cv2.fillConvexPoly(255), cv2.erode / dilate with the k x k box, the 2*sigmaY border fade, cv2.GaussianBlur
 * (0, 0, sigmaX, sigmaY), / 255.  H*W <= 57344, H <= 256; ws >= ghost_face_masks_workspace_bytes(F, H, W).
 * A frame whose sigmaX or sigmaY is outside 1..42 (the blur holds 253 taps at the most) gets an all-zero mask. */
int64_t ghost_face_masks_workspace_bytes(int F, int H, int W);
int ghost_face_masks(const int32_t* poly, const int32_t* nv, const int32_t* params, int F, int H, int W, float* masks,
                     int64_t mask_stride, void* ws, int64_t ws_bytes, void* stream);
/* Device (csrc/mask_poly.hip): what ghost_mask_polygons and face_mask_static's parameter choice compute on the host,
 * in one launch for F faces and equal to them bit for bit, so that poly / nv / params for ghost_face_masks are
 * produced without a device -> host copy.  Every pointer is a device pointer.  landmarks [F][106][2] f32 (finite,
 * |v| <= 2^20).  Exactly one of two forms: params_in [F][3] given (used as they are; the four reference arguments
 * null), or params_in null and all of landmarks_ref [n_ref][106][2], ref_index [F], landmarks_tgt [n_tgt][106][2],
 * tgt_index [F] given: face f's (erode, sigmaX, sigmaY) are masks.py:43-65 of landmarks_ref[ref_index[f]] (the swap's
 * landmarks) and landmarks_tgt[tgt_index[f]] (the target crop's), in fp32 in numpy's order; an index outside its set
 * yields params 0, 0, 0.  Anything else is GHOST_EINVAL.  Writes params_out [F][3] (the chosen parameters in either
 * form), poly [F][128][2] (zero from nv[f] on) and nv [F].  F = 0 returns GHOST_OK without a launch.  The call
 * neither allocates nor synchronises. */
int ghost_mask_polygons_dev(const float* landmarks, const int32_t* params_in, const float* landmarks_ref,
                            const int32_t* ref_index, int n_ref, const float* landmarks_tgt, const int32_t* tgt_index,
                            int n_tgt, int32_t* params_out, int32_t* poly, int32_t* nv, int F, void* stream);

/* ---- plan log (test support) ----
 * While enabled, every launcher that chooses among kernel variants by shape (the conv dispatcher and everything
 * it dispatches to, the AAD launchers) appends one text signature per launch: the kernel with every template or
 * runtime parameter the host chose and the edge classes of the launch (split-K: count class, ragged last split,
 * split shorter than the ring's prologue, fix-up kind, reduction form; M / N tails; an uneven persistent grid).
 * A signature holds no batch size, row count or pointer, so every batch that selects the same plan yields the same
 * text.  Process-wide, guarded by a mutex; disabled it costs one relaxed atomic load per launch.
 * ghost_plan_log(1) clears the log and starts recording, ghost_plan_log(0) stops.  ghost_plan_log_read copies
 * the newline-separated signatures in launch order into buf (at most cap bytes, NUL-terminated) and returns the
 * bytes needed including the NUL; buf = NULL asks for the size. */
int ghost_plan_log(int enable);
int64_t ghost_plan_log_read(char* buf, int64_t cap);
/* Test support, touches no device: the signature that a ghost_aad_layers_v3_dt_nhwc launch (or the runtime's launch)
 * of this shape would append to the plan log, from the same path rule, planners and formatter as the launch.
 * L = 1 or 2 AADLayers with ldo[L]; up2x = 1: h_in read through the x2 upsample of an [H/2, W/2] source;
 * zp_mask bit l: layer l writes tap partials.  Copies the NUL-terminated text into buf (at most cap bytes;
 * buf = NULL with cap = 0 asks for the size) and returns the bytes needed including the NUL, or GHOST_EINVAL when
 * neither aad_v3 nor aad_wide takes the shape (the fused kernel or the mask pass + GEMM epilogue would). */
int64_t ghost_aad_plan(int dtype, int B, int H, int W, int C, int Ca, int L, int up2x, int zp_mask, float slope,
                       int lda, int ldh, const int ldo[], char* buf, int64_t cap);
/* Test support, touches no device: the newline-separated signatures, in launch order, that one convolution launch
 * of this descriptor would append to the plan log (the kernel's line, then a split-K reduction's), from the same
 * family rule, planners and formatters as the launch.  ti / to: GhostDType of operands and output; kind 0: Conv2d
 * kh x kw / stride / pad, 1: ConvTranspose2d 4x4/s2/p1; epi 0: standard, 1: the AADLayer epilogue (N = 2 C);
 * split_k > 0 forces the split; min_wgs as the runtime's small-batch hint (0: none); nsem: arrival counters offered
 * to the split-K fix-up (0: none; the runtime gives 4096); ncu: the device's compute units (MI355X: 256); flags: which
 * optional pointers the descriptor sets.  Every pointer counts as 16-byte aligned, ldres = ldy2 = ldy.  *ws_bytes
 * (may be NULL) receives the workspace the launch needs.  Copies the NUL-terminated text into buf (at most cap bytes;
 * buf = NULL with cap = 0 asks for the size) and returns the bytes needed including the NUL, or GHOST_EINVAL when
 * the launch would be refused. */
enum {
  GHOST_CONV_PLAN_RES = 1, GHOST_CONV_PLAN_RES_FIRST = 2, GHOST_CONV_PLAN_PRELU = 4, GHOST_CONV_PLAN_Y2 = 8,
  GHOST_CONV_PLAN_U8 = 16, GHOST_CONV_PLAN_TANH = 32, GHOST_CONV_PLAN_IN_PART = 64, GHOST_CONV_PLAN_FLAGS = 127
};
int64_t ghost_conv_plan(int ti, int to, int kind, int B, int H, int W, int Cin, int ldx, int N, int Npad, int Kpad,
                        int kh, int kw, int stride, int pad, int ldy, int epi, int split_k, int min_wgs, int nsem,
                        int ncu, int flags, int64_t* ws_bytes, char* buf, int64_t cap);
/* Test support, touches no device: the one line "in_stats t=<type> kernel=partial|partial_up|up_quad chunk=<pixels per
 * record> nchunk=<records per sample> end=self|final_kernel|fused" of the plan that a statistics pass of this shape
 * launches.  up2x = 0: an [B, H, W, C] tensor (only H * W matters); 1: the statistics of upsample2x of an [B, H, W, C]
 * source.  nsem: arrival counters offered to the fused final pass (0: none).  *ws_bytes (may be NULL) receives the
 * workspace the entries ask for.  The statistics are not in the plan log.  Returns as ghost_conv_plan does. */
int64_t ghost_instnorm_plan(int dtype, int B, int H, int W, int C, int ldx, int up2x, int nsem, int64_t* ws_bytes,
                            char* buf, int64_t cap);
/* ---- Test support: single operators as the runtimes call them.  The last-arriver reductions (the split-K fix-up in
 * the GEMM kernels, the fused final pass of the statistics) and the GEMMs whose output type differs from their
 * operand type run only when the caller gives arrival counters or a second type, which only the network runtimes do;
 * these entries take both as arguments, so that an op test can launch them alone.  sem / nsem: nsem > 0 32-bit
 * counters, zero on entry and left zero, or (NULL, 0) for none; no global state.  GHOST_EINVAL, nothing launched: a
 * bad argument, or a descriptor / type pair for which no kernel instance exists. */
/* ghost_conv2d_ex_nhwc (kind 0) or ghost_conv_transpose4x4s2_nhwc (kind 1: kh, kw, stride, pad are ignored) with the
 * operand type in_dtype, the output type out_dtype (f32 operands: any output; bf16 operands: bf16 or f32; f16
 * operands: f16) and the counters of the split-K fix-up (one per tile and phase, else the reduction kernel runs) */
int ghost_conv_rt_nhwc(int in_dtype, int out_dtype, int kind, const void* x, int B, int H, int W, int Cin, int ldx,
                       const void* w_packed, int Cout, int Npad, int Kpad, int kh, int kw, int stride, int pad,
                       const ghost_conv_epi* epi, void* y, int ldy, void* ws, int64_t ws_bytes, unsigned* sem, int nsem,
                       void* stream);
/* ghost_aad_layer_nhwc with a forced split of the GEMM's K (0: the heuristic's) and the counters, given to the
 * statistics and to the GEMM */
int ghost_aad_layer_rt_nhwc(int dtype, const void* h_in, int ldh, const void* z_attr, int lda, int B, int H, int W,
                            int C, int Ca, const void* gbw_packed, int Npad, int Kpad, const float* gbb,
                            const float* wh, const float* bh, const float* idgb, int id_ld, float slope, void* out,
                            int ldo, void* ws, int64_t ws_bytes, int split_k, unsigned* sem, int nsem, void* stream);
/* ghost_instnorm_stats_nhwc (up2x 0, HW = H * W) / ghost_instnorm_stats_up2x_nhwc (up2x 1) with the counters: one per
 * (sample, 64-channel group), else the final kernel runs */
int ghost_instnorm_stats_rt_nhwc(int dtype, const void* x, int B, int H, int W, int C, int ldx, int up2x, float* stat,
                                 void* ws, int64_t ws_bytes, unsigned* sem, int nsem, void* stream);

/* ---- SCRFD face detector (insightface scrfd_10g_bnkps) ----
 * The network, its letterbox and SCRFD.detect's post-processing for F device-resident frames of one size.  dtype:
 * GHOST_F32 (the default of the Python module), GHOST_F16 or GHOST_BF16 storage of activations and conv weights; det_w,
 * det_h: multiples of 32.  Slots: "<unit>.w" (packed as ghost_conv2d_nhwc takes it; "backbone.stem.0.w" fp32 [27][28],
 * K = (ky*3 + kx)*3 + rgb channel) and "<unit>.b" (fp32 bias, padded to 128), <unit> from ghost_amd/detection/pack.py;
 * per stride s the three output convs as one: "bbox_head.out.<s>.w" fp32 [720][30] (K = (ky*3 + kx)*80 + c; columns cls
 * 0-1, reg 2-9, kps 10-29), ".b" fp32 [32] and ".m" fp32 [32] (bbox_scale on the reg columns, 1 elsewhere).  The caller
 * computes the letterbox on the host as SCRFD.detect does: the frame is resized to (new_w, new_h) and placed top-left in
 * a zero canvas; det_scale = new_h / H. */
typedef struct ghost_det ghost_det;
int ghost_det_create(int dtype, int det_w, int det_h, ghost_det** out);
void ghost_det_destroy(ghost_det* h);
int ghost_det_bind(ghost_det* h, const char* name, const void* dev_ptr, int64_t numel);
int ghost_det_missing(ghost_det* h);
/* sized for ghost_det_detect_u8 (which covers ghost_det_forward_u8); N <= 4096 and N * det_h/2 * det_w/2 < 2^31 */
int64_t ghost_det_workspace_bytes(ghost_det* h, int N);
/* the launches of one detect call, one text line each (test support; no device needed): returns the bytes needed */
int64_t ghost_det_plan(ghost_det* h, int N, char* buf, int64_t cap);
/* frames_bgr uint8 [F,H,W,3] -> maps[9] = cls (scores, after the sigmoid) [F,Hl,Wl,2], reg [F,Hl,Wl,8] (times
 * bbox_scale), kps [F,Hl,Wl,20] for strides 8, 16, 32 in that order (cls0..2, reg0..2, kps0..2), NHWC fp32; channel
 * a*K + k belongs to anchor a.  No synchronisation; F == 0 returns GHOST_OK without a launch. */
int ghost_det_forward_u8(ghost_det* h, const uint8_t* frames_bgr, int64_t frame_stride, int F, int H, int W, int new_h,
                         int new_w, float* const* maps, void* ws, int64_t ws_bytes, void* stream);
/* SCRFD.detect per frame: det [F,max_faces,5] (x1, y1, x2, y2, score, in frame pixels), kps [F,max_faces,5,2], anchor
 * [F,max_faces] (the kept candidates' indices in the concatenated anchor order, -1 beyond), count [F,2] = (kept boxes,
 * candidates at or above thresh), all in kept order, zero beyond.  At most 4096 candidates per frame enter the sort (the
 * first 4096 in anchor order; count reports the true number) and kept boxes past max_faces are dropped (count reports
 * the true number).  Equal scores go by ascending anchor index. */
int ghost_det_detect_u8(ghost_det* h, const uint8_t* frames_bgr, int64_t frame_stride, int F, int H, int W, int new_h,
                        int new_w, float det_scale, float thresh, float nms_thresh, int max_faces, float* det,
                        float* kps, int32_t* anchor, int32_t* count, void* ws, int64_t ws_bytes, void* stream);
/* Diagnostic taps: while set (ntaps = 4), every forward copies the stored outputs of the stem after its pool
 * [N,Hd/4,Wd/4,56], stage 1 [N,Hd/4,Wd/4,56], stage 4 [N,Hd/32,Wd/32,224] and P3 [N,Hd/8,Wd/8,56] (NHWC, handle dtype)
 * into the non-NULL taps[i]. */
int ghost_det_set_taps(ghost_det* h, void* const* taps, int ntaps);
/* The detector's single operators.  letterbox: cv2.resize(frame, (new_w, new_h)) (ghost_resize_u8_linear's bytes) into
 * the top-left of a zero canvas [F,Hd,Wd,3].  stem: canvas -> (x - 127.5) / 128, R,G,B order (bgr != 0: the canvas is
 * B,G,R) -> conv 3x3 s2 p1 3 -> 28 + bias + ReLU in fp32, rounded once to dtype, [N,Hd/2,Wd/2,28].  maxpool: 3x3 s2 p1
 * (the padding never wins), H, W even, C % 4 == 0.  upsample2x_add: y [N,2h,2w,C] = round(y + nearest-x2(x)) in place.
 * head: a level's cls / reg / kps convs as one 3x3 p1 conv 80 -> 30 in fp32 from fp32 weights (the slots above): v = (acc
 * + bias[o]) * mul[o], cls = sigmoid(v); fp32 outputs whatever dtype, the storage type of x [N,H,W,80].
 * decode_nms: the post-processing of ghost_det_detect_u8 on nine given maps (cls holds scores), cap a power of two in
 * 2..4096; ws of ghost_det_decode_workspace_bytes(F, cap). */
int ghost_det_letterbox_u8(const uint8_t* frames, int64_t frame_stride, int F, int H, int W, int new_h, int new_w,
                           uint8_t* canvas, int Hd, int Wd, void* stream);
int ghost_det_stem_u8(int dtype, const uint8_t* canvas, int64_t batch_stride, int bgr, int N, int Hd, int Wd,
                      const float* w, const float* bias, void* y, void* stream);
int ghost_maxpool3x3s2_nhwc(int dtype, const void* x, int N, int H, int W, int C, void* y, void* stream);
int ghost_upsample2x_add_nhwc(int dtype, const void* x, int N, int h, int w, int C, void* y, void* stream);
int ghost_det_head_nhwc(int dtype, const void* x, int N, int H, int W, const float* w, const float* bias, const float* mul,
                        float* cls, float* reg, float* kps, void* stream);
int64_t ghost_det_decode_workspace_bytes(int F, int cap);
int ghost_det_decode_nms(const float* const* cls, const float* const* reg, const float* const* kps_maps, int F, int Hd,
                         int Wd, float thresh, float det_scale, float nms_thresh, int cap, int max_faces, float* det,
                         float* kps, int32_t* anchor, int32_t* count, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GHOST_AMD_H */
