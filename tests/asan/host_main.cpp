// Host-side sanitizer run of the native library's CPU code (sanitizers on host code only — GPU
// AddressSanitizer is not available on this pool).  Built by tools/asan_host.sh with -fsanitize=address,undefined
// on the host pass of every ghost_amd/csrc/*.hip (-Xarch_host), linked into this executable and run on the CPU:
// no kernel is launched.  It exercises
//   * ghost_aei_create / ghost_aei_destroy for every backbone, num_blocks and dtype,
//   * the native plan's dry run and its bump allocator (ghost_aei_workspace_bytes, _swap_workspace_bytes,
//     identity-table sizing) at batch sizes 1 .. 128, including the two-stream plan's second scratch region,
//   * argument validation paths (ghost_last_error strings),
//   * ghost_mask_polygons (eyebrow expansion + convex hull, masks.hip) on random and degenerate landmark sets,
//   * the handle base and the run bracket the ArcFace, landmark and detector runtimes share (plan_ctx.h): create,
//     bind, set_taps, the dry-run sizing, ghost_det_plan and every forward entry point up to the workspace check.
// Exit status 0 and no sanitizer report = clean.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ghost_amd.h"

static int fails = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                          \
    }                                                                   \
  } while (0)

// One handle of the arc / lmk / det runtimes through everything that needs no device.  The slot names come from
// asking which slot is unbound; the addresses bound are never read.
template <class H>
struct Rt {
  H* h;
  int (*bind)(H*, const char*, const void*, int64_t);
  int (*missing)(H*);
  int64_t (*bytes)(H*, int);
  int (*set_taps)(H*, void* const*, int);
  void (*destroy)(H*);
  int max_batch;
  bool any_taps, empty_ok;   // arc: any number of taps, no empty batch, and sizing has no upper batch limit
};

static char g_dummy[64] __attribute__((aligned(16)));

template <class H, class Fwd>
static int64_t walk(const Rt<H>& r, Fwd&& forward) {
  static const char kUnbound[] = "unbound weight slot ";
  int64_t sized = 0;
  H* h = r.h;
  CHECK(r.missing(h) > 0);
  CHECK(forward(h, 2) == GHOST_ENOTREADY && std::strncmp(ghost_last_error(), kUnbound, sizeof kUnbound - 1) == 0);
  CHECK(r.bind(h, "no.such.slot", g_dummy, 1) == GHOST_EINVAL);
  CHECK(r.bind(nullptr, "stem.w", g_dummy, 1) == GHOST_EINVAL && r.missing(nullptr) == GHOST_EINVAL);
  for (int pass = 0; pass < 2; ++pass) {      // sizes with nothing bound, then with everything bound
    for (int N : {0, 1, 2, 3, 8, 33}) {
      const int64_t b = r.bytes(h, N);
      CHECK(N == 0 ? b == (r.empty_ok ? 256 : GHOST_EINVAL) : b > 256);
      CHECK(r.bytes(h, N) == b);
      ++sized;
    }
    CHECK((r.bytes(h, r.max_batch + 1) < 0) == r.empty_ok && r.bytes(nullptr, 1) < 0);
    if (pass) break;
    int left = r.missing(h);
    while (left > 0) {
      const std::string name = ghost_last_error() + (sizeof kUnbound - 1);
      CHECK(r.bind(h, name.c_str(), nullptr, 1) == GHOST_EINVAL && r.bind(h, name.c_str(), g_dummy, 0) == GHOST_EINVAL);
      CHECK(r.bind(h, name.c_str(), g_dummy, 1) == 0);
      const int now = r.missing(h);
      CHECK(now == left - 1);
      if (now != left - 1) break;
      left = now;
    }
  }
  void* taps[4] = {g_dummy, nullptr, g_dummy, g_dummy};
  CHECK(r.set_taps(h, taps, 4) == 0 && r.set_taps(h, nullptr, 0) == 0);
  CHECK(r.set_taps(h, taps, 3) == (r.any_taps ? 0 : GHOST_EINVAL));
  CHECK(r.set_taps(h, nullptr, 4) == GHOST_EINVAL && r.set_taps(h, taps, -1) == GHOST_EINVAL);
  CHECK(r.set_taps(nullptr, taps, 4) == GHOST_EINVAL && r.set_taps(h, nullptr, 0) == 0);
  CHECK(forward(h, 3) == GHOST_ENOWS && std::strstr(ghost_last_error(), "workspace too small: need "));
  CHECK(forward(h, 0) == (r.empty_ok ? GHOST_OK : GHOST_EINVAL));
  CHECK(forward(h, r.max_batch + 1) == GHOST_EINVAL && forward(h, -1) == GHOST_EINVAL);
  CHECK(forward(nullptr, 3) == GHOST_EINVAL);
  r.destroy(h);
  return sized;
}

static int64_t shared_runtimes() {
  int64_t sized = 0;
  void* const p = g_dummy;
  const uint8_t* const u8 = (const uint8_t*)g_dummy;
  float* const f = (float*)g_dummy;
  const int arc_layers[2][4] = {{3, 13, 30, 3}, {1, 1, 1, 1}};
  for (int dt : {GHOST_DTYPE_F32, GHOST_DTYPE_BF16})
    for (const int* layers : arc_layers) {
      ghost_arc* h = nullptr;
      CHECK(ghost_arc_create(layers, 512, dt, &h) == 0 && h);
      if (!h) continue;
      const Rt<ghost_arc> r{h, ghost_arc_bind, ghost_arc_missing, ghost_arc_workspace_bytes, ghost_arc_set_taps,
                            ghost_arc_destroy, 65535, true, false};
      const int64_t st[4] = {3 * 112 * 112, 112 * 112, 112, 1};
      sized += walk(r, [&](ghost_arc* a, int N) {
        const int rc = ghost_arc_forward(a, p, GHOST_DTYPE_F32, st, N, f, nullptr, 0, nullptr);
        CHECK(ghost_arc_embed_u8(a, u8, 224 * 224 * 3, N, 224, 224, f, nullptr, 0, nullptr) == rc);
        return rc;
      });
    }
  for (int dt : {GHOST_DTYPE_F32, GHOST_DTYPE_BF16, GHOST_DTYPE_F16}) {
    ghost_lmk* h = nullptr;
    CHECK(ghost_lmk_create(dt, &h) == 0 && h);
    if (!h) continue;
    const Rt<ghost_lmk> r{h, ghost_lmk_bind, ghost_lmk_missing, ghost_lmk_workspace_bytes, ghost_lmk_set_taps,
                          ghost_lmk_destroy, 65535, false, true};
    sized += walk(r, [&](ghost_lmk* a, int N) {
      const int rc = ghost_lmk_forward(a, u8, 192 * 192 * 3, 1, N, f, nullptr, 0, nullptr);
      CHECK(ghost_lmk_landmarks_u8(a, u8, 224 * 224 * 3, N, f, f, nullptr, 0, nullptr) == rc);
      return rc;
    });
  }
  const int det_sizes[2][2] = {{96, 64}, {640, 640}};
  for (int dt : {GHOST_DTYPE_F32, GHOST_DTYPE_BF16, GHOST_DTYPE_F16})
    for (const int* wh : det_sizes) {
      ghost_det* h = nullptr;
      CHECK(ghost_det_create(dt, wh[0], wh[1], &h) == 0 && h);
      if (!h) continue;
      char small[16];
      const int64_t need = ghost_det_plan(h, 3, nullptr, 0);
      CHECK(need > 16 && ghost_det_plan(h, 3, small, sizeof small) == need && std::strlen(small) == sizeof small - 1);
      std::vector<char> text((size_t)need);
      CHECK(ghost_det_plan(h, 3, text.data(), need) == need && (int64_t)std::strlen(text.data()) == need - 1);
      CHECK(ghost_det_plan(h, 0, nullptr, 0) < 0 && ghost_det_plan(h, 3, nullptr, 8) < 0);
      const Rt<ghost_det> r{h, ghost_det_bind, ghost_det_missing, ghost_det_workspace_bytes, ghost_det_set_taps,
                            ghost_det_destroy, 4096, false, true};
      float* maps[9];
      for (float*& m : maps) m = f;
      sized += walk(r, [&](ghost_det* a, int N) {
        const int rc = ghost_det_forward_u8(a, u8, 45 * 80 * 3, N, 45, 80, 36, 64, maps, nullptr, 0, nullptr);
        CHECK(ghost_det_detect_u8(a, u8, 45 * 80 * 3, N, 45, 80, 36, 64, 0.8f, 0.5f, 0.4f, 16, f, f, (int32_t*)p,
                                  (int32_t*)p, nullptr, 0, nullptr) == rc);
        return rc;
      });
    }
  ghost_arc* a = nullptr;
  ghost_lmk* l = nullptr;
  ghost_det* d = nullptr;
  CHECK(ghost_arc_create(arc_layers[0], 512, GHOST_DTYPE_F16, &a) != 0 && !a);      // arc has no fp16 path
  CHECK(ghost_arc_create(arc_layers[0], 500, GHOST_DTYPE_F32, &a) != 0 && ghost_arc_create(nullptr, 512, 0, &a) != 0);
  CHECK(ghost_lmk_create(GHOST_DTYPE_U8, &l) != 0 && !l && ghost_lmk_create(GHOST_DTYPE_F32, nullptr) != 0);
  CHECK(ghost_det_create(GHOST_DTYPE_U8, 96, 64, &d) != 0 && ghost_det_create(GHOST_DTYPE_F32, 100, 64, &d) != 0 && !d);
  return sized;
}

int main() {
  const char* bbs[3] = {"unet", "linknet", "resnet"};
  const int dts[3] = {GHOST_DTYPE_F32, GHOST_DTYPE_BF16, GHOST_DTYPE_F16};
  int64_t checked = 0;
  for (const char* bb : bbs)
    for (int nb = 1; nb <= 3; ++nb)
      for (int dt : dts) {
        ghost_aei* h = nullptr;
        CHECK(ghost_aei_create(bb, nb, 512, dt, &h) == 0 && h);
        if (!h) continue;
        CHECK(ghost_aei_missing(h) > 0);   // nothing bound
        for (int k = 1; k <= 8; ++k) {
          int C = 0, H = 0, W = 0;
          CHECK(ghost_aei_attr_geometry(h, k, &C, &H, &W) == 0 && C > 0 && H == (1 << k) && W == H);
        }
        for (int B : {1, 2, 3, 7, 8, 9, 16, 33, 64, 128}) {
          for (int two = 0; two <= 1; ++two) {
            CHECK(ghost_aei_set_option(h, GHOST_AEI_OPT_TWO_STREAMS, two) == 0);
            const int64_t f = ghost_aei_workspace_bytes(h, B), s = ghost_aei_swap_workspace_bytes(h, B);
            CHECK(f > 0 && s > 0);
            checked += 2;
          }
          for (int fr = 0; fr <= 1; ++fr) {
            CHECK(ghost_aei_set_option(h, GHOST_AEI_OPT_FUSE_REDUCE, fr) == 0);
            CHECK(ghost_aei_swap_workspace_bytes(h, B) > 0);
          }
          CHECK(ghost_aei_identity_table_bytes(h, B) > 0);
          CHECK(ghost_aei_identity_table_workspace_bytes(h, B) > 0);
          checked += 3;
        }
        int v = -1;
        CHECK(ghost_aei_get_option(h, GHOST_AEI_OPT_TAP_PARTIALS, &v) == 0 && v >= 0);
        CHECK(ghost_aei_set_option(h, 99, 1) != 0 && std::strlen(ghost_last_error()) > 0);
        CHECK(ghost_aei_workspace_bytes(h, 0) < 0);
        CHECK(ghost_aei_bind(h, "no.such.slot", nullptr, 1) != 0);
        ghost_aei_destroy(h);
      }
  ghost_aei* bad = nullptr;
  CHECK(ghost_aei_create("vgg", 2, 512, GHOST_DTYPE_BF16, &bad) != 0 && bad == nullptr);
  CHECK(ghost_aei_create("unet", 0, 512, GHOST_DTYPE_BF16, &bad) != 0);
  CHECK(ghost_aei_create("unet", 2, 500, GHOST_DTYPE_BF16, &bad) != 0);

  // face-mask polygons: random landmark clouds, a collinear set, all points equal
  std::mt19937 rng(7);
  std::uniform_real_distribution<float> U(0.f, 224.f);
  const int F = 64;
  std::vector<float> lm(F * 106 * 2);
  for (auto& x : lm) x = U(rng);
  for (int i = 0; i < 106; ++i) { lm[(1 * 106 + i) * 2] = 10.f + i; lm[(1 * 106 + i) * 2 + 1] = 20.f + i; }
  for (int i = 0; i < 106 * 2; ++i) lm[2 * 106 * 2 + i] = 100.f;
  std::vector<int32_t> params(F * 3);
  for (int f = 0; f < F; ++f) { params[f * 3] = (f % 3 == 0) ? 15 : (f % 3 == 1 ? -5 : 10); params[f * 3 + 1] = 7; params[f * 3 + 2] = 5; }
  std::vector<int32_t> poly(F * 128 * 2, -1), nv(F, -1);
  CHECK(ghost_mask_polygons(lm.data(), F, 106, params.data(), poly.data(), nv.data()) == 0);
  for (int f = 0; f < F; ++f) CHECK(nv[f] >= 1 && nv[f] <= 128);
  CHECK(ghost_mask_polygons(lm.data(), F, 68, params.data(), poly.data(), nv.data()) != 0);
  CHECK(ghost_face_masks_workspace_bytes(F, 224, 224) > 0);

  checked += shared_runtimes();

  std::printf("asan host run: %lld plan sizings, %d failed checks\n", (long long)checked, fails);
  return fails ? 1 : 0;
}
