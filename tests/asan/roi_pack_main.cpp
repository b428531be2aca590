// Sanitizer run of the packed ROI transfer's host code (ghost_roi_packed_layout, ghost_roi_pack_host and the argument
// checks of ghost_roi_unpack_u8).  Built by tools/asan_roi_pack.sh from this file and ghost_amd/csrc/roi_pack.hip
// alone (ghost::set_last_error is defined here), once with -fsanitize=address,undefined and once with
// -fsanitize=thread on the host pass, and run on the CPU: no kernel is launched.  It exercises the layout, pack and
// unpack of hand-made and of large rectangles with 1, 4 and 16 threads, patch ranges, and every refusal.
// Exit status 0, "0 failed checks" and no sanitizer report = clean.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ghost_amd.h"

static std::string g_error;
namespace ghost {
int set_last_error(int rc, const char* msg) {
  g_error = msg ? msg : "";
  return rc;
}
}  // namespace ghost

static int fails = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                          \
    }                                                                   \
  } while (0)

namespace {

constexpr uint8_t kFill = 0xEE;

struct Case {
  int H, W, F;
  std::vector<int32_t> rects;      // [Np][4]
  std::vector<int> frame_of;
  std::vector<std::vector<uint8_t>> frames;
  std::vector<int64_t> offsets;
  int64_t total = 0;
  int Np() const { return (int)frame_of.size(); }
  std::vector<uint8_t*> ptrs(std::vector<std::vector<uint8_t>>& fr) const {
    std::vector<uint8_t*> p;
    for (int f : frame_of) p.push_back(fr[(size_t)f].data());
    return p;
  }
};

int64_t pitch(int64_t w) { return (3 * w + 15) & ~(int64_t)15; }

void fill_frames(Case& c, unsigned seed) {
  std::mt19937 g(seed);
  c.frames.assign((size_t)c.F, std::vector<uint8_t>((size_t)c.H * c.W * 3));
  for (auto& f : c.frames)
    for (auto& b : f) b = (uint8_t)(g() % kFill);
}

void layout(Case& c) {
  c.offsets.assign((size_t)c.Np(), -1);
  CHECK(ghost_roi_packed_layout(c.rects.data(), c.Np(), c.offsets.data(), &c.total) == GHOST_OK);
  int64_t off = 0;
  for (int p = 0; p < c.Np(); ++p) {
    const int64_t w = c.rects[(size_t)p * 4 + 2], h = c.rects[(size_t)p * 4 + 3];
    CHECK(c.offsets[(size_t)p] == off && off % 256 == 0);
    off = (off + (w > 0 && h > 0 ? pitch(w) * h : 0) + 255) & ~(int64_t)255;
  }
  CHECK(c.total == off);
}

std::vector<uint8_t> expected(const Case& c) {
  std::vector<uint8_t> e((size_t)c.total, kFill);
  for (int p = 0; p < c.Np(); ++p) {
    const int32_t* r = &c.rects[(size_t)p * 4];
    for (int y = 0; y < r[3] && r[2] > 0; ++y)
      std::memcpy(&e[(size_t)(c.offsets[(size_t)p] + y * pitch(r[2]))],
                  &c.frames[(size_t)c.frame_of[(size_t)p]][((size_t)(r[1] + y) * c.W + r[0]) * 3], (size_t)r[2] * 3);
  }
  return e;
}

int pack(const Case& c, std::vector<uint8_t>& staging, std::vector<uint8_t*>& ptrs, int p0, int p1, int to_staging,
         int threads) {
  return ghost_roi_pack_host(staging.data(), (int64_t)staging.size(), c.rects.data(), c.offsets.data(), ptrs.data(),
                             c.Np(), p0, p1, c.H, c.W, to_staging, threads);
}

void round_trip(Case& c) {
  layout(c);
  const std::vector<uint8_t> want = expected(c);
  for (int threads : {1, 4, 16, 0}) {
    std::vector<uint8_t> staging((size_t)c.total, kFill);
    auto src = c.ptrs(c.frames);
    CHECK(pack(c, staging, src, 0, c.Np(), 1, threads) == GHOST_OK);
    CHECK(staging == want);
    // in two ranges, at every boundary
    for (int cut = 0; cut <= c.Np(); cut += (c.Np() > 40 ? 7 : 1)) {
      std::vector<uint8_t> s2((size_t)c.total, kFill);
      CHECK(pack(c, s2, src, 0, cut, 1, threads) == GHOST_OK);
      CHECK(pack(c, s2, src, cut, c.Np(), 1, threads) == GHOST_OK);
      CHECK(s2 == want);
    }
    // back into blank frames: the rectangles arrive, every other byte stays
    std::vector<std::vector<uint8_t>> back((size_t)c.F, std::vector<uint8_t>((size_t)c.H * c.W * 3, 0xFF));
    std::vector<std::vector<uint8_t>> ref = back;
    for (int p = 0; p < c.Np(); ++p) {
      const int32_t* r = &c.rects[(size_t)p * 4];
      const size_t f = (size_t)c.frame_of[(size_t)p];
      for (int y = 0; y < r[3] && r[2] > 0; ++y) {
        const size_t at = ((size_t)(r[1] + y) * c.W + r[0]) * 3;
        std::memcpy(&ref[f][at], &c.frames[f][at], (size_t)r[2] * 3);
      }
    }
    auto dst = c.ptrs(back);
    CHECK(pack(c, staging, dst, 0, c.Np(), 0, threads) == GHOST_OK);
    CHECK(back == ref);
    CHECK(staging == want);
  }
}

void refusals(Case& c) {
  const int n = c.Np(), last = n - 1;
  std::vector<uint8_t> staging((size_t)c.total, kFill);
  const std::vector<uint8_t> blank = staging;
  const auto frames0 = c.frames;
  auto refused = [&](const Case& bad, std::vector<uint8_t*> ptrs, int64_t bytes, const char* msg) {
    for (int to_staging = 0; to_staging <= 1; ++to_staging) {
      const int rc = ghost_roi_pack_host(staging.data(), bytes, bad.rects.data(), bad.offsets.data(), ptrs.data(), n, 0,
                                         n, bad.H, bad.W, to_staging, 4);
      CHECK(rc == GHOST_EINVAL);
      CHECK(g_error.find(msg) != std::string::npos);
      CHECK(staging == blank);
      CHECK(c.frames == frames0);
    }
  };
  auto ptrs = c.ptrs(c.frames);
  const int32_t bad_rects[5][4] = {{c.W - 3, 0, 4, 4}, {0, c.H - 3, 4, 4}, {-1, 0, 4, 4}, {0, 0, 4, -3}, {0, 0, -4, 3}};
  for (const auto& r : bad_rects) {
    Case b = c;
    std::memcpy(&b.rects[(size_t)last * 4], r, sizeof r);
    refused(b, ptrs, c.total, "leaves the frame");
  }
  {
    Case b = c;
    b.offsets[(size_t)last] += 8;                       // unaligned
    refused(b, ptrs, c.total, "offset");
    b = c;
    b.offsets[(size_t)last] = -256;                     // negative
    refused(b, ptrs, c.total, "offset");
    b = c;
    b.offsets[1] = b.offsets[0] + 16;                   // patch 0 runs into patch 1
    refused(b, ptrs, c.total, "overlap or descend");
    b = c;
    std::swap(b.offsets[1], b.offsets[2]);              // descending
    refused(b, ptrs, c.total, "overlap or descend");
  }
  const int32_t* r = &c.rects[(size_t)last * 4];
  const int64_t end = c.offsets[(size_t)last] + pitch(r[2]) * r[3];
  refused(c, ptrs, end - 1, "staging buffer");          // one byte short
  {
    auto p2 = ptrs;
    p2[(size_t)last] = nullptr;
    refused(c, p2, c.total, "null");
  }
  CHECK(ghost_roi_pack_host(nullptr, 0, nullptr, nullptr, nullptr, n, 0, n, c.H, c.W, 1, 0) == GHOST_EINVAL);
  CHECK(ghost_roi_pack_host(staging.data(), c.total, c.rects.data(), c.offsets.data(), ptrs.data(), n, 2, 1, c.H, c.W,
                            1, 0) == GHOST_EINVAL);
  CHECK(ghost_roi_pack_host(staging.data(), c.total, c.rects.data(), c.offsets.data(), ptrs.data(), n, 0, n + 1, c.H,
                            c.W, 1, 0) == GHOST_EINVAL);
  CHECK(ghost_roi_pack_host(staging.data(), c.total, c.rects.data(), c.offsets.data(), ptrs.data(), n, 3, 3, c.H, c.W,
                            1, 0) == GHOST_OK);
  // the exact size is accepted
  CHECK(ghost_roi_pack_host(staging.data(), end, c.rects.data(), c.offsets.data(), ptrs.data(), n, 0, n, c.H, c.W, 1,
                            4) == GHOST_OK);
  // layout
  int64_t total = -7;
  std::vector<int64_t> offs(2, -7);
  const int32_t neg[8] = {0, 0, 4, 4, 0, 0, -1, 4};
  CHECK(ghost_roi_packed_layout(neg, 2, offs.data(), &total) == GHOST_EINVAL && total == -7 && offs[0] == -7);
  CHECK(ghost_roi_packed_layout(nullptr, 0, nullptr, &total) == GHOST_OK && total == 0);
  CHECK(ghost_roi_packed_layout(neg, 2, offs.data(), nullptr) == GHOST_EINVAL);
  // the device entry refuses on the host, before any launch
  uint8_t dummy[16];
  int32_t drect[4] = {0, 0, 1, 1};
  int64_t doff[1] = {0};
  CHECK(ghost_roi_unpack_u8(nullptr, 48, 1, 4, 4, drect, doff, dummy, 16, 0, 1, 1, nullptr) == GHOST_EINVAL);
  CHECK(ghost_roi_unpack_u8(dummy, 48, 1, 4, 4, drect, doff, nullptr, 16, 0, 1, 1, nullptr) == GHOST_EINVAL);
  CHECK(ghost_roi_unpack_u8(dummy, 47, 1, 4, 4, drect, doff, dummy, 16, 0, 1, 1, nullptr) == GHOST_EINVAL);
  CHECK(ghost_roi_unpack_u8(dummy, 48, 70000, 4, 4, drect, doff, dummy, 16, 0, 65536, 1, nullptr) == GHOST_EINVAL);
  CHECK(ghost_roi_unpack_u8(dummy, 48, 1, 4, 4, drect, doff, dummy, 16, 1, 1, 1, nullptr) == GHOST_OK);
}

}  // namespace

int main() {
  // hand-made: 3 frames of 96 x 128, narrow and wide rows, edges touching the frame, an empty rectangle in the middle
  Case small;
  small.H = 96, small.W = 128, small.F = 3;
  const int hand[][5] = {{0, 0, 128, 96, 0}, {0, 0, 1, 1, 1}, {3, 0, 2, 2, 1}, {8, 1, 3, 5, 1}, {13, 0, 4, 1, 1},
                         {20, 3, 5, 2, 1}, {27, 0, 6, 5, 1}, {0, 0, 1, 96, 2}, {10, 10, 0, 7, 1}, {36, 2, 7, 1, 1},
                         {45, 0, 16, 2, 1}, {63, 1, 21, 5, 1}, {85, 0, 43, 5, 1}, {121, 0, 7, 96, 2}, {4, 4, 5, 0, 2},
                         {0, 91, 43, 5, 1}, {16, 94, 16, 2, 2}};
  for (const auto& h : hand) {
    small.rects.insert(small.rects.end(), h, h + 4);
    small.frame_of.push_back(h[4]);
  }
  fill_frames(small, 1);
  round_trip(small);
  refusals(small);

  // large: 24 faces of about 300 x 300, each in its own 360 x 480 frame, so that the workers really split the rows
  Case big;
  big.H = 360, big.W = 480, big.F = 24;
  std::mt19937 g(2);
  for (int p = 0; p < 24; ++p) {
    const int w = 250 + (int)(g() % 90), h = 250 + (int)(g() % 90);
    const int32_t r[4] = {(int32_t)(g() % (unsigned)(big.W - w + 1)), (int32_t)(g() % (unsigned)(big.H - h + 1)), w, h};
    big.rects.insert(big.rects.end(), r, r + 4);
    big.frame_of.push_back(p);
  }
  fill_frames(big, 3);
  round_trip(big);
  refusals(big);

  std::printf("%d failed checks\n", fails);
  return fails ? 1 : 0;
}
