// ghost_amd — what the runtimes (aei_runtime.hip, arc_runtime.hip) share on the host: one plan runs twice, as a
// dry run that sizes the workspace and as the real run that launches, over the same bump allocator.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <string>

#include "../../include/ghost_amd.h"
#include "conv_igemm.h"

namespace ghost {

// one ghost_last_error() per thread for the whole library (defined in aei_runtime.hip); rc == 0 reads GHOST_EINVAL
int set_last_error(int rc, const std::string& msg);
int set_last_error(int rc, const char* msg);

inline int rup(int v, int m) { return (v + m - 1) / m * m; }
// every workspace region starts on a 256-byte boundary
inline size_t align_up(size_t v) { return (v + 255) & ~size_t(255); }
inline char* align_up(void* p) { return (char*)align_up((size_t)(uintptr_t)p); }

// a square image and k x k taps with the padding the host packs weights to (pack.py): N to 128, K to 32
inline ConvDesc conv_desc(int ti, int to, const void* x, int B, int H, int Cin, int ldx, const void* w, int N, int kind,
                          int k, int stride, int pad, void* y, int ldy) {
  const int taps = kind == CONV_T4S2 ? 4 : k * k;
  return conv_desc(ti, to, x, B, H, H, Cin, ldx, w, N, rup(N, 128), rup(taps * Cin, 32), kind, k, k, stride, pad, y, ldy);
}

typedef std::map<std::string, const void*> Slots;   // name -> device pointer (nullptr = unbound)

struct PlanCtx {
  bool dry = false;
  char* base = nullptr;
  size_t off = 0;
  size_t scratch_need = 0;  // max split-K / IN-stats partial bytes (dry run)
  char* scratch = nullptr;
  size_t scratch_cap = 0;
  hipStream_t s = nullptr;
  int rc = 0;               // the first failure sticks; every later step is skipped
  std::string where;

  void* alloc(size_t bytes) {
    off = align_up(off);
    void* p = dry ? reinterpret_cast<void*>(uintptr_t(0x10000000) + off) : base + off;
    off += bytes;
    return p;
  }
  bool ok() const { return rc == 0; }
  template <class S>
  void check(int r, const S& what) {
    if (r != 0 && rc == 0) {
      rc = r;
      where = what;
    }
  }
  void need_scratch(size_t bytes) {
    if (bytes > scratch_need) scratch_need = bytes;
  }
  const void* W(const Slots& slots, const std::string& name) {
    auto it = slots.find(name);
    if (dry) {  // sizing needs no weights, but every slot the plan reads must be declared
      if (it == slots.end()) check(GHOST_EINVAL, "plan reads undeclared slot " + name);
      return reinterpret_cast<const void*>(uintptr_t(0x1000));
    }
    if (it == slots.end() || !it->second) {
      check(GHOST_ENOTREADY, "unbound weight slot " + name);
      return nullptr;
    }
    return it->second;
  }
};

// ghost_*_bind: `empty` is the runtime's text for a null / empty tensor, `aligned16` whether it asks for alignment
inline int bind_slot(Slots* slots, const char* name, const void* p, int64_t numel, const char* empty, bool aligned16) {
  if (!slots || !name) return set_last_error(GHOST_EINVAL, "null argument");
  auto it = slots->find(name);
  if (it == slots->end()) return set_last_error(GHOST_EINVAL, std::string("unknown weight slot ") + name);
  if (!p || numel <= 0) return set_last_error(GHOST_EINVAL, std::string(empty) + name);
  if (aligned16 && (uintptr_t)p % 16) return set_last_error(GHOST_EINVAL, std::string("slot not 16-byte aligned: ") + name);
  it->second = p;
  return 0;
}

// the number of unbound slots; the last error names the first of them
inline int count_missing(const Slots& slots) {
  int n = 0;
  for (auto& kv : slots)
    if (!kv.second && !n++) set_last_error(GHOST_ENOTREADY, "unbound weight slot " + kv.first);
  return n;
}

}  // namespace ghost
