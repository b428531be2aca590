// ghost_amd — what the four network runtimes share on the host.  One plan runs twice, as a dry run that sizes the
// workspace and as the real run that launches, over the same bump allocator: PlanCtx, the slot helpers, the storage
// type check and the sticky error serve all four.  arc_runtime.hip, lmk_runtime.hip and det_runtime.hip also share
// the handle base, the context that reads it (HandleCtx), the dry-run sizing (size_plan) and the bracket of a forward
// call (run_plan).  aei_runtime.hip keeps its own handle and bracket: two scratch regions, the arrival counters, the
// device guard and the profiler would make the shared ones branch on their caller.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

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

// bytes per element of a storage type, 0 for anything else (f16 only where the runtime has fp16 kernels)
inline int storage_esz(int dtype, bool f16_ok = true) {
  if (dtype == GHOST_F32) return 4;
  return dtype == GHOST_BF16 || (f16_ok && dtype == GHOST_F16) ? 2 : 0;
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

// ---- the handle, context, sizing and run bracket of arc_runtime.hip, lmk_runtime.hip and det_runtime.hip ----

// A runtime's handle derives from Handle and says what its C ABI demands: kTaps, the number of tap pointers set_taps
// takes (0: any number), and kAligned16, whether bind asks for 16-byte aligned tensors.
struct Handle {
  int dt = GHOST_F32, esz = 4;
  Slots slots;
  std::vector<void*> taps;  // diagnostic taps: a live plan copies stored activations into the non-null ones
  void set_storage(int dtype) { dt = dtype; esz = storage_esz(dtype); }
};

// ghost_*_bind, ghost_*_missing and ghost_*_set_taps; h may be null
template <class H>
int handle_bind(H* h, const char* name, const void* p, int64_t numel) {
  return bind_slot(h ? &h->slots : nullptr, name, p, numel, "empty tensor for ", H::kAligned16);
}
inline int handle_missing(const Handle* h) {
  return h ? count_missing(h->slots) : set_last_error(GHOST_EINVAL, "null handle");
}
template <class H>
int handle_set_taps(H* h, void* const* taps, int ntaps) {
  if (!h || ntaps < 0 || (ntaps && !taps) || (H::kTaps && ntaps && ntaps != H::kTaps))
    return set_last_error(GHOST_EINVAL, H::kTaps ? "bad argument (0 or " + std::to_string(H::kTaps) + " taps)"
                                                 : std::string("bad argument"));
  h->taps.assign(taps, taps + ntaps);
  return 0;
}

// the first checks of a forward call; lo is 0 where an empty batch is a no-op
inline int check_batch(const Handle* h, int N, int lo, int hi) {
  if (!h) return set_last_error(GHOST_EINVAL, "null handle");
  if (N < lo || N > hi)
    return set_last_error(GHOST_EINVAL, "batch must be in " + std::to_string(lo) + ".." + std::to_string(hi));
  return 0;
}

template <class H>
struct HandleCtx : PlanCtx {
  H* h = nullptr;
  const void* W(const std::string& name) { return PlanCtx::W(h->slots, name); }
  const float* F(const std::string& name) { return (const float*)W(name); }
  void tap(size_t i, const void* src, size_t bytes) {
    if (dry || !ok() || i >= h->taps.size() || !h->taps[i]) return;
    check((int)hipMemcpyAsync(h->taps[i], src, bytes, hipMemcpyDeviceToDevice, s), "tap copy");
  }
};

// what a dry run yields: the plan's regions end at plan_end, the scratch follows, 256 bytes allow for aligning ws
struct PlanSize {
  int rc = 0;               // the dry run's failure (where says which step); need() is this code then
  std::string where;
  size_t plan_end = 0, scratch = 0;
  int64_t need() const { return rc ? rc : (int64_t)(plan_end + scratch + 256); }
};

// runs plan(Ctx&) dry; it makes the same allocations, in the same order, as the body given to run_plan
template <class Ctx, class H, class Plan>
PlanSize size_plan(H* h, Plan&& plan) {
  Ctx c{};
  c.h = h; c.dry = true;
  plan(c);
  return PlanSize{c.rc, c.where, align_up(c.off), c.scratch_need};
}

// The live half of a forward call: the workspace check, the live context, body(Ctx&) -> int, which issues the front
// kernels and the plan (a non-zero return is passed on as it is: the body has set the last error), and the failure
// text "<name> failed at <where>[: hip error]".
template <class Ctx, class H, class Body>
int run_plan(H* h, const PlanSize& z, void* ws, int64_t ws_bytes, void* stream, const char* name, Body&& body) {
  if (z.rc) return set_last_error(z.rc, "plan sizing failed");
  if (!ws || ws_bytes < z.need())
    return set_last_error(GHOST_ENOWS, "workspace too small: need " + std::to_string(z.need()));
  Ctx c{};
  c.h = h; c.dry = false;
  c.base = align_up(ws);
  c.s = (hipStream_t)stream;
  c.scratch = c.base + z.plan_end;
  c.scratch_cap = z.scratch;
  if (const int rc = body(c)) return rc;
  if (!c.ok())
    return set_last_error(c.rc, std::string(name) + " failed at " + c.where +
                                    (c.rc > 0 ? std::string(": ") + hipGetErrorString((hipError_t)c.rc) : ""));
  return 0;
}

}  // namespace ghost
