// ghost_amd — plan log (test support): while enabled, every launcher that chooses among kernel variants by
// shape appends one text signature per launch, written at the branch that launches.  A signature names the
// kernel with every template / runtime parameter the host chose plus the edge classes of the launch (split-K
// shape, M / N tails, uneven persistent grid); it never holds the batch, M or a pointer, so batch sizes that
// select the same plan produce the same text (tests/test_batch_sweep.py, tools/plan_sweep.py).
// Disabled, a launch pays one relaxed atomic load.
#pragma once
#include <atomic>

namespace ghost {

extern std::atomic<int> g_plan_log_on;
void plan_log_append(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

// one signature, formatted by a launcher's own function (only while the log is on, or for ghost_aad_plan)
struct PlanSig { char s[160]; };

// "bf16" / "f16" / "f32" of a GhostDType
inline const char* plan_dt(int dt) { return dt == 1 ? "bf16" : dt == 2 ? "f16" : dt == 0 ? "f32" : "u8"; }

}  // namespace ghost

#define GHOST_PLAN_LOG(...)                                                                      \
  do {                                                                                           \
    if (ghost::g_plan_log_on.load(std::memory_order_relaxed)) ghost::plan_log_append(__VA_ARGS__); \
  } while (0)
