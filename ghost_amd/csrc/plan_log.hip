// ghost_amd — plan log storage and its C ABI (include/ghost_amd.h: ghost_plan_log, ghost_plan_log_read).
#include "plan_log.h"

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>

#include "ghost_amd.h"

namespace ghost {

std::atomic<int> g_plan_log_on{0};

namespace {
std::mutex g_plan_mu;
std::string g_plan_text;
}  // namespace

void plan_log_append(const char* fmt, ...) {
  char line[512];
  va_list ap;
  va_start(ap, fmt);
  int n = vsnprintf(line, sizeof(line), fmt, ap);
  va_end(ap);
  if (n < 0) return;
  if (n >= (int)sizeof(line)) n = (int)sizeof(line) - 1;
  std::lock_guard<std::mutex> lk(g_plan_mu);
  if (!g_plan_log_on.load(std::memory_order_relaxed)) return;   // stopped while this launch formatted its line
  g_plan_text.append(line, (size_t)n);
  g_plan_text.push_back('\n');
}

}  // namespace ghost

extern "C" int ghost_plan_log(int enable) {
  std::lock_guard<std::mutex> lk(ghost::g_plan_mu);
  if (enable) ghost::g_plan_text.clear();
  ghost::g_plan_log_on.store(enable ? 1 : 0, std::memory_order_relaxed);
  return 0;
}

extern "C" int64_t ghost_plan_log_read(char* buf, int64_t cap) {
  std::lock_guard<std::mutex> lk(ghost::g_plan_mu);
  const int64_t need = (int64_t)ghost::g_plan_text.size() + 1;   // with the terminating NUL
  if (buf && cap > 0) {
    const int64_t n = need - 1 < cap - 1 ? need - 1 : cap - 1;
    memcpy(buf, ghost::g_plan_text.data(), (size_t)n);
    buf[n] = '\0';
  }
  return need;
}
