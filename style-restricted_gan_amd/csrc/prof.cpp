// The launch timer's storage (prof.h): the slots of the current session, the pool of events they draw from, and the
// srgan_prof_* entries bench.py reads them through.
#include <utility>
#include <vector>
#include "common.h"
#include "prof.h"

namespace srgan {

struct ProfSlot { hipEvent_t a, b; int kid; double flops; };
static bool g_prof_on = false;
static std::vector<ProfSlot> g_prof_slots;      // used slots of the current session
static std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_pool;
static size_t g_prof_next = 0;

static const char* const kProfNames[] = {
#define SRGAN_PROF_NAME(id, name) name,
    SRGAN_PROF_KERNELS(SRGAN_PROF_NAME)
#undef SRGAN_PROF_NAME
};
static_assert(sizeof(kProfNames) / sizeof(kProfNames[0]) == kProfKernels, "one name per enumerator");

long prof_open(ProfKernel kid, double flops, hipStream_t st) {
  if (!g_prof_on) return -1;
  if (g_prof_next == g_prof_pool.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return -1;
    g_prof_pool.emplace_back(a, b);
  }
  auto& ev = g_prof_pool[g_prof_next++];
  g_prof_slots.push_back({ev.first, ev.second, kid, flops});
  (void)hipEventRecord(ev.first, st);
  return (long)g_prof_slots.size() - 1;
}

void prof_close(long slot, hipStream_t st) { (void)hipEventRecord(g_prof_slots[slot].b, st); }

}  // namespace srgan

using namespace srgan;

// ---- launch-timer API (used only by bench.py) ------------------------------------------------
extern "C" int srgan_prof_enable(int on) {
  if (on) {
    g_prof_slots.clear();
    g_prof_next = 0;
  }
  g_prof_on = on != 0;
  return 0;
}
extern "C" int srgan_prof_num_kernels(void) { return kProfKernels; }
extern "C" const char* srgan_prof_kernel_name(int kid) {
  return (kid >= 0 && kid < kProfKernels) ? kProfNames[kid] : "";
}
// One timed launch of the session (index < srgan_prof_num_slots()): kernel id, duration, algorithmic FLOPs.
extern "C" int srgan_prof_num_slots(void) { return (int)g_prof_slots.size(); }
extern "C" int srgan_prof_slot(int index, int* kid, double* ms, double* flops) {
  SRGAN_REQUIRE(kid && ms && flops, "prof_slot: null pointer");
  SRGAN_REQUIRE(index >= 0 && (size_t)index < g_prof_slots.size(), "prof_slot: index out of range");
  const ProfSlot& s = g_prof_slots[index];
  float t = 0.f;
  hipError_t e = hipEventElapsedTime(&t, s.a, s.b);
  if (e != hipSuccess) { set_error("prof_slot: %s", hipGetErrorString(e)); return (int)e; }
  *kid = s.kid; *ms = t; *flops = s.flops;
  return 0;
}
// Totals of the session for one kernel id; call after the streams have been synchronised.
extern "C" int srgan_prof_collect(int kid, double* total_ms, long long* launches, double* total_flops) {
  SRGAN_REQUIRE(total_ms && launches && total_flops, "prof_collect: null pointer");
  double ms = 0.0, fl = 0.0;
  long long n = 0;
  for (const ProfSlot& s : g_prof_slots) {
    if (s.kid != kid) continue;
    float t = 0.f;
    hipError_t e = hipEventElapsedTime(&t, s.a, s.b);
    if (e != hipSuccess) { set_error("prof_collect: %s", hipGetErrorString(e)); return (int)e; }
    ms += t; fl += s.flops; ++n;
  }
  *total_ms = ms; *launches = n; *total_flops = fl;
  return 0;
}
