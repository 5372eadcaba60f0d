// Adaptive discriminator augmentation (Karras et al., 2020, "Training Generative Adversarial Networks with Limited Data", sections
// 2.2 and 3): the probability p with which each DiffAugment group is applied to a sample, held and moved on the device.  Extension,
// no counterpart in the reference.  DESIGN.md section 7 ("Adaptive augmentation") has the controller; srgan_amd/ada.py drives it.
//
// A recorded step is replayed without the host, so p, the overfitting heuristic's counters and the per-sample decision "is this
// group applied?" are device state:
//
//   ada_gate_kernel     one thread per sample: row of 16 floats [7 parameters of a stage's table row, -, u_0 .. u_{n_groups - 1}, ...]
//                       (the uniforms in [0, 1) pre-drawn on the host; DiffAugment has 3 groups, the geometric stage 4) -> row of 8
//                       floats for the gated kernels of augment.hip / augment_geom.hip: slots 0..6 copied, slot 7 = the float of
//                       the skip mask whose bit g < n_groups is set iff !(u_g < p).  p = 0 skips everything, p = 1 nothing, a NaN
//                       uniform skips.
//   ada_observe_kernel  one workgroup of 256 threads: over the first B rows of up to 4 discriminator maps n_pos += #(v > thr),
//                       n_neg += #(v < thr), n_total += #elements (a NaN counts in n_total only); integer counts, so the order of
//                       the reduction does not matter: thread-strided, a butterfly inside each wave, four LDS slots.  Thread 0 then
//                       runs the controller:
//                         seen += 1
//                         if seen >= interval:                    (== in every run that starts below interval)
//                           r = float(n_pos - n_neg) / float(n_total);  d = (r > target) - (r < target)
//                           p = min(max(p + d * step, 0), p_max)        (one fp32 add, then the clamp)
//                           n_pos = n_neg = n_total = seen = 0;  adjustments += 1;  last_r = r
//
// Plain global stores, no atomics, fp contraction off.
#include "common.h"
#include "records.h"
#include <cstdint>

#pragma clang fp contract(off)

namespace srgan {

constexpr int kAdaMaxScales = 4;
constexpr int kAdaRowIn = 16;       // floats per row the gate reads
constexpr int kAdaRowOut = 8;       // floats per row it writes (the table row of augment.hip and augment_geom.hip)
constexpr int kAdaMaxGroups = 4;    // uniforms per row it can read (slots 8..11)

struct AdaMaps {
  const float* map[kAdaMaxScales];
  long long count[kAdaMaxScales];   // elements of the first B rows
};

__global__ __launch_bounds__(256) void ada_gate_kernel(const float* __restrict__ rows, const AdaState* __restrict__ st,
                                                       float* __restrict__ table, int n, int n_groups) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n) return;
  const float p = st->p;
  const float* r = rows + (size_t)i * kAdaRowIn;
  float* t = table + (size_t)i * kAdaRowOut;
  const f32x4 a = *reinterpret_cast<const f32x4*>(r), b = *reinterpret_cast<const f32x4*>(r + 4);
  const f32x4 u = *reinterpret_cast<const f32x4*>(r + 8);
  int mask = 0;
#pragma unroll
  for (int g = 0; g < kAdaMaxGroups; ++g) mask |= (g >= n_groups || u[g] < p) ? 0 : (1 << g);
  *reinterpret_cast<f32x4*>(t) = a;
  const f32x4 hi = {b[0], b[1], b[2], (float)mask};
  *reinterpret_cast<f32x4*>(t + 4) = hi;
}

__device__ __forceinline__ long long ada_wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void ada_observe_kernel(AdaMaps m, int n_scales, float thr, AdaState* __restrict__ s) {
  __shared__ long long red[4][3];
  long long pos = 0, neg = 0, tot = 0;
  for (int k = 0; k < n_scales; ++k) {
    const float* __restrict__ v = m.map[k];
    const long long cnt = m.count[k];
    for (long long i = threadIdx.x; i < cnt; i += 256) {
      const float x = v[i];
      pos += x > thr ? 1 : 0;
      neg += x < thr ? 1 : 0;
    }
    tot += cnt;                                     // (every thread holds the whole count; thread 0's is used)
  }
  pos = ada_wave_sum(pos);
  neg = ada_wave_sum(neg);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = pos;
    red[threadIdx.x >> 6][1] = neg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long n_pos = s->n_pos + (red[0][0] + red[1][0] + red[2][0] + red[3][0]);
    const long long n_neg = s->n_neg + (red[0][1] + red[1][1] + red[2][1] + red[3][1]);
    const long long n_total = s->n_total + tot;
    const int seen = s->seen + 1;
    if (seen >= s->interval) {
      const float r = (float)(n_pos - n_neg) / (float)n_total;
      const float target = s->target;
      const float d = (float)((r > target ? 1 : 0) - (r < target ? 1 : 0));
      const float p = s->p + d * s->step;
      s->p = fminf(fmaxf(p, 0.f), s->p_max);
      s->last_r = r;
      s->n_pos = 0; s->n_neg = 0; s->n_total = 0; s->seen = 0;
      s->adjustments += 1;
    } else {
      s->n_pos = n_pos; s->n_neg = n_neg; s->n_total = n_total; s->seen = seen;
    }
  }
}

static bool ada_settings_ok(float target, float step, float p_max, int interval) {
  return target >= -3.0e38f && target <= 3.0e38f && step >= 0.f && step <= 3.0e38f && p_max >= 0.f && p_max <= 1.f && interval >= 1;
}

}  // namespace srgan

using namespace srgan;

extern "C" size_t srgan_ada_state_bytes(void) { return sizeof(srgan::AdaState); }

extern "C" int srgan_ada_state_init(void* state, float p, float target, float step, float p_max, int interval, void* stream) {
  SRGAN_REQUIRE(state && srgan::ada_settings_ok(target, step, p_max, interval) && p >= 0.f && p <= p_max,
                "ada_state_init: bad argument (target finite, step >= 0 and finite, 0 <= p <= p_max <= 1, interval >= 1; NaN refused)");
  srgan::AdaState s = {};                // the counters and last_r at zero
  s.p = p; s.target = target; s.step = step; s.p_max = p_max; s.interval = interval;
  return srgan::record_write(state, &s, sizeof s, srgan::record_all_words<srgan::AdaState>(), as_stream(stream), "ada_state_init");
}

extern "C" int srgan_ada_state_set(void* state, float target, float step, float p_max, int interval, int set_p, float p,
                                   void* stream) {
  SRGAN_REQUIRE(state && srgan::ada_settings_ok(target, step, p_max, interval) && (!set_p || (p >= 0.f && p <= p_max)),
                "ada_state_set: bad argument (target finite, step >= 0 and finite, 0 <= p <= p_max <= 1, interval >= 1; NaN refused)");
  srgan::AdaState s = {};
  s.target = target; s.step = step; s.p_max = p_max; s.interval = interval; s.p = set_p ? p : 0.f;
  return srgan::record_write(state, &s, sizeof s, srgan::kAdaSet | (set_p ? srgan::kAdaSetP : 0u), as_stream(stream),
                             "ada_state_set");
}

extern "C" int srgan_ada_state_set_counters(void* state, int seen, long long n_pos, long long n_neg, long long n_total,
                                            int adjustments, float last_r, void* stream) {
  SRGAN_REQUIRE(state && seen >= 0 && n_pos >= 0 && n_neg >= 0 && n_total >= 0 && n_pos + n_neg <= n_total && adjustments >= 0,
                "ada_state_set_counters: bad argument (counts >= 0, n_pos + n_neg <= n_total)");
  srgan::AdaState s = {};                // resume: the settings and p stay
  s.seen = seen; s.n_pos = n_pos; s.n_neg = n_neg; s.n_total = n_total; s.adjustments = adjustments; s.last_r = last_r;
  return srgan::record_write(state, &s, sizeof s, srgan::kAdaSetCounters, as_stream(stream), "ada_state_set_counters");
}

extern "C" int srgan_ada_gate(const float* rows, const void* state, float* table, int n, int n_groups, void* stream) {
  SRGAN_REQUIRE(rows && state && table, "ada_gate: null pointer");
  SRGAN_REQUIRE(n > 0, "ada_gate: n = %d rows (n > 0)", n);
  SRGAN_REQUIRE(n_groups >= 1 && n_groups <= srgan::kAdaMaxGroups, "ada_gate: n_groups = %d (1 to %d)", n_groups,
                srgan::kAdaMaxGroups);
  SRGAN_REQUIRE(((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(table)) & 15) == 0,
                "ada_gate: rows / table not 16-byte aligned");
  SRGAN_REQUIRE(static_cast<const void*>(rows) != static_cast<const void*>(table), "ada_gate: the table must not alias the rows");
  hipLaunchKernelGGL(srgan::ada_gate_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, as_stream(stream), rows,
                     static_cast<const srgan::AdaState*>(state), table, n, n_groups);
  return check_launch("ada_gate_kernel");
}

extern "C" int srgan_ada_observe(const float* const* maps, const long long* per_sample, int n_scales, int rows_first, float thr,
                                 void* state, void* stream) {
  SRGAN_REQUIRE(state, "ada_observe: null record");
  SRGAN_REQUIRE(n_scales >= 1 && n_scales <= srgan::kAdaMaxScales, "ada_observe: %d scales (1 to %d)", n_scales, srgan::kAdaMaxScales);
  SRGAN_REQUIRE(maps && per_sample, "ada_observe: null pointer");
  SRGAN_REQUIRE(rows_first > 0, "ada_observe: B = %d real rows (B > 0)", rows_first);
  SRGAN_REQUIRE(thr >= -3.0e38f && thr <= 3.0e38f, "ada_observe: the threshold must be finite");
  srgan::AdaMaps m = {};
  for (int k = 0; k < n_scales; ++k) {
    SRGAN_REQUIRE(maps[k], "ada_observe: map %d is a null pointer", k);
    SRGAN_REQUIRE((reinterpret_cast<uintptr_t>(maps[k]) & 3) == 0, "ada_observe: map %d not 4-byte aligned", k);
    SRGAN_REQUIRE(per_sample[k] > 0 && per_sample[k] <= (1LL << 40) / rows_first, "ada_observe: map %d has %lld elements per row (> 0)",
                  k, per_sample[k]);
    m.map[k] = maps[k];
    m.count[k] = per_sample[k] * rows_first;
  }
  hipLaunchKernelGGL(srgan::ada_observe_kernel, dim3(1), dim3(256), 0, as_stream(stream), m, n_scales, thr,
                     static_cast<srgan::AdaState*>(state));
  return check_launch("ada_observe_kernel");
}
