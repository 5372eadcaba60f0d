// LeCam regularisation of the discriminator (Tseng et al., 2021, "Regularizing Generative Adversarial Networks under Limited Data"):
// extension, no counterpart in the reference.  DESIGN.md section 7 ("LeCam regularisation") has the formulas; srgan_amd/lecam.py
// holds the record, ops.d_losses / ops.d_losses_cr launch the kernel behind their own.
//
//   lecam_kernel    one launch per discriminator update, one workgroup, no atomics, every sum has one owner and a fixed order.
//                   Maps o_s [rows][per_s]; the front P rows are what D reads anyway: elements [0, n1) of a map are real, [n1, n1 + n2)
//                   generated (n1 = rows_first per_s, n2 = (P - rows_first) per_s); back rows (bCR partners) are never touched.
//                     pass 1   the 2S sums of the front elements -> the batch means -> the anchors (exponential moving averages in the
//                              device record: the first update sets them, a non-finite mean moves none and does not count)
//                     pass 2   R = (1/S) sum_s [ mean_real phi(o - a_F,s)^2 + mean_fake phi(a_R,s - o)^2 ] with the UPDATED anchors as
//                              constants, and -- iff weight != 0 and updates >= start, a SELECT: otherwise d_o is not even read --
//                              d_o += the term's gradient.  phi: identity, or relu (clamp).
//                   Order of a sum: element e belongs to quad e / 4, thread t owns quads t, t + 256, ... and adds its elements
//                   ascending into ONE accumulator per sum; the 64 lanes of a wave by the xor butterfly (32, 16, ... 1), the four
//                   waves ascending.  A quad is one 16-byte load where the map's base and per_s allow (vec), four 4-byte loads
//                   otherwise: same owner, same order, same bits.  No contraction in this file: products and sums round separately
//                   (tests/lecam_common.py replays the order in numpy).
#include "common.h"
#include "records.h"
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace srgan {

struct LcParams {
  const float* o[4];
  float* d_o[4];
  int per[4];
  int vec[4];
  const float* total_in;
  float* vals;
  LcState* st;
  int n_scales, pairs, rows_first, clamp;
};

// The four waves' sums of eight values at once: two barriers for all of them.  `red` holds 32 floats.
__device__ __forceinline__ void lc_block_sum8(float (&v)[8], float* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = wave_sum(v[j]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[w * 8 + j] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float t = 0.f;
    for (int i = 0; i < 4; ++i) t += red[i * 8 + j];
    v[j] = t;
  }
}

// Quad q of a map's N front elements into x[0, cnt)
__device__ __forceinline__ int lc_load_quad(const float* __restrict__ o, int q, int N, int vec, float (&x)[4]) {
  const long long e0 = 4LL * q;
  if (vec) {                                                 // N % 4 == 0: the four floats exist
    const f32x4 v = *reinterpret_cast<const f32x4*>(o + e0);
    x[0] = v[0]; x[1] = v[1]; x[2] = v[2]; x[3] = v[3];
    return 4;
  }
  const int cnt = N - e0 < 4 ? (int)(N - e0) : 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = k < cnt ? o[e0 + k] : 0.f;
  return cnt;
}

__device__ __forceinline__ bool lc_finite(float v) { return fabsf(v) <= 3.4028234664e38f; }      // false for NaN, +-Inf

__global__ __launch_bounds__(256) void lecam_kernel(LcParams p) {
  __shared__ float red[32];
  const int tid = threadIdx.x;
  const int S = p.n_scales, P = p.pairs, B1 = p.rows_first, B2 = P - B1;
  const float ws = 1.f / (float)S;
  const float weight = p.st->weight, decay = p.st->decay;
  const int start = p.st->start, n = p.st->updates;
  float a_r[4], a_f[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) { a_r[s] = p.st->a_real[s]; a_f[s] = p.st->a_fake[s]; }
  const float total_in = *p.total_in;

  // ---- pass 1: the 2S sums ----
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};         // [2 s]: real, [2 s + 1]: generated
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s >= S) break;
    const int per = p.per[s], n1 = B1 * per, N = P * per, nq = (int)(((long long)N + 3) >> 2);
    float sr = 0.f, sf = 0.f;
#pragma unroll 4
    for (int q = tid; q < nq; q += 256) {
      float x[4];
      const int cnt = lc_load_quad(p.o[s], q, N, p.vec[s], x);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < cnt) {
          if (4LL * q + k < n1) sr += x[k]; else sf += x[k];
        }
      }
    }
    acc[2 * s] = sr; acc[2 * s + 1] = sf;
  }
  lc_block_sum8(acc, red);

  // ---- the anchors: every thread computes the same values, thread 0 stores them at the end ----
  bool ok = true;
  float m_r[4], m_f[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s >= S) break;
    const int per = p.per[s];
    m_r[s] = acc[2 * s] / (float)(B1 * per);
    m_f[s] = acc[2 * s + 1] / (float)(B2 * per);
    if (B1 > 0) ok = ok && lc_finite(m_r[s]);
    if (B2 > 0) ok = ok && lc_finite(m_f[s]);
  }
  const float d = n == 0 ? 0.f : decay;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s >= S) break;
    if (ok && B1 > 0) a_r[s] = d * a_r[s] + (1.f - d) * m_r[s];
    if (ok && B2 > 0) a_f[s] = d * a_f[s] + (1.f - d) * m_f[s];
  }

  // ---- pass 2: the term and its gradient ----
  const bool active = weight != 0.f && n >= start;
  const bool relu = p.clamp != 0;
  float q8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s >= S) break;
    const int per = p.per[s], n1 = B1 * per, n2 = B2 * per, N = P * per, nq = (int)(((long long)N + 3) >> 2);
    const float k1 = n1 > 0 ? 2.f * weight * ws / (float)n1 : 0.f;
    const float k2 = n2 > 0 ? 2.f * weight * ws / (float)n2 : 0.f;
    const float af = a_f[s], ar = a_r[s];
    const int vec = p.vec[s];
    float* __restrict__ go = p.d_o[s];
    float q1 = 0.f, q2 = 0.f;
#pragma unroll 2
    for (int q = tid; q < nq; q += 256) {
      float x[4], g[4];
      const int cnt = lc_load_quad(p.o[s], q, N, vec, x);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        g[k] = 0.f;
        if (k < cnt) {
          const bool real = 4LL * q + k < n1;
          float ph = real ? x[k] - af : ar - x[k];
          if (relu) ph = ph < 0.f ? 0.f : ph;               // a NaN stays a NaN, as in torch.relu
          const float sq = ph * ph;
          if (real) q1 += sq; else q2 += sq;
          g[k] = real ? k1 * ph : -(k2 * ph);
        }
      }
      if (active) {
        if (vec) {
          f32x4 v = *reinterpret_cast<const f32x4*>(go + 4LL * q);
          v[0] += g[0]; v[1] += g[1]; v[2] += g[2]; v[3] += g[3];
          *reinterpret_cast<f32x4*>(go + 4LL * q) = v;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < cnt) go[4LL * q + k] += g[k];
        }
      }
    }
    q8[2 * s] = q1; q8[2 * s + 1] = q2;
  }
  lc_block_sum8(q8, red);

  if (tid == 0) {
    float R = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (s >= S) break;
      const int per = p.per[s], n1 = B1 * per, n2 = B2 * per;
      if (n1 > 0) R += ws * q8[2 * s] / (float)n1;
      if (n2 > 0) R += ws * q8[2 * s + 1] / (float)n2;
    }
    const float wr = weight * R;
    p.vals[0] = R;
    p.vals[1] = active ? wr : 0.f;
    p.vals[2] = active ? total_in + wr : total_in;          // a select: off, the incoming total's bits
    LcState* st = p.st;
    if (ok) {
#pragma unroll
      for (int s = 0; s < 4; ++s) { st->a_real[s] = a_r[s]; st->a_fake[s] = a_f[s]; }       // (scales past S: what was read)
      st->updates = n + 1;
    }
    st->penalty = R;
    st->applied = active ? 1 : 0;
  }
}

static bool lc_settings_ok(float weight, float decay, int start) {
  return weight >= 0.f && weight <= 3.0e38f && decay >= 0.f && decay < 1.f && start >= 0;
}

}  // namespace srgan

using namespace srgan;

extern "C" size_t srgan_lc_state_bytes(void) { return sizeof(srgan::LcState); }

extern "C" int srgan_lc_state_init(void* state, float weight, float decay, int start, void* stream) {
  SRGAN_REQUIRE(state && lc_settings_ok(weight, decay, start),
                "lc_state_init: bad argument (a record; weight >= 0 and finite, decay in [0, 1), start >= 0; NaN refused)");
  LcState s = {};                        // the counter, the anchors, the term and the flag at zero
  s.weight = weight; s.decay = decay; s.start = start;
  return record_write(state, &s, sizeof s, record_all_words<LcState>(), as_stream(stream), "lc_state_init");
}

extern "C" int srgan_lc_state_set(void* state, float weight, float decay, int start, void* stream) {
  SRGAN_REQUIRE(state && lc_settings_ok(weight, decay, start),
                "lc_state_set: bad argument (a record; weight >= 0 and finite, decay in [0, 1), start >= 0; NaN refused)");
  LcState s = {};
  s.weight = weight; s.decay = decay; s.start = start;
  return record_write(state, &s, sizeof s, kLcSet, as_stream(stream), "lc_state_set");
}

extern "C" int srgan_lc_state_restore(void* state, int updates, const float* a_real, const float* a_fake, void* stream) {
  SRGAN_REQUIRE(state && a_real && a_fake && updates >= 0, "lc_state_restore: bad argument (a record; two host arrays of 4; updates >= 0)");
  LcState s = {};                        // resume: the settings, the last term and the flag stay
  s.updates = updates;
  for (int i = 0; i < 4; ++i) {
    SRGAN_REQUIRE(std::fabs(a_real[i]) <= 3.0e38f && std::fabs(a_fake[i]) <= 3.0e38f,
                  "lc_state_restore: anchor %d is not finite (NaN refused)", i);
    s.a_real[i] = a_real[i]; s.a_fake[i] = a_fake[i];
  }
  return record_write(state, &s, sizeof s, kLcRestore, as_stream(stream), "lc_state_restore");
}

extern "C" int srgan_lecam(const float* const* o, const long long* per_row, int n_scales, int rows, int pairs, int rows_first, int clamp,
                           const float* total_in, float* vals, float* const* d_o, void* state, void* stream) {
  SRGAN_REQUIRE(o && per_row && d_o && total_in && vals && state, "lecam: null pointer");
  SRGAN_REQUIRE(n_scales >= 1 && n_scales <= 4, "lecam: %d scales (1..4)", n_scales);
  SRGAN_REQUIRE(pairs >= 1 && (rows == pairs || (long long)rows == 2LL * pairs),
                "lecam: rows = %d, the maps hold pairs = %d rows or 2 * pairs", rows, pairs);
  SRGAN_REQUIRE(rows_first >= 0 && rows_first <= pairs, "lecam: bad row split (rows_first = %d outside [0, pairs = %d])", rows_first,
                pairs);
  SRGAN_REQUIRE(clamp == 0 || clamp == 1, "lecam: clamp = %d (0: the squared distance, 1: the one-sided form)", clamp);
  SRGAN_REQUIRE(((reinterpret_cast<uintptr_t>(total_in) | reinterpret_cast<uintptr_t>(vals) | reinterpret_cast<uintptr_t>(state)) & 3) == 0,
                "lecam: pointer not 4-byte aligned");
  LcParams p{};
  p.n_scales = n_scales; p.pairs = pairs; p.rows_first = rows_first; p.clamp = clamp;
  p.total_in = total_in; p.vals = vals; p.st = static_cast<LcState*>(state);
  for (int s = 0; s < n_scales; ++s) {
    SRGAN_REQUIRE(o[s] && d_o[s] && per_row[s] > 0, "lecam: null scale");
    SRGAN_REQUIRE(per_row[s] * rows < (1LL << 31), "lecam: map %d has %lld elements per row (rows * per_row < 2^31)", s, per_row[s]);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(o[s]) | reinterpret_cast<uintptr_t>(d_o[s]);
    SRGAN_REQUIRE((bits & 3) == 0, "lecam: pointer not 4-byte aligned");
    p.o[s] = o[s]; p.d_o[s] = d_o[s]; p.per[s] = (int)per_row[s];
    p.vec[s] = (bits & 15) == 0 && per_row[s] % 4 == 0;
  }
  hipLaunchKernelGGL(lecam_kernel, dim3(1), dim3(256), 0, as_stream(stream), p);      // no launch-timer slot, as d_losses_kernel
  return check_launch("lecam_kernel");
}
