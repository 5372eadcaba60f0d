// Balanced consistency regularisation of the discriminator (Zhang et al., 2020; the balanced form on real AND generated samples:
// Zhao et al., 2020): extension, no counterpart in the reference.  DESIGN.md section 7 ("Balanced consistency regularisation") has
// the formulas; srgan_amd/consistency.py draws the tables and holds the record, the trainer's update_D drives the two kernels.
//
//   cr_pairs_kernel       y[2n] from one or two fp32 NHWC-dense three-channel sources of n = n0 + n1 images: rows [0, n) are a bit
//                         copy of the concatenated sources, row n + r is T of row r -- an x-flip, then an integer translation with
//                         zeros shifted in: T(x)[i, j] = xf[i - ty, j - tx] inside the image, else 0, xf[i, j] = fx ? x[i, W-1-j] :
//                         x[i, j].  One table row of 8 floats per source image, [fx, ty, tx, 0, ...]; the groups that run (flags:
//                         flip 1, translation 2) are a launch argument, a group that is off is the identity.  T copies VALUES: no
//                         arithmetic touches a pixel, so -0.0 and NaN payloads arrive as they are.  An item = 4096 consecutive floats
//                         of one output image; a thread owns 4 consecutive floats (one 16-byte store, and one 16-byte load in a copy
//                         row; the gather of a T row is scalar) -- scalar path: float t + 256 u.  Same bits on both paths.
//   d_losses_cr_kernel    everything d_losses_kernel (losses.hip) does for the front P rows of maps that hold 2P, then the consistency
//                         terms between row r and row r + P and their gradients.  One workgroup, no atomics, every sum has one owner
//                         and a fixed order.  The weights come from the device record.
//
// The loss kernel keeps the default fp contraction of losses.hip, and the front rows' statements are d_losses_kernel's own: with both
// weights 0 its vals[0..3], d_o and dz of the front rows are that kernel's bits (tests/test_cr_kernels_gpu.py holds it to that).
#include "common.h"
#include "prof.h"
#include "loss_math.h"
#include "records.h"
#include <algorithm>
#include <cstdint>

namespace srgan {

constexpr int kCrRow = 8;           // floats per table row
constexpr int kCrItem = 4096;       // floats per item
constexpr int kCrGridCap = 2048;    // 256 CUs x 8 workgroups; the rest by grid stride
constexpr int CR_FLIP = 1, CR_TRANSLATION = 2, CR_ALL = 3;

// A table value as an integer in [lo, hi]: truncated, clamped while still a float; a non-finite value reads 0.
__device__ __forceinline__ int cr_int(float v, int lo, int hi) {
  if (!(fabsf(v) <= 3.0e38f)) return 0;                      // NaN, +-Inf
  return (int)fminf(fmaxf(truncf(v), (float)lo), (float)hi);
}

struct CrXf { int fx, ty, tx; };

__device__ __forceinline__ CrXf cr_xf(const float* __restrict__ row, int flags, int H, int W) {
  CrXf t{0, 0, 0};
  if (flags & CR_FLIP) t.fx = cr_int(row[0], 0, 1);
  if (flags & CR_TRANSLATION) { t.ty = cr_int(row[1], -(H - 1), H - 1); t.tx = cr_int(row[2], -(W - 1), W - 1); }
  return t;
}

// T(x) at element e (channel-fastest) of one image
__device__ __forceinline__ float cr_gather(const float* __restrict__ src, const CrXf& t, int e, int H, int W) {
  const int p = e / 3, c = e - 3 * p;
  const int i = p / W, j = p - i * W;
  const int si = i - t.ty, sj = j - t.tx;
  if (si < 0 || si >= H || sj < 0 || sj >= W) return 0.f;
  const int sc = t.fx ? W - 1 - sj : sj;
  return src[((size_t)si * W + sc) * 3 + c];
}

__global__ __launch_bounds__(256) void cr_pairs_kernel(const float* __restrict__ x0, int n0, const float* __restrict__ x1, int n,
                                                       const float* __restrict__ table, float* __restrict__ y, int H, int W,
                                                       int flags, int nitem, long long items, int vec) {
  const int E = 3 * H * W;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int r = (int)(it / nitem), item = (int)(it - (long long)r * nitem);       // output image r of 2n
    const int q = r < n ? r : r - n;                                                  // its source image
    const float* src = q < n0 ? x0 + (size_t)q * E : x1 + (size_t)(q - n0) * E;
    float* dst = y + (size_t)r * E;
    const bool copy = r < n;                                                           // uniform per item
    CrXf t{0, 0, 0};
    if (!copy) t = cr_xf(table + (size_t)q * kCrRow, flags, H, W);
    const int base = item * kCrItem;
    if (vec) {                                               // E % 4 == 0, every pointer 16-byte aligned: the four floats exist
#pragma unroll
      for (int u = 0; u < kCrItem / 1024; ++u) {
        const int e0 = base + (u * 256 + (int)threadIdx.x) * 4;
        if (e0 >= E) continue;
        f32x4 v;
        if (copy) {
          v = *reinterpret_cast<const f32x4*>(src + e0);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = cr_gather(src, t, e0 + k, H, W);
        }
        *reinterpret_cast<f32x4*>(dst + e0) = v;
      }
    } else {
#pragma unroll 4
      for (int u = 0; u < kCrItem / 256; ++u) {
        const int e = base + u * 256 + (int)threadIdx.x;
        if (e >= E) continue;
        dst[e] = copy ? src[e] : cr_gather(src, t, e, H, W);
      }
    }
  }
}

// ---- the fused loss ------------------------------------------------------------------------------------------------------------
// Maps o_s [2P][per_s], class logits z_s [2P][nc].  Front rows [0, P): d_losses_kernel with rows = P.  Row r + P is the consistency
// partner of row r; pairs [0, pairs_first) are group 1 (lambda_real), the rest group 2 (lambda_fake).  With m_s(r) the mean of row r:
//   cr_g   = (1 / S) sum_s (1 / B_g) sum_{r in g} (m_s(r) - m_s(r + P))^2
//   d_o_s[r, j] += k_g (m_s(r) - m_s(r + P)),  d_o_s[r + P, j] = -k_g (...),  k_g = 2 c_g / (S B_g per_s),  c_g = lambda_g * every
// A group with c_g == 0 or B_g == 0 is taken out by a SELECT: its front rows keep the GAN gradient's bits, its back rows get exactly 0
// whatever they hold, and total_with_cr does not see its term.
struct CrLossParams {
  const float* o[4];
  const float* z[4];
  float* d_o[4];
  float* dz[4];
  long long per[4];
  const long long* label;
  float* vals;
  CrState* st;
  int n_scales, pairs, pairs_first, rows_first, nc;
  float t_first, t_rest, w_class;
};

template <int GK, int CK>
__global__ __launch_bounds__(256) void d_losses_cr_kernel(CrLossParams p) {
  __shared__ float red[16];
  __shared__ float coef[2 * SRGAN_CR_MAX_PAIRS];      // the 2P row means of a scale; then [0, P): k_g * difference of the pair
  const int P = p.pairs, B1 = p.pairs_first, B2 = P - B1;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float ws = 1.f / (float)p.n_scales;
  const float c1 = p.st->lambda_real * (float)p.st->every, c2 = p.st->lambda_fake * (float)p.st->every;
  const bool on1 = c1 != 0.f && B1 > 0, on2 = c2 != 0.f && B2 > 0;
  float first = 0.f, rest = 0.f, cls = 0.f, cr1 = 0.f, cr2 = 0.f;
  for (int s = 0; s < p.n_scales; ++s) {
    const int per = (int)p.per[s];
    // row means: a wave per row, lane l adds elements l, l + 64, ... ascending, then the butterfly.  A wave takes four rows at a
    // time (independent sums: their loads are in flight together; the passes are latency-bound), each in that same order.
    for (int r0 = wv * 4; r0 < 2 * P; r0 += 16) {
      float a[4] = {0.f, 0.f, 0.f, 0.f};
      for (int j = lane; j < per; j += 64) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (r0 + u < 2 * P) a[u] += p.o[s][(size_t)(r0 + u) * per + j];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float m = wave_sum(a[u]);
        if (lane == 0 && r0 + u < 2 * P) coef[r0 + u] = m / (float)per;
      }
    }
    __syncthreads();
    // thread t owns pairs t, t + 256, ...: it alone reads coef[r], coef[r + P] and rewrites coef[r]
    const float k1 = on1 ? 2.f * c1 * ws / ((float)B1 * (float)per) : 0.f;
    const float k2 = on2 ? 2.f * c2 * ws / ((float)B2 * (float)per) : 0.f;
    float q1 = 0.f, q2 = 0.f;
    for (int r = tid; r < P; r += 256) {
      const float d = coef[r] - coef[r + P];
      const bool in1 = r < B1;
      if (in1) q1 += d * d; else q2 += d * d;
      coef[r] = in1 ? (on1 ? k1 * d : 0.f) : (on2 ? k2 * d : 0.f);
    }
    q1 = block_sum(q1, red);                           // (its barriers also publish coef[0, P))
    q2 = block_sum(q2, red);
    if (B1 > 0) cr1 += ws * q1 / (float)B1;
    if (B2 > 0) cr2 += ws * q2 / (float)B2;

    // ---- the front P rows: d_losses_kernel's statements, the store extended by the pair's coefficient ----
    const long long n1 = (long long)p.rows_first * p.per[s], n2 = (long long)(P - p.rows_first) * p.per[s];
    float g1, g2;
    if constexpr (GK == CRIT_MSE) {
      g1 = n1 > 0 ? 2.f * ws / (float)n1 : 0.f; g2 = n2 > 0 ? 2.f * ws / (float)n2 : 0.f;
    } else {
      g1 = n1 > 0 ? ws / (float)n1 : 0.f; g2 = n2 > 0 ? ws / (float)n2 : 0.f;
    }
    float s1 = 0.f, s2 = 0.f;
    for (long long i = threadIdx.x; i < n1 + n2; i += blockDim.x) {
      const bool f = i < n1;
      const int r = (int)i / per;
      const bool on = r < B1 ? on1 : on2;
      if constexpr (GK == CRIT_MSE) {
        const float d = p.o[s][i] - (f ? p.t_first : p.t_rest);
        if (f) s1 += d * d; else s2 += d * d;
        const float base = (f ? g1 : g2) * d;
        p.d_o[s][i] = on ? base + coef[r] : base;
      } else {
        float d;
        const float v = bce_logit(p.o[s][i], f ? p.t_first : p.t_rest, d);
        if (f) s1 += v; else s2 += v;
        const float base = (f ? g1 : g2) * d;
        p.d_o[s][i] = on ? base + coef[r] : base;
      }
    }
    // ---- the back P rows: the negative coefficient, nothing else ----
    for (int i = tid; i < P * per; i += 256) {
      const int r = i / per;
      const bool on = r < B1 ? on1 : on2;
      p.d_o[s][(size_t)P * per + i] = on ? -coef[r] : 0.f;
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    if (n1 > 0) first += ws * s1 / (float)n1;
    if (n2 > 0) rest += ws * s2 / (float)n2;
    if (p.z[s]) {
      const int nc = p.nc;
      const float gs = CK == CRIT_MSE ? 2.f * ws * p.w_class / (float)(p.rows_first * nc) : ws * p.w_class / (float)(p.rows_first * nc);
      float sc = 0.f;
      for (int b = threadIdx.x; b < 2 * P; b += blockDim.x) {
        if (b >= p.rows_first) {                        // the translated half, and every back row: no class loss
          for (int j = 0; j < nc; ++j) p.dz[s][b * nc + j] = 0.f;
          continue;
        }
        float qq[16], dq[16];
        if constexpr (CK == CRIT_BCE) {
          for (int j = 0; j < nc; ++j) dq[j] = p.z[s][b * nc + j];
          sc += softmax_bce_row(dq, nc, (int)p.label[b], gs, qq, p.dz[s] + b * nc);
          continue;
        }
        float mx = -INFINITY;
        for (int j = 0; j < nc; ++j) mx = fmaxf(mx, p.z[s][b * nc + j]);
        float den = 0.f;
        for (int j = 0; j < nc; ++j) { qq[j] = expf(p.z[s][b * nc + j] - mx); den += qq[j]; }
        const int lab = (int)p.label[b];
        float dot = 0.f;
        for (int j = 0; j < nc; ++j) {
          qq[j] /= den;
          const float d = qq[j] - (j == lab ? 1.f : 0.f);
          sc += d * d;
          dq[j] = gs * d;
          dot += qq[j] * dq[j];
        }
        for (int j = 0; j < nc; ++j) p.dz[s][b * nc + j] = qq[j] * (dq[j] - dot);
      }
      sc = block_sum(sc, red);
      cls += ws * sc / (float)(p.rows_first * nc);
    }
    __syncthreads();                                    // coef is rewritten by the next scale
  }
  if (threadIdx.x == 0) {
    p.vals[0] = first;
    p.vals[1] = cls;
    p.vals[2] = rest;
    p.vals[3] = first + cls * p.w_class + rest;
    p.vals[4] = cr1;
    p.vals[5] = cr2;
    // the select is on the operand: a group that is off adds exactly 0 even where its raw term is NaN
    p.vals[6] = p.vals[3] + (c1 * (on1 ? cr1 : 0.f) + c2 * (on2 ? cr2 : 0.f));
    p.st->cr_real = cr1;
    p.st->cr_fake = cr2;
    p.st->updates += 1;
  }
}

static bool cr_weights_ok(float lr, float lf, int every) {
  return lr >= 0.f && lr <= 3.0e38f && lf >= 0.f && lf <= 3.0e38f && every >= 1;
}

static bool cr_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + nb && pb < pa + na;
}

}  // namespace srgan

using namespace srgan;

extern "C" int srgan_cr_pairs_fwd(const float* x0, int n0, const float* x1, int n1, const float* table, float* y, int c, int h, int w,
                                  int flags, void* stream) {
  SRGAN_REQUIRE(c == 3, "cr_pairs_fwd: C = %d (three-channel images only)", c);
  SRGAN_REQUIRE(x0 && table && y && (x1 != nullptr) == (n1 > 0), "cr_pairs_fwd: null pointer (x1 is NULL exactly when n1 is 0)");
  SRGAN_REQUIRE((flags & ~CR_ALL) == 0, "cr_pairs_fwd: flags = %d (flip 1, translation 2)", flags);
  SRGAN_REQUIRE(n0 > 0 && n1 >= 0 && h > 0 && w > 0 && 3LL * h * w < (1LL << 31) - kCrItem && (long long)n0 + n1 < (1 << 29),
                "cr_pairs_fwd: n0 = %d, n1 = %d, H = %d, W = %d (n0, H, W > 0, n1 >= 0, 3 H W < 2^31, n0 + n1 < 2^29)", n0, n1, h, w);
  const int n = n0 + n1;
  const size_t E = (size_t)3 * h * w;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(x1) | reinterpret_cast<uintptr_t>(y);
  SRGAN_REQUIRE(((bits | reinterpret_cast<uintptr_t>(table)) & 3) == 0, "cr_pairs_fwd: pointer not 4-byte aligned");
  SRGAN_REQUIRE(!cr_overlap(y, 2 * n * E * sizeof(float), x0, n0 * E * sizeof(float)) &&
                    !(x1 && cr_overlap(y, 2 * n * E * sizeof(float), x1, n1 * E * sizeof(float))),
                "cr_pairs_fwd: the result must not alias a source");
  const int nitem = (int)ceil_div((long long)E, kCrItem);
  const long long items = 2LL * n * nitem;
  const int vec = (bits & 15) == 0 && (3LL * w) % 4 == 0;
  hipStream_t st = as_stream(stream);
  ProfScope scope(PROF_CR_PAIRS, 0.0, st);
  hipLaunchKernelGGL(cr_pairs_kernel, dim3((unsigned)std::min<long long>(items, kCrGridCap)), dim3(256), 0, st, x0, n0, x1, n, table, y,
                     h, w, flags, nitem, items, vec);
  return check_launch("cr_pairs_kernel");
}

extern "C" size_t srgan_cr_state_bytes(void) { return sizeof(srgan::CrState); }

extern "C" int srgan_cr_state_init(void* state, float lambda_real, float lambda_fake, int every, void* stream) {
  SRGAN_REQUIRE(state && cr_weights_ok(lambda_real, lambda_fake, every),
                "cr_state_init: bad argument (a record; weights >= 0 and finite, every >= 1; NaN refused)");
  CrState s = {};                        // the two terms and the counter at zero
  s.lambda_real = lambda_real; s.lambda_fake = lambda_fake; s.every = every;
  return record_write(state, &s, sizeof s, record_all_words<CrState>(), as_stream(stream), "cr_state_init");
}

extern "C" int srgan_cr_state_set(void* state, float lambda_real, float lambda_fake, int every, void* stream) {
  SRGAN_REQUIRE(state && cr_weights_ok(lambda_real, lambda_fake, every),
                "cr_state_set: bad argument (a record; weights >= 0 and finite, every >= 1; NaN refused)");
  CrState s = {};
  s.lambda_real = lambda_real; s.lambda_fake = lambda_fake; s.every = every;
  return record_write(state, &s, sizeof s, kCrSet, as_stream(stream), "cr_state_set");
}

extern "C" int srgan_cr_state_set_updates(void* state, int updates, void* stream) {
  SRGAN_REQUIRE(state && updates >= 0, "cr_state_set_updates: bad argument (a record; updates >= 0)");
  CrState s = {};                        // resume: everything else stays
  s.updates = updates;
  return record_write(state, &s, sizeof s, kCrSetUpdates, as_stream(stream), "cr_state_set_updates");
}

extern "C" int srgan_d_losses_cr(const float* const* o, const long long* per_row, const float* const* z, int n_scales, int rows,
                                 int rows_first, int n_class, const long long* label, float t_first, float t_rest, float w_class,
                                 int gan_kind, int class_kind, float* vals, float* const* d_o, float* const* dz, int pairs,
                                 int pairs_first, void* state, void* stream) {
  SRGAN_REQUIRE(o && per_row && d_o && vals && state, "d_losses_cr: null pointer");
  SRGAN_REQUIRE(n_scales >= 1 && n_scales <= 4, "d_losses_cr: %d scales (1..4)", n_scales);
  SRGAN_REQUIRE((gan_kind == SRGAN_CRIT_MSE || gan_kind == SRGAN_CRIT_BCE) && (class_kind == SRGAN_CRIT_MSE || class_kind == SRGAN_CRIT_BCE),
                "d_losses_cr: gan_kind / class_kind are 0 (MSE) or 1 (BCE)");
  SRGAN_REQUIRE(pairs >= 1 && pairs <= SRGAN_CR_MAX_PAIRS, "d_losses_cr: pairs = %d (1..%d: the row means are staged in LDS)", pairs,
                SRGAN_CR_MAX_PAIRS);
  SRGAN_REQUIRE(rows == 2 * pairs, "d_losses_cr: rows = %d, the maps hold 2 * pairs = %d rows", rows, 2 * pairs);
  SRGAN_REQUIRE(pairs_first >= 0 && pairs_first <= pairs, "d_losses_cr: pairs_first = %d outside [0, pairs = %d]", pairs_first, pairs);
  SRGAN_REQUIRE(rows_first >= 0 && rows_first <= pairs, "d_losses_cr: bad row split (rows_first = %d outside [0, pairs = %d])", rows_first,
                pairs);
  CrLossParams p{};
  p.n_scales = n_scales; p.pairs = pairs; p.pairs_first = pairs_first; p.rows_first = rows_first; p.nc = n_class;
  p.t_first = t_first; p.t_rest = t_rest; p.w_class = w_class; p.label = label; p.vals = vals;
  p.st = static_cast<CrState*>(state);
  for (int s = 0; s < n_scales; ++s) {
    SRGAN_REQUIRE(o[s] && d_o[s] && per_row[s] > 0, "d_losses_cr: null scale");
    SRGAN_REQUIRE(per_row[s] * rows < (1LL << 31), "d_losses_cr: map %d has %lld elements per row (rows * per_row < 2^31)", s, per_row[s]);
    p.o[s] = o[s]; p.d_o[s] = d_o[s]; p.per[s] = per_row[s];
    p.z[s] = z ? z[s] : nullptr;
    p.dz[s] = dz ? dz[s] : nullptr;
    SRGAN_REQUIRE(!p.z[s] || (p.dz[s] && label && rows_first > 0 && n_class > 0 && n_class <= 16),
                  "d_losses_cr: class head needs dz, labels, <= 16 classes");
  }
  hipStream_t st = as_stream(stream);
  ProfScope scope(PROF_D_LOSSES_CR, 0.0, st);
  if (gan_kind == SRGAN_CRIT_MSE && class_kind == SRGAN_CRIT_MSE)
    hipLaunchKernelGGL((d_losses_cr_kernel<CRIT_MSE, CRIT_MSE>), dim3(1), dim3(256), 0, st, p);
  else if (gan_kind == SRGAN_CRIT_MSE)
    hipLaunchKernelGGL((d_losses_cr_kernel<CRIT_MSE, CRIT_BCE>), dim3(1), dim3(256), 0, st, p);
  else if (class_kind == SRGAN_CRIT_MSE)
    hipLaunchKernelGGL((d_losses_cr_kernel<CRIT_BCE, CRIT_MSE>), dim3(1), dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL((d_losses_cr_kernel<CRIT_BCE, CRIT_BCE>), dim3(1), dim3(256), 0, st, p);
  return check_launch("d_losses_cr_kernel");
}
