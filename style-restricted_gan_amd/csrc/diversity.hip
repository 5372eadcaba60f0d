// Mode-seeking (diversity) regularisation of the generator: the ratio term of MSGAN (Mao et al., CVPR 2019) and its per-sample,
// clamped form of DSGAN (Yang et al., ICLR 2019).  Extension, no counterpart in the reference.  DESIGN.md section 7 ("Mode-seeking
// regularisation") has the formulas; srgan_amd/diversity.py owns the record.
//
// Two translations I1, I2 [B, E] (E = C H W, fp32, NHWC-dense rows: the generator's tanh writes fp32 in every compute mode) of the
// same sources under two latent codes z1, z2 [B, d].  s_i = sum |I1_i - I2_i|, t_i = sum |z1_i - z2_i|.
//
//   ms_rows_kernel    item (row n, chunk c) = kMsChunk consecutive floats of row n -> part[n * nchunk + c] = their sum of
//                     |a - b| in fp32.  Element e of a chunk belongs to thread (e / 4) % 256, slot (e / 1024) * 4 + e % 4: 16 serial
//                     adds in slot order, 6 butterfly levels over the wave, (w0 + w1) + (w2 + w3) over the four waves.  16-byte loads
//                     where both row bases are 16-byte aligned (decided per item: a row slice of a larger batch with odd E is 4-byte
//                     aligned only), else 4-byte loads; the same element -> thread / slot map, so the same bits.  One index division
//                     per ITEM, none per element.
//   ms_finish_kernel  one workgroup, everything in double: s_i = the row's partials in ascending order, t_i = |z1 - z2| over d in
//                     ascending order (thread r % 256 owns row r), the batch sums by thread-ascending accumulation and a fixed LDS
//                     tree; ms, weight * ms, dI, dz and updates += 1 into the record, {weight * ms, ms} into vals, the per-row
//                     gradient coefficient (weight included) into coef[B].  weight, eps, tau are READ from the record.
//   ms_grad_kernel    the same items: dI1 = g * coef[n] * sign(a - b), dI2 = -dI1 (either may be absent: nothing is written for
//                     it), sign(0) = 0, g the incoming gradient read from device memory.
//
// No atomics, plain stores, every sum has one owner and an order that depends on E, d and B only -- not on the grid.
#include "common.h"
#include "prof.h"
#include "records.h"
#include <algorithm>
#include <cstdint>

#pragma clang fp contract(off)

namespace srgan {

constexpr int kMsBlock = 256;       // threads per workgroup
constexpr int kMsChunk = 4096;      // floats of ONE row per workgroup item: a row of more than this spans several items
constexpr int kMsRowsPerItem = 1;   // an item never holds more than one row
constexpr int kMsGridCap = 2048;    // 256 CUs x 8 workgroups; the rest by grid stride
static_assert(kMsRowsPerItem == 1 && kMsChunk == 16 * kMsBlock, "16 elements per thread and item, one row per item");

__device__ __forceinline__ bool ms_aligned16(const float* a, const float* b) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}

__global__ __launch_bounds__(256) void ms_rows_kernel(const float* __restrict__ i1, const float* __restrict__ i2,
                                                      float* __restrict__ part, int E, int nchunk, long long items) {
  __shared__ float red[4];
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int n = (int)(it / nchunk), chunk = (int)(it - (long long)n * nchunk);
    const float* a = i1 + (size_t)n * E;
    const float* b = i2 + (size_t)n * E;
    const bool vec = ms_aligned16(a, b);                    // uniform over the workgroup
    float acc = 0.f;
#pragma unroll
    for (int jv = 0; jv < 4; ++jv) {
      const int e0 = chunk * kMsChunk + (jv * kMsBlock + (int)threadIdx.x) * 4;
      if (e0 >= E) continue;
      f32x4 dlt = {0.f, 0.f, 0.f, 0.f};
      if (vec && e0 + 4 <= E) {
        const f32x4 va = *reinterpret_cast<const f32x4*>(a + e0);
        const f32x4 vb = *reinterpret_cast<const f32x4*>(b + e0);
#pragma unroll
        for (int q = 0; q < 4; ++q) dlt[q] = __builtin_fabsf(va[q] - vb[q]);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (e0 + q < E) dlt[q] = __builtin_fabsf(a[e0 + q] - b[e0 + q]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = acc + dlt[q];       // a missing element adds +0: acc unchanged
    }
    acc = wave_sum(acc);
    __syncthreads();                                        // the previous item's reads of red[]
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[it] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// a fixed tree over the 256 threads' values; every thread gets the sum
__device__ __forceinline__ double ms_block_sum(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = kMsBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(256) void ms_finish_kernel(const float* __restrict__ part, const float* __restrict__ z1,
                                                        const float* __restrict__ z2, double* __restrict__ rows, int B, int E,
                                                        int d, int nchunk, int form, MsState* __restrict__ st,
                                                        float* __restrict__ vals, float* __restrict__ coef) {
  __shared__ double red[kMsBlock];
  const double weight = (double)st->weight, eps = (double)st->eps, tau = (double)st->tau;
  double* srow = rows;
  double* trow = rows + B;
  double accs = 0.0, acct = 0.0;
  for (int r = threadIdx.x; r < B; r += kMsBlock) {
    double s = 0.0, t = 0.0;
    for (int c = 0; c < nchunk; ++c) s += (double)part[(size_t)r * nchunk + c];
    for (int k = 0; k < d; ++k) t += (double)__builtin_fabsf(z1[(size_t)r * d + k] - z2[(size_t)r * d + k]);
    srow[r] = s; trow[r] = t;                               // read back by the thread that wrote them
    accs += s; acct += t;
  }
  const double S = ms_block_sum(accs, red);
  const double T = ms_block_sum(acct, red);
  const double dI = S / ((double)B * (double)E), dz = T / ((double)B * (double)d);
  double ms;
  if (form == 0) {                                          // msgan
    const double den = dI + eps * dz;
    ms = dz == 0.0 ? 0.0 : dz / den;
    const double cf = dz == 0.0 ? 0.0 : -weight * dz / (den * den) / ((double)B * (double)E);
    for (int r = threadIdx.x; r < B; r += kMsBlock) coef[r] = (float)cf;
  } else {                                                  // dsgan
    double acc = 0.0;
    for (int r = threadIdx.x; r < B; r += kMsBlock) {
      const double s = srow[r], t = trow[r];
      double term = tau, cf = 0.0;
      if (t != 0.0) {
        const double ri = (s / (double)E) / (t / (double)d);
        if (ri <= tau) {                                    // torch.clamp's mask: <=
          term = ri;
          cf = -weight / (double)B * ((double)d / t) / (double)E;
        }
      }
      acc += term;
      coef[r] = (float)cf;
    }
    ms = -ms_block_sum(acc, red) / (double)B;
  }
  if (threadIdx.x == 0) {
    st->ms = (float)ms; st->weighted = (float)(weight * ms); st->d_image = (float)dI; st->d_latent = (float)dz;
    st->updates += 1;
    vals[0] = (float)(weight * ms);
    vals[1] = (float)ms;
  }
}

__device__ __forceinline__ float ms_sign(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

__global__ __launch_bounds__(256) void ms_grad_kernel(const float* __restrict__ i1, const float* __restrict__ i2,
                                                      const float* __restrict__ coef, const float* __restrict__ gin,
                                                      float* __restrict__ d1, float* __restrict__ d2, int E, int nchunk,
                                                      long long items) {
  const float g = *gin;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int n = (int)(it / nchunk), chunk = (int)(it - (long long)n * nchunk);
    const float* a = i1 + (size_t)n * E;
    const float* b = i2 + (size_t)n * E;
    float* o1 = d1 ? d1 + (size_t)n * E : nullptr;
    float* o2 = d2 ? d2 + (size_t)n * E : nullptr;
    const float c = g * coef[n];
    const bool vin = ms_aligned16(a, b);
    const bool v1 = o1 && (reinterpret_cast<uintptr_t>(o1) & 15) == 0, v2 = o2 && (reinterpret_cast<uintptr_t>(o2) & 15) == 0;
#pragma unroll
    for (int jv = 0; jv < 4; ++jv) {
      const int e0 = chunk * kMsChunk + (jv * kMsBlock + (int)threadIdx.x) * 4;
      if (e0 >= E) continue;
      const bool full = e0 + 4 <= E;
      f32x4 r = {0.f, 0.f, 0.f, 0.f};
      if (vin && full) {
        const f32x4 va = *reinterpret_cast<const f32x4*>(a + e0);
        const f32x4 vb = *reinterpret_cast<const f32x4*>(b + e0);
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = c * ms_sign(va[q] - vb[q]);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (e0 + q < E) r[q] = c * ms_sign(a[e0 + q] - b[e0 + q]);
      }
      if (o1) {
        if (v1 && full) {
          *reinterpret_cast<f32x4*>(o1 + e0) = r;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (e0 + q < E) o1[e0 + q] = r[q];
        }
      }
      if (o2) {
        if (v2 && full) {
          *reinterpret_cast<f32x4*>(o2 + e0) = -r;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (e0 + q < E) o2[e0 + q] = -r[q];
        }
      }
    }
  }
}

static long long ms_chunks(long long e) { return ceil_div(e, kMsChunk); }
static bool ms_geometry_ok(int b, long long e) {
  return b > 0 && e > 0 && e < (1LL << 31) - kMsChunk && (long long)b * ms_chunks(e) < (1LL << 40);
}
static size_t ms_part_bytes(int b, long long e) { return (size_t)round_up((long long)b * ms_chunks(e) * (long long)sizeof(float), 8); }
static bool ms_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace srgan

using namespace srgan;

extern "C" size_t srgan_ms_state_bytes(void) { return sizeof(srgan::MsState); }

static bool ms_settings_ok(float weight, float eps, float tau) {
  return weight >= 0.f && weight <= 3.0e38f && eps > 0.f && eps <= 3.0e38f && tau >= 0.f && tau <= 3.0e38f;
}

extern "C" int srgan_ms_state_init(void* state, float weight, float eps, float tau, void* stream) {
  SRGAN_REQUIRE(state && ms_settings_ok(weight, eps, tau),
                "ms_state_init: bad argument (weight >= 0, eps > 0, tau >= 0, all finite; NaN refused)");
  srgan::MsState s = {};                 // the last values and the counter at zero
  s.weight = weight; s.eps = eps; s.tau = tau;
  return srgan::record_write(state, &s, sizeof s, srgan::record_all_words<srgan::MsState>(), as_stream(stream), "ms_state_init");
}

extern "C" int srgan_ms_state_set(void* state, float weight, float eps, float tau, void* stream) {
  SRGAN_REQUIRE(state && ms_settings_ok(weight, eps, tau),
                "ms_state_set: bad argument (weight >= 0, eps > 0, tau >= 0, all finite; NaN refused)");
  srgan::MsState s = {};
  s.weight = weight; s.eps = eps; s.tau = tau;
  return srgan::record_write(state, &s, sizeof s, srgan::kMsSet, as_stream(stream), "ms_state_set");
}

extern "C" int srgan_ms_state_restore(void* state, int updates, float ms, float d_image, float d_latent, void* stream) {
  SRGAN_REQUIRE(state && updates >= 0, "ms_state_restore: bad argument (updates >= 0)");
  srgan::MsState s = {};                 // resume: the settings stay, and `weighted` until the next ms_finish
  s.updates = updates; s.ms = ms; s.d_image = d_image; s.d_latent = d_latent;
  return srgan::record_write(state, &s, sizeof s, srgan::kMsRestore, as_stream(stream), "ms_state_restore");
}

extern "C" size_t srgan_ms_workspace(int b, long long e) {
  if (!srgan::ms_geometry_ok(b, e)) {
    srgan::set_error("ms_workspace: bad argument (b, e > 0, e < 2^31)");
    return 0;
  }
  return srgan::ms_part_bytes(b, e) + 2 * (size_t)b * sizeof(double);
}

extern "C" int srgan_ms_rows(const float* i1, const float* i2, int b, long long e, void* ws, size_t ws_bytes, void* stream) {
  SRGAN_REQUIRE(i1 && i2 && ws, "ms_rows: null pointer");
  SRGAN_REQUIRE(srgan::ms_geometry_ok(b, e), "ms_rows: bad geometry (b, e > 0, e < 2^31)");
  SRGAN_REQUIRE(ws_bytes >= srgan::ms_part_bytes(b, e), "ms_rows: workspace of %zu bytes, %zu needed (srgan_ms_workspace)", ws_bytes,
                srgan::ms_part_bytes(b, e));
  SRGAN_REQUIRE(srgan::ms_aligned4(i1) && srgan::ms_aligned4(i2) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
                "ms_rows: images not 4-byte aligned or workspace not 8-byte aligned");
  const long long nchunk = srgan::ms_chunks(e), items = (long long)b * nchunk;
  const unsigned bx = (unsigned)std::min<long long>(items, srgan::kMsGridCap);
  hipStream_t st = as_stream(stream);
  ProfScope scope(PROF_MS_ROWS, 8.0 * (double)b * (double)e, st);
  hipLaunchKernelGGL(srgan::ms_rows_kernel, dim3(bx), dim3(srgan::kMsBlock), 0, st, i1, i2, static_cast<float*>(ws), (int)e,
                     (int)nchunk, items);
  return check_launch("ms_rows_kernel");
}

extern "C" int srgan_ms_finish(const void* ws, size_t ws_bytes, const float* z1, const float* z2, int b, long long e, int d, int form,
                               void* state, float* vals, float* coef, void* stream) {
  SRGAN_REQUIRE(ws && z1 && z2 && state && vals && coef, "ms_finish: null pointer");
  SRGAN_REQUIRE(srgan::ms_geometry_ok(b, e) && d > 0, "ms_finish: bad geometry (b, e, d > 0, e < 2^31)");
  SRGAN_REQUIRE(form == 0 || form == 1, "ms_finish: form = %d (0 msgan, 1 dsgan)", form);
  const size_t need = srgan::ms_part_bytes(b, e) + 2 * (size_t)b * sizeof(double);
  SRGAN_REQUIRE(ws_bytes >= need, "ms_finish: workspace of %zu bytes, %zu needed (srgan_ms_workspace)", ws_bytes, need);
  SRGAN_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0 && srgan::ms_aligned4(z1) && srgan::ms_aligned4(z2) &&
                    srgan::ms_aligned4(vals) && srgan::ms_aligned4(coef),
                "ms_finish: workspace not 8-byte aligned or a pointer not 4-byte aligned");
  const char* base = static_cast<const char*>(ws);
  double* rows = reinterpret_cast<double*>(const_cast<char*>(base) + srgan::ms_part_bytes(b, e));
  hipStream_t st = as_stream(stream);
  ProfScope scope(PROF_MS_FINISH, 0.0, st);
  hipLaunchKernelGGL(srgan::ms_finish_kernel, dim3(1), dim3(srgan::kMsBlock), 0, st, reinterpret_cast<const float*>(base), z1, z2,
                     rows, b, (int)e, d, (int)srgan::ms_chunks(e), form, static_cast<srgan::MsState*>(state), vals, coef);
  return check_launch("ms_finish_kernel");
}

extern "C" int srgan_ms_grad(const float* i1, const float* i2, const float* coef, const float* g, float* d1, float* d2, int b,
                             long long e, void* stream) {
  SRGAN_REQUIRE(i1 && i2 && coef && g && (d1 || d2), "ms_grad: null pointer (one of d1 / d2 may be NULL, not both)");
  SRGAN_REQUIRE(srgan::ms_geometry_ok(b, e), "ms_grad: bad geometry (b, e > 0, e < 2^31)");
  SRGAN_REQUIRE(srgan::ms_aligned4(i1) && srgan::ms_aligned4(i2) && srgan::ms_aligned4(coef) && srgan::ms_aligned4(g) &&
                    srgan::ms_aligned4(d1) && srgan::ms_aligned4(d2), "ms_grad: pointer not 4-byte aligned");
  SRGAN_REQUIRE(d1 != i1 && d1 != i2 && d2 != i1 && d2 != i2 && (d1 != d2), "ms_grad: an output aliases an input or the other output");
  const long long nchunk = srgan::ms_chunks(e), items = (long long)b * nchunk;
  const unsigned bx = (unsigned)std::min<long long>(items, srgan::kMsGridCap);
  hipStream_t st = as_stream(stream);
  ProfScope scope(PROF_MS_GRAD, 4.0 * (double)b * (double)e * (2.0 + (d1 ? 1.0 : 0.0) + (d2 ? 1.0 : 0.0)), st);
  hipLaunchKernelGGL(srgan::ms_grad_kernel, dim3(bx), dim3(srgan::kMsBlock), 0, st, i1, i2, coef, g, d1, d2, (int)e, (int)nchunk,
                     items);
  return check_launch("ms_grad_kernel");
}
