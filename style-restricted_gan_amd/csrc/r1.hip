// R1 gradient penalty on real samples (Mescheder et al., 2018) for the two-scale discriminator: extension, no counterpart in the
// reference.  DESIGN.md section 7 ("R1 gradient penalty") has the formulas; srgan_amd/r1.py drives the convolution passes.
//
// The discriminator is piecewise linear in its input (bias-free convolutions, LeakyReLU, one bias conv per head, a 3x3 / stride-2
// average pool in front of the second scale), so the penalty's weight gradients need no double backward: an input-gradient chain
// per scale (h1 on the image, h2 on the pooled image), ONE pass of this file, a tangent forward and the weight-gradient kernels.
//
//   r1_seed_kernel      g = h1 + pool^T(h2), u0 = c * g, part[n][chunk] = sum g^2 over 4096 consecutive floats of sample n.
//                       fp32 NHWC, 3 channels.  pool = avg_pool2d(3, stride 2, padding 1, count_include_pad=False): pooled pixel
//                       (i2, j2) averages rows 2 i2 - 1 .. 2 i2 + 1 and columns 2 j2 - 1 .. 2 j2 + 1 that exist, so its divisor is
//                       rows(i2) * cols(j2) = 4, 6 or 9 (and 1, 2, 3 on one-pixel-wide images); an image pixel with an even
//                       coordinate is read by one pooled coordinate, with an odd one by two (the second only if it exists).
//                       Element e of a chunk belongs to thread (e / 4) % 256, slot (e / 1024) * 4 + e % 4, on the 16-byte and on
//                       the scalar path: 16 serial fused multiply-adds (g * g + acc, one rounding each, slot order), 6 butterfly
//                       levels over the wave, (w0 + w1) + (w2 + w3) over the four waves (grad_sumsq_partials_kernel's order).
//   r1_finalize_kernel  one workgroup: S = sum of the partials in double (thread t adds t, t + 256, ... ascending, then a fixed LDS
//                       tree), mean_sq_norm = S / N, penalty = gamma * every / 2 * S / N, updates += 1 into the device record.
//
// No atomics, plain global stores, every sum has one owner and an order that depends on H and W only: a sample's u0 and partials
// depend neither on N nor on its position in the batch nor on the grid.  fp contraction is off: both paths round alike.
#include "common.h"
#include "records.h"
#include <algorithm>
#include <cstdint>

#pragma clang fp contract(off)

namespace srgan {

constexpr int kR1Chunk = 4096;      // floats per partial sum
constexpr int kR1GridCap = 2048;    // 256 CUs x 8 workgroups; the rest by grid stride

// rows (or columns) of the image the pooled coordinate k averages: those of 2k - 1 .. 2k + 1 inside [0, len)
__device__ __forceinline__ int r1_span(int k, int len) { return min(2 * k + 1, len - 1) - max(2 * k - 1, 0) + 1; }

// pool^T(h2) at element e (channel-fastest) of one sample.  The up to four pooled pixels are added in a fixed order:
// ((first row: first column + second column) + (second row: first + second)).
__device__ __forceinline__ float r1_pool_t(const float* __restrict__ h2, int e, int H, int W, int H2, int W2) {
  const int p = e / 3, c = e - 3 * p;
  const int i = p / W, j = p - i * W;
  const int ia = i >> 1, ja = j >> 1;                       // even: the only reader; odd: the first of two
  const bool i2nd = (i & 1) && ia + 1 < H2, j2nd = (j & 1) && ja + 1 < W2;
  const float ca = (float)r1_span(ja, W), cb = (float)r1_span(ja + 1, W);
  const float* rowa = h2 + ((size_t)ia * W2 + ja) * 3 + c;
  float t = rowa[0] / ((float)r1_span(ia, H) * ca);
  if (j2nd) t = t + rowa[3] / ((float)r1_span(ia, H) * cb);
  if (i2nd) {
    const float* rowb = rowa + (size_t)W2 * 3;
    float t2 = rowb[0] / ((float)r1_span(ia + 1, H) * ca);
    if (j2nd) t2 = t2 + rowb[3] / ((float)r1_span(ia + 1, H) * cb);
    t = t + t2;
  }
  return t;
}

__global__ __launch_bounds__(256) void r1_seed_kernel(const float* __restrict__ h1, const float* __restrict__ h2,
                                                      const R1State* __restrict__ st, float* __restrict__ u0,
                                                      float* __restrict__ part, int H, int W, int H2, int W2, int nchunk,
                                                      long long items, int vec) {
  __shared__ float red[4];
  const int E = 3 * H * W, E2 = 3 * H2 * W2;
  const float cs = st->c;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int n = (int)(it / nchunk), chunk = (int)(it - (long long)n * nchunk);
    const float* a = h1 + (size_t)n * E;
    const float* b = h2 + (size_t)n * E2;
    float* dst = u0 + (size_t)n * E;
    float acc = 0.f;
#pragma unroll
    for (int jv = 0; jv < 4; ++jv) {
      const int e0 = chunk * kR1Chunk + (jv * 256 + (int)threadIdx.x) * 4;
      if (e0 >= E) continue;
      f32x4 g = {0.f, 0.f, 0.f, 0.f};
      if (vec) {                                            // E % 4 == 0 and 16-byte aligned bases: the four elements exist
        const f32x4 v = *reinterpret_cast<const f32x4*>(a + e0);
#pragma unroll
        for (int q = 0; q < 4; ++q) g[q] = v[q] + r1_pool_t(b, e0 + q, H, W, H2, W2);
        f32x4 u;
#pragma unroll
        for (int q = 0; q < 4; ++q) u[q] = cs * g[q];
        *reinterpret_cast<f32x4*>(dst + e0) = u;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (e0 + q < E) {
            g[q] = a[e0 + q] + r1_pool_t(b, e0 + q, H, W, H2, W2);
            dst[e0 + q] = cs * g[q];
          }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = __builtin_fmaf(g[q], g[q], acc);     // a missing element adds +0: acc unchanged
    }
    acc = wave_sum(acc);
    __syncthreads();                                        // the previous item's reads of red[]
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[it] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

__global__ __launch_bounds__(256) void r1_finalize_kernel(const float* __restrict__ part, long long items, int n,
                                                          R1State* __restrict__ s) {
  __shared__ double red[256];
  double acc = 0.0;
  for (long long i = threadIdx.x; i < items; i += 256) acc += (double)part[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double m = red[0] / (double)n;
    s->mean_sq_norm = (float)m;
    s->penalty = (float)(0.5 * (double)s->gamma * (double)s->every_scale * m);
    s->updates += 1;
  }
}

// The settings of a record (R1State, records.h) with c = gamma * every / n: one fp32 multiply, one fp32 divide, each rounded once
// (contraction is off in this file and there is nothing to contract); the rest at zero.
static R1State r1_settings(float gamma, int every, int n) {
  R1State s = {};
  s.gamma = gamma; s.every_scale = every; s.c = gamma * (float)every / (float)n; s.n = n;
  return s;
}

static long long r1_chunks(int h, int w) { return ceil_div(3LL * h * w, kR1Chunk); }
static bool r1_geometry_ok(int n, int h, int w) {
  return n > 0 && h > 0 && w > 0 && 3LL * h * w < (1LL << 31) - kR1Chunk && (long long)n * r1_chunks(h, w) < (1LL << 40);
}

}  // namespace srgan

using namespace srgan;

extern "C" size_t srgan_r1_state_bytes(void) { return sizeof(srgan::R1State); }

extern "C" int srgan_r1_state_init(void* state, float gamma, int every, int n, void* stream) {
  SRGAN_REQUIRE(state && gamma >= 0.f && gamma <= 3.0e38f && every >= 1 && n >= 1,
                "r1_state_init: bad argument (gamma >= 0 and finite, every >= 1, n >= 1; NaN refused)");
  const srgan::R1State s = srgan::r1_settings(gamma, every, n);
  return srgan::record_write(state, &s, sizeof s, srgan::record_all_words<srgan::R1State>(), as_stream(stream), "r1_state_init");
}

extern "C" int srgan_r1_state_set(void* state, float gamma, int every, int n, void* stream) {
  SRGAN_REQUIRE(state && gamma >= 0.f && gamma <= 3.0e38f && every >= 1 && n >= 1,
                "r1_state_set: bad argument (gamma >= 0 and finite, every >= 1, n >= 1; NaN refused)");
  const srgan::R1State s = srgan::r1_settings(gamma, every, n);
  return srgan::record_write(state, &s, sizeof s, srgan::kR1Set, as_stream(stream), "r1_state_set");
}

extern "C" int srgan_r1_state_set_updates(void* state, int updates, void* stream) {
  SRGAN_REQUIRE(state && updates >= 0, "r1_state_set_updates: bad argument (updates >= 0)");
  srgan::R1State s = {};                 // resume: everything else stays
  s.updates = updates;
  return srgan::record_write(state, &s, sizeof s, srgan::kR1SetUpdates, as_stream(stream), "r1_state_set_updates");
}

extern "C" size_t srgan_r1_workspace(int n, int h, int w) {
  if (!srgan::r1_geometry_ok(n, h, w)) {
    srgan::set_error("r1_workspace: bad argument (n, h, w > 0, 3 h w < 2^31)");
    return 0;
  }
  return (size_t)((long long)n * srgan::r1_chunks(h, w)) * sizeof(float);
}

extern "C" int srgan_r1_seed(const float* h1, const float* h2, const void* state, float* u0, int n, int c, int h, int w, void* ws,
                             size_t ws_bytes, void* stream) {
  SRGAN_REQUIRE(c == 3, "r1_seed: C = %d, the input-gradient images have 3 channels", c);
  SRGAN_REQUIRE(h1 && h2 && state && u0 && ws, "r1_seed: null pointer");
  SRGAN_REQUIRE(srgan::r1_geometry_ok(n, h, w), "r1_seed: bad geometry (n, h, w > 0, 3 h w < 2^31)");
  const long long nchunk = srgan::r1_chunks(h, w), items = (long long)n * nchunk;
  SRGAN_REQUIRE(ws_bytes >= (size_t)items * sizeof(float), "r1_seed: workspace of %zu bytes, %zu needed (srgan_r1_workspace)", ws_bytes,
                (size_t)items * sizeof(float));
  SRGAN_REQUIRE(((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(h1) | reinterpret_cast<uintptr_t>(h2) |
                  reinterpret_cast<uintptr_t>(u0)) & 3) == 0, "r1_seed: pointer not 4-byte aligned");
  SRGAN_REQUIRE(h1 != u0 && h2 != u0, "r1_seed: u0 must not alias h1 / h2 (neighbouring pixels read h2 after u0 is written)");
  const int vec = ((3LL * h * w) % 4 == 0 && ((reinterpret_cast<uintptr_t>(h1) | reinterpret_cast<uintptr_t>(u0)) & 15) == 0) ? 1 : 0;
  const unsigned bx = (unsigned)std::min<long long>(items, srgan::kR1GridCap);
  hipLaunchKernelGGL(srgan::r1_seed_kernel, dim3(bx), dim3(256), 0, as_stream(stream), h1, h2,
                     static_cast<const srgan::R1State*>(state), u0, static_cast<float*>(ws), h, w, (h - 1) / 2 + 1, (w - 1) / 2 + 1,
                     (int)nchunk, items, vec);
  return check_launch("r1_seed_kernel");
}

extern "C" int srgan_r1_finalize(const void* ws, size_t ws_bytes, int n, int h, int w, void* state, void* stream) {
  SRGAN_REQUIRE(ws && state, "r1_finalize: null pointer");
  SRGAN_REQUIRE(srgan::r1_geometry_ok(n, h, w), "r1_finalize: bad geometry (n, h, w > 0, 3 h w < 2^31)");
  const long long items = (long long)n * srgan::r1_chunks(h, w);
  SRGAN_REQUIRE(ws_bytes >= (size_t)items * sizeof(float), "r1_finalize: workspace of %zu bytes, %zu needed (srgan_r1_workspace)",
                ws_bytes, (size_t)items * sizeof(float));
  hipLaunchKernelGGL(srgan::r1_finalize_kernel, dim3(1), dim3(256), 0, as_stream(stream), static_cast<const float*>(ws), items, n,
                     static_cast<srgan::R1State*>(state));
  return check_launch("r1_finalize_kernel");
}
