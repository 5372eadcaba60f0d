// Small HBM-bound kernels of the train step: activations, pools, layout repacks, Linear heads,
// fused Adam.  NHWC fp32.  Reference call sites are listed in include/srgan_hip.h.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include "common.h"
#include "records.h"

namespace srgan {

static inline unsigned grid_for(long long n, int per_thread = 1) {
  long long b = ceil_div(ceil_div(n, per_thread), 256);
  return (unsigned)std::max<long long>(1, std::min<long long>(b, 8192));
}

#define GRID_STRIDE(i, n) \
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)

__global__ void act_fwd_kernel(const float* x, float* y, long long n, int act, float slope) {
  GRID_STRIDE(i, n) y[i] = apply_act(x[i], act, slope);
}
__global__ void act_bwd_kernel(const float* y, const float* dy, float* dx, long long n, int act, float slope) {
  GRID_STRIDE(i, n) dx[i] = dy[i] * act_grad(y[i], act, slope);
}
// 16-bit I/O (round 6: the discriminator trunks' bf16 activations): 8 elements per thread, any mix of fp32 / bf16 tensors
template <bool Y16, bool D16, bool X16>
__global__ __launch_bounds__(256) void act_bwd_io_kernel(const void* y, const void* dy, void* dx, long long n8, int act, float slope) {
  const float neg = act_neg_slope(act, slope);
  GRID_STRIDE(i, n8) {
    float yv[8], dv[8];
    if constexpr (Y16) {
      const bf16x8 t = reinterpret_cast<const bf16x8*>(y)[i];
#pragma unroll
      for (int e = 0; e < 8; ++e) yv[e] = (float)t[e];
    } else {
      const f32x4 a = reinterpret_cast<const f32x4*>(y)[2 * i], b = reinterpret_cast<const f32x4*>(y)[2 * i + 1];
#pragma unroll
      for (int e = 0; e < 4; ++e) { yv[e] = a[e]; yv[4 + e] = b[e]; }
    }
    if constexpr (D16) {
      const bf16x8 t = reinterpret_cast<const bf16x8*>(dy)[i];
#pragma unroll
      for (int e = 0; e < 8; ++e) dv[e] = (float)t[e];
    } else {
      const f32x4 a = reinterpret_cast<const f32x4*>(dy)[2 * i], b = reinterpret_cast<const f32x4*>(dy)[2 * i + 1];
#pragma unroll
      for (int e = 0; e < 4; ++e) { dv[e] = a[e]; dv[4 + e] = b[e]; }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) dv[e] = dv[e] * (yv[e] > 0.f ? 1.f : neg);
    if constexpr (X16) {
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (__bf16)dv[e];
      reinterpret_cast<bf16x8*>(dx)[i] = o;
    } else {
      reinterpret_cast<f32x4*>(dx)[2 * i] = f32x4{dv[0], dv[1], dv[2], dv[3]};
      reinterpret_cast<f32x4*>(dx)[2 * i + 1] = f32x4{dv[4], dv[5], dv[6], dv[7]};
    }
  }
}
__global__ void tanh_fwd_kernel(const float* x, float* y, long long n) {
  GRID_STRIDE(i, n) y[i] = tanhf(x[i]);
}
__global__ void tanh_bwd_kernel(const float* y, const float* dy, float* dx, long long n) {
  GRID_STRIDE(i, n) { const float t = y[i]; dx[i] = dy[i] * (1.f - t * t); }
}
__global__ void add_kernel(const float* a, const float* b, float* y, long long n) {
  GRID_STRIDE(i, n) y[i] = a[i] + b[i];
}

// AvgPool2d(3, s2, p1, count_include_pad=False): Ho = (H+2-3)/2+1
__global__ void avgpool3s2_fwd_kernel(const float* x, float* y, int N, int H, int W, int C, int Ho, int Wo) {
  const long long total = (long long)N * Ho * Wo * C;
  GRID_STRIDE(i, total) {
    const int c = (int)(i % C);
    long long r = i / C;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int n = (int)(r / Ho);
    float s = 0.f;
    int cnt = 0;
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = oy * 2 + dy;
      if ((unsigned)yy >= (unsigned)H) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        const int xx = ox * 2 + dx;
        if ((unsigned)xx >= (unsigned)W) continue;
        s += x[((size_t)(n * H + yy) * W + xx) * C + c];
        ++cnt;
      }
    }
    y[i] = s / (float)cnt;
  }
}
__device__ __forceinline__ int valid3(int o, int L) {  // taps of window o that fall inside [0,L)
  int c = 0;
  for (int d = -1; d <= 1; ++d) c += ((unsigned)(o * 2 + d) < (unsigned)L);
  return c;
}
__global__ void avgpool3s2_bwd_kernel(const float* dy, float* dx, int N, int H, int W, int C, int Ho, int Wo) {
  const long long total = (long long)N * H * W * C;
  GRID_STRIDE(i, total) {
    const int c = (int)(i % C);
    long long r = i / C;
    const int x = (int)(r % W); r /= W;
    const int y = (int)(r % H);
    const int n = (int)(r / H);
    float s = 0.f;
    // windows oy with |2*oy - y| <= 1
    for (int oy = (y - 1 + 1) / 2 - 1; oy <= (y + 1) / 2; ++oy) {
      if (oy < 0 || oy >= Ho || abs(2 * oy - y) > 1) continue;
      const int cy = valid3(oy, H);
      for (int ox = (x - 1 + 1) / 2 - 1; ox <= (x + 1) / 2; ++ox) {
        if (ox < 0 || ox >= Wo || abs(2 * ox - x) > 1) continue;
        const int cx = valid3(ox, W);
        s += dy[((size_t)(n * Ho + oy) * Wo + ox) * C + c] / (float)(cy * cx);
      }
    }
    dx[i] = s;
  }
}

__global__ void avgpool2_fwd_kernel(const float* x, float* y, int N, int H, int W, int C, int Ho, int Wo) {
  const long long total = (long long)N * Ho * Wo * C;
  GRID_STRIDE(i, total) {
    const int c = (int)(i % C);
    long long r = i / C;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int n = (int)(r / Ho);
    const size_t b = ((size_t)(n * H + oy * 2) * W + ox * 2) * C + c;
    y[i] = 0.25f * (x[b] + x[b + C] + x[b + (size_t)W * C] + x[b + (size_t)W * C + C]);
  }
}
__global__ void avgpool2_bwd_kernel(const float* dy, float* dx, int N, int H, int W, int C, int Ho, int Wo) {
  const long long total = (long long)N * H * W * C;
  GRID_STRIDE(i, total) {
    const int c = (int)(i % C);
    long long r = i / C;
    const int x = (int)(r % W); r /= W;
    const int y = (int)(r % H);
    const int n = (int)(r / H);
    const int oy = y >> 1, ox = x >> 1;
    dx[i] = (oy < Ho && ox < Wo) ? 0.25f * dy[((size_t)(n * Ho + oy) * Wo + ox) * C + c] : 0.f;
  }
}

// AvgPool2d(2, 2) with an fp32 or bf16 tensor on either side (the bf16 mode's 16-bit activations around the style encoder's
// convolutions, pyfiles/model.py:409-411): 4 channels per thread (C % 4 == 0), the mean in fp32.
template <bool B16>
__device__ __forceinline__ f32x4 ld4_io(const void* base, size_t idx) {
  if constexpr (B16) return __builtin_convertvector(*reinterpret_cast<const bf16x4*>(static_cast<const __bf16*>(base) + idx), f32x4);
  else return *reinterpret_cast<const f32x4*>(static_cast<const float*>(base) + idx);
}
template <bool B16>
__device__ __forceinline__ void st4_io(void* base, size_t idx, f32x4 v) {
  if constexpr (B16) *reinterpret_cast<bf16x4*>(static_cast<__bf16*>(base) + idx) = __builtin_convertvector(v, bf16x4);
  else *reinterpret_cast<f32x4*>(static_cast<float*>(base) + idx) = v;
}
template <bool X16, bool Y16>
__global__ void avgpool2_fwd_io_kernel(const void* x, void* y, int N, int H, int W, int C, int Ho, int Wo) {
  const int C4 = C >> 2;
  const long long total = (long long)N * Ho * Wo * C4;
  GRID_STRIDE(i, total) {
    const int c = (int)(i % C4) * 4;
    long long r = i / C4;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int n = (int)(r / Ho);
    const size_t b = ((size_t)(n * H + oy * 2) * W + ox * 2) * C + c;
    const f32x4 v = 0.25f * (ld4_io<X16>(x, b) + ld4_io<X16>(x, b + C) + ld4_io<X16>(x, b + (size_t)W * C) +
                             ld4_io<X16>(x, b + (size_t)W * C + C));
    st4_io<Y16>(y, (size_t)i * 4, v);
  }
}
template <bool G16, bool D16>
__global__ void avgpool2_bwd_io_kernel(const void* dy, void* dx, int N, int H, int W, int C, int Ho, int Wo) {
  const int C4 = C >> 2;
  const long long total = (long long)N * H * W * C4;
  GRID_STRIDE(i, total) {
    const int c = (int)(i % C4) * 4;
    long long r = i / C4;
    const int x = (int)(r % W); r /= W;
    const int y = (int)(r % H);
    const int n = (int)(r / H);
    const int oy = y >> 1, ox = x >> 1;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (oy < Ho && ox < Wo) v = 0.25f * ld4_io<G16>(dy, ((size_t)(n * Ho + oy) * Wo + ox) * C + c);
    st4_io<D16>(dx, (size_t)i * 4, v);
  }
}

__global__ void lrelu_gap_fwd_kernel(const float* x, float* y, int N, int HW, int C, float slope) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N * C) return;
  const int n = idx / C, c = idx - n * C;
  float s = 0.f;
  for (int r = 0; r < HW; ++r) {
    const float v = x[((size_t)n * HW + r) * C + c];
    s += v > 0.f ? v : v * slope;
  }
  y[idx] = s / (float)HW;
}
__global__ void lrelu_gap_bwd_kernel(const float* x, const float* dy, float* dx, int N, int HW, int C, float slope) {
  const long long total = (long long)N * HW * C;
  const float inv = 1.f / (float)HW;
  GRID_STRIDE(i, total) {
    const int c = (int)(i % C);
    const int n = (int)(i / ((long long)HW * C));
    dx[i] = dy[n * C + c] * inv * (x[i] > 0.f ? 1.f : slope);
  }
}

// Linear heads: one wave per output element (M, N small; K = 1024)
__global__ void linear_fwd_kernel(const float* x, const float* W, const float* b, float* y, int M, int N, int K) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (wave >= M * N) return;
  const int m = wave / N, n = wave - m * N;
  float s = 0.f;
  for (int k = lane; k < K; k += 64) s += x[(size_t)m * K + k] * W[(size_t)n * K + k];
  s = wave_sum(s);
  if (lane == 0) y[wave] = s + (b ? b[n] : 0.f);
}
__global__ void linear_bwd_dx_kernel(const float* W, const float* dy, float* dx, int M, int N, int K) {
  const long long total = (long long)M * K;
  GRID_STRIDE(i, total) {
    const int k = (int)(i % K), m = (int)(i / K);
    float s = 0.f;
    for (int n = 0; n < N; ++n) s += dy[m * N + n] * W[(size_t)n * K + k];
    dx[i] = s;
  }
}
__global__ void linear_bwd_dw_kernel(const float* x, const float* dy, float* dW, float* db, int M, int N, int K) {
  const long long total = (long long)N * K;
  GRID_STRIDE(i, total) {
    const int k = (int)(i % K), n = (int)(i / K);
    float s = 0.f;
    for (int m = 0; m < M; ++m) s += dy[m * N + n] * x[(size_t)m * K + k];
    dW[i] = s;
    if (k == 0 && db) {
      float t = 0.f;
      for (int m = 0; m < M; ++m) t += dy[m * N + n];
      db[n] = t;
    }
  }
}

// layout repack through a 32x33 LDS tile: [N][C][P] <-> [N][P][C], P = H*W
__global__ void transpose_cp_kernel(const float* x, float* y, int rows, int cols) {
  // x: [n][rows][cols] -> y: [n][cols][rows]
  __shared__ float tile[32][33];
  const int n = blockIdx.z;
  const float* xp = x + (size_t)n * rows * cols;
  float* yp = y + (size_t)n * rows * cols;
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int j = ty; j < 32; j += 8) {
    const int r = r0 + j, c = c0 + tx;
    if (r < rows && c < cols) tile[j][tx] = xp[(size_t)r * cols + c];
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int c = c0 + j, r = r0 + tx;
    if (r < rows && c < cols) yp[(size_t)c * rows + r] = tile[tx][j];
  }
}

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, long long n, float step_size, float beta1, float beta2, float eps,
                            float inv_sqrt_bc2) {
  GRID_STRIDE(i, n) {
    const float gi = g[i];
    const float mi = beta1 * m[i] + (1.f - beta1) * gi;
    const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] = p[i] - step_size * (mi / (sqrtf(vi) * inv_sqrt_bc2 + eps));
  }
}

// multi-tensor Adam: one launch for a whole parameter list.  `table` holds n_tensors records of 5 x 8 bytes:
// {p, g, m, v, numel}; blockIdx.y selects the tensor, blockIdx.x grid-strides over its elements.
__global__ __launch_bounds__(256) void adam_multi_kernel(const unsigned long long* __restrict__ table, float step_size,
                                                         float beta1, float beta2, float eps, float inv_sqrt_bc2) {
  const unsigned long long* rec = table + (size_t)blockIdx.y * 5;
  float* __restrict__ p = reinterpret_cast<float*>(rec[0]);
  const float* __restrict__ g = reinterpret_cast<const float*>(rec[1]);
  float* __restrict__ m = reinterpret_cast<float*>(rec[2]);
  float* __restrict__ v = reinterpret_cast<float*>(rec[3]);
  const long long n = (long long)rec[4];
  // a block owns chunks of 4096 elements (blockIdx.x, then a grid stride); blocks past a small tensor's end leave at once
  const bool vec = ((rec[0] | rec[1] | rec[2] | rec[3]) & 15) == 0;
  for (long long c0 = (long long)blockIdx.x * 4096; c0 < n; c0 += (long long)gridDim.x * 4096) {
    if (vec && c0 + 4096 <= n) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long i = c0 + (j * 256 + threadIdx.x) * 4;
        const f32x4 gi = *reinterpret_cast<const f32x4*>(g + i);
        const f32x4 mi = beta1 * *reinterpret_cast<const f32x4*>(m + i) + (1.f - beta1) * gi;
        const f32x4 vi = beta2 * *reinterpret_cast<const f32x4*>(v + i) + (1.f - beta2) * gi * gi;
        f32x4 pi = *reinterpret_cast<const f32x4*>(p + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) pi[e] = pi[e] - step_size * (mi[e] / (sqrtf(vi[e]) * inv_sqrt_bc2 + eps));
        *reinterpret_cast<f32x4*>(m + i) = mi;
        *reinterpret_cast<f32x4*>(v + i) = vi;
        *reinterpret_cast<f32x4*>(p + i) = pi;
      }
    } else {
      const long long end = c0 + 4096 < n ? c0 + 4096 : n;
      for (long long i = c0 + threadIdx.x; i < end; i += 256) {
        const float gi = g[i];
        const float mi = beta1 * m[i] + (1.f - beta1) * gi;
        const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] = p[i] - step_size * (mi / (sqrtf(vi) * inv_sqrt_bc2 + eps));
      }
    }
  }
}


// ---- small host -> device uploads carried in the kernel ARGUMENTS -------------------------------------------------
// Pointer tables (multi-tensor Adam, the central-biasing layer records, the weight-repack entries) are a few KB that the host
// knows at launch time.  A pinned staging buffer + hipMemcpyAsync needs the staging block kept alive until the copy has run
// and, captured into a hipGraph, would re-read that host address on every replay; a kernel whose by-value argument IS the
// data has neither problem: the bytes travel in the launch packet (and are stored in the graph node).
constexpr int kUploadChunk = 2048;
struct UploadBlob { unsigned int w[kUploadChunk / 4]; };
__global__ __launch_bounds__(256) void upload_small_kernel(unsigned int* __restrict__ dst, UploadBlob blob, int nwords) {
  for (int i = threadIdx.x; i < nwords; i += 256) dst[i] = blob.w[i];
}

// The one write path of the device records (records.h): one wave, lane i < 16 stores word i of the by-value image iff bit i of
// `mask` is set.  Ordinary stream work, like the launches that read the record; a word that is not named keeps what it holds.
__global__ __launch_bounds__(64) void record_write_kernel(unsigned int* __restrict__ rec, RecordImage img, unsigned mask) {
  const unsigned i = threadIdx.x;
  if (i < (unsigned)kRecordWords && ((mask >> i) & 1u)) rec[i] = img.w[i];
}
int record_write(void* rec, const void* image, size_t bytes, unsigned mask, hipStream_t st, const char* name) {
  SRGAN_REQUIRE(rec && (reinterpret_cast<uintptr_t>(rec) & 3) == 0 && bytes % 4 == 0 && bytes <= sizeof(RecordImage) &&
                    (mask >> (bytes / 4)) == 0, "%s: words %#x of a record of %zu bytes at %p", name, mask, bytes, rec);
  RecordImage img = {};
  std::memcpy(img.w, image, bytes);
  hipLaunchKernelGGL(record_write_kernel, dim3(1), dim3(64), 0, st, static_cast<unsigned int*>(rec), img, mask);
  return check_launch(name);
}

// ---- device-resident Adam state ---------------------------------------------------------------------------------------
// AdamState (records.h): the step counter lives on the device so that a captured train step (hipGraph) advances it on every
// replay; the host mirrors the count for checkpoints only.
// torch 1.4: p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)   (bias corrections in double, as the host path did)
// The betas enter as the float32 numbers of the record: 1 - b^t here and 1.f - b in the update come from b = float32(beta), where
// torch 1.4 takes float32(1 - beta) and 1 - beta^t from the Python doubles.  On the update that is a relative difference of at most
// c = |float32(beta) - beta| / (1 - beta) per beta (1.29e-5 for beta2 = 0.999, 0 for beta1 = 0.5);
// tests/test_adam_kernels_gpu.py::test_distance_to_torch14_stays_inside_c holds it there (derivation: tests/adam_common.py).
__global__ void adam_tick_kernel(AdamState* s) {
  const int t = s->step + 1;
  s->step = t;
  const double bc1 = 1.0 - pow((double)s->beta1, (double)t);
  const double bc2 = 1.0 - pow((double)s->beta2, (double)t);
  s->step_size = (float)((double)s->lr / bc1);
  s->inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
}
// The scaled gradient enters the update as an opaque value, like the loaded one of the plain kernel: left visible, the product
// g * scale changes which of the two multiplies of beta * m + (1 - beta) * g the compiler contracts into the fused multiply-add
// (fma(1 - beta1, g, beta1 * m) in the plain kernel became fma(beta1, m, (1 - beta1) * g)), and the guarded update with
// scale = 1 no longer matched the plain one bit for bit.
__device__ __forceinline__ float adam_opaque(float x) {
  asm volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ f32x4 adam_opaque(f32x4 x) {
  asm volatile("" : "+v"(x));
  return x;
}
// The update of one blockIdx.y record of the table, shared by the plain and the guarded kernel so that the two cannot drift:
// kScaled multiplies every gradient element by `scale` first (one fp32 multiply, the gradient tensor itself is not written) and
// is otherwise the same arithmetic; with kScaled = false `scale` is not read.
template <bool kScaled>
__device__ __forceinline__ void adam_multi_dev_update(const unsigned long long* __restrict__ table,
                                                      const AdamState* __restrict__ st, float scale) {
  const float step_size = st->step_size, beta1 = st->beta1, beta2 = st->beta2, eps = st->eps, inv_sqrt_bc2 = st->inv_sqrt_bc2;
  const unsigned long long* rec = table + (size_t)blockIdx.y * 5;
  float* __restrict__ p = reinterpret_cast<float*>(rec[0]);
  const float* __restrict__ g = reinterpret_cast<const float*>(rec[1]);
  float* __restrict__ m = reinterpret_cast<float*>(rec[2]);
  float* __restrict__ v = reinterpret_cast<float*>(rec[3]);
  const long long n = (long long)rec[4];
  const bool vec = ((rec[0] | rec[1] | rec[2] | rec[3]) & 15) == 0;
  for (long long c0 = (long long)blockIdx.x * 4096; c0 < n; c0 += (long long)gridDim.x * 4096) {
    if (vec && c0 + 4096 <= n) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long i = c0 + (j * 256 + threadIdx.x) * 4;
        f32x4 gi = *reinterpret_cast<const f32x4*>(g + i);
        if (kScaled) gi = adam_opaque(gi * scale);
        const f32x4 mi = beta1 * *reinterpret_cast<const f32x4*>(m + i) + (1.f - beta1) * gi;
        const f32x4 vi = beta2 * *reinterpret_cast<const f32x4*>(v + i) + (1.f - beta2) * gi * gi;
        f32x4 pi = *reinterpret_cast<const f32x4*>(p + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) pi[e] = pi[e] - step_size * (mi[e] / (sqrtf(vi[e]) * inv_sqrt_bc2 + eps));
        *reinterpret_cast<f32x4*>(m + i) = mi;
        *reinterpret_cast<f32x4*>(v + i) = vi;
        *reinterpret_cast<f32x4*>(p + i) = pi;
      }
    } else {
      const long long end = c0 + 4096 < n ? c0 + 4096 : n;
      for (long long i = c0 + threadIdx.x; i < end; i += 256) {
        float gi = g[i];
        if (kScaled) gi = adam_opaque(gi * scale);
        const float mi = beta1 * m[i] + (1.f - beta1) * gi;
        const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] = p[i] - step_size * (mi / (sqrtf(vi) * inv_sqrt_bc2 + eps));
      }
    }
  }
}
__global__ __launch_bounds__(256) void adam_multi_dev_kernel(const unsigned long long* __restrict__ table,
                                                             const AdamState* __restrict__ st) {
  adam_multi_dev_update<false>(table, st, 1.f);
}

// ---- device-side gradient guard (extension, no counterpart in the reference) ------------------------------------------------------
// GradScaler's "found inf: skip the step" and clip_grad_norm_ (norm type 2) for an optimiser whose step the host never sees (a
// replayed hipGraph).  One record per optimiser (GuardState, records.h); norm / scale / skip are those of the last step, the
// counters are cumulative.

// Sum of squares of every gradient, one fp32 partial per 4096-element chunk.  `table`: n_records records of three 64-bit words
// {g, numel, chunk0}; the work is the flat chunk list of ema_multi_dev_kernel (chunk0 = prefix sum of ceil(numel / 4096)), so 300
// tiny tensors cost one chunk each.  Element e of a chunk belongs to thread (e / 4) % 256, slot (e / 1024) * 4 + e % 4 -- the same
// owner whether the chunk is read with 16-byte loads (aligned pointer, full chunk) or element by element (tail, misaligned view;
// missing elements count as +0, which an add returns unchanged), so a partial does not depend on the path taken.
// Add depth of one chunk, D = 24: 16 serial fused multiply-adds per thread (x * x + acc, ONE rounding each, slot order), 6 levels
// of the xor butterfly over the 64 lanes of a wave, 2 levels over the 4 waves through LDS ((w0 + w1) + (w2 + w3)).  Every partial
// has one owner block and a fixed order: no atomics, and the grid only decides which block computes which chunk.
constexpr int kGuardChunk = 4096;
constexpr int kGuardRecWords = 3;
__global__ __launch_bounds__(256) void grad_sumsq_partials_kernel(const unsigned long long* __restrict__ table, int n_records,
                                                                  long long total_chunks, float* __restrict__ partials) {
  __shared__ float red[4];
  for (long long ch = blockIdx.x; ch < total_chunks; ch += gridDim.x) {
    int lo = 0, hi = n_records - 1;          // the last record whose first chunk is <= ch (block-uniform: scalar loads)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((long long)table[(size_t)mid * kGuardRecWords + 2] <= ch) lo = mid; else hi = mid - 1;
    }
    const unsigned long long* rec = table + (size_t)lo * kGuardRecWords;
    const float* __restrict__ g = reinterpret_cast<const float*>(rec[0]);
    const long long n = (long long)rec[1];
    const long long c0 = (ch - (long long)rec[2]) * kGuardChunk;
    f32x4 x[4];
    if (c0 >= 0 && c0 + kGuardChunk <= n && (rec[0] & 15) == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = *reinterpret_cast<const f32x4*>(g + c0 + (j * 256 + threadIdx.x) * 4);
    } else {                                  // (a table whose prefix sums disagree with its sizes reads nothing: partial 0)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long long i = c0 + (j * 256 + threadIdx.x) * 4 + e;
          x[j][e] = (c0 >= 0 && i < n) ? g[i] : 0.f;
        }
      }
    }
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_fmaf(x[j][e], x[j][e], acc);
    }
    acc = wave_sum(acc);
    __syncthreads();                          // the previous chunk's reads of red[]
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[ch] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// One workgroup: S = sum of the partials in double -- thread t adds partials t, t + 256, ... in ascending order, then a fixed
// LDS tree over the 256 threads -- and the decision.  S not finite (a NaN, an Inf, squares that overflowed): skip.  Otherwise
// scale = min(1, max_norm / (norm + 1e-6f)) in fp32 (clip_grad_norm_; max_norm = +inf gives exactly 1).
__global__ __launch_bounds__(256) void grad_guard_finalize_kernel(const float* __restrict__ partials, long long total_chunks,
                                                                  GuardState* __restrict__ s) {
  __shared__ double red[256];
  double acc = 0.0;
  for (long long i = threadIdx.x; i < total_chunks; i += 256) acc += (double)partials[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double S = red[0];
    const float norm = (float)sqrt(S);
    const bool skip = !isfinite(S);
    const float scale = skip ? 0.f : fminf(1.f, s->max_norm / (norm + 1e-6f));
    s->norm = norm;
    s->scale = scale;
    s->skip = skip ? 1 : 0;
    s->steps += 1;
    if (skip) s->skipped += 1;
    else if (scale < 1.f) s->clipped += 1;
  }
}

// adam_multi_dev_kernel behind the guard record: nothing is stored when the step is skipped, otherwise the update runs on
// g * scale (scale = 1 returns g bit for bit, so an idle guard changes no result).
__global__ __launch_bounds__(256) void adam_multi_dev_guard_kernel(const unsigned long long* __restrict__ table,
                                                                   const AdamState* __restrict__ st,
                                                                   const GuardState* __restrict__ gs) {
  if (gs->skip) return;
  adam_multi_dev_update<true>(table, st, gs->scale);
}

// ---- exponential moving average of the sampling weights (extension, no counterpart in the reference) ------------------
// EmaState (records.h) {n, ramp, decay, c}: n = updates done, c = 1 - d_n of the update in flight.  Like AdamState the count lives
// on the device so that a captured train step advances it on every replay; the host mirrors n for checkpoints only.
// d_n = ramp ? min(decay, (1 + n) / (10 + n)) : decay in double, rounded to float once; c = 1 - d_n in float
__global__ void ema_tick_kernel(EmaState* s) {
  const int n = s->n + 1;
  s->n = n;
  double d = (double)s->decay;
  if (s->ramp) {
    const double r = (1.0 + (double)n) / (10.0 + (double)n);
    d = r < d ? r : d;
  }
  s->c = 1.f - (float)d;
}

// One launch for every tensor of every averaged network.  `table`: n_records records of five 64-bit words
// {dst, src, numel, kind, chunk0}.  The work is the FLAT list of 4096-element chunks of all records (chunk0 = index of a record's
// first chunk, a prefix sum the host wrote); blocks grid-stride over that list, so a network of many small tensors costs one chunk
// each instead of a grid row of idle blocks.  kind 0: e <- e + c * (p - e) on fp32 (returns e exactly where p == e); kind 1:
// dst <- src bit for bit, numel counting 32-bit words.  Every element is written by exactly one thread from its own old value:
// no atomics, and the result does not depend on the grid.
constexpr int kEmaChunk = 4096;
constexpr int kEmaRecWords = 5;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void ema_multi_dev_kernel(const unsigned long long* __restrict__ table, int n_records,
                                                            long long total_chunks, const EmaState* __restrict__ st) {
  const float c = st->c;
  for (long long ch = blockIdx.x; ch < total_chunks; ch += gridDim.x) {
    int lo = 0, hi = n_records - 1;          // the last record whose first chunk is <= ch (block-uniform: scalar loads)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((long long)table[(size_t)mid * kEmaRecWords + 4] <= ch) lo = mid; else hi = mid - 1;
    }
    const unsigned long long* rec = table + (size_t)lo * kEmaRecWords;
    const long long n = (long long)rec[2];
    const long long c0 = (ch - (long long)rec[4]) * kEmaChunk;
    if (c0 < 0 || c0 >= n) continue;         // (a table whose prefix sums disagree with its sizes touches nothing)
    const bool vec = ((rec[0] | rec[1]) & 15) == 0 && c0 + kEmaChunk <= n;
    const long long end = c0 + kEmaChunk < n ? c0 + kEmaChunk : n;
    if (rec[3] == 0) {
      float* e = reinterpret_cast<float*>(rec[0]);
      const float* p = reinterpret_cast<const float*>(rec[1]);
      if (vec) {
        f32x4 pv[4], ev[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const long long i = c0 + (j * 256 + threadIdx.x) * 4;
          pv[j] = *reinterpret_cast<const f32x4*>(p + i);
          ev[j] = *reinterpret_cast<const f32x4*>(e + i);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const long long i = c0 + (j * 256 + threadIdx.x) * 4;
          *reinterpret_cast<f32x4*>(e + i) = ev[j] + c * (pv[j] - ev[j]);
        }
      } else {
        for (long long i = c0 + threadIdx.x; i < end; i += 256) {
          const float ei = e[i];
          e[i] = ei + c * (p[i] - ei);
        }
      }
    } else {
      unsigned int* d = reinterpret_cast<unsigned int*>(rec[0]);
      const unsigned int* s = reinterpret_cast<const unsigned int*>(rec[1]);
      if (vec) {
        u32x4 sv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) sv[j] = *reinterpret_cast<const u32x4*>(s + c0 + (j * 256 + threadIdx.x) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<u32x4*>(d + c0 + (j * 256 + threadIdx.x) * 4) = sv[j];
      } else {
        for (long long i = c0 + threadIdx.x; i < end; i += 256) d[i] = s[i];
      }
    }
  }
}

}  // namespace srgan

using namespace srgan;

#define LAUNCH1D(kernel, n, st, ...)                                                        \
  do {                                                                                      \
    hipLaunchKernelGGL(kernel, dim3(grid_for(n)), dim3(256), 0, as_stream(st), __VA_ARGS__); \
    return check_launch(#kernel);                                                           \
  } while (0)

extern "C" int srgan_act_fwd(const float* x, float* y, long long n, int act, float slope, void* stream) {
  SRGAN_REQUIRE(x && y && n >= 0, "act_fwd: bad argument");
  if (n == 0) return 0;
  LAUNCH1D(act_fwd_kernel, n, stream, x, y, n, act, slope);
}
extern "C" int srgan_act_bwd(const float* y, const float* dy, float* dx, long long n, int act, float slope, void* stream) {
  SRGAN_REQUIRE(y && dy && dx && n >= 0, "act_bwd: bad argument");
  if (n == 0) return 0;
  LAUNCH1D(act_bwd_kernel, n, stream, y, dy, dx, n, act, slope);
}
extern "C" int srgan_act_bwd_io(const void* y, int y_bf16, const void* dy, int dy_bf16, void* dx, int dx_bf16, long long n, int act,
                                float slope, void* stream) {
  SRGAN_REQUIRE(y && dy && dx && n >= 0, "act_bwd_io: bad argument");
  SRGAN_REQUIRE((n & 7) == 0, "act_bwd_io: n %% 8 != 0");
  if (n == 0) return 0;
  const long long n8 = n / 8;
  const int sel = (y_bf16 ? 4 : 0) | (dy_bf16 ? 2 : 0) | (dx_bf16 ? 1 : 0);
  switch (sel) {
    case 0: LAUNCH1D((act_bwd_io_kernel<false, false, false>), n8, stream, y, dy, dx, n8, act, slope);
    case 1: LAUNCH1D((act_bwd_io_kernel<false, false, true>), n8, stream, y, dy, dx, n8, act, slope);
    case 2: LAUNCH1D((act_bwd_io_kernel<false, true, false>), n8, stream, y, dy, dx, n8, act, slope);
    case 3: LAUNCH1D((act_bwd_io_kernel<false, true, true>), n8, stream, y, dy, dx, n8, act, slope);
    case 4: LAUNCH1D((act_bwd_io_kernel<true, false, false>), n8, stream, y, dy, dx, n8, act, slope);
    case 5: LAUNCH1D((act_bwd_io_kernel<true, false, true>), n8, stream, y, dy, dx, n8, act, slope);
    case 6: LAUNCH1D((act_bwd_io_kernel<true, true, false>), n8, stream, y, dy, dx, n8, act, slope);
    default: LAUNCH1D((act_bwd_io_kernel<true, true, true>), n8, stream, y, dy, dx, n8, act, slope);
  }
}
extern "C" int srgan_tanh_fwd(const float* x, float* y, long long n, void* stream) {
  SRGAN_REQUIRE(x && y && n >= 0, "tanh_fwd: bad argument");
  if (n == 0) return 0;
  LAUNCH1D(tanh_fwd_kernel, n, stream, x, y, n);
}
extern "C" int srgan_tanh_bwd(const float* y, const float* dy, float* dx, long long n, void* stream) {
  SRGAN_REQUIRE(y && dy && dx && n >= 0, "tanh_bwd: bad argument");
  if (n == 0) return 0;
  LAUNCH1D(tanh_bwd_kernel, n, stream, y, dy, dx, n);
}
extern "C" int srgan_add(const float* a, const float* b, float* y, long long n, void* stream) {
  SRGAN_REQUIRE(a && b && y && n >= 0, "add: bad argument");
  if (n == 0) return 0;
  LAUNCH1D(add_kernel, n, stream, a, b, y, n);
}

extern "C" int srgan_avgpool3s2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream) {
  SRGAN_REQUIRE(x && y && N > 0 && H > 0 && W > 0 && C > 0, "avgpool3s2_fwd: bad argument");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  LAUNCH1D(avgpool3s2_fwd_kernel, (long long)N * Ho * Wo * C, stream, x, y, N, H, W, C, Ho, Wo);
}
extern "C" int srgan_avgpool3s2_bwd(const float* dy, float* dx, int N, int H, int W, int C, void* stream) {
  SRGAN_REQUIRE(dy && dx && N > 0 && H > 0 && W > 0 && C > 0, "avgpool3s2_bwd: bad argument");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  LAUNCH1D(avgpool3s2_bwd_kernel, (long long)N * H * W * C, stream, dy, dx, N, H, W, C, Ho, Wo);
}
extern "C" int srgan_avgpool2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream) {
  SRGAN_REQUIRE(x && y && N > 0 && H > 1 && W > 1 && C > 0, "avgpool2_fwd: bad argument");
  LAUNCH1D(avgpool2_fwd_kernel, (long long)N * (H / 2) * (W / 2) * C, stream, x, y, N, H, W, C, H / 2, W / 2);
}
extern "C" int srgan_avgpool2_bwd(const float* dy, float* dx, int N, int H, int W, int C, void* stream) {
  SRGAN_REQUIRE(dy && dx && N > 0 && H > 1 && W > 1 && C > 0, "avgpool2_bwd: bad argument");
  LAUNCH1D(avgpool2_bwd_kernel, (long long)N * H * W * C, stream, dy, dx, N, H, W, C, H / 2, W / 2);
}
extern "C" int srgan_avgpool2_fwd_io(const void* x, int x_bf16, void* y, int y_bf16, int N, int H, int W, int C, void* stream) {
  SRGAN_REQUIRE(x && y && N > 0 && H > 1 && W > 1 && C > 0 && (C & 3) == 0, "avgpool2_fwd_io: bad argument (C % 4 == 0)");
  const long long n = (long long)N * (H / 2) * (W / 2) * (C / 4);
  if (x_bf16 && y_bf16) { LAUNCH1D((avgpool2_fwd_io_kernel<true, true>), n, stream, x, y, N, H, W, C, H / 2, W / 2); }
  if (x_bf16) { LAUNCH1D((avgpool2_fwd_io_kernel<true, false>), n, stream, x, y, N, H, W, C, H / 2, W / 2); }
  if (y_bf16) { LAUNCH1D((avgpool2_fwd_io_kernel<false, true>), n, stream, x, y, N, H, W, C, H / 2, W / 2); }
  LAUNCH1D((avgpool2_fwd_io_kernel<false, false>), n, stream, x, y, N, H, W, C, H / 2, W / 2);
}
extern "C" int srgan_avgpool2_bwd_io(const void* dy, int dy_bf16, void* dx, int dx_bf16, int N, int H, int W, int C, void* stream) {
  SRGAN_REQUIRE(dy && dx && N > 0 && H > 1 && W > 1 && C > 0 && (C & 3) == 0, "avgpool2_bwd_io: bad argument (C % 4 == 0)");
  const long long n = (long long)N * H * W * (C / 4);
  if (dy_bf16 && dx_bf16) { LAUNCH1D((avgpool2_bwd_io_kernel<true, true>), n, stream, dy, dx, N, H, W, C, H / 2, W / 2); }
  if (dy_bf16) { LAUNCH1D((avgpool2_bwd_io_kernel<true, false>), n, stream, dy, dx, N, H, W, C, H / 2, W / 2); }
  if (dx_bf16) { LAUNCH1D((avgpool2_bwd_io_kernel<false, true>), n, stream, dy, dx, N, H, W, C, H / 2, W / 2); }
  LAUNCH1D((avgpool2_bwd_io_kernel<false, false>), n, stream, dy, dx, N, H, W, C, H / 2, W / 2);
}
extern "C" int srgan_lrelu_gap_fwd(const float* x, float* y, int N, int HW, int C, float slope, void* stream) {
  SRGAN_REQUIRE(x && y && N > 0 && HW > 0 && C > 0, "lrelu_gap_fwd: bad argument");
  LAUNCH1D(lrelu_gap_fwd_kernel, (long long)N * C, stream, x, y, N, HW, C, slope);
}
extern "C" int srgan_lrelu_gap_bwd(const float* x, const float* dy, float* dx, int N, int HW, int C, float slope, void* stream) {
  SRGAN_REQUIRE(x && dy && dx && N > 0 && HW > 0 && C > 0, "lrelu_gap_bwd: bad argument");
  LAUNCH1D(lrelu_gap_bwd_kernel, (long long)N * HW * C, stream, x, dy, dx, N, HW, C, slope);
}

// Encoder.reparametrize (pyfiles/model.py:459-463): c = eps * exp(logvar / 2) + mu on [B, ndim].  The reference is four
// elementwise launches forward and three backward on 256 floats; here one each.  Every product and sum is rounded on its own
// (no FMA contraction): the same values as the chain of separate elementwise passes.
namespace srgan {
__global__ void reparam_fwd_kernel(const float* mu, const float* logvar, const float* eps, float* out, float* stdv, long long n) {
  GRID_STRIDE(i, n) {
    const float s = expf(__fmul_rn(0.5f, logvar[i]));
    stdv[i] = s;
    out[i] = __fadd_rn(__fmul_rn(eps[i], s), mu[i]);
  }
}
__global__ void reparam_bwd_kernel(const float* g, const float* eps, const float* stdv, float* dlogvar, long long n) {
  GRID_STRIDE(i, n) dlogvar[i] = __fmul_rn(__fmul_rn(__fmul_rn(g[i], eps[i]), stdv[i]), 0.5f);
}
}  // namespace srgan
extern "C" int srgan_reparam_fwd(const float* mu, const float* logvar, const float* eps, float* out, float* stdv, long long n,
                                 void* stream) {
  SRGAN_REQUIRE(mu && logvar && eps && out && stdv && n > 0, "reparam_fwd: bad argument");
  LAUNCH1D(srgan::reparam_fwd_kernel, n, stream, mu, logvar, eps, out, stdv, n);
}
extern "C" int srgan_reparam_bwd(const float* g, const float* eps, const float* stdv, float* dlogvar, long long n, void* stream) {
  SRGAN_REQUIRE(g && eps && stdv && dlogvar && n > 0, "reparam_bwd: bad argument");
  LAUNCH1D(srgan::reparam_bwd_kernel, n, stream, g, eps, stdv, dlogvar, n);
}

extern "C" int srgan_linear_fwd(const float* x, const float* W, const float* b, float* y, int M, int N, int K, void* stream) {
  SRGAN_REQUIRE(x && W && y && M > 0 && N > 0 && K > 0, "linear_fwd: bad argument");
  const long long threads = (long long)M * N * 64;
  hipLaunchKernelGGL(linear_fwd_kernel, dim3((unsigned)ceil_div(threads, 256)), dim3(256), 0, as_stream(stream), x, W, b, y, M, N, K);
  return check_launch("linear_fwd_kernel");
}
extern "C" int srgan_linear_bwd(const float* x, const float* W, const float* dy, float* dx, float* dW, float* db,
                                int M, int N, int K, void* stream) {
  SRGAN_REQUIRE(x && W && dy && M > 0 && N > 0 && K > 0, "linear_bwd: bad argument");
  hipStream_t st = as_stream(stream);
  if (dx) hipLaunchKernelGGL(linear_bwd_dx_kernel, dim3(grid_for((long long)M * K)), dim3(256), 0, st, W, dy, dx, M, N, K);
  if (dW) hipLaunchKernelGGL(linear_bwd_dw_kernel, dim3(grid_for((long long)N * K)), dim3(256), 0, st, x, dy, dW, db, M, N, K);
  return check_launch("linear_bwd");
}

extern "C" int srgan_nchw_to_nhwc(const float* x, float* y, int N, int C, int H, int W, void* stream) {
  SRGAN_REQUIRE(x && y && N > 0 && C > 0 && H > 0 && W > 0, "nchw_to_nhwc: bad argument");
  const int P = H * W;  // [N][C][P] -> [N][P][C]
  dim3 g((P + 31) / 32, (C + 31) / 32, N);
  hipLaunchKernelGGL(transpose_cp_kernel, g, dim3(256), 0, as_stream(stream), x, y, C, P);
  return check_launch("transpose_cp_kernel");
}
extern "C" int srgan_nhwc_to_nchw(const float* x, float* y, int N, int C, int H, int W, void* stream) {
  SRGAN_REQUIRE(x && y && N > 0 && C > 0 && H > 0 && W > 0, "nhwc_to_nchw: bad argument");
  const int P = H * W;  // [N][P][C] -> [N][C][P]
  dim3 g((C + 31) / 32, (P + 31) / 32, N);
  hipLaunchKernelGGL(transpose_cp_kernel, g, dim3(256), 0, as_stream(stream), x, y, P, C);
  return check_launch("transpose_cp_kernel");
}

extern "C" int srgan_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                               float beta2, float eps, int step_count, void* stream) {
  SRGAN_REQUIRE(n >= 0 && step_count >= 1, "adam_step: bad argument");
  if (n == 0) return 0;                  // an empty tensor: nothing to do (torch hands out null pointers for those)
  SRGAN_REQUIRE(p && g && m && v, "adam_step: bad argument");
  // torch 1.4: p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
  const double bc1 = 1.0 - std::pow((double)beta1, step_count);
  const double bc2 = 1.0 - std::pow((double)beta2, step_count);
  const float step_size = (float)((double)lr / bc1);
  const float inv_sqrt_bc2 = (float)(1.0 / std::sqrt(bc2));
  LAUNCH1D(adam_kernel, n, stream, p, g, m, v, n, step_size, beta1, beta2, eps, inv_sqrt_bc2);
}

extern "C" int srgan_adam_multi(const void* table, int n_tensors, long long max_numel, float lr, float beta1, float beta2,
                                float eps, int step_count, void* stream) {
  SRGAN_REQUIRE(table && n_tensors > 0 && max_numel > 0 && step_count >= 1, "adam_multi: bad argument");
  const double bc1 = 1.0 - std::pow((double)beta1, step_count);
  const double bc2 = 1.0 - std::pow((double)beta2, step_count);
  const float step_size = (float)((double)lr / bc1);
  const float inv_sqrt_bc2 = (float)(1.0 / std::sqrt(bc2));
  const unsigned bx = (unsigned)std::max<long long>(1, std::min<long long>(ceil_div(max_numel, 4096), 2048));
  hipLaunchKernelGGL(adam_multi_kernel, dim3(bx, (unsigned)n_tensors), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const unsigned long long*>(table), step_size, beta1, beta2, eps, inv_sqrt_bc2);
  return check_launch("adam_multi_kernel");
}

extern "C" int srgan_upload_small(void* dst_dev, const void* src_host, size_t nbytes, void* stream) {
  SRGAN_REQUIRE(dst_dev && src_host && nbytes % 4 == 0, "upload_small: bad argument (bytes must be a multiple of 4)");
  SRGAN_REQUIRE(nbytes <= (1u << 20), "upload_small: meant for tables of a few KB (%zu bytes asked)", nbytes);
  const unsigned char* src = static_cast<const unsigned char*>(src_host);
  unsigned char* dst = static_cast<unsigned char*>(dst_dev);
  for (size_t off = 0; off < nbytes; off += srgan::kUploadChunk) {
    const size_t n = std::min<size_t>(srgan::kUploadChunk, nbytes - off);
    srgan::UploadBlob blob;
    std::memcpy(blob.w, src + off, n);
    hipLaunchKernelGGL(srgan::upload_small_kernel, dim3(1), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<unsigned int*>(dst + off), blob, (int)(n / 4));
  }
  return check_launch("upload_small_kernel");
}

extern "C" size_t srgan_adam_state_bytes(void) { return sizeof(srgan::AdamState); }

extern "C" int srgan_adam_state_init(void* state, float lr, float beta1, float beta2, float eps, int steps_done, void* stream) {
  SRGAN_REQUIRE(state && steps_done >= 0, "adam_state_init: bad argument");
  srgan::AdamState s = {};               // step_size, inv_sqrt_bc2 (the tick derives them) and the pad at zero
  s.step = steps_done; s.lr = lr; s.beta1 = beta1; s.beta2 = beta2; s.eps = eps;
  return srgan::record_write(state, &s, sizeof s, srgan::record_all_words<srgan::AdamState>(), as_stream(stream), "adam_state_init");
}

extern "C" int srgan_adam_state_set_lr(void* state, float lr, void* stream) {
  SRGAN_REQUIRE(state, "adam_state_set_lr: bad argument");
  srgan::AdamState s = {};
  s.lr = lr;
  return srgan::record_write(state, &s, sizeof s, srgan::kAdamSetLr, as_stream(stream), "adam_state_set_lr");
}

extern "C" int srgan_adam_multi_dev(const void* table, int n_tensors, long long max_numel, void* state, void* stream) {
  SRGAN_REQUIRE(table && state && n_tensors > 0 && max_numel > 0, "adam_multi_dev: bad argument");
  hipLaunchKernelGGL(srgan::adam_tick_kernel, dim3(1), dim3(1), 0, as_stream(stream), static_cast<srgan::AdamState*>(state));
  const unsigned bx = (unsigned)std::max<long long>(1, std::min<long long>(ceil_div(max_numel, 4096), 2048));
  hipLaunchKernelGGL(srgan::adam_multi_dev_kernel, dim3(bx, (unsigned)n_tensors), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const unsigned long long*>(table), static_cast<const srgan::AdamState*>(state));
  return check_launch("adam_multi_dev_kernel");
}

extern "C" size_t srgan_grad_guard_state_bytes(void) { return sizeof(srgan::GuardState); }

extern "C" int srgan_grad_guard_state_init(void* state, float max_norm, void* stream) {
  SRGAN_REQUIRE(state && max_norm > 0.f, "grad_guard_state_init: bad argument (max_norm > 0, +inf = no clipping; NaN refused)");
  srgan::GuardState s = {};              // the last step's decision and the counters at zero
  s.max_norm = max_norm; s.scale = 1.f;
  return srgan::record_write(state, &s, sizeof s, srgan::record_all_words<srgan::GuardState>(), as_stream(stream),
                             "grad_guard_state_init");
}

extern "C" int srgan_grad_guard_state_set_max_norm(void* state, float max_norm, void* stream) {
  SRGAN_REQUIRE(state && max_norm > 0.f, "grad_guard_state_set_max_norm: bad argument (max_norm > 0, +inf = no clipping; NaN refused)");
  srgan::GuardState s = {};
  s.max_norm = max_norm;
  return srgan::record_write(state, &s, sizeof s, srgan::kGuardSetMaxNorm, as_stream(stream), "grad_guard_state_set_max_norm");
}

extern "C" int srgan_grad_guard_state_set_counters(void* state, int steps, int skipped, int clipped, void* stream) {
  SRGAN_REQUIRE(state && steps >= 0 && skipped >= 0 && clipped >= 0,
                "grad_guard_state_set_counters: bad argument (steps, skipped, clipped >= 0)");
  srgan::GuardState s = {};              // resume: the threshold and the last step's decision stay
  s.steps = steps; s.skipped = skipped; s.clipped = clipped;
  return srgan::record_write(state, &s, sizeof s, srgan::kGuardSetCounters, as_stream(stream), "grad_guard_state_set_counters");
}

extern "C" size_t srgan_grad_guard_workspace(long long total_chunks) {
  if (total_chunks <= 0) {
    srgan::set_error("grad_guard_workspace: bad argument (total_chunks > 0)");
    return 0;
  }
  return (size_t)total_chunks * sizeof(float);
}

extern "C" int srgan_grad_guard_reduce(const void* table, int n_records, long long total_chunks, void* ws, size_t ws_bytes,
                                       void* state, void* stream) {
  SRGAN_REQUIRE(table && ws && state && n_records > 0 && total_chunks > 0, "grad_guard_reduce: bad argument");
  SRGAN_REQUIRE(total_chunks >= n_records, "grad_guard_reduce: %lld chunks for %d records (every record holds at least one)",
                total_chunks, n_records);
  SRGAN_REQUIRE(ws_bytes >= (size_t)total_chunks * sizeof(float), "grad_guard_reduce: workspace of %zu bytes, %zu needed", ws_bytes,
                (size_t)total_chunks * sizeof(float));
  SRGAN_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3) == 0, "grad_guard_reduce: workspace not 4-byte aligned");
  // memory bound: one block per chunk up to 256 CUs x 8 blocks, the rest by grid stride
  const unsigned bx = (unsigned)std::min<long long>(total_chunks, 2048);
  hipLaunchKernelGGL(srgan::grad_sumsq_partials_kernel, dim3(bx), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const unsigned long long*>(table), n_records, total_chunks, static_cast<float*>(ws));
  hipLaunchKernelGGL(srgan::grad_guard_finalize_kernel, dim3(1), dim3(256), 0, as_stream(stream), static_cast<const float*>(ws),
                     total_chunks, static_cast<srgan::GuardState*>(state));
  return check_launch("grad_guard_reduce");
}

extern "C" int srgan_adam_multi_dev_guard(const void* table, int n_tensors, long long max_numel, void* adam_state, void* guard_state,
                                          void* stream) {
  SRGAN_REQUIRE(table && adam_state && guard_state && n_tensors > 0 && max_numel > 0, "adam_multi_dev_guard: bad argument");
  hipLaunchKernelGGL(srgan::adam_tick_kernel, dim3(1), dim3(1), 0, as_stream(stream), static_cast<srgan::AdamState*>(adam_state));
  const unsigned bx = (unsigned)std::max<long long>(1, std::min<long long>(ceil_div(max_numel, 4096), 2048));
  hipLaunchKernelGGL(srgan::adam_multi_dev_guard_kernel, dim3(bx, (unsigned)n_tensors), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const unsigned long long*>(table), static_cast<const srgan::AdamState*>(adam_state),
                     static_cast<const srgan::GuardState*>(guard_state));
  return check_launch("adam_multi_dev_guard_kernel");
}

extern "C" size_t srgan_ema_state_bytes(void) { return sizeof(srgan::EmaState); }

extern "C" size_t srgan_ema_chunk(void) { return (size_t)srgan::kEmaChunk; }

extern "C" int srgan_ema_state_init(void* state, float decay, int ramp, int n_done, void* stream) {
  SRGAN_REQUIRE(state && decay >= 0.f && decay < 1.f && n_done >= 0, "ema_state_init: bad argument (decay in [0, 1), n_done >= 0)");
  srgan::EmaState s = {};                // c (the tick derives it) at zero
  s.n = n_done; s.ramp = ramp ? 1 : 0; s.decay = decay;
  return srgan::record_write(state, &s, sizeof s, srgan::record_all_words<srgan::EmaState>(), as_stream(stream), "ema_state_init");
}

extern "C" int srgan_ema_state_set_decay(void* state, float decay, void* stream) {
  SRGAN_REQUIRE(state && decay >= 0.f && decay < 1.f, "ema_state_set_decay: bad argument (decay in [0, 1))");
  srgan::EmaState s = {};
  s.decay = decay;
  return srgan::record_write(state, &s, sizeof s, srgan::kEmaSetDecay, as_stream(stream), "ema_state_set_decay");
}

extern "C" int srgan_ema_multi_dev(const void* table, int n_records, long long total_chunks, void* state, void* stream) {
  SRGAN_REQUIRE(table && state && n_records > 0 && total_chunks > 0, "ema_multi_dev: bad argument");
  hipLaunchKernelGGL(srgan::ema_tick_kernel, dim3(1), dim3(1), 0, as_stream(stream), static_cast<srgan::EmaState*>(state));
  // memory bound: one block per chunk up to 256 CUs x 8 blocks, the rest by grid stride
  const unsigned bx = (unsigned)std::min<long long>(total_chunks, 2048);
  hipLaunchKernelGGL(srgan::ema_multi_dev_kernel, dim3(bx), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const unsigned long long*>(table), n_records, total_chunks,
                     static_cast<const srgan::EmaState*>(state));
  return check_launch("ema_multi_dev_kernel");
}
