// Batch normalisation on NHWC fp32 tensors: nn.BatchNorm2d and the central-biasing CBBNorm2d of the reference's
// norm_type="batch" (pyfiles/model.py:75-182), forward (train / eval) and backward, with the running buffers updated on
// the device.  Statistics reduce across the whole batch; every reduction is a fixed-order sum (no atomics) and workgroups
// hand over only at kernel boundaries, so results are bit-identical run to run and under graph replay.
//
//   mu_c, var_c : biased mean / variance over (n, h, w);  mu_nc : one image's channel mean over (h, w);  r_c = (var_c + eps)^-1/2
//   BN : y = act((x - mu_c) * r_c * gamma + beta)            (eval: running_mean / running_var stand in for mu_c / var_c)
//   CBB: y = act((x - mu_nc) * r_c * scale[n,c] + shift[n,c]) (+ res); scale / shift are CBIN's affine (ops.cbin_affine)
//
// Forward: per-slab (mean, M2) partials -> a finalize, one wave per channel (Chan's merge in a fixed order, the running-buffer
// update, the folded per-(n, c) coefficients m, a, b) -> an apply pass y = act((x - m) * a + b) (+ res) that also advances
// num_batches_tracked.
// Backward: per-slab {sum g, sum g * xh} partials (the activation mask rebuilt from (x - m) * a + b) -> a per-channel
// combine -> the dx pass.  Formulas: DESIGN.md section 7.
//
// Data parallel (srgan_batchnorm_sync_*): a rank holds images [n0, n0 + Nl) of a global batch of N.  Its
// slab passes run with the slab plan of the GLOBAL batch and write into the rank's chunk of an exchange buffer; after an
// all-gather of the chunks the finalize / combine read the partials of all N images in the one-process order, so the merged
// statistics are bit-identical to one process with N images.  Only this rank's images get coefficients.
#include <algorithm>
#include "common.h"

namespace srgan {
namespace {

constexpr int BN_CH = 32;      // channels per workgroup of the slab passes (8 lanes x 4 channels)

// S slabs per image: enough workgroups to cover the device, at least 64 pixel rows per slab
void bn_plan(int N, int HW, int C, int& S, int& rps) {
  const long long blocks = (long long)N * ((C + BN_CH - 1) / BN_CH);
  S = 1;
  while (blocks * S < 1024 && HW / (S * 2) >= 64) S *= 2;
  rps = (HW + S - 1) / S;
}

size_t bn_part_bytes(int N, int HW, int C) {
  int S, rps;
  bn_plan(N, HW, C, S, rps);
  return (size_t)N * S * C * sizeof(float2);
}

__device__ __forceinline__ f32x4 ldf4(const float* p, size_t i) { return *reinterpret_cast<const f32x4*>(p + i); }

// part[(n*S + s)*C + c] = {mean, M2} of the slab's pixels (sums shifted by the slab's first pixel: no E[x^2] - E[x]^2)
__global__ __launch_bounds__(256) void bn_stats_partial(const float* __restrict__ x, float2* __restrict__ part,
                                                        int HW, int C, int S, int rps) {
  const int q = threadIdx.x & 7, ty = threadIdx.x >> 3;
  const int c = blockIdx.x * BN_CH + q * 4;
  const int s = blockIdx.y, n = blockIdx.z;
  const int r0 = s * rps, r1 = min(HW, r0 + rps);
  __shared__ f32x4 sh[2][32][8];
  f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
  if (c < C && r0 < r1) {
    const size_t xb = (size_t)n * HW * C + c;
    const f32x4 x0 = ldf4(x, xb + (size_t)r0 * C);
    int r = r0 + ty;
    for (; r + 96 < r1; r += 128) {          // four rows in flight; the sums keep the row order r, r + 32, ...
      const f32x4 w0 = ldf4(x, xb + (size_t)r * C) - x0, w1 = ldf4(x, xb + (size_t)(r + 32) * C) - x0;
      const f32x4 w2 = ldf4(x, xb + (size_t)(r + 64) * C) - x0, w3 = ldf4(x, xb + (size_t)(r + 96) * C) - x0;
      a += w0; b += w0 * w0;
      a += w1; b += w1 * w1;
      a += w2; b += w2 * w2;
      a += w3; b += w3 * w3;
    }
    for (; r < r1; r += 32) {
      const f32x4 v = ldf4(x, xb + (size_t)r * C) - x0;
      a += v;
      b += v * v;
    }
  }
  sh[0][ty][q] = a;
  sh[1][ty][q] = b;
  __syncthreads();
  if (threadIdx.x < BN_CH) {
    const int cc = threadIdx.x, qq = cc >> 2, e = cc & 3;
    const int ch = blockIdx.x * BN_CH + cc;
    if (ch < C) {
      float sa = 0.f, sb = 0.f;
#pragma unroll 8
      for (int i = 0; i < 32; ++i) { sa += sh[0][i][qq][e]; sb += sh[1][i][qq][e]; }
      float mean = 0.f, m2 = 0.f;
      if (r1 > r0) {
        const float cnt = (float)(r1 - r0);
        const float dm = sa / cnt;
        mean = x[((size_t)n * HW + r0) * C + ch] + dm;
        m2 = fmaxf(sb - sa * dm, 0.f);
      }
      part[((size_t)n * S + s) * C + ch] = make_float2(mean, m2);
    }
  }
}

// Chan's merge of (mean, M2, count) with a second group
__device__ __forceinline__ void chan_merge(float& m, float& m2, float& cnt, float mb, float m2b, float cb) {
  if (cb <= 0.f) return;
  const float tot = cnt + cb, d = mb - m;
  m += d * (cb / tot);
  m2 += m2b + d * d * (cnt * (cb / tot));
  cnt = tot;
}

// wave-wide Chan merge towards lane 0, in a fixed order (shuffle-down tree)
__device__ __forceinline__ void wave_chan_merge(float& m, float& m2, float& cnt) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float mb = __shfl_down(m, o, 64), m2b = __shfl_down(m2, o, 64), cb = __shfl_down(cnt, o, 64);
    if (lane < o) chan_merge(m, m2, cnt, mb, m2b, cb);
  }
}
__device__ __forceinline__ float wave_sum_down(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// Where image n's slab partials are.  One process: rows of a dense [N][S][C] array.  Synced: the exchange buffer, rank chunks of
// Nl images each, `chunk` floats apart ([Nl][S][C] float2, then -- CBB backward -- the images' scale rows [Nl][C]).
template <bool SYNC>
__device__ __forceinline__ const float2* part_row(const float2* part, int n, int S, int C, int Nl, size_t chunk) {
  if constexpr (SYNC)
    return reinterpret_cast<const float2*>(reinterpret_cast<const float*>(part) + (size_t)(n / Nl) * chunk) + (size_t)(n % Nl) * S * C;
  else
    return part + (size_t)n * S * C;
}

// One WAVE per channel, its lanes over the images: merges the partials (slabs in order per image, then the lanes' images in a
// fixed tree), updates the running buffers, writes the statistics the backward keeps (mean / rstd [C]) and the folded per-(n, c)
// coefficients of the apply pass: y = act((x - m) * a + b).  part == null: eval-mode BN (running statistics only).  The
// counter is READ here (the factor of momentum=None) and incremented by the apply pass, after every wave has read it.
// SYNC: the merge runs over the N images of the global batch; scale / shift / m / a / b are those of images [n0, n0 + Nl).
template <bool SYNC>
__device__ __forceinline__ void bn_finalize_body(const float2* __restrict__ part, const float* __restrict__ scale,
                                                 const float* __restrict__ shift, float* __restrict__ mean,
                                                 float* __restrict__ rstd, float* __restrict__ m, float* __restrict__ a,
                                                 float* __restrict__ b, float* __restrict__ rmean, float* __restrict__ rvar,
                                                 const long long* __restrict__ nbt, int N, int HW, int C, int S, int rps,
                                                 int cbb, int batch_stats, int update, float momentum, int cumulative,
                                                 float eps, int n0, int Nl, size_t chunk) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  float mu = 0.f, m2 = 0.f, cnt = 0.f;
  if (part) {
    for (int n = lane; n < N; n += 64) {
      const float2* row = part_row<SYNC>(part, n, S, C, Nl, chunk);
      float mn = 0.f, m2n = 0.f, cn = 0.f;
      for (int s = 0; s < S; ++s) {
        const int r0 = s * rps, r1 = min(HW, r0 + rps);
        if (r1 <= r0) continue;
        const float2 p = row[(size_t)s * C + c];
        chan_merge(mn, m2n, cn, p.x, p.y, (float)(r1 - r0));
      }
      if (cbb && n >= n0 && n < n0 + Nl) m[(n - n0) * C + c] = mn;
      chan_merge(mu, m2, cnt, mn, m2n, cn);
    }
    wave_chan_merge(mu, m2, cnt);
  }
  mu = __shfl(mu, 0, 64);
  m2 = __shfl(m2, 0, 64);
  cnt = __shfl(cnt, 0, 64);
  float var;
  if (batch_stats) {
    var = m2 / cnt;
  } else {
    mu = rmean[c];
    var = rvar[c];
  }
  const float rs = 1.0f / sqrtf(var + eps);
  if (lane == 0) {
    mean[c] = mu;
    rstd[c] = rs;
    if (update) {                            // F.batch_norm's update: unbiased variance M2 / (M - 1)
      const float f = cumulative ? (float)(1.0 / (double)(*nbt + 1)) : momentum;
      rmean[c] = (1.f - f) * rmean[c] + f * mu;
      rvar[c] = (1.f - f) * rvar[c] + f * (m2 / (cnt - 1.f));
    }
  }
  for (int n = lane; n < Nl; n += 64) {
    const int nc = n * C + c;
    if (cbb) {                               // (x - mu_nc) * r_c * scale + shift
      a[nc] = rs * scale[nc];
      b[nc] = shift[nc];
    } else {                                 // (x - mu_c) * r_c * gamma + beta
      m[nc] = mu;
      a[nc] = scale ? rs * scale[c] : rs;
      b[nc] = shift ? shift[c] : 0.f;
    }
  }
}

__global__ __launch_bounds__(256) void bn_finalize(const float2* __restrict__ part, const float* __restrict__ scale,
                                                   const float* __restrict__ shift, float* __restrict__ mean,
                                                   float* __restrict__ rstd, float* __restrict__ m, float* __restrict__ a,
                                                   float* __restrict__ b, float* __restrict__ rmean, float* __restrict__ rvar,
                                                   const long long* __restrict__ nbt, int N, int HW, int C, int S, int rps,
                                                   int cbb, int batch_stats, int update, float momentum, int cumulative,
                                                   float eps) {
  bn_finalize_body<false>(part, scale, shift, mean, rstd, m, a, b, rmean, rvar, nbt, N, HW, C, S, rps, cbb, batch_stats, update,
                          momentum, cumulative, eps, 0, N, 0);
}

// the synced finalize: training mode only (batch statistics of the global batch)
__global__ __launch_bounds__(256) void bn_sync_finalize(const float2* __restrict__ part, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, float* __restrict__ mean,
                                                        float* __restrict__ rstd, float* __restrict__ m, float* __restrict__ a,
                                                        float* __restrict__ b, float* __restrict__ rmean,
                                                        float* __restrict__ rvar, const long long* __restrict__ nbt, int N,
                                                        int HW, int C, int S, int rps, int cbb, int update, float momentum,
                                                        int cumulative, float eps, int n0, int Nl, size_t chunk) {
  bn_finalize_body<true>(part, scale, shift, mean, rstd, m, a, b, rmean, rvar, nbt, N, HW, C, S, rps, cbb, 1, update, momentum,
                         cumulative, eps, n0, Nl, chunk);
}

// y = act((x - m[n,c]) * a[n,c] + b[n,c]) (+ res), float4 per lane; grid (x: strides over one image, y: image), so the
// channel index is a 32-bit remainder within the image (HW * C < 2^31, checked by the host)
template <bool RES>
__global__ __launch_bounds__(256) void bn_apply(const float* __restrict__ x, const float* __restrict__ m,
                                                const float* __restrict__ a, const float* __restrict__ b,
                                                const float* __restrict__ res, float* __restrict__ y, int HWC, int C,
                                                int act, float slope, long long* __restrict__ nbt) {
  if (nbt && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *nbt += 1;   // num_batches_tracked (bn_finalize read it)
  const int n = blockIdx.y;
  const size_t base = (size_t)n * HWC;
  for (int j = (blockIdx.x * blockDim.x + threadIdx.x) * 4; j < HWC; j += gridDim.x * blockDim.x * 4) {
    const size_t i = base + j;
    const int nc = n * C + j % C;
    const f32x4 xv = ldf4(x, i), mv = ldf4(m, nc), av = ldf4(a, nc), bv = ldf4(b, nc);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = apply_act((xv[k] - mv[k]) * av[k] + bv[k], act, slope);
    if constexpr (RES) o += ldf4(res, i);
    *reinterpret_cast<f32x4*>(y + i) = o;
  }
}

// backward partial: part[(n*S + s)*C + c] = {sum g, sum g * xh}, g = dy * act'((x - m) * a + b), xh = (x - m) * r_c
__global__ __launch_bounds__(256) void bn_bwd_partial(const float* __restrict__ x, const float* __restrict__ dy,
                                                      const float* __restrict__ m, const float* __restrict__ a,
                                                      const float* __restrict__ b, const float* __restrict__ rstd,
                                                      float2* __restrict__ part, int HW, int C, int S, int rps, int act,
                                                      float slope) {
  const int q = threadIdx.x & 7, ty = threadIdx.x >> 3;
  const int c = blockIdx.x * BN_CH + q * 4;
  const int s = blockIdx.y, n = blockIdx.z;
  const int r0 = s * rps, r1 = min(HW, r0 + rps);
  __shared__ f32x4 sh[2][32][8];
  f32x4 sg = {0.f, 0.f, 0.f, 0.f}, sgx = {0.f, 0.f, 0.f, 0.f};
  if (c < C && r0 < r1) {
    const int nc = n * C + c;
    const f32x4 mv = ldf4(m, nc), av = ldf4(a, nc), bv = ldf4(b, nc), rv = ldf4(rstd, c);
    const size_t base = (size_t)n * HW * C + c;
    for (int r = r0 + ty; r < r1; r += 32) {
      const size_t o = base + (size_t)r * C;
      const f32x4 d = ldf4(x, o) - mv, gy = ldf4(dy, o);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float g = gy[k] * act_grad(d[k] * av[k] + bv[k], act, slope);
        sg[k] += g;
        sgx[k] += g * (d[k] * rv[k]);
      }
    }
  }
  sh[0][ty][q] = sg;
  sh[1][ty][q] = sgx;
  __syncthreads();
  if (threadIdx.x < BN_CH) {
    const int cc = threadIdx.x, qq = cc >> 2, e = cc & 3;
    const int ch = blockIdx.x * BN_CH + cc;
    if (ch < C) {
      float ta = 0.f, tb = 0.f;
#pragma unroll 8
      for (int i = 0; i < 32; ++i) { ta += sh[0][i][qq][e]; tb += sh[1][i][qq][e]; }
      part[((size_t)n * S + s) * C + ch] = make_float2(ta, tb);
    }
  }
}

// one WAVE per channel, its lanes over the images: the parameter gradients and the dx coefficients,
// dx = alpha[n,c] * g + k[n,c] + delta[c] * xb, xb = (x - mean_c) * r_c.
//   CBB: alpha = a = r_c * scale (the forward-time affine, as the reference's weight.repeat(b) copy);
//        dshift / dscale per (n, c); k = -alpha * dshift / HW; delta = -r_c * sum_n scale * dscale / M.
//   BN : alpha = weight[c] * r_c with the weight read NOW (nn.BatchNorm2d's autograd holds it by reference: the stale-graph
//        rule of the convolutions); dbeta / dgamma per channel; k = -alpha * dbeta / M; delta = -alpha * dgamma / M.
//   Eval statistics: the batch terms vanish.
//   SYNC: the sums over the batch that enter dx (k, delta) run over the N images of the global batch, in the one-process order;
//        the parameter gradients stay sums over THIS rank's images [n0, n0 + Nl) (dp.GradReducer averages them over the ranks,
//        and every rank's loss is a mean over its own rows).  CBB's delta needs the other ranks' scale: it travels in the
//        exchange buffer behind the partials, and the product scale * dscale is formed here exactly as one process forms it.
template <bool SYNC>
__device__ __forceinline__ void bn_bwd_combine_body(const float2* __restrict__ part, const float* __restrict__ scale,
                                                    const float* __restrict__ weight, const float* __restrict__ a,
                                                    const float* __restrict__ rstd, float* __restrict__ dscale,
                                                    float* __restrict__ dshift, float* __restrict__ alpha,
                                                    float* __restrict__ kcoef, float* __restrict__ delta, int N, int HW,
                                                    int C, int S, int cbb, int batch_stats, int n0, int Nl, size_t chunk) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  const float M = (float)N * (float)HW;
  float sg = 0.f, sgx = 0.f, T = 0.f, lg = 0.f, lgx = 0.f;
  for (int n = lane; n < N; n += 64) {
    const float2* row = part_row<SYNC>(part, n, S, C, Nl, chunk);
    float tg = 0.f, tgx = 0.f;
    for (int s = 0; s < S; ++s) {
      const float2 p = row[(size_t)s * C + c];
      tg += p.x;
      tgx += p.y;
    }
    const bool mine = n >= n0 && n < n0 + Nl;
    if (cbb) {
      if (mine) {
        const int nc = (n - n0) * C + c;
        dshift[nc] = tg;
        dscale[nc] = tgx;
        alpha[nc] = a[nc];
        kcoef[nc] = -a[nc] * (tg / (float)HW);
      }
      float sc;
      if constexpr (SYNC)      // the scale rows behind the chunk's partials
        sc = (reinterpret_cast<const float*>(part) + (size_t)(n / Nl) * chunk + (size_t)Nl * S * C * 2)[(size_t)(n % Nl) * C + c];
      else
        sc = scale[n * C + c];
      T += sc * tgx;
    } else {
      sg += tg;
      sgx += tgx;
      if (SYNC && mine) {
        lg += tg;
        lgx += tgx;
      }
    }
  }
  if (cbb) {
    T = wave_sum_down(T);
    if (lane == 0) delta[c] = batch_stats ? -rstd[c] * (T / M) : 0.f;
    return;
  }
  sg = __shfl(wave_sum_down(sg), 0, 64);
  sgx = __shfl(wave_sum_down(sgx), 0, 64);
  if constexpr (SYNC) {
    lg = wave_sum_down(lg);
    lgx = wave_sum_down(lgx);
  } else {
    lg = sg;
    lgx = sgx;
  }
  const float ac = weight ? weight[c] * rstd[c] : rstd[c];      // the same for every image
  if (lane == 0) {
    dshift[c] = lg;
    dscale[c] = lgx;
    delta[c] = batch_stats ? -ac * (sgx / M) : 0.f;
  }
  for (int n = lane; n < Nl; n += 64) {
    alpha[n * C + c] = ac;
    kcoef[n * C + c] = batch_stats ? -ac * (sg / M) : 0.f;
  }
}

__global__ __launch_bounds__(256) void bn_bwd_combine(const float2* __restrict__ part, const float* __restrict__ scale,
                                                      const float* __restrict__ weight, const float* __restrict__ a,
                                                      const float* __restrict__ rstd, float* __restrict__ dscale,
                                                      float* __restrict__ dshift, float* __restrict__ alpha,
                                                      float* __restrict__ kcoef, float* __restrict__ delta, int N, int HW,
                                                      int C, int S, int cbb, int batch_stats) {
  bn_bwd_combine_body<false>(part, scale, weight, a, rstd, dscale, dshift, alpha, kcoef, delta, N, HW, C, S, cbb, batch_stats, 0, N,
                             0);
}

__global__ __launch_bounds__(256) void bn_sync_bwd_combine(const float2* __restrict__ part, const float* __restrict__ weight,
                                                           const float* __restrict__ a, const float* __restrict__ rstd,
                                                           float* __restrict__ dscale, float* __restrict__ dshift,
                                                           float* __restrict__ alpha, float* __restrict__ kcoef,
                                                           float* __restrict__ delta, int N, int HW, int C, int S, int cbb,
                                                           int n0, int Nl, size_t chunk) {
  bn_bwd_combine_body<true>(part, nullptr, weight, a, rstd, dscale, dshift, alpha, kcoef, delta, N, HW, C, S, cbb, 1, n0, Nl, chunk);
}

// CBB backward, phase 1: this rank's scale rows [Nl][C] into its chunk of the exchange buffer (four channels per lane)
__global__ __launch_bounds__(256) void bn_sync_pack_scale(const float* __restrict__ scale, float* __restrict__ dst, int count) {
  const int i = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i < count) *reinterpret_cast<f32x4*>(dst + i) = ldf4(scale, i);
}

// the activation mask from the forward's own coefficients (m, a, b); the linear part from the combine's (alpha, k, delta)
__global__ __launch_bounds__(256) void bn_bwd_dx(const float* __restrict__ x, const float* __restrict__ dy,
                                                 const float* __restrict__ m, const float* __restrict__ a,
                                                 const float* __restrict__ b, const float* __restrict__ mean,
                                                 const float* __restrict__ rstd, const float* __restrict__ alpha,
                                                 const float* __restrict__ kcoef, const float* __restrict__ delta,
                                                 float* __restrict__ dx, int HWC, int C, int act, float slope) {
  const int n = blockIdx.y;
  const size_t base = (size_t)n * HWC;
  for (int j = (blockIdx.x * blockDim.x + threadIdx.x) * 4; j < HWC; j += gridDim.x * blockDim.x * 4) {
    const size_t i = base + j;
    const int c = j % C;
    const int nc = n * C + c;
    const f32x4 xv = ldf4(x, i), gy = ldf4(dy, i), mv = ldf4(m, nc), av = ldf4(a, nc), bv = ldf4(b, nc);
    const f32x4 al = ldf4(alpha, nc), kv = ldf4(kcoef, nc), mu = ldf4(mean, c), rs = ldf4(rstd, c), dl = ldf4(delta, c);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float g = gy[k] * act_grad((xv[k] - mv[k]) * av[k] + bv[k], act, slope);
      o[k] = al[k] * g + kv[k] + dl[k] * ((xv[k] - mu[k]) * rs[k]);
    }
    *reinterpret_cast<f32x4*>(dx + i) = o;
  }
}

// workgroups per image of the streaming passes: one float4 per lane if that takes fewer, ~2048 over the batch otherwise
dim3 stream_grid(int N, int HWC) {
  const long long per_image = ceil_div(HWC / 4, 256);
  const long long want = std::max(1, 2048 / N);
  return dim3((unsigned)std::max<long long>(1, std::min(per_image, want)), (unsigned)N);
}

const char* bn_check(const char* what, const float* x, const float* y, const float* mean, const float* rstd, const float* m,
                     const float* a, const float* b, const float* rmean, const float* rvar, const long long* nbt, int N,
                     int HW, int C, int training, int cumulative, const void* ws, size_t ws_bytes) {
  (void)what;
  if (!x || !y || !mean || !rstd || !m || !a || !b) return "null pointer";
  if (N <= 0 || HW <= 0 || C <= 0) return "bad shape";
  if (C % 4) return "C % 4 != 0 (channels are read four at a time)";
  if ((long long)HW * C >= (1LL << 31) || N > 65535) return "image too large (HW * C >= 2^31 or N > 65535)";
  if ((rmean == nullptr) != (rvar == nullptr)) return "running_mean and running_var go together";
  if (training && (long long)N * HW <= 1) return "Expected more than 1 value per channel when training";
  if (!training && !rmean) return "eval mode without running statistics";
  if (training && rmean && cumulative && !nbt) return "momentum=None needs num_batches_tracked";
  if (!ws || ws_bytes < srgan_batchnorm_workspace(N, HW, C)) return "workspace too small";
  return nullptr;
}

int bn_forward(const char* what, int cbb, const float* x, const float* scale, const float* shift, const float* res, float* y,
               float* mean, float* rstd, float* m, float* a, float* b, float* rmean, float* rvar, long long* nbt, int N,
               int HW, int C, int training, float momentum, int cumulative, float eps, int act, float slope, void* ws,
               size_t ws_bytes, void* stream) {
  const char* err = bn_check(what, x, y, mean, rstd, m, a, b, rmean, rvar, nbt, N, HW, C, training, cumulative, ws, ws_bytes);
  SRGAN_REQUIRE(!err, "%s: %s", what, err);
  if (cbb) SRGAN_REQUIRE(scale && shift, "%s: null pointer (scale / shift)", what);
  else SRGAN_REQUIRE((scale == nullptr) == (shift == nullptr), "%s: weight and bias go together", what);
  hipStream_t st = as_stream(stream);
  int S, rps;
  bn_plan(N, HW, C, S, rps);
  float2* part = reinterpret_cast<float2*>(ws);
  const bool need_pass = training || cbb;    // eval-mode BN needs no statistics of x
  if (need_pass)
    hipLaunchKernelGGL(bn_stats_partial, dim3((unsigned)ceil_div(C, BN_CH), (unsigned)S, (unsigned)N), dim3(256), 0, st, x, part,
                       HW, C, S, rps);
  const int update = training && rmean != nullptr;
  hipLaunchKernelGGL(bn_finalize, dim3((unsigned)ceil_div(C, 4)), dim3(256), 0, st, need_pass ? (const float2*)part : nullptr, scale, shift, mean, rstd,
                     m, a, b, rmean, rvar, nbt, N, HW, C, S, rps, cbb, training, update, momentum, cumulative, eps);
  long long* count = update ? nbt : nullptr;
  if (res)
    hipLaunchKernelGGL(bn_apply<true>, stream_grid(N, HW * C), dim3(256), 0, st, x, m, a, b, res, y, HW * C, C, act, slope, count);
  else
    hipLaunchKernelGGL(bn_apply<false>, stream_grid(N, HW * C), dim3(256), 0, st, x, m, a, b, res, y, HW * C, C, act, slope, count);
  return check_launch(what);
}

int bn_backward(const char* what, int cbb, const float* x, const float* dy, const float* scale, const float* weight,
                const float* mean, const float* rstd, const float* m, const float* a, const float* b, float* dx, float* dscale,
                float* dshift, int N, int HW, int C, int training, int act, float slope, void* ws, size_t ws_bytes,
                void* stream) {
  SRGAN_REQUIRE(x && dy && mean && rstd && m && a && b && dx && dscale && dshift, "%s: null pointer", what);
  SRGAN_REQUIRE(!cbb || scale, "%s: null pointer (scale)", what);
  SRGAN_REQUIRE(N > 0 && HW > 0 && C > 0, "%s: bad shape", what);
  SRGAN_REQUIRE(C % 4 == 0, "%s: C %% 4 != 0 (channels are read four at a time)", what);
  SRGAN_REQUIRE((long long)HW * C < (1LL << 31) && N <= 65535, "%s: image too large (HW * C >= 2^31 or N > 65535)", what);
  SRGAN_REQUIRE(!training || (long long)N * HW > 1, "%s: Expected more than 1 value per channel when training", what);
  SRGAN_REQUIRE(ws && ws_bytes >= srgan_batchnorm_workspace(N, HW, C), "%s: workspace too small", what);
  hipStream_t st = as_stream(stream);
  int S, rps;
  bn_plan(N, HW, C, S, rps);
  float2* part = reinterpret_cast<float2*>(ws);
  float* alpha = reinterpret_cast<float*>(static_cast<char*>(ws) + bn_part_bytes(N, HW, C));
  float* kcoef = alpha + (size_t)N * C;
  float* delta = kcoef + (size_t)N * C;
  hipLaunchKernelGGL(bn_bwd_partial, dim3((unsigned)ceil_div(C, BN_CH), (unsigned)S, (unsigned)N), dim3(256), 0, st, x, dy, m, a,
                     b, rstd, part, HW, C, S, rps, act, slope);
  hipLaunchKernelGGL(bn_bwd_combine, dim3((unsigned)ceil_div(C, 4)), dim3(256), 0, st, (const float2*)part, scale, weight, a, rstd,
                     dscale, dshift, alpha, kcoef, delta, N, HW, C, S, cbb, training);
  hipLaunchKernelGGL(bn_bwd_dx, stream_grid(N, HW * C), dim3(256), 0, st, x, dy, m, a, b, mean, rstd, (const float*)alpha,
                     (const float*)kcoef, (const float*)delta, dx, HW * C, C, act, slope);
  return check_launch(what);
}

// ---- data parallel: the same passes split around the all-gathers of the per-image partials -------------------------------
struct SyncPlan {
  int S, rps;
  size_t chunk;      // floats per rank chunk of the exchange buffer
  size_t bytes;      // the whole buffer: N / Nl chunks
};

// plan of the GLOBAL batch (bn_plan(N_local, ...) may give another S); with_scale: CBB backward (the chunk ends in [Nl][C] scale rows)
const char* sync_plan(int N, int n0, int Nl, int HW, int C, int with_scale, SyncPlan& p) {
  if (N <= 0 || Nl <= 0 || HW <= 0 || C <= 0) return "bad shape";
  if (C % 4) return "C % 4 != 0 (channels are read four at a time)";
  if (Nl > N) return "N_local > N_global";
  if (N % Nl) return "N_global is not a multiple of N_local (every rank holds the same number of images)";
  if (n0 < 0 || n0 + Nl > N || n0 % Nl) return "rank offset outside the global batch (n0 = rank * N_local)";
  if ((long long)HW * C >= (1LL << 31) || N > 65535) return "image too large (HW * C >= 2^31 or N > 65535)";
  if ((long long)N * HW <= 1) return "Expected more than 1 value per channel when training";
  bn_plan(N, HW, C, p.S, p.rps);
  p.chunk = (size_t)Nl * ((size_t)p.S * C * 2 + (with_scale ? (size_t)C : 0));
  p.bytes = (size_t)(N / Nl) * p.chunk * sizeof(float);
  return nullptr;
}

// this rank's chunk, as the [Nl][S][C] partial rows the slab passes write
float2* sync_chunk(void* xbuf, const SyncPlan& p, int n0, int Nl) {
  return reinterpret_cast<float2*>(static_cast<float*>(xbuf) + (size_t)(n0 / Nl) * p.chunk);
}

int bn_sync_fwd_partial(const char* what, const float* x, void* xbuf, size_t xbuf_bytes, int N, int n0, int Nl, int HW, int C,
                        void* stream) {
  SyncPlan p;
  const char* err = sync_plan(N, n0, Nl, HW, C, 0, p);
  SRGAN_REQUIRE(!err, "%s: %s", what, err);
  SRGAN_REQUIRE(x && xbuf, "%s: null pointer", what);
  SRGAN_REQUIRE(xbuf_bytes >= p.bytes, "%s: exchange buffer too small (it holds the partials of the GLOBAL batch)", what);
  hipLaunchKernelGGL(bn_stats_partial, dim3((unsigned)ceil_div(C, BN_CH), (unsigned)p.S, (unsigned)Nl), dim3(256), 0,
                     as_stream(stream), x, sync_chunk(xbuf, p, n0, Nl), HW, C, p.S, p.rps);
  return check_launch(what);
}

int bn_sync_fwd_apply(const char* what, int cbb, const float* x, const float* scale, const float* shift, const float* res,
                      float* y, float* mean, float* rstd, float* m, float* a, float* b, float* rmean, float* rvar,
                      long long* nbt, const void* xbuf, size_t xbuf_bytes, int N, int n0, int Nl, int HW, int C, float momentum,
                      int cumulative, float eps, int act, float slope, void* stream) {
  SyncPlan p;
  const char* err = sync_plan(N, n0, Nl, HW, C, 0, p);
  SRGAN_REQUIRE(!err, "%s: %s", what, err);
  SRGAN_REQUIRE(x && y && mean && rstd && m && a && b && xbuf, "%s: null pointer", what);
  SRGAN_REQUIRE((rmean == nullptr) == (rvar == nullptr), "%s: running_mean and running_var go together", what);
  SRGAN_REQUIRE(!(rmean && cumulative && !nbt), "%s: momentum=None needs num_batches_tracked", what);
  if (cbb) SRGAN_REQUIRE(scale && shift, "%s: null pointer (scale / shift)", what);
  else SRGAN_REQUIRE((scale == nullptr) == (shift == nullptr), "%s: weight and bias go together", what);
  SRGAN_REQUIRE(xbuf_bytes >= p.bytes, "%s: exchange buffer too small (it holds the partials of the GLOBAL batch)", what);
  hipStream_t st = as_stream(stream);
  const int update = rmean != nullptr;
  hipLaunchKernelGGL(bn_sync_finalize, dim3((unsigned)ceil_div(C, 4)), dim3(256), 0, st, static_cast<const float2*>(xbuf), scale,
                     shift, mean, rstd, m, a, b, rmean, rvar, nbt, N, HW, C, p.S, p.rps, cbb, update, momentum, cumulative, eps, n0,
                     Nl, p.chunk);
  long long* count = update ? nbt : nullptr;
  if (res)
    hipLaunchKernelGGL(bn_apply<true>, stream_grid(Nl, HW * C), dim3(256), 0, st, x, m, a, b, res, y, HW * C, C, act, slope, count);
  else
    hipLaunchKernelGGL(bn_apply<false>, stream_grid(Nl, HW * C), dim3(256), 0, st, x, m, a, b, res, y, HW * C, C, act, slope, count);
  return check_launch(what);
}

int bn_sync_bwd_partial(const char* what, const float* x, const float* dy, const float* scale, const float* rstd, const float* m,
                        const float* a, const float* b, void* xbuf, size_t xbuf_bytes, int N, int n0, int Nl, int HW, int C,
                        int act, float slope, void* stream) {
  SyncPlan p;
  const char* err = sync_plan(N, n0, Nl, HW, C, scale != nullptr, p);
  SRGAN_REQUIRE(!err, "%s: %s", what, err);
  SRGAN_REQUIRE(x && dy && rstd && m && a && b && xbuf, "%s: null pointer", what);
  SRGAN_REQUIRE(xbuf_bytes >= p.bytes, "%s: exchange buffer too small (it holds the partials of the GLOBAL batch)", what);
  hipStream_t st = as_stream(stream);
  float2* mine = sync_chunk(xbuf, p, n0, Nl);
  hipLaunchKernelGGL(bn_bwd_partial, dim3((unsigned)ceil_div(C, BN_CH), (unsigned)p.S, (unsigned)Nl), dim3(256), 0, st, x, dy, m, a, b,
                     rstd, mine, HW, C, p.S, p.rps, act, slope);
  if (scale)
    hipLaunchKernelGGL(bn_sync_pack_scale, dim3((unsigned)ceil_div((long long)Nl * C / 4, 256)), dim3(256), 0, st, scale,
                       reinterpret_cast<float*>(mine) + (size_t)Nl * p.S * C * 2, Nl * C);
  return check_launch(what);
}

int bn_sync_bwd_apply(const char* what, int cbb, const float* x, const float* dy, const float* weight, const float* mean,
                      const float* rstd, const float* m, const float* a, const float* b, const void* xbuf, size_t xbuf_bytes,
                      float* dx, float* dscale, float* dshift, int N, int n0, int Nl, int HW, int C, int act, float slope, void* ws,
                      size_t ws_bytes, void* stream) {
  SyncPlan p;
  const char* err = sync_plan(N, n0, Nl, HW, C, cbb, p);
  SRGAN_REQUIRE(!err, "%s: %s", what, err);
  SRGAN_REQUIRE(x && dy && mean && rstd && m && a && b && dx && dscale && dshift && xbuf, "%s: null pointer", what);
  SRGAN_REQUIRE(xbuf_bytes >= p.bytes, "%s: exchange buffer too small (it holds the partials of the GLOBAL batch)", what);
  SRGAN_REQUIRE(ws && ws_bytes >= srgan_batchnorm_sync_workspace(Nl, C), "%s: workspace too small", what);
  hipStream_t st = as_stream(stream);
  float* alpha = static_cast<float*>(ws);
  float* kcoef = alpha + (size_t)Nl * C;
  float* delta = kcoef + (size_t)Nl * C;
  hipLaunchKernelGGL(bn_sync_bwd_combine, dim3((unsigned)ceil_div(C, 4)), dim3(256), 0, st, static_cast<const float2*>(xbuf), weight,
                     a, rstd, dscale, dshift, alpha, kcoef, delta, N, HW, C, p.S, cbb, n0, Nl, p.chunk);
  hipLaunchKernelGGL(bn_bwd_dx, stream_grid(Nl, HW * C), dim3(256), 0, st, x, dy, m, a, b, mean, rstd, (const float*)alpha,
                     (const float*)kcoef, (const float*)delta, dx, HW * C, C, act, slope);
  return check_launch(what);
}

}  // namespace
}  // namespace srgan

using namespace srgan;

extern "C" size_t srgan_batchnorm_workspace(int N, int HW, int C) {
  if (N <= 0 || HW <= 0 || C <= 0) return 0;
  return bn_part_bytes(N, HW, C) + (2 * (size_t)N * C + (size_t)C) * sizeof(float);
}

extern "C" int srgan_batchnorm_fwd(const float* x, const float* weight, const float* bias, float* y, float* mean, float* rstd,
                                   float* m, float* a, float* b, float* running_mean, float* running_var,
                                   long long* num_batches_tracked, int N, int HW, int C, int training, float momentum,
                                   int cumulative, float eps, int act, float slope, void* ws, size_t ws_bytes, void* stream) {
  return bn_forward("batchnorm_fwd", 0, x, weight, bias, nullptr, y, mean, rstd, m, a, b, running_mean, running_var,
                    num_batches_tracked, N, HW, C, training, momentum, cumulative, eps, act, slope, ws, ws_bytes, stream);
}

extern "C" int srgan_cbbnorm_fwd(const float* x, const float* scale, const float* shift, const float* res, float* y, float* mean,
                                 float* rstd, float* m, float* a, float* b, float* running_mean, float* running_var,
                                 long long* num_batches_tracked, int N, int HW, int C, int training, float momentum,
                                 int cumulative, float eps, int act, float slope, void* ws, size_t ws_bytes, void* stream) {
  return bn_forward("cbbnorm_fwd", 1, x, scale, shift, res, y, mean, rstd, m, a, b, running_mean, running_var,
                    num_batches_tracked, N, HW, C, training, momentum, cumulative, eps, act, slope, ws, ws_bytes, stream);
}

extern "C" int srgan_batchnorm_bwd(const float* x, const float* dy, const float* weight, const float* mean, const float* rstd,
                                   const float* m, const float* a, const float* b, float* dx, float* dweight, float* dbias, int N,
                                   int HW, int C, int training, int act, float slope, void* ws, size_t ws_bytes, void* stream) {
  return bn_backward("batchnorm_bwd", 0, x, dy, nullptr, weight, mean, rstd, m, a, b, dx, dweight, dbias, N, HW, C, training, act,
                     slope, ws, ws_bytes, stream);
}

extern "C" int srgan_cbbnorm_bwd(const float* x, const float* dy, const float* scale, const float* mean, const float* rstd,
                                 const float* m, const float* a, const float* b, float* dx, float* dscale, float* dshift, int N,
                                 int HW, int C, int training, int act, float slope, void* ws, size_t ws_bytes, void* stream) {
  return bn_backward("cbbnorm_bwd", 1, x, dy, scale, nullptr, mean, rstd, m, a, b, dx, dscale, dshift, N, HW, C, training, act, slope, ws,
                     ws_bytes, stream);
}

// ---- data parallel: statistics of the global batch (include/srgan_hip.h) ---------------------------------------------------
extern "C" size_t srgan_batchnorm_sync_exchange_bytes(int N_global, int N_local, int HW, int C, int with_scale) {
  SyncPlan p;
  return sync_plan(N_global, 0, N_local, HW, C, with_scale, p) ? 0 : p.bytes;
}

extern "C" size_t srgan_batchnorm_sync_workspace(int N_local, int C) {
  if (N_local <= 0 || C <= 0) return 0;
  return (2 * (size_t)N_local * C + (size_t)C) * sizeof(float);
}

extern "C" int srgan_batchnorm_sync_fwd_partial(const float* x, void* xbuf, size_t xbuf_bytes, int N_global, int n0, int N_local,
                                                int HW, int C, void* stream) {
  return bn_sync_fwd_partial("batchnorm_sync_fwd_partial", x, xbuf, xbuf_bytes, N_global, n0, N_local, HW, C, stream);
}

extern "C" int srgan_batchnorm_sync_fwd_apply(const float* x, const float* weight, const float* bias, float* y, float* mean,
                                              float* rstd, float* m, float* a, float* b, float* running_mean, float* running_var,
                                              long long* num_batches_tracked, const void* xbuf, size_t xbuf_bytes, int N_global,
                                              int n0, int N_local, int HW, int C, float momentum, int cumulative, float eps, int act,
                                              float slope, void* stream) {
  return bn_sync_fwd_apply("batchnorm_sync_fwd_apply", 0, x, weight, bias, nullptr, y, mean, rstd, m, a, b, running_mean, running_var,
                           num_batches_tracked, xbuf, xbuf_bytes, N_global, n0, N_local, HW, C, momentum, cumulative, eps, act, slope,
                           stream);
}

extern "C" int srgan_cbbnorm_sync_fwd_apply(const float* x, const float* scale, const float* shift, const float* res, float* y,
                                            float* mean, float* rstd, float* m, float* a, float* b, float* running_mean,
                                            float* running_var, long long* num_batches_tracked, const void* xbuf, size_t xbuf_bytes,
                                            int N_global, int n0, int N_local, int HW, int C, float momentum, int cumulative,
                                            float eps, int act, float slope, void* stream) {
  return bn_sync_fwd_apply("cbbnorm_sync_fwd_apply", 1, x, scale, shift, res, y, mean, rstd, m, a, b, running_mean, running_var,
                           num_batches_tracked, xbuf, xbuf_bytes, N_global, n0, N_local, HW, C, momentum, cumulative, eps, act, slope,
                           stream);
}

extern "C" int srgan_batchnorm_sync_bwd_partial(const float* x, const float* dy, const float* scale, const float* rstd,
                                                const float* m, const float* a, const float* b, void* xbuf, size_t xbuf_bytes,
                                                int N_global, int n0, int N_local, int HW, int C, int act, float slope,
                                                void* stream) {
  return bn_sync_bwd_partial("batchnorm_sync_bwd_partial", x, dy, scale, rstd, m, a, b, xbuf, xbuf_bytes, N_global, n0, N_local, HW,
                             C, act, slope, stream);
}

extern "C" int srgan_batchnorm_sync_bwd_apply(const float* x, const float* dy, const float* weight, const float* mean,
                                              const float* rstd, const float* m, const float* a, const float* b, const void* xbuf,
                                              size_t xbuf_bytes, float* dx, float* dweight, float* dbias, int N_global, int n0,
                                              int N_local, int HW, int C, int act, float slope, void* ws, size_t ws_bytes,
                                              void* stream) {
  return bn_sync_bwd_apply("batchnorm_sync_bwd_apply", 0, x, dy, weight, mean, rstd, m, a, b, xbuf, xbuf_bytes, dx, dweight, dbias,
                           N_global, n0, N_local, HW, C, act, slope, ws, ws_bytes, stream);
}

extern "C" int srgan_cbbnorm_sync_bwd_apply(const float* x, const float* dy, const float* mean, const float* rstd, const float* m,
                                            const float* a, const float* b, const void* xbuf, size_t xbuf_bytes, float* dx,
                                            float* dscale, float* dshift, int N_global, int n0, int N_local, int HW, int C, int act,
                                            float slope, void* ws, size_t ws_bytes, void* stream) {
  return bn_sync_bwd_apply("cbbnorm_sync_bwd_apply", 1, x, dy, nullptr, mean, rstd, m, a, b, xbuf, xbuf_bytes, dx, dscale, dshift,
                           N_global, n0, N_local, HW, C, act, slope, ws, ws_bytes, stream);
}
