// Structural similarity (Wang et al. 2004) of two fp32 NHWC-dense images with 1..3 channels, as a loss term with its gradient and
// as a metric, and PSNR.  Extension, no counterpart in the reference.  DESIGN.md section 7 ("Structural similarity") has the
// definition and the bound; csrc/ssim_math.h the arithmetic; srgan_amd/structural.py owns the record.
//
// Valid positions only: Ho x Wo = (H - window + 1) x (W - window + 1) per plane.  Every windowed moment is taken of SHIFTED values
// x - p, y - q with one pivot per (sample, channel, image): that plane's pixel (0, 0).  The variances are differences of numbers of
// the size of the local contrast then, not of the size of the signal (raw fp32 moments lose 1e-4 of a map value on a flat image
// near +-1; the shifted ones stay at 2e-7).  Forward and gradient use the same pivot.
//
//   ssim_map_kernel     one workgroup per (sample, tile of 8 x 32 valid positions), all channels.  The two (8 + window - 1) x
//                       (32 + window - 1) x C input tiles go to LDS shifted (a row of the tile is ONE contiguous run of the NHWC
//                       image: 16-byte loads on the run's 16-byte grid, 4-byte loads for the head and the tail left over), a row
//                       pass writes the five moments of every tile row to LDS, a column pass ends them.  In both passes the lanes of a
//                       wave read consecutive floats of one tile row (the channel is the fastest index and a tap moves by C floats):
//                       no two lanes of a group share a bank whatever the strides are.  Taps ascending, one accumulator per moment, no
//                       contraction.  A thread owns positions tid, tid + 256, ... of the tile (row-major, channel fastest) and adds
//                       their values ascending; the 64 lanes by the xor butterfly (32 ... 1); (w0 + w1) + (w2 + w3) -> part[wg].
//                       A position outside the valid extent adds +0 (a select).  With a gradient wanted it also stores the
//                       coefficient maps g_sxy, g_s and A_x = g_mux - 2 g_s (mu_x - p) - g_sxy (mu_y - q) (and / or A_y).
//   ssim_finish_kernel  one workgroup, float64: per sample the tile partials (thread t adds tiles t, t + 256, ... ascending, then a
//                       fixed LDS tree), value_n = sum / (Ho Wo C); term = 1 - (sum_n value_n ascending) / N; the per-sample values,
//                       {weight * term, term} and the record's last values and count.
//   ssim_grad_kernel    one workgroup per (sample, tile of 8 x 32 INPUT pixels): the adjoint of the valid filter as a gather.  Per
//                       coefficient map: the tile with its window - 1 halo to LDS (zero outside the valid extent), a row and a column
//                       pass with the taps reversed.  dx = k (T[A_x] + 2 (x - p) T[g_s] + (y - q) T[g_sxy]), dy likewise, k = -weight *
//                       g / (N Ho Wo C) -- the gradient of weight * (1 - mean SSIM) times the incoming one.  Plain stores.
//   psnr_rows_kernel    partial sums of (x - y)^2 over 4096 floats of one sample; psnr_finish_kernel adds them in float64.
//
// No atomics; every sum has one owner and a fixed order, so a replayed hipGraph gives the eager bits.
#include "common.h"
#include "records.h"
#include "ssim_math.h"
#include <algorithm>
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace srgan {

constexpr int kSsBlock = 256;
constexpr int kSsTH = 8, kSsTW = 32;                          // the tile: rows x columns (valid positions / input pixels)
constexpr int kSsMaxC = 3;
constexpr int kSsInH = kSsTH + kSsMaxWindow - 1;              // 18
constexpr int kSsInW = kSsTW + kSsMaxWindow - 1;              // 42: at C = 3 a tile with its halo is 2268 floats per image,
                                                              // a moment after the row pass 18 x 96 = 1728 -> 52.7 KB of LDS
constexpr int kPsnrChunk = 4096;

struct SsMapParams {
  const float* x; const float* y;
  float* part;
  float* m_sxy; float* m_s; float* m_ax; float* m_ay;          // coefficient maps [N, Ho, Wo, C]; NULL: not wanted
  const SsState* st;
  float c1, c2;                                                // used when st == NULL
  SsTaps taps;
  int h, w, ho, wo, tiles_x, tiles;
};

struct SsGradParams {
  const float* x; const float* y;
  const float* m_sxy; const float* m_s; const float* m_ax; const float* m_ay;
  const SsState* st; const float* g;
  float* dx; float* dy;
  SsTaps taps;
  int h, w, ho, wo, tiles_x, tiles;
  double count;                                                // N Ho Wo C
};

// The rows_all x S floats of a tile into LDS, `piv[channel]` subtracted.  Float e of tile row r is float g0 + r * grs + e of `base`;
// rows [r_lo, r_hi) and floats [e_lo, e_hi) of a row exist (g0 may point in front of a row that starts outside), everything else
// reads 0.  A quad is four floats on the 16-byte grid of global memory: one 16-byte load where all four exist, 4-byte loads else.
template <int C>
__device__ __forceinline__ void ss_load_tile(float* __restrict__ lds, const float* __restrict__ base, long long g0, long long grs,
                                             int r_lo, int r_hi, int e_lo, int e_hi, int rows_all, int S, const float (&piv)[C]) {
  const int nq = (S + 6) >> 2;                                 // quads of a row, whatever its alignment
  for (int it = threadIdx.x; it < rows_all * nq; it += kSsBlock) {
    const int r = it / nq, q = it - r * nq;
    const long long gr = g0 + (long long)r * grs;
    const int s = (int)(((reinterpret_cast<uintptr_t>(base) >> 2) + (unsigned long long)gr) & 3);
    const int e0 = 4 * q - s;
    const bool row = r >= r_lo && r < r_hi;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (row && e0 >= e_lo && e0 + 4 <= e_hi) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(base + (gr + e0));
      v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = v[k] - piv[(e0 + k) % C];
    } else if (row) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = e0 + k;
        if (e >= e_lo && e < e_hi) v[k] = base[gr + e] - piv[e % C];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = e0 + k;
      if (e >= 0 && e < S) lds[r * S + e] = v[k];
    }
  }
}

template <int C>
__global__ __launch_bounds__(kSsBlock) void ssim_map_kernel(SsMapParams p) {
  constexpr int TWC = kSsTW * C;
  __shared__ float sa[kSsInH * kSsInW * C];
  __shared__ float sb[kSsInH * kSsInW * C];
  __shared__ float rowm[5][kSsInH * TWC];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int n = blockIdx.x / p.tiles, t = blockIdx.x - n * p.tiles;
  const int ty = t / p.tiles_x, tx = t - ty * p.tiles_x;
  const int y0 = ty * kSsTH, x0 = tx * kSsTW;
  const int win = p.taps.n;
  const int rows_all = kSsTH + win - 1, S = (kSsTW + win - 1) * C;
  const long long grs = (long long)p.w * C;
  const long long plane = (long long)n * p.h * grs;
  float px[C], py[C];
#pragma unroll
  for (int c = 0; c < C; ++c) { px[c] = p.x[plane + c]; py[c] = p.y[plane + c]; }      // the pivots: pixel (0, 0) of the plane
  const float c1 = p.st ? p.st->c1 : p.c1, c2 = p.st ? p.st->c2 : p.c2;

  const long long g0 = plane + (long long)y0 * grs + (long long)x0 * C;
  const int rows_in = min(rows_all, p.h - y0), e_hi = min(S, (p.w - x0) * C);
  ss_load_tile<C>(sa, p.x, g0, grs, 0, rows_in, 0, e_hi, rows_all, S, px);
  ss_load_tile<C>(sb, p.y, g0, grs, 0, rows_in, 0, e_hi, rows_all, S, py);
  __syncthreads();

  // row pass: the five moments of every tile row at the TWC output floats of the row
  for (int it = tid; it < rows_all * TWC; it += kSsBlock) {
    const int r = it / TWC, j = it - r * TWC;
    const float* a = sa + r * S + j;
    const float* b = sb + r * S + j;
    float m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f, m5 = 0.f;
    for (int k = 0; k < win; ++k) {
      const float wk = p.taps.w[k], u = a[k * C], v = b[k * C];
      m1 += wk * u; m2 += wk * v; m3 += wk * (u * u); m4 += wk * (v * v); m5 += wk * (u * v);
    }
    rowm[0][it] = m1; rowm[1][it] = m2; rowm[2][it] = m3; rowm[3][it] = m4; rowm[4][it] = m5;
  }
  __syncthreads();

  // column pass, the quotient, the tile's sum
  float acc = 0.f;
  const bool maps = p.m_sxy != nullptr;
  for (int it = tid; it < kSsTH * TWC; it += kSsBlock) {
    const int oy = it / TWC, j = it - oy * TWC, c = j % C;
    float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < win; ++k) {
      const float wk = p.taps.w[k];
#pragma unroll
      for (int i = 0; i < 5; ++i) m[i] += wk * rowm[i][(oy + k) * TWC + j];
    }
    const bool valid = y0 + oy < p.ho && x0 + j / C < p.wo;
    const SsCentral<float> ce = ss_central<float>(m[0], m[1], m[2], m[3], m[4], px[c], py[c], p.taps.excess);
    const SsPoint<float> pt = ss_point<float>(px[c] + ce.dx, py[c] + ce.dy, ce.sx, ce.sy, ce.sxy, c1, c2);
    acc += valid ? pt.value : 0.f;
    if (maps && valid) {
      const long long o = (((long long)n * p.ho + (y0 + oy)) * p.wo + x0) * C + j;
      p.m_sxy[o] = pt.g_sxy;
      p.m_s[o] = pt.g_s;
      if (p.m_ax) p.m_ax[o] = pt.g_mux - 2.f * pt.g_s * ce.dx - pt.g_sxy * ce.dy;
      if (p.m_ay) p.m_ay[o] = pt.g_muy - 2.f * pt.g_s * ce.dy - pt.g_sxy * ce.dx;
    }
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) p.part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// a fixed tree over the 256 threads' values; every thread gets the sum
__device__ __forceinline__ double ss_block_sum(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = kSsBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(kSsBlock) void ssim_finish_kernel(const float* __restrict__ part, int n, int tiles, double per_sample,
                                                               SsState* __restrict__ st, float* __restrict__ vals,
                                                               float* __restrict__ values) {
  __shared__ double red[kSsBlock];
  double total = 0.0;
  for (int s = 0; s < n; ++s) {
    double acc = 0.0;
    for (int t = threadIdx.x; t < tiles; t += kSsBlock) acc += (double)part[(size_t)s * tiles + t];
    const double v = ss_block_sum(acc, red) / per_sample;
    if (threadIdx.x == 0) values[s] = (float)v;
    total += v;
  }
  if (threadIdx.x == 0) {
    const double term = 1.0 - total / (double)n;
    const double weight = st ? (double)st->weight : 1.0;
    vals[0] = (float)(weight * term);
    vals[1] = (float)term;
    if (st) {
      st->term = (float)term;
      st->weighted = (float)(weight * term);
      st->updates += 1;
    }
  }
}

// T[M] at the thread's input pixels: the full correlation of coefficient map M with the product taps, through LDS
template <int C>
__device__ __forceinline__ void ss_adjoint(const SsGradParams& p, const float* __restrict__ map, int n, int y0, int x0, float* tile,
                                           float* rowb, float (&out)[(kSsTH * kSsTW * C + kSsBlock - 1) / kSsBlock]) {
  constexpr int TWC = kSsTW * C;
  const int tid = threadIdx.x;
  const int win = p.taps.n, halo = win - 1;
  const int rows_all = kSsTH + halo, S = (kSsTW + halo) * C;
  const long long grs = (long long)p.wo * C;
  const long long g0 = ((long long)n * p.ho + (y0 - halo)) * grs + (long long)(x0 - halo) * C;      // may lie in front of the map
  const float zero[C] = {};
  __syncthreads();                                            // the previous map's readers of tile / rowb
  ss_load_tile<C>(tile, map, g0, grs, max(0, halo - y0), min(rows_all, p.ho - y0 + halo), max(0, (halo - x0) * C),
                  min(S, (p.wo - x0 + halo) * C), rows_all, S, zero);
  __syncthreads();
  for (int it = tid; it < rows_all * TWC; it += kSsBlock) {
    const int r = it / TWC, j = it - r * TWC;
    const float* a = tile + r * S + j + halo * C;
    float m = 0.f;
    for (int k = 0; k < win; ++k) m += p.taps.w[k] * a[-k * C];
    rowb[it] = m;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < (kSsTH * TWC + kSsBlock - 1) / kSsBlock; ++i) {
    const int it = tid + i * kSsBlock;
    float m = 0.f;
    if (it < kSsTH * TWC) {
      const int l = it / TWC, j = it - l * TWC;
      for (int k = 0; k < win; ++k) m += p.taps.w[k] * rowb[(l + halo - k) * TWC + j];
    }
    out[i] = m;
  }
}

template <int C>
__global__ __launch_bounds__(kSsBlock) void ssim_grad_kernel(SsGradParams p) {
  constexpr int TWC = kSsTW * C;
  constexpr int kPer = (kSsTH * TWC + kSsBlock - 1) / kSsBlock;
  __shared__ float tile[kSsInH * kSsInW * C];
  __shared__ float rowb[kSsInH * TWC];
  const int tid = threadIdx.x;
  const int n = blockIdx.x / p.tiles, t = blockIdx.x - n * p.tiles;
  const int ty = t / p.tiles_x, tx = t - ty * p.tiles_x;
  const int y0 = ty * kSsTH, x0 = tx * kSsTW;
  const long long plane = (long long)n * p.h * p.w * C;
  const double weight = p.st ? (double)p.st->weight : 1.0, g = p.g ? (double)*p.g : 1.0;
  const float scale = (float)(-(weight * g) / p.count);

  float t_s[kPer], t_sxy[kPer], t_a[kPer];
  ss_adjoint<C>(p, p.m_s, n, y0, x0, tile, rowb, t_s);
  ss_adjoint<C>(p, p.m_sxy, n, y0, x0, tile, rowb, t_sxy);
  for (int which = 0; which < 2; ++which) {
    float* __restrict__ d = which == 0 ? p.dx : p.dy;
    if (!d) continue;                                           // uniform
    ss_adjoint<C>(p, which == 0 ? p.m_ax : p.m_ay, n, y0, x0, tile, rowb, t_a);
    const float* own = which == 0 ? p.x : p.y;
    const float* oth = which == 0 ? p.y : p.x;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int it = tid + i * kSsBlock;
      const int l = it / TWC, j = it - l * TWC;
      if (it < kSsTH * TWC && y0 + l < p.h && x0 + j / C < p.w) {
        const int c = j % C;
        const long long o = plane + ((long long)(y0 + l) * p.w + x0) * C + j;
        const float u = own[o] - own[plane + c], v = oth[o] - oth[plane + c];
        d[o] = scale * (t_a[i] + 2.f * u * t_s[i] + v * t_sxy[i]);
      }
    }
  }
}

__global__ __launch_bounds__(256) void psnr_rows_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                        float* __restrict__ part, long long e, int nchunk, long long items) {
  __shared__ float red[4];
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const long long n = it / nchunk;
    const int chunk = (int)(it - n * nchunk);
    const float* a = x + n * e;
    const float* b = y + n * e;
    float acc = 0.f;
#pragma unroll
    for (int jv = 0; jv < kPsnrChunk / 256; ++jv) {            // element chunk * 4096 + jv * 256 + tid: 16 serial adds per thread
      const long long i = (long long)chunk * kPsnrChunk + jv * 256 + (int)threadIdx.x;
      if (i < e) {
        const float d = a[i] - b[i];
        acc += d * d;
      }
    }
    acc = wave_sum(acc);
    __syncthreads();                                           // the previous item's reads of red[]
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[it] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// thread r % 256 owns sample r: its partials ascending in float64; 10 log10(L^2 / mse), +inf at mse == 0
__global__ __launch_bounds__(256) void psnr_finish_kernel(const float* __restrict__ part, int n, int nchunk, double e, double range,
                                                          double* __restrict__ out) {
  for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) s += (double)part[(size_t)r * nchunk + c];
    const double mse = s / e;
    out[r] = mse == 0.0 ? (double)INFINITY : 10.0 * log10(range * range / mse);
  }
}

struct SsGeom { int ho, wo, tiles_x, tiles_y; long long tiles, positions; };

static bool ss_geometry(int n, int c, int h, int w, int window, SsGeom* g) {
  if (!(n > 0 && c >= 1 && c <= kSsMaxC && ss_window_ok(window) && h >= window && w >= window)) return false;
  if ((long long)n * c * h * w >= (1LL << 31)) return false;
  g->ho = h - window + 1; g->wo = w - window + 1;
  g->positions = (long long)g->ho * g->wo;
  return true;
}
static void ss_tiles(int extent_y, int extent_x, SsGeom* g) {
  g->tiles_y = (int)ceil_div(extent_y, kSsTH); g->tiles_x = (int)ceil_div(extent_x, kSsTW);
  g->tiles = (long long)g->tiles_y * g->tiles_x;
}
static size_t ss_part_bytes(int n, const SsGeom& g) { return (size_t)round_up((long long)n * g.tiles * (long long)sizeof(float), 16); }
static size_t ss_map_bytes(int n, int c, const SsGeom& g) { return (size_t)round_up((long long)n * g.positions * c * (long long)sizeof(float), 16); }
static int ss_n_maps(int want_dx, int want_dy) { return want_dx || want_dy ? 2 + (want_dx ? 1 : 0) + (want_dy ? 1 : 0) : 0; }
static bool ss_aligned(const void* p, int to) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(to - 1)) == 0; }
static bool ss_settings_ok(float weight, float c1, float c2) {
  return weight >= 0.f && weight <= 3.0e38f && c1 >= 0.f && c1 <= 3.0e38f && c2 > 0.f && c2 <= 3.0e38f;
}
static bool ss_taps_ok(const float* taps, int window) {
  for (int k = 0; k < window; ++k)
    if (!(taps[k] >= 0.f && taps[k] <= 3.0e38f)) return false;
  return true;
}

}  // namespace srgan

using namespace srgan;

#define SS_GEOMETRY_TEXT "n > 0, 1..3 channels, window odd in 3..11, h and w >= window, n c h w < 2^31"

extern "C" size_t srgan_ssim_state_bytes(void) { return sizeof(SsState); }

extern "C" int srgan_ssim_state_init(void* state, float weight, float c1, float c2, void* stream) {
  SRGAN_REQUIRE(state && ss_settings_ok(weight, c1, c2),
                "ssim_state_init: bad argument (a record; weight >= 0, c1 >= 0, c2 > 0, all finite; NaN refused)");
  SsState s = {};                          // the last values and the counter at zero
  s.weight = weight; s.c1 = c1; s.c2 = c2;
  return record_write(state, &s, sizeof s, record_all_words<SsState>(), as_stream(stream), "ssim_state_init");
}

extern "C" int srgan_ssim_state_set(void* state, float weight, float c1, float c2, void* stream) {
  SRGAN_REQUIRE(state && ss_settings_ok(weight, c1, c2),
                "ssim_state_set: bad argument (a record; weight >= 0, c1 >= 0, c2 > 0, all finite; NaN refused)");
  SsState s = {};
  s.weight = weight; s.c1 = c1; s.c2 = c2;
  return record_write(state, &s, sizeof s, kSsSet, as_stream(stream), "ssim_state_set");
}

extern "C" int srgan_ssim_state_restore(void* state, int updates, float term, float weighted, void* stream) {
  SRGAN_REQUIRE(state && updates >= 0 && std::fabs(term) <= 3.0e38f && std::fabs(weighted) <= 3.0e38f,
                "ssim_state_restore: bad argument (a record; updates >= 0; finite last values, NaN refused)");
  SsState s = {};                          // resume: the settings stay
  s.updates = updates; s.term = term; s.weighted = weighted;
  return record_write(state, &s, sizeof s, kSsRestore, as_stream(stream), "ssim_state_restore");
}

extern "C" int srgan_ssim_taps(int window, double sigma, float* taps) {
  SRGAN_REQUIRE(taps && ss_window_ok(window), "ssim_taps: bad argument (an array of window floats; window odd in 3..11)");
  SRGAN_REQUIRE(sigma > 0.0 && sigma <= 1.0e30, "ssim_taps: sigma must be finite and > 0 (NaN refused)");
  ss_gaussian_taps(window, sigma, taps);
  return 0;
}

extern "C" size_t srgan_ssim_workspace(int n, int c, int h, int w, int window, int want_dx, int want_dy) {
  SsGeom g;
  if (!ss_geometry(n, c, h, w, window, &g)) {
    set_error("ssim_workspace: bad geometry (" SS_GEOMETRY_TEXT ")");
    return 0;
  }
  ss_tiles(g.ho, g.wo, &g);
  return ss_part_bytes(n, g) + (size_t)ss_n_maps(want_dx, want_dy) * ss_map_bytes(n, c, g);
}

// the maps of a workspace in their order: g_sxy, g_s, then A_x and / or A_y
static void ss_map_slots(char* ws, int n, int c, const SsGeom& g, int want_dx, int want_dy, float** sxy, float** s, float** ax, float** ay) {
  char* m = ws + ss_part_bytes(n, g);
  const size_t mb = ss_map_bytes(n, c, g);
  *sxy = *s = *ax = *ay = nullptr;
  if (!want_dx && !want_dy) return;
  *sxy = reinterpret_cast<float*>(m);
  *s = reinterpret_cast<float*>(m + mb);
  if (want_dx) *ax = reinterpret_cast<float*>(m + 2 * mb);
  if (want_dy) *ay = reinterpret_cast<float*>(m + (want_dx ? 3 : 2) * mb);
}

extern "C" int srgan_ssim_map(const float* x, const float* y, int n, int c, int h, int w, int window, const float* taps,
                              const void* state, float c1, float c2, int want_dx, int want_dy, void* ws, size_t ws_bytes,
                              void* stream) {
  SRGAN_REQUIRE(x && y && taps && ws, "ssim_map: null pointer");
  SsGeom g;
  SRGAN_REQUIRE(ss_geometry(n, c, h, w, window, &g), "ssim_map: bad geometry (" SS_GEOMETRY_TEXT ")");
  ss_tiles(g.ho, g.wo, &g);
  SRGAN_REQUIRE((long long)n * g.tiles < (1LL << 31), "ssim_map: too many tiles");
  SRGAN_REQUIRE(ss_taps_ok(taps, window), "ssim_map: a tap is negative or not finite (NaN refused)");
  SRGAN_REQUIRE(state || ss_settings_ok(0.f, c1, c2), "ssim_map: without a record, c1 >= 0 and c2 > 0, finite (NaN refused)");
  const size_t need = ss_part_bytes(n, g) + (size_t)ss_n_maps(want_dx, want_dy) * ss_map_bytes(n, c, g);
  SRGAN_REQUIRE(ws_bytes >= need, "ssim_map: workspace of %zu bytes, %zu needed (srgan_ssim_workspace)", ws_bytes, need);
  SRGAN_REQUIRE(ss_aligned(x, 4) && ss_aligned(y, 4) && ss_aligned(state, 4) && ss_aligned(ws, 16),
                "ssim_map: images or record not 4-byte aligned, or workspace not 16-byte aligned");
  SsMapParams p{};
  p.x = x; p.y = y; p.part = static_cast<float*>(ws);
  ss_map_slots(static_cast<char*>(ws), n, c, g, want_dx, want_dy, &p.m_sxy, &p.m_s, &p.m_ax, &p.m_ay);
  p.st = static_cast<const SsState*>(state); p.c1 = c1; p.c2 = c2;
  p.taps = ss_taps(taps, window);
  p.h = h; p.w = w; p.ho = g.ho; p.wo = g.wo; p.tiles_x = g.tiles_x; p.tiles = (int)g.tiles;
  const dim3 grid((unsigned)((long long)n * g.tiles)), block(kSsBlock);
  hipStream_t st = as_stream(stream);                          // no launch-timer slot, as lecam_kernel
  if (c == 1) hipLaunchKernelGGL(ssim_map_kernel<1>, grid, block, 0, st, p);
  else if (c == 2) hipLaunchKernelGGL(ssim_map_kernel<2>, grid, block, 0, st, p);
  else hipLaunchKernelGGL(ssim_map_kernel<3>, grid, block, 0, st, p);
  return check_launch("ssim_map_kernel");
}

extern "C" int srgan_ssim_finish(const void* ws, size_t ws_bytes, int n, int c, int h, int w, int window, void* state, float* vals,
                                 float* values, void* stream) {
  SRGAN_REQUIRE(ws && vals && values, "ssim_finish: null pointer");
  SsGeom g;
  SRGAN_REQUIRE(ss_geometry(n, c, h, w, window, &g), "ssim_finish: bad geometry (" SS_GEOMETRY_TEXT ")");
  ss_tiles(g.ho, g.wo, &g);
  SRGAN_REQUIRE((long long)n * g.tiles < (1LL << 31), "ssim_finish: too many tiles");
  SRGAN_REQUIRE(ws_bytes >= ss_part_bytes(n, g), "ssim_finish: workspace of %zu bytes, %zu needed (srgan_ssim_workspace)", ws_bytes,
                ss_part_bytes(n, g));
  SRGAN_REQUIRE(ss_aligned(ws, 16) && ss_aligned(state, 4) && ss_aligned(vals, 4) && ss_aligned(values, 4),
                "ssim_finish: workspace not 16-byte aligned or a pointer not 4-byte aligned");
  hipLaunchKernelGGL(ssim_finish_kernel, dim3(1), dim3(kSsBlock), 0, as_stream(stream), static_cast<const float*>(ws), n, (int)g.tiles,
                     (double)g.positions * (double)c, static_cast<SsState*>(state), vals, values);
  return check_launch("ssim_finish_kernel");
}

extern "C" int srgan_ssim_grad(const float* x, const float* y, int n, int c, int h, int w, int window, const float* taps,
                               const void* ws, size_t ws_bytes, const void* state, const float* g_in, float* dx, float* dy,
                               void* stream) {
  SRGAN_REQUIRE(x && y && taps && ws && (dx || dy), "ssim_grad: null pointer (one of dx / dy may be NULL, not both)");
  SsGeom g;
  SRGAN_REQUIRE(ss_geometry(n, c, h, w, window, &g), "ssim_grad: bad geometry (" SS_GEOMETRY_TEXT ")");
  ss_tiles(g.ho, g.wo, &g);                                    // the workspace's layout follows the map launch's tiles
  SRGAN_REQUIRE(ss_taps_ok(taps, window), "ssim_grad: a tap is negative or not finite (NaN refused)");
  const int want_dx = dx != nullptr, want_dy = dy != nullptr;
  const size_t need = ss_part_bytes(n, g) + (size_t)ss_n_maps(want_dx, want_dy) * ss_map_bytes(n, c, g);
  SRGAN_REQUIRE(ws_bytes >= need, "ssim_grad: workspace of %zu bytes, %zu needed (srgan_ssim_workspace)", ws_bytes, need);
  SRGAN_REQUIRE(ss_aligned(x, 4) && ss_aligned(y, 4) && ss_aligned(state, 4) && ss_aligned(g_in, 4) && ss_aligned(dx, 4) &&
                    ss_aligned(dy, 4) && ss_aligned(ws, 16),
                "ssim_grad: a pointer not 4-byte aligned, or workspace not 16-byte aligned");
  SRGAN_REQUIRE(dx != x && dx != y && dy != x && dy != y && dx != dy, "ssim_grad: an output aliases an input or the other output");
  SsGradParams p{};
  p.x = x; p.y = y; p.st = static_cast<const SsState*>(state); p.g = g_in; p.dx = dx; p.dy = dy;
  float *sxy, *s, *ax, *ay;
  ss_map_slots(static_cast<char*>(const_cast<void*>(ws)), n, c, g, want_dx, want_dy, &sxy, &s, &ax, &ay);
  p.m_sxy = sxy; p.m_s = s; p.m_ax = ax; p.m_ay = ay;
  p.taps = ss_taps(taps, window);
  p.h = h; p.w = w; p.ho = g.ho; p.wo = g.wo;
  p.count = (double)n * (double)g.positions * (double)c;
  SsGeom gi = g;
  ss_tiles(h, w, &gi);                                         // this launch tiles the INPUT pixels
  SRGAN_REQUIRE((long long)n * gi.tiles < (1LL << 31), "ssim_grad: too many tiles");
  p.tiles_x = gi.tiles_x; p.tiles = (int)gi.tiles;
  const dim3 grid((unsigned)((long long)n * gi.tiles)), block(kSsBlock);
  hipStream_t st = as_stream(stream);
  if (c == 1) hipLaunchKernelGGL(ssim_grad_kernel<1>, grid, block, 0, st, p);
  else if (c == 2) hipLaunchKernelGGL(ssim_grad_kernel<2>, grid, block, 0, st, p);
  else hipLaunchKernelGGL(ssim_grad_kernel<3>, grid, block, 0, st, p);
  return check_launch("ssim_grad_kernel");
}

static long long psnr_chunks(long long e) { return ceil_div(e, kPsnrChunk); }
static bool psnr_geometry_ok(int n, long long e) {
  return n > 0 && e > 0 && e < (1LL << 31) && (long long)n * e < (1LL << 31);
}
static size_t psnr_part_bytes(int n, long long e) { return (size_t)round_up((long long)n * psnr_chunks(e) * (long long)sizeof(float), 8); }

extern "C" size_t srgan_psnr_workspace(int n, long long e) {
  if (!psnr_geometry_ok(n, e)) {
    set_error("psnr_workspace: bad geometry (n, e > 0, n e < 2^31)");
    return 0;
  }
  return psnr_part_bytes(n, e);
}

extern "C" int srgan_psnr(const float* x, const float* y, int n, long long e, float data_range, double* out, void* ws, size_t ws_bytes,
                          void* stream) {
  SRGAN_REQUIRE(x && y && out && ws, "psnr: null pointer");
  SRGAN_REQUIRE(psnr_geometry_ok(n, e), "psnr: bad geometry (n, e > 0, n e < 2^31)");
  SRGAN_REQUIRE(data_range > 0.f && data_range <= 3.0e38f, "psnr: data_range must be finite and > 0 (NaN refused)");
  SRGAN_REQUIRE(ws_bytes >= psnr_part_bytes(n, e), "psnr: workspace of %zu bytes, %zu needed (srgan_psnr_workspace)", ws_bytes,
                psnr_part_bytes(n, e));
  SRGAN_REQUIRE(ss_aligned(x, 4) && ss_aligned(y, 4) && ss_aligned(out, 8) && ss_aligned(ws, 8),
                "psnr: images not 4-byte aligned, or the output or the workspace not 8-byte aligned");
  const long long nchunk = psnr_chunks(e), items = (long long)n * nchunk;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(psnr_rows_kernel, dim3((unsigned)std::min<long long>(items, 2048)), dim3(256), 0, st, x, y, static_cast<float*>(ws),
                     e, (int)nchunk, items);
  int rc = check_launch("psnr_rows_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(psnr_finish_kernel, dim3((unsigned)std::min<long long>(ceil_div(n, 256), 2048)), dim3(256), 0, st,
                     static_cast<const float*>(ws), n, (int)nchunk, (double)e, (double)data_range, out);
  return check_launch("psnr_finish_kernel");
}
