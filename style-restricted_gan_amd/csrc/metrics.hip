// Set metrics over feature matrices [N, D] beyond the reference's PRDC: the Frechet distance of the two Gaussians fitted to
// the sets (FID's formula; Heusel et al. 2017) and the Kernel Inception Distance (Binkowski et al. 2018) in StyleGAN2-ADA's
// estimator.  The reference has neither; both are held to their published definitions in float64 (tests/metric_common.py).
//   gram_kernel<STORE>    G = A B^T on the fp32 MFMA, rows optionally gathered through an index table
//   gram_kernel<POLY3>    the same product, epilogue sum of (g / D + 1)^3 per workgroup (KID's three sums per subset)
//   colsum / mean / centre  column means in float64, A = (X - mean) / sqrt(N - 1) in fp32, trace = sum A^2 in float64
//   jacobi_*              one-sided (Hestenes) Jacobi on the n vectors of W [n, L]: tr sqrt(S1 S2) = |A1 A2^T|_* 
// Every sum runs in a fixed order (register order, xor shuffles, LDS slots in index order, partials in index order): no
// floating-point atomics, results are reproducible bit for bit.
#include <algorithm>
#include "common.h"
#include "metric_math.h"

namespace srgan {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- Gram matrix on v_mfma_f32_32x32x2_f32 -----------------------------------------------------------------------------------------------
// workgroup = 64 x 64 tile of G, wave = one 32 x 32 accumulator; the feature axis goes through LDS in chunks of 16 ([row][k],
// row stride 17 floats).  One MFMA adds features k, k + 1 (lanes 0-31 hold k, lanes 32-63 hold k + 1) as
// fma(a[k+1], b[k+1], fma(a[k], b[k], acc)): every entry is the fp32 fma chain over k = 0, 1, ..., D - 1 from acc = 0, whatever
// the tile or the lane.  Features past D and rows past the matrix read as 0 (fma(0, 0, acc) = acc exactly).  Row r of the
// product is source row idx[z * Na + r] (idx = null: r); an index outside [0, rows) reads as a row of zeros, never memory.
enum { GRAM_STORE = 0, GRAM_POLY3 = 1 };
constexpr int GR_T = 64, GR_K = 16, GR_LD = GR_K + 1;

struct GramArgs {
  const float* a; const int* idx_a; int rows_a, na;
  const float* b; const int* idx_b; int rows_b, nb;
  int d, skip_diag;
  float* g;            // STORE: [na][nb]
  double* partial;     // POLY3: [gridDim.z][gridDim.y][gridDim.x]
};

template <int EPI>
__global__ __launch_bounds__(256) void gram_kernel(GramArgs p) {
  __shared__ float as[GR_T][GR_LD], bs[GR_T][GR_LD];
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.y * GR_T, j0 = blockIdx.x * GR_T;
  const int lr = tid >> 2, lk = (tid & 3) * 4;                 // load role: row lr of the tile, features lk .. lk + 3 of the chunk
  long long ra = -1, rb = -1;                                  // source rows, -1: reads zeros
  if (i0 + lr < p.na) {
    const int r = p.idx_a ? p.idx_a[(size_t)blockIdx.z * p.na + i0 + lr] : i0 + lr;
    if ((unsigned)r < (unsigned)p.rows_a) ra = r;
  }
  if (j0 + lr < p.nb) {
    const int r = p.idx_b ? p.idx_b[(size_t)blockIdx.z * p.nb + j0 + lr] : j0 + lr;
    if ((unsigned)r < (unsigned)p.rows_b) rb = r;
  }
  const float* ap = p.a + (size_t)(ra < 0 ? 0 : ra) * p.d + lk;
  const float* bp = p.b + (size_t)(rb < 0 ? 0 : rb) * p.d + lk;
  const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
  const int fr = lane & 31, fk = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  for (int k0 = 0; k0 < p.d; k0 += GR_K) {
    float xa[4], xb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool kv = k0 + lk + e < p.d;
      xa[e] = (ra >= 0 && kv) ? ap[k0 + e] : 0.f;
      xb[e] = (rb >= 0 && kv) ? bp[k0 + e] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) { as[lr][lk + e] = xa[e]; bs[lr][lk + e] = xb[e]; }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GR_K; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[wi + fr][kk + fk], bs[wj + fr][kk + fk], acc, 0, 0, 0);
  }
  // accumulator register e of lane l: row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31 of the wave's tile
  const int j = j0 + wj + fr;
  if (EPI == GRAM_STORE) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int i = i0 + wi + (e & 3) + 8 * (e >> 2) + 4 * fk;
      if (i < p.na && j < p.nb) p.g[(size_t)i * p.nb + j] = acc[e];
    }
  } else {
    // registers in index order, lanes by xor shuffles (32, 16, ..., 1), waves 0..3 through LDS in index order
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int i = i0 + wi + (e & 3) + 8 * (e >> 2) + 4 * fk;
      if (i < p.na && j < p.nb && !(p.skip_diag && i == j)) s += (double)kid_poly3(acc[e], p.d);
    }
    s = wave_sum_f64(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (tid == 0)
      p.partial[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

// out[t] = part[t][0] + part[t][1] + ... in index order, t < count
__global__ __launch_bounds__(256) void sum_partials_kernel(const double* __restrict__ part, int per, int count, double* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= count) return;
  double s = 0.0;
  for (int e = 0; e < per; ++e) s += part[(size_t)t * per + e];
  out[t] = s;
}

// KID: sums[s][kind] = the partials of (kind, subset s) in index order (part is [3][S][per]), then one thread forms
// kid = (1 / S) sum_s [(Sxx + Syy) / (m (m - 1)) - 2 Sxy / m^2] over the subsets in index order
__global__ __launch_bounds__(256) void kid_final_kernel(const double* __restrict__ part, int per, int S, int m, double* sums, double* kid) {
  for (int t = threadIdx.x; t < 3 * S; t += 256) {
    const int s = t / 3, kind = t % 3;
    const double* q = part + ((size_t)kind * S + s) * per;
    double v = 0.0;
    for (int e = 0; e < per; ++e) v += q[e];
    sums[t] = v;
  }
  __syncthreads();                     // (workgroup-scope fence: thread 0 reads what this workgroup's threads stored)
  if (threadIdx.x == 0) {
    const double mm = (double)m, off = mm * (mm - 1.0);
    double v = 0.0;
    for (int s = 0; s < S; ++s) v += (sums[3 * s] + sums[3 * s + 1]) / off - 2.0 * sums[3 * s + 2] / (mm * mm);
    *kid = v / (double)S;
  }
}

// ---- feature statistics ------------------------------------------------------------------------------------------------------------------
// column sums in float64: thread = column (a wave reads 256 contiguous bytes of a row), grid.y = a block of rows; the row blocks
// are added in index order by mean_kernel, which rounds sum / N once to fp32
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ x, int N, int D, int rows_per, double* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= D) return;
  const int r0 = blockIdx.y * rows_per, r1 = min(N, r0 + rows_per);
  double s = 0.0;
  for (int r = r0; r < r1; ++r) s += (double)x[(size_t)r * D + c];
  part[(size_t)blockIdx.y * D + c] = s;
}
__global__ __launch_bounds__(256) void mean_kernel(const double* __restrict__ part, int chunks, int N, int D, float* __restrict__ mean) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= D) return;
  double s = 0.0;
  for (int e = 0; e < chunks; ++e) s += part[(size_t)e * D + c];
  mean[c] = (float)(s / (double)N);
}
// A = (X - mean) / sqrt(N - 1) in fp32 (subtract, divide by the rounded root: three roundings with the root's own);
// a^2 is exact in float64.  Grid-stride; thread sums in visiting order, then shuffles, then the waves in index order.
__global__ __launch_bounds__(256) void centre_kernel(const float* __restrict__ x, const float* __restrict__ mean, long long total, int D,
                                                     float scale, float* __restrict__ a, double* __restrict__ part) {
  __shared__ double red[4];
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const float v = (x[i] - mean[(int)(i % D)]) / scale;
    a[i] = v;
    s += (double)v * (double)v;
  }
  s = wave_sum_f64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- one-sided Jacobi --------------------------------------------------------------------------------------------------------------------
// workspace: [0] fp32 |W|_F^2, at byte 16 double norm2[n], then int flags[np / 2]
struct JacobiWs { float* frob2; double* norm2; int* flags; };
__host__ __device__ inline JacobiWs jacobi_ws(void* ws, int n) {
  JacobiWs w;
  w.frob2 = static_cast<float*>(ws);
  w.norm2 = reinterpret_cast<double*>(static_cast<char*>(ws) + 16);
  w.flags = reinterpret_cast<int*>(w.norm2 + n);
  return w;
}

// norm2[i] = |w_i|^2 in float64: workgroup = vector, thread sums k = tid, tid + 256, ... in that order
__global__ __launch_bounds__(256) void row_norm2_kernel(const float* __restrict__ w, int L, double* __restrict__ norm2) {
  __shared__ double red[4];
  const float* r = w + (size_t)blockIdx.x * L;
  double s = 0.0;
  for (int k = threadIdx.x; k < L; k += 256) { const double v = (double)r[k]; s += v * v; }
  s = wave_sum_f64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) norm2[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}
// start of a sweep: the flags of its slots to 0, |W|_F^2 = sum of the norms in index order, rounded to fp32
__global__ __launch_bounds__(256) void jacobi_begin_kernel(const double* __restrict__ norm2, int n, int half, float* frob2, int* flags) {
  for (int k = threadIdx.x; k < half; k += 256) flags[k] = 0;
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += norm2[i];
    *frob2 = (float)s;
  }
}
// one round: workgroup = the pair of slot blockIdx.x.  The three dot products run as fp32 fma chains per thread (k = tid,
// tid + 256, ...), xor shuffles per wave and the four wave sums in index order; every thread then rotates the elements it
// read (the second read of the 2 L floats comes from the cache).  The phantom vector of an odd n is index np - 1 >= n: its
// pair returns before any address is formed.
__global__ __launch_bounds__(256) void jacobi_round_kernel(float* w, int n, int np, int L, int round, const float* frob2, int* flags) {
  __shared__ float red[3][4];
  int i, j;
  jacobi_pair(np, round, (int)blockIdx.x, &i, &j);
  if (j >= n) return;
  float* wi = w + (size_t)i * L;
  float* wj = w + (size_t)j * L;
  float a = 0.f, b = 0.f, g = 0.f;
  for (int k = threadIdx.x; k < L; k += 256) {
    const float x = wi[k], y = wj[k];
    a = fmaf(x, x, a); b = fmaf(y, y, b); g = fmaf(x, y, g);
  }
  a = wave_sum(a); b = wave_sum(b); g = wave_sum(g);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; red[2][threadIdx.x >> 6] = g; }
  __syncthreads();
  a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
  b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  g = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
  if (jacobi_skip(a, b, g, *frob2)) return;                  // uniform over the workgroup
  const JacobiRot rot = jacobi_rotation(a, b, g);
  for (int k = threadIdx.x; k < L; k += 256) {
    float x = wi[k], y = wj[k];
    jacobi_apply(rot, &x, &y);
    wi[k] = x; wj[k] = y;
  }
  if (threadIdx.x == 0) flags[blockIdx.x] += 1;              // this slot's own counter: one workgroup per slot and round
}
// end of a sweep: the rotations of all its slots (integers, any order gives the same sum)
__global__ __launch_bounds__(256) void jacobi_end_kernel(const int* __restrict__ flags, int half, int* __restrict__ count) {
  __shared__ int red[256];
  int s = 0;
  for (int k = threadIdx.x; k < half; k += 256) s += flags[k];
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int e = 0; e < 256; ++e) t += red[e];
    *count = t;
  }
}
// |W|_* = sum_i sqrt(|w_i|^2) in float64, index order
__global__ void nuclear_sum_kernel(const double* __restrict__ norm2, int n, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += sqrt(norm2[i]);
  *out = s;
}

constexpr int kCentreGrid = 1024;     // workgroups of centre_kernel at most (its partial sums are one double each)
constexpr int kColChunks = 64;        // row blocks of colsum_kernel at most
static int col_chunks(int N) { return (int)std::min<long long>(kColChunks, ceil_div(N, 64)); }
static int centre_grid(long long total) { return (int)std::min<long long>(kCentreGrid, ceil_div(total, 256)); }
static long long kid_tiles(int m) { return ceil_div(m, GR_T) * ceil_div(m, GR_T); }

template <int EPI>
static void gram_launch(const GramArgs& p, int z, hipStream_t st) {
  hipLaunchKernelGGL(gram_kernel<EPI>, dim3((unsigned)ceil_div(p.nb, GR_T), (unsigned)ceil_div(p.na, GR_T), (unsigned)z), dim3(256), 0, st, p);
}

}  // namespace srgan

using namespace srgan;

extern "C" int srgan_gram_f32(const float* a, int rows_a, const int* idx_a, int na, const float* b, int rows_b, const int* idx_b,
                              int nb, int D, float* g, void* stream) {
  SRGAN_REQUIRE(a && b && g, "gram_f32: null pointer");
  SRGAN_REQUIRE(D >= 1, "gram_f32: D = %d must be at least 1", D);
  SRGAN_REQUIRE(rows_a >= 1 && rows_b >= 1 && na >= 1 && nb >= 1, "gram_f32: empty matrix");
  SRGAN_REQUIRE((idx_a || na <= rows_a) && (idx_b || nb <= rows_b), "gram_f32: more rows asked for than the matrix has (no index table)");
  SRGAN_REQUIRE(ceil_div(na, GR_T) <= 65535, "gram_f32: more than 65535 row tiles");
  GramArgs p = {a, idx_a, rows_a, na, b, idx_b, rows_b, nb, D, 0, g, nullptr};
  gram_launch<GRAM_STORE>(p, 1, as_stream(stream));
  return check_launch("gram_kernel<STORE>");
}

extern "C" size_t srgan_feature_stats_workspace(int N, int D) {
  if (N < 2 || D < 1) return 0;
  return ((size_t)col_chunks(N) * (size_t)D + (size_t)kCentreGrid) * sizeof(double);
}

extern "C" int srgan_feature_stats(const float* x, int N, int D, float* mean, float* a, double* trace, void* ws, size_t ws_bytes,
                                   void* stream) {
  SRGAN_REQUIRE(x && mean && a && trace && ws, "feature_stats: null pointer");
  SRGAN_REQUIRE(N >= 2, "feature_stats: N = %d, the unbiased covariance needs at least 2 rows", N);
  SRGAN_REQUIRE(D >= 1, "feature_stats: D = %d must be at least 1", D);
  SRGAN_REQUIRE(ws_bytes >= srgan_feature_stats_workspace(N, D), "feature_stats: workspace too small");
  hipStream_t st = as_stream(stream);
  const int chunks = col_chunks(N), rows_per = (int)ceil_div(N, chunks);
  double* colpart = static_cast<double*>(ws);
  double* trpart = colpart + (size_t)chunks * D;
  const long long total = (long long)N * D;
  const int cg = centre_grid(total);
  const unsigned cb = (unsigned)ceil_div(D, 256);
  hipLaunchKernelGGL(colsum_kernel, dim3(cb, (unsigned)chunks), dim3(256), 0, st, x, N, D, rows_per, colpart);
  hipLaunchKernelGGL(mean_kernel, dim3(cb), dim3(256), 0, st, colpart, chunks, N, D, mean);
  hipLaunchKernelGGL(centre_kernel, dim3((unsigned)cg), dim3(256), 0, st, x, mean, total, D, sqrtf((float)(N - 1)), a, trpart);
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, st, trpart, cg, 1, trace);
  return check_launch("feature_stats kernels");
}

extern "C" size_t srgan_kid_workspace(int num_subsets, int m) {
  if (num_subsets < 1 || m < 2) return 0;
  return (size_t)3 * (size_t)num_subsets * (size_t)kid_tiles(m) * sizeof(double);
}

extern "C" int srgan_kid_poly3(const float* x, int n_real, const float* y, int n_fake, int D, const int* idx_x, const int* idx_y,
                               int num_subsets, int m, double* sums, double* kid, void* ws, size_t ws_bytes, void* stream) {
  SRGAN_REQUIRE(x && y && idx_x && idx_y && sums && kid && ws, "kid_poly3: null pointer");
  SRGAN_REQUIRE(D >= 1, "kid_poly3: D = %d must be at least 1", D);
  SRGAN_REQUIRE(m >= 2, "kid_poly3: subset size m = %d, the off-diagonal mean needs at least 2", m);
  SRGAN_REQUIRE(m <= n_real && m <= n_fake, "kid_poly3: subset size m = %d exceeds a set (%d real, %d fake)", m, n_real, n_fake);
  SRGAN_REQUIRE(num_subsets >= 1 && num_subsets <= 65535, "kid_poly3: num_subsets = %d outside 1..65535", num_subsets);
  SRGAN_REQUIRE(ws_bytes >= srgan_kid_workspace(num_subsets, m), "kid_poly3: workspace too small");
  hipStream_t st = as_stream(stream);
  const int per = (int)kid_tiles(m);
  double* part = static_cast<double*>(ws);
  GramArgs xx = {x, idx_x, n_real, m, x, idx_x, n_real, m, D, 1, nullptr, part};
  GramArgs yy = {y, idx_y, n_fake, m, y, idx_y, n_fake, m, D, 1, nullptr, part + (size_t)num_subsets * per};
  GramArgs xy = {x, idx_x, n_real, m, y, idx_y, n_fake, m, D, 0, nullptr, part + (size_t)2 * num_subsets * per};
  gram_launch<GRAM_POLY3>(xx, num_subsets, st);
  gram_launch<GRAM_POLY3>(yy, num_subsets, st);
  gram_launch<GRAM_POLY3>(xy, num_subsets, st);
  hipLaunchKernelGGL(kid_final_kernel, dim3(1), dim3(256), 0, st, part, per, num_subsets, m, sums, kid);
  return check_launch("kid kernels");
}

extern "C" size_t srgan_jacobi_workspace(int n) {
  if (n < 1) return 0;
  const int np = n + (n & 1);
  return 16 + (size_t)n * sizeof(double) + (size_t)(np / 2) * sizeof(int);
}

extern "C" int srgan_jacobi_sweep(float* w, int n, int L, int* rotations, void* ws, size_t ws_bytes, void* stream) {
  SRGAN_REQUIRE(w && rotations && ws, "jacobi_sweep: null pointer");
  SRGAN_REQUIRE(n >= 2, "jacobi_sweep: n = %d, a sweep needs at least 2 vectors", n);
  SRGAN_REQUIRE(L >= 1, "jacobi_sweep: L = %d must be at least 1", L);
  SRGAN_REQUIRE(ws_bytes >= srgan_jacobi_workspace(n), "jacobi_sweep: workspace too small");
  SRGAN_REQUIRE((reinterpret_cast<size_t>(ws) & 7) == 0, "jacobi_sweep: workspace not 8-byte aligned");
  hipStream_t st = as_stream(stream);
  const int np = n + (n & 1), half = np / 2;
  const JacobiWs q = jacobi_ws(ws, n);
  hipLaunchKernelGGL(row_norm2_kernel, dim3((unsigned)n), dim3(256), 0, st, w, L, q.norm2);
  hipLaunchKernelGGL(jacobi_begin_kernel, dim3(1), dim3(256), 0, st, q.norm2, n, half, q.frob2, q.flags);
  for (int round = 0; round < np - 1; ++round)
    hipLaunchKernelGGL(jacobi_round_kernel, dim3((unsigned)half), dim3(256), 0, st, w, n, np, L, round, q.frob2, q.flags);
  hipLaunchKernelGGL(jacobi_end_kernel, dim3(1), dim3(256), 0, st, q.flags, half, rotations);
  return check_launch("jacobi kernels");
}

extern "C" int srgan_nuclear_from_rows(const float* w, int n, int L, double* out, void* ws, size_t ws_bytes, void* stream) {
  SRGAN_REQUIRE(w && out && ws, "nuclear_from_rows: null pointer");
  SRGAN_REQUIRE(n >= 1 && L >= 1, "nuclear_from_rows: empty matrix");
  SRGAN_REQUIRE(ws_bytes >= srgan_jacobi_workspace(n), "nuclear_from_rows: workspace too small");
  SRGAN_REQUIRE((reinterpret_cast<size_t>(ws) & 7) == 0, "nuclear_from_rows: workspace not 8-byte aligned");
  hipStream_t st = as_stream(stream);
  const JacobiWs q = jacobi_ws(ws, n);
  hipLaunchKernelGGL(row_norm2_kernel, dim3((unsigned)n), dim3(256), 0, st, w, L, q.norm2);
  hipLaunchKernelGGL(nuclear_sum_kernel, dim3(1), dim3(64), 0, st, q.norm2, n, out);
  return check_launch("nuclear kernels");
}
