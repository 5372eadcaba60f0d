// Spectral normalisation of convolution weights (Miyato et al., 2018) for the discriminator: extension, no counterpart in the
// reference.  fp32 in both compute modes.  DESIGN.md section 7 ("Spectral normalisation") has the formulas and the cost.
//
// One record of the device table is one layer, W viewed as Wm[O][K] (K = I * kh * kw, row-major): sixteen 64-bit words
//   {W, W_sn, u, v, sigma, O, K, slab0, col0, elem0, ws_part, ws_t, ws_nsq, ws_y, ws_dot, 0}.
// Three flat work lists run over all records (the *0 words are a record's first item, prefix sums written by srgan_spectral_plan):
//   slab items  (slab, cc): rows [32 slab, 32 slab + 32) x columns [1024 cc, 1024 cc + 1024)      ceil(O / 32) * ceil(K / 1024) per layer
//   column items      (cc): columns [1024 cc, 1024 cc + 1024)                                     ceil(K / 1024) per layer
//   element items          : 4096 consecutive elements of the flat weight                         ceil(O K / 4096) per layer
// so a wide-short matrix (4 x 16384) is cut along its columns and a tall one (512 x 4096) along both.  The ws_* words are float
// offsets into the workspace.  Every phase that needs a sum over a whole layer ends its launch; no workgroup waits on another; no
// atomics: every partial has one owner and every sum a fixed order, so a result does not depend on the grid.
//
// Refresh with iteration, per power iteration:
//   1 sn_wtu_partials     part[slab][k] = sum_{o in slab} W[o][k] u[o]             (<= 32 serial fused multiply-adds, ascending o)
//   2 sn_vnorm_partials   t[k] = sum_slab part[slab][k] (ascending, serial); nsq[cc] = sum_k t[k]^2 over the 1024 columns
//                         (4 serial fma per thread, 6 butterfly levels, (w0 + w1) + (w2 + w3))
//   3 sn_wv_partials      n = sqrt(sum_cc nsq[cc]) (ascending, serial); v[k] = t[k] / max(n, eps) (written by slab 0);
//                         y[o][cc] = sum_k W[o][k] v[k] over the 1024 columns: one wave per row, 16 serial fma per lane, 6 levels
//   4 sn_unorm_sigma      one workgroup per layer: y[o] = sum_cc y[o][cc] (ascending, serial); S = sum_o y[o]^2; u = y / max(sqrt S,
//                         eps); sigma = sum_o u[o] y[o]  (thread-strided serial fma, 6 butterfly levels, waves added in ascending order)
// then 5 sn_scale: W_sn = W / sigma (IEEE division).  Without iteration: 3 (v read, not written), 4 (u read), 5.
// Project (in place on the gradient G of W_sn):
//   1 sn_dot_partials     dot[chunk] = sum G W_sn over 4096 elements (the order of grad_sumsq_partials_kernel, depth 24)
//   2 sn_project          c = sum_chunk dot[chunk] (thread-strided serial, then the block sum); G <- (G - c u[o] v[k]) / sigma
#include "common.h"
#include <algorithm>
#include <cstdint>
#include <cstring>

namespace srgan {

typedef unsigned long long sn_word;
constexpr int kSnRecWords = 16;
constexpr int kSnSlabRows = 32;
constexpr int kSnCols = 1024;
constexpr int kSnChunk = 4096;
enum { SN_W, SN_WSN, SN_U, SN_V, SN_SIGMA, SN_O, SN_K, SN_SLAB0, SN_COL0, SN_ELEM0, SN_WS_PART, SN_WS_T, SN_WS_NSQ, SN_WS_Y, SN_WS_DOT,
       SN_RESERVED };

// host-side summary of a table (srgan_spectral_plan)
struct SnPlan { int n_records, pad; long long slab_items, col_items, elem_items, ws_floats; };
static_assert(sizeof(SnPlan) == 40, "SnPlan layout");

// the last record whose first item (word `word`) is <= item (block-uniform: scalar loads)
__device__ __forceinline__ const sn_word* sn_find(const sn_word* __restrict__ table, int n_records, int word, long long item) {
  int lo = 0, hi = n_records - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((long long)table[(size_t)mid * kSnRecWords + word] <= item) lo = mid; else hi = mid - 1;
  }
  return table + (size_t)lo * kSnRecWords;
}

// sum over the 256 threads of a workgroup: butterfly inside each wave, then (w0 + w1) + (w2 + w3); every thread gets the sum
__device__ __forceinline__ float sn_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();                            // the previous use of red[]
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void sn_wtu_partials_kernel(const sn_word* __restrict__ table, int n_records, long long items,
                                                              float* ws) {
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const sn_word* rec = sn_find(table, n_records, SN_SLAB0, it);
    const float* W = reinterpret_cast<const float*>(rec[SN_W]);
    const float* u = reinterpret_cast<const float*>(rec[SN_U]);
    const int O = (int)rec[SN_O], K = (int)rec[SN_K];
    const int ncc = (K + kSnCols - 1) / kSnCols;
    const long long local = it - (long long)rec[SN_SLAB0];
    const int slab = (int)(local / ncc), cc = (int)(local % ncc);
    const int o0 = slab * kSnSlabRows;
    if (local < 0 || o0 >= O) continue;       // (a table whose prefix sums disagree with its sizes touches nothing)
    const int o1 = o0 + kSnSlabRows < O ? o0 + kSnSlabRows : O;
    const int k = cc * kSnCols + (int)threadIdx.x * 4;
    float* part = ws + rec[SN_WS_PART] + (size_t)slab * K;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if ((rec[SN_W] & 15) == 0 && (K & 3) == 0) {
      if (k < K) {
        for (int o = o0; o < o1; ++o) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(W + (size_t)o * K + k);
          const float uo = u[o];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(w[e], uo, acc[e]);
        }
        *reinterpret_cast<f32x4*>(part + k) = acc;
      }
    } else {
      for (int o = o0; o < o1; ++o) {
        const float uo = u[o];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k + e < K) acc[e] = __builtin_fmaf(W[(size_t)o * K + k + e], uo, acc[e]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (k + e < K) part[k + e] = acc[e];
    }
  }
}

__global__ __launch_bounds__(256) void sn_vnorm_partials_kernel(const sn_word* __restrict__ table, int n_records, long long items,
                                                                float* ws) {
  __shared__ float red[4];
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const sn_word* rec = sn_find(table, n_records, SN_COL0, it);
    const int O = (int)rec[SN_O], K = (int)rec[SN_K];
    const int nslab = (O + kSnSlabRows - 1) / kSnSlabRows;
    const long long cc = it - (long long)rec[SN_COL0];
    if (cc < 0 || cc * kSnCols >= K) continue;
    const int k = (int)cc * kSnCols + (int)threadIdx.x * 4;
    const float* part = ws + rec[SN_WS_PART];
    float* t = ws + rec[SN_WS_T];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if ((K & 3) == 0) {                       // (the workspace regions are 16-byte aligned)
      if (k < K) {
        for (int s = 0; s < nslab; ++s) acc += *reinterpret_cast<const f32x4*>(part + (size_t)s * K + k);
        *reinterpret_cast<f32x4*>(t + k) = acc;
      }
    } else {
      for (int s = 0; s < nslab; ++s) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k + e < K) acc[e] += part[(size_t)s * K + k + e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (k + e < K) t[k + e] = acc[e];
    }
    float sq = 0.f;                           // columns past K hold +0
#pragma unroll
    for (int e = 0; e < 4; ++e) sq = __builtin_fmaf(acc[e], acc[e], sq);
    sq = sn_block_sum(sq, red);
    if (threadIdx.x == 0) (ws + rec[SN_WS_NSQ])[cc] = sq;
  }
}

template <bool ITERATE>
__global__ __launch_bounds__(256) void sn_wv_partials_kernel(const sn_word* __restrict__ table, int n_records, long long items,
                                                             float* ws, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const sn_word* rec = sn_find(table, n_records, SN_SLAB0, it);
    const float* W = reinterpret_cast<const float*>(rec[SN_W]);
    float* v = reinterpret_cast<float*>(rec[SN_V]);
    const int O = (int)rec[SN_O], K = (int)rec[SN_K];
    const int ncc = (K + kSnCols - 1) / kSnCols;
    const long long local = it - (long long)rec[SN_SLAB0];
    const int slab = (int)(local / ncc), cc = (int)(local % ncc);
    const int o0 = slab * kSnSlabRows;
    if (local < 0 || o0 >= O) continue;
    const int o1 = o0 + kSnSlabRows < O ? o0 + kSnSlabRows : O;
    // every wave holds the 1024 columns of the item: lane l has columns cc * 1024 + j * 256 + l * 4 + e
    float denom = 1.f;
    if (ITERATE) {
      const float* nsq = ws + rec[SN_WS_NSQ];
      float n2 = 0.f;
      for (int c = 0; c < ncc; ++c) n2 += nsq[c];
      denom = fmaxf(sqrtf(n2), eps);
    }
    const float* t = ws + rec[SN_WS_T];
    f32x4 vv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int col = cc * kSnCols + j * 256 + lane * 4 + e;
        float x = 0.f;
        if (col < K) {
          if (ITERATE) {
            x = t[col] / denom;
            if (slab == 0 && wave == 0) v[col] = x;
          } else {
            x = v[col];
          }
        }
        vv[j][e] = x;
      }
    }
    float* y = ws + rec[SN_WS_Y];
    const bool vec = (rec[SN_W] & 15) == 0 && (K & 3) == 0;
    for (int o = o0 + wave; o < o1; o += 4) {
      const float* row = W + (size_t)o * K;
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = cc * kSnCols + j * 256 + lane * 4;
        f32x4 w = {0.f, 0.f, 0.f, 0.f};
        if (vec) {
          if (col < K) w = *reinterpret_cast<const f32x4*>(row + col);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (col + e < K) w[e] = row[col + e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_fmaf(w[e], vv[j][e], acc);
      }
      acc = wave_sum(acc);
      if (lane == 0) y[(size_t)o * ncc + cc] = acc;
    }
  }
}

template <bool ITERATE>
__global__ __launch_bounds__(256) void sn_unorm_sigma_kernel(const sn_word* __restrict__ table, const float* ws, float eps) {
  __shared__ float red[4];
  const sn_word* rec = table + (size_t)blockIdx.x * kSnRecWords;
  float* u = reinterpret_cast<float*>(rec[SN_U]);
  const int O = (int)rec[SN_O], K = (int)rec[SN_K];
  const int ncc = (K + kSnCols - 1) / kSnCols;
  const float* yp = ws + rec[SN_WS_Y];
  float denom = 1.f;
  if (ITERATE) {
    float sq = 0.f;
    for (int o = threadIdx.x; o < O; o += 256) {
      float y = 0.f;
      for (int c = 0; c < ncc; ++c) y += yp[(size_t)o * ncc + c];
      sq = __builtin_fmaf(y, y, sq);
    }
    denom = fmaxf(sqrtf(sn_block_sum(sq, red)), eps);
  }
  float sg = 0.f;
  for (int o = threadIdx.x; o < O; o += 256) {
    float y = 0.f;
    for (int c = 0; c < ncc; ++c) y += yp[(size_t)o * ncc + c];
    float uo;
    if (ITERATE) {
      uo = y / denom;
      u[o] = uo;
    } else {
      uo = u[o];
    }
    sg = __builtin_fmaf(uo, y, sg);
  }
  sg = sn_block_sum(sg, red);
  if (threadIdx.x == 0) *reinterpret_cast<float*>(rec[SN_SIGMA]) = sg;
}

__global__ __launch_bounds__(256) void sn_scale_kernel(const sn_word* __restrict__ table, int n_records, long long items) {
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const sn_word* rec = sn_find(table, n_records, SN_ELEM0, it);
    const float* W = reinterpret_cast<const float*>(rec[SN_W]);
    float* Wsn = reinterpret_cast<float*>(rec[SN_WSN]);
    const long long n = (long long)rec[SN_O] * (long long)rec[SN_K];
    const long long c0 = (it - (long long)rec[SN_ELEM0]) * kSnChunk;
    if (c0 < 0 || c0 >= n) continue;
    const float sigma = *reinterpret_cast<const float*>(rec[SN_SIGMA]);
    if (((rec[SN_W] | rec[SN_WSN]) & 15) == 0 && c0 + kSnChunk <= n) {
      f32x4 w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = *reinterpret_cast<const f32x4*>(W + c0 + (j * 256 + threadIdx.x) * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = w[j][e] / sigma;
        *reinterpret_cast<f32x4*>(Wsn + c0 + (j * 256 + threadIdx.x) * 4) = r;
      }
    } else {
      const long long end = c0 + kSnChunk < n ? c0 + kSnChunk : n;
      for (long long i = c0 + threadIdx.x; i < end; i += 256) Wsn[i] = W[i] / sigma;
    }
  }
}

// element e of a chunk belongs to thread (e / 4) % 256, slot (e / 1024) * 4 + e % 4 on both paths (grad_sumsq_partials_kernel)
__global__ __launch_bounds__(256) void sn_dot_partials_kernel(const sn_word* __restrict__ table, int n_records, long long items,
                                                              const sn_word* __restrict__ grads, float* ws) {
  __shared__ float red[4];
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const sn_word* rec = sn_find(table, n_records, SN_ELEM0, it);
    const sn_word gp = grads[(rec - table) / kSnRecWords];
    const float* G = reinterpret_cast<const float*>(gp);
    const float* Wsn = reinterpret_cast<const float*>(rec[SN_WSN]);
    const long long n = (long long)rec[SN_O] * (long long)rec[SN_K];
    const long long ch = it - (long long)rec[SN_ELEM0];
    const long long c0 = ch * kSnChunk;
    if (gp == 0 || c0 < 0 || c0 >= n) continue;            // a layer without a gradient is left alone
    f32x4 g[4], w[4];
    if (((gp | rec[SN_WSN]) & 15) == 0 && c0 + kSnChunk <= n) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        g[j] = *reinterpret_cast<const f32x4*>(G + c0 + (j * 256 + threadIdx.x) * 4);
        w[j] = *reinterpret_cast<const f32x4*>(Wsn + c0 + (j * 256 + threadIdx.x) * 4);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long long i = c0 + (j * 256 + threadIdx.x) * 4 + e;
          g[j][e] = i < n ? G[i] : 0.f;
          w[j][e] = i < n ? Wsn[i] : 0.f;
        }
      }
    }
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_fmaf(g[j][e], w[j][e], acc);
    }
    acc = sn_block_sum(acc, red);
    if (threadIdx.x == 0) (ws + rec[SN_WS_DOT])[ch] = acc;
  }
}

__global__ __launch_bounds__(256) void sn_project_kernel(const sn_word* __restrict__ table, int n_records, long long items,
                                                         const sn_word* __restrict__ grads, const float* ws) {
  __shared__ float red[4];
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const sn_word* rec = sn_find(table, n_records, SN_ELEM0, it);
    const sn_word gp = grads[(rec - table) / kSnRecWords];
    float* G = reinterpret_cast<float*>(gp);
    const float* u = reinterpret_cast<const float*>(rec[SN_U]);
    const float* v = reinterpret_cast<const float*>(rec[SN_V]);
    const long long K = (long long)rec[SN_K];
    const long long n = (long long)rec[SN_O] * K;
    const long long c0 = (it - (long long)rec[SN_ELEM0]) * kSnChunk;
    if (gp == 0 || c0 < 0 || c0 >= n) continue;
    const float* dot = ws + rec[SN_WS_DOT];
    const long long nch = (n + kSnChunk - 1) / kSnChunk;
    float c = 0.f;
    for (long long i = threadIdx.x; i < nch; i += 256) c += dot[i];
    c = sn_block_sum(c, red);
    const float sigma = *reinterpret_cast<const float*>(rec[SN_SIGMA]);
    if ((gp & 15) == 0 && (K & 3) == 0 && c0 + kSnChunk <= n) {
      f32x4 g[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) g[j] = *reinterpret_cast<const f32x4*>(G + c0 + (j * 256 + threadIdx.x) * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long i = c0 + (j * 256 + threadIdx.x) * 4;     // four elements of one row (K % 4 == 0)
        const long long o = i / K, k = i - o * K;
        const float cu = c * u[o];
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = (g[j][e] - cu * v[k + e]) / sigma;
        *reinterpret_cast<f32x4*>(G + i) = r;
      }
    } else {
      const long long end = c0 + kSnChunk < n ? c0 + kSnChunk : n;
      for (long long i = c0 + threadIdx.x; i < end; i += 256) {
        const long long o = i / K, k = i - o * K;
        const float cu = c * u[o];
        G[i] = (G[i] - cu * v[k]) / sigma;
      }
    }
  }
}

static long long sn_round4(long long x) { return (x + 3) / 4 * 4; }

static int sn_check_plan(const char* what, const void* table, const SnPlan* plan, const void* ws, size_t ws_bytes) {
  SRGAN_REQUIRE(table && plan, "%s: NULL table or plan", what);
  SRGAN_REQUIRE(plan->n_records > 0, "%s: a table of %d records", what, plan->n_records);
  SRGAN_REQUIRE(plan->slab_items >= plan->n_records && plan->col_items >= plan->n_records && plan->elem_items >= plan->n_records &&
                    plan->ws_floats > 0,
                "%s: the plan does not describe %d records (srgan_spectral_plan fills it)", what, plan->n_records);
  SRGAN_REQUIRE(ws, "%s: NULL workspace", what);
  SRGAN_REQUIRE(ws_bytes >= (size_t)plan->ws_floats * sizeof(float), "%s: workspace of %zu bytes, %zu needed", what, ws_bytes,
                (size_t)plan->ws_floats * sizeof(float));
  SRGAN_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: workspace not 16-byte aligned", what);
  return 0;
}

// memory bound: one block per item up to 256 CUs x 8 blocks, the rest by grid stride
static unsigned sn_grid(long long items) { return (unsigned)std::min<long long>(items, 2048); }

}  // namespace srgan

using namespace srgan;

extern "C" size_t srgan_spectral_record_bytes(void) { return kSnRecWords * sizeof(sn_word); }

extern "C" size_t srgan_spectral_plan_bytes(void) { return sizeof(SnPlan); }

extern "C" int srgan_spectral_plan(void* host_table, int n_records, void* plan_out) {
  SRGAN_REQUIRE(host_table && plan_out, "spectral_plan: NULL table or plan");
  SRGAN_REQUIRE(n_records > 0, "spectral_plan: a table of %d records", n_records);
  sn_word* rec = static_cast<sn_word*>(host_table);
  for (int i = 0; i < n_records; ++i, rec += kSnRecWords) {      // everything is checked before anything is written
    for (int w = SN_W; w <= SN_SIGMA; ++w)
      SRGAN_REQUIRE(rec[w] != 0 && (rec[w] & 3) == 0, "spectral_plan: record %d: pointer %d is NULL or not 4-byte aligned", i, w);
    const long long O = (long long)rec[SN_O], K = (long long)rec[SN_K];
    SRGAN_REQUIRE(O >= 1 && K >= 1 && O <= (1LL << 31) / K - 1, "spectral_plan: record %d: O = %lld, K = %lld (O, K >= 1, O * K < 2^31)",
                  i, O, K);
  }
  SnPlan plan = {n_records, 0, 0, 0, 0, 0};
  rec = static_cast<sn_word*>(host_table);
  for (int i = 0; i < n_records; ++i, rec += kSnRecWords) {
    const long long O = (long long)rec[SN_O], K = (long long)rec[SN_K];
    const long long nslab = ceil_div(O, kSnSlabRows), ncc = ceil_div(K, kSnCols), nch = ceil_div(O * K, kSnChunk);
    rec[SN_SLAB0] = (sn_word)plan.slab_items;
    rec[SN_COL0] = (sn_word)plan.col_items;
    rec[SN_ELEM0] = (sn_word)plan.elem_items;
    plan.slab_items += nslab * ncc;
    plan.col_items += ncc;
    plan.elem_items += nch;
    long long at = plan.ws_floats;               // every region starts on a 16-byte boundary
    rec[SN_WS_PART] = (sn_word)at; at += sn_round4(nslab * K);
    rec[SN_WS_T] = (sn_word)at;    at += sn_round4(K);
    rec[SN_WS_NSQ] = (sn_word)at;  at += sn_round4(ncc);
    rec[SN_WS_Y] = (sn_word)at;    at += sn_round4(O * ncc);
    rec[SN_WS_DOT] = (sn_word)at;  at += sn_round4(nch);
    rec[SN_RESERVED] = 0;
    plan.ws_floats = at;
  }
  std::memcpy(plan_out, &plan, sizeof(plan));
  return 0;
}

extern "C" size_t srgan_spectral_workspace(const void* plan) {
  const SnPlan* p = static_cast<const SnPlan*>(plan);
  if (!p || p->n_records <= 0 || p->ws_floats <= 0) {
    srgan::set_error("spectral_workspace: bad argument (a plan filled by srgan_spectral_plan)");
    return 0;
  }
  return (size_t)p->ws_floats * sizeof(float);
}

extern "C" int srgan_spectral_refresh(const void* table, const void* plan, int iterate, int n_power_iterations, float eps, void* ws,
                                      size_t ws_bytes, void* stream) {
  const SnPlan* p = static_cast<const SnPlan*>(plan);
  if (int rc = sn_check_plan("spectral_refresh", table, p, ws, ws_bytes)) return rc;
  SRGAN_REQUIRE(eps > 0.f, "spectral_refresh: eps must be > 0 (NaN refused)");
  SRGAN_REQUIRE(n_power_iterations >= 1, "spectral_refresh: n_power_iterations = %d (>= 1)", n_power_iterations);
  const sn_word* tab = static_cast<const sn_word*>(table);
  float* w = static_cast<float*>(ws);
  hipStream_t st = as_stream(stream);
  const dim3 block(256);
  if (iterate) {
    for (int i = 0; i < n_power_iterations; ++i) {
      hipLaunchKernelGGL(sn_wtu_partials_kernel, dim3(sn_grid(p->slab_items)), block, 0, st, tab, p->n_records, p->slab_items, w);
      hipLaunchKernelGGL(sn_vnorm_partials_kernel, dim3(sn_grid(p->col_items)), block, 0, st, tab, p->n_records, p->col_items, w);
      hipLaunchKernelGGL(sn_wv_partials_kernel<true>, dim3(sn_grid(p->slab_items)), block, 0, st, tab, p->n_records, p->slab_items, w,
                         eps);
      hipLaunchKernelGGL(sn_unorm_sigma_kernel<true>, dim3((unsigned)p->n_records), block, 0, st, tab, w, eps);
    }
  } else {
    hipLaunchKernelGGL(sn_wv_partials_kernel<false>, dim3(sn_grid(p->slab_items)), block, 0, st, tab, p->n_records, p->slab_items, w,
                       eps);
    hipLaunchKernelGGL(sn_unorm_sigma_kernel<false>, dim3((unsigned)p->n_records), block, 0, st, tab, w, eps);
  }
  hipLaunchKernelGGL(sn_scale_kernel, dim3(sn_grid(p->elem_items)), block, 0, st, tab, p->n_records, p->elem_items);
  return check_launch("spectral_refresh");
}

extern "C" int srgan_spectral_project(const void* table, const void* plan, const void* grads, void* ws, size_t ws_bytes, void* stream) {
  const SnPlan* p = static_cast<const SnPlan*>(plan);
  if (int rc = sn_check_plan("spectral_project", table, p, ws, ws_bytes)) return rc;
  SRGAN_REQUIRE(grads, "spectral_project: NULL gradient table");
  const sn_word* tab = static_cast<const sn_word*>(table);
  const sn_word* g = static_cast<const sn_word*>(grads);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(sn_dot_partials_kernel, dim3(sn_grid(p->elem_items)), dim3(256), 0, st, tab, p->n_records, p->elem_items, g,
                     static_cast<float*>(ws));
  hipLaunchKernelGGL(sn_project_kernel, dim3(sn_grid(p->elem_items)), dim3(256), 0, st, tab, p->n_records, p->elem_items, g,
                     static_cast<const float*>(ws));
  return check_launch("spectral_project");
}
