// Differentiable augmentation (DiffAugment: Zhao et al., 2020) of the images the discriminator reads: extension, no counterpart in
// the reference.  fp32, NHWC-dense, three channels, in both compute modes.  DESIGN.md section 7 ("DiffAugment") has the formulas.
//
// One table row of 8 floats per sample: [b, s, a, ty, tx, cy, cx, 0] (the integers as exact floats); the cutout window ch x cw and
// the groups that run (flags: colour 1, translation 2, cutout 4) are launch arguments.  A written pixel w = (i, j) reads pixel
// r = w + (ty, tx) (forward) or r = w - (ty, tx) (backward); a pixel outside the image reads 0.  The cutout window zeroes OUTPUT
// pixels: the forward tests w, the backward tests r.  Colour is per pixel once the sample's sum is known:
//   forward   M = sum(x) / (3 H W) + b;  x1 = x + b;  m = (x1[0] + x1[1] + x1[2]) / 3;  x2 = (x1 - m) s + m;  y = (x2 - M) a + M
//   backward  gx[c] = a s g'[c] + a (1 - s) / 3 * (g'[0] + g'[1] + g'[2]) + (1 - a) / (3 H W) * sum(g')
// Two launches each way with colour on, one with colour off (pure copy-or-zero, no arithmetic):
//   1 aug_sum_partials  part[n][chunk] = sum over 4096 consecutive floats of sample n (the backward: of the gy elements whose
//                       pixel survives cutout and translation).  Element e of a chunk belongs to thread (e / 4) % 256, slot
//                       (e / 1024) * 4 + e % 4 on the 16-byte and on the scalar path: 16 serial adds, then the block sum.
//   2 aug_apply         every workgroup first adds its sample's partials (thread-strided serial, then the block sum), then one
//                       item = 2048 pixels of one sample: a thread owns 4 consecutive pixels = three 16-byte stores (scalar path:
//                       pixel t + 256 k); the gather reads the same 48 bytes at a 4-byte aligned address when all four pixels exist.
// No atomics, every sum has one owner and a fixed order that depends on H and W only: a sample's result does not depend on N, on
// its position in the batch or on the grid.  fp contraction is off: both paths of a kernel round alike.
//
// Gated form (srgan_diffaugment_fwd_gated / _bwd_gated; adaptive augmentation, csrc/ada.hip writes the tables): slot 7 of a row is
// a skip mask, an exact float in 0..7 with the bits of flags.  A group whose bit is set is not applied to that sample -- no colour
// arithmetic, shift (0, 0), empty window -- so the sample comes out as the ungated kernels give it with flags & ~mask, bit for bit;
// all launched groups skipped: a bit copy.  An item belongs to one sample: the branch is uniform per workgroup iteration.  The
// partial sums of a sample whose colour bit is skipped are neither written nor read.  The ungated kernels never read slot 7.
#include "common.h"
#include <algorithm>
#include <cstdint>

#pragma clang fp contract(off)

namespace srgan {

constexpr int kAugChunk = 4096;        // floats per partial sum
constexpr int kAugItemPixels = 2048;   // pixels per item of the apply pass
constexpr int kAugGridCap = 2048;      // 256 CUs x 8 workgroups; the rest by grid stride
constexpr int kAugRow = 8;             // floats per table row
enum { AUG_B, AUG_S, AUG_A, AUG_TY, AUG_TX, AUG_CY, AUG_CX, AUG_SKIP };

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));     // a 16-byte access at a 4-byte aligned address

struct AugGeom {
  int H, W;
  int dy, dx;            // read pixel = written pixel + (dy, dx)
  int r0, r1, c0, c1;    // cutout rows [r0, r1) and columns [c0, c1); empty when the group is off
};

// a table integer; whatever the float holds, the index arithmetic below stays inside int (|value| <= 2^29, a NaN reads -2^29)
__device__ __forceinline__ int aug_int(float v) { return (int)fminf(fmaxf(v, -536870912.f), 536870912.f); }

// the groups that run for the sample of `row`: the launch's, less (gated form) those of the row's skip mask.  Whatever slot 7
// holds, the mask is in 0..7 (8.0 and 1e30 read 0, -1.0 reads 7, a NaN reads 0).
template <int FLAGS, bool GATED>
__device__ __forceinline__ int aug_flags(const float* __restrict__ row) {
  return GATED ? (FLAGS & ~(aug_int(row[AUG_SKIP]) & 7)) : FLAGS;
}

// `flags`: aug_flags() of the sample, a compile-time constant in the ungated kernels
template <bool BWD>
__device__ __forceinline__ AugGeom aug_geom(const float* __restrict__ row, int H, int W, int ch, int cw, int flags) {
  AugGeom g = {H, W, 0, 0, 0, 0, 0, 0};
  if (flags & 2) {                        // a shift of the whole size already moves everything out
    g.dy = min(max(aug_int(row[AUG_TY]), -H), H);
    g.dx = min(max(aug_int(row[AUG_TX]), -W), W);
    if (BWD) { g.dy = -g.dy; g.dx = -g.dx; }
  }
  if (flags & 4) {
    g.r0 = aug_int(row[AUG_CY]) - ch / 2;
    g.c0 = aug_int(row[AUG_CX]) - cw / 2;
    g.r1 = g.r0 + ch;
    g.c1 = g.c0 + cw;
  }
  return g;
}

__device__ __forceinline__ bool aug_inside(const AugGeom& g, int i, int j) {
  return (unsigned)i < (unsigned)g.H && (unsigned)j < (unsigned)g.W;
}
__device__ __forceinline__ bool aug_cut(const AugGeom& g, int i, int j) { return i >= g.r0 && i < g.r1 && j >= g.c0 && j < g.c1; }

// does written pixel (i, j) read a pixel of the source (and not a zero)?
template <bool BWD>
__device__ __forceinline__ bool aug_reads(const AugGeom& g, int i, int j) {
  const int ri = i + g.dy, rj = j + g.dx;
  return aug_inside(g, ri, rj) && !(BWD ? aug_cut(g, ri, rj) : aug_cut(g, i, j));
}

struct AugColour { float k0, k1, k2, k3; };

// forward: {b, s, a, M}; backward: {a s, a (1 - s) / 3, (1 - a) / (3 H W) * sum, unused}
template <bool BWD>
__device__ __forceinline__ AugColour aug_colour(const float* __restrict__ row, float sum, float elems) {
  const float b = row[AUG_B], s = row[AUG_S], a = row[AUG_A];
  if (BWD) return {a * s, a * (1.f - s) / 3.f, (1.f - a) / elems * sum, 0.f};
  return {b, s, a, sum / elems + b};
}

template <bool BWD>
__device__ __forceinline__ void aug_pixel(const AugColour& k, float& v0, float& v1, float& v2) {
  if (BWD) {
    const float t = (v0 + v1 + v2) * k.k1 + k.k2;
    v0 = v0 * k.k0 + t;
    v1 = v1 * k.k0 + t;
    v2 = v2 * k.k0 + t;
  } else {
    v0 += k.k0; v1 += k.k0; v2 += k.k0;
    const float m = (v0 + v1 + v2) / 3.f;
    v0 = ((v0 - m) * k.k1 + m - k.k3) * k.k2 + k.k3;
    v1 = ((v1 - m) * k.k1 + m - k.k3) * k.k2 + k.k3;
    v2 = ((v2 - m) * k.k1 + m - k.k3) * k.k2 + k.k3;
  }
}

// sum over the 256 threads of a workgroup: butterfly inside each wave, then (w0 + w1) + (w2 + w3); every thread gets the sum
__device__ __forceinline__ float aug_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();                            // the previous use of red[]
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// sample n of the batch the two sources make up
__device__ __forceinline__ const float* aug_sample(const float* __restrict__ x0, int n0, const float* __restrict__ x1, int n, size_t E) {
  return n < n0 ? x0 + (size_t)n * E : x1 + (size_t)(n - n0) * E;
}

template <int FLAGS, bool BWD, bool GATED>
__global__ __launch_bounds__(256) void aug_sum_partials_kernel(const float* __restrict__ x0, int n0, const float* __restrict__ x1,
                                                               const float* __restrict__ table, float* __restrict__ part, int H, int W,
                                                               int ch, int cw, int nchunk, long long items, int vec) {
  __shared__ float red[4];
  const int E = 3 * H * W;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int n = (int)(it / nchunk), chunk = (int)(it - (long long)n * nchunk);
    const float* src = aug_sample(x0, n0, x1, n, (size_t)E);
    const int F = aug_flags<FLAGS, GATED>(table + (size_t)n * kAugRow);
    if (GATED && !(F & 1)) continue;                                 // colour skipped for this sample: nobody reads its partials
    const AugGeom g = aug_geom<false>(table + (size_t)n * kAugRow, H, W, ch, cw, F);        // gy is indexed by the OUTPUT pixel
    float acc = 0.f;
#pragma unroll
    for (int jv = 0; jv < 4; ++jv) {
      const int e0 = chunk * kAugChunk + (jv * 256 + (int)threadIdx.x) * 4;
      if (e0 >= E) continue;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (vec) {                                                    // E % 4 == 0: the four elements exist
        v = *reinterpret_cast<const f32x4*>(src + e0);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (e0 + q < E) v[q] = src[e0 + q];
      }
      if (BWD && (F & 6)) {                                          // the gradient of a pixel no output reads does not count
        int p = e0 / 3, c = e0 - 3 * p;
        int i = p / W, j = p - i * W;
        bool keep = aug_reads<false>(g, i, j);                       // the forward's test: not cut, and its source pixel exists
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          acc += keep ? v[q] : 0.f;
          if (++c == 3) {
            c = 0;
            if (++j == W) { j = 0; ++i; }
            keep = aug_reads<false>(g, i, j);
          }
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc += v[q];
      }
    }
    acc = aug_block_sum(acc, red);
    if (threadIdx.x == 0) part[it] = acc;
  }
}

// four consecutive pixels starting at pixel p0 (p0 % 4 == 0, all four exist)
// FLAGS: the launch's (may the read address be off 16-byte alignment?); F: the sample's
template <int FLAGS, bool BWD>
__device__ __forceinline__ void aug_quad(const float* __restrict__ src, float* __restrict__ dst, const AugGeom& g, const AugColour& k,
                                         int p0, int F) {
  int i = p0 / g.W, j = p0 - i * g.W;
  bool rd[4];
  bool all = true;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    rd[q] = aug_reads<BWD>(g, i, j);
    all = all && rd[q];
    if (++j == g.W) { j = 0; ++i; }
  }
  // the read pixels of a quad are consecutive in memory whenever they all exist: pixel index + dy * W + dx
  const long long shift = (long long)g.dy * g.W + g.dx;
  const float* s = src + ((long long)p0 + shift) * 3;
  float v[12];
  if (all) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const f32x4 t = (FLAGS & 2) ? (f32x4)*reinterpret_cast<const f32x4u*>(s + 4 * q) : *reinterpret_cast<const f32x4*>(s + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * q + e] = t[e];
    }
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[3 * q + c] = rd[q] ? s[3 * q + c] : 0.f;
    }
  }
  if (F & 1) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (BWD || rd[q]) aug_pixel<BWD>(k, v[3 * q], v[3 * q + 1], v[3 * q + 2]);      // forward: a zero pixel stays zero
    }
  }
  float* d = dst + (size_t)p0 * 3;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const f32x4 t = {v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
    *reinterpret_cast<f32x4*>(d + 4 * q) = t;
  }
}

template <bool BWD>
__device__ __forceinline__ void aug_one(const float* __restrict__ src, float* __restrict__ dst, const AugGeom& g, const AugColour& k,
                                        int p, int F) {
  const int i = p / g.W, j = p - i * g.W;
  const bool rd = aug_reads<BWD>(g, i, j);
  const float* s = src + ((long long)p + (long long)g.dy * g.W + g.dx) * 3;
  float v0 = rd ? s[0] : 0.f, v1 = rd ? s[1] : 0.f, v2 = rd ? s[2] : 0.f;
  if ((F & 1) && (BWD || rd)) aug_pixel<BWD>(k, v0, v1, v2);
  float* d = dst + (size_t)p * 3;
  d[0] = v0; d[1] = v1; d[2] = v2;
}

template <int FLAGS, bool BWD, bool GATED>
__global__ __launch_bounds__(256) void aug_apply_kernel(const float* __restrict__ x0, int n0, const float* __restrict__ x1,
                                                        const float* __restrict__ table, const float* __restrict__ part,
                                                        float* __restrict__ y, int H, int W, int ch, int cw, int nchunk, int nitem,
                                                        long long items, int vec) {
  __shared__ float red[4];
  const int P = H * W;
  const size_t E = (size_t)P * 3;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int n = (int)(it / nitem), item = (int)(it - (long long)n * nitem);
    const float* src = aug_sample(x0, n0, x1, n, E);
    float* dst = y + (size_t)n * E;
    const float* row = table + (size_t)n * kAugRow;
    const int F = aug_flags<FLAGS, GATED>(row);
    const AugGeom g = aug_geom<BWD>(row, H, W, ch, cw, F);
    AugColour k = {0.f, 0.f, 0.f, 0.f};
    if (F & 1) {
      float sum = 0.f;
      for (int c = threadIdx.x; c < nchunk; c += 256) sum += part[(size_t)n * nchunk + c];
      sum = aug_block_sum(sum, red);
      k = aug_colour<BWD>(row, sum, (float)E);
    }
    const int base = item * kAugItemPixels;
    if (vec) {                                                      // P % 4 == 0, x0 / x1 / y 16-byte aligned
#pragma unroll
      for (int u = 0; u < kAugItemPixels / 1024; ++u) {
        const int p0 = base + (u * 256 + (int)threadIdx.x) * 4;
        if (p0 < P) aug_quad<FLAGS, BWD>(src, dst, g, k, p0, F);
      }
    } else {
#pragma unroll 2
      for (int u = 0; u < kAugItemPixels / 256; ++u) {
        const int p = base + u * 256 + (int)threadIdx.x;
        if (p < P) aug_one<BWD>(src, dst, g, k, p, F);
      }
    }
  }
}

struct AugPlan { int nchunk, nitem; long long sum_items, apply_items; };

static bool aug_plan(int n, int h, int w, AugPlan* p) {
  if (n <= 0 || h <= 0 || w <= 0 || (long long)h * w > (1LL << 29)) return false;       // 3 H W < 2^31
  const long long P = (long long)h * w;
  p->nchunk = (int)ceil_div(3 * P, kAugChunk);
  p->nitem = (int)ceil_div(P, kAugItemPixels);
  p->sum_items = (long long)n * p->nchunk;
  p->apply_items = (long long)n * p->nitem;
  return true;
}

static unsigned aug_grid(long long items) { return (unsigned)std::min<long long>(items, kAugGridCap); }

template <int FLAGS, bool BWD, bool GATED>
static void aug_launch(const float* x0, int n0, const float* x1, const float* table, float* y, int h, int w, int ch, int cw,
                       const AugPlan& p, float* ws, int vec, hipStream_t st) {
  if constexpr ((FLAGS & 1) != 0)
    hipLaunchKernelGGL((aug_sum_partials_kernel<FLAGS, BWD, GATED>), dim3(aug_grid(p.sum_items)), dim3(256), 0, st, x0, n0, x1,
                       table, ws, h, w, ch, cw, p.nchunk, p.sum_items, vec);
  hipLaunchKernelGGL((aug_apply_kernel<FLAGS, BWD, GATED>), dim3(aug_grid(p.apply_items)), dim3(256), 0, st, x0, n0, x1, table,
                     static_cast<const float*>(ws), y, h, w, ch, cw, p.nchunk, p.nitem, p.apply_items, vec);
}

template <bool BWD, bool GATED>
static int aug_run(const char* what, const float* x0, int n0, const float* x1, int n1, const float* table, float* y, int c, int h,
                   int w, int flags, int ch, int cw, void* ws, size_t ws_bytes, void* stream) {
  SRGAN_REQUIRE(c == 3, "%s: C = %d (three-channel images only)", what, c);
  SRGAN_REQUIRE(x0 && table && y, "%s: null pointer", what);
  SRGAN_REQUIRE(n0 > 0 && n1 >= 0 && (x1 != nullptr) == (n1 > 0), "%s: n0 = %d, n1 = %d (n0 > 0; n1 > 0 with a second source only)",
                what, n0, n1);
  SRGAN_REQUIRE((flags & ~7) == 0, "%s: flags = %d (colour 1, translation 2, cutout 4)", what, flags);
  SRGAN_REQUIRE(ch >= 0 && cw >= 0 && ch <= (1 << 29) && cw <= (1 << 29), "%s: cutout window %d x %d", what, ch, cw);
  AugPlan p;
  SRGAN_REQUIRE((long long)n0 + n1 < (1LL << 31) && aug_plan(n0 + n1, h, w, &p), "%s: N = %d + %d, H = %d, W = %d (all > 0, H W <= 2^29)",
                what, n0, n1, h, w);
  if (flags & 1) {
    SRGAN_REQUIRE(ws, "%s: null workspace", what);
    SRGAN_REQUIRE(ws_bytes >= (size_t)p.sum_items * sizeof(float), "%s: workspace of %zu bytes, %zu needed", what, ws_bytes,
                  (size_t)p.sum_items * sizeof(float));
  }
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(x1) | reinterpret_cast<uintptr_t>(y);
  const int vec = (bits & 15) == 0 && ((long long)h * w) % 4 == 0;
  hipStream_t st = as_stream(stream);
  float* wsf = static_cast<float*>(ws);
  switch (flags) {
#define AUG_CASE(F) case F: aug_launch<F, BWD, GATED>(x0, n0, x1, table, y, h, w, ch, cw, p, wsf, vec, st); break;
    AUG_CASE(0) AUG_CASE(1) AUG_CASE(2) AUG_CASE(3) AUG_CASE(4) AUG_CASE(5) AUG_CASE(6) AUG_CASE(7)
#undef AUG_CASE
  }
  return check_launch(what);
}

}  // namespace srgan

using namespace srgan;

extern "C" size_t srgan_diffaugment_workspace(int n, int h, int w) {
  AugPlan p;
  if (!aug_plan(n, h, w, &p)) {
    srgan::set_error("diffaugment_workspace: N = %d, H = %d, W = %d (all > 0, H W <= 2^29)", n, h, w);
    return 0;
  }
  return (size_t)p.sum_items * sizeof(float);
}

extern "C" int srgan_diffaugment_fwd(const float* x0, int n0, const float* x1, int n1, const float* table, float* y, int c, int h,
                                     int w, int flags, int cut_h, int cut_w, void* ws, size_t ws_bytes, void* stream) {
  return aug_run<false, false>("diffaugment_fwd", x0, n0, x1, n1, table, y, c, h, w, flags, cut_h, cut_w, ws, ws_bytes, stream);
}

extern "C" int srgan_diffaugment_bwd(const float* gy, const float* table, float* gx, int n, int c, int h, int w, int flags,
                                     int cut_h, int cut_w, void* ws, size_t ws_bytes, void* stream) {
  return aug_run<true, false>("diffaugment_bwd", gy, n, nullptr, 0, table, gx, c, h, w, flags, cut_h, cut_w, ws, ws_bytes, stream);
}

extern "C" int srgan_diffaugment_fwd_gated(const float* x0, int n0, const float* x1, int n1, const float* table, float* y, int c, int h,
                                           int w, int flags, int cut_h, int cut_w, void* ws, size_t ws_bytes, void* stream) {
  return aug_run<false, true>("diffaugment_fwd_gated", x0, n0, x1, n1, table, y, c, h, w, flags, cut_h, cut_w, ws, ws_bytes, stream);
}

extern "C" int srgan_diffaugment_bwd_gated(const float* gy, const float* table, float* gx, int n, int c, int h, int w, int flags,
                                           int cut_h, int cut_w, void* ws, size_t ws_bytes, void* stream) {
  return aug_run<true, true>("diffaugment_bwd_gated", gy, n, nullptr, 0, table, gx, c, h, w, flags, cut_h, cut_w, ws, ws_bytes, stream);
}
