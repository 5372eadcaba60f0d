// Geometric augmentation of the images the discriminator reads -- x-flip, 90-degree turns, isotropic scale, arbitrary rotation (the
// pixel-blitting and geometric groups of Karras et al., 2020) as ONE bilinear affine warp per sample: extension, no counterpart in
// the reference; a second stage after csrc/augment.hip with kernels of its own.  fp32, NHWC-dense, three channels, in both compute
// modes.  DESIGN.md section 7 ("Geometric augmentation") has the formulas; csrc/geom_math.h the arithmetic, shared with a host test.
//
// One table row of 8 floats per sample: [fx, k, zoom, cos, sin, 0, 0, mask]; the groups that run (flags: flip 1, rot90 2, scale 4,
// rotate 8) are a launch argument, a group that is off takes its identity value.  With cen = ((H - 1) / 2, (W - 1) / 2):
//   forward   y[q] = bilinear(x, s(q)),  s(q) = cen + R(cos, sin) Q(k) F(fx) (q - cen) / zoom;  a neighbour outside the image reads 0
//   backward  gx[p] = sum_q hat(s_i(q) - p_i) hat(s_j(q) - p_j) gy[q],  hat(t) = max(0, 1 - |t|), over the (2 r + 1)^2 output pixels
//             around round(q*), q* = cen + zoom (R Q F)^T (p - cen), r = min(ceil(zoom (|cos| + |sin|)), 3): a superset of the
//             support (|q - q*|_inf < zoom (|cos| + |sin|)), a candidate outside it weighs exactly 0; row-major, serial.
// One launch each way.  An item = 2048 consecutive pixels of one sample: a thread owns 4 consecutive pixels = three 16-byte stores
// (scalar path: pixel t + 256 u); the gathers are scalar.  No atomics, every sum has one owner and a fixed order: a sample's result
// depends neither on N nor on its position in the batch nor on the grid.  fp contraction is off: both paths round alike.
//
// Gated form (adaptive augmentation, csrc/ada.hip writes the tables): slot 7 of a row is a skip mask, an exact float in 0..15 with
// the bits of flags.  A group whose bit is set takes its identity value for that sample, so the sample comes out as the ungated
// kernel gives it with flags & ~mask, bit for bit.  A sample without a group left is a bit copy, in both forms; an item belongs to
// one sample, so that branch is uniform per workgroup iteration.  The ungated kernels never read slot 7.
//
// What "a pure flip / rot90 row is a permutation" means: every sample that is NOT a bit copy goes through the weighted sum
// 0 + x * 1 (+ neighbours * 0 where they exist), so its values are equal to the permuted input's but a -0.0 comes out as +0.0, and a
// non-finite neighbour under a zero weight (inf * 0) makes the pixel a NaN.  Finite inputs of either zero sign compare equal.
#include "common.h"
#include <algorithm>
#include <cstdint>

#pragma clang fp contract(off)

#include "geom_math.h"

namespace srgan {

constexpr int kGeomItemPixels = 2048;   // pixels per item (kAugItemPixels of augment.hip)
constexpr int kGeomGridCap = 2048;      // 256 CUs x 8 workgroups; the rest by grid stride (kAugGridCap)

// y[q], three channels
__device__ __forceinline__ void geom_fwd_pixel(const float* __restrict__ src, const GeomXf& g, int q, float& v0, float& v1, float& v2) {
  const int qi = q / g.W, qj = q - qi * g.W;
  float si, sj;
  geom_src(g, qi, qj, &si, &sj);
  const GeomTaps t = geom_taps(si, sj);
  v0 = v1 = v2 = 0.f;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int i = t.i0 + a, j = t.j0 + b;
      if (geom_inside(i, j, g.H, g.W)) {
        const float wgt = (a ? t.fi : 1.f - t.fi) * (b ? t.fj : 1.f - t.fj);
        const float* s = src + ((size_t)i * g.W + j) * 3;
        v0 += s[0] * wgt; v1 += s[1] * wgt; v2 += s[2] * wgt;
      }
    }
  }
}

// gx[p], three channels
__device__ __forceinline__ void geom_bwd_pixel(const float* __restrict__ gy, const GeomXf& g, int p, float& v0, float& v1, float& v2) {
  const int pi = p / g.W, pj = p - pi * g.W;
  int ri, rj;
  geom_centre(g, pi, pj, &ri, &rj);
  v0 = v1 = v2 = 0.f;
  for (int qi = ri - g.radius; qi <= ri + g.radius; ++qi) {
    for (int qj = rj - g.radius; qj <= rj + g.radius; ++qj) {
      if (!geom_inside(qi, qj, g.H, g.W)) continue;
      float si, sj;
      geom_src(g, qi, qj, &si, &sj);
      const float wgt = geom_hat(si - (float)pi) * geom_hat(sj - (float)pj);
      const float* s = gy + ((size_t)qi * g.W + qj) * 3;
      v0 += s[0] * wgt; v1 += s[1] * wgt; v2 += s[2] * wgt;
    }
  }
}

template <bool BWD>
__device__ __forceinline__ void geom_pixel(const float* __restrict__ src, const GeomXf& g, int p, float& v0, float& v1, float& v2) {
  if (BWD) geom_bwd_pixel(src, g, p, v0, v1, v2);
  else geom_fwd_pixel(src, g, p, v0, v1, v2);
}

// the body of both kernels: `x` is the image (forward) or the output's gradient (backward), `y` what is written
template <bool BWD, bool GATED>
__device__ __forceinline__ void geom_items(const float* __restrict__ x, const float* __restrict__ table, float* __restrict__ y, int H,
                                           int W, int flags, int nitem, long long items, int vec) {
  const int P = H * W;
  const size_t E = (size_t)P * 3;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int n = (int)(it / nitem), item = (int)(it - (long long)n * nitem);
    const float* src = x + (size_t)n * E;
    float* dst = y + (size_t)n * E;
    const float* row = table + (size_t)n * kGeomRow;
    const int F = geom_flags(row, flags, GATED);
    const GeomXf g = geom_xf(geom_sanitise(row, F), H, W);
    const int base = item * kGeomItemPixels;
    if (vec) {                                                      // P % 4 == 0, x / y 16-byte aligned
#pragma unroll
      for (int u = 0; u < kGeomItemPixels / 1024; ++u) {
        const int p0 = base + (u * 256 + (int)threadIdx.x) * 4;
        if (p0 >= P) continue;
        float* d = dst + (size_t)p0 * 3;
        if (F == 0) {                                               // nothing left for this sample: a bit copy
          const float* s = src + (size_t)p0 * 3;
#pragma unroll
          for (int q = 0; q < 3; ++q) *reinterpret_cast<f32x4*>(d + 4 * q) = *reinterpret_cast<const f32x4*>(s + 4 * q);
          continue;
        }
        float v[12];
#pragma unroll
        for (int q = 0; q < 4; ++q) geom_pixel<BWD>(src, g, p0 + q, v[3 * q], v[3 * q + 1], v[3 * q + 2]);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const f32x4 t = {v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
          *reinterpret_cast<f32x4*>(d + 4 * q) = t;
        }
      }
    } else {
#pragma unroll 2
      for (int u = 0; u < kGeomItemPixels / 256; ++u) {
        const int p = base + u * 256 + (int)threadIdx.x;
        if (p >= P) continue;
        float* d = dst + (size_t)p * 3;
        float v0, v1, v2;
        if (F == 0) {
          const float* s = src + (size_t)p * 3;
          v0 = s[0]; v1 = s[1]; v2 = s[2];
        } else {
          geom_pixel<BWD>(src, g, p, v0, v1, v2);
        }
        d[0] = v0; d[1] = v1; d[2] = v2;
      }
    }
  }
}

template <bool GATED>
__global__ __launch_bounds__(256) void geom_fwd_kernel(const float* __restrict__ x, const float* __restrict__ table,
                                                       float* __restrict__ y, int H, int W, int flags, int nitem, long long items,
                                                       int vec) {
  geom_items<false, GATED>(x, table, y, H, W, flags, nitem, items, vec);
}

template <bool GATED>
__global__ __launch_bounds__(256) void geom_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ table,
                                                       float* __restrict__ gx, int H, int W, int flags, int nitem, long long items,
                                                       int vec) {
  geom_items<true, GATED>(gy, table, gx, H, W, flags, nitem, items, vec);
}

template <bool BWD, bool GATED>
static void geom_launch(dim3 grid, hipStream_t st, const float* x, const float* table, float* y, int h, int w, int flags, int nitem,
                        long long items, int vec) {
  if constexpr (BWD) hipLaunchKernelGGL((geom_bwd_kernel<GATED>), grid, dim3(256), 0, st, x, table, y, h, w, flags, nitem, items, vec);
  else hipLaunchKernelGGL((geom_fwd_kernel<GATED>), grid, dim3(256), 0, st, x, table, y, h, w, flags, nitem, items, vec);
}

template <bool BWD>
static int geom_run(const char* what, const float* x, const float* table, float* y, int n, int c, int h, int w, int flags, int gated,
                    void* stream) {
  SRGAN_REQUIRE(c == 3, "%s: C = %d (three-channel images only)", what, c);
  SRGAN_REQUIRE(x && table && y, "%s: null pointer", what);
  SRGAN_REQUIRE((flags & ~GEOM_ALL) == 0, "%s: flags = %d (flip 1, rot90 2, scale 4, rotate 8)", what, flags);
  SRGAN_REQUIRE(n > 0 && h > 0 && w > 0 && (long long)h * w <= (1LL << 29), "%s: N = %d, H = %d, W = %d (all > 0, H W <= 2^29)", what,
                n, h, w);
  SRGAN_REQUIRE(static_cast<const void*>(x) != static_cast<const void*>(y), "%s: the result must not alias the source", what);
  const int nitem = (int)ceil_div((long long)h * w, kGeomItemPixels);
  const long long items = (long long)n * nitem;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y);
  const int vec = (bits & 15) == 0 && ((long long)h * w) % 4 == 0;
  const dim3 grid((unsigned)std::min<long long>(items, kGeomGridCap));
  hipStream_t st = as_stream(stream);
  if (gated) geom_launch<BWD, true>(grid, st, x, table, y, h, w, flags, nitem, items, vec);
  else geom_launch<BWD, false>(grid, st, x, table, y, h, w, flags, nitem, items, vec);
  return check_launch(what);
}

}  // namespace srgan

extern "C" int srgan_geom_augment_fwd(const float* x, const float* table, float* y, int n, int c, int h, int w, int flags, int gated,
                                      void* stream) {
  return srgan::geom_run<false>("geom_augment_fwd", x, table, y, n, c, h, w, flags, gated, stream);
}

extern "C" int srgan_geom_augment_bwd(const float* gy, const float* table, float* gx, int n, int c, int h, int w, int flags, int gated,
                                      void* stream) {
  return srgan::geom_run<true>("geom_augment_bwd", gy, table, gx, n, c, h, w, flags, gated, stream);
}
