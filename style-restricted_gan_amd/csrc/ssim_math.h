// The arithmetic of the structural-similarity kernels (csrc/ssim.hip): the tap table of the Gaussian window, the central moments
// from the windowed moments of SHIFTED values, the SSIM quotient and its partial derivatives.  Plain C++ with no HIP dependency, so
// that a host program can evaluate the very functions the kernels run (tests/ssim_host_check.cpp does, in double, against central
// differences).  DESIGN.md section 7 ("Structural similarity") has the derivation.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SSIM_HD __host__ __device__ __forceinline__
#else
#define SSIM_HD inline
#endif

namespace srgan {

constexpr int kSsMinWindow = 3, kSsMaxWindow = 11;

// What a launch carries by value: the taps as fp32 numbers, and excess = (sum of the taps, in double)^2 - 1 -- the fp32 taps of a
// normalised window do not sum to exactly 1, and the definition's E[.] is the sum with THESE taps (ss_central puts it back).
struct SsTaps { float w[kSsMaxWindow]; float excess; int n; };

inline bool ss_window_ok(int window) { return window >= kSsMinWindow && window <= kSsMaxWindow && (window & 1) == 1; }

// exp(-d^2 / (2 sigma^2)) at d = k - (window - 1) / 2 in double, normalised to sum 1 in double (ascending), rounded to fp32
inline void ss_gaussian_taps(int window, double sigma, float* out) {
  double g[kSsMaxWindow], s = 0.0;
  for (int k = 0; k < window; ++k) {
    const double d = (double)(k - (window - 1) / 2);
    g[k] = exp(-(d * d) / (2.0 * sigma * sigma));
    s += g[k];
  }
  for (int k = 0; k < window; ++k) out[k] = (float)(g[k] / s);
}

inline SsTaps ss_taps(const float* taps, int window) {
  SsTaps t = {};
  double s = 0.0;
  for (int k = 0; k < window; ++k) { t.w[k] = taps[k]; s += (double)taps[k]; }
  t.excess = (float)(s * s - 1.0);
  t.n = window;
  return t;
}

// With x' = x - px, y' = y - py and m1..m5 = E[x'], E[y'], E[x'^2], E[y'^2], E[x'y'] (E = the sum over the window with the product
// taps, whose total is 1 + excess): dx = mu_x - px, dy = mu_y - py and the definition's s_x = E[x^2] - mu_x^2, s_y, s_xy.  The
// differences m3 - m1^2 are those of SMALL numbers (the pivot is a pixel of the plane); the terms in `excess` are what the
// definition's raw form holds on top of the shift-invariant one, of relative size 1e-8.
template <class T>
struct SsCentral { T dx, dy, sx, sy, sxy; };

template <class T>
SSIM_HD SsCentral<T> ss_central(T m1, T m2, T m3, T m4, T m5, T px, T py, T excess) {
  SsCentral<T> c;
  const T tot = (T)1 + excess;
  c.dx = m1 + px * excess;
  c.dy = m2 + py * excess;
  c.sx = (m3 - m1 * m1) - excess * (px * ((T)2 * m1 + px * tot));
  c.sy = (m4 - m2 * m2) - excess * (py * ((T)2 * m2 + py * tot));
  c.sxy = (m5 - m1 * m2) - excess * (px * m2 + py * m1 + px * py * tot);
  return c;
}

// SSIM = (2 a b + c1)(2 s_xy + c2) / ((a^2 + b^2 + c1)(s_x + s_y + c2)) at a = mu_x, b = mu_y, and its partial derivatives with
// a, b, s_x, s_y, s_xy as independent variables.  d/ds_x = d/ds_y = g_s.
template <class T>
struct SsPoint { T value, g_mux, g_muy, g_s, g_sxy; };

template <class T>
SSIM_HD SsPoint<T> ss_point(T a, T b, T sx, T sy, T sxy, T c1, T c2) {
  const T a1 = (T)2 * a * b + c1, a2 = (T)2 * sxy + c2;
  const T b1 = a * a + b * b + c1, b2 = sx + sy + c2;
  SsPoint<T> p;
  p.value = (a1 * a2) / (b1 * b2);
  const T r = a2 / b2, t = (T)2 / b1;
  p.g_mux = t * (b * r - a * p.value);
  p.g_muy = t * (a * r - b * p.value);
  p.g_s = -p.value / b2;
  p.g_sxy = ((T)2 * a1) / (b1 * b2);
  return p;
}

}  // namespace srgan
