// The arithmetic of the set metrics (csrc/metrics.hip): the polynomial kernel of KID, the round-robin pairing of the one-sided
// Jacobi sweep, its skip rule and its rotation.  Plain C++ with no HIP dependency, so that a host program can run the very
// functions the kernels run (tests/metric_host_check.cpp).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define METRIC_HD __host__ __device__ __forceinline__
#else
#define METRIC_HD inline
#endif

namespace srgan {

constexpr float kEps32 = 1.1920929e-7f;      // 2^-23, numpy's finfo(float32).eps

// KID's kernel k = (g / D + 1)^3 of one Gram entry: four fp32 roundings (divide, add, two products); (float)D is exact below 2^24
METRIC_HD float kid_poly3(float g, int D) {
  const float v = g / (float)D + 1.f;
  return v * v * v;
}

// Round-robin tournament (circle method) over np players, np even: round r in [0, np - 2], slot k in [0, np / 2).  Player
// np - 1 stays put and meets r in slot 0; slot k >= 1 pairs r + k with r - k modulo np - 1.  Every unordered pair meets once
// in the np - 1 rounds and no player twice in a round.  Returned with *i < *j, so a phantom player (np - 1, when the real
// count is odd) is always *j of slot 0.
METRIC_HD void jacobi_pair(int np, int round, int slot, int* i, int* j) {
  const int q = np - 1;
  int a, b;
  if (slot == 0) {
    a = q; b = round;
  } else {
    a = (round + slot) % q;
    b = (round - slot + q) % q;
  }
  *i = a < b ? a : b;
  *j = a < b ? b : a;
}

// a = |wi|^2, b = |wj|^2, g = wi . wj: the pair counts as orthogonal when |g| <= 4 eps sqrt(a b), and is left alone when
// sqrt(a b) <= eps^2 |W|_F^2 (a vector that is zero to working precision has no direction to rotate).  sqrt(a) sqrt(b) rather
// than sqrt(a b): the product of two squared norms may leave the fp32 range.  A NaN anywhere skips.
METRIC_HD bool jacobi_skip(float a, float b, float g, float frob2) {
  const float sab = sqrtf(a) * sqrtf(b);
  return !(fabsf(g) > 4.f * kEps32 * sab) || !(sab > kEps32 * kEps32 * frob2);
}

struct JacobiRot { float t, c, s; };

// zeta = (b - a) / (2 g); t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), the smaller root of t^2 + 2 zeta t - 1 = 0;
// c = 1 / sqrt(1 + t^2), s = c t.  From |zeta| = 2^13 on, 1 + zeta^2 rounds to zeta^2 in fp32, so sqrt(1 + zeta^2) is |zeta|
// itself there and zeta^2 is never formed where it could overflow; an infinite zeta gives t = 0, the identity.  zeta = 0
// (equal norms) takes the sign of the zero: |t| = 1, a rotation by 45 degrees.
METRIC_HD JacobiRot jacobi_rotation_zeta(float zeta) {
  const float az = fabsf(zeta);
  const float root = az >= 8192.f ? az : sqrtf(az * az + 1.f);
  JacobiRot r;
  r.t = copysignf(1.f, zeta) / (az + root);
  r.c = 1.f / sqrtf(r.t * r.t + 1.f);
  r.s = r.c * r.t;
  return r;
}

METRIC_HD JacobiRot jacobi_rotation(float a, float b, float g) { return jacobi_rotation_zeta((b - a) / (2.f * g)); }

// wi' = c wi - s wj, wj' = s wi + c wj: the new wi' . wj' = c s (a - b) + (c^2 - s^2) g = 0 for the t above
METRIC_HD void jacobi_apply(const JacobiRot& r, float* x, float* y) {
  const float u = *x, v = *y;
  *x = r.c * u - r.s * v;
  *y = r.s * u + r.c * v;
}

}  // namespace srgan
