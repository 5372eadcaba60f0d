// Element and row criteria the fused loss kernels share (losses.hip, consistency.hip): one text, so the kernels that must agree
// bit for bit compile the same arithmetic.
#pragma once
#include <cmath>
#include "common.h"

namespace srgan {

// The criterion kinds of the templated kernels (SRGAN_CRIT_* of srgan_hip.h).  The MSE instantiations hold the arithmetic
// of the LSGAN-only kernels they replace, operation for operation.
constexpr int CRIT_MSE = SRGAN_CRIT_MSE, CRIT_BCE = SRGAN_CRIT_BCE;

// nn.BCEWithLogitsLoss of one logit against the target t (any real t): value max(x,0) - x*t + log1p(exp(-|x|)), and
// d = sigmoid(x) - t with the sigmoid evaluated from exp(-|x|) <= 1 (no overflow for either sign).
__device__ __forceinline__ float bce_logit(float x, float t, float& d) {
  const float e = expf(-fabsf(x));
  const float r = 1.f / (1.f + e);
  d = (x >= 0.f ? r : e * r) - t;
  return fmaxf(x, 0.f) - x * t + log1pf(e);
}

// nn.BCELoss of one probability p against the target y (ATen binary_cross_entropy: both logs clamped at -100)
__device__ __forceinline__ float bce_prob(float p, float log_1mp /* log(1 - p) */, float y) {
  return (y - 1.f) * fmaxf(log_1mp, -100.f) - y * fmaxf(logf(p), -100.f);
}

// One row of nn.BCELoss(softmax(z), onehot(lab)): returns the row's sum of the nc element losses, leaves q in qq and writes
// dz (may be null) = gs * d(sum)/dz.  With e_j = exp(z_j - max), q_j = e_j / den and r_j = 1 - q_j = (den - e_j) / den formed from
// the OTHER exponentials (1.f - q_j would carry q_j's rounding error at full size into a difference that can be 1e-5 of it):
//   dq_j = (q_j - y_j) / max(q_j r_j, 1e-12)          nn.BCELoss's own gradient (ATen binary_cross_entropy_backward), and
//   dz_j = q_j (dq_j - sum_i q_i dq_i) = q_j dq_j r_j - q_j sum_{i != j} q_i dq_i
// -- the softmax Jacobian with the j-th term of the sum taken out, so that a class with q -> 1 (dq ~ 1/r) does not leave the
// difference of two numbers of size 1/r.  A saturated row (q exactly 0 / 1) gives element losses of 100 and dz = 0, as ATen does.
__device__ __forceinline__ float softmax_bce_row(const float* z, int nc, int lab, float gs, float* qq, float* dz) {
  float ee[16], rr[16], t[16];
  float mx = -INFINITY;
  for (int j = 0; j < nc; ++j) mx = fmaxf(mx, z[j]);
  float den = 0.f;
  for (int j = 0; j < nc; ++j) { ee[j] = expf(z[j] - mx); den += ee[j]; }
  float s = 0.f;
  for (int j = 0; j < nc; ++j) {
    float oth = 0.f;
    for (int i = 0; i < nc; ++i) if (i != j) oth += ee[i];
    const float q = ee[j] / den, r = oth / den;
    const float y = j == lab ? 1.f : 0.f;
    qq[j] = q;
    // log(1 - q): log1p(-q) for small q (r rounds to 1), log(r) where r is the small one; a q that has rounded to 1 is a
    // saturated element for nn.BCELoss, which sees only q: log1p(-1) = -inf -> the -100 clamp
    s += bce_prob(q, (q < 0.5f || q == 1.f) ? log1pf(-q) : logf(r), y);
    const float dq = gs * (j == lab ? -r : q) / fmaxf(q * r, 1e-12f);
    t[j] = q * dq;
    rr[j] = r;
  }
  if (dz)
    for (int j = 0; j < nc; ++j) {
      float oth = 0.f;
      for (int i = 0; i < nc; ++i) if (i != j) oth += t[i];
      dz[j] = t[j] * rr[j] - qq[j] * oth;
    }
  return s;
}

}  // namespace srgan
