// The arithmetic of the geometric augmentation (csrc/augment_geom.hip): table row -> sanitised parameters -> the affine maps,
// the source position s(q) of an output pixel, its four taps, the window centre q* and radius of the gather-form adjoint.  Plain
// C++ with no HIP dependency, so that a host program can sweep the very functions the kernels run (tests/geom_host_sweep.cpp).
//
// Contract, whatever a row holds: zoom in [0.5, 2] (non-finite reads 1); fx in {0, 1} and k in {0..3} (the float clamped to
// +-2^29, truncated, masked; non-finite reads 0); a non-finite cos or sin makes the rotation the identity; the radius is <= 3;
// every coordinate is clamped into a range that converts to int before the conversion.  The callers bounds-test every index as
// an integer.  Compile with fp contraction off: both kernels and the host restatement round alike.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define GEOM_HD __host__ __device__ __forceinline__
#else
#define GEOM_HD inline
#endif

namespace srgan {

enum { GEOM_FX, GEOM_K, GEOM_ZOOM, GEOM_COS, GEOM_SIN, GEOM_PAD5, GEOM_PAD6, GEOM_SKIP };
enum { GEOM_FLIP = 1, GEOM_ROT90 = 2, GEOM_SCALE = 4, GEOM_ROTATE = 8, GEOM_ALL = 15 };
constexpr int kGeomRow = 8;          // floats per table row
constexpr int kGeomMaxRadius = 3;    // ceil(2 sqrt(2)): zoom 2 at 45 degrees

GEOM_HD bool geom_finite(float v) { return fabsf(v) <= 3.4028234e38f; }          // false for a NaN and for +-inf

// a table integer: |value| <= 2^29, a non-finite float reads 0
GEOM_HD int geom_int(float v) { return geom_finite(v) ? (int)fminf(fmaxf(v, -536870912.f), 536870912.f) : 0; }

// the groups that run for the sample of `row`: the launch's, less (gated form) those of the row's skip mask in slot 7
GEOM_HD int geom_flags(const float* row, int flags, bool gated) {
  return gated ? (flags & ~(geom_int(row[GEOM_SKIP]) & GEOM_ALL)) : (flags & GEOM_ALL);
}

struct GeomRow { int fx, k; float zoom, c, s; };

// `F`: geom_flags() of the sample; a group that is off takes its identity value
GEOM_HD GeomRow geom_sanitise(const float* row, int F) {
  GeomRow r = {0, 0, 1.f, 1.f, 0.f};
  if (F & GEOM_FLIP) r.fx = geom_int(row[GEOM_FX]) & 1;
  if (F & GEOM_ROT90) r.k = geom_int(row[GEOM_K]) & 3;
  if (F & GEOM_SCALE) {
    const float z = row[GEOM_ZOOM];
    r.zoom = geom_finite(z) ? fminf(fmaxf(z, 0.5f), 2.f) : 1.f;
  }
  if (F & GEOM_ROTATE) {
    const float c = row[GEOM_COS], s = row[GEOM_SIN];
    if (geom_finite(c) && geom_finite(s)) { r.c = c; r.s = s; }
  }
  return r;
}

// source offset = M (output offset), M = R Q F / zoom; window centre offset = T (input offset), T = zoom (R Q F)^T.  Offsets are
// from the image centre (ci, cj), in (row, col) order.
struct GeomXf {
  float m00, m01, m10, m11;
  float t00, t01, t10, t11;
  float ci, cj;
  int radius, H, W;
};

GEOM_HD GeomXf geom_xf(const GeomRow& r, int H, int W) {
  const float ck = r.k == 0 ? 1.f : (r.k == 2 ? -1.f : 0.f), sk = r.k == 1 ? 1.f : (r.k == 3 ? -1.f : 0.f);
  const float sgn = r.fx ? -1.f : 1.f;
  // A = R Q F; one product of every pair is an exact zero, so the entries are +-cos, +-sin exactly
  const float a00 = r.c * ck - r.s * sk;
  const float a01 = (r.c * -sk - r.s * ck) * sgn;
  const float a10 = r.s * ck + r.c * sk;
  const float a11 = (r.s * -sk + r.c * ck) * sgn;
  GeomXf x;
  x.m00 = a00 / r.zoom; x.m01 = a01 / r.zoom; x.m10 = a10 / r.zoom; x.m11 = a11 / r.zoom;
  x.t00 = r.zoom * a00; x.t01 = r.zoom * a10; x.t10 = r.zoom * a01; x.t11 = r.zoom * a11;
  x.ci = (float)(H - 1) * 0.5f;
  x.cj = (float)(W - 1) * 0.5f;
  x.radius = (int)fminf(ceilf(r.zoom * (fabsf(r.c) + fabsf(r.s))), (float)kGeomMaxRadius);      // (inf reads 3)
  x.H = H; x.W = W;
  return x;
}

// a coordinate along an axis of `size` pixels, clamped where the answer no longer changes: at or below -1 and at or above size
// both neighbours are outside the image.  A NaN reads -2.
GEOM_HD float geom_clamp(float s, int size) { return fminf(fmaxf(s, -2.f), (float)size + 1.f); }

// s(q): where output pixel (qi, qj) reads the source
GEOM_HD void geom_src(const GeomXf& x, int qi, int qj, float* si, float* sj) {
  const float di = (float)qi - x.ci, dj = (float)qj - x.cj;
  *si = geom_clamp(x.m00 * di + x.m01 * dj + x.ci, x.H);
  *sj = geom_clamp(x.m10 * di + x.m11 * dj + x.cj, x.W);
}

// the four taps of a clamped position: rows i0, i0 + 1 with weights 1 - fi, fi; the same in j.  i0 in [-2, H + 1].
struct GeomTaps { int i0, j0; float fi, fj; };

GEOM_HD GeomTaps geom_taps(float si, float sj) {
  const float fl_i = floorf(si), fl_j = floorf(sj);
  GeomTaps t = {(int)fl_i, (int)fl_j, si - fl_i, sj - fl_j};
  return t;
}

GEOM_HD bool geom_inside(int i, int j, int H, int W) { return (unsigned)i < (unsigned)H && (unsigned)j < (unsigned)W; }

// round(q*): the centre of the window of output pixels that can read input pixel (pi, pj); in [-4, H + 3] x [-4, W + 3]: a
// centre farther out has no pixel of the image within the largest radius
GEOM_HD void geom_centre(const GeomXf& x, int pi, int pj, int* ri, int* rj) {
  const float di = (float)pi - x.ci, dj = (float)pj - x.cj;
  const float qi = x.t00 * di + x.t01 * dj + x.ci, qj = x.t10 * di + x.t11 * dj + x.cj;
  *ri = (int)floorf(fminf(fmaxf(qi, -4.f), (float)x.H + 3.f) + 0.5f);
  *rj = (int)floorf(fminf(fmaxf(qj, -4.f), (float)x.W + 3.f) + 0.5f);
}

GEOM_HD float geom_hat(float t) { return fmaxf(0.f, 1.f - fabsf(t)); }

}  // namespace srgan
