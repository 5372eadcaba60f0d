// Stand-alone host program (tests/test_geom_refs_cpu.py builds and runs it): sweeps hostile table rows through the very functions
// the geometric-augmentation kernels run (csrc/geom_math.h) and walks the index arithmetic of both kernels the way
// csrc/augment_geom.hip does, over images from 1 x 1 to 256 x 256.  Asserts, for every row, flag set and visited pixel:
//   - the sanitised parameters are as specified (zoom in [0.5, 2], non-finite -> 1; fx in {0, 1}, k in {0..3}, non-finite -> 0; a
//     non-finite cos or sin -> the identity rotation);
//   - the radius is <= 3 and the window is at most 7 x 7;
//   - every float that becomes an int is finite and inside [-4, size + 3] at the conversion;
//   - every tap the kernels would dereference (the ones that pass the integer bounds test) lies inside the image, and its float
//     offset inside the sample.
// The integer bounds tests of the kernels are restated here, not shared, so the "tap inside" lines only confirm that test; what the
// sweep adds is the range of every float at its conversion to int (with -fsanitize=float-cast-overflow the conversions themselves)
// and the sanitised parameters.  Exit status 0 and "ok <count>" on success; the first violation is printed and the status is 1.
// No GPU, no library: compiled from the header alone (optionally with -fsanitize=address,undefined).
// A second mode, `probe`, prints what the header makes of one row (below).
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "geom_math.h"

using namespace srgan;

static long long g_checks = 0;

#define CHECK(cond, ...)                          \
  do {                                            \
    ++g_checks;                                   \
    if (!(cond)) {                                \
      std::printf("FAILED %s: ", #cond);          \
      std::printf(__VA_ARGS__);                   \
      std::printf("\n");                          \
      std::exit(1);                               \
    }                                             \
  } while (0)

static bool finite_f(float v) { return v == v && v != std::numeric_limits<float>::infinity() && v != -std::numeric_limits<float>::infinity(); }

// the conversions of geom_math.h, re-done here on the clamped floats to check the range BEFORE an int is made
static void check_convertible(float v, int size, const char* what) {
  CHECK(finite_f(v) && v >= -4.5f && v <= (float)size + 4.5f, "%s = %g for size %d", what, (double)v, size);
}

// one pixel, as an output pixel of the forward kernel and as an input pixel of the backward kernel
static void sweep_pixel(const GeomXf& g, int H, int W, int pi, int pj) {
  const size_t E = (size_t)H * W * 3;
  // forward: the four taps of output pixel (pi, pj)
  float si, sj;
  geom_src(g, pi, pj, &si, &sj);
  check_convertible(si, H, "s_i");
  check_convertible(sj, W, "s_j");
  CHECK(si >= -2.f && si <= (float)H + 1.f && sj >= -2.f && sj <= (float)W + 1.f, "s = (%g, %g) not clamped", (double)si, (double)sj);
  const GeomTaps t = geom_taps(si, sj);
  CHECK(t.i0 >= -2 && t.i0 <= H + 1 && t.j0 >= -2 && t.j0 <= W + 1, "i0 = %d, j0 = %d", t.i0, t.j0);
  CHECK(t.fi >= 0.f && t.fi <= 1.f && t.fj >= 0.f && t.fj <= 1.f, "fi = %g, fj = %g", (double)t.fi, (double)t.fj);
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) {
      const int i = t.i0 + a, j = t.j0 + b;
      if (!geom_inside(i, j, H, W)) continue;
      CHECK(i >= 0 && i < H && j >= 0 && j < W, "forward tap (%d, %d) in %d x %d", i, j, H, W);
      CHECK(((size_t)i * W + j) * 3 + 2 < E, "forward tap offset");
    }
  // backward: the window of input pixel (pi, pj)
  int ri, rj;
  geom_centre(g, pi, pj, &ri, &rj);
  CHECK(ri >= -4 && ri <= H + 4 && rj >= -4 && rj <= W + 4, "centre (%d, %d) in %d x %d", ri, rj, H, W);
  int visited = 0;
  for (int qi = ri - g.radius; qi <= ri + g.radius; ++qi)
    for (int qj = rj - g.radius; qj <= rj + g.radius; ++qj) {
      ++visited;
      if (!geom_inside(qi, qj, H, W)) continue;
      CHECK(qi >= 0 && qi < H && qj >= 0 && qj < W, "backward tap (%d, %d) in %d x %d", qi, qj, H, W);
      CHECK(((size_t)qi * W + qj) * 3 + 2 < E, "backward tap offset");
      float ti, tj;
      geom_src(g, qi, qj, &ti, &tj);
      const float wgt = geom_hat(ti - (float)pi) * geom_hat(tj - (float)pj);
      CHECK(wgt >= 0.f && wgt <= 1.f, "weight %g", (double)wgt);
    }
  CHECK(visited <= 49, "window of %d candidates", visited);
}


static void sweep_image(const float* row, int flags, bool gated, int H, int W) {
  const int F = geom_flags(row, flags, gated);
  CHECK(F >= 0 && F <= 15 && (F & ~flags) == 0, "F = %d from flags %d", F, flags);
  const GeomRow r = geom_sanitise(row, F);
  CHECK(r.fx == 0 || r.fx == 1, "fx = %d", r.fx);
  CHECK(r.k >= 0 && r.k <= 3, "k = %d", r.k);
  CHECK(r.zoom >= 0.5f && r.zoom <= 2.f, "zoom = %g", (double)r.zoom);
  CHECK(finite_f(r.c) && finite_f(r.s), "cos = %g, sin = %g", (double)r.c, (double)r.s);
  if (!(F & GEOM_FLIP)) CHECK(r.fx == 0, "flip off, fx = %d", r.fx);
  if (!(F & GEOM_ROT90)) CHECK(r.k == 0, "rot90 off, k = %d", r.k);
  if (!(F & GEOM_SCALE)) CHECK(r.zoom == 1.f, "scale off, zoom = %g", (double)r.zoom);
  if (!(F & GEOM_ROTATE)) CHECK(r.c == 1.f && r.s == 0.f, "rotate off, (%g, %g)", (double)r.c, (double)r.s);
  if (F & GEOM_SCALE) {
    const float z = row[GEOM_ZOOM];
    const float want = finite_f(z) ? (z < 0.5f ? 0.5f : (z > 2.f ? 2.f : z)) : 1.f;
    CHECK(r.zoom == want, "zoom %g reads %g, %g expected", (double)z, (double)r.zoom, (double)want);
  }
  if (F & GEOM_ROTATE) {
    const bool ok = finite_f(row[GEOM_COS]) && finite_f(row[GEOM_SIN]);
    CHECK(ok ? (r.c == row[GEOM_COS] && r.s == row[GEOM_SIN]) : (r.c == 1.f && r.s == 0.f), "(cos, sin) = (%g, %g) read (%g, %g)",
          (double)row[GEOM_COS], (double)row[GEOM_SIN], (double)r.c, (double)r.s);
  }
  if ((F & GEOM_FLIP) && !finite_f(row[GEOM_FX])) CHECK(r.fx == 0, "non-finite fx reads %d", r.fx);
  if ((F & GEOM_ROT90) && !finite_f(row[GEOM_K])) CHECK(r.k == 0, "non-finite k reads %d", r.k);
  if ((F & GEOM_ROT90) && row[GEOM_K] == -1.f) CHECK(r.k == 3, "k = -1 reads %d", r.k);
  if ((F & GEOM_ROT90) && row[GEOM_K] == 7.5f) CHECK(r.k == 3, "k = 7.5 reads %d", r.k);

  const GeomXf g = geom_xf(r, H, W);
  CHECK(g.radius >= 0 && g.radius <= kGeomMaxRadius, "radius = %d", g.radius);
  const long long P = (long long)H * W;
  const long long step = P > 4096 ? 37 : 1;                 // large images: every 37th pixel, and the last one
  for (long long lin = 0; lin < P; lin += step) sweep_pixel(g, H, W, (int)(lin / W), (int)(lin % W));
  sweep_pixel(g, H, W, H - 1, W - 1);
}

// `probe H W flags fx k zoom cos sin`: what geom_math.h makes of ONE row on an H x W image, for the tests to hold their Python
// restatement to -- the radius, the largest weight any output pixel OUTSIDE an input pixel's window gives that input pixel (the
// window is a superset of the support iff this is exactly 0), and s(q) of every output pixel.
static int probe(char** a) {
  const int H = std::atoi(a[0]), W = std::atoi(a[1]), flags = std::atoi(a[2]);
  float row[kGeomRow] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < 5; ++i) row[i] = std::strtof(a[3 + i], nullptr);
  const GeomXf g = geom_xf(geom_sanitise(row, geom_flags(row, flags, false)), H, W);
  float outside = 0.f, inside = 0.f;
  for (int pi = 0; pi < H; ++pi)
    for (int pj = 0; pj < W; ++pj) {
      int ri, rj;
      geom_centre(g, pi, pj, &ri, &rj);
      for (int qi = 0; qi < H; ++qi)
        for (int qj = 0; qj < W; ++qj) {
          float si, sj;
          geom_src(g, qi, qj, &si, &sj);
          const float wgt = geom_hat(si - (float)pi) * geom_hat(sj - (float)pj);
          const bool in = std::abs(qi - ri) <= g.radius && std::abs(qj - rj) <= g.radius;
          if (in) inside = wgt > inside ? wgt : inside;
          else outside = wgt > outside ? wgt : outside;
        }
    }
  std::printf("radius %d\noutside %.9g\ninside %.9g\n", g.radius, (double)outside, (double)inside);
  for (int qi = 0; qi < H; ++qi)
    for (int qj = 0; qj < W; ++qj) {
      float si, sj;
      geom_src(g, qi, qj, &si, &sj);
      const GeomTaps t = geom_taps(si, sj);
      std::printf("src %d %d %.9g %.9g %d %d %.9g %.9g\n", qi, qj, (double)si, (double)sj, t.i0, t.j0, (double)t.fi, (double)t.fj);
    }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 10 && std::string(argv[1]) == "probe") return probe(argv + 2);
  if (argc != 1) {
    std::printf("usage: %s [probe H W flags fx k zoom cos sin]\n", argv[0]);
    return 2;
  }
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float hostile[] = {nan, inf, -inf, 1e30f, -1e30f, 3.0e38f, -3.0e38f, 1e-6f, 1e6f, -1e6f, -1.f, 7.5f, 0.f, 1.f, 0.5f, 2.f, 9.f, -0.f};
  const int nh = (int)(sizeof(hostile) / sizeof(hostile[0]));
  std::vector<std::vector<float>> rows;
  // one slot hostile at a time on top of a plain row, every slot hostile at once, and the rotation pair hostile together
  for (int slot = 0; slot < kGeomRow; ++slot)
    for (int v = 0; v < nh; ++v) {
      std::vector<float> r = {1.f, 1.f, 1.25f, 0.8f, 0.6f, 0.f, 0.f, 0.f};
      r[slot] = hostile[v];
      rows.push_back(r);
    }
  for (int v = 0; v < nh; ++v) rows.push_back(std::vector<float>(kGeomRow, hostile[v]));
  const float pair[] = {nan, inf, -1e30f, 3.0e38f, 1e6f, -1e6f, 0.f, 1.f};
  for (float c : pair)
    for (float s : pair) rows.push_back({1.f, 3.f, 2.f, c, s, 0.f, 0.f, 0.f});
  for (int z = 0; z < nh; ++z) rows.push_back({0.f, 0.f, hostile[z], 1e6f, -1e6f, 0.f, 0.f, 0.f});
  const int sizes[][2] = {{1, 1}, {1, 2}, {2, 1}, {2, 2}, {3, 5}, {7, 7}, {8, 8}, {16, 12}, {31, 33}, {128, 128}, {1, 256}, {256, 1}, {256, 256}};
  for (const auto& r : rows)
    for (const auto& hw : sizes) {
      const bool big = hw[0] * hw[1] > 4096;
      for (int flags = big ? 15 : 0; flags <= 15; ++flags) {
        sweep_image(r.data(), flags, false, hw[0], hw[1]);
        if (flags == 15) sweep_image(r.data(), flags, true, hw[0], hw[1]);
      }
    }
  std::printf("ok %lld\n", g_checks);
  return 0;
}
