// Stand-alone host program over csrc/records.h and csrc/ssim_math.h (tests/test_ssim_refs_cpu.py builds it with the address and
// undefined-behaviour sanitizers and runs it): the SSIM record's layout and the word masks of its write entries against literal
// values, the write rule of record_write_kernel replayed on the host for the two partial writes, the tap table, and -- in double --
// the central moments from shifted moments against the raw definition and the quotient's partial derivatives against central
// differences.  Prints the taps of every window as hexadecimal floats ("taps <window> ..."): the test compares them with numpy's.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include "records.h"
#include "ssim_math.h"

using namespace srgan;

// word:   0       1   2   3     4         5        6 .. 7
// Ss      weight  c1  c2  term  weighted  updates  pad
static_assert(sizeof(SsState) == 32 && sizeof(SsState) <= sizeof(RecordImage), "the record fits the image of a write");
static_assert(offsetof(SsState, weight) == 0 && offsetof(SsState, c1) == 4 && offsetof(SsState, c2) == 8 && offsetof(SsState, term) == 12 &&
              offsetof(SsState, weighted) == 16 && offsetof(SsState, updates) == 20 && offsetof(SsState, pad) == 24, "SsState offsets");
static_assert(record_all_words<SsState>() == 0xffu && kSsSet == 0x07u && kSsRestore == 0x38u, "SsState masks");
static_assert((kSsSet & kSsRestore) == 0 && ((kSsSet | kSsRestore) & SRGAN_WORDS(SsState, pad)) == 0, "set and restore are disjoint");

static void write_like_the_kernel(SsState* rec, const SsState& image, unsigned mask) {
  RecordImage img = {};
  std::memcpy(img.w, &image, sizeof(SsState));
  unsigned int words[kRecordWords] = {};
  std::memcpy(words, rec, sizeof(SsState));
  for (int i = 0; i < kRecordWords; ++i)
    if ((mask >> i) & 1u) words[i] = img.w[i];
  std::memcpy(rec, words, sizeof(SsState));
}

static int check_record() {
  int bad = 0;
  SsState rec;
  std::memset(&rec, 0xA5, sizeof rec);
  const SsState before = rec;
  SsState img = {};
  img.weight = 0.5f; img.c1 = 4e-4f; img.c2 = 3.6e-3f;
  write_like_the_kernel(&rec, img, kSsSet);
  bad += !(rec.weight == 0.5f && rec.c1 == 4e-4f && rec.c2 == 3.6e-3f);
  bad += std::memcmp(&rec.term, &before.term, sizeof(SsState) - offsetof(SsState, term)) != 0;       // the rest keeps the sentinel
  SsState img2 = {};
  img2.updates = 11; img2.term = 0.25f; img2.weighted = 0.125f;
  write_like_the_kernel(&rec, img2, kSsRestore);
  bad += !(rec.updates == 11 && rec.term == 0.25f && rec.weighted == 0.125f && rec.weight == 0.5f && rec.c1 == 4e-4f && rec.c2 == 3.6e-3f);
  bad += std::memcmp(rec.pad, before.pad, sizeof rec.pad) != 0;
  return bad;
}

static double lcg(unsigned long long* s) {                    // uniform in [-1, 1)
  *s = *s * 6364136223846793005ULL + 1442695040888963407ULL;
  return (double)(*s >> 11) / 4503599627370496.0 - 1.0;
}

// one window of random values: the definition's raw moments with the product taps against ss_central of the shifted moments
static int check_central(int window, double centre, double spread, unsigned long long seed) {
  float taps[kSsMaxWindow];
  ss_gaussian_taps(window, 1.5, taps);
  const SsTaps t = ss_taps(taps, window);
  double tot = 0.0;
  for (int k = 0; k < window; ++k) tot += (double)taps[k];
  const double excess = tot * tot - 1.0;
  double x[kSsMaxWindow * kSsMaxWindow], y[kSsMaxWindow * kSsMaxWindow];
  for (int i = 0; i < window * window; ++i) { x[i] = centre + spread * lcg(&seed); y[i] = centre + spread * lcg(&seed); }
  const double p = x[0], q = y[0];
  long double ex = 0, ey = 0, exx = 0, eyy = 0, exy = 0;
  double m1 = 0, m2 = 0, m3 = 0, m4 = 0, m5 = 0;
  for (int i = 0; i < window; ++i)
    for (int j = 0; j < window; ++j) {
      const double w = (double)t.w[i] * (double)t.w[j], a = x[i * window + j], b = y[i * window + j];
      ex += w * a; ey += w * b; exx += w * a * a; eyy += w * b * b; exy += w * a * b;
      m1 += w * (a - p); m2 += w * (b - q); m3 += w * (a - p) * (a - p); m4 += w * (b - q) * (b - q); m5 += w * (a - p) * (b - q);
    }
  const SsCentral<double> c = ss_central<double>(m1, m2, m3, m4, m5, p, q, excess);
  const double tol = 1e-13;
  int bad = 0;
  bad += std::fabs((double)(ex - p) - c.dx) > tol;
  bad += std::fabs((double)(ey - q) - c.dy) > tol;
  bad += std::fabs((double)(exx - ex * ex) - c.sx) > tol;
  bad += std::fabs((double)(eyy - ey * ey) - c.sy) > tol;
  bad += std::fabs((double)(exy - ex * ey) - c.sxy) > tol;
  bad += std::fabs((double)t.excess - excess) > 1e-15 || t.n != window;
  return bad;
}

static int check_point(double a, double b, double sx, double sy, double sxy) {
  const double c1 = 4e-4, c2 = 3.6e-3, h = 1e-6;
  const SsPoint<double> p = ss_point<double>(a, b, sx, sy, sxy, c1, c2);
  const double direct = (2 * a * b + c1) * (2 * sxy + c2) / ((a * a + b * b + c1) * (sx + sy + c2));
  auto v = [&](double da, double db, double dsx, double dsy, double dsxy) {
    return ss_point<double>(a + da, b + db, sx + dsx, sy + dsy, sxy + dsxy, c1, c2).value;
  };
  const double fa = (v(h, 0, 0, 0, 0) - v(-h, 0, 0, 0, 0)) / (2 * h), fb = (v(0, h, 0, 0, 0) - v(0, -h, 0, 0, 0)) / (2 * h);
  const double fsx = (v(0, 0, h, 0, 0) - v(0, 0, -h, 0, 0)) / (2 * h), fsy = (v(0, 0, 0, h, 0) - v(0, 0, 0, -h, 0)) / (2 * h);
  const double fsxy = (v(0, 0, 0, 0, h) - v(0, 0, 0, 0, -h)) / (2 * h);
  auto off = [](double got, double want) { return std::fabs(got - want) > 1e-6 * (1.0 + std::fabs(want)); };
  return (std::fabs(p.value - direct) > 1e-14) + off(p.g_mux, fa) + off(p.g_muy, fb) + off(p.g_s, fsx) + off(p.g_s, fsy) + off(p.g_sxy, fsxy);
}

int main() {
  int bad = check_record();
  for (int window = kSsMinWindow - 1; window <= kSsMaxWindow + 1; ++window) {
    if (!ss_window_ok(window)) {
      bad += window % 2 == 1 && window >= 3 && window <= 11;
      continue;
    }
    float taps[kSsMaxWindow];
    ss_gaussian_taps(window, 1.5, taps);
    std::printf("taps %d", window);
    double s = 0.0;
    for (int k = 0; k < window; ++k) {
      std::printf(" %a", (double)taps[k]);
      s += (double)taps[k];
      bad += taps[k] != taps[window - 1 - k];
    }
    std::printf("\n");
    bad += std::fabs(s - 1.0) > 1e-6;
    bad += check_central(window, 0.0, 1.0, 17 + window);
    bad += check_central(window, 0.95, 0.01, 29 + window);
    bad += check_central(window, -0.95, 0.001, 31 + window);
  }
  bad += check_point(0.3, -0.2, 0.05, 0.04, 0.01);
  bad += check_point(0.95, 0.95, 1e-4, 1.2e-4, 0.9e-4);
  bad += check_point(-0.5, 0.7, 0.3, 0.2, -0.15);
  bad += check_point(0.0, 0.0, 0.0, 0.0, 0.0);
  std::printf("ssim host check %s\n", bad ? "BAD" : "ok");
  return bad ? 1 : 0;
}
