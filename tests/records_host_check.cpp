// Stand-alone host program over csrc/records.h (tests/test_records_cpu.py builds and runs it; it is also the sanitizer target:
// -fsanitize=address,undefined).  The word mask of every record entry against literal values -- the one place that fails when a
// layout or a mask moves -- and the write rule of record_write_kernel ("lane i stores word i iff bit i") replayed on the host.
#include <cstdio>
#include <cstring>
#include "records.h"

using namespace srgan;

// word:   0         1       2      3        4          5          6         7
// Adam    step      lr      beta1  beta2    eps        step_size  inv_sqrt  pad
// Guard   max_norm  norm    scale  skip     steps      skipped    clipped   pad
// Ema     n         ramp    decay  c
// Ada     p         target  step   p_max    interval   seen       n_pos (6, 7)  n_neg (8, 9)  n_total (10, 11)  adjustments 12  last_r 13
// R1      gamma     every   c      penalty  mean_sq    updates    n         pad
// Cr      l_real    l_fake  every  cr_real  cr_fake    updates    pad (6, 7)
// Ms      weight    eps     tau    ms       weighted   d_image    d_latent  updates
static_assert(record_all_words<AdamState>() == 0xffu && kAdamSetLr == 0x02u, "AdamState masks");
static_assert(record_all_words<GuardState>() == 0xffu && kGuardSetMaxNorm == 0x01u && kGuardSetCounters == 0x70u, "GuardState masks");
static_assert(record_all_words<EmaState>() == 0x0fu && kEmaSetDecay == 0x04u, "EmaState masks");
static_assert(record_all_words<AdaState>() == 0x3fffu && kAdaSet == 0x1eu && kAdaSetP == 0x01u && kAdaSetCounters == 0x3fe0u,
              "AdaState masks");
static_assert(record_all_words<R1State>() == 0xffu && kR1Set == 0x47u && kR1SetUpdates == 0x20u, "R1State masks");
static_assert(record_all_words<CrState>() == 0xffu && kCrSet == 0x07u && kCrSetUpdates == 0x20u, "CrState masks");
static_assert(record_all_words<MsState>() == 0xffu && kMsSet == 0x07u && kMsRestore == 0xe8u, "MsState masks (restore: not weighted)");
static_assert(SRGAN_WORDS(AdaState, n_total) == 0xc00u && SRGAN_WORDS(CrState, pad) == 0xc0u, "a 64-bit field and a pad pair: two bits");
static_assert(sizeof(RecordImage) == 64 && sizeof(AdaState) <= sizeof(RecordImage), "the image holds the largest record");

// what record_write + record_write_kernel do to a record of sizeof(S) bytes
template <class S>
static void write_like_the_kernel(S* rec, const S& image, unsigned mask) {
  RecordImage img = {};
  std::memcpy(img.w, &image, sizeof(S));
  unsigned int words[kRecordWords];
  std::memcpy(words, rec, sizeof(S));
  for (int i = 0; i < kRecordWords; ++i)
    if ((mask >> i) & 1u) words[i] = img.w[i];
  std::memcpy(rec, words, sizeof(S));
}

int main() {
  int bad = 0;
  AdaState rec;
  std::memset(&rec, 0xA5, sizeof rec);
  const AdaState before = rec;
  AdaState img = {};
  img.seen = 3; img.n_pos = (1LL << 32) + 1; img.n_neg = 3; img.n_total = (1LL << 33) + 5; img.adjustments = 7; img.last_r = 0.25f;
  write_like_the_kernel(&rec, img, kAdaSetCounters);
  bad += !(rec.seen == 3 && rec.n_pos == (1LL << 32) + 1 && rec.n_neg == 3 && rec.n_total == (1LL << 33) + 5 && rec.adjustments == 7 &&
           rec.last_r == 0.25f);
  bad += std::memcmp(&rec, &before, offsetof(AdaState, seen)) != 0;           // p, the settings and interval keep the sentinel
  MsState ms;
  std::memset(&ms, 0xA5, sizeof ms);
  const MsState ms_before = ms;
  MsState ms_img = {};
  ms_img.updates = 9; ms_img.ms = 1.5f; ms_img.d_image = 2.5f; ms_img.d_latent = 3.5f;
  write_like_the_kernel(&ms, ms_img, kMsRestore);
  bad += !(ms.updates == 9 && ms.ms == 1.5f && ms.d_image == 2.5f && ms.d_latent == 3.5f);
  bad += std::memcmp(&ms.weighted, &ms_before.weighted, 4) != 0 || std::memcmp(&ms, &ms_before, 12) != 0;
  std::printf("records %s\n", bad ? "BAD" : "ok");
  return bad ? 1 : 0;
}
