// Stand-alone host program over csrc/records.h (tests/test_lecam_refs_cpu.py builds and runs it): the LeCam record's layout and the
// word masks of its write entries against literal values, and the write rule of record_write_kernel ("lane i stores word i iff
// bit i") replayed on the host for the two partial writes.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include "records.h"

using namespace srgan;

// word:   0       1      2      3        4 .. 7   8 .. 11  12       13
// Lc      weight  decay  start  updates  a_real   a_fake   penalty  applied
static_assert(sizeof(LcState) == 56 && sizeof(LcState) <= sizeof(RecordImage), "the record fits the image of a write");
static_assert(offsetof(LcState, weight) == 0 && offsetof(LcState, decay) == 4 && offsetof(LcState, start) == 8 &&
              offsetof(LcState, updates) == 12 && offsetof(LcState, a_real) == 16 && offsetof(LcState, a_fake) == 32 &&
              offsetof(LcState, penalty) == 48 && offsetof(LcState, applied) == 52, "LcState offsets");
static_assert(record_all_words<LcState>() == 0x3fffu && kLcSet == 0x0007u && kLcRestore == 0x0ff8u, "LcState masks");
static_assert(SRGAN_WORDS(LcState, a_real) == 0x00f0u && SRGAN_WORDS(LcState, a_fake) == 0x0f00u, "an array of four: four bits");
static_assert((kLcSet & kLcRestore) == 0 && ((kLcSet | kLcRestore) & (SRGAN_WORDS(LcState, penalty) | SRGAN_WORDS(LcState, applied))) == 0,
              "set and restore are disjoint and leave the last call's outputs alone");

static void write_like_the_kernel(LcState* rec, const LcState& image, unsigned mask) {
  RecordImage img = {};
  std::memcpy(img.w, &image, sizeof(LcState));
  unsigned int words[kRecordWords] = {};
  std::memcpy(words, rec, sizeof(LcState));
  for (int i = 0; i < kRecordWords; ++i)
    if ((mask >> i) & 1u) words[i] = img.w[i];
  std::memcpy(rec, words, sizeof(LcState));
}

int main() {
  int bad = 0;
  LcState rec;
  std::memset(&rec, 0xA5, sizeof rec);
  const LcState before = rec;
  LcState img = {};
  img.weight = 0.3f; img.decay = 0.99f; img.start = 7;
  write_like_the_kernel(&rec, img, kLcSet);
  bad += !(rec.weight == 0.3f && rec.decay == 0.99f && rec.start == 7);
  bad += std::memcmp(&rec.updates, &before.updates, sizeof(LcState) - offsetof(LcState, updates)) != 0;      // the rest keeps the sentinel
  LcState img2 = {};
  img2.updates = 11;
  for (int i = 0; i < 4; ++i) { img2.a_real[i] = 1.f + i; img2.a_fake[i] = -1.f - i; }
  write_like_the_kernel(&rec, img2, kLcRestore);
  bad += !(rec.updates == 11 && rec.weight == 0.3f && rec.decay == 0.99f && rec.start == 7);
  for (int i = 0; i < 4; ++i) bad += !(rec.a_real[i] == 1.f + i && rec.a_fake[i] == -1.f - i);
  bad += std::memcmp(&rec.penalty, &before.penalty, 8) != 0;                                                  // penalty, applied
  std::printf("lecam record %s\n", bad ? "BAD" : "ok");
  return bad ? 1 : 0;
}
