// The device records: state that a recorded train step (hipGraph) reads on every replay, so that the host can change a setting
// between steps without a new recording.  Every layout is declared HERE, once: srgan_amd/_lib.py mirrors it as a ctypes.Structure
// (tests/test_records_cpu.py holds the two together), the kernels that compute use these types.  The host writes a record through
// ONE kernel (record_write, pointwise.hip): an image of the struct travels by value in the launch packet and a mask names the
// 32-bit words to store.  An entry's mask is built from its fields, so it follows the layout.  Host code only besides the structs.
#pragma once
#include <cstddef>

namespace srgan {

constexpr int kRecordWords = 16;                      // 32-bit words of the image a write carries: the largest of the nine records (AdaState, LcState) have 14
struct RecordImage { unsigned int w[kRecordWords]; };

// Bit i = word i of the record: a field of kSize bytes at kOffset yields kSize / 4 adjacent bits (two for a 64-bit field).
template <size_t kOffset, size_t kSize>
constexpr unsigned record_words() {
  static_assert(kOffset % 4 == 0 && kSize % 4 == 0 && kSize > 0 && kOffset + kSize <= 4 * kRecordWords,
                "a record field is made of whole 32-bit words inside the image");
  return (unsigned)(((1ull << (kSize / 4)) - 1) << (kOffset / 4));
}
#define SRGAN_WORDS(S, f) (srgan::record_words<offsetof(S, f), sizeof(S::f)>())
template <class S>
constexpr unsigned record_all_words() { return record_words<0, sizeof(S)>(); }     // pads included: every *_state_init

// ---- each record, and the words its set entries store -----------------------------------------------------------------------------
// The step counter lives on the device so that a captured train step advances it on every replay (adam_tick_kernel, which derives
// step_size and inv_sqrt_bc2); the host mirrors the count for checkpoints only.
struct AdamState { int step; float lr, beta1, beta2, eps, step_size, inv_sqrt_bc2; int pad; };
static_assert(sizeof(AdamState) == 32, "AdamState layout");
constexpr unsigned kAdamSetLr = SRGAN_WORDS(AdamState, lr);

// norm / scale / skip are those of the last step (grad_guard_finalize_kernel), the counters are cumulative
struct GuardState { float max_norm, norm, scale; int skip, steps, skipped, clipped, pad; };
static_assert(sizeof(GuardState) == 32, "GuardState layout");
constexpr unsigned kGuardSetMaxNorm = SRGAN_WORDS(GuardState, max_norm);
constexpr unsigned kGuardSetCounters = SRGAN_WORDS(GuardState, steps) | SRGAN_WORDS(GuardState, skipped) | SRGAN_WORDS(GuardState, clipped);

// n = updates done, c = 1 - d_n of the update in flight (ema_tick_kernel)
struct EmaState { int n; int ramp; float decay; float c; };
static_assert(sizeof(EmaState) == 16, "EmaState layout");
constexpr unsigned kEmaSetDecay = SRGAN_WORDS(EmaState, decay);

// p, seen, the three counts, adjustments and last_r are moved by ada_observe_kernel; the rest is written by the host between steps
struct AdaState { float p, target, step, p_max; int interval, seen; long long n_pos, n_neg, n_total; int adjustments; float last_r; };
static_assert(sizeof(AdaState) == 56, "AdaState layout");
constexpr unsigned kAdaSetP = SRGAN_WORDS(AdaState, p);                             // joins kAdaSet iff set_p
constexpr unsigned kAdaSet = SRGAN_WORDS(AdaState, target) | SRGAN_WORDS(AdaState, step) | SRGAN_WORDS(AdaState, p_max) |
                             SRGAN_WORDS(AdaState, interval);
constexpr unsigned kAdaSetCounters = SRGAN_WORDS(AdaState, seen) | SRGAN_WORDS(AdaState, n_pos) | SRGAN_WORDS(AdaState, n_neg) |
                                     SRGAN_WORDS(AdaState, n_total) | SRGAN_WORDS(AdaState, adjustments) | SRGAN_WORDS(AdaState, last_r);

// gamma, every and n are written by the host between steps, c = gamma * every / n with them; penalty, mean_sq_norm are those of
// the last finalize, updates counts them.
struct R1State { float gamma; int every_scale; float c; float penalty; float mean_sq_norm; int updates; int n; int pad; };
static_assert(sizeof(R1State) == 32, "R1State layout");
constexpr unsigned kR1Set = SRGAN_WORDS(R1State, gamma) | SRGAN_WORDS(R1State, every_scale) | SRGAN_WORDS(R1State, c) |
                            SRGAN_WORDS(R1State, n);
constexpr unsigned kR1SetUpdates = SRGAN_WORDS(R1State, updates);

// The weights and every are written by the host between steps; cr_real, cr_fake are the unweighted terms of the last
// srgan_d_losses_cr, updates counts them.
struct CrState { float lambda_real; float lambda_fake; int every; float cr_real; float cr_fake; int updates; int pad[2]; };
static_assert(sizeof(CrState) == 32, "CrState layout");
constexpr unsigned kCrSet = SRGAN_WORDS(CrState, lambda_real) | SRGAN_WORDS(CrState, lambda_fake) | SRGAN_WORDS(CrState, every);
constexpr unsigned kCrSetUpdates = SRGAN_WORDS(CrState, updates);

// weight, eps, tau are written by the host between steps; the rest by ms_finish_kernel.  A restore leaves `weighted` to it.
struct MsState { float weight; float eps; float tau; float ms; float weighted; float d_image; float d_latent; int updates; };
static_assert(sizeof(MsState) == 32, "MsState layout");
constexpr unsigned kMsSet = SRGAN_WORDS(MsState, weight) | SRGAN_WORDS(MsState, eps) | SRGAN_WORDS(MsState, tau);
constexpr unsigned kMsRestore = SRGAN_WORDS(MsState, updates) | SRGAN_WORDS(MsState, ms) | SRGAN_WORDS(MsState, d_image) |
                                SRGAN_WORDS(MsState, d_latent);

// weight, decay, start are written by the host between steps; updates counts the anchor updates, a_real / a_fake are the anchors
// per scale (exponential moving averages of D's mean prediction), penalty the unweighted term and applied (0 / 1) whether its
// gradient was added, both of the last srgan_lecam.  A restore writes the counter and the anchors.
struct LcState { float weight; float decay; int start; int updates; float a_real[4]; float a_fake[4]; float penalty; int applied; };
static_assert(sizeof(LcState) == 56, "LcState layout");
constexpr unsigned kLcSet = SRGAN_WORDS(LcState, weight) | SRGAN_WORDS(LcState, decay) | SRGAN_WORDS(LcState, start);
constexpr unsigned kLcRestore = SRGAN_WORDS(LcState, updates) | SRGAN_WORDS(LcState, a_real) | SRGAN_WORDS(LcState, a_fake);

// weight, c1 = (k1 L)^2, c2 = (k2 L)^2 are written by the host between steps; term = 1 - mean SSIM and weighted = weight * term are
// those of the last ssim_finish_kernel, updates counts them.  A restore writes the counter and the two last values.
struct SsState { float weight; float c1; float c2; float term; float weighted; int updates; int pad[2]; };
static_assert(sizeof(SsState) == 32, "SsState layout");
constexpr unsigned kSsSet = SRGAN_WORDS(SsState, weight) | SRGAN_WORDS(SsState, c1) | SRGAN_WORDS(SsState, c2);
constexpr unsigned kSsRestore = SRGAN_WORDS(SsState, updates) | SRGAN_WORDS(SsState, term) | SRGAN_WORDS(SsState, weighted);

}  // namespace srgan
