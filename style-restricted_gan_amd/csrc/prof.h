// Optional in-process launch timer (bench.py's roofline leg): while a session is open (srgan_prof_enable(1)) every bracketed
// launch sits between two HIP events on ITS stream; the durations are read back after the timed region (srgan_prof_collect /
// srgan_prof_slot, prof.cpp).  Off by default: a bracket is then one flag test -- no events, no allocation.
#pragma once
#include <hip/hip_runtime.h>

namespace srgan {

// The timed kernels: X(enumerator, name).  The position in this list is the kernel id of the srgan_prof_* entries, and the names
// are what bench.py and the tests select kernels by -- append, never reorder or respell.
#define SRGAN_PROF_KERNELS(X)                                                                                                  \
  X(IGEMM_128x128_GEN, "igemm_kernel<128,128,2,2,gen>") X(IGEMM_128x128_VEC, "igemm_kernel<128,128,2,2,vec>")                  \
  X(IGEMM_128x64_GEN, "igemm_kernel<128,64,2,2,gen>") X(IGEMM_128x64_VEC, "igemm_kernel<128,64,2,2,vec>")                      \
  X(IGEMM_128x32_GEN, "igemm_kernel<128,32,4,1,gen>") X(IGEMM_128x32_VEC, "igemm_kernel<128,32,4,1,vec>")                      \
  X(IGEMM_64x64_GEN, "igemm_kernel<64,64,2,2,gen>") X(IGEMM_64x64_VEC, "igemm_kernel<64,64,2,2,vec>")                          \
  X(WGRAD_GEN, "wgrad_kernel<gen>") X(WGRAD_VEC, "wgrad_kernel<vec>")                                                          \
  X(IGEMM_256x128_GEN, "igemm_kernel<256,128,4,2,gen>") X(IGEMM_256x128_VEC, "igemm_kernel<256,128,4,2,vec>")                  \
  X(IGEMM_256x64_GEN, "igemm_kernel<256,64,4,2,gen>") X(IGEMM_256x64_VEC, "igemm_kernel<256,64,4,2,vec>")                      \
  X(WINO, "wino_kernel") X(WINO_WGRAD, "wino_wgrad_kernel") X(WINO_S2, "wino_kernel<4x4s2>")                                   \
  X(WINO_S2_WGRAD, "wino_wgrad_kernel<4x4s2>")                                                                                 \
  X(WINO43, "wino43_kernel") X(WINO43_INPUT, "wino43_input_kernel") X(RGBIN_CONV, "rgbin_conv_kernel")                         \
  X(RGB_WGRAD, "rgb_wgrad_kernel") X(WINO43_WGRAD, "wino43_wgrad_kernel") X(WINO43_DY, "wino43_dy_kernel")                     \
  X(HALO16, "halo16_kernel") X(HALO16_WGRAD, "halo16_wgrad_kernel") X(HALO16S2_WGRAD, "halo16s2_wgrad_kernel")                 \
  X(HALO16T, "halo16t_kernel") X(RGBOUT_CONV, "rgbout_conv_kernel") X(HALO16S, "halo16s_kernel")                               \
  /* HBM-bound passes (norm.hip): the "flops" slot of their brackets carries ALGORITHMIC BYTES (tensor bytes each pass must */ \
  /* move) */                                                                                                                  \
  X(IN_STATS_PARTIAL, "in_stats_partial") X(IN_APPLY, "in_apply") X(IN_BWD_PARTIAL, "in_bwd_partial")                          \
  X(IN_BWD_APPLY, "in_bwd_apply") X(IN_FWD_SLAB, "in_fwd_slab") X(IN_BWD_SLAB, "in_bwd_slab")                                  \
  X(IGEMM16, "igemm16_kernel") X(WINO42, "wino42_kernel")                                                                      \
  /* the fused norm + Winograd-transform kernels of the trunk (conv_wino43.hip), HBM-bound too: bytes in the "flops" slot */   \
  X(IN_FWD_SLAB_V, "in_fwd_slab_v") X(IN_BWD_SLAB_VZ, "in_bwd_slab_vz")                                                        \
  /* balanced consistency regularisation (consistency.hip): launch counts and per-launch times only, nothing in the "flops" */ \
  /* slot */                                                                                                                   \
  X(CR_PAIRS, "cr_pairs_kernel") X(D_LOSSES_CR, "d_losses_cr_kernel")                                                          \
  /* mode-seeking regularisation (diversity.hip): the bytes the pass must move in the "flops" slot of the two streaming */     \
  /* passes */                                                                                                                 \
  X(MS_ROWS, "ms_rows_kernel") X(MS_FINISH, "ms_finish_kernel") X(MS_GRAD, "ms_grad_kernel")

enum ProfKernel : int {
#define SRGAN_PROF_ENUM(id, name) PROF_##id,
  SRGAN_PROF_KERNELS(SRGAN_PROF_ENUM)
#undef SRGAN_PROF_ENUM
  kProfKernels      // their number
};

// the slot of igemm_kernel<BM, BN, .., VEC>: the pairing of tile and slot, next to the list that names them
constexpr ProfKernel prof_igemm_kernel(int BM, int BN, bool vec) {
  if (BM == 256 && BN == 64) return vec ? PROF_IGEMM_256x64_VEC : PROF_IGEMM_256x64_GEN;
  if (BM == 256) return vec ? PROF_IGEMM_256x128_VEC : PROF_IGEMM_256x128_GEN;
  if (BM == 128 && BN == 128) return vec ? PROF_IGEMM_128x128_VEC : PROF_IGEMM_128x128_GEN;
  if (BM == 128 && BN == 64) return vec ? PROF_IGEMM_128x64_VEC : PROF_IGEMM_128x64_GEN;
  if (BM == 128 && BN == 32) return vec ? PROF_IGEMM_128x32_VEC : PROF_IGEMM_128x32_GEN;
  return vec ? PROF_IGEMM_64x64_VEC : PROF_IGEMM_64x64_GEN;
}

// prof.cpp: the start event of a new slot on `st`; -1 when no session is open (or no event could be made).  The end event.
long prof_open(ProfKernel kid, double flops, hipStream_t st);
void prof_close(long slot, hipStream_t st);

// The bracket: open for as long as the object lives, so whatever way the launching function is left the end event is recorded.
// Refuse (set_error + return) BEFORE opening one, and end it with a block where further launches follow in the same function.
class ProfScope {
 public:
  ProfScope(ProfKernel kid, double flops, hipStream_t st) : st_(st), slot_(prof_open(kid, flops, st)) {}
  ~ProfScope() {
    if (slot_ >= 0) prof_close(slot_, st_);
  }
  ProfScope(const ProfScope&) = delete;
  ProfScope& operator=(const ProfScope&) = delete;

 private:
  hipStream_t st_;
  long slot_;
};

}  // namespace srgan
