// Shared helpers for the gfx950 kernels of libsrgan_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include "srgan_hip.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

namespace srgan {

void set_error(const char* fmt, ...);

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

#define SRGAN_REQUIRE(cond, ...)            \
  do {                                      \
    if (!(cond)) {                          \
      srgan::set_error(__VA_ARGS__);        \
      return -1;                            \
    }                                       \
  } while (0)

// Timing ablations (wrong results) and phase stamps are compile-time variants of the kernels: never in the product library.
#if !defined(SRGAN_EXPERIMENTS) && (defined(WINO_EXP) || defined(WINO42_EXP) || defined(RGBOUT_EXP) || defined(W43_DIAG) || defined(H16R_EXP))
#error "WINO_EXP / WINO42_EXP / RGBOUT_EXP / W43_DIAG / H16R_EXP are experiment builds: make exp EXPFLAGS=-DWINO_EXP=n (writes scratch/libsrgan_exp.so)"
#endif

// A/B switches of the measurement scripts under scratch/: only `make exp` (-DSRGAN_EXPERIMENTS, which writes
// scratch/libsrgan_exp.so, loaded through SRGAN_HIP_LIB) reads them from the environment.  In the product library every switch is
// a compile-time constant and its name is not in the binary (tests/test_abi_cpu.py checks the strings).
#ifdef SRGAN_EXPERIMENTS
#include <cstdlib>
#define SRGAN_AB_SET(name) (std::getenv(name) != nullptr)
#define SRGAN_AB_INT(name, dflt) (std::getenv(name) ? std::atoll(std::getenv(name)) : (long long)(dflt))
#else
#define SRGAN_AB_SET(name) false
#define SRGAN_AB_INT(name, dflt) ((long long)(dflt))
#endif

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// pointwise.hip: the one write path of the device records (records.h).  `image`: a host struct of `bytes` bytes, carried by value in
// the launch packet (nothing has to outlive the call); bit i of `mask` = store its 32-bit word i.  Returns check_launch(name).
int record_write(void* rec, const void* image, size_t bytes, unsigned mask, hipStream_t st, const char* name);

inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }
inline long long round_up(long long a, long long b) { return ceil_div(a, b) * b; }

// 64-lane wavefront reductions (gfx950 wave = 64).
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Block-wide sum for blockDim.x <= 1024 (multiple of 64). `red` must hold 16 floats.
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < nw; ++i) t += red[i];
  return t;
}

// The activation as one select: `act` is uniform, and written as `if (act == ...)` the compiler keeps a scalar branch per
// ELEMENT of an unrolled epilogue (~30 instructions and two taken branches around each 16-byte store: the row pass + stores of
// the F(4x4,2x2) kernel's epilogue took 7000 cycles, round 5).  Negative-side slope: 1 (none), 0 (ReLU), slope (LeakyReLU); the
// `+ 0.f` keeps ReLU's zero positive.  Same values as the branch form for every FINITE input and for NaN (a NaN stays a NaN, as
// in torch.relu); the one difference: ReLU of -inf is fma(-inf, 0, 0) = NaN here where the branch form and
// torch.relu give 0 -- an overflowed activation now poisons what follows instead of being clamped.  Accepted: an infinite
// pre-activation means the step has already diverged, and bench.py / the trainer tests check the losses for finiteness.
__device__ __forceinline__ float act_neg_slope(int act, float slope) {
  return act == SRGAN_ACT_LRELU ? slope : (act == SRGAN_ACT_RELU ? 0.f : 1.f);
}
__device__ __forceinline__ float apply_act(float v, int act, float slope) {
  return v > 0.f ? v : __builtin_fmaf(v, act_neg_slope(act, slope), 0.f);
}
// derivative from the (pre- or post-activation) sign; slope > 0 keeps signs equal
__device__ __forceinline__ float act_grad(float v, int act, float slope) {
  return v > 0.f ? 1.f : act_neg_slope(act, slope);
}

}  // namespace srgan
