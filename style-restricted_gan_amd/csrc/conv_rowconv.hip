// The 3-channel 7x7 heads as a 7x1 row convolution on the implicit GEMM plus a shift-add pass.
#include <algorithm>
#include "conv.h"

namespace srgan {

// ---- 3-channel 7x7 heads (the generator's RGB output layer, model.py:232, and the input gradient of its 7x7 RGB input
// layer, model.py:212) on the matrix pipe.  With Cout = 3 a 32-wide MFMA tile would be 90 % padding, so the layer is split:
//   P[b][y][x'][(co, kx)] = sum_{ky, c} x[b][y + ky - pad][x'][c] * w[co][c][ky][kx]     -- a 7x1 conv with 21 (-> 32) outputs
//   y[b][y][x][co]        = bias[co] + sum_kx P[b][y][x + kx - pad][(co, kx)]             -- a shift-add over 7 columns
// The first is the ordinary implicit GEMM (N tile 32, 66 % useful), the second a memory-bound pass over P (21 floats per pixel,
// kept behind the packed weights).  1.3x faster than the VALU kernel of conv_narrow.hip on the 128x128 maps (230 vs 305 us at
// batch 32; the N = 32 tile runs at 74 TFLOP/s executed -- a 256x32 tile with 64x32 wave tiles was tried and was slower).
bool rowconv_applicable(const srgan_conv_desc* d) {
  static const bool off = SRGAN_AB_SET("SRGAN_NO_ROWCONV");
  return !off && d->O == 3 && d->kh == 7 && d->kw == 7 && d->stride == 1 && d->pad_mode == SRGAN_PAD_ZERO && (d->I % BK) == 0 &&
         d->Wo >= 64 && d->Ho >= 8 && (long long)d->N * d->Ho * d->Wi * 21 < (1LL << 30);
}
constexpr int RC_N = 21, RC_NPAD = 32;
static size_t rowconv_weight_elems(const srgan_conv_desc* d) { return (size_t)RC_NPAD * d->kh * d->I; }
// (round 3: where conv_rgbout.hip's direct 4x4x1-MFMA kernel applies it takes the layer over -- same dispatch slot, own packed
// filter, no intermediate)
size_t rowconv_packed_elems(const srgan_conv_desc* d) {
  if (rgbout_applicable(d)) return rgbout_packed_elems(d);
  return round_up((long long)rowconv_weight_elems(d), 64) + (size_t)d->N * d->Ho * d->Wi * RC_N;
}

// wp[n = co*7 + kx][k = ky*I + c] = w[co][c][ky][kx], rows 21..31 zero
__global__ void rowconv_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, long long sO, long long sI, long long sH,
                                    long long sW, int I, int kh, int kw) {
  const int K = kh * I, total = RC_NPAD * K;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int k = idx % K, n = idx / K;
    const int ky = k / I, c = k - ky * I;
    const int co = n / kw, kx = n - co * kw;
    wp[idx] = n < RC_N ? w[co * sO + c * sI + ky * sH + kx * sW] : 0.f;
  }
}

// y[pix][co] = bias[co] + sum_kx P[row, x + kx - pad][co*7 + kx]
__global__ void rowconv_shift_add_kernel(const float* __restrict__ P, const float* __restrict__ bias, float* __restrict__ y,
                                         long long rows, int Wi, int Wo, int pad) {
  const long long total = rows * Wo;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(idx % Wo);
    const long long row = idx / Wo;
    const float* pr = P + row * Wi * RC_N;
    float a0 = bias ? bias[0] : 0.f, a1 = bias ? bias[1] : 0.f, a2 = bias ? bias[2] : 0.f;
#pragma unroll
    for (int kx = 0; kx < 7; ++kx) {
      const int xs = x + kx - pad;
      if ((unsigned)xs < (unsigned)Wi) {
        const float* q = pr + (size_t)xs * RC_N + kx;
        a0 += q[0];
        a1 += q[7];
        a2 += q[14];
      }
    }
    float* o = y + idx * 3;
    o[0] = a0; o[1] = a1; o[2] = a2;
  }
}

int rowconv_pack(const srgan_conv_desc* d, const float* w, float* dst, hipStream_t st) {
  if (rgbout_applicable(d)) return rgbout_pack(d, w, dst, st);
  const int total = RC_NPAD * d->kh * d->I;
  hipLaunchKernelGGL(rowconv_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, st, w, dst, d->sO, d->sI, d->sH, d->sW, d->I,
                     d->kh, d->kw);
  return check_launch("rowconv_pack_kernel");
}

// `packed` = [32 x 7*I weights | P scratch]
int rowconv_run(const srgan_conv_desc* d, const float* x, const float* packed, const float* bias, float* y, hipStream_t st) {
  if (rgbout_applicable(d)) return rgbout_run(d, x, packed, bias, y, st);
  float* P = const_cast<float*>(packed) + round_up((long long)rowconv_weight_elems(d), 64);
  IgemmParams p{};
  p.src = x; p.wp = packed; p.bias = nullptr; p.dst = P;
  p.NB = d->N; p.Hs = d->Hi; p.Ws = d->Wi; p.Cs = d->I;
  p.Hg = d->Ho; p.Wg = d->Wi; p.Hd = d->Ho; p.Wd = d->Wi; p.Cd = RC_N;
  p.mode = 0; p.stride = 1; p.pad = d->pad; p.xpad_off = d->pad;      // rows padded, columns not
  p.Ty = d->kh; p.Tx = 1;
  p.K = d->kh * d->I; p.Kpad = p.K; p.Npad = RC_NPAD;
  p.M = d->N * d->Ho * d->Wi;
  p.reflect = 0; p.act = SRGAN_ACT_NONE; p.slope = 0.f;
  if (int e = run_igemm(p, 1, st, conv_flops(d))) return e;
  const long long rows = (long long)d->N * d->Ho, total = rows * d->Wo;
  hipLaunchKernelGGL(rowconv_shift_add_kernel, dim3((unsigned)std::min<long long>(ceil_div(total, 256), 16384)), dim3(256), 0, st,
                     (const float*)P, bias, y, rows, d->Wi, d->Wo, d->pad);
  return check_launch("rowconv_shift_add_kernel");
}

}  // namespace srgan
