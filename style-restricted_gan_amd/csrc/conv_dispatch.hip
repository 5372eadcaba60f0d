// Which kernel family serves a forward or input-gradient convolution, and the C entries of both directions: descriptor
// validation, the workspace query, the per-family geometry, the reflect fold behind a reflect-padded input gradient, and the
// process-wide compute mode every one of those decisions reads.
#include <algorithm>
#include "conv.h"

namespace srgan {

// ---- compute mode: 0 = exact fp32 (default), 1 = bf16 MFMA operands with fp32 accumulation ----
static int g_compute_mode = 0;
bool compute_bf16() { return g_compute_mode == 1; }

// algorithmic FLOPs of one conv pass: 2 * (N*Ho*Wo) * O * (kh*kw*I)
double conv_flops(const srgan_conv_desc* d) {
  return 2.0 * d->N * d->Ho * d->Wo * (double)d->O * d->kh * d->kw * d->I;
}

int conv_validate(const srgan_conv_desc* d) {
  SRGAN_REQUIRE(d != nullptr, "conv desc is null");
  SRGAN_REQUIRE(d->N > 0 && d->Hi > 0 && d->Wi > 0 && d->I > 0 && d->O > 0 && d->kh > 0 && d->kw > 0,
                "conv desc: non-positive dimension");
  SRGAN_REQUIRE(d->stride >= 1 && d->pad >= 0, "conv desc: bad stride/pad");
  const int ho = (d->Hi + 2 * d->pad - d->kh) / d->stride + 1;
  const int wo = (d->Wi + 2 * d->pad - d->kw) / d->stride + 1;
  SRGAN_REQUIRE(ho == d->Ho && wo == d->Wo, "conv desc: Ho/Wo (%d,%d) do not match geometry (%d,%d)", d->Ho, d->Wo, ho, wo);
  SRGAN_REQUIRE(d->pad_mode == SRGAN_PAD_ZERO || d->pad_mode == SRGAN_PAD_REFLECT, "conv desc: bad pad_mode");
  if (d->pad_mode == SRGAN_PAD_REFLECT)
    SRGAN_REQUIRE(d->stride == 1 && d->pad < d->Hi && d->pad < d->Wi, "reflect padding needs stride 1 and pad < size");
  SRGAN_REQUIRE((long long)d->N * d->Hi * d->Wi * (long long)d->I < (1LL << 30) - (1LL << 24) &&
                (long long)d->N * d->Ho * d->Wo * (long long)d->O < (1LL << 30) - (1LL << 24),
                "tensor too large: the gather uses 32-bit byte offsets (< 4 GiB per activation tensor)");
  SRGAN_REQUIRE(d->kh * d->kw <= 64, "kernel window larger than 64 taps is not supported");
  return 0;
}

// ---- reflect-pad fold (dgrad of a reflect-padded conv) --------------------------------------
// dxp: [N][H+2P][W+2P][C] gradient w.r.t. the padded image; dx[n][y][x][c] sums every padded
// position that mirrors onto (y,x).  P = pad (1 in the reference).
template <bool OUT16 = false>
__global__ void reflect_fold_kernel(const float* dxp, float* dx, int N, int H, int W, int C, int P) {
  const long long total = (long long)N * H * W * C;
  const int Hp = H + 2 * P, Wp = W + 2 * P;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    long long r = idx / C;
    const int x = (int)(r % W); r /= W;
    const int y = (int)(r % H);
    const int n = (int)(r / H);
    // candidate padded rows: y+P (direct), P-y (top mirror, needs 1<=y<=P), 2H-2-y+P (bottom)
    int ys[3], xs[3], ny = 0, nx = 0;
    ys[ny++] = y + P;
    if (y >= 1 && y <= P) ys[ny++] = P - y;
    if (y <= H - 2 && y >= H - 1 - P) ys[ny++] = 2 * H - 2 - y + P;
    xs[nx++] = x + P;
    if (x >= 1 && x <= P) xs[nx++] = P - x;
    if (x <= W - 2 && x >= W - 1 - P) xs[nx++] = 2 * W - 2 - x + P;
    float v = 0.f;
    for (int i = 0; i < ny; ++i)
      for (int j = 0; j < nx; ++j) v += dxp[((size_t)(n * Hp + ys[i]) * Wp + xs[j]) * C + c];
    if constexpr (OUT16) reinterpret_cast<__bf16*>(dx)[idx] = (__bf16)v;
    else dx[idx] = v;
  }
}

// ---- forward: which kernel family serves this layer, and the packed-weight layout it wants ----
FwdPath fwd_path(const srgan_conv_desc* d, int act) {
  if (act == SRGAN_ACT_NONE) {
    if (dense_head_applicable(d)) return PATH_DENSE;
    if (narrow_wave_applicable(d)) return PATH_WAVE;
    if (rowconv_applicable(d)) return PATH_ROWCONV;
    if (narrow_applicable(d)) return PATH_NARROW;
  }
  if (rgbin_applicable(d)) return PATH_RGBIN;       // 3-channel 7x7 input layer: LDS-staged halo on the MFMA (conv_rgbin.hip)
  if (wino_applicable(d, 0)) return PATH_WINO;      // bias / activation fused in its epilogue too
  return PATH_IGEMM;
}

void fwd_geometry(const srgan_conv_desc* d, FwdPath path, IgemmParams& p) {
  p.NB = d->N; p.Hs = d->Hi; p.Ws = d->Wi; p.Cs = d->I;
  p.Hg = d->Ho; p.Wg = d->Wo; p.Hd = d->Ho; p.Wd = d->Wo; p.Cd = d->O;
  p.mode = 0; p.stride = d->stride; p.pad = d->pad; p.Ty = d->kh; p.Tx = d->kw;
  p.K = d->kh * d->kw * d->I; p.Kpad = (int)round_up(p.K, BK);
  p.M = d->N * d->Ho * d->Wo;
  p.Npad = (path == PATH_WAVE || path == PATH_DENSE) ? d->O : npad_for(p.M, d->O);
  p.reflect = d->pad_mode == SRGAN_PAD_REFLECT;
}

static int fwd_run(const srgan_conv_desc* d, const float* x, const float* wp, const float* bias, float* y, int act,
                   float slope, float* scratch, hipStream_t st) {
  const FwdPath path = fwd_path(d, act);
  if (path == PATH_ROWCONV) return rowconv_run(d, x, wp, bias, y, st);
  if (path == PATH_NARROW) return narrow_fwd_packed(d, x, wp, bias, y, st);
  if (path == PATH_RGBIN) return rgbin_run(d, x, wp, bias, y, act, slope, st);
  if (path == PATH_WINO) return wino_run(d, 0, x, wp, bias, y, act, slope, scratch, st);
  IgemmParams p{};
  fwd_geometry(d, path, p);
  p.src = x; p.bias = bias; p.dst = y; p.act = act; p.slope = slope; p.wp = wp;
  if (path == PATH_DENSE) return dense_head_fwd(d, x, wp, p.Kpad, bias, y, st);
  if (path == PATH_WAVE) return narrow_wave_fwd(d, x, wp, p.Kpad, bias, y, st);
  return run_igemm(p, 1, st, conv_flops(d), scratch);      // scratch (may be null): room for split-K slabs
}

// ---- input gradient / transposed-conv forward ----
// Input gradient of a stride-1 zero-padded conv with <= 4 INPUT channels (the generator's 7x7 RGB layer inside the
// cycle / identity passes) = a narrow-OUTPUT convolution of dy with the flipped, transposed filter.  The implicit
// GEMM would pad those 3 channels to a 32-wide MFMA tile (9 % useful); conv_narrow.hip serves them directly.
bool narrow_dgrad_desc(const srgan_conv_desc* d, srgan_conv_desc* f, long long* w_off) {
  if (d->stride != 1 || d->pad_mode != SRGAN_PAD_ZERO || d->I > 4 || d->kh != d->kw || d->kh - 1 - d->pad < 0) return false;
  *f = *d;
  f->Hi = d->Ho; f->Wi = d->Wo; f->Ho = d->Hi; f->Wo = d->Wi; f->I = d->O; f->O = d->I;
  f->pad = d->kh - 1 - d->pad;
  f->sO = d->sI; f->sI = d->sO; f->sH = -d->sH; f->sW = -d->sW;     // w'[i][o][ky][kx] = w[o][i][kh-1-ky][kw-1-kx]
  *w_off = (long long)(d->kh - 1) * d->sH + (long long)(d->kw - 1) * d->sW;
  return narrow_applicable(f);
}

// Input gradient of a stride-1 zero-padded conv with 3 OUTPUT channels (the generator's 7x7 RGB head) = a 3-channel-INPUT
// convolution of dy with the flipped, transposed filter: conv_rgbin.hip.
bool rgbin_dgrad_desc(const srgan_conv_desc* d, srgan_conv_desc* f, long long* w_off) {
  if (d->stride != 1 || d->pad_mode != SRGAN_PAD_ZERO || d->O != 3 || d->kh != d->kw || d->kh - 1 - d->pad < 0) return false;
  *f = *d;
  f->Hi = d->Ho; f->Wi = d->Wo; f->Ho = d->Hi; f->Wo = d->Wi; f->I = d->O; f->O = d->I;
  f->pad = d->kh - 1 - d->pad;
  f->sO = d->sI; f->sI = d->sO; f->sH = -d->sH; f->sW = -d->sW;     // w'[i][o][ky][kx] = w[o][i][kh-1-ky][kw-1-kx]
  *w_off = (long long)(d->kh - 1) * d->sH + (long long)(d->kw - 1) * d->sW;
  return rgbin_applicable(f);
}

// Input gradient of a STRIDE-2 zero-padded conv with <= 4 input channels (the encoder's 7x7 / stride-2 RGB layer inside phase 2,
// D's 4x4 / stride-2 RGB layers inside phase 1): the implicit GEMM pads the 3 channels to a 32-wide MFMA tile (6.7 TFLOP/s,
// 0.69 ms for one launch of the step).  Row parity pp of the input pixel selects the taps ky = ky0 + 2a (ky0 = (pp + pad) & 1),
// so phase image (pp, qq) = dx[2u + pp][2v + qq] is a STRIDE-1 narrow-output convolution of dy with the flipped sub-filter:
//   dx_pq[u][v][c] = sum_{o, a', b'} dy[u + a' - pad_y][v + b' - pad_x][o] * w[o][c][ky0 + 2 (na - 1 - a')][kx0 + 2 (nb - 1 - b')]
// with pad_y = (na - 1) - (pp + pad - ky0) / 2: four launches of conv_narrow.hip's generic kernel that scatter their pixels with
// stride 2 into dx.  Returns false when the layer does not qualify.
bool narrow_s2_phase(const srgan_conv_desc* d, int pp, int qq, srgan_conv_desc* f, long long* w_off, int* pad_x,
                            size_t* packed_off) {
  static const bool off = SRGAN_AB_SET("SRGAN_NO_NARROW_S2");
  if (off || d->stride != 2 || d->pad_mode != SRGAN_PAD_ZERO || d->I > 4 || d->O % 16 != 0 || d->kh != d->kw || d->kh < 2 ||
      d->kh > 8 || d->Hi < 2 || d->Wi < 2)
    return false;
  size_t off_elems = 0;
  for (int ph = 0; ph < 4; ++ph) {
    const int p1 = ph >> 1, q1 = ph & 1;
    const int ky0 = (p1 + d->pad) & 1, kx0 = (q1 + d->pad) & 1;
    const int na = (d->kh - ky0 + 1) / 2, nb = (d->kw - kx0 + 1) / 2;
    if (p1 == pp && q1 == qq) {
      *f = *d;
      f->Hi = d->Ho; f->Wi = d->Wo; f->I = d->O; f->O = d->I;
      f->Ho = (d->Hi - pp + 1) / 2; f->Wo = (d->Wi - qq + 1) / 2;
      f->kh = na; f->kw = nb; f->stride = 1;
      f->pad = (na - 1) - (pp + d->pad - ky0) / 2;
      *pad_x = (nb - 1) - (qq + d->pad - kx0) / 2;
      f->sO = d->sI; f->sI = d->sO; f->sH = -2 * d->sH; f->sW = -2 * d->sW;
      *w_off = (long long)(ky0 + 2 * (na - 1)) * d->sH + (long long)(kx0 + 2 * (nb - 1)) * d->sW;
      *packed_off = off_elems;
      return f->Ho > 0 && f->Wo > 0 && na > 0 && nb > 0 && f->pad >= 0 && *pad_x >= 0;
    }
    off_elems += (size_t)d->O * na * nb * 4;
  }
  return false;
}
static size_t narrow_s2_packed_elems(const srgan_conv_desc* d) {
  size_t n = 0;
  for (int ph = 0; ph < 4; ++ph) {
    const int ky0 = ((ph >> 1) + d->pad) & 1, kx0 = ((ph & 1) + d->pad) & 1;
    n += (size_t)d->O * ((d->kh - ky0 + 1) / 2) * ((d->kw - kx0 + 1) / 2) * 4;
  }
  return n;
}

DgradGeom dgrad_geometry(const srgan_conv_desc* d) {
  DgradGeom g{};
  g.reflect = d->pad_mode == SRGAN_PAD_REFLECT;
  const int s = d->stride;
  // reflect: gradient w.r.t. the padded image (a pad-0 conv over Hi+2P), then fold.
  const int P = g.reflect ? d->pad : 0;
  g.Hd = d->Hi + 2 * P; g.Wd = d->Wi + 2 * P;
  IgemmParams& p = g.p;
  p.bias = nullptr;
  p.NB = d->N; p.Hs = d->Ho; p.Ws = d->Wo; p.Cs = d->O;
  p.Hg = (int)ceil_div(g.Hd, s); p.Wg = (int)ceil_div(g.Wd, s);
  p.Hd = g.Hd; p.Wd = g.Wd; p.Cd = d->I;
  p.mode = 1; p.stride = s; p.pad = g.reflect ? 0 : d->pad;
  p.Ty = (int)ceil_div(d->kh, s); p.Tx = (int)ceil_div(d->kw, s);
  p.K = p.Ty * p.Tx * d->O; p.Kpad = (int)round_up(p.K, BK);
  p.M = d->N * p.Hg * p.Wg;
  p.Npad = npad_for(p.M, d->I);
  p.reflect = 0; p.act = SRGAN_ACT_NONE; p.slope = 0.f;
  g.phases = s * s;
  g.packed_elems = (size_t)g.phases * p.Npad * p.Kpad;
  g.wino = wino_applicable(d, 1);
  if (g.wino) g.packed_elems = wino_packed_bytes(d, 1) / sizeof(float);
  srgan_conv_desc f;
  long long w_off;
  g.narrow = !g.wino && narrow_dgrad_desc(d, &f, &w_off);
  if (g.narrow) g.packed_elems = rowconv_applicable(&f) ? rowconv_packed_elems(&f) : (size_t)f.I * f.kh * f.kw * 4;
  g.rgbin = !g.wino && !g.narrow && rgbin_dgrad_desc(d, &f, &w_off);
  if (g.rgbin) g.packed_elems = rgbin_packed_elems(&f);
  int px;
  size_t po;
  g.narrow_s2 = !g.wino && !g.narrow && !g.rgbin && narrow_s2_phase(d, 0, 0, &f, &w_off, &px, &po);
  if (g.narrow_s2) g.packed_elems = narrow_s2_packed_elems(d);
  return g;
}

// bytes of split-K slabs the implicit-GEMM forward (kind 0) / input gradient (kind 1) of d wants (0: another kernel family
// serves it, or the layer is not split)
size_t conv_splitk_bytes(const srgan_conv_desc* d, int kind) {
  if (kind == 0) {
    const FwdPath path = fwd_path(d, SRGAN_ACT_NONE);
    if (path != PATH_IGEMM) return 0;
    IgemmParams p{};
    fwd_geometry(d, path, p);
    return igemm_splitk_bytes(p, 1);
  }
  const DgradGeom g = dgrad_geometry(d);
  if (g.wino || g.narrow || g.rgbin || g.narrow_s2) return 0;
  return igemm_splitk_bytes(g.p, g.phases);
}

__global__ void add_inplace_kernel(float* __restrict__ y, const float* __restrict__ r, long long n4, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x)
    reinterpret_cast<f32x4*>(y)[i] += reinterpret_cast<const f32x4*>(r)[i];
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) y[n4 * 4 + threadIdx.x] += r[n4 * 4 + threadIdx.x];
}

// `scratch`: room for the padded gradient when the conv is reflect-padded
static int dgrad_run_core(const srgan_conv_desc* d, const float* dy, const float* wp, float* dx, float* scratch, hipStream_t st,
                          const float* res, bool* res_done, const float* mask, float mask_slope, bool* mask_done) {
  DgradGeom g = dgrad_geometry(d);
  g.p.src = dy; g.p.wp = wp;
  g.p.dst = g.reflect ? scratch : dx;
  if (g.narrow) {
    srgan_conv_desc f;
    long long w_off;
    narrow_dgrad_desc(d, &f, &w_off);
    if (rowconv_applicable(&f)) return rowconv_run(&f, dy, wp, nullptr, dx, st);
    return narrow_fwd_packed(&f, dy, wp, nullptr, dx, st);
  }
  if (g.rgbin) {
    srgan_conv_desc f;
    long long w_off;
    rgbin_dgrad_desc(d, &f, &w_off);
    return rgbin_run(&f, dy, wp, nullptr, dx, SRGAN_ACT_NONE, 0.f, st);
  }
  if (g.narrow_s2) {
    for (int ph = 0; ph < 4; ++ph) {
      srgan_conv_desc f;
      long long w_off;
      int px;
      size_t po;
      if (!narrow_s2_phase(d, ph >> 1, ph & 1, &f, &w_off, &px, &po)) { set_error("narrow stride-2 dgrad: phase geometry"); return -1; }
      if (int e = narrow_fwd_strided(&f, px, dy, wp + po, dx, d->Hi, d->Wi, ph >> 1, ph & 1, st)) return e;
    }
    return 0;
  }
  if (g.wino) {
    // (F(4,3) needs zero padding, the fold scratch needs reflect padding: the two uses of `scratch` never meet)
    // (the mask rides in the epilogue only when nothing is added to dx afterwards)
    if (int e = wino_run(d, 1, dy, wp, nullptr, g.p.dst, SRGAN_ACT_NONE, 0.f, g.reflect ? nullptr : scratch, st,
                         g.reflect ? nullptr : res, res_done, false, (g.reflect || res) ? nullptr : mask, mask_slope, mask_done)) return e;
  } else {
    // split-K slabs sit behind the padded-gradient temp of a reflect layer
    float* slab = scratch ? (g.reflect ? scratch + round_up((long long)d->N * g.Hd * g.Wd * d->I, 64) : scratch) : nullptr;
    if (int e = run_igemm(g.p, g.phases, st, conv_flops(d), slab)) return e;
  }
  if (g.reflect) {
    long long n = (long long)d->N * d->Hi * d->Wi * d->I;
    hipLaunchKernelGGL(reflect_fold_kernel<false>, dim3((unsigned)std::min<long long>(ceil_div(n, 256), 8192)), dim3(256), 0, st,
                       (const float*)scratch, dx, d->N, d->Hi, d->Wi, d->I, d->pad);
    return check_launch("reflect_fold_kernel");
  }
  return 0;
}

// dx = dgrad(dy) (+ res): the F(4x4,3x3) kernel adds `res` in its epilogue; every other dispatch gets one in-place add pass
// ... (* mask): the LeakyReLU backward of the layer that produced this layer's input (mask = that activated tensor): in the
// epilogue of the transposed F(3x3,2x2) kernel, one in-place elementwise pass behind every other dispatch
static int dgrad_run(const srgan_conv_desc* d, const float* dy, const float* wp, float* dx, float* scratch, hipStream_t st,
                     const float* res = nullptr, const float* mask = nullptr, float mask_slope = 0.f) {
  bool done = false, mdone = false;
  if (int e = dgrad_run_core(d, dy, wp, dx, scratch, st, res, &done, mask, mask_slope, &mdone)) return e;
  if (res && !done) {
    const long long n = (long long)d->N * d->Hi * d->Wi * d->I, n4 = n / 4;
    hipLaunchKernelGGL(add_inplace_kernel, dim3((unsigned)std::max<long long>(1, std::min<long long>(ceil_div(n4, 256), 8192))),
                       dim3(256), 0, st, dx, res, n4, n);
    if (int e = check_launch("add_inplace_kernel")) return e;
  }
  if (mask && !mdone)
    return srgan_act_bwd(mask, dx, dx, (long long)d->N * d->Hi * d->Wi * d->I, SRGAN_ACT_LRELU, mask_slope, st);
  return 0;
}

// every direction of the layer on the generic bf16 kernels, with the vector paths their 16-bit loads need
bool igemm16_io_ok(const srgan_conv_desc* d, int act) {
  if (!compute_bf16() || (d->I & 3) || (d->O & 3)) return false;
  if (fwd_path(d, act) != PATH_IGEMM) return false;
  IgemmParams p{};
  fwd_geometry(d, PATH_IGEMM, p);
  if (!igemm16_ok(p)) return false;
  const DgradGeom g = dgrad_geometry(d);
  if (g.wino || g.narrow || g.rgbin || g.narrow_s2 || !igemm16_ok(g.p)) return false;
  if (wino_wgrad_applicable(d) || rgb_wgrad_kind(d) >= 0 || narrow_applicable(d)) return false;
  const WgradPlan w = plan_wgrad(d);
  return w.vec && !w.rows && w.BMc >= 64 && w.BNn >= 64;
}

// The implicit-GEMM route of srgan_igemm16_conv and srgan_conv2d_io_fwd / _dgrad.  `scratch`: the checked workspace, or null.
static int igemm16_io_fwd(const srgan_conv_desc* d, const void* src, int src_bf16, const void* packed, const float* bias, void* dst,
                          int dst_bf16, int act, float slope, float* scratch, hipStream_t st) {
  IgemmParams p{};
  fwd_geometry(d, PATH_IGEMM, p);
  p.src = static_cast<const float*>(src); p.bias = bias; p.dst = static_cast<float*>(dst); p.act = act; p.slope = slope;
  p.wp = static_cast<const float*>(packed); p.src16 = src_bf16 != 0; p.dst16 = dst_bf16 != 0;
  return run_igemm(p, 1, st, conv_flops(d), scratch);
}

static int igemm16_io_dgrad(const srgan_conv_desc* d, const void* src, int src_bf16, const void* packed, void* dst, int dst_bf16,
                            float* scratch, hipStream_t st) {
  DgradGeom g = dgrad_geometry(d);
  g.p.src = static_cast<const float*>(src); g.p.wp = static_cast<const float*>(packed); g.p.src16 = src_bf16 != 0;
  // reflect: the gradient with respect to the padded image stays an fp32 temp; the fold writes the tensor's type
  g.p.dst = g.reflect ? scratch : static_cast<float*>(dst); g.p.dst16 = !g.reflect && dst_bf16 != 0;
  float* slab = scratch ? (g.reflect ? scratch + round_up((long long)d->N * g.Hd * g.Wd * d->I, 64) : scratch) : nullptr;
  if (int e = run_igemm(g.p, g.phases, st, conv_flops(d), slab)) return e;
  if (!g.reflect) return 0;
  const long long n = (long long)d->N * d->Hi * d->Wi * d->I;
  const dim3 fg((unsigned)std::min<long long>(ceil_div(n, 256), 8192));
  if (dst_bf16)
    hipLaunchKernelGGL(reflect_fold_kernel<true>, fg, dim3(256), 0, st, (const float*)scratch, static_cast<float*>(dst), d->N, d->Hi,
                       d->Wi, d->I, d->pad);
  else
    hipLaunchKernelGGL(reflect_fold_kernel<false>, fg, dim3(256), 0, st, (const float*)scratch, static_cast<float*>(dst), d->N, d->Hi,
                       d->Wi, d->I, d->pad);
  return check_launch("reflect_fold_kernel");
}

// The 7x7 / stride-1 / pad-3 layers between a 3-channel and a 64-channel tensor (the generator's RGB input and output layers,
// pyfiles/model.py:212, 232) with the 64-channel side in bf16: 3 = input layer (forward rgbin16 writes bf16, input gradient =
// rgbout16 form reads bf16 dy, weight gradient takes bf16 dy), 4 = output layer (forward rgbout16 reads bf16, input gradient =
// rgbin16 form writes bf16, weight gradient takes bf16 x).  The 3-channel side is always fp32.
static int conv_io_rgb(const srgan_conv_desc* d, int act) {
  if (!compute_bf16() || act != SRGAN_ACT_NONE || !rgb_wgrad16_served(d)) return 0;
  const DgradGeom g = dgrad_geometry(d);
  srgan_conv_desc f;
  long long w_off;
  if (d->I == 3) {
    if (fwd_path(d, act) != PATH_RGBIN || !rgbin16_served(d)) return 0;
    if (!g.narrow || !narrow_dgrad_desc(d, &f, &w_off) || !rowconv_applicable(&f) || !rgbout16_served(&f)) return 0;
    return 3;
  }
  if (fwd_path(d, act) != PATH_ROWCONV || !rgbout16_served(d)) return 0;
  if (!g.rgbin || !rgbin_dgrad_desc(d, &f, &w_off) || !rgbin16_served(&f)) return 0;
  return 4;
}

static bool conv_io_dirs(const srgan_conv_desc* d, int act, int* fwd, int* bwd) {      // 1: patch kernel, 2: igemm16_kernel
  if (const int r = conv_io_rgb(d, act)) { *fwd = *bwd = r; return true; }
  if (!compute_bf16() || d->kh != 4 || d->kw != 4 || d->stride != 2 || d->pad != 1 || d->pad_mode != SRGAN_PAD_ZERO) return false;
  if ((d->I & 7) || (d->O & 7)) return false;
  const FwdPath path = fwd_path(d, act);
  if (path == PATH_WINO && halo16s_applicable(d)) *fwd = 1;
  else if (path == PATH_IGEMM) {
    IgemmParams p{};
    fwd_geometry(d, PATH_IGEMM, p);
    if (!igemm16_ok(p)) return false;
    *fwd = 2;
  } else return false;
  const DgradGeom g = dgrad_geometry(d);
  if (g.wino && halo16t_applicable(d)) *bwd = 1;
  else if (!g.wino && !g.narrow && !g.rgbin && !g.narrow_s2 && !g.reflect && igemm16_ok(g.p)) *bwd = 2;
  else return false;
  return halo16_wgrad_applicable(d);
}
}  // namespace srgan

using namespace srgan;

extern "C" size_t srgan_conv2d_workspace(const srgan_conv_desc* d) {
  if (conv_validate(d) != 0) return 0;
  size_t bytes = pack_bytes(d);
  // reflect dgrad: padded-gradient temp
  if (d->pad_mode == SRGAN_PAD_REFLECT)
    bytes += (size_t)d->N * (d->Hi + 2 * d->pad) * (d->Wi + 2 * d->pad) * d->I * sizeof(float);
  // split-K slabs of the implicit-GEMM forward / input gradient, behind the packed operand (and the reflect temp)
  bytes += 256 + std::max(conv_splitk_bytes(d, 0), conv_splitk_bytes(d, 1));
  // F(4x4,3x3) layers: the transformed-input image, behind the packed operand (64-float aligned)
  bytes = std::max(bytes, (size_t)round_up((long long)pack_bytes(d), 256) + std::max(wino_scratch_bytes(d, 0), wino_scratch_bytes(d, 1)));
  WgradPlan w = plan_wgrad(d);
  if (wino_wgrad_applicable(d)) wino_wgrad_slab(d, &w.splits, &w.Cdpad, &w.NNpad);
  if (rgb_wgrad_kind(d) >= 0) rgb_wgrad_slab(d, &w.splits, &w.Cdpad, &w.NNpad);
  size_t wg = (size_t)w.splits * w.Cdpad * w.NNpad * sizeof(float);
  size_t cs = (size_t)1024 * d->O * sizeof(float);
  if (wg + cs > bytes) bytes = wg + cs;
  if (narrow_applicable(d)) bytes = std::max(bytes, narrow_workspace(d) + cs);
  {
    Wino43WgradGeom wg43{};
    if (wino43_wgrad_geometry(d, &wg43)) bytes = std::max(bytes, (size_t)round_up((long long)(wg43.slab_bytes + cs), 256) + wg43.z_bytes);
  }
  return bytes + 4096;
}

extern "C" int srgan_conv2d_fwd(const srgan_conv_desc* d, const float* x, const float* w, const float* bias,
                                float* y, int act, float slope, void* ws, size_t ws_bytes, void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(x && w && y && ws, "conv2d_fwd: null pointer");
  SRGAN_REQUIRE(ws_bytes >= srgan_conv2d_workspace(d), "conv2d_fwd: workspace too small");
  hipStream_t st = as_stream(stream);
  if (int e = fwd_pack(d, act, w, (float*)ws, st)) return e;
  return fwd_run(d, x, (const float*)ws, bias, y, act, slope, (float*)ws + round_up((long long)(pack_bytes(d) / sizeof(float)), 64), st);
}

extern "C" int srgan_conv2d_dgrad(const srgan_conv_desc* d, const float* dy, const float* w, float* dx,
                                  void* ws, size_t ws_bytes, void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(dy && w && dx && ws, "conv2d_dgrad: null pointer");
  SRGAN_REQUIRE(ws_bytes >= srgan_conv2d_workspace(d), "conv2d_dgrad: workspace too small");
  hipStream_t st = as_stream(stream);
  DgradGeom g = dgrad_geometry(d);
  if (int e = dgrad_pack(d, w, (float*)ws, st)) return e;
  return dgrad_run(d, dy, (const float*)ws, dx, (float*)ws + round_up((long long)g.packed_elems, 64), st);
}

extern "C" int srgan_conv2d_fwd_packed(const srgan_conv_desc* d, const float* x, const void* packed, const float* bias,
                                       float* y, int act, float slope, void* ws, size_t ws_bytes, void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(x && packed && y, "conv2d_fwd_packed: null pointer");
  const size_t need = srgan_conv2d_packed_scratch(d, 0);
  SRGAN_REQUIRE(need == 0 || (ws && ws_bytes >= need), "conv2d_fwd_packed: workspace too small (srgan_conv2d_packed_scratch)");
  return fwd_run(d, x, (const float*)packed, bias, y, act, slope, (float*)ws, as_stream(stream));
}

extern "C" int srgan_conv2d_dgrad_packed(const srgan_conv_desc* d, const float* dy, const void* packed, float* dx,
                                         void* ws, size_t ws_bytes, void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(dy && packed && dx, "conv2d_dgrad_packed: null pointer");
  const size_t need = srgan_conv2d_packed_scratch(d, 1);
  SRGAN_REQUIRE(need == 0 || (ws && ws_bytes >= need), "conv2d_dgrad_packed: workspace too small (srgan_conv2d_packed_scratch)");
  return dgrad_run(d, dy, (const float*)packed, dx, (float*)ws, as_stream(stream));
}

// ---- instance norm + activation feeding an F(4x4,3x3) layer without materialising the normalised tensor ----
extern "C" int srgan_instnorm_conv_v_applicable(const srgan_conv_desc* d) {
  if (conv_validate(d) != 0) return 0;
  return d->Hi == 32 && d->Wi == 32 && d->I % 32 == 0 && d->kh == 3 && d->stride == 1 && d->pad == 1 &&
         d->pad_mode == SRGAN_PAD_ZERO && fwd_path(d, SRGAN_ACT_NONE) == PATH_WINO && wino43_fwd_applicable(d) ? 1 : 0;
}

extern "C" int srgan_instnorm_fwd_v(const srgan_conv_desc* d, const float* x, const float* scale, const float* shift, float* mean,
                                    float* rstd, void* v_image, size_t v_bytes, float eps, int act, float slope, void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(x && mean && rstd && v_image, "instnorm_fwd_v: null pointer");
  SRGAN_REQUIRE((scale == nullptr) == (shift == nullptr), "instnorm_fwd_v: scale and shift go together");
  SRGAN_REQUIRE(srgan_instnorm_conv_v_applicable(d), "instnorm_fwd_v: layer not applicable (32x32 map into an F(4x4,3x3) layer)");
  SRGAN_REQUIRE(v_bytes >= srgan_conv2d_packed_scratch(d, 0), "instnorm_fwd_v: V image too small (srgan_conv2d_packed_scratch)");
  return in_fwd_slab_v_launch(x, scale, shift, mean, rstd, static_cast<float*>(v_image), d->N, d->I, eps, act, slope, as_stream(stream));
}

extern "C" int srgan_conv2d_fwd_from_v(const srgan_conv_desc* d, const void* v_image, const void* packed, const float* bias,
                                       float* y, int act, float slope, void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(v_image && packed && y, "conv2d_fwd_from_v: null pointer");
  SRGAN_REQUIRE(fwd_path(d, act) == PATH_WINO && wino43_fwd_applicable(d), "conv2d_fwd_from_v: layer does not run on F(4x4,3x3)");
  return wino_run(d, 0, nullptr, (const float*)packed, bias, y, act, slope, const_cast<float*>(static_cast<const float*>(v_image)),
                  as_stream(stream), nullptr, nullptr, true);
}

// ---- instance-norm backward feeding the F(4x4,3x3) input-gradient and weight-gradient kernels of the preceding convolution ----
// d describes that convolution (its OUTPUT is what the norm normalises).
extern "C" int srgan_instnorm_bwd_vz_applicable(const srgan_conv_desc* d) {
  if (conv_validate(d) != 0) return 0;
  Wino43WgradGeom g{};
  const DgradGeom dg = dgrad_geometry(d);
  return d->Ho == 32 && d->Wo == 32 && d->Hi == 32 && d->Wi == 32 && d->O % 32 == 0 && d->kh == 3 && d->stride == 1 && d->pad == 1 &&
         d->pad_mode == SRGAN_PAD_ZERO && dg.wino && !dg.reflect && wino43_dgrad_applicable(d) && wino43_wgrad_geometry(d, &g) ? 1 : 0;
}

extern "C" size_t srgan_instnorm_bwd_vz_z_bytes(const srgan_conv_desc* d) {
  if (conv_validate(d) != 0) return 0;
  Wino43WgradGeom g{};
  return wino43_wgrad_geometry(d, &g) ? g.z_bytes : 0;
}

extern "C" int srgan_instnorm_bwd_vz(const srgan_conv_desc* d, const float* x, const float* dy, const float* scale, const float* shift,
                                     const float* mean, const float* rstd, float* dscale, float* dshift, void* v_image, size_t v_bytes,
                                     void* z_image, size_t z_bytes, int act, float slope, void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(x && dy && mean && rstd && dscale && dshift && v_image && z_image, "instnorm_bwd_vz: null pointer");
  SRGAN_REQUIRE((scale == nullptr) == (shift == nullptr), "instnorm_bwd_vz: scale and shift go together");
  SRGAN_REQUIRE(srgan_instnorm_bwd_vz_applicable(d), "instnorm_bwd_vz: layer not applicable");
  SRGAN_REQUIRE(v_bytes >= srgan_conv2d_packed_scratch(d, 1) && z_bytes >= srgan_instnorm_bwd_vz_z_bytes(d),
                "instnorm_bwd_vz: image buffers too small (srgan_conv2d_packed_scratch(d, 1), srgan_instnorm_bwd_vz_z_bytes)");
  return in_bwd_slab_vz_launch(x, dy, scale, shift, mean, rstd, dscale, dshift, static_cast<float*>(v_image),
                               static_cast<float*>(z_image), d->N, d->O, act, slope, as_stream(stream));
}

extern "C" int srgan_conv2d_dgrad_from_v(const srgan_conv_desc* d, const void* v_image, const void* packed, const float* res,
                                         float* dx, void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(v_image && packed && dx, "conv2d_dgrad_from_v: null pointer");
  SRGAN_REQUIRE(res != dx, "conv2d_dgrad_from_v: res must not alias dx");
  const DgradGeom dg = dgrad_geometry(d);
  SRGAN_REQUIRE(dg.wino && !dg.reflect && wino43_dgrad_applicable(d), "conv2d_dgrad_from_v: the input gradient does not run on F(4x4,3x3)");
  return wino_run(d, 1, nullptr, (const float*)packed, nullptr, dx, SRGAN_ACT_NONE, 0.f,
                  const_cast<float*>(static_cast<const float*>(v_image)), as_stream(stream), res, nullptr, true);
}

extern "C" int srgan_conv2d_dgrad_packed_mask(const srgan_conv_desc* d, const float* dy, const void* packed, const float* mask,
                                              float slope, float* dx, void* ws, size_t ws_bytes, void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(dy && packed && dx && mask, "conv2d_dgrad_packed_mask: null pointer");
  SRGAN_REQUIRE(mask != dx, "conv2d_dgrad_packed_mask: mask must not alias dx");
  const size_t need = srgan_conv2d_packed_scratch(d, 1);
  SRGAN_REQUIRE(need == 0 || (ws && ws_bytes >= need), "conv2d_dgrad_packed_mask: workspace too small (srgan_conv2d_packed_scratch)");
  return dgrad_run(d, dy, (const float*)packed, dx, (float*)ws, as_stream(stream), nullptr, mask, slope);
}

extern "C" int srgan_conv2d_dgrad_packed_add(const srgan_conv_desc* d, const float* dy, const void* packed, const float* res,
                                             float* dx, void* ws, size_t ws_bytes, void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(dy && packed && dx && res, "conv2d_dgrad_packed_add: null pointer");
  SRGAN_REQUIRE(res != dx, "conv2d_dgrad_packed_add: res must not alias dx");
  const size_t need = srgan_conv2d_packed_scratch(d, 1);
  SRGAN_REQUIRE(need == 0 || (ws && ws_bytes >= need), "conv2d_dgrad_packed_add: workspace too small (srgan_conv2d_packed_scratch)");
  return dgrad_run(d, dy, (const float*)packed, dx, (float*)ws, as_stream(stream), res);
}

// ---- bf16 mode, residual-trunk shapes (conv_halo16.hip) with bf16 TENSORS on either side: the convolution kernels of the fused
// residual block (srgan_amd.ops._ResBlockBf16Fn), whose intermediates (conv outputs, normalised activation, the gradients between
// the norm and conv backward kernels) live in HBM as bf16.  `packed`: the ordinary packed operand of (d, kind) in bf16 mode
// (srgan_conv2d_pack / the pack cache).
extern "C" int srgan_halo16_applicable(const srgan_conv_desc* d) {
  if (conv_validate(d) != 0) return 0;
  return compute_bf16() && halo16_applicable(d, 0) && halo16_wgrad_applicable(d) && wino_applicable(d, 0) && wino_applicable(d, 1) ? 1 : 0;
}

// 4x4 / stride-2 / pad-1 layers whose forward (halo16s_kernel), input gradient (halo16t_kernel) and weight gradient
// (halo16s2_wgrad_kernel) all run on the LDS-resident-patch kernels in the bf16 mode: these take and write bf16 tensors
// (srgan_halo16_conv / srgan_halo16_wgrad with the *_bf16 flags) -- the generator's down / up convolutions.
extern "C" int srgan_halo16s2_applicable(const srgan_conv_desc* d) {
  if (conv_validate(d) != 0) return 0;
  return compute_bf16() && halo16s_applicable(d) && halo16t_applicable(d) && halo16_wgrad_applicable(d) && wino_applicable(d, 0) &&
         wino_applicable(d, 1) ? 1 : 0;
}

extern "C" int srgan_halo16_conv(const srgan_conv_desc* d, int kind, const void* src, int src_bf16, const void* packed,
                                 const float* res, void* dst, int dst_bf16, void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(src && packed && dst, "halo16_conv: null pointer");
  SRGAN_REQUIRE(kind == 0 || kind == 1, "halo16_conv: kind must be 0 (forward) or 1 (input gradient)");
  if (srgan_halo16s2_applicable(d)) {
    SRGAN_REQUIRE(!res, "halo16_conv: no skip tensor on the stride-2 layers");
    if (kind == 0) return halo16s_run(d, src, packed, nullptr, dst, SRGAN_ACT_NONE, 0.f, conv_flops(d), as_stream(stream), src_bf16 != 0, dst_bf16 != 0);
    return halo16t_run(d, src, packed, dst, conv_flops(d), as_stream(stream), src_bf16 != 0, dst_bf16 != 0);
  }
  SRGAN_REQUIRE(srgan_halo16_applicable(d), "halo16_conv: layer / compute mode not applicable (srgan_halo16_applicable / srgan_halo16s2_applicable)");
  return halo16_run(d, kind, src, packed, nullptr, res, dst, SRGAN_ACT_NONE, 0.f, conv_flops(d), as_stream(stream), src_bf16 != 0,
                    dst_bf16 != 0);
}

// ---- bf16 mode, the generic layers (igemm16_kernel, wgrad_kernel<BF>) with bf16 TENSORS on either side: the 3x3 reflect-padded
// convolutions of the style encoder's blocks (pyfiles/model.py:413-437), whose normalised inputs, outputs and the gradients of
// both live in HBM as bf16 (srgan_amd.ops.conv2d_io).  `packed`: the ordinary packed operand of (d, kind, act) in bf16 mode.
extern "C" int srgan_igemm16_io_applicable(const srgan_conv_desc* d, int act) {
  if (conv_validate(d) != 0) return 0;
  return igemm16_io_ok(d, act) ? 1 : 0;
}

extern "C" int srgan_igemm16_conv(const srgan_conv_desc* d, int kind, const void* src, int src_bf16, const void* packed,
                                  const float* bias, void* dst, int dst_bf16, int act, float slope, void* ws, size_t ws_bytes,
                                  void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(src && packed && dst, "igemm16_conv: null pointer");
  SRGAN_REQUIRE(kind == 0 || kind == 1, "igemm16_conv: kind must be 0 (forward) or 1 (input gradient)");
  SRGAN_REQUIRE(kind == 0 || (!bias && act == SRGAN_ACT_NONE), "igemm16_conv: bias / activation belong to the forward");
  SRGAN_REQUIRE(igemm16_io_ok(d, kind == 0 ? act : SRGAN_ACT_NONE), "igemm16_conv: layer / compute mode not applicable (srgan_igemm16_io_applicable)");
  const size_t need = srgan_conv2d_packed_scratch(d, kind);
  SRGAN_REQUIRE(need == 0 || (ws && ws_bytes >= need), "igemm16_conv: workspace too small (srgan_conv2d_packed_scratch)");
  hipStream_t st = as_stream(stream);
  float* scratch = need ? static_cast<float*>(ws) : nullptr;
  if (kind == 0) return igemm16_io_fwd(d, src, src_bf16, packed, bias, dst, dst_bf16, act, slope, scratch, st);
  return igemm16_io_dgrad(d, src, src_bf16, packed, dst, dst_bf16, scratch, st);
}

// ---- bf16 mode, round 6: 16-bit activations in the discriminator trunks (VERDICT r5 item 1 iii) ----
// SingleDiscriminator_solo (pyfiles/model.py:294-316) is [conv 4x4 / stride 2 / pad 1, no bias -> LeakyReLU(0.01)] x num_cls with
// no norm between: the tensors between the layers are written by one convolution's epilogue and read by the next one's gather.
// These entry points run such a layer with bf16 tensors on either side on whatever kernel serves the direction in the bf16 mode
// -- forward: halo16s_kernel or igemm16_kernel (bias / activation in the epilogue, LDS-DMA tiles from a bf16 source); input
// gradient: halo16t_kernel or igemm16_kernel; weight gradient: srgan_halo16_wgrad (halo16s2_wgrad_kernel takes bf16 x / dy).
// `packed`: the ordinary packed operand of (d, kind, act) in the bf16 mode (srgan_conv2d_pack / the pack cache).
extern "C" int srgan_conv2d_io_applicable(const srgan_conv_desc* d, int act) {
  if (conv_validate(d) != 0) return 0;
  int f = 0, b = 0;
  return conv_io_dirs(d, act, &f, &b) ? 1 : 0;
}

extern "C" int srgan_conv2d_io_fwd(const srgan_conv_desc* d, const void* x, int x_bf16, const void* packed, const float* bias, void* y,
                                   int y_bf16, int act, float slope, void* ws, size_t ws_bytes, void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(x && packed && y, "conv2d_io_fwd: null pointer");
  int f = 0, b = 0;
  SRGAN_REQUIRE(conv_io_dirs(d, act, &f, &b), "conv2d_io_fwd: layer / compute mode not applicable (srgan_conv2d_io_applicable)");
  hipStream_t st = as_stream(stream);
  if (f == 3) {
    SRGAN_REQUIRE(!x_bf16, "conv2d_io_fwd: the 3-channel input of the RGB input layer is fp32");
    return rgbin_run(d, static_cast<const float*>(x), static_cast<const float*>(packed), bias, static_cast<float*>(y), act, slope, st, y_bf16 != 0);
  }
  if (f == 4) {
    SRGAN_REQUIRE(!y_bf16, "conv2d_io_fwd: the 3-channel result of the RGB output layer is fp32");
    return rgbout_run(d, x, static_cast<const float*>(packed), bias, static_cast<float*>(y), st, x_bf16 != 0);
  }
  if (f == 1) return halo16s_run(d, x, packed, bias, y, act, slope, conv_flops(d), st, x_bf16 != 0, y_bf16 != 0);
  const size_t need = srgan_conv2d_packed_scratch(d, 0);
  SRGAN_REQUIRE(need == 0 || (ws && ws_bytes >= need), "conv2d_io_fwd: workspace too small (srgan_conv2d_packed_scratch)");
  return igemm16_io_fwd(d, x, x_bf16, packed, bias, y, y_bf16, act, slope, need ? static_cast<float*>(ws) : nullptr, st);
}

extern "C" int srgan_conv2d_io_dgrad(const srgan_conv_desc* d, const void* dy, int dy_bf16, const void* packed, void* dx, int dx_bf16,
                                     void* ws, size_t ws_bytes, void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(dy && packed && dx, "conv2d_io_dgrad: null pointer");
  int f = 0, b = 0;
  SRGAN_REQUIRE(conv_io_dirs(d, SRGAN_ACT_NONE, &f, &b) || conv_io_dirs(d, SRGAN_ACT_LRELU, &f, &b),
                "conv2d_io_dgrad: layer / compute mode not applicable (srgan_conv2d_io_applicable)");
  hipStream_t st = as_stream(stream);
  if (b == 3 || b == 4) {
    srgan_conv_desc f;
    long long w_off;
    if (b == 3) {          // the RGB input layer's input gradient: a 64 -> 3 channel convolution of dy (rgbout16 form)
      SRGAN_REQUIRE(!dx_bf16, "conv2d_io_dgrad: the 3-channel input gradient of the RGB input layer is fp32");
      narrow_dgrad_desc(d, &f, &w_off);
      return rgbout_run(&f, dy, static_cast<const float*>(packed), nullptr, static_cast<float*>(dx), st, dy_bf16 != 0);
    }
    SRGAN_REQUIRE(!dy_bf16, "conv2d_io_dgrad: the 3-channel gradient of the RGB output layer's result is fp32");
    rgbin_dgrad_desc(d, &f, &w_off);
    return rgbin_run(&f, static_cast<const float*>(dy), static_cast<const float*>(packed), nullptr, static_cast<float*>(dx), SRGAN_ACT_NONE, 0.f, st,
                     dx_bf16 != 0);
  }
  if (b == 1) return halo16t_run(d, dy, packed, dx, conv_flops(d), st, dy_bf16 != 0, dx_bf16 != 0);
  const size_t need = srgan_conv2d_packed_scratch(d, 1);
  SRGAN_REQUIRE(need == 0 || (ws && ws_bytes >= need), "conv2d_io_dgrad: workspace too small (srgan_conv2d_packed_scratch)");
  return igemm16_io_dgrad(d, dy, dy_bf16, packed, dx, dx_bf16, need ? static_cast<float*>(ws) : nullptr, st);
}

// ---- compute mode (BASELINE configs [2]-[4] are bf16): process-wide, set between steps ----
extern "C" int srgan_set_compute_mode(int mode) {
  SRGAN_REQUIRE(mode == 0 || mode == 1, "set_compute_mode: 0 (fp32) or 1 (bf16 MFMA, fp32 accumulate)");
  g_compute_mode = mode;
  return 0;
}
extern "C" int srgan_get_compute_mode(void) { return g_compute_mode; }
