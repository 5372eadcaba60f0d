// What the convolution files (conv_*.hip) share and nobody else needs: the parameter blocks of the implicit-GEMM kernels, the
// host functions that cross between those files, and the entry points of each kernel family.
#pragma once
#include "common.h"

namespace srgan {

// ---- conv_dispatch.hip ----
// process-wide compute mode: true = bf16 MFMA operands, fp32 accumulate
bool compute_bf16();
int conv_validate(const srgan_conv_desc* d);      // 0, or set_error + non-zero
// algorithmic FLOPs of one conv pass: 2 * (N*Ho*Wo) * O * (kh*kw*I)
double conv_flops(const srgan_conv_desc* d);

constexpr int BK = 32;      // K-tile depth of igemm_kernel: the packed operands are padded to it
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

struct IgemmParams {
  const float* src;
  const float* wp;    // packed weights [phases][Npad][Kpad]
  const float* bias;  // [Cd] or null
  float* dst;
  int NB, Hs, Ws, Cs;  // source tensor
  int Hg, Wg;          // destination grid per phase
  int Hd, Wd, Cd;      // destination tensor
  int mode, stride, pad;
  int xpad_off;        // mode 0: the column origin is b*stride - pad + xpad_off (0, or +pad for the 7x1 row convolution)
  int Ty, Tx;          // taps per phase
  int K, Kpad, Npad;
  int reflect;
  int act;
  float slope;
  int M;               // NB*Hg*Wg
  int m_tiles, n_tiles;
  int ksplit, kt_per_split;      // split-K (blockIdx.z): K tiles [z * kt_per_split, ...) -> partial sums into dst + z * split_stride
  long long split_stride;
  int src16, dst16;              // igemm16_kernel only: src / dst are bf16 tensors (the 16-bit activations of the bf16 mode)
#ifdef SRGAN_EXPERIMENTS
  int exp;                       // timing ablations of igemm16_kernel (wrong results): scratch/README.md
#endif
};

struct WgradParams {
  const float* x;
  const float* dy;
  float* slab;
  int NB, Hi, Wi, Cs, Hg, Wg, Cd, stride, pad, kw, reflect;
  int NN, NNpad, Cdpad, M, rows_per_split, co_tiles, nn_tiles;
};

struct TileChoice { int BM, BN; };
struct SplitKPlan { int ksplit, kt_per_split; long long dst_elems; };
struct WgradPlan { int BMc, BNn, splits, rows_per_split, Cdpad, NNpad, co_tiles, nn_tiles; bool vec, rows; };

// forward: which kernel family serves this layer, and the packed-weight layout it wants
enum FwdPath { PATH_IGEMM = 0, PATH_NARROW = 1, PATH_WAVE = 2, PATH_DENSE = 3, PATH_WINO = 4, PATH_ROWCONV = 5, PATH_RGBIN = 6 };
struct DgradGeom { IgemmParams p; int phases; bool reflect, wino, narrow, rgbin, narrow_s2; int Hd, Wd; size_t packed_elems; };

FwdPath fwd_path(const srgan_conv_desc* d, int act);
void fwd_geometry(const srgan_conv_desc* d, FwdPath path, IgemmParams& p);
DgradGeom dgrad_geometry(const srgan_conv_desc* d);
// the forward-convolution descriptor f (and filter offset) an input gradient runs as; false: the layer does not qualify
bool narrow_dgrad_desc(const srgan_conv_desc* d, srgan_conv_desc* f, long long* w_off);
bool rgbin_dgrad_desc(const srgan_conv_desc* d, srgan_conv_desc* f, long long* w_off);
bool narrow_s2_phase(const srgan_conv_desc* d, int pp, int qq, srgan_conv_desc* f, long long* w_off, int* pad_x, size_t* packed_off);
size_t conv_splitk_bytes(const srgan_conv_desc* d, int kind);
bool igemm16_io_ok(const srgan_conv_desc* d, int act);

// ---- conv_igemm.hip ----
bool igemm16_ok(const IgemmParams& p);
bool halo16e_ok(const IgemmParams& p);
size_t igemm_splitk_bytes(const IgemmParams& p, int phases);
// `slab`: igemm_splitk_bytes(p, phases) bytes of scratch, or null (then the layer runs unsplit)
int run_igemm(IgemmParams p, int phases, hipStream_t st, double flops, float* slab = nullptr);
int npad_for(long long M, int N);

// ---- conv_wgrad.hip ----
WgradPlan plan_wgrad(const srgan_conv_desc* d);

// ---- conv_rowconv.hip ----
bool rowconv_applicable(const srgan_conv_desc* d);
size_t rowconv_packed_elems(const srgan_conv_desc* d);
int rowconv_pack(const srgan_conv_desc* d, const float* w, float* dst, hipStream_t st);
int rowconv_run(const srgan_conv_desc* d, const float* x, const float* packed, const float* bias, float* y, hipStream_t st);

// ---- conv_pack.hip ----
size_t pack_bytes(const srgan_conv_desc* d);
int fwd_pack(const srgan_conv_desc* d, int act, const float* w, float* dst, hipStream_t st);
int dgrad_pack(const srgan_conv_desc* d, const float* w, float* dst, hipStream_t st);

// parameters of the fused Winograd forward / input-gradient kernels (conv_wino.hip, conv_wino43.hip)
struct WinoParams {
  const float* src;   // [NB][H][W][C]
  const float* u;     // [n_tiles][nchunk][16 pos][2 halves][64 couts][4 ch] transformed filters
  const float* bias;  // [Cd] or null
  float* dst;         // [NB][Ho][Wo][Cd]
  int NB, H, W, C, Ho, Wo, Cd;   // source tensor, destination tensor (Cd = its channels)
  int pad, reflect;
  int TH, TW, T;      // tile grid per image (of the phase image in mode 2), tiles in total
  int nchunk, n_tiles, m_tiles;
  int cpp;            // mode 1: chunks per input phase (C / 8; F(4x4,2x2): C / 16)
  int ipw;            // F(4x4,2x2): items per workgroup (set by wino42_launch)
  int act;            // fused activation of the epilogue (SRGAN_ACT_*)
  float slope;
  const float* res;   // F(4x4,3x3) only: tensor of the destination's shape added in the epilogue (residual gradient), or null
  const float* mask;  // transposed F(3x3,2x2) only: tensor of the destination's shape whose sign selects 1 / mask_slope per element
  float mask_slope;   //   (the LeakyReLU backward of the layer that produced the destination's forward tensor), or null
};

// conv_wino42.hip: F(4x4,2x2) kernels of the 4x4 / stride-2 layers behind wino_run (variant 7): kind 0 = strided form, 1 = transposed
int wino42_launch(const WinoParams& p, int kind, long long grid, bool mask, double flops, hipStream_t st);
// conv_wino43.hip: F(4x4,3x3) kernel behind wino_run
size_t wino43_scratch_floats(long long T, int C);
int wino43_launch(const WinoParams& p, float* vimg, long long grid, double flops, hipStream_t st, bool v_ready = false);
// instance norm + activation of a 32x32 map written straight as the V image of the following F(4x4,3x3) layer (conv_wino43.hip)
int in_fwd_slab_v_launch(const float* x, const float* scale, const float* shift, float* mean, float* rstd, float* vimg, int N,
                         int C, float eps, int act, float slope, hipStream_t st);
// F(4x4,3x3) weight gradient from the forward's V image (conv_wino43.hip; geometry and dispatch in conv_wino.hip)
struct Wino43WgradGeom { int NB, H, W, C, O, ntc, splits, chunks_per_split; size_t v_bytes, z_bytes, slab_bytes; };
bool wino43_wgrad_geometry(const srgan_conv_desc* d, Wino43WgradGeom* g);      // false: not applicable
int wino43_wgrad_launch(const Wino43WgradGeom& g, const float* vimg, const float* dy, float* zimg, float* slab, double flops, hipStream_t st, bool z_ready = false);
// instance-norm backward of a 32x32 map writing the two F(4x4,3x3) transforms of its result instead of the result (conv_wino43.hip)
int in_bwd_slab_vz_launch(const float* x, const float* gup, const float* scale, const float* shift, const float* mean,
                          const float* rstd, float* dscale, float* dshift, float* vimg, float* zimg, int N, int C, int act,
                          float slope, hipStream_t st);
bool wino43_dgrad_applicable(const srgan_conv_desc* d);    // the input gradient of d runs on F(4x4,3x3)
// conv_wino.hip: Winograd F(2x2,3x3) for 3x3 stride-1 pad-1 layers; kind 0 = forward, 1 = input gradient
bool wino_applicable(const srgan_conv_desc* d, int kind);
double wino_threshold_scale();     // test hook SRGAN_WINOGRAD_THRESHOLD_SCALE: scales the minimum-workgroup thresholds of the dispatch
size_t wino_packed_bytes(const srgan_conv_desc* d, int kind);
int wino_pack(const srgan_conv_desc* d, int kind, const float* w, float* dst, hipStream_t st);
size_t wino_scratch_bytes(const srgan_conv_desc* d, int kind);
int wino_run(const srgan_conv_desc* d, int kind, const float* src, const float* packed, const float* bias, float* dst, int act, float slope, float* scratch, hipStream_t st, const float* res = nullptr, bool* res_done = nullptr, bool v_ready = false, const float* mask = nullptr, float mask_slope = 0.f, bool* mask_done = nullptr);
bool wino43_fwd_applicable(const srgan_conv_desc* d);      // the forward of d runs on F(4x4,3x3)
bool wino_wgrad_applicable(const srgan_conv_desc* d);
void wino_wgrad_slab(const srgan_conv_desc* d, int* splits, int* Cdpad, int* NNpad);
int wino_wgrad_run(const srgan_conv_desc* d, const float* x, const float* dy, float* slab, hipStream_t st);

// conv_halo16.hip: bf16-mode 3x3 stride-1 trunk convolution with the activation patch resident in LDS (dispatch: variant 4 of
// conv_wino.hip's slot -- not a Winograd transform, it shares the packed-filter plumbing)
bool halo16_applicable(const srgan_conv_desc* d, int kind);
size_t halo16_packed_bytes(const srgan_conv_desc* d);
int halo16_run(const srgan_conv_desc* d, int kind, const void* src, const void* packed, const float* bias, const float* res,
               void* dst, int act, float slope, double flops, hipStream_t st, bool in16 = false, bool out16 = false);
bool halo16t_applicable(const srgan_conv_desc* d);        // kind 1 of a 4x4 / stride-2 layer (transposed form)
size_t halo16t_packed_bytes(const srgan_conv_desc* d);
int halo16t_run(const srgan_conv_desc* d, const void* dy, const void* packed, void* dx, double flops, hipStream_t st,
                bool in16 = false, bool out16 = false);
bool halo16s_applicable(const srgan_conv_desc* d);        // kind 0 of a 4x4 / stride-2 layer (strided form, variant 6)
size_t halo16s_packed_bytes(const srgan_conv_desc* d);
int halo16s_run(const srgan_conv_desc* d, const void* x, const void* packed, const float* bias, void* y, int act, float slope,
                double flops, hipStream_t st, bool in16 = false, bool out16 = false);
bool halo16_wgrad_applicable(const srgan_conv_desc* d);
void halo16_wgrad_slab(const srgan_conv_desc* d, int* splits, int* Cdpad, int* NNpad);
int halo16_wgrad_run(const srgan_conv_desc* d, const void* x, const void* dy, float* slab, double flops, hipStream_t st,
                     bool x16 = false, bool d16 = false);

// conv_halo16e.hip (round 6): the style encoder's 3x3 / stride-1 layers on 62- and 31-pixel maps in the bf16 mode -- LDS-resident
// halo of a ragged destination patch, filter operand from the packed register image (PackParams::regimg).  Geometry as the
// implicit GEMM states it (IgemmParams): source map Hs x Ws x Cs, destination map Hd x Wd x N, halo origin = patch origin +
// (oy0, ox0), `flip`: the filter image holds tap 8 - t at halo tap t (input gradient), `reflect`: mirrored halo coordinates.
struct Halo16eParams {
  const void* src;             // [NB][Hs][Ws][Cs] fp32, or bf16 (src16)
  const unsigned short* wp;    // register image, bf16
  const float* bias;           // [N] or null
  void* dst;                   // [NB][Hd][Wd][N] fp32, or bf16 (dst16)
  int NB, Hs, Ws, Cs, Hd, Wd, N;
  int oy0, ox0, flip, reflect, act;
  float slope;
  int src16, dst16;
  int tiles_y, tiles_x, n_tiles;       // set by halo16e_run
};
bool halo16e_shape_ok(int Cs, int N);
int halo16e_patch_rows(int Cs, int N);
int halo16e_run(Halo16eParams p, double flops, hipStream_t st);

// conv_rgbin.hip: 3-channel-input 7x7 stride-1 layers on the MFMA (LDS-staged halo)
// conv_rgbout.hip: 7x7 / stride-1 / pad-3 layers with <= 4 OUTPUT channels on the 4x4x1 MFMA (direct, LDS-resident halo and filter)
bool rgbout_applicable(const srgan_conv_desc* d);
size_t rgbout_packed_elems(const srgan_conv_desc* d);
int rgbout_pack(const srgan_conv_desc* d, const float* w, float* dst, hipStream_t st);
// src16 (bf16 mode, rgbout16_served layers): x is a bf16 tensor
int rgbout_run(const srgan_conv_desc* d, const void* x, const float* packed, const float* bias, float* y, hipStream_t st, bool src16 = false);
bool rgbout16_served(const srgan_conv_desc* d);
bool rgbin_applicable(const srgan_conv_desc* d);
size_t rgbin_packed_elems(const srgan_conv_desc* d);
int rgbin_pack(const srgan_conv_desc* d, const float* w, float* dst, hipStream_t st);
// dst16 (bf16 mode, rgbin16_served layers): y is written as bf16
int rgbin_run(const srgan_conv_desc* d, const float* x, const float* packed, const float* bias, float* y, int act, float slope, hipStream_t st,
              bool dst16 = false);
bool rgbin16_served(const srgan_conv_desc* d);
int rgb_wgrad_kind(const srgan_conv_desc* d);      // -1: not applicable
void rgb_wgrad_slab(const srgan_conv_desc* d, int* splits, int* Cdpad, int* NNpad);
int rgb_wgrad_run(const srgan_conv_desc* d, const void* x, const void* dy, float* slab, hipStream_t st, bool c64_bf16 = false);
bool rgb_wgrad16_served(const srgan_conv_desc* d);      // bf16 mode: the bf16-MFMA kernel runs (and takes a bf16 64-channel tensor)

// conv_narrow.hip: direct kernels for Cout <= 4, stride-1, zero-pad layers
bool narrow_applicable(const srgan_conv_desc* d);
size_t narrow_workspace(const srgan_conv_desc* d);
int narrow_pack(const srgan_conv_desc* d, const float* w, float* wp, hipStream_t st);
int narrow_fwd_packed(const srgan_conv_desc* d, const float* x, const float* wp, const float* bias, float* y, hipStream_t st);
int narrow_fwd_strided(const srgan_conv_desc* f, int pad_x, const float* x, const float* wp, float* y, int Hd, int Wd, int oy_off,
                       int ox_off, hipStream_t st);
bool narrow_wave_applicable(const srgan_conv_desc* d);
int narrow_wave_fwd(const srgan_conv_desc* d, const float* x, const float* wp, int Kpad, const float* bias, float* y, hipStream_t st);
bool dense_head_applicable(const srgan_conv_desc* d);
int dense_head_fwd(const srgan_conv_desc* d, const float* x, const float* wp, int Kpad, const float* bias, float* y, hipStream_t st);
int narrow_wgrad(const srgan_conv_desc* d, const float* x, const float* dy, void* ws, int* n_slabs, hipStream_t st);

}  // namespace srgan
