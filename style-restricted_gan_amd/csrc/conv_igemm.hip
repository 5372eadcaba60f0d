// Implicit-GEMM convolution for gfx950 on the exact-fp32 matrix pipe (v_mfma_f32_32x32x2_f32).
//
//   out[m][n] = sum_k A[m][k] * B[n][k]
//     m = (image, grid-y, grid-x)       rows of the destination (NHWC pixels)
//     n = destination channel
//     k = (tap-y, tap-x, source channel)  gathered on the fly from the NHWC source tensor
//
// One kernel serves three reference ops (see include/srgan_hip.h):
//   mode 0  nn.Conv2d forward           src = x,  dst = y    in_y = a*stride + ty - pad
//   mode 1  conv input-gradient and     src = dy, dst = dx   in_y = a + floor((py+pad)/s) - ty
//           nn.ConvTranspose2d forward  (one launch z-slice per output parity phase (py,px);
//                                        taps ky = (py+pad)%s + s*ty, zero-weighted if ky>=kh)
// The weight operand is first repacked to [phase][Npad][Kpad] (K contiguous, zero padded) by
// pack_weights_kernel so the main loop needs no masks on B.
//
// Tiling: 256 threads = 4 waves, block tile BM x BN x 32, each wave owns TM x TN MFMA tiles of
// 32x32.  A and B tiles are staged global -> registers -> LDS (rows padded by one 16-B access
// so the ds_read_b128 fragment reads are conflict-free); the next tile's global loads are in
// flight while the current tile is multiplied.  Within a 32-deep K tile lane (r, h) feeds the
// MFMA k-slots {8q+4h+e} so that A and B fragments come from single ds_read_b128's.
//
// This file: the two forward / input-gradient kernels, their tile choice, split-K and launch (run_igemm).  Which layers come
// here is decided in conv_dispatch.hip, the packed operand is written by conv_pack.hip, the weight gradient is conv_wgrad.hip.
#include <algorithm>
#include "conv.h"
#include "prof.h"

namespace srgan {

constexpr int LDK = BK + 4;

// BF = bf16 MFMA compute (BASELINE configs [2]-[4]): operands are rounded to bf16 (RNE) when the tile is written to LDS and
// multiplied on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; HBM tensors, the gather and the epilogue stay fp32.
template <int BM, int BN, int WM, int WN, bool VEC, bool BF = false>
__global__ __launch_bounds__(WM * WN * 64) void igemm_kernel(IgemmParams p) {
  static_assert(!BF || VEC, "the bf16 variant rides on the vector gather");
  constexpr int TM = BM / (WM * 32), TN = BN / (WN * 32);
  constexpr int NT = WM * WN * 64;        // threads per workgroup (4 or 8 waves)
  constexpr int RP = NT / 8;              // tile rows staged per pass of float4 loads (8 float4 = 32 floats per row)
  constexpr int RG = NT / 32;             // tile rows staged per pass of the generic element gather
  static_assert(WM * WN == 4 || WM * WN == 8, "4 or 8 waves");
  // double-buffered operand tiles: tile t+1 is written while tile t is multiplied (one barrier per K tile)
  __shared__ __attribute__((aligned(16))) float As2[2][BM * LDK];
  __shared__ __attribute__((aligned(16))) float Bs2[2][BN * LDK];
  __shared__ int row_n[BM], row_y[BM], row_x[BM], row_o[BM];

  const int tid = threadIdx.x;
  const int mt = blockIdx.x % p.m_tiles, nt = blockIdx.x / p.m_tiles;
  const int phase = blockIdx.y;
  const int s = p.stride;
  int py = 0, px = 0;
  if (p.mode == 1) { py = phase / s; px = phase % s; }
  const int sgn = p.mode == 0 ? 1 : -1;
  const int m0 = mt * BM, n0 = nt * BN;

  for (int r = tid; r < BM; r += NT) {
    int m = m0 + r;
    int n = 0, y0 = -(1 << 28), x0 = -(1 << 28), o = -1;
    if (m < p.M) {
      n = m / (p.Hg * p.Wg);
      int rem = m - n * (p.Hg * p.Wg);
      int a = rem / p.Wg, b = rem - a * p.Wg;
      if (p.mode == 0) {
        y0 = a * s - p.pad; x0 = b * s - p.pad + p.xpad_off;
        o = (n * p.Hd + a) * p.Wd + b;
      } else {
        int oy = a * s + py, ox = b * s + px;
        if (oy < p.Hd && ox < p.Wd) {
          y0 = a + (py + p.pad) / s; x0 = b + (px + p.pad) / s;
          o = (n * p.Hd + oy) * p.Wd + ox;
        }
      }
    }
    row_n[r] = n; row_y[r] = y0; row_x[r] = x0; row_o[r] = o;
  }
  __syncthreads();

  const float* wp = p.wp + (size_t)phase * p.Npad * p.Kpad + (size_t)n0 * p.Kpad;
  // split-K: this workgroup multiplies K tiles [kt0, kt0 + nk) only and writes raw partial sums into its own slab
  const int kt0 = p.ksplit > 1 ? (int)blockIdx.z * p.kt_per_split : 0;
  const int nk = p.ksplit > 1 ? max(min(p.Kpad / BK - kt0, p.kt_per_split), 0) : p.Kpad / BK;

  // staging registers
  constexpr int A_VEC_IT = BM / RP;      // float4 per thread (VEC)
  constexpr int A_SC_IT = BM / RG;       // scalars per thread (generic)
  constexpr int B_IT = BN / RP;
  f32x4 a_reg[VEC ? A_VEC_IT : 1];
  float a_sc[VEC ? 1 : A_SC_IT];
  f32x4 b_reg[B_IT];

  auto src_index = [&](int r, int ty, int tx, bool& ok) -> size_t {
    int y = row_y[r] + sgn * ty, x = row_x[r] + sgn * tx;
    if (p.reflect) {
      if (y < 0) y = -y;
      if (y >= p.Hs) y = 2 * p.Hs - 2 - y;
      if (x < 0) x = -x;
      if (x >= p.Ws) x = 2 * p.Ws - 2 - x;
    }
    ok = (unsigned)y < (unsigned)p.Hs && (unsigned)x < (unsigned)p.Ws;
    return ((size_t)(row_n[r] * p.Hs + y) * p.Ws + x) * p.Cs;
  };

  // VEC path: the BM/32 rows a thread stages are fixed for the whole K loop.  Per row keep ONE 32-bit byte offset
  // and a tap-validity bitmask in registers; the tap / channel position is wave-uniform, so each gather is
  //   address = (scalar base of this tap & channel block) + (row offset or a safe offset)   [saddr + voffset form]
  // and costs a handful of VALU ops instead of a multiply-add chain per load.
  unsigned voff[VEC ? A_VEC_IT : 1];
  unsigned long long vmask[VEC ? A_VEC_IT : 1];
  unsigned mapy[VEC ? A_VEC_IT : 1], mapx[VEC ? A_VEC_IT : 1];   // reflect: mirrored tap displacement per nibble
  float a_msk[VEC ? A_VEC_IT : 1];
  const long long bias = ((long long)max(p.pad, p.Ty) * p.Ws + max(p.pad, p.Tx)) * p.Cs;   // keeps offsets >= 0
  if constexpr (VEC) {
    const unsigned seg16 = (tid & 7) * 16;
#pragma unroll
    for (int i = 0; i < A_VEC_IT; ++i) {
      const int r = (tid >> 3) + RP * i;
      const int y0 = row_y[r], x0 = row_x[r];
      const bool rowok = y0 > -(1 << 27);
      const long long lin = rowok ? ((long long)(row_n[r] * p.Hs + y0) * p.Ws + x0) * p.Cs : 0;
      voff[i] = (unsigned)((lin + bias) * 4) + seg16;
      unsigned long long m = 0;
      unsigned my = 0, mx = 0;
      if (rowok) {
        if (p.reflect) {
          m = ~0ull;
          for (int t = 0; t < p.Ty; ++t) {
            int y = y0 + t;
            y = y < 0 ? -y : y;
            y = y >= p.Hs ? 2 * p.Hs - 2 - y : y;
            my |= (unsigned)(y - y0) << (4 * t);
          }
          for (int t = 0; t < p.Tx; ++t) {
            int x = x0 + t;
            x = x < 0 ? -x : x;
            x = x >= p.Ws ? 2 * p.Ws - 2 - x : x;
            mx |= (unsigned)(x - x0) << (4 * t);
          }
        } else {
          int t = 0;
          for (int ty = 0; ty < p.Ty; ++ty) {
            const bool yok = (unsigned)(y0 + sgn * ty) < (unsigned)p.Hs;
            for (int tx = 0; tx < p.Tx; ++tx, ++t)
              if (yok && (unsigned)(x0 + sgn * tx) < (unsigned)p.Ws) m |= 1ull << t;
          }
        }
      }
      vmask[i] = m; mapy[i] = my; mapx[i] = mx;
    }
  }
  int tap_y = 0, tap_x = 0, tap_c = 0;       // position of the NEXT tile to load (VEC path)
  if (VEC && kt0 > 0) {
    const int k0 = kt0 * BK, t = k0 / p.Cs;
    tap_c = k0 - t * p.Cs;
    tap_y = t / p.Tx;
    tap_x = t - tap_y * p.Tx;
  }
  // generic path: per-row window origin and linear element offset of the thread's BM/RG rows
  int g_y[VEC ? 1 : A_SC_IT], g_x[VEC ? 1 : A_SC_IT], g_lin[VEC ? 1 : A_SC_IT];
  if constexpr (!VEC) {
#pragma unroll
    for (int i = 0; i < A_SC_IT; ++i) {
      const int r = (tid >> 5) + RG * i;
      g_y[i] = row_y[r];
      g_x[i] = row_x[r];
      const bool rowok = row_y[r] > -(1 << 27);
      g_lin[i] = rowok ? ((row_n[r] * p.Hs + row_y[r]) * p.Ws + row_x[r]) * p.Cs : 0;
    }
  }

  auto load_tiles = [&](int kt_rel) {
    const int kt = kt0 + kt_rel;
    const int k0 = kt * BK;
    if constexpr (VEC) {
      const unsigned seg16 = (tid & 7) * 16;
      const unsigned cs4 = p.Cs * 4;
      const int t = tap_y * p.Tx + tap_x;
      const long long tap_lin = p.reflect ? 0 : (long long)sgn * (tap_y * p.Ws + tap_x) * p.Cs;
      const char* sb = reinterpret_cast<const char*>(p.src) + (tap_lin + tap_c - bias) * 4;   // wave-uniform
      const unsigned safe = (unsigned)((bias - tap_lin) * 4) + seg16;                          // -> src + tap_c
#pragma unroll
      for (int i = 0; i < A_VEC_IT; ++i) {
        const bool ok = (vmask[i] >> t) & 1;
        // reflect: mirrored displacement from the nibble maps (all-zero maps otherwise, so no branch is needed)
        const unsigned dyv = (mapy[i] >> (4 * tap_y)) & 15u, dxv = (mapx[i] >> (4 * tap_x)) & 15u;
        unsigned off = voff[i] + (dyv * p.Ws + dxv) * cs4;
        off = ok ? off : safe;
        a_reg[i] = *reinterpret_cast<const f32x4*>(sb + off);
        a_msk[i] = ok ? 1.f : 0.f;          // applied when the tile is written to LDS (keeps the load in flight)
      }
      tap_c += BK;                                  // wave-uniform counters, branch-free wrap
      const int wc = tap_c == p.Cs;
      tap_c = wc ? 0 : tap_c;
      tap_x += wc;
      const int wx = tap_x == p.Tx;
      tap_x = wx ? 0 : tap_x;
      tap_y += wx;
    } else {
      const int kk = tid & 31;
      const int k = k0 + kk;
      const bool kok = k < p.K;
      const int t = kok ? k / p.Cs : 0;
      const int c = k - t * p.Cs;
      const int ty = t / p.Tx, tx = t - ty * p.Tx;
      if (p.reflect) {
#pragma unroll
        for (int i = 0; i < A_SC_IT; ++i) {
          const int r = (tid >> 5) + RG * i;
          bool ok;
          size_t off = src_index(r, ty, tx, ok);
          a_sc[i] = (ok && kok) ? p.src[off + c] : 0.f;
        }
      } else {
        // zero padding: the thread's rows are fixed -> row origin and linear offset live in registers; one tap /
        // channel offset per tile per thread, ~7 VALU ops per gathered element
        const int dy = sgn * ty, dx = sgn * tx;
        const int tapoff = (dy * p.Ws + dx) * p.Cs + c;
#pragma unroll
        for (int i = 0; i < A_SC_IT; ++i) {
          const bool ok = kok && (unsigned)(g_y[i] + dy) < (unsigned)p.Hs && (unsigned)(g_x[i] + dx) < (unsigned)p.Ws;
          const int off = ok ? g_lin[i] + tapoff : 0;
          const float v = p.src[off];
          a_sc[i] = ok ? v : 0.f;
        }
      }
    }
    const int seg = tid & 7;
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      const int r = (tid >> 3) + RP * i;
      b_reg[i] = *reinterpret_cast<const f32x4*>(wp + (size_t)r * p.Kpad + k0 + seg * 4);
    }
  };

  constexpr int LDH = BK + 8;              // bf16 row stride (80 B): 16-lane ds_read_b128 groups land on distinct banks
  auto store_tiles = [&](int buf) {
    float* As = As2[buf];
    float* Bs = Bs2[buf];
    if constexpr (BF) {
      unsigned short* Ah = reinterpret_cast<unsigned short*>(As);
      unsigned short* Bh = reinterpret_cast<unsigned short*>(Bs);
      const int seg = tid & 7;
#pragma unroll
      for (int i = 0; i < A_VEC_IT; ++i) {
        const int r = (tid >> 3) + RP * i;
        *reinterpret_cast<bf16x4*>(&Ah[r * LDH + seg * 4]) = __builtin_convertvector(a_reg[i] * a_msk[i], bf16x4);
      }
#pragma unroll
      for (int i = 0; i < B_IT; ++i) {
        const int r = (tid >> 3) + RP * i;
        *reinterpret_cast<bf16x4*>(&Bh[r * LDH + seg * 4]) = __builtin_convertvector(b_reg[i], bf16x4);
      }
      return;
    }
    if constexpr (VEC) {
      const int seg = tid & 7;
#pragma unroll
      for (int i = 0; i < A_VEC_IT; ++i) {
        const int r = (tid >> 3) + RP * i;
        *reinterpret_cast<f32x4*>(&As[r * LDK + seg * 4]) = a_reg[i] * a_msk[i];
      }
    } else {
      const int kk = tid & 31;
#pragma unroll
      for (int i = 0; i < A_SC_IT; ++i) {
        const int r = (tid >> 5) + RG * i;
        As[r * LDK + kk] = a_sc[i];
      }
    }
    const int seg = tid & 7;
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      const int r = (tid >> 3) + RP * i;
      *reinterpret_cast<f32x4*>(&Bs[r * LDK + seg * 4]) = b_reg[i];
    }
  };

  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave / WN, wn = wave % WN;
  const int lr = lane & 31, lh = lane >> 5;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // Software pipeline over K tiles (one barrier per tile):
  //   global loads of tile t+2 are issued right after the barrier of tile t and written to LDS during tile t+1,
  //   the q=0 fragments of tile t+1 are read right after that barrier, under the last 16 MFMAs of tile t,
  //   fragments of step q+1 are read before the MFMAs of step q.
  f32x4 af[2][TM], bf[2][TN];
  auto read_frags = [&](int buf, int q, int slot) {
    const float* As = As2[buf];
    const float* Bs = Bs2[buf];
#pragma unroll
    for (int i = 0; i < TM; ++i)
      af[slot][i] = *reinterpret_cast<const f32x4*>(&As[(wm * TM * 32 + i * 32 + lr) * LDK + q * 8 + lh * 4]);
#pragma unroll
    for (int j = 0; j < TN; ++j)
      bf[slot][j] = *reinterpret_cast<const f32x4*>(&Bs[(wn * TN * 32 + j * 32 + lr) * LDK + q * 8 + lh * 4]);
  };
  auto mfma_step = [&](int slot) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[slot][i][e], bf[slot][j][e], acc[i][j], 0, 0, 0);
  };

  if (nk > 0) {
  if constexpr (BF) {
    // 8 MFMAs (2 K-steps of 16) per wave and K tile: 256 matrix cycles against ~1000 of loads / LDS / barrier -- the loop
    // is bound by data movement, so it is kept simple: fragments of the whole tile first, then the next tile's stores
    bf16x8 ah[2][TM], bh[2][TN];
    load_tiles(0);
    store_tiles(0);
    __syncthreads();
    if (nk > 1) load_tiles(1);
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      const unsigned short* Ah = reinterpret_cast<const unsigned short*>(As2[cur]);
      const unsigned short* Bh = reinterpret_cast<const unsigned short*>(Bs2[cur]);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
          ah[q][i] = *reinterpret_cast<const bf16x8*>(&Ah[(wm * TM * 32 + i * 32 + lr) * LDH + q * 16 + lh * 8]);
#pragma unroll
        for (int j = 0; j < TN; ++j)
          bh[q][j] = *reinterpret_cast<const bf16x8*>(&Bh[(wn * TN * 32 + j * 32 + lr) * LDH + q * 16 + lh * 8]);
      }
      if (kt + 1 < nk) store_tiles(cur ^ 1);
      if (kt + 2 < nk) load_tiles(kt + 2);
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[q][i], bh[q][j], acc[i][j], 0, 0, 0);
      __syncthreads();
    }
  } else {
  load_tiles(0);
  store_tiles(0);
  __syncthreads();
  read_frags(0, 0, 0);
  if (nk > 1) load_tiles(1);

  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nk;
    read_frags(cur, 1, 1);
    mfma_step(0);
    read_frags(cur, 2, 0);
    mfma_step(1);
    if (more) store_tiles(cur ^ 1);          // tile kt+1 (its loads were issued a whole tile ago)
    read_frags(cur, 3, 1);
    mfma_step(0);
    __syncthreads();                         // tile kt+1 visible; everyone has read the last fragments of tile kt
    if (more) {
      read_frags(cur ^ 1, 0, 0);
      if (kt + 2 < nk) load_tiles(kt + 2);
    }
    mfma_step(1);
  }
  }
  }

  // epilogue: C/D map of the 32x32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
  float* const dst_base = p.ksplit > 1 ? p.dst + (size_t)blockIdx.z * p.split_stride : p.dst;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + wn * TN * 32 + j * 32 + lr;
    const bool nok = n < p.Cd;
    const float bv = (nok && p.bias) ? p.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = wm * TM * 32 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        const int o = row_o[r];
        if (nok && o >= 0) {
          float v = acc[i][j][e] + bv;
          v = apply_act(v, p.act, p.slope);
          dst_base[(size_t)o * p.Cd + n] = v;
        }
      }
    }
  }
}

// ---- bf16 mode: implicit GEMM with 64-deep K tiles (round 4) --------------------------------------------------------------
// The layers of the bf16 compute mode that no LDS-resident-patch kernel serves (the style encoder's 3x3 reflect-padded
// convolutions on 62 / 31 / 15 / 7-pixel maps, the discriminators' 4x4 stride-2 layers on 16- and 8-pixel maps, and the input
// gradients of both; pyfiles/model.py:100-121, 128-160) ran on igemm_kernel<.., BF>: a 32-deep K tile per barrier with 2-8 MFMAs
// per wave, ~100 vector instructions of address arithmetic, masking and conversion around them and fp32 weights (158-290
// TFLOP/s).  Here: 128 x BN output tiles, 4 waves of 64 x (BN / 2), K tiles of 64 channels of ONE tap (Cs % 64 == 0), 16 or 32
// MFMAs (32x32x16 bf16) per wave and barrier; the gathered rows are masked by a select on the packed bf16 pairs; fragments of
// K step q + 1 are read under the MFMAs of step q; tile kt + 1 goes to LDS in the middle of tile kt and the loads of tile
// kt + 2 are issued behind it.  Rows are 144 bytes apart in LDS (36 banks: the 16-lane groups of ds_read_b128 and the 8-lane
// row segments of ds_write_b64 land on distinct banks).  Source and destination stay fp32 in HBM and the source is rounded to
// bf16 (RNE) on the way into LDS; the weights are packed [phases][Npad][Kpad] as for igemm_kernel but already as bf16
// (PackParams::out16: the same RNE rounding, done once per optimiser step instead of once per tile), so the two kernels
// produce the same sums up to fp32 summation order.
constexpr int BK16 = 64;
constexpr int LDH16 = BK16 + 8;

// one 16-byte LDS-DMA piece per lane: lane L's bytes land at `lds` (wave-uniform) + 16 L; an out-of-range `voff` (>= bytes)
// writes zeros.  `base` / `bytes` are wave-uniform (made so here: a descriptor the compiler cannot prove uniform gets a
// waterfall loop).  A __device__ helper on raw pointers: with the builtin, or a buffer-resource VALUE, in the __global__
// template itself the HOST pass of hipcc (ROCm 7.2) drops the instantiation without a diagnostic (undefined kernel stub at load).
__device__ __forceinline__ void lds_dma16(const void* base, unsigned bytes, unsigned char* lds, unsigned voff) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(base);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  void* q = reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo);
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(q, 0, __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds, 16, voff, 0, 0, 0);
}

// DMA (round 6, VERDICT r5 item 1 ii; bf16 source tensors only): both operand tiles go global -> LDS by LDS-DMA
// (`buffer_load_dwordx4 ... lds`: lane L's 16 bytes land at the wave's LDS base + 16 L), no registers, no ds_write -- the store
// path (~80 B/clk per CU, shared by the two resident workgroups) was what bounded the loop.  The LDS image is then lane-linear:
// rows of 128 bytes WITHOUT padding, so the bank spread comes from an XOR swizzle applied on the SOURCE side -- slot s of row r
// holds the 16-byte piece s ^ ((r >> 1) & 7) (the 16 rows of a ds_read_b128 lane group hit 16 different 16-byte columns of the
// 256-byte bank row).  A masked row (zero padding, rows past M) is an out-of-range buffer offset: the DMA writes zeros
// (scratch/dma_test).  Tile kt + 1 is requested when tile kt - 1's buffer is released, one barrier per tile; the wait for a
// tile's own pieces is a counted vmcnt in front of that barrier (which then publishes every wave's pieces).
template <int BN, bool IN16 = false, bool OUT16 = false, bool DMA = false>
__global__ __launch_bounds__(256, 2) void igemm16_kernel(IgemmParams p) {
  constexpr int BM = 128;
  constexpr int ESZ = IN16 ? 2 : 4;         // bytes per source element
  constexpr int TN = BN / 64;               // 32-wide column blocks per wave (2 waves across N)
  constexpr int A_IT = BM / 32, B_IT = BN / 32;
  static_assert(BN == 128 || BN == 64, "BN");
  static_assert(!DMA || IN16, "LDS-DMA moves bf16 source rows as they are");
  constexpr int LDR = DMA ? BK16 : LDH16;   // bf16 elements per LDS row
  // ONE shared array (a second __shared__ object beside an LDS-DMA target makes hipcc drain vmcnt in front of every fragment read)
  constexpr int A_BYTES = BM * LDR * 2, B_BYTES = BN * LDR * 2, OFF_B = 2 * A_BYTES, OFF_ROW = OFF_B + 2 * B_BYTES;
  __shared__ __attribute__((aligned(16))) unsigned char smem[OFF_ROW + BM * 4];
  int* const row_o = reinterpret_cast<int*>(smem + OFF_ROW);
  auto Ah_of = [&](int buf) __attribute__((always_inline)) { return reinterpret_cast<unsigned short*>(smem + buf * A_BYTES); };
  auto Bh_of = [&](int buf) __attribute__((always_inline)) { return reinterpret_cast<unsigned short*>(smem + OFF_B + buf * B_BYTES); };

  const int tid = threadIdx.x;
  const int phase = blockIdx.y;
  const int s = p.stride;
  int py = 0, px = 0;
  if (p.mode == 1) { py = phase / s; px = phase % s; }
  const int sgn = p.mode == 0 ? 1 : -1;
  // Persistent over the output tiles (launch_igemm16: at most two workgroups per CU): a workgroup's result stores drain under
  // its next tile's prologue and K loop instead of holding its CU slot until they have landed -- with one tile per workgroup
  // the rounds run in lockstep and the epilogue of a 9-tile K loop (the encoder's 62 x 62 maps) was 40 % of the kernel.
  const int total_tiles = p.m_tiles * p.n_tiles;
  for (int tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
  int bid = tile;
  if ((total_tiles & 7) == 0) bid = (bid & 7) * (total_tiles >> 3) + (bid >> 3);   // neighbouring pixel tiles (shared image rows) on one XCD
  const int mt = bid % p.m_tiles, nt = bid / p.m_tiles;
  const int m0 = mt * BM, n0 = nt * BN;

  // window origin and destination pixel of GEMM row m.  The two divisions are float multiplications by a reciprocal with one
  // correction step (exact for m < 2^23, igemm16_ok): the prologue runs once per 128 x BN tile and K loops here are as short as
  // 9 tiles, so the ~60-instruction integer divisions and per-tap loops of igemm_kernel's prologue cost as much as the loop
  const int hw_g = p.Hg * p.Wg;
  const float inv_hw = 1.f / (float)hw_g, inv_w = 1.f / (float)p.Wg;
  const int qy = p.mode == 1 ? (py + p.pad) / s : 0, qx = p.mode == 1 ? (px + p.pad) / s : 0;
  auto fdiv = [](int m, int d, float inv, int& q, int& r) __attribute__((always_inline)) {
    q = (int)((float)m * inv);
    r = m - q * d;
    if (r >= d) { ++q; r -= d; }
    if (r < 0) { --q; r += d; }
  };
  auto row_geom = [&](int m, int& n, int& y0, int& x0, int& o) __attribute__((always_inline)) {
    n = 0; y0 = -(1 << 28); x0 = -(1 << 28); o = -1;
    if (m < p.M) {
      int rem, a, b;
      fdiv(m, hw_g, inv_hw, n, rem);
      fdiv(rem, p.Wg, inv_w, a, b);
      if (p.mode == 0) {
        y0 = a * s - p.pad; x0 = b * s - p.pad + p.xpad_off;
        o = (n * p.Hd + a) * p.Wd + b;
      } else {
        const int oy = a * s + py, ox = b * s + px;
        if (oy < p.Hd && ox < p.Wd) {
          y0 = a + qy; x0 = b + qx;
          o = (n * p.Hd + oy) * p.Wd + ox;
        }
      }
    }
  };
  if (tid < BM) {
    int n, y0, x0, o;
    row_geom(m0 + tid, n, y0, x0, o);
    row_o[tid] = o;
  }

  const unsigned short* wp = reinterpret_cast<const unsigned short*>(p.wp) + (size_t)phase * p.Npad * p.Kpad;
  const int kt0 = p.ksplit > 1 ? (int)blockIdx.z * p.kt_per_split : 0;
  int nk = p.ksplit > 1 ? max(min(p.Kpad / BK16 - kt0, p.kt_per_split), 0) : p.Kpad / BK16;
#ifdef SRGAN_EXPERIMENTS
  if (p.exp & 16) nk = 0;
#endif

  // a thread stages 4 pixel rows (8 lanes per row: floats [4 seg, 4 seg + 4) and [32 + 4 seg, ...) of the 64-channel slice);
  // per row ONE 32-bit byte offset, the valid tap rows / tap columns as two 8-bit ranges (zero padding is separable) and, for
  // reflect padding, the mirrored tap displacements as nibbles
  const unsigned seg16 = (tid & 7) * 16;
  unsigned voff[A_IT], vmask[A_IT];          // vmask: bits 0-7 valid tap rows, bits 8-15 valid tap columns
  unsigned mapy[A_IT], mapx[A_IT];
  const long long bias = ((long long)max(p.pad, p.Ty) * p.Ws + max(p.pad, p.Tx)) * p.Cs;   // keeps offsets >= 0
  auto bits = [](int lo, int hi) -> unsigned { return hi >= lo ? ((2u << (hi & 31)) - 1u) & ~((1u << (lo & 31)) - 1u) : 0u; };
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    int n, y0, x0, o;
    row_geom(m0 + (tid >> 3) + 32 * i, n, y0, x0, o);
    const bool rowok = y0 > -(1 << 27);
    const long long lin = rowok ? ((long long)(n * p.Hs + y0) * p.Ws + x0) * p.Cs : 0;
    voff[i] = (unsigned)((lin + bias) * ESZ) + seg16;
    unsigned m = 0, my = 0, mx = 0;
    if (p.reflect) {
      if (rowok) {
        m = 0xffffu;
        for (int t = 0; t < p.Ty; ++t) {
          int y = y0 + t;
          y = y < 0 ? -y : y;
          y = y >= p.Hs ? 2 * p.Hs - 2 - y : y;
          my |= (unsigned)(y - y0) << (4 * t);
        }
        for (int t = 0; t < p.Tx; ++t) {
          int x = x0 + t;
          x = x < 0 ? -x : x;
          x = x >= p.Ws ? 2 * p.Ws - 2 - x : x;
          mx |= (unsigned)(x - x0) << (4 * t);
        }
      }
    } else if (rowok) {
      // tap ty reads image row y0 + sgn ty: valid for ty in [lo, hi]
      const unsigned ym = sgn > 0 ? bits(max(0, -y0), min(p.Ty - 1, p.Hs - 1 - y0)) : bits(max(0, y0 - p.Hs + 1), min(p.Ty - 1, y0));
      const unsigned xm = sgn > 0 ? bits(max(0, -x0), min(p.Tx - 1, p.Ws - 1 - x0)) : bits(max(0, x0 - p.Ws + 1), min(p.Tx - 1, x0));
      m = ym | (xm << 8);
    }
    vmask[i] = m; mapy[i] = my; mapx[i] = mx;
  }
  int tap_y = 0, tap_x = 0, tap_c = 0;       // position of the NEXT tile to load (wave-uniform)
  if (kt0 > 0) {
    const int k0 = kt0 * BK16, t = k0 / p.Cs;
    tap_c = k0 - t * p.Cs;
    tap_y = t / p.Tx;
    tap_x = t - tap_y * p.Tx;
  }
  // weight rows of this thread: n0 + (tid >> 3) + 32 i, clamped to the packed rows (columns >= Cd are never stored)
  unsigned woff[B_IT];
#pragma unroll
  for (int i = 0; i < B_IT; ++i) woff[i] = (unsigned)(((size_t)min(n0 + (tid >> 3) + 32 * i, p.Npad - 1) * p.Kpad) * 2) + seg16;

  f32x4 a_reg[A_IT][2], b_reg[B_IT];          // b_reg: 8 bf16 weights (row, k = 8 seg .. 8 seg + 7)
  bool a_ok[A_IT];
  auto load_tiles = [&](int kt_rel) __attribute__((always_inline)) {
    const int k0 = (kt0 + kt_rel) * BK16;
    const unsigned cs4 = p.Cs * ESZ;
    const long long tap_lin = p.reflect ? 0 : (long long)sgn * (tap_y * p.Ws + tap_x) * p.Cs;
    const char* sb = reinterpret_cast<const char*>(p.src) + (tap_lin + tap_c - bias) * ESZ;   // wave-uniform
    const unsigned safe = (unsigned)((bias - tap_lin) * ESZ) + seg16;                          // -> src + tap_c
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const bool ok = ((vmask[i] >> tap_y) & (vmask[i] >> (8 + tap_x)) & 1u) != 0;
      // reflect: mirrored displacement from the nibble maps (all-zero maps otherwise)
      const unsigned dyv = (mapy[i] >> (4 * tap_y)) & 15u, dxv = (mapx[i] >> (4 * tap_x)) & 15u;
      unsigned off = voff[i] + (dyv * p.Ws + dxv) * cs4;
      off = ok ? off : safe;
#ifdef SRGAN_EXPERIMENTS
      if (p.exp & 1) { a_reg[i][0] = f32x4{1.f, 1.f, 1.f, 1.f}; a_reg[i][1] = a_reg[i][0]; a_ok[i] = ok; continue; }
#endif
      // IN16: the 64-channel slice of a pixel is 128 bytes -- one 16-byte piece per lane, already in LDS order
      a_reg[i][0] = *reinterpret_cast<const f32x4*>(sb + off);
      if constexpr (!IN16) a_reg[i][1] = *reinterpret_cast<const f32x4*>(sb + off + 128);
      a_ok[i] = ok;
    }
    tap_c += BK16;
    const int wc = tap_c == p.Cs;
    tap_c = wc ? 0 : tap_c;
    tap_x += wc;
    const int wx = tap_x == p.Tx;
    tap_x = wx ? 0 : tap_x;
    tap_y += wx;
    const char* wb = reinterpret_cast<const char*>(wp) + (size_t)k0 * 2;
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
#ifdef SRGAN_EXPERIMENTS
      if (p.exp & 2) { b_reg[i] = f32x4{1.f, 1.f, 1.f, 1.f}; continue; }
#endif
      b_reg[i] = *reinterpret_cast<const f32x4*>(wb + woff[i]);
    }
  };
  auto store_tiles = [&](int buf) __attribute__((always_inline)) {
    unsigned short* Ah = Ah_of(buf);
    unsigned short* Bh = Bh_of(buf);
    const int seg = tid & 7;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const int r = (tid >> 3) + 32 * i;
      if constexpr (IN16) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(&Ah[r * LDH16 + seg * 8]) = a_ok[i] ? a_reg[i][0] : z;
        continue;
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        u32x2 v = __builtin_bit_cast(u32x2, __builtin_convertvector(a_reg[i][h], bf16x4));
        v[0] = a_ok[i] ? v[0] : 0u;
        v[1] = a_ok[i] ? v[1] : 0u;
        *reinterpret_cast<u32x2*>(&Ah[r * LDH16 + h * 32 + seg * 4]) = v;
      }
    }
#pragma unroll
    for (int i = 0; i < B_IT; ++i) *reinterpret_cast<f32x4*>(&Bh[((tid >> 3) + 32 * i) * LDH16 + seg * 8]) = b_reg[i];
  };

  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int lr = lane & 31, lh = lane >> 5;

  f32x16 acc[2][TN];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  bf16x8 ah[2][2], bh[2][TN];
  auto read_frags = [&](int buf, int q, int slot) __attribute__((always_inline)) {
    const unsigned short* Ah = Ah_of(buf);
    const unsigned short* Bh = Bh_of(buf);
    // DMA image: piece 2 q + lh of a row sits in slot (2 q + lh) ^ ((row >> 1) & 7); the row bases are multiples of 16
    const int col = DMA ? (((2 * q + lh) ^ ((lr >> 1) & 7)) * 8) : (q * 16 + lh * 8);
#pragma unroll
    for (int i = 0; i < 2; ++i) ah[slot][i] = *reinterpret_cast<const bf16x8*>(&Ah[(wm * 64 + i * 32 + lr) * LDR + col]);
#pragma unroll
    for (int j = 0; j < TN; ++j) bh[slot][j] = *reinterpret_cast<const bf16x8*>(&Bh[(wn * (BN / 2) + j * 32 + lr) * LDR + col]);
  };
  auto mma = [&](int slot) __attribute__((always_inline)) {
#ifdef SRGAN_EXPERIMENTS
    if (p.exp & 4) return;
#endif
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[slot][i], bh[slot][j], acc[i][j], 0, 0, 0);
  };

  if constexpr (DMA) {
    // ---- LDS-DMA tiles: per thread 4 source rows (A) and B_IT weight rows, one 16-byte piece each, slot = tid & 7 ----
    const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned key = (tid >> 4) & 7, piece16 = ((tid & 7) ^ key) * 16;       // the piece this lane's slot holds
    const unsigned a_bytes = (unsigned)((size_t)p.NB * p.Hs * p.Ws * p.Cs * 2), b_bytes = (unsigned)((size_t)p.Npad * p.Kpad * 2);
    constexpr unsigned kOutside = 0x80000000u;
    int abase[A_IT];                      // byte offset of the row's window origin (tap (0, 0), channel 0) + this lane's piece
#pragma unroll
    for (int i = 0; i < A_IT; ++i) abase[i] = (int)voff[i] - (int)(bias * ESZ) - (int)seg16 + (int)piece16;
    unsigned wbase[B_IT];
#pragma unroll
    for (int i = 0; i < B_IT; ++i) wbase[i] = woff[i] - seg16 + piece16;
    auto dma_tile = [&](int buf, int kt_rel) __attribute__((always_inline)) {
      const int k0 = (kt0 + kt_rel) * BK16;
      const int tap_off = ((p.reflect ? 0 : sgn * (tap_y * p.Ws + tap_x)) * p.Cs + tap_c) * 2;    // wave-uniform
      unsigned char* const lds_a = smem + buf * A_BYTES + wave_u * 1024;
      unsigned char* const lds_b = smem + OFF_B + buf * B_BYTES + wave_u * 1024;
#pragma unroll
      for (int i = 0; i < A_IT; ++i) {
        const bool ok = ((vmask[i] >> tap_y) & (vmask[i] >> (8 + tap_x)) & 1u) != 0;
        const unsigned dyv = (mapy[i] >> (4 * tap_y)) & 15u, dxv = (mapx[i] >> (4 * tap_x)) & 15u;
        const unsigned off = (unsigned)(abase[i] + tap_off + (int)((dyv * p.Ws + dxv) * p.Cs * 2));
        lds_dma16(p.src, a_bytes, lds_a + i * 4096, ok ? off : kOutside);
      }
#pragma unroll
      for (int i = 0; i < B_IT; ++i)
        lds_dma16(wp, b_bytes, lds_b + i * 4096, wbase[i] + (unsigned)(k0 * 2));
      tap_c += BK16;
      const int wc = tap_c == p.Cs;
      tap_c = wc ? 0 : tap_c;
      tap_x += wc;
      const int wx = tap_x == p.Tx;
      tap_x = wx ? 0 : tap_x;
      tap_y += wx;
    };
    if (nk > 0) {
      dma_tile(0, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();                                   // tile 0 and row_o are visible
      if (nk > 1) dma_tile(1, 1);
      for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        read_frags(cur, 0, 0);
        read_frags(cur, 1, 1);
        mma(0);
        read_frags(cur, 2, 0);
        mma(1);
        read_frags(cur, 3, 1);
        mma(0);
        mma(1);
        if (kt + 1 < nk) {
          // this wave's pieces of tile kt + 1 have landed; behind the barrier so have everyone's, and nobody reads buffer
          // `cur` any more: tile kt + 2 may overwrite it
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();
          asm volatile("" ::: "memory");
          if (kt + 2 < nk) dma_tile(cur, kt + 2);
        }
      }
    }
    __syncthreads();
  } else {
  if (nk > 0) {
    load_tiles(0);
    store_tiles(0);
    if (nk > 1) load_tiles(1);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      read_frags(cur, 0, 0);
      read_frags(cur, 1, 1);
      mma(0);
      read_frags(cur, 2, 0);
      mma(1);
      if (kt + 1 < nk) store_tiles(cur ^ 1);       // tile kt + 1: requested a whole tile ago
      read_frags(cur, 3, 1);
      if (kt + 2 < nk) load_tiles(kt + 2);
      mma(0);
      mma(1);
      __syncthreads();
    }
  } else {
    __syncthreads();
  }
  }

  // epilogue: C/D map of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  float* const dst_base = p.ksplit > 1 ? p.dst + (size_t)blockIdx.z * p.split_stride : p.dst;
#ifdef SRGAN_EXPERIMENTS
  if ((p.exp & 8) && acc[0][0][0] != 12345.f) { __syncthreads(); continue; }
#endif
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  const bool relu = p.act == SRGAN_ACT_RELU;
  const float neg = p.act == SRGAN_ACT_LRELU ? p.slope : 1.f;      // branch-free apply_act (same values)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    i32x4 ro[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) ro[g] = *reinterpret_cast<const i32x4*>(&row_o[wm * 64 + i * 32 + 8 * g + 4 * lh]);
    if constexpr (OUT16 && TN == 2) {
      // A bf16 row of this wave's 64 columns is ONE 128-byte line.  With a column per lane a half-wave store covers 64 bytes of
      // it (and the other column block another 64 bytes, 16 instructions later): every store is a partial-line write, and the
      // layer's result took as long to write as the fp32 one (55 us for 63 MB: scratch/io16/bench_io.py).  Lanes are paired
      // instead: the even lane of a pair takes both lanes' values of column block 0 (columns lr, lr + 1), the odd lane those of
      // block 1 (columns 32 + lr - 1, 32 + lr) -- one 4-byte store per lane and row, the 32 lanes of a half-wave write the whole
      // line, half the store instructions.  (a split-K launch writes fp32 slabs: launch_igemm16 takes OUT16 only with ksplit == 1)
      const int odd = lr & 1;
      const int n = n0 + wn * 64 + (odd ? 31 + lr : lr);        // first of this lane's two adjacent columns
      const bool nok = n < p.Cd;                                  // Cd % 4 == 0 (igemm16_io_ok): both columns in or out
      const float b0 = (nok && p.bias) ? p.bias[n] : 0.f, b1 = (nok && p.bias) ? p.bias[n + 1] : 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int o = ro[e >> 2][e & 3];
        const float own = odd ? acc[i][1][e] : acc[i][0][e], give = odd ? acc[i][0][e] : acc[i][1][e];
        const float got = __shfl_xor(give, 1, 64);
        const float v0 = (odd ? got : own) + b0, v1 = (odd ? own : got) + b1;
        const float r0 = v0 > 0.f ? v0 : (relu ? 0.f : v0 * neg), r1 = v1 > 0.f ? v1 : (relu ? 0.f : v1 * neg);
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        const bf16x2 pk = {(__bf16)r0, (__bf16)r1};
        if (nok && o >= 0) *reinterpret_cast<bf16x2*>(reinterpret_cast<__bf16*>(dst_base) + (size_t)o * p.Cd + n) = pk;
      }
    } else {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + wn * (BN / 2) + j * 32 + lr;
      const bool nok = n < p.Cd;
      const float bv = (nok && p.bias) ? p.bias[n] : 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int o = ro[e >> 2][e & 3];
        const float v = acc[i][j][e] + bv;
        const float r = v > 0.f ? v : (relu ? 0.f : v * neg);
        if constexpr (OUT16) {      // (a split-K launch writes fp32 slabs: launch_igemm16 takes OUT16 only with ksplit == 1)
          if (nok && o >= 0) reinterpret_cast<__bf16*>(dst_base)[(size_t)o * p.Cd + n] = (__bf16)r;
        } else {
          if (nok && o >= 0) dst_base[(size_t)o * p.Cd + n] = r;
        }
      }
    }
    }
  }
  __syncthreads();        // row_o and the operand buffers are rewritten by the next tile
  }
}

// ---- host side ----------------------------------------------------------------------------
static TileChoice choose_tile(long long M, int N) {
  static const bool big = !SRGAN_AB_SET("SRGAN_NO_BIG_TILE");
  if (N <= 32) return {128, 32};
  if (N <= 64) return (big && ceil_div(M, 256) >= 256) ? TileChoice{256, 64} : TileChoice{128, 64};
  long long tiles = ceil_div(M, 128) * ceil_div(N, 128);
  if (tiles < 256) return {64, 64};
  // 8-wave 256x128 workgroups (one per CU, both waves of a SIMD barrier-coupled) when the grid fills the chip in whole
  // rounds: avoids the tail in which one of two independent co-resident workgroups runs alone on its SIMDs
  long long big_tiles = ceil_div(M, 256) * ceil_div(N, 128);
  if (big && big_tiles >= 256) return {256, 128};
  return {128, 128};
}

template <int BM, int BN, int WM, int WN>
static int launch_igemm(const IgemmParams& p, int phases, bool vec, hipStream_t st, double flops) {
  ProfScope scope(prof_igemm_kernel(BM, BN, vec), flops, st);
  dim3 grid((unsigned)(p.m_tiles * p.n_tiles), (unsigned)phases, (unsigned)std::max(p.ksplit, 1));
  if (vec && compute_bf16())
    hipLaunchKernelGGL((igemm_kernel<BM, BN, WM, WN, true, true>), grid, dim3(WM * WN * 64), 0, st, p);
  else if (vec)
    hipLaunchKernelGGL((igemm_kernel<BM, BN, WM, WN, true>), grid, dim3(WM * WN * 64), 0, st, p);
  else
    hipLaunchKernelGGL((igemm_kernel<BM, BN, WM, WN, false>), grid, dim3(WM * WN * 64), 0, st, p);
  return check_launch("igemm_kernel");
}

// bf16 mode: layers whose K tiles are 64 channels of one tap run on igemm16_kernel (128 x 128 tiles; 128 x 64 for 64 outputs)
bool igemm16_ok(const IgemmParams& p) {
  static const bool off = SRGAN_AB_SET("SRGAN_NO_IGEMM16");
  if (off || !compute_bf16() || p.Cs % BK16 != 0 || p.Kpad != p.K || p.Cd < 64 || p.Ty > 8 || p.Tx > 8 || p.M >= (1 << 23)) return false;
  // byte offsets of the gather are 32-bit (as in igemm_kernel's vector path)
  return (long long)p.NB * p.Hs * p.Ws * p.Cs < (1LL << 29) && (long long)p.Npad * p.Kpad < (1LL << 29);
}
static int igemm16_bn(const IgemmParams& p) { return p.Cd <= 64 ? 64 : 128; }

// Round 6: of igemm16's layers, the 3x3 / stride-1 ones on maps large enough to fill the device run on halo16e_kernel
// (conv_halo16e.hip) -- the style encoder's convolutions on its 62- and 31-pixel maps and their input gradients.  Geometry only
// (the packed operand is laid out for the kernel that will read it, whatever the tensors' types turn out to be).
bool halo16e_ok(const IgemmParams& p) {
  if (!igemm16_ok(p) || p.stride != 1 || p.Ty != 3 || p.Tx != 3 || p.xpad_off != 0) return false;
  if (!halo16e_shape_ok(p.Cs, p.Cd) || p.Npad != p.Cd || p.K != 9 * p.Cs) return false;
  if (p.mode == 0 && p.reflect && (p.pad != 1 || p.Hs < 2 || p.Ws < 2)) return false;
  if (p.mode == 1 && p.reflect) return false;
  // a destination a few pixels wider than a multiple of the 32-column patch wastes most of its last column of patches (the
  // 33 x 33 padded gradient of a 31 x 31 layer: 73 us against the implicit GEMM's 37): at least 3/4 of the patch columns filled
  if ((long long)p.Wd * 4 < 3LL * 32 * ceil_div(p.Wd, 32) && wino_threshold_scale() > 0) return false;
  // enough workgroups for about half a device round (tests: SRGAN_WINOGRAD_THRESHOLD_SCALE=0 drives small shapes through it)
  const long long wgs = (long long)p.NB * ceil_div(p.Hd, halo16e_patch_rows(p.Cs, p.Cd)) * ceil_div(p.Wd, 32);
  return wgs >= 120 * wino_threshold_scale() && (long long)p.NB * p.Hd * p.Wd * p.Cd < (1LL << 30);
}

static int launch_halo16e(const IgemmParams& p, hipStream_t st, double flops) {
  Halo16eParams q{};
  q.src = p.src; q.wp = reinterpret_cast<const unsigned short*>(p.wp); q.bias = p.bias; q.dst = p.dst;
  q.NB = p.NB; q.Hs = p.Hs; q.Ws = p.Ws; q.Cs = p.Cs; q.Hd = p.Hd; q.Wd = p.Wd; q.N = p.Cd;
  if (p.mode == 0) {            // destination row a reads source rows a - pad + ty
    q.oy0 = -p.pad; q.ox0 = -p.pad; q.flip = 0;
  } else {                      // destination row a reads source rows a + pad - ty = (a + pad - 2) + (2 - ty)
    q.oy0 = p.pad - 2; q.ox0 = p.pad - 2; q.flip = 1;
  }
  q.reflect = p.reflect; q.act = p.act; q.slope = p.slope; q.src16 = p.src16; q.dst16 = p.dst16;
  return halo16e_run(q, flops, st);
}

static int launch_igemm16(IgemmParams p, int phases, hipStream_t st, double flops) {
  const int bn = igemm16_bn(p);
#ifdef SRGAN_EXPERIMENTS
  p.exp = (int)SRGAN_AB_INT("SRGAN_IG16_EXP", 0);
#endif
  p.m_tiles = (int)ceil_div(p.M, 128);
  p.n_tiles = (int)ceil_div(p.Cd, bn);
  ProfScope scope(PROF_IGEMM16, flops, st);
  // two resident workgroups per CU over all (phase, split) planes; a workgroup walks its plane's tiles with that stride
  const long long planes = (long long)phases * std::max(p.ksplit, 1), tiles = (long long)p.m_tiles * p.n_tiles;
  const long long gx = std::min<long long>(tiles, std::max<long long>(8, (512 / planes) & ~7LL));
  dim3 grid((unsigned)gx, (unsigned)phases, (unsigned)std::max(p.ksplit, 1));
  const bool o16 = p.dst16 != 0 && p.ksplit <= 1;
  static const bool no_dma = SRGAN_AB_SET("SRGAN_NO_IG16_DMA");       // (A/B, experiment builds only)
  const bool dma = !no_dma;
#define SRGAN_IG16(BN_)                                                                                      \
  do {                                                                                                        \
    if (p.src16 && o16 && dma) hipLaunchKernelGGL((igemm16_kernel<BN_, true, true, true>), grid, dim3(256), 0, st, p);      \
    else if (p.src16 && dma) hipLaunchKernelGGL((igemm16_kernel<BN_, true, false, true>), grid, dim3(256), 0, st, p);       \
    else if (p.src16 && o16) hipLaunchKernelGGL((igemm16_kernel<BN_, true, true>), grid, dim3(256), 0, st, p);      \
    else if (p.src16) hipLaunchKernelGGL((igemm16_kernel<BN_, true, false>), grid, dim3(256), 0, st, p);       \
    else if (o16) hipLaunchKernelGGL((igemm16_kernel<BN_, false, true>), grid, dim3(256), 0, st, p);           \
    else hipLaunchKernelGGL((igemm16_kernel<BN_, false, false>), grid, dim3(256), 0, st, p);                  \
  } while (0)
  if (bn == 64) SRGAN_IG16(64);
  else SRGAN_IG16(128);
#undef SRGAN_IG16
  return check_launch("igemm16_kernel");
}

namespace {
// ---- split-K for layers with few pixel tiles and long K loops (the encoder's 7x7 / 3x3 maps, the discriminators' 8x8 / 4x4
// maps): 64-200 four-wave workgroups walking 64-144 K tiles leave most SIMDs with one wave and nothing to hide its loads
// behind (22-48 TFLOP/s).  The K range is cut into `ksplit` pieces (grid z), every piece writes raw partial sums into its own
// destination-shaped slab, and splitk_reduce_kernel adds the slabs in split order (deterministic), the bias and the activation.
template <bool OUT16 = false>
__global__ void splitk_reduce_kernel(const float* __restrict__ slab, int ksplit, long long n4, long long stride,
                                     const float* __restrict__ bias, int Cd, int act, float slope, float* __restrict__ dst) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    f32x4 v = *reinterpret_cast<const f32x4*>(slab + i * 4);
    for (int k = 1; k < ksplit; ++k) v += *reinterpret_cast<const f32x4*>(slab + (size_t)k * stride + i * 4);
    if (bias) v += *reinterpret_cast<const f32x4*>(bias + (i * 4) % Cd);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = apply_act(v[e], act, slope);
    if constexpr (OUT16) *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(dst) + i * 4) = __builtin_convertvector(v, bf16x4);
    else *reinterpret_cast<f32x4*>(dst + i * 4) = v;
  }
}
}  // namespace

static TileChoice final_tile(const IgemmParams& p) {
  TileChoice tc = choose_tile(p.M, p.Cd);
  const bool vec = (p.Cs % BK) == 0;
  if (tc.BM == 256 && !vec) tc = {128, tc.BN};
  return tc;
}

static SplitKPlan plan_splitk(const IgemmParams& p, int phases) {
  SplitKPlan s{1, 0, (long long)p.NB * p.Hd * p.Wd * p.Cd};
  static const bool off = SRGAN_AB_SET("SRGAN_NO_SPLITK");
  static const int target = SRGAN_AB_INT("SRGAN_SPLITK_TARGET", 768);
  const bool k16 = igemm16_ok(p);
  if (phases == 1 && halo16e_ok(p)) return s;      // served by halo16e_kernel (its packed operand is the register image)
  const TileChoice tc = k16 ? TileChoice{128, igemm16_bn(p)} : final_tile(p);
  if (off || tc.BM == 256 || (p.Cd & 3) != 0 || s.dst_elems >= (1LL << 28)) return s;
  const long long wgs = ceil_div(p.M, tc.BM) * ceil_div(p.Cd, tc.BN) * phases;
  const int nk = p.Kpad / (k16 ? BK16 : BK);      // kt_per_split counts the serving kernel's K tiles
  long long ks = std::min<long long>(8, std::min<long long>(target / std::max<long long>(wgs, 1), nk / 8));
  if (ks < 2) return s;
  s.kt_per_split = (int)ceil_div(nk, ks);
  s.ksplit = (int)ceil_div(nk, s.kt_per_split);
  if (s.ksplit < 2) s.ksplit = 1;
  return s;
}

size_t igemm_splitk_bytes(const IgemmParams& p, int phases) {
  const SplitKPlan s = plan_splitk(p, phases);
  return s.ksplit > 1 ? (size_t)s.ksplit * s.dst_elems * sizeof(float) : 0;
}

static int run_igemm_tiles(IgemmParams p, int phases, hipStream_t st, double flops) {
  if (phases == 1 && p.ksplit <= 1 && halo16e_ok(p)) return launch_halo16e(p, st, flops);
  if (igemm16_ok(p)) return launch_igemm16(p, phases, st, flops);
  TileChoice tc = choose_tile(p.M, p.Cd);
  p.m_tiles = (int)ceil_div(p.M, tc.BM);
  p.n_tiles = (int)ceil_div(p.Cd, tc.BN);
  const bool vec = (p.Cs % BK) == 0;
  if (tc.BM == 256 && tc.BN == 128 && vec) return launch_igemm<256, 128, 4, 2>(p, phases, true, st, flops);
  if (tc.BM == 256 && tc.BN == 64 && vec) return launch_igemm<256, 64, 4, 2>(p, phases, true, st, flops);
  if (tc.BM == 256) { tc = {128, tc.BN}; p.m_tiles = (int)ceil_div(p.M, 128); }
  if (tc.BM == 128 && tc.BN == 128) return launch_igemm<128, 128, 2, 2>(p, phases, vec, st, flops);
  if (tc.BM == 128 && tc.BN == 64) return launch_igemm<128, 64, 2, 2>(p, phases, vec, st, flops);
  if (tc.BM == 128 && tc.BN == 32) return launch_igemm<128, 32, 4, 1>(p, phases, vec, st, flops);
  return launch_igemm<64, 64, 2, 2>(p, phases, vec, st, flops);
}

// `slab`: igemm_splitk_bytes(p, phases) bytes of scratch, or null (then the layer runs unsplit)
int run_igemm(IgemmParams p, int phases, hipStream_t st, double flops, float* slab) {
  const SplitKPlan sk = slab ? plan_splitk(p, phases) : SplitKPlan{1, 0, 0};
  float* const real_dst = p.dst;
  const float* const real_bias = p.bias;
  const int real_act = p.act;
  if (sk.ksplit > 1) {
    p.ksplit = sk.ksplit; p.kt_per_split = sk.kt_per_split; p.split_stride = sk.dst_elems;
    p.dst = slab; p.bias = nullptr; p.act = SRGAN_ACT_NONE;
  } else {
    p.ksplit = 1; p.kt_per_split = 0; p.split_stride = 0;
  }
  if (int e = run_igemm_tiles(p, phases, st, flops)) return e;
  if (sk.ksplit > 1) {
    const long long n4 = sk.dst_elems / 4;
    const dim3 rg((unsigned)std::max<long long>(1, std::min<long long>(ceil_div(n4, 256), 4096)));
    if (p.dst16)
      hipLaunchKernelGGL(splitk_reduce_kernel<true>, rg, dim3(256), 0, st, (const float*)slab, sk.ksplit, n4, sk.dst_elems, real_bias,
                         p.Cd, real_act, p.slope, real_dst);
    else
      hipLaunchKernelGGL(splitk_reduce_kernel<false>, rg, dim3(256), 0, st, (const float*)slab, sk.ksplit, n4, sk.dst_elems, real_bias,
                         p.Cd, real_act, p.slope, real_dst);
    return check_launch("splitk_reduce_kernel");
  }
  return 0;
}

int npad_for(long long M, int N) {
  TileChoice tc = choose_tile(M, N);
  return (int)round_up(N, tc.BN);
}

}  // namespace srgan
