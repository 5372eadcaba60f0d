// The weight gradient of the implicit-GEMM convolution, and the end every weight-gradient kernel of the family shares: the slab
// sum into dW (immediate, or queued between srgan_wgrad_defer_begin and _end), the bias column sums and the accumulate switch.
#include <algorithm>
#include <cstdlib>
#include <map>
#include <mutex>
#include <vector>
#include "conv.h"
#include "prof.h"

namespace srgan {

// ---- weight gradient ----------------------------------------------------------------------
//   dW[co][nn] = sum_m dy[m][co] * X[m][nn],  nn = (ky*kw+kx)*Cs + ci, X gathered from x.
// Block tile BMc (co) x BNn (nn) over a split of the m range; partial tiles go to
// slab[split][co_pad][NNpad] and are summed by wgrad_reduce_kernel.

// ROWS: every 32-pixel K tile lies inside one image row (Wg % 32 == 0, VEC only): the tile's (n, y) and the source row
// base are wave-uniform scalars advanced with counters; a thread only adds its constant column offset.
// BF (bf16 compute mode): the 32-pixel tiles are written to LDS as bf16 [pixel][channel] rows (channel-contiguous, as they
// come from NHWC memory) and the MFMA operands -- 8 consecutive PIXELS of one channel per lane -- are fetched with the
// transposing read ds_read_b64_tr_b16 (a 16-lane group reads 4 pixel rows x 16 channels and receives them column-major).
// Row stride = channels * 2 + 64 bytes: the four rows of a block start 16 banks apart, the two blocks of a half 8 banks.
// IO16 (with BF, without ROWS): x and dy are bf16 TENSORS (the 16-bit activations of the bf16 mode outside the patch kernels:
// the style encoder's blocks); a staged piece is 4 channels = 8 bytes and goes to LDS as loaded.
template <int BMc, int BNn, int WM, int WN, bool VEC, bool ROWS = false, bool BF = false, bool IO16 = false>
__global__ __launch_bounds__((WM * WN > 4 ? WM * WN : 4) * 64) void wgrad_kernel(WgradParams p) {
  static_assert(!BF || VEC, "the bf16 variant rides on the vector gather");
  static_assert(!IO16 || (BF && !ROWS), "16-bit tensors: bf16 compute, generic row decode");
  constexpr int TM = BMc / (WM * 32), TN = BNn / (WN * 32);
  constexpr int NT = (WM * WN > 4 ? WM * WN : 4) * 64;   // threads: 4 waves (some idle for small tiles) or 8 waves
  constexpr int A_IT = 8 * BMc / NT, B_IT = 8 * BNn / NT;     // float4 per thread per 32-row tile
  constexpr int A_PR = BMc / 4, B_PR = BNn / 4;       // float4 per tile row
  // double-buffered tiles: tile t+1 is written to LDS in the middle of tile t's MFMAs (one barrier per tile)
  __shared__ __attribute__((aligned(16))) float As2[2][32 * BMc];
  __shared__ __attribute__((aligned(16))) float Bs2[2][32 * BNn];
  __shared__ int rowtab[2][3][32];

  const int tid = threadIdx.x;
  // (an XCD-contiguous work order was measured here and was slower for the 256-channel layers: 530 vs 465 us)
  const int tiles = p.co_tiles * p.nn_tiles;
  const int split = blockIdx.x / tiles, tile = blockIdx.x - split * tiles;
  const int ct = tile % p.co_tiles, nt = tile / p.co_tiles;
  const int co0 = ct * BMc, nn0 = nt * BNn;
  const int m_begin = split * p.rows_per_split;
  const int m_end = min(p.M, m_begin + p.rows_per_split);
  const int ntiles = (m_end - m_begin + 31) / 32;

  const int wave = tid >> 6, lane = tid & 63;
  const bool active = wave < WM * WN;   // small tiles use fewer than 4 MFMA waves
  const int wm = wave / WN, wn = wave % WN;
  const int lr = lane & 31, lh = lane >> 5;
  const bool cd_vec = (p.Cd & 3) == 0;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  f32x4 a_reg[A_IT], b_reg[B_IT];
  u32x2 a16[A_IT], b16[B_IT];          // IO16: the staged pieces are 4 bf16 values
  float a_msk[A_IT], b_msk[B_IT];      // 0 / 1 per staged float4, applied when the tile is written to LDS (keeps the loads in flight)
#pragma unroll
  for (int i = 0; i < A_IT; ++i) a_msk[i] = 1.f;
#pragma unroll
  for (int i = 0; i < B_IT; ++i) b_msk[i] = 1.f;

  auto fill_rowtab = [&](int t) {     // decode the 32 pixels of tile t (tid < 32 only)
    const int m = m_begin + t * 32 + tid;
    int n = 0, y0 = -(1 << 28), x0 = -(1 << 28);
    if (m < m_end) {
      n = m / (p.Hg * p.Wg);
      int rem = m - n * (p.Hg * p.Wg);
      int a = rem / p.Wg, b = rem - a * p.Wg;
      y0 = a * p.stride - p.pad; x0 = b * p.stride - p.pad;
    }
    rowtab[t & 1][0][tid] = n; rowtab[t & 1][1][tid] = y0; rowtab[t & 1][2][tid] = x0;
  };

  auto gather = [&](int buf, int r, int ty, int tx, bool& ok) -> size_t {
    int y = rowtab[buf][1][r] + ty, x = rowtab[buf][2][r] + tx;
    if (p.reflect) {
      if (y < 0) y = -y;
      if (y >= p.Hi) y = 2 * p.Hi - 2 - y;
      if (x < 0) x = -x;
      if (x >= p.Wi) x = 2 * p.Wi - 2 - x;
    }
    ok = (unsigned)y < (unsigned)p.Hi && (unsigned)x < (unsigned)p.Wi;
    return ((size_t)(rowtab[buf][0][r] * p.Hi + y) * p.Wi + x) * p.Cs;
  };

  // ---- ROWS fast path state (wave-uniform) ----
  int rw_n = 0, rw_a = 0, rw_b = 0;            // image, grid row, first grid column of the NEXT tile to load
  int tap_ty = 0, tap_tx = 0, tap_c0 = 0;
  if constexpr (ROWS) {
    const int hw = p.Hg * p.Wg;
    rw_n = m_begin / hw;
    const int rem = m_begin - rw_n * hw;
    rw_a = rem / p.Wg;
    rw_b = rem - rw_a * p.Wg;
    const int tp = nn0 / p.Cs;
    tap_c0 = nn0 - tp * p.Cs;
    tap_ty = tp / p.kw;
    tap_tx = tp - tap_ty * p.kw;
  }

  // generic-path column decode (K-invariant): columns nn0 + (tid % B_PR)*4 + e
  int gq_ty[4] = {0, 0, 0, 0}, gq_tx[4] = {0, 0, 0, 0}, gq_off[4] = {0, 0, 0, 0};
  bool gq_ok[4] = {false, false, false, false};
  if constexpr (!VEC) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int nn = nn0 + (tid % B_PR) * 4 + e;
      gq_ok[e] = nn < p.NN;
      const int tp = gq_ok[e] ? nn / p.Cs : 0, c = gq_ok[e] ? nn - tp * p.Cs : 0;
      gq_ty[e] = tp / p.kw;
      gq_tx[e] = tp - gq_ty[e] * p.kw;
      gq_off[e] = (gq_ty[e] * p.Wi + gq_tx[e]) * p.Cs + c;
    }
  }

  auto load_tile_rows = [&](int t) {
    const int mb = m_begin + t * 32;
    // A': 32 dense rows of dy starting at row mb (all valid: m_end - m_begin is a multiple of 32 on this path)
    const float* abase = p.dy + (size_t)mb * p.Cd + co0;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const int idx = tid + NT * i;
      const int r = idx / A_PR, c4 = idx - r * A_PR;
      const bool ok = co0 + c4 * 4 < p.Cd;      // unconditional load, masked at the LDS store (see load_tile)
      a_reg[i] = *reinterpret_cast<const f32x4*>(ok ? abase + (size_t)r * p.Cd + c4 * 4 : p.dy);
      a_msk[i] = ok ? 1.f : 0.f;
    }
    // B': source row y is uniform for the tile; x = (b0 + r)*stride - pad + tx varies with the thread's row
    int y = rw_a * p.stride - p.pad + tap_ty;
    if (p.reflect) {
      y = y < 0 ? -y : y;
      y = y >= p.Hi ? 2 * p.Hi - 2 - y : y;
    }
    const bool yok = (unsigned)y < (unsigned)p.Hi;
    const float* bbase = p.x + ((size_t)(rw_n * p.Hi + (yok ? y : 0)) * p.Wi) * p.Cs + tap_c0;
    const int x0 = rw_b * p.stride - p.pad + tap_tx;
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      const int idx = tid + NT * i;
      const int r = idx / B_PR, c4 = idx - r * B_PR;
      int x = x0 + r * p.stride;
      if (p.reflect) {
        x = x < 0 ? -x : x;
        x = x >= p.Wi ? 2 * p.Wi - 2 - x : x;
      }
      const bool ok = yok && (unsigned)x < (unsigned)p.Wi;
      b_reg[i] = *reinterpret_cast<const f32x4*>(bbase + (size_t)(ok ? x : 0) * p.Cs + c4 * 4);
      b_msk[i] = ok ? 1.f : 0.f;        // applied when the tile is written to LDS (keeps the load in flight)
    }
    rw_b += 32;                                  // next tile: same image row, or wrap (Wg % 32 == 0)
    const int wb = rw_b == p.Wg;
    rw_b = wb ? 0 : rw_b;
    rw_a += wb;
    const int wa = rw_a == p.Hg;
    rw_a = wa ? 0 : rw_a;
    rw_n += wa;
  };

  auto load_tile = [&](int t) {
    if constexpr (ROWS) { load_tile_rows(t); return; }
    const int mb = m_begin + t * 32, buf = t & 1;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const int idx = tid + NT * i;
      const int r = idx / A_PR, c4 = idx - r * A_PR;
      const int m = mb + r, co = co0 + c4 * 4;
      if (cd_vec) {
        // UNCONDITIONAL load from a clamped (always valid) address, masked at the LDS store: a load under a branch whose result is
        // merged with zeros makes the compiler wait for every load in turn (round 4: ~6 us per tile against 2 us of MFMAs)
        const bool ok = m < m_end && co < p.Cd;
        if constexpr (IO16) {
          const u32x2 t = *reinterpret_cast<const u32x2*>(reinterpret_cast<const __bf16*>(p.dy) + (ok ? (size_t)m * p.Cd + co : (size_t)0));
          a16[i] = t;
        } else {
          a_reg[i] = *reinterpret_cast<const f32x4*>(p.dy + (ok ? (size_t)m * p.Cd + co : (size_t)0));
        }
        a_msk[i] = ok ? 1.f : 0.f;
      } else {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (m < m_end) {
          const float* src = p.dy + (size_t)m * p.Cd + co;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (co + e < p.Cd) v[e] = src[e];
        }
        a_reg[i] = v;
      }
    }
    if constexpr (VEC) {
      const int tp = nn0 / p.Cs, c0 = nn0 - tp * p.Cs;
      const int ty = tp / p.kw, tx = tp - ty * p.kw;
#pragma unroll
      for (int i = 0; i < B_IT; ++i) {
        const int idx = tid + NT * i;
        const int r = idx / B_PR, c4 = idx - r * B_PR;
        bool ok;
        const size_t off = gather(buf, r, ty, tx, ok);
        if constexpr (IO16) {
          const u32x2 t = *reinterpret_cast<const u32x2*>(reinterpret_cast<const __bf16*>(p.x) + (ok ? off + c0 + c4 * 4 : (size_t)0));
          b16[i] = t;
        } else {
          b_reg[i] = *reinterpret_cast<const f32x4*>(p.x + (ok ? off + c0 + c4 * 4 : (size_t)0));      // (see the A operand above)
        }
        b_msk[i] = ok ? 1.f : 0.f;
      }
    } else {
      // generic channel counts: the thread's 4 columns nn = (tap, channel) are the same for every tile -> their
      // tap displacement / element offset were decoded once (gq_*); per tile only the row origin changes
#pragma unroll
      for (int i = 0; i < B_IT; ++i) {
        const int idx = tid + NT * i;
        const int r = idx / B_PR;
        const int y0 = rowtab[buf][1][r], x0 = rowtab[buf][2][r];
        const int lin = ((rowtab[buf][0][r] * p.Hi + y0) * p.Wi + x0) * p.Cs;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          int y = y0 + gq_ty[e], x = x0 + gq_tx[e];
          int off = lin + gq_off[e];
          if (p.reflect) {
            const int yr = y < 0 ? -y : (y >= p.Hi ? 2 * p.Hi - 2 - y : y);
            const int xr = x < 0 ? -x : (x >= p.Wi ? 2 * p.Wi - 2 - x : x);
            off += ((yr - y) * p.Wi + (xr - x)) * p.Cs;
            y = yr; x = xr;
          }
          const bool ok = gq_ok[e] && (unsigned)y < (unsigned)p.Hi && (unsigned)x < (unsigned)p.Wi;
          const float t = p.x[ok ? off : 0];
          v[e] = ok ? t : 0.f;
        }
        b_reg[i] = v;
      }
    }
  };

  constexpr int LDA = BMc + 32, LDB = BNn + 32;      // bf16 row strides (elements)
  auto store_tile = [&](int buf) {
    float* As = As2[buf];
    float* Bs = Bs2[buf];
    if constexpr (BF) {
      unsigned short* Ah = reinterpret_cast<unsigned short*>(As);
      unsigned short* Bh = reinterpret_cast<unsigned short*>(Bs);
#pragma unroll
      for (int i = 0; i < A_IT; ++i) {
        const int idx = tid + NT * i;
        const int r = idx / A_PR, c4 = idx - r * A_PR;
        if constexpr (IO16) {
          const u32x2 z = {0u, 0u};
          *reinterpret_cast<u32x2*>(&Ah[r * LDA + c4 * 4]) = a_msk[i] != 0.f ? a16[i] : z;
        } else {
          *reinterpret_cast<bf16x4*>(&Ah[r * LDA + c4 * 4]) = __builtin_convertvector(a_reg[i] * a_msk[i], bf16x4);
        }
      }
#pragma unroll
      for (int i = 0; i < B_IT; ++i) {
        const int idx = tid + NT * i;
        const int r = idx / B_PR, c4 = idx - r * B_PR;
        if constexpr (IO16) {
          const u32x2 z = {0u, 0u};
          *reinterpret_cast<u32x2*>(&Bh[r * LDB + c4 * 4]) = b_msk[i] != 0.f ? b16[i] : z;
        } else {
          *reinterpret_cast<bf16x4*>(&Bh[r * LDB + c4 * 4]) = __builtin_convertvector(b_reg[i] * b_msk[i], bf16x4);
        }
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < A_IT; ++i) *reinterpret_cast<f32x4*>(&As[(tid + NT * i) * 4]) = a_reg[i] * a_msk[i];
#pragma unroll
    for (int i = 0; i < B_IT; ++i) *reinterpret_cast<f32x4*>(&Bs[(tid + NT * i) * 4]) = b_reg[i] * b_msk[i];
  };
  auto mfma_range = [&](int buf, int kp0, int kp1) {
    const float* As = As2[buf];
    const float* Bs = Bs2[buf];
    float af[2][TM], bf[2][TN];          // fragments of step kp+1 are read before the MFMAs of step kp
    auto read = [&](int kp, int slot) {
#pragma unroll
      for (int i = 0; i < TM; ++i) af[slot][i] = As[(2 * kp + lh) * BMc + wm * TM * 32 + i * 32 + lr];
#pragma unroll
      for (int j = 0; j < TN; ++j) bf[slot][j] = Bs[(2 * kp + lh) * BNn + wn * TN * 32 + j * 32 + lr];
    };
    read(kp0, 0);
#pragma unroll
    for (int kp = kp0; kp < kp1; ++kp) {
      const int slot = (kp - kp0) & 1;
      if (kp + 1 < kp1) read(kp + 1, slot ^ 1);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[slot][i], bf[slot][j], acc[i][j], 0, 0, 0);
    }
  };

  // bf16: the 2 x 16-pixel K steps of a tile; lane = (channel lr, pixel half lh), group of 16 lanes = one transposed block
  auto mfma_bf16 = [&](int buf) {
    typedef bf16x4 __attribute__((address_space(3))) * lds_bf16x4;
    const unsigned short* Ah = reinterpret_cast<const unsigned short*>(As2[buf]);
    const unsigned short* Bh = reinterpret_cast<const unsigned short*>(Bs2[buf]);
    const int li = lane & 15, q = li >> 2, pq = li & 3, g1 = (lane >> 4) & 1;
    bf16x8 af[2][TM], bfr[2][TN];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int px = 16 * s + 8 * lh + q;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const unsigned short* a0 = &Ah[px * LDA + wm * TM * 32 + i * 32 + 16 * g1 + 4 * pq];
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4)a0);
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4)(a0 + 4 * LDA));
        af[s][i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const unsigned short* b0 = &Bh[px * LDB + wn * TN * 32 + j * 32 + 16 * g1 + 4 * pq];
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4)b0);
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4)(b0 + 4 * LDB));
        bfr[s][j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s][i], bfr[s][j], acc[i][j], 0, 0, 0);
  };

  if (ntiles > 0) {
    if (!ROWS && tid < 32) fill_rowtab(0);
    __syncthreads();
    load_tile(0);
    if (!ROWS && ntiles > 1 && tid < 32) fill_rowtab(1);
    store_tile(0);
    __syncthreads();                    // tile 0 in LDS, rowtab[1] visible
    if (ntiles > 1) load_tile(1);
  }
  if constexpr (BF) {
    // the transposing read needs EXEC all ones: every wave executes it (idle waves of small tiles read valid addresses
    // and discard), no lane-dependent branch around it
    for (int t = 0; t < ntiles; ++t) {
      const int cur = t & 1;
      if (t + 1 < ntiles) store_tile(cur ^ 1);
      if (!ROWS && t + 2 < ntiles && tid < 32) fill_rowtab(t + 2);
      if (active) mfma_bf16(cur);
      __syncthreads();
      if (t + 2 < ntiles) load_tile(t + 2);
    }
  } else
  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    if (active) mfma_range(cur, 0, 8);
    if (t + 1 < ntiles) store_tile(cur ^ 1);               // tile t+1: its loads were issued half a tile ago
    if (!ROWS && t + 2 < ntiles && tid < 32) fill_rowtab(t + 2);   // into rowtab[cur]: tile t's rows are no longer needed
    if (active) mfma_range(cur, 8, 16);
    __syncthreads();                    // tile t+1 and rowtab[cur] visible; everyone is done reading tile t
    if (t + 2 < ntiles) load_tile(t + 2);                  // in flight during the first half of tile t+1
  }

  if (!active) return;
  float* slab = p.slab + (size_t)split * p.Cdpad * p.NNpad;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int nn = nn0 + wn * TN * 32 + j * 32 + lr;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int co = co0 + wm * TM * 32 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        slab[(size_t)co * p.NNpad + nn] = acc[i][j][e];
      }
  }
}

struct WgradReduceParams {
  const float* slab;
  float* dw;
  long long sO, sI, sH, sW;
  int O, I, kh, kw, splits, Cdpad, NNpad;
  int accumulate;      // 1: dw += the slab sum (a second use of the same weight in one backward pass: srgan_set_wgrad_accumulate)
};

// Workgroup = one output channel x 64 input channels x all taps: the slab row is read in its own order ([tap][i]: runs of 64
// floats), summed over the splits in split order, transposed in LDS and written in dW's order ([i][tap]: one contiguous run for
// the standard weight layout).  Round 3: the first version walked a flat 64-bit index (three 64-bit divisions per output, every
// store 36 bytes from its neighbour's) and ran at a sixth of the memory rate -- 145 launches, 1.7 ms of the step.
constexpr int kReduceIC = 64, kReduceMaxTaps = 64;      // (validate: at most 64 taps)

__device__ __forceinline__ int reduce_row_blocks(const WgradReduceParams& p) { return p.O * ((p.I + kReduceIC - 1) / kReduceIC); }

__device__ __forceinline__ void reduce_row_block(const WgradReduceParams& p, int blk, float* sm) {
  const int ichunks = (p.I + kReduceIC - 1) / kReduceIC;
  const int o = blk / ichunks, i0 = (blk - o * ichunks) * kReduceIC;
  const int ic = min(kReduceIC, p.I - i0), taps = p.kh * p.kw, n = ic * taps;
  const size_t slab_stride = (size_t)p.Cdpad * p.NNpad;
  const float* row = p.slab + (size_t)o * p.NNpad + i0;
  if (((p.I | p.NNpad | ic) & 3) == 0 && (slab_stride & 3) == 0) {
    // 16 bytes per lane and four splits in flight: with one dword load per wave between dependent adds the sums ran at the
    // round-trip latency (1.7 TB/s over the step's 2.4 GB of slabs)
    const int icq = ic >> 2, nq = icq * taps;
    for (int e = threadIdx.x; e < nq; e += blockDim.x) {
      const int tap = e / icq, il = (e - tap * icq) * 4;
      const float* src = row + tap * p.I + il;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      int s = 0;
      for (; s + 4 <= p.splits; s += 4) {
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(src + (size_t)s * slab_stride);
        const f32x4 a1 = *reinterpret_cast<const f32x4*>(src + (size_t)(s + 1) * slab_stride);
        const f32x4 a2 = *reinterpret_cast<const f32x4*>(src + (size_t)(s + 2) * slab_stride);
        const f32x4 a3 = *reinterpret_cast<const f32x4*>(src + (size_t)(s + 3) * slab_stride);
        v += a0; v += a1; v += a2; v += a3;             // split order, one rounding per addition, as the scalar loop
      }
      for (; s < p.splits; ++s) v += *reinterpret_cast<const f32x4*>(src + (size_t)s * slab_stride);
#pragma unroll
      for (int c = 0; c < 4; ++c) sm[(il + c) * taps + tap] = v[c];
    }
  } else {
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
      const int tap = e / ic, il = e - tap * ic;
      const float* src = row + tap * p.I + il;
      float v = 0.f;
      for (int s = 0; s < p.splits; ++s) v += src[s * slab_stride];
      sm[il * taps + tap] = v;
    }
  }
  __syncthreads();
  float* dst0 = p.dw + o * p.sO;
  for (int w = threadIdx.x; w < n; w += blockDim.x) {
    const int il = w / taps, tap = w - il * taps;
    const int ky = tap / p.kw, kx = tap - ky * p.kw;
    float* dst = dst0 + ((i0 + il) * p.sI + ky * p.sH + kx * p.sW);
    *dst = p.accumulate ? *dst + sm[w] : sm[w];
  }
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(WgradReduceParams p) {
  __shared__ float sm[kReduceIC * kReduceMaxTaps];
  reduce_row_block(p, blockIdx.x, sm);
}

// many slabs, few outputs (first-layer weights: 64x3x4x4 summed over 1024 pixel ranges; the discriminator heads): workgroup =
// 64 consecutive elements of one slab row x 4 waves; wave w sums splits w, w + 4, ... (eight 256-byte loads in flight), the
// four partial sums meet in LDS and are added in wave order: fixed order, deterministic.  (Round 3; before, one wave per output
// with the lanes striding over the splits: every load touched 64 different lines for 4 bytes each.)
__device__ __forceinline__ int reduce_col_blocks(const WgradReduceParams& p) { return p.O * ((p.kh * p.kw * p.I + 63) / 64); }

__device__ __forceinline__ void reduce_col_block(const WgradReduceParams& p, int blk, float* sm) {
  const int nn = p.kh * p.kw * p.I, cols = (nn + 63) / 64;
  const int o = blk / cols, e = (blk - o * cols) * 64 + (threadIdx.x & 63), wave = threadIdx.x >> 6;
  const size_t slab_stride = (size_t)p.Cdpad * p.NNpad;
  float v = 0.f;
  if (e < nn) {
    const float* src = p.slab + (size_t)o * p.NNpad + e;
    int s = wave;
    for (; s + 28 < p.splits; s += 32) {
      float a[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = src[(size_t)(s + 4 * j) * slab_stride];
#pragma unroll
      for (int j = 0; j < 8; ++j) v += a[j];
    }
    for (; s < p.splits; s += 4) v += src[(size_t)s * slab_stride];
  }
  sm[threadIdx.x] = v;
  __syncthreads();
  if (wave == 0 && e < nn) {
    v = ((sm[threadIdx.x] + sm[threadIdx.x + 64]) + sm[threadIdx.x + 128]) + sm[threadIdx.x + 192];
    const int tap = e / p.I, i = e - tap * p.I;
    const int ky = tap / p.kw, kx = tap - ky * p.kw;
    float* dst = p.dw + (o * p.sO + i * p.sI + ky * p.sH + kx * p.sW);
    *dst = p.accumulate ? *dst + v : v;
  }
}

__global__ __launch_bounds__(256) void wgrad_reduce_wave_kernel(WgradReduceParams p) {
  __shared__ float sm[256];
  reduce_col_block(p, blockIdx.x, sm);
}

// Many slab sums in one launch (srgan_wgrad_defer_begin: the weight gradients of a whole backward pass leave their slabs in an
// arena and are summed together when the pass ends -- 145 launches of ~12 us per train step, each too small to fill the chip,
// become a handful that run at the memory rate).  The records travel in the kernel arguments (a captured train step replays
// them as they were); a workgroup = one row block (reduce_row_block) or one column block (reduce_col_block) of one record: the
// same code, order and single store as the one-record kernels above: identical bits.
constexpr int kMultiReduceMax = 40;
struct MultiReduceEntry {
  WgradReduceParams r;
  int first_block;     // first workgroup of this record
  int wave;            // 1: column blocks (wgrad_reduce_wave_kernel's rule: many splits, few outputs)
};
struct MultiReduceArgs {
  int n;
  MultiReduceEntry e[kMultiReduceMax];
};

__global__ __launch_bounds__(256) void wgrad_reduce_multi_kernel(MultiReduceArgs a) {
  __shared__ float sm[kReduceIC * kReduceMaxTaps];
  int k = 0;
  while (k + 1 < a.n && (int)blockIdx.x >= a.e[k + 1].first_block) ++k;
  const WgradReduceParams& p = a.e[k].r;
  const int blk = blockIdx.x - a.e[k].first_block;
  if (a.e[k].wave) reduce_col_block(p, blk, sm);
  else reduce_row_block(p, blk, sm);
}

// column sums of a dense [M][C] matrix -> out[C] (bias gradients); two-stage, deterministic.
__global__ void colsum_partial_kernel(const float* a, float* part, int M, int C, int rows_per_block) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const int m0 = blockIdx.y * rows_per_block, m1 = min(M, m0 + rows_per_block);
  float s = 0.f;
  for (int m = m0; m < m1; ++m) s += a[(size_t)m * C + c];
  part[(size_t)blockIdx.y * C + c] = s;
}
// one WAVE per column: lane l sums partials l, l + 64, ... (fixed assignment), then a shuffle tree -- deterministic, and the
// up-to-1024 partials no longer sit in one thread's serial chain (18 us per launch, 25 launches per step)
__global__ __launch_bounds__(256) void colsum_final_kernel(const float* part, float* out, int C, int nparts, int accumulate) {
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (c >= C) return;
  float s = 0.f;
  for (int i = lane; i < nparts; i += 64) s += part[(size_t)i * C + c];
  s = wave_sum(s);
  if (lane == 0) out[c] = accumulate ? out[c] + s : s;
}

// at most four columns (the discriminator's PatchGAN and class heads: the only biased convolutions of a train step): one
// workgroup, thread t sums rows t, t + 256, ... of every column, the 256 partial sums meet in LDS and are added in thread order
// -- one launch instead of the partial + final pair (25 pairs per step)
__global__ __launch_bounds__(256) void colsum_narrow_kernel(const float* __restrict__ a, float* __restrict__ out, int M, int C,
                                                            int accumulate) {
  __shared__ float sh[4][256];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int m = threadIdx.x; m < M; m += 256)
    for (int c = 0; c < C; ++c) s[c] += a[(size_t)m * C + c];
  for (int c = 0; c < C; ++c) sh[c][threadIdx.x] = s[c];
  __syncthreads();
  if (threadIdx.x < C) {
    float t = 0.f;
    for (int i = 0; i < 256; ++i) t += sh[threadIdx.x][i];
    out[threadIdx.x] = accumulate ? out[threadIdx.x] + t : t;
  }
}

// ---- host side ----------------------------------------------------------------------------
// the instantiation that serves a (tile, vec, rows) choice
struct WgradVariant { void (*fn)(WgradParams); int threads; };

template <int BMc, int BNn, int WM, int WN>
static WgradVariant wgrad_variant(bool vec, bool rows, bool io16 = false) {
  constexpr int NT = (WM * WN > 4 ? WM * WN : 4) * 64;
  if constexpr (BMc >= 64 && BNn >= 64) {
    if (io16) return {wgrad_kernel<BMc, BNn, WM, WN, true, false, true, true>, NT};      // (wgrad_io16_ok: vec, not rows, bf16 mode)
  }
  if constexpr (BMc >= 64 && BNn >= 64) {
    if (vec && rows && compute_bf16()) return {wgrad_kernel<BMc, BNn, WM, WN, true, true, true>, NT};
    if (vec && rows) return {wgrad_kernel<BMc, BNn, WM, WN, true, true>, NT};
  }
  if (vec && compute_bf16()) return {wgrad_kernel<BMc, BNn, WM, WN, true, false, true>, NT};
  if (vec) return {wgrad_kernel<BMc, BNn, WM, WN, true>, NT};
  return {wgrad_kernel<BMc, BNn, WM, WN, false>, NT};
}

static bool wgrad_lookup(int BMc, int BNn, bool vec, bool rows, WgradVariant* k, bool io16 = false) {
  if (BMc == 128 && BNn == 128) *k = wgrad_variant<128, 128, 2, 2>(vec, rows, io16);
  else if (BMc == 128 && BNn == 64) *k = wgrad_variant<128, 64, 2, 2>(vec, rows, io16);
  else if (BMc == 128 && BNn == 32) *k = wgrad_variant<128, 32, 4, 1>(vec, rows);
  else if (BMc == 64 && BNn == 128) *k = wgrad_variant<64, 128, 2, 2>(vec, rows, io16);
  else if (BMc == 64 && BNn == 64) *k = wgrad_variant<64, 64, 2, 2>(vec, rows, io16);
  else if (BMc == 64 && BNn == 32) *k = wgrad_variant<64, 32, 2, 1>(vec, rows);
  else if (BMc == 32 && BNn == 128) *k = wgrad_variant<32, 128, 1, 4>(vec, rows);
  else if (BMc == 32 && BNn == 64) *k = wgrad_variant<32, 64, 1, 2>(vec, rows);
  else if (BMc == 32 && BNn == 32) *k = wgrad_variant<32, 32, 1, 1>(vec, rows);
  else return false;
  return true;
}

// Workgroups of a weight-gradient variant the whole device holds at once (one "round" of the grid).  The split count is
// chosen so that the grid is a whole number of rounds: a grid of 2.04 rounds costs three (measured: 1044 blocks on 512
// slots ran 409 us where 1008 blocks need 373 us).  Falls back to the LDS bound when no device is present (the
// workspace query is a host-only call).
static long long wgrad_round_slots(const WgradPlan& w) {
  static std::mutex mu;
  static std::map<int, long long> cache;
  const int key = (w.BMc << 16) | (w.BNn << 4) | (compute_bf16() ? 4 : 0) | (w.vec ? 2 : 0) | (w.rows ? 1 : 0);
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int per_cu = 0, cus = 0, dev = 0;
  WgradVariant k{};
  if (wgrad_lookup(w.BMc, w.BNn, w.vec, w.rows, &k) && hipGetDevice(&dev) == hipSuccess &&
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.fn, k.threads, 0) == hipSuccess && per_cu > 0 && cus > 0) {
    // measured
  } else {
    (void)hipGetLastError();
    cus = 256;
    const int lds = 2 * 32 * (std::max(w.BMc, 64) + std::max(w.BNn, 64)) * 4 + 1024;
    per_cu = std::max(1, std::min(8, 163840 / lds));
  }
  return cache[key] = (long long)per_cu * cus;
}

WgradPlan plan_wgrad(const srgan_conv_desc* d) {
  WgradPlan w;
  const long long M = (long long)d->N * d->Ho * d->Wo;
  const int NN = d->kh * d->kw * d->I;
  // (8-wave 256x128 weight-gradient tiles were measured SLOWER in the train step: 88 vs 98 TFLOP/s, A/B on one device)
  w.BMc = d->O <= 32 ? 32 : (d->O <= 64 ? 64 : 128);
  w.vec = (d->I % 32) == 0;
  if (w.vec) w.BNn = (d->I % 128 == 0) ? 128 : ((d->I % 64 == 0) ? 64 : 32);
  else w.BNn = 64;
  // supported shapes: (128,128) (128,64) (128,32) (64,128) (64,64) (64,32) (32,128) (32,64) (32,32)
  // row-aligned fast path: every 32-pixel tile inside one image row, every split a whole number of tiles
  w.rows = w.vec && (d->Wo % 32) == 0 && (M % 32) == 0 && (d->O % 4) == 0;
  w.co_tiles = (int)ceil_div(d->O, w.BMc);
  w.nn_tiles = (int)ceil_div(NN, w.BNn);
  w.Cdpad = w.co_tiles * w.BMc;
  w.NNpad = w.nn_tiles * w.BNn;
  const long long tiles = (long long)w.co_tiles * w.nn_tiles;
  const long long max_splits = std::max<long long>(1, ceil_div(M, 256));   // at least 8 K-tiles per split
  static const long long wg_target = SRGAN_AB_INT("SRGAN_WGRAD_BLOCKS", 512);
  long long splits;
  {
    // about wg_target blocks, rounded to whole device rounds; among the candidate round counts take the best-filled
    const long long slots = wgrad_round_slots(w);
    const long long r0 = std::max<long long>(1, (wg_target + slots / 2) / slots);
    double best_fill = -1.0;
    splits = 1;
    for (long long r = r0; r <= r0 + 2; ++r) {
      long long s = std::min(std::max<long long>(1, (slots * r) / tiles), max_splits);
      const long long blocks = tiles * s;
      const long long rounds = ceil_div(blocks, slots);
      const double fill = (double)blocks / (double)(rounds * slots);
      if (fill > best_fill + 0.04) { best_fill = fill; splits = s; }
    }
  }
  if (splits > max_splits) splits = max_splits;
  if (splits < 1) splits = 1;
  w.rows_per_split = (int)round_up(ceil_div(M, splits), 32);
  w.splits = (int)ceil_div(M, w.rows_per_split);
  return w;
}

static int launch_wgrad(const WgradParams& p, const WgradPlan& w, hipStream_t st, bool io16 = false) {
  WgradVariant k{};
  if (!wgrad_lookup(w.BMc, w.BNn, w.vec, w.rows, &k, io16)) { set_error("wgrad: unsupported tile %dx%d", w.BMc, w.BNn); return -1; }
  ProfScope scope(w.vec ? PROF_WGRAD_VEC : PROF_WGRAD_GEN, 2.0 * p.M * (double)p.Cd * p.NN, st);
  dim3 grid((unsigned)(w.co_tiles * w.nn_tiles * w.splits), 1, 1);
  hipLaunchKernelGGL(k.fn, grid, dim3(k.threads), 0, st, p);
  return check_launch("wgrad_kernel");
}

// srgan_set_wgrad_accumulate: while on, the weight-gradient entry points of this host thread ADD to dw / dbias
static thread_local int g_wgrad_accumulate = 0;
// bit 1 of the same switch: nobody reads dw before srgan_wgrad_defer_end (the caller's gradient sink) -- the call may be deferred
static thread_local int g_wgrad_deferrable = 0;

// srgan_wgrad_defer_begin .. _end (process-wide: autograd runs the backward functions on its own device thread, not on the thread
// that opened the scope; one backward pass at a time, g_defer_mutex only keeps a misuse from corrupting the queue):
// deferrable weight-gradient calls take their workspace (slab first) from the arena
// instead of the caller's shared scratch and queue their slab sum; the queue is launched as wgrad_reduce_multi_kernel when it
// is full, when the arena is, when a second record for the same dw arrives (stream order then keeps the two sums in call
// order), and at _end.
struct WgradDefer {
  bool active = false;
  char* arena = nullptr;
  size_t bytes = 0, used = 0;
  size_t asked = 0;         // workspace bytes the deferrable calls of the scope asked for (srgan_wgrad_defer_need)
  hipStream_t st = nullptr;
  std::vector<MultiReduceEntry> pending;
};
static WgradDefer g_defer;
static std::mutex g_defer_mutex;
static long long g_defer_sums = 0, g_defer_launches = 0;      // srgan_wgrad_defer_stats
static thread_local bool g_call_deferred = false;

static bool reduce_by_wave(const WgradReduceParams& r) {
  return r.splits >= 64 && (long long)r.O * r.kh * r.kw * r.I <= 131072;
}
static long long reduce_row_blocks_host(const WgradReduceParams& r) { return (long long)r.O * ceil_div(r.I, kReduceIC); }
static long long reduce_col_blocks_host(const WgradReduceParams& r) { return (long long)r.O * ceil_div((long long)r.kh * r.kw * r.I, 64); }

static int defer_launch_pending(bool reset_arena) {
  WgradDefer& q = g_defer;
  if (!q.pending.empty()) {
    MultiReduceArgs a{};
    a.n = (int)q.pending.size();
    long long blocks = 0;
    for (int k = 0; k < a.n; ++k) {
      a.e[k] = q.pending[k];
      a.e[k].first_block = (int)blocks;
      blocks += a.e[k].wave ? reduce_col_blocks_host(a.e[k].r) : reduce_row_blocks_host(a.e[k].r);
    }
    q.pending.clear();
    static const bool dbg = std::getenv("SRGAN_DEBUG_REDUCE") != nullptr;
    if (dbg) {
      double bytes = 0;
      for (int k = 0; k < a.n; ++k) {
        const WgradReduceParams& r = a.e[k].r;
        bytes += 4.0 * r.O * r.kh * r.kw * r.I * (r.splits + 1 + r.accumulate);
        std::fprintf(stderr, "  sum O %d I %d k %dx%d splits %d Cdpad %d NNpad %d wave %d acc %d\n", r.O, r.I, r.kh, r.kw, r.splits, r.Cdpad,
                     r.NNpad, a.e[k].wave, r.accumulate);
      }
      std::fprintf(stderr, "multi launch: %d sums, %lld blocks, %.1f MB\n", a.n, blocks, bytes / 1e6);
    }
    g_defer_sums += a.n;
    ++g_defer_launches;
    SRGAN_REQUIRE(blocks < (1LL << 31), "wgrad defer: grid too large");
    hipLaunchKernelGGL(wgrad_reduce_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, q.st, a);
    if (int e = check_launch("wgrad_reduce_multi_kernel")) return e;
  }
  if (reset_arena) q.used = 0;
  return 0;
}

// Called first by every weight-gradient entry point: when the call can be deferred, *ws / *ws_bytes become a fresh piece of the arena
static int defer_take(const srgan_conv_desc* d, void** ws, size_t* ws_bytes, hipStream_t st) {
  g_call_deferred = false;
  if (!g_wgrad_deferrable) return 0;
  std::lock_guard<std::mutex> lock(g_defer_mutex);
  WgradDefer& q = g_defer;
  if (!q.active) return 0;
  if (st != q.st) return 0;          // a call on another stream (the discriminator's second scale): immediate sum, own scratch
  const size_t need = (size_t)round_up((long long)srgan_conv2d_workspace(d), 256);
  q.asked += need;
  if (need == 0 || need > q.bytes) return 0;
  if (q.used + need > q.bytes)
    if (int e = defer_launch_pending(true)) return e;
  *ws = q.arena + q.used;
  *ws_bytes = need;
  q.used += need;
  g_call_deferred = true;
  return 0;
}

// slab sum -> dW (through the weight strides) and optional bias column sums
static int finish_wgrad(const srgan_conv_desc* d, const WgradPlan& w, const float* dy, float* dw, float* dbias, void* ws,
                        hipStream_t st) {
  WgradReduceParams r{};
  r.slab = (const float*)ws; r.dw = dw; r.sO = d->sO; r.sI = d->sI; r.sH = d->sH; r.sW = d->sW;
  r.O = d->O; r.I = d->I; r.kh = d->kh; r.kw = d->kw; r.splits = w.splits; r.Cdpad = w.Cdpad; r.NNpad = w.NNpad;
  r.accumulate = g_wgrad_accumulate;
  long long total = (long long)d->O * d->kh * d->kw * d->I;
  if (g_call_deferred) {
    g_call_deferred = false;
    std::lock_guard<std::mutex> lock(g_defer_mutex);
    WgradDefer& q = g_defer;
    bool again = false;
    for (const MultiReduceEntry& e : q.pending) again = again || e.r.dw == dw;
    if (again || (int)q.pending.size() == kMultiReduceMax)
      if (int e = defer_launch_pending(false)) return e;
    MultiReduceEntry me{};
    me.r = r;
    me.wave = reduce_by_wave(r) ? 1 : 0;
    q.pending.push_back(me);
  } else if (reduce_by_wave(r))
    hipLaunchKernelGGL(wgrad_reduce_wave_kernel, dim3((unsigned)reduce_col_blocks_host(r)), dim3(256), 0, st, r);
  else
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)reduce_row_blocks_host(r)), dim3(256), 0, st, r);
  if (int e2 = check_launch("wgrad_reduce_kernel")) return e2;
  (void)total;
  if (dbias) {
    const int M = d->N * d->Ho * d->Wo;
    if (d->O <= 4 && M <= (1 << 16)) {
      hipLaunchKernelGGL(colsum_narrow_kernel, dim3(1), dim3(256), 0, st, dy, dbias, M, d->O, g_wgrad_accumulate);
      return check_launch("colsum_narrow_kernel");
    }
    float* part = (float*)ws + (size_t)w.splits * w.Cdpad * w.NNpad;
    int nparts = (int)std::min<long long>(1024, ceil_div(M, 64));
    int rpb = (int)ceil_div(M, nparts);
    nparts = (int)ceil_div(M, rpb);
    dim3 g1((unsigned)ceil_div(d->O, 64), (unsigned)nparts);
    hipLaunchKernelGGL(colsum_partial_kernel, g1, dim3(64), 0, st, dy, part, M, d->O, rpb);
    if (int e3 = check_launch("colsum_partial_kernel")) return e3;
    hipLaunchKernelGGL(colsum_final_kernel, dim3((unsigned)ceil_div(d->O, 4)), dim3(256), 0, st, (const float*)part, dbias, d->O, nparts,
                       g_wgrad_accumulate);
    return check_launch("colsum_final_kernel");
  }
  return 0;
}

// the implicit-GEMM weight gradient (wgrad_kernel + slab sum); io16: x and dy are bf16 tensors (igemm16_io_ok layers)
static int generic_wgrad(const srgan_conv_desc* d, const WgradPlan& w, const float* x, const float* dy, float* dw, float* dbias,
                         void* ws, hipStream_t st, bool io16) {
  WgradParams p{};
  p.x = x; p.dy = dy; p.slab = (float*)ws;
  p.NB = d->N; p.Hi = d->Hi; p.Wi = d->Wi; p.Cs = d->I; p.Hg = d->Ho; p.Wg = d->Wo; p.Cd = d->O;
  p.stride = d->stride; p.pad = d->pad; p.kw = d->kw; p.reflect = d->pad_mode == SRGAN_PAD_REFLECT;
  p.NN = d->kh * d->kw * d->I; p.NNpad = w.NNpad; p.Cdpad = w.Cdpad;
  p.M = d->N * d->Ho * d->Wo; p.rows_per_split = w.rows_per_split;
  p.co_tiles = w.co_tiles; p.nn_tiles = w.nn_tiles;
  if (int e = launch_wgrad(p, w, st, io16)) return e;
  return finish_wgrad(d, w, io16 ? nullptr : dy, dw, dbias, ws, st);
}
}  // namespace srgan

using namespace srgan;

extern "C" int srgan_conv2d_wgrad(const srgan_conv_desc* d, const float* x, const float* dy, float* dw,
                                  float* dbias, void* ws, size_t ws_bytes, void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(x && dy && dw && ws, "conv2d_wgrad: null pointer");
  SRGAN_REQUIRE(ws_bytes >= srgan_conv2d_workspace(d), "conv2d_wgrad: workspace too small");
  hipStream_t st = as_stream(stream);
  if (int e = defer_take(d, &ws, &ws_bytes, st)) return e;
  WgradPlan w = plan_wgrad(d);
  if (wino_wgrad_applicable(d)) {
    wino_wgrad_slab(d, &w.splits, &w.Cdpad, &w.NNpad);
    if (int e = wino_wgrad_run(d, x, dy, (float*)ws, st)) return e;
    return finish_wgrad(d, w, dy, dw, dbias, ws, st);
  }
  if (rgb_wgrad_kind(d) >= 0) {
    rgb_wgrad_slab(d, &w.splits, &w.Cdpad, &w.NNpad);
    if (int e = rgb_wgrad_run(d, x, dy, (float*)ws, st)) return e;
    return finish_wgrad(d, w, dy, dw, dbias, ws, st);
  }
  if (narrow_applicable(d)) {
    int n_slabs = 0;
    if (int e = narrow_wgrad(d, x, dy, ws, &n_slabs, st)) return e;
    w.splits = n_slabs; w.Cdpad = 4; w.NNpad = d->kh * d->kw * d->I;
    return finish_wgrad(d, w, dy, dw, dbias, ws, st);
  }
  return generic_wgrad(d, w, x, dy, dw, dbias, ws, st, false);
}

// Weight gradient of a layer whose forward kept its F(4x4,3x3) V image (srgan_conv2d_wgrad_v_bytes(d) != 0 bytes, handed to
// srgan_conv2d_fwd_packed as `ws` and kept alive by the caller instead of the shared scratch).
extern "C" size_t srgan_conv2d_wgrad_v_bytes(const srgan_conv_desc* d) {
  if (conv_validate(d) != 0) return 0;
  Wino43WgradGeom g{};
  return wino43_wgrad_geometry(d, &g) ? g.v_bytes : 0;
}

extern "C" int srgan_conv2d_wgrad_v(const srgan_conv_desc* d, const float* v_image, const float* dy, float* dw, float* dbias,
                                    void* ws, size_t ws_bytes, void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(v_image && dy && dw && ws, "conv2d_wgrad_v: null pointer");
  SRGAN_REQUIRE(ws_bytes >= srgan_conv2d_workspace(d), "conv2d_wgrad_v: workspace too small");
  Wino43WgradGeom g{};
  SRGAN_REQUIRE(wino43_wgrad_geometry(d, &g), "conv2d_wgrad_v: layer not applicable");
  hipStream_t st = as_stream(stream);
  if (int e = defer_take(d, &ws, &ws_bytes, st)) return e;
  const size_t cs = (size_t)1024 * d->O * sizeof(float);
  float* zimg = reinterpret_cast<float*>(static_cast<char*>(ws) + round_up((long long)(g.slab_bytes + cs), 256));
  if (int e = wino43_wgrad_launch(g, v_image, dy, zimg, (float*)ws, conv_flops(d), st)) return e;
  if (int e = check_launch("wino43_wgrad_kernel")) return e;
  WgradPlan w = plan_wgrad(d);
  w.splits = g.splits; w.Cdpad = d->O; w.NNpad = 9 * d->I;
  return finish_wgrad(d, w, dy, dw, dbias, ws, st);
}

// The same with the Z image (A dy A^T) already written by srgan_instnorm_bwd_vz.
extern "C" int srgan_conv2d_wgrad_vz(const srgan_conv_desc* d, const float* v_image, const float* z_image, float* dw, void* ws,
                                     size_t ws_bytes, void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(v_image && z_image && dw && ws, "conv2d_wgrad_vz: null pointer");
  SRGAN_REQUIRE(ws_bytes >= srgan_conv2d_workspace(d), "conv2d_wgrad_vz: workspace too small");
  Wino43WgradGeom g{};
  SRGAN_REQUIRE(wino43_wgrad_geometry(d, &g), "conv2d_wgrad_vz: layer not applicable");
  hipStream_t st = as_stream(stream);
  if (int e = defer_take(d, &ws, &ws_bytes, st)) return e;
  if (int e = wino43_wgrad_launch(g, v_image, nullptr, const_cast<float*>(z_image), (float*)ws, conv_flops(d), st, true)) return e;
  if (int e = check_launch("wino43_wgrad_kernel")) return e;
  WgradPlan w = plan_wgrad(d);
  w.splits = g.splits; w.Cdpad = d->O; w.NNpad = 9 * d->I;
  return finish_wgrad(d, w, nullptr, dw, nullptr, ws, st);
}

// bf16 mode, residual-trunk and stride-2 shapes (conv_halo16.hip) and the 7x7 RGB layers, with bf16 TENSORS on either side
extern "C" int srgan_halo16_wgrad(const srgan_conv_desc* d, const void* x, int x_bf16, const void* dy, int dy_bf16, float* dw,
                                  void* ws, size_t ws_bytes, void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(x && dy && dw && ws, "halo16_wgrad: null pointer");
  // (round 6: also the stride-2 layers no patch kernel serves forward -- the discriminators' 16- and 8-pixel maps,
  //  srgan_conv2d_io_applicable -- whose weight gradient halo16s2_wgrad_kernel takes all the same)
  if (compute_bf16() && rgb_wgrad16_served(d)) {      // round 6: the 7x7 RGB layers, 64-channel side fp32 or bf16
    const int kind = rgb_wgrad_kind(d);
    SRGAN_REQUIRE(kind == 0 ? !x_bf16 : !dy_bf16, "halo16_wgrad: the 3-channel tensor of an RGB layer is fp32");
    SRGAN_REQUIRE(ws_bytes >= srgan_conv2d_workspace(d), "halo16_wgrad: workspace too small (srgan_conv2d_workspace)");
    hipStream_t st = as_stream(stream);
    if (int e = defer_take(d, &ws, &ws_bytes, st)) return e;
    WgradPlan w = plan_wgrad(d);
    rgb_wgrad_slab(d, &w.splits, &w.Cdpad, &w.NNpad);
    if (int e = rgb_wgrad_run(d, x, dy, (float*)ws, st, (kind == 0 ? dy_bf16 : x_bf16) != 0)) return e;
    return finish_wgrad(d, w, nullptr, dw, nullptr, ws, st);
  }
  SRGAN_REQUIRE(compute_bf16() && halo16_wgrad_applicable(d),
                "halo16_wgrad: layer / compute mode not applicable (srgan_halo16_applicable / srgan_halo16s2_applicable / srgan_conv2d_io_applicable)");
  SRGAN_REQUIRE(ws_bytes >= srgan_conv2d_workspace(d), "halo16_wgrad: workspace too small (srgan_conv2d_workspace)");
  hipStream_t st = as_stream(stream);
  if (int e = defer_take(d, &ws, &ws_bytes, st)) return e;
  WgradPlan w = plan_wgrad(d);
  halo16_wgrad_slab(d, &w.splits, &w.Cdpad, &w.NNpad);
  if (int e = halo16_wgrad_run(d, x, dy, (float*)ws, conv_flops(d), st, x_bf16 != 0, dy_bf16 != 0)) return e;
  return finish_wgrad(d, w, nullptr, dw, nullptr, ws, st);
}

// x, dy: bf16 tensors.  Same workspace, gradient sink and deferred slab sum as srgan_conv2d_wgrad.
extern "C" int srgan_igemm16_wgrad(const srgan_conv_desc* d, const void* x, const void* dy, float* dw, void* ws, size_t ws_bytes,
                                   void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(x && dy && dw && ws, "igemm16_wgrad: null pointer");
  SRGAN_REQUIRE(igemm16_io_ok(d, SRGAN_ACT_NONE), "igemm16_wgrad: layer / compute mode not applicable (srgan_igemm16_io_applicable)");
  SRGAN_REQUIRE(ws_bytes >= srgan_conv2d_workspace(d), "igemm16_wgrad: workspace too small (srgan_conv2d_workspace)");
  hipStream_t st = as_stream(stream);
  if (int e = defer_take(d, &ws, &ws_bytes, st)) return e;
  const WgradPlan w = plan_wgrad(d);
  return generic_wgrad(d, w, static_cast<const float*>(x), static_cast<const float*>(dy), dw, nullptr, ws, st, true);
}

// A weight used more than once in one backward pass (the generator runs twice inside util_notebook.py:664 and :689) gets its
// later contributions added by the split-K slab reduce instead of by a separate elementwise pass of the caller.
extern "C" int srgan_set_wgrad_accumulate(int on) {
  srgan::g_wgrad_accumulate = (on & 1) != 0;
  srgan::g_wgrad_deferrable = (on & 2) != 0;
  return 0;
}

extern "C" int srgan_wgrad_defer_begin(void* arena, size_t arena_bytes, void* stream) {
  SRGAN_REQUIRE(arena && arena_bytes >= 4096, "wgrad_defer_begin: null or tiny arena");
  SRGAN_REQUIRE((reinterpret_cast<uintptr_t>(arena) & 255) == 0, "wgrad_defer_begin: the arena must be 256-byte aligned");
  std::lock_guard<std::mutex> lock(srgan::g_defer_mutex);
  SRGAN_REQUIRE(!srgan::g_defer.active, "wgrad_defer_begin: already active");
  srgan::g_defer.active = true;
  srgan::g_defer.arena = static_cast<char*>(arena);
  srgan::g_defer.bytes = arena_bytes & ~(size_t)255;
  srgan::g_defer.used = 0;
  srgan::g_defer.asked = 0;
  srgan::g_defer.st = as_stream(stream);
  srgan::g_defer.pending.clear();
  return 0;
}

extern "C" int srgan_wgrad_defer_stats(long long* sums, long long* launches) {
  SRGAN_REQUIRE(sums && launches, "wgrad_defer_stats: null pointer");
  std::lock_guard<std::mutex> lock(srgan::g_defer_mutex);
  *sums = srgan::g_defer_sums;
  *launches = srgan::g_defer_launches;
  return 0;
}

extern "C" int srgan_wgrad_defer_need(long long* bytes) {
  SRGAN_REQUIRE(bytes, "wgrad_defer_need: null pointer");
  std::lock_guard<std::mutex> lock(srgan::g_defer_mutex);
  *bytes = (long long)srgan::g_defer.asked;
  return 0;
}

extern "C" int srgan_wgrad_defer_end(void) {
  std::lock_guard<std::mutex> lock(srgan::g_defer_mutex);
  if (!srgan::g_defer.active) return 0;
  const int e = srgan::defer_launch_pending(true);
  srgan::g_defer.active = false;
  return e;
}
