// The packed weight operand of a forward / input-gradient convolution: its size, its layout (written by whichever kernel family
// conv_dispatch.hip routes the layer to) and the entries that pack one operand, or every cached operand of a network at once.
#include <algorithm>
#include <cstring>
#include "conv.h"
#include "pack_device.h"

namespace srgan {

// ---- weight repack ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_weights_kernel(PackParams p) {
  if (pack_weights_block_ok(p)) {
    __shared__ float tile[PACK_LDS_FLOATS];
    pack_weights_rows(p, tile);
    return;
  }
  const long long total = pack_weights_total(p);
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x)
    pack_weights_item(p, idx);
}

// every cached operand of a network in one launch: blockIdx.y = entry, blockIdx.x grid-strides over its elements
__global__ __launch_bounds__(256) void pack_multi_kernel(const PackEntry* __restrict__ entries) {
  const PackEntry& e = entries[blockIdx.y];
  __shared__ float tile[PACK_LDS_FLOATS];
  static_assert(PACK_LDS_FLOATS >= 32 * WP43_ROW, "one LDS tile serves both cooperative paths");
  if (e.type == 0) {
    if (pack_weights_block_ok(e.ig)) { pack_weights_rows(e.ig, tile); return; }
    const long long total = pack_weights_total(e.ig);
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x)
      pack_weights_item(e.ig, idx);
  } else if (wino43_pack_block_ok(e.wn)) {
    const long long total = wino_pack_total(e.wn);       // a multiple of 256 (nchunk % 4 == 0)
    for (long long base = (long long)blockIdx.x * 256; base < total; base += (long long)gridDim.x * 256)
      wino43_pack_block(e.wn, base, tile);
  } else {
    const long long total = wino_pack_total(e.wn);
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x)
      wino_pack_item(e.wn, idx);
  }
}

static size_t fwd_packed_bytes(const srgan_conv_desc* d, int act) {
  const FwdPath path = fwd_path(d, act);
  if (path == PATH_NARROW) return (size_t)d->I * d->kh * d->kw * 4 * sizeof(float);
  if (path == PATH_ROWCONV) return rowconv_packed_elems(d) * sizeof(float);
  if (path == PATH_RGBIN) return rgbin_packed_elems(d) * sizeof(float);
  if (path == PATH_WINO) return wino_packed_bytes(d, 0);
  IgemmParams p{};
  fwd_geometry(d, path, p);
  return (size_t)p.Npad * p.Kpad * sizeof(float);
}

static PackParams fwd_pack_params(const srgan_conv_desc* d, FwdPath path, const float* w, float* dst) {
  IgemmParams p{};
  fwd_geometry(d, path, p);
  PackParams q{};
  q.w = w; q.dst = dst; q.sO = d->sO; q.sI = d->sI; q.sH = d->sH; q.sW = d->sW;
  q.O = d->O; q.I = d->I; q.kh = d->kh; q.kw = d->kw; q.mode = 0; q.stride = d->stride; q.pad = d->pad;
  q.Ty = d->kh; q.Tx = d->kw; q.Cs = d->I; q.N = d->O; q.K = p.K; q.Kpad = p.Kpad; q.Npad = p.Npad; q.phases = 1;
  q.out16 = (path == PATH_IGEMM && igemm16_ok(p)) ? 1 : 0;
  q.regimg = (q.out16 && halo16e_ok(p)) ? 1 : 0;
  return q;
}

int fwd_pack(const srgan_conv_desc* d, int act, const float* w, float* dst, hipStream_t st) {
  const FwdPath path = fwd_path(d, act);
  if (path == PATH_NARROW) return narrow_pack(d, w, dst, st);
  if (path == PATH_ROWCONV) return rowconv_pack(d, w, dst, st);
  if (path == PATH_RGBIN) return rgbin_pack(d, w, dst, st);
  if (path == PATH_WINO) return wino_pack(d, 0, w, dst, st);
  const PackParams q = fwd_pack_params(d, path, w, dst);
  long long total = (long long)q.Npad * q.Kpad;
  hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)std::min<long long>(ceil_div(total, 256), 4096)), dim3(256), 0, st, q);
  return check_launch("pack_weights_kernel");
}

static PackParams dgrad_pack_params(const srgan_conv_desc* d, const DgradGeom& g, const float* w, float* dst) {
  PackParams q{};
  q.w = w; q.dst = dst; q.sO = d->sO; q.sI = d->sI; q.sH = d->sH; q.sW = d->sW;
  q.O = d->O; q.I = d->I; q.kh = d->kh; q.kw = d->kw; q.mode = 1; q.stride = d->stride; q.pad = g.p.pad;
  q.Ty = g.p.Ty; q.Tx = g.p.Tx; q.Cs = d->O; q.N = d->I; q.K = g.p.K; q.Kpad = g.p.Kpad; q.Npad = g.p.Npad; q.phases = g.phases;
  q.out16 = (!g.wino && !g.narrow && !g.rgbin && !g.narrow_s2 && igemm16_ok(g.p)) ? 1 : 0;
  q.regimg = (q.out16 && g.phases == 1 && halo16e_ok(g.p)) ? 1 : 0;
  return q;
}

int dgrad_pack(const srgan_conv_desc* d, const float* w, float* dst, hipStream_t st) {
  DgradGeom g = dgrad_geometry(d);
  if (g.wino) return wino_pack(d, 1, w, dst, st);
  if (g.narrow) {
    srgan_conv_desc f;
    long long w_off;
    narrow_dgrad_desc(d, &f, &w_off);
    if (rowconv_applicable(&f)) return rowconv_pack(&f, w + w_off, dst, st);
    return narrow_pack(&f, w + w_off, dst, st);
  }
  if (g.rgbin) {
    srgan_conv_desc f;
    long long w_off;
    rgbin_dgrad_desc(d, &f, &w_off);
    return rgbin_pack(&f, w + w_off, dst, st);
  }
  if (g.narrow_s2) {
    for (int ph = 0; ph < 4; ++ph) {
      srgan_conv_desc f;
      long long w_off;
      int px;
      size_t po;
      if (!narrow_s2_phase(d, ph >> 1, ph & 1, &f, &w_off, &px, &po)) { set_error("narrow stride-2 dgrad: phase geometry"); return -1; }
      if (int e = narrow_pack(&f, w + w_off, dst + po, st)) return e;
    }
    return 0;
  }
  const PackParams q = dgrad_pack_params(d, g, w, dst);
  long long total = (long long)g.packed_elems;
  hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)std::min<long long>(ceil_div(total, 256), 4096)), dim3(256), 0, st, q);
  return check_launch("pack_weights_kernel");
}

size_t pack_bytes(const srgan_conv_desc* d) {
  // fwd pack and dgrad pack upper bounds
  const long long M_f = (long long)d->N * d->Ho * d->Wo;
  const long long Kf = round_up((long long)d->kh * d->kw * d->I, BK);
  const long long f = (long long)npad_for(M_f, d->O) * Kf;
  const int s = d->stride;
  const int Ty = (int)ceil_div(d->kh, s), Tx = (int)ceil_div(d->kw, s);
  const long long Kd = round_up((long long)Ty * Tx * d->O, BK);
  const long long g = (long long)s * s * round_up(d->I, 128) * Kd;
  size_t bytes = (size_t)((f > g ? f : g) * sizeof(float));
  if (rowconv_applicable(d)) bytes = std::max(bytes, rowconv_packed_elems(d) * sizeof(float));
  {
    srgan_conv_desc f;
    long long w_off;
    if (narrow_dgrad_desc(d, &f, &w_off) && rowconv_applicable(&f)) bytes = std::max(bytes, rowconv_packed_elems(&f) * sizeof(float));
  }
  if (wino_applicable(d, 0)) bytes = std::max(bytes, wino_packed_bytes(d, 0));
  if (wino_applicable(d, 1)) bytes = std::max(bytes, wino_packed_bytes(d, 1));
  if (d->I == 3 || d->O == 3) bytes = std::max(bytes, (size_t)d->kh * ((d->kw * 3 + 1) & ~1) * std::max(d->I, d->O) * sizeof(float));   // conv_rgbin.hip
  return bytes;
}

}  // namespace srgan

using namespace srgan;

// ---- packed-weight variants: pack once per optimiser step, reuse across the step's forwards / backwards ----
extern "C" size_t srgan_conv2d_packed_bytes(const srgan_conv_desc* d, int kind, int act) {
  if (conv_validate(d) != 0) return 0;
  return kind == 0 ? fwd_packed_bytes(d, act) : dgrad_geometry(d).packed_elems * sizeof(float);
}

extern "C" int srgan_conv2d_pack(const srgan_conv_desc* d, int kind, int act, const float* w, void* packed, size_t bytes,
                                 void* stream) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(w && packed, "conv2d_pack: null pointer");
  SRGAN_REQUIRE(kind == 0 || kind == 1, "conv2d_pack: kind must be 0 (forward) or 1 (input gradient)");
  SRGAN_REQUIRE(bytes >= srgan_conv2d_packed_bytes(d, kind, act), "conv2d_pack: destination too small");
  return kind == 0 ? fwd_pack(d, act, w, (float*)packed, as_stream(stream)) : dgrad_pack(d, w, (float*)packed, as_stream(stream));
}

// ---- one launch for many packs: the host collects one record per cached operand (srgan_conv2d_pack_entry), copies the
// array to the device and calls srgan_conv2d_pack_multi after the optimiser step that changed those weights ----
extern "C" size_t srgan_pack_entry_bytes(void) { return sizeof(PackEntry); }

// fills `entry` (host memory, srgan_pack_entry_bytes() bytes).  Returns 0, or 1 when this layer's operand is produced by a
// kernel outside the multi-pack launch (narrow-output layers): pack it with srgan_conv2d_pack.
extern "C" int srgan_conv2d_pack_entry(const srgan_conv_desc* d, int kind, int act, const float* w, void* packed, void* entry) {
  if (int e = conv_validate(d)) return e;
  SRGAN_REQUIRE(w && packed && entry, "conv2d_pack_entry: null pointer");
  SRGAN_REQUIRE(kind == 0 || kind == 1, "conv2d_pack_entry: kind must be 0 (forward) or 1 (input gradient)");
  PackEntry pe{};
  if (kind == 0) {
    const FwdPath path = fwd_path(d, act);
    if (path == PATH_NARROW || path == PATH_ROWCONV || path == PATH_RGBIN) return 1;
    if (path == PATH_WINO) { pe.type = 1; wino_pack_params(d, 0, w, (float*)packed, &pe.wn); }
    else { pe.type = 0; pe.ig = fwd_pack_params(d, path, w, (float*)packed); }
  } else {
    const DgradGeom g = dgrad_geometry(d);
    if (g.narrow || g.rgbin || g.narrow_s2) return 1;
    if (g.wino) { pe.type = 1; wino_pack_params(d, 1, w, (float*)packed, &pe.wn); }
    else { pe.type = 0; pe.ig = dgrad_pack_params(d, g, w, (float*)packed); }
  }
  std::memcpy(entry, &pe, sizeof(pe));
  return 0;
}

extern "C" int srgan_conv2d_pack_multi(const void* entries_dev, int n_entries, void* stream) {
  SRGAN_REQUIRE(entries_dev && n_entries > 0, "conv2d_pack_multi: bad argument");
  hipLaunchKernelGGL(pack_multi_kernel, dim3(256, (unsigned)n_entries), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const PackEntry*>(entries_dev));
  return check_launch("pack_multi_kernel");
}

// Non-zero when the packed operand of (d, kind, act) does not depend on the batch size or the map size (the Winograd filter
// images and the RGB-input image depend on the weights and the channel counts only): a caller may then share one packed buffer
// between descriptors that differ in N / H / W only and return the same signature.  0: the layout follows the geometry.
// Round 6: the implicit-GEMM operands too.  Their bytes are a function of the weights and of PackParams' layout fields; two
// descriptors of one weight that differ in N / H / W only often agree in all of them (the discriminators see 64 images in their
// own update and 32 in the generator's, the encoder 32 and 64: every one of their operands was packed -- and re-packed after
// every optimiser step -- twice).  The signature is a hash of those fields (bit 62 set: never one of the small values above).
static unsigned long long pack_layout_signature(const PackParams& q, int kind) {
  static const bool off = SRGAN_AB_SET("SRGAN_NO_PACK_SHARE");
  if (off) return 0;
  unsigned long long h = 1469598103934665603ull;
  const long long f[] = {q.O, q.I, q.kh, q.kw, q.mode, q.stride, q.pad, q.Ty, q.Tx, q.Cs, q.N, q.K, q.Kpad, q.Npad, q.phases, q.out16,
                         q.regimg, kind};
  for (long long v : f)
    for (int b = 0; b < 8; ++b) {
      h ^= (unsigned long long)((v >> (8 * b)) & 0xff);
      h *= 1099511628211ull;
    }
  return (h >> 2) | (1ull << 62);
}

extern "C" unsigned long long srgan_conv2d_pack_signature(const srgan_conv_desc* d, int kind, int act) {
  if (conv_validate(d) != 0) return 0;
  if (kind == 0) {
    const FwdPath path = fwd_path(d, act);
    if (path == PATH_RGBIN) return 100;
    if (path == PATH_WINO) return 10 + (unsigned long long)(wino_packed_bytes(d, 0) % 1000003) * 16 + 1;
    if (path == PATH_NARROW || path == PATH_ROWCONV) return 0;      // (their buffers carry per-geometry scratch behind the filter)
    return pack_layout_signature(fwd_pack_params(d, path, nullptr, nullptr), 0);
  }
  const DgradGeom g = dgrad_geometry(d);
  if (g.rgbin) return 101;
  if (g.wino) return 10 + (unsigned long long)(wino_packed_bytes(d, 1) % 1000003) * 16 + 2;
  if (g.narrow || g.narrow_s2) return 0;
  return pack_layout_signature(dgrad_pack_params(d, g, nullptr, nullptr), 1);
}

extern "C" size_t srgan_conv2d_packed_scratch(const srgan_conv_desc* d, int kind) {
  if (conv_validate(d) != 0) return 0;
  if (kind == 1 && d->pad_mode == SRGAN_PAD_REFLECT) return srgan_conv2d_workspace(d);      // padded-gradient temp (+ split-K slabs)
  if (kind == 0 ? fwd_path(d, SRGAN_ACT_NONE) == PATH_WINO : dgrad_geometry(d).wino) return wino_scratch_bytes(d, kind);
  return conv_splitk_bytes(d, kind);      // implicit-GEMM layers with few pixel tiles: split-K slabs (0 for everything else)
}
