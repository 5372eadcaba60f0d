"""torch.autograd.Function wrappers over the C ABI of libsrgan_hip.so.

PyTorch is used for device memory, streams and the autograd graph only; every forward and
backward computation below is a hand-written gfx950 kernel reached through ctypes.

Layout: 4-D activations are *NHWC-dense* tensors with logical NCHW shape (what PyTorch calls
channels_last), so they interoperate with callers written against the reference's NCHW API.

Stale-graph semantics: convolution / transposed-convolution weights
are kept on the autograd context by reference and read when backward RUNS (torch 1.4 behaviour
the reference's train step relies on, util_notebook.py:664-690); activations, norm statistics
and the CBIN gamma copy are the forward-time values.
"""
import ctypes
import struct
import weakref

import torch
from torch.autograd import Function

from . import _lib
from ._lib import ConvDesc

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
PAD_ZERO, PAD_REFLECT = 0, 1

_workspaces = {}
import os as _os
_DEBUG_FRESH_WS = _lib.ab('SRGAN_DEBUG_FRESH_WS')
_DEBUG_CLONE = _lib.ab('SRGAN_DEBUG_CLONE')


def _require_gpu(t, what):
    if not t.is_cuda:
        raise _lib.SrganHipError(f"{what}: tensor is on {t.device}; srgan_amd runs on the MI355X HIP path only "
                                 "(no CPU fallback)")
    if t.dtype != torch.float32:
        raise _lib.SrganHipError(f"{what}: expected float32, got {t.dtype}")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def workspace(device, nbytes):
    """Cached scratch buffer (per device); grown on demand, reused in stream order."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    if _DEBUG_FRESH_WS:
        return torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes * 1.25), 1 << 22), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


# Streams that carry parts of one backward pass (model._second_scale: the discriminator's second scale runs on a side stream).
# Code that reads gradients from INSIDE the pass -- the eager data-parallel reducer sends a bucket from the hook of its last
# parameter, on whatever stream that parameter's node ran -- first makes its stream wait for the others.
_compute_streams = {}


def register_compute_streams(device, *streams):
    known = _compute_streams.setdefault(device.index, [])
    for s in streams:
        if all(s != k for k in known):
            known.append(s)
        if len(known) > 8:          # callers' streams come and go (tests); keep the recent ones
            del known[0]


def wait_compute_streams(device):
    cur = torch.cuda.current_stream(device)
    for s in _compute_streams.get(device.index, ()):
        if s != cur:
            cur.wait_stream(s)


def upload_small(blob, device, out=None):
    """bytes / bytearray (a pointer table of a few KB, multiple of 4 bytes) -> device uint8 tensor.  The bytes travel in the
    arguments of a tiny kernel (C ABI ``srgan_upload_small``): no pinned staging buffer to keep alive, and inside a captured
    hipGraph the node stores the bytes, so a replay rewrites the same table instead of re-reading a host address."""
    n = len(blob)
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=device)
    elif out.numel() < n:
        raise _lib.SrganHipError("upload_small: destination too small")
    buf = (ctypes.c_char * n).from_buffer_copy(bytes(blob))
    _lib.check(_lib.load().srgan_upload_small(_ptr(out), ctypes.byref(buf), n, _stream()), "upload_small")
    return out


def nhwc_empty(n, c, h, w, device, dtype=torch.float32):
    return torch.empty((n, h, w, c), dtype=dtype, device=device).permute(0, 3, 1, 2)


def is_nhwc_dense(t):
    return t.dim() == 4 and t.permute(0, 2, 3, 1).is_contiguous()


def to_nhwc(t):
    """Return an NHWC-dense tensor with the same logical NCHW shape/values (HIP repack kernel)."""
    if t.dim() != 4:
        raise ValueError('expected 4D input (got {}D input)'.format(t.dim()))
    if t.dtype == torch.bfloat16 and t.is_cuda and is_nhwc_dense(t):      # a 16-bit activation of the bf16 mode (already dense)
        return t
    _require_gpu(t, "to_nhwc")
    if is_nhwc_dense(t):
        return t
    if t.dtype != torch.float32:
        raise _lib.SrganHipError(f"to_nhwc: a {t.dtype} tensor must already be NHWC-dense (the repack kernel is fp32)")
    t = t.contiguous()
    n, c, h, w = t.shape
    out = nhwc_empty(n, c, h, w, t.device)
    _lib.check(_lib.load().srgan_nchw_to_nhwc(_ptr(t), _ptr(out), n, c, h, w, _stream()), "nchw_to_nhwc")
    return out


def to_nchw(t):
    """NCHW-contiguous copy of an NHWC-dense tensor (HIP repack kernel)."""
    _require_gpu(t, "to_nchw")
    if t.is_contiguous():
        return t
    t = to_nhwc(t)
    n, c, h, w = t.shape
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=t.device)
    _lib.check(_lib.load().srgan_nhwc_to_nchw(_ptr(t), _ptr(out), n, c, h, w, _stream()), "nhwc_to_nchw")
    return out


def cat_batch(tensors):
    """Concatenate NHWC-dense activations along the batch dimension (stays NHWC-dense, differentiable).
    Every layer of G / D / E is per-sample (instance norm, no batch norm), so running two batches as one is exact
    and gives the GEMM kernels twice the rows per launch."""
    tensors = [to_nhwc(t) for t in tensors]
    return torch.cat([t.permute(0, 2, 3, 1) for t in tensors], 0).permute(0, 3, 1, 2)


def _dense2d(t):
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------
# convolution
# ------------------------------------------------------------------------------------------
def _conv_desc(n, hi, wi, i, ho, wo, o, kh, kw, stride, pad, pad_mode, weight):
    so, si, sh, sw = weight.stride()
    return ConvDesc(n, hi, wi, i, ho, wo, o, kh, kw, stride, pad, pad_mode, so, si, sh, sw)


def _conv_ws(desc, device):
    lib = _lib.load()
    nbytes = lib.srgan_conv2d_workspace(ctypes.byref(desc))
    if nbytes == 0:
        raise _lib.SrganHipError("conv2d: " + lib.srgan_last_error().decode())
    return workspace(device, nbytes), nbytes


# ---- packed-weight cache ---------------------------------------------------------------------------
# The repacked weight operand of a conv depends only on (weight values, geometry, kind).  Inside a trainer step the
# weights change only at optimiser steps, so the trainer turns the cache on for the duration of ``train()`` and, after
# each optimiser step, re-packs every cached operand of that network in ONE launch (``refresh_packed``).  Entries persist
# across ``train()`` calls; an entry is only trusted while the parameter's autograd version counter is unchanged (any
# ordinary in-place update -- ``load_state_dict``, ``copy_`` -- bumps it; the raw-pointer Adam does not, which is why the
# trainer refreshes explicitly), and everything is re-packed once when a scope is entered.  Outside such a scope (plain
# module calls) every call repacks.
_pack_cache_on = False
_pack_cache = {}          # (id(weight), kind, act_flag, geometry) -> _Packed
_structure_epoch = 0      # bumped whenever a buffer a captured hipGraph may point at is dropped or re-allocated


def structure_epoch():
    return _structure_epoch


def bump_structure_epoch():
    global _structure_epoch
    _structure_epoch += 1


def graph_keepalive():
    """Every persistent device buffer the conv / norm ops hand to kernels by pointer (packed operands, repack tables,
    workspaces).  A captured train step holds these references for its lifetime: the caches may move on to new buffers
    (a new geometry rebuilds a repack table), but memory a recorded launch points at is never handed to anyone else."""
    keep = [h.buf for h in _pack_cache.values()]
    keep += [t[1] for t in _tables.values() if t[1] is not None]
    keep += list(_workspaces.values())
    return keep


class _Packed:
    """A cached packed operand.  The parameter is held WEAKLY: when a network is dropped (a notebook re-run, a sweep, the test
    suite building many trainers) its entries die with it and are purged at the next scope entry, instead of pinning the weight,
    its packed device buffer and a slot of every later refresh for the life of the process."""
    __slots__ = ("buf", "_wref", "desc", "kind", "act", "version", "fresh", "ptr", "scratch")

    def __init__(self, buf, weight, desc, kind, act, scratch):
        self.buf, self._wref, self.desc, self.kind, self.act = buf, weakref.ref(weight), desc, kind, act
        self.scratch = scratch                 # bytes of per-call scratch the packed run wants (shared workspace)
        self.version, self.fresh, self.ptr = weight._version, True, weight.data_ptr()

    @property
    def weight(self):
        return self._wref()


def _purge_dead_packed():
    dead = [k for k, h in _pack_cache.items() if h.weight is None]
    if not dead:
        return
    for k in dead:
        del _pack_cache[k]
    for k in [k for k, g in _geo_cache.items() if g[0].weight is None]:
        del _geo_cache[k]
    _tables.clear()


class pack_cache:
    """Context manager: cache packed conv weights (see above).  ``refresh_on_entry=False``: the caller vouches that no
    parameter was written behind the cache's back since the last scope (the captured train step does: it checks the
    parameters' version counters itself before every replay)."""

    def __init__(self, refresh_on_entry=True):
        self._refresh = refresh_on_entry

    def __enter__(self):
        global _pack_cache_on
        self._prev = _pack_cache_on
        _pack_cache_on = True
        if not self._prev:
            _purge_dead_packed()
        if self._refresh and not self._prev and _pack_cache:
            # entries persist between scopes; a ``.data`` update made outside (no version bump) would go unseen, so the
            # whole cache is re-packed on entry -- one multi-pack launch
            refresh_packed([h.weight for h in _pack_cache.values()])
        return self

    def __exit__(self, *exc):
        global _pack_cache_on
        _pack_cache_on = self._prev
        return False


def set_compute_dtype(name):
    """"fp32" (default: exact fp32 MFMA, Winograd where it applies) or "bf16" (BASELINE configs [2]-[4]: conv operands rounded
    to bf16 on their way into LDS, v_mfma_f32_32x32x16_bf16 with fp32 accumulation; everything else stays fp32).
    Process-wide; drops the packed-weight cache because the two modes use different kernels / layouts."""
    mode = {"fp32": 0, "float32": 0, "bf16": 1, "bfloat16": 1}[str(name).replace("torch.", "")]
    _lib.check(_lib.load().srgan_set_compute_mode(mode), "set_compute_mode")
    bump_structure_epoch()
    _pack_cache.clear()
    _geo_cache.clear()
    _tables.clear()


def pack_cache_active():
    """True inside a ``pack_cache()`` scope (the 16-bit activation paths of the bf16 mode live on cached operands)."""
    return _pack_cache_on


def get_compute_dtype():
    return "bf16" if _lib.load().srgan_get_compute_mode() == 1 else "fp32"


def invalidate_packed(params=None):
    """Forget cached operands (all, or those of ``params``): they are re-packed one by one at their next use."""
    bump_structure_epoch()
    if params is None:
        _pack_cache.clear()
        _geo_cache.clear()
        _tables.clear()
        return
    ids = {id(p) for p in params}
    for key in [k for k in _pack_cache if k[0] in ids]:
        del _pack_cache[key]
    for key in [k for k in _geo_cache if k[0] in ids]:
        del _geo_cache[key]
    _tables.clear()


def mark_stale(params):
    """The raw-pointer optimiser calls this after writing ``params``: their cached operands must be re-packed before the
    next use (in one launch by ``refresh_packed``, else one by one)."""
    if not _pack_cache:
        return
    ids = {id(p) for p in params}
    for k, h in _pack_cache.items():
        if k[0] in ids:
            h.fresh = False


def _pack_one(hit):
    lib = _lib.load()
    _lib.check(lib.srgan_conv2d_pack(ctypes.byref(hit.desc), hit.kind, hit.act, _ptr(hit.weight), _ptr(hit.buf), hit.buf.numel(),
                                     _stream()), "conv2d_pack")
    hit.version, hit.fresh = hit.weight._version, True
    if hit.ptr != hit.weight.data_ptr():       # storage swapped under the parameter (``p.data = ...``): tables hold the old pointer
        hit.ptr = hit.weight.data_ptr()
        _tables.clear()


_geo_cache = {}           # (id(weight), kind, act_flag, full geometry) -> (_Packed, scratch bytes of that geometry)


def _packed(desc, weight, kind, act):
    """-> (_Packed, scratch bytes).  Operands whose layout does not depend on batch / map size (srgan_conv2d_pack_signature:
    the Winograd filter images) are shared between the geometries a weight is used with (the trainer runs the generator at
    batch 32, 64 and 128: one repack per optimiser step instead of three)."""
    gkey = (id(weight), kind, int(act != ACT_NONE), desc.N, desc.Hi, desc.Wi, desc.I, desc.O, desc.kh, desc.stride,
            desc.pad, desc.pad_mode)
    g = _geo_cache.get(gkey)
    if g is not None and g[0].weight is weight and _pack_cache.get(g[2]) is g[0]:
        hit, scratch = g[0], g[1]
    else:
        lib = _lib.load()
        sig = lib.srgan_conv2d_pack_signature(ctypes.byref(desc), kind, act)
        key = gkey if sig == 0 else (id(weight), kind, int(act != ACT_NONE), "sig", sig, desc.I, desc.O, desc.kh, desc.stride,
                                     desc.pad, desc.pad_mode)
        scratch = lib.srgan_conv2d_packed_scratch(ctypes.byref(desc), kind)
        hit = _pack_cache.get(key)
        if hit is None or hit.weight is not weight:
            nbytes = lib.srgan_conv2d_packed_bytes(ctypes.byref(desc), kind, act)
            if nbytes == 0:
                raise _lib.SrganHipError("conv2d pack: " + lib.srgan_last_error().decode())
            own = _lib.ConvDesc()
            ctypes.memmove(ctypes.byref(own), ctypes.byref(desc), ctypes.sizeof(own))
            hit = _Packed(torch.empty(nbytes, dtype=torch.uint8, device=weight.device), weight, own, kind, act, scratch)
            _pack_cache[key] = hit
            _tables.clear()
            _pack_one(hit)
            _geo_cache[gkey] = (hit, scratch, key)
            return hit, scratch
        _geo_cache[gkey] = (hit, scratch, key)
    if not hit.fresh or hit.version != weight._version or hit.ptr != weight.data_ptr():
        _pack_one(hit)
    return hit, scratch


_tables = {}              # frozenset of parameter ids -> (entries, device table, singles)


def refresh_packed(params, force=False):
    """Re-pack every cached operand of ``params`` after their optimiser step: one multi-pack launch for the implicit-GEMM /
    Winograd operands (device table built once per parameter set), single launches for the few narrow-output layers."""
    if not (_pack_cache_on or force):
        return
    params = list(params)
    if not params:
        return
    lib = _lib.load()
    tkey = frozenset(id(p) for p in params)
    tab = _tables.get(tkey)
    if tab is None:
        ids = set(tkey)
        hits = [h for k, h in _pack_cache.items() if k[0] in ids and h.weight is not None]
        for h in hits:
            # the layout of an operand follows the kernel dispatch (compute mode, SRGAN_* switches): an entry made under another
            # dispatch gets a buffer of the size the current one wants before anything is packed into it
            want = lib.srgan_conv2d_packed_bytes(ctypes.byref(h.desc), h.kind, h.act)
            if want != h.buf.numel():
                bump_structure_epoch()
                h.buf = torch.empty(want, dtype=torch.uint8, device=h.buf.device)
                h.scratch = lib.srgan_conv2d_packed_scratch(ctypes.byref(h.desc), h.kind)
        nb = lib.srgan_pack_entry_bytes()
        multi, singles, blob = [], [], bytearray()
        for h in hits:
            rec = (ctypes.c_char * nb)()
            rc = lib.srgan_conv2d_pack_entry(ctypes.byref(h.desc), h.kind, h.act, _ptr(h.weight), _ptr(h.buf), ctypes.byref(rec))
            if rc == 0:
                multi.append(h)
                blob += bytes(rec)
            elif rc == 1:
                singles.append(h)
            else:
                _lib.check(rc, "conv2d_pack_entry")
        dev = None
        if multi:
            dev = upload_small(blob, params[0].device)
        tab = (multi, dev, singles)
        _tables[tkey] = tab
    multi, dev, singles = tab
    if any(h.ptr != h.weight.data_ptr() for h in multi):       # a parameter's storage moved: rebuild the table next time
        _tables.pop(tkey, None)
        for h in multi + singles:
            _pack_one(h)
        return
    if multi:
        _lib.check(lib.srgan_conv2d_pack_multi(_ptr(dev), len(multi), _stream()), "conv2d_pack_multi")
        for h in multi:
            h.version, h.fresh = h.weight._version, True
    # The operands outside the multi-pack launch (narrow-output layers, the RGB layers: one small kernel each, four for a
    # stride-2 input gradient) are re-packed at their next USE instead: the discriminator's image-gradient operands are used
    # once per train step (generator update) but went stale -- and were re-packed -- after each of its k optimiser steps.
    for h in singles:
        if _EAGER_SINGLE_PACKS:
            _pack_one(h)
        else:
            h.fresh = False


_EAGER_SINGLE_PACKS = _lib.ab("SRGAN_EAGER_SINGLE_PACKS")


def mark_singles_stale():
    """Before a train step is RECORDED: every operand that is re-packed at use (see refresh_packed) is marked stale, so that the
    recording holds a pack launch at the first use of each one -- a replay starts from whatever the previous step's optimisers
    left, not from the state the cache happened to be in when the step was captured."""
    lib = _lib.load()
    nb = lib.srgan_pack_entry_bytes()
    rec = (ctypes.c_char * nb)()
    for h in _pack_cache.values():
        if h.weight is not None and lib.srgan_conv2d_pack_entry(ctypes.byref(h.desc), h.kind, h.act, _ptr(h.weight), _ptr(h.buf),
                                                                 ctypes.byref(rec)) == 1:
            h.fresh = False


def _run_conv_fwd(desc, x, weight, bias, y, act, slope, keep_v=None):
    lib = _lib.load()
    if _pack_cache_on:
        hit, scratch = _packed(desc, weight, 0, act)
        # keep_v: the caller's own buffer for the F(4x4,3x3) transformed input (kept for the weight gradient) instead of scratch
        ws = keep_v if keep_v is not None else (workspace(x.device, scratch) if scratch else None)
        _lib.check(lib.srgan_conv2d_fwd_packed(ctypes.byref(desc), _ptr(x), _ptr(hit.buf), _ptr(bias), _ptr(y), act,
                                               float(slope), _ptr(ws), scratch, _stream()), "conv2d_fwd_packed")
        return
    ws, nb = _conv_ws(desc, x.device)
    _lib.check(lib.srgan_conv2d_fwd(ctypes.byref(desc), _ptr(x), _ptr(weight), _ptr(bias), _ptr(y), act,
                                    float(slope), _ptr(ws), nb, _stream()), "conv2d_fwd")


def _run_conv_dgrad(desc, dy, weight, dx, res=None, mask=None, mask_slope=0.0):
    """dx = input gradient (+ res: the gradient of a skip connection that shares the conv's input, added in the kernel's
    epilogue where the dispatch supports it) (* LeakyReLU'(mask): the activation backward of the layer that produced the
    conv's input, in the epilogue of the transposed stride-2 Winograd kernel, else one in-place pass)."""
    lib = _lib.load()
    if mask is not None and (res is not None or not _pack_cache_on):
        _run_conv_dgrad(desc, dy, weight, dx, res)
        _lib.check(lib.srgan_act_bwd(_ptr(mask), _ptr(dx), _ptr(dx), dx.numel(), ACT_LRELU, float(mask_slope), _stream()), "act_bwd")
        return
    if _pack_cache_on:
        hit, scratch = _packed(desc, weight, 1, ACT_NONE)
        ws = workspace(dy.device, scratch) if scratch else None
        if mask is not None:
            _lib.check(lib.srgan_conv2d_dgrad_packed_mask(ctypes.byref(desc), _ptr(dy), _ptr(hit.buf), _ptr(mask), float(mask_slope),
                                                          _ptr(dx), _ptr(ws), scratch, _stream()), "conv2d_dgrad_packed_mask")
            return
        if res is not None:
            _lib.check(lib.srgan_conv2d_dgrad_packed_add(ctypes.byref(desc), _ptr(dy), _ptr(hit.buf), _ptr(res), _ptr(dx), _ptr(ws),
                                                         scratch, _stream()), "conv2d_dgrad_packed_add")
            return
        _lib.check(lib.srgan_conv2d_dgrad_packed(ctypes.byref(desc), _ptr(dy), _ptr(hit.buf), _ptr(dx), _ptr(ws), scratch,
                                                 _stream()), "conv2d_dgrad_packed")
        return
    ws, nb = _conv_ws(desc, dy.device)
    _lib.check(lib.srgan_conv2d_dgrad(ctypes.byref(desc), _ptr(dy), _ptr(weight), _ptr(dx), _ptr(ws), nb,
                                      _stream()), "conv2d_dgrad")
    if res is not None:
        _lib.check(lib.srgan_add(_ptr(dx), _ptr(res), _ptr(dx), dx.numel(), _stream()), "add")


def _run_conv_wgrad(desc, x, dy, dw, dbias, ws, nb, v_image=None):
    """``(ws, nb)``: the workspace of ``_conv_ws(desc, ...)`` (``_wgrad_to_sink`` fetches it)."""
    if v_image is not None:
        _lib.check(_lib.load().srgan_conv2d_wgrad_v(ctypes.byref(desc), _ptr(v_image), _ptr(dy), _ptr(dw), _ptr(dbias), _ptr(ws),
                                                    nb, _stream()), "conv2d_wgrad_v")
        return
    _lib.check(_lib.load().srgan_conv2d_wgrad(ctypes.byref(desc), _ptr(x), _ptr(dy), _ptr(dw), _ptr(dbias), _ptr(ws),
                                              nb, _stream()), "conv2d_wgrad")


# ---- parameter-gradient sink ------------------------------------------------------------------------------
# A parameter reached through several graphs in ONE backward call (the generator inside util_notebook.py:664 and :689: the
# reconstruction / identity graph and the kept ``target_image`` graph) gets one gradient per use; torch's engine sums them in
# the AccumulateGrad input buffer -- 156 small elementwise launches per train step.  Inside a ``fused_param_grads`` scope the
# weight-gradient kernels of this module write a parameter's FIRST contribution of the pass into a fresh buffer and ADD the
# later ones in their own epilogue (split-K slab reduce with beta = 1, central-biasing records with the accumulate flag); the
# Functions return no gradient for such a parameter, and when the scope closes ``p.grad`` is bound to the buffer (added to an
# existing ``p.grad``, as AccumulateGrad would).  Same operands, same single rounding per addition as the engine's ``a += b``:
# bit-identical results.  A parameter's post-accumulate-grad hooks still fire once per backward call -- the engine runs the
# AccumulateGrad node with an undefined gradient -- but DURING the pass, before ``p.grad`` is bound: fine for hooks that count
# (``dp.GradReducer`` while a step is recorded), wrong for hooks that read the gradient, which is why the eager data-parallel
# step (buckets sent from the hooks) keeps the ordinary path.  Opt-in (the trainer wraps its backward calls): plain
# ``.backward()`` / ``autograd.grad`` on the modules are untouched.
#
# The sink's buffers are read by nobody until the scope closes, which also lets the library DEFER the split-K slab sums of the
# weight-gradient calls (``srgan_wgrad_defer_begin``): they wait in an arena and run as a few large launches instead of one
# ~12 us launch per layer (145 per train step).  ``SRGAN_NO_WGRAD_DEFER=1`` keeps the immediate sums.
_grad_sink = None
_sink_alloc = None          # optional callable(parameter) -> buffer for its first contribution of a pass (dp.grad_slot), or None
_sink_seed = False
_defer_depth = 0
_NO_WGRAD_DEFER = _lib.ab("SRGAN_NO_WGRAD_DEFER")
_WGRAD_ARENA_BYTES = 32 << 20      # first size; grown to what a pass asks for (below)
_WGRAD_ARENA_MAX = 2048 << 20
_arena_want = {}                    # device index -> bytes the largest pass so far asked for


def _wgrad_arena(device=None):
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    # one arena per DEVICE: its uses are serialised by stream order (srgan_wgrad_defer_begin records the stream, a
    # recorded step replays on the caller's stream), so a re-recorded step -- a new capture stream each time -- takes no new GiB.
    # Sized from use (it was a fixed 1 GiB): the library reports what the deferrable calls of a pass asked
    # for (srgan_wgrad_defer_need); a pass that did not fit -- it still runs right, with an early flush of the queued sums --
    # makes the NEXT scope take a larger arena.  A trainer's step 0 is eager, so the arena has its final size before a step is
    # recorded; growing later drops the recordings (structure epoch), never while a capture is in flight.
    key = ("wgrad_arena", dev.index)
    a = _workspaces.get(key)
    want = min(max(_WGRAD_ARENA_BYTES, _arena_want.get(dev.index, 0)), _WGRAD_ARENA_MAX)
    if a is None or (a.numel() < want and not capturing()):
        if a is not None:
            bump_structure_epoch()
        want = (want + (16 << 20) - 1) // (16 << 20) * (16 << 20)
        a = _workspaces[key] = torch.empty(want, dtype=torch.uint8, device=dev)
    return a


class fused_param_grads:
    """``device``: where the pass runs (default: the current device) -- the arena of the deferred slab sums lives there and the
    sums run on that device's current stream."""

    def __init__(self, enabled=True, device=None, seed=False):
        """``seed``: a parameter that already HAS a gradient (an earlier scope of the same backward pass bound it) takes this
        scope's contributions on top of it -- its ``p.grad`` is the sink slot and the kernels add into it -- instead of into a
        fresh buffer that the scope's exit would add with one elementwise launch per parameter."""
        self._enabled = enabled
        self._device = device
        self._seed = seed

    def __enter__(self):
        global _grad_sink, _defer_depth
        global _sink_seed
        self._prev = _grad_sink
        self._prev_seed = _sink_seed
        _grad_sink = {} if self._enabled else None
        _sink_seed = bool(self._seed and self._enabled)
        self._defer = False
        if self._enabled and not _NO_WGRAD_DEFER and _defer_depth == 0:
            a = _wgrad_arena(self._device)
            self._arena_index = a.device.index
            st = ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)
            _lib.check(_lib.load().srgan_wgrad_defer_begin(_ptr(a), a.numel(), st), "wgrad_defer_begin")
            self._defer = True
            _defer_depth = 1
        return self

    def __exit__(self, et, ev, tb):
        global _grad_sink, _defer_depth
        global _sink_seed
        sink, _grad_sink = _grad_sink, self._prev
        _sink_seed = self._prev_seed
        if self._defer:
            _defer_depth = 0
            err = _lib.load().srgan_wgrad_defer_end()          # the queued sums, before anyone binds or reads the buffers
            if et is None:
                _lib.check(err, "wgrad_defer_end")
            need = ctypes.c_longlong(0)
            _lib.load().srgan_wgrad_defer_need(ctypes.byref(need))
            idx = self._arena_index
            if need.value > _arena_want.get(idx, 0):
                _arena_want[idx] = int(need.value)
        if et is None and sink:
            with torch.no_grad():
                for p, buf in sink.values():
                    if p.grad is None:
                        p.grad = buf
                    elif p.grad is not buf:      # (a seeded slot IS p.grad: the kernels have added into it)
                        p.grad.add_(buf)
        return False


def _sink_slots(*params):
    """-> ([buffer per parameter], accumulate) when every parameter can take its gradient through the sink of the current
    scope (leaf parameters, all visited before or none), else None: the caller then returns ordinary gradients."""
    if _grad_sink is None:
        return None
    if not all(p.is_leaf and p.requires_grad for p in params):
        return None
    seen = [id(p) in _grad_sink for p in params]
    if any(seen) and not all(seen):
        return None
    if not seen[0]:
        if _sink_seed and all(p.grad is not None and p.grad.dtype == torch.float32 and p.grad.is_contiguous() for p in params):
            for p in params:                     # seeded scope: add into the gradient an earlier scope left
                _grad_sink[id(p)] = (p, p.grad)
            return [p.grad for p in params], True
        bufs = [_sink_alloc(p) if _sink_alloc is not None else None for p in params]   # data parallel: the bucket slices
        # a bucket slice is the SAME storage an earlier pass bound to p.grad (GradReducer.finish / a previous
        # scope's exit).  Without a zero_grad in between (gradient accumulation, two backward calls) that gradient is still
        # live: writing this pass's first contribution over it would lose it, and the exit's `p.grad is not buf` test would
        # skip the add.  Such a slot is a seeded one -- the kernels add into it; all or none, since one launch serves the group.
        live = [b is not None and p.grad is not None and p.grad.data_ptr() == b.data_ptr() for p, b in zip(params, bufs)]
        if any(live):
            if all(live) and all(p.grad.dtype == torch.float32 and p.grad.is_contiguous() for p in params):
                for p in params:
                    _grad_sink[id(p)] = (p, p.grad)
                return [p.grad for p in params], True
            bufs = [None] * len(params)          # mixed: fresh buffers, added to p.grad at the exit like any unseeded slot
        for p, buf in zip(params, bufs):
            if buf is None:
                buf = torch.empty(p.shape, dtype=torch.float32, device=p.device)
            _grad_sink[id(p)] = (p, buf)
    return [_grad_sink[id(p)][1] for p in params], seen[0]


class _wgrad_accumulate:
    """``srgan_set_wgrad_accumulate`` around the weight-gradient calls of one Function.backward (thread-local in the library):
    bit 0 = add to the buffer (a later use of the parameter in this pass), bit 1 = the buffer is a sink slot, so the slab sum
    may wait for the end of the scope."""

    def __init__(self, on, sink=False):
        self._mode = (1 if on else 0) | (2 if sink and _defer_depth else 0)

    def __enter__(self):
        if self._mode:
            _lib.load().srgan_set_wgrad_accumulate(self._mode)

    def __exit__(self, *exc):
        if self._mode:
            _lib.load().srgan_set_wgrad_accumulate(0)
        return False


def _wgrad_to_sink(desc, params, launch):
    """The weight (and bias) gradient of the convolution ``desc``, through the gradient sink of the current scope when it takes
    ``params`` = (weight,) or (weight, bias), else into fresh buffers.  ``launch(dd, dw, db, ws, nb)`` makes the one library
    call: ``dd`` is ``desc`` with the strides of the buffer ``dw``, ``(ws, nb)`` the workspace of ``srgan_conv2d_workspace``.
    -> (dw, db), both None when the sink took them (the Function then returns no gradient for the parameters)."""
    slots = _sink_slots(*params)
    if slots is not None:
        bufs, acc = slots
    else:
        bufs, acc = [torch.empty(p.shape, dtype=torch.float32, device=p.device) for p in params], False
    dw, db = bufs[0], (bufs[1] if len(bufs) > 1 else None)
    dd = ConvDesc.from_buffer_copy(desc)
    dd.sO, dd.sI, dd.sH, dd.sW = dw.stride()
    ws, nb = _conv_ws(dd, dw.device)
    with _wgrad_accumulate(acc, slots is not None):
        launch(dd, dw, db, ws, nb)
    return (None, None) if slots is not None else (dw, db)


def _act_bwd(y, gy, act, slope):
    g = torch.empty_like(gy)
    _lib.check(_lib.load().srgan_act_bwd(_ptr(y), _ptr(gy), _ptr(g), gy.numel(), act, float(slope), _stream()), "act_bwd")
    return g


class _Conv2dFn(Function):
    """``skip=True``: also returns the input itself as a second output -- the tensor a residual connection should use.  Its
    gradient then arrives in THIS backward next to the conv output's, and the input-gradient kernel adds it in its epilogue
    (``srgan_conv2d_dgrad_packed_add``) instead of autograd accumulating the two paths with a separate pass.

    A chain conv + LeakyReLU -> conv (+ LeakyReLU) -> ... whose intermediate tensors have no other consumer (the discriminator
    trunk, ``model._run_trunk``) moves each activation's backward into the NEXT layer's input-gradient kernel: the producer is
    called with ``act_bwd_by_consumer=True`` (its backward takes the incoming gradient as already multiplied by its own
    activation's derivative) and the consumer with ``in_slope`` = the producer's slope (its input gradient is multiplied by 1 or
    ``in_slope`` after the sign of its input: ``srgan_conv2d_dgrad_packed_mask``)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, pad_mode, act, slope, skip=False, in_slope=None, act_bwd_by_consumer=False):
        x = to_nhwc(x)
        _require_gpu(weight, "conv2d weight")
        n, i, hi, wi = x.shape
        o, i2, kh, kw = weight.shape
        if i != i2:
            raise _lib.SrganHipError(f"conv2d: input has {i} channels, weight expects {i2}")
        ho = (hi + 2 * pad - kh) // stride + 1
        wo = (wi + 2 * pad - kw) // stride + 1
        desc = _conv_desc(n, hi, wi, i, ho, wo, o, kh, kw, stride, pad, pad_mode, weight)
        y = nhwc_empty(n, o, ho, wo, x.device)
        # F(4x4,3x3) layers: the forward's transformed input serves the weight gradient too -- keep it instead of scratch
        keep_v = None
        if _pack_cache_on and ctx.needs_input_grad[1]:
            nv = _lib.load().srgan_conv2d_wgrad_v_bytes(ctypes.byref(desc))
            if nv:
                keep_v = torch.empty(nv, dtype=torch.uint8, device=x.device)
        _run_conv_fwd(desc, x, weight, bias, y, act, slope, keep_v)
        ctx.v_image = keep_v
        ctx.desc, ctx.act, ctx.slope = desc, act, slope
        ctx.weight = weight            # by reference: read at backward time (torch 1.4 semantics)
        ctx.has_bias = bias is not None
        ctx.bias = bias
        ctx.in_slope, ctx.act_bwd_by_consumer = in_slope, bool(act_bwd_by_consumer) and act == ACT_LRELU
        if in_slope is not None and skip:
            raise _lib.SrganHipError("conv2d: in_slope and skip do not combine")
        ctx.save_for_backward(x, y if (act != ACT_NONE and not ctx.act_bwd_by_consumer) else None)
        if skip:
            return y, x
        return y

    @staticmethod
    def backward(ctx, gy, gskip=None):
        x, y = ctx.saved_tensors
        weight = ctx.weight
        dx = dw = db = None
        if gy is None:                     # only the skip path was used downstream
            return (to_nhwc(gskip) if gskip is not None else None), None, None, None, None, None, None, None, None, None, None
        gy = to_nhwc(gy)
        if ctx.act != ACT_NONE and not ctx.act_bwd_by_consumer:
            gy = _act_bwd(y, gy, ctx.act, ctx.slope)
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            res = to_nhwc(gskip) if gskip is not None else None
            if res is not None and res.data_ptr() == dx.data_ptr():
                res = res.clone()
            if ctx.in_slope is not None:
                _run_conv_dgrad(ctx.desc, gy, weight, dx, res, x, ctx.in_slope)
            else:
                _run_conv_dgrad(ctx.desc, gy, weight, dx, res)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = _wgrad_to_sink(ctx.desc, (weight, ctx.bias) if ctx.has_bias else (weight,),
                                    lambda dd, dw, db, ws, nb: _run_conv_wgrad(dd, x, gy, dw, db, ws, nb, ctx.v_image))
        return dx, dw, db, None, None, None, None, None, None, None, None


def conv2d(x, weight, bias=None, stride=1, padding=0, pad_mode=PAD_ZERO, act=ACT_NONE, slope=0.0, in_slope=None,
           act_bwd_by_consumer=False):
    return _Conv2dFn.apply(x, weight, bias, stride, padding, pad_mode, act, slope, False, in_slope, act_bwd_by_consumer)


def conv2d_skip(x, weight, bias=None, stride=1, padding=0, pad_mode=PAD_ZERO, act=ACT_NONE, slope=0.0):
    """-> (conv2d(x, ...), x): use the second result for a skip connection around the convolution (see _Conv2dFn)."""
    return _Conv2dFn.apply(x, weight, bias, stride, padding, pad_mode, act, slope, True)


class _ConvTranspose2dFn(Function):
    """y = conv_transpose2d(x, w[Cin,Cout,kh,kw]): the input-gradient kernel of the conv C whose
    weight is w viewed as [O=Cin][I=Cout]; backward = C forward (dx) and C's weight gradient."""

    @staticmethod
    def forward(ctx, x, weight, stride, pad):
        x = to_nhwc(x)
        _require_gpu(weight, "conv_transpose2d weight")
        n, ci, hi, wi = x.shape
        ci2, co, kh, kw = weight.shape
        if ci != ci2:
            raise _lib.SrganHipError(f"conv_transpose2d: input has {ci} channels, weight expects {ci2}")
        ho = (hi - 1) * stride - 2 * pad + kh
        wo = (wi - 1) * stride - 2 * pad + kw
        # conv C: input = y-space [n,co,ho,wo], output = x-space [n,ci,hi,wi]
        desc = _conv_desc(n, ho, wo, co, hi, wi, ci, kh, kw, stride, pad, PAD_ZERO, weight)
        y = nhwc_empty(n, co, ho, wo, x.device)
        _run_conv_dgrad(desc, x, weight, y)
        ctx.desc, ctx.weight = desc, weight
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        gy = to_nhwc(gy)
        weight = ctx.weight
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _run_conv_fwd(ctx.desc, gy, weight, None, dx, ACT_NONE, 0.0)
        if ctx.needs_input_grad[1]:
            dw, _ = _wgrad_to_sink(ctx.desc, (weight,), lambda dd, dw, db, ws, nb: _run_conv_wgrad(dd, gy, x, dw, None, ws, nb))
        return dx, dw, None, None


def conv_transpose2d(x, weight, stride=2, padding=1):
    return _ConvTranspose2dFn.apply(x, weight, stride, padding)


# ------------------------------------------------------------------------------------------
# instance norm (+affine, activation, residual) and the CBIN affine
# ------------------------------------------------------------------------------------------
# The two entry families of csrc/norm.hip.  ``out_dtype`` / ``io`` select one: None / False = srgan_instnorm_fwd / _bwd (fp32
# tensors, every shape); a dtype / True = srgan_instnorm_fwd_io / _bwd_io (fp32 or bf16 x, a result of that dtype, dx of x's
# type; the shapes of srgan_instnorm_io_applicable).
def _instnorm_fwd(x, scale, shift, res, act, slope, eps, out_dtype=None):
    """-> (y, mean, rstd) of an NHWC-dense x (and skip tensor ``res``, fp32, or None)."""
    n, c, h, w = x.shape
    lib = _lib.load()
    y = torch.empty_like(x, dtype=out_dtype)
    mean = torch.empty(n * c, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    nb = lib.srgan_instnorm_workspace(n, h * w, c)
    ws = workspace(x.device, nb)
    tail = (_ptr(mean), _ptr(rstd), n, h * w, c, float(eps), act, float(slope), _ptr(ws), nb, _stream())
    if out_dtype is None:
        rc, what = lib.srgan_instnorm_fwd(_ptr(x), _ptr(scale), _ptr(shift), _ptr(res), _ptr(y), *tail), "instnorm_fwd"
    else:
        rc, what = lib.srgan_instnorm_fwd_io(_ptr(x), _is16(x), _ptr(scale), _ptr(shift), _ptr(res), _ptr(y), _is16(y), *tail), "instnorm_fwd_io"
    _lib.check(rc, what)
    return y, mean, rstd


def _instnorm_bwd(x, gy, scale, shift, mean, rstd, act, slope, io=False):
    """-> (dx, dscale, dshift) from the forward's NHWC-dense x and statistics and the NHWC-dense upstream gradient."""
    n, c, h, w = x.shape
    lib = _lib.load()
    dx = torch.empty_like(x)
    dscale = torch.empty(n, c, dtype=torch.float32, device=x.device)
    dshift = torch.empty_like(dscale)
    nb = lib.srgan_instnorm_workspace(n, h * w, c)
    ws = workspace(x.device, nb)
    tail = (_ptr(dscale), _ptr(dshift), n, h * w, c, act, float(slope), _ptr(ws), nb, _stream())
    if io:
        rc, what = lib.srgan_instnorm_bwd_io(_ptr(x), _is16(x), _ptr(gy), _is16(gy), _ptr(scale), _ptr(shift), _ptr(mean), _ptr(rstd),
                                             _ptr(dx), _is16(dx), *tail), "instnorm_bwd_io"
    else:
        rc, what = lib.srgan_instnorm_bwd(_ptr(x), _ptr(gy), _ptr(scale), _ptr(shift), _ptr(mean), _ptr(rstd), _ptr(dx), *tail), "instnorm_bwd"
    _lib.check(rc, what)
    return dx, dscale, dshift


class _InstNormFn(Function):
    """instance_norm_act (``out_dtype`` None) and instance_norm_act_io (a dtype: fp32 or bf16 input, a result of that type; dx
    has x's type)."""

    @staticmethod
    def forward(ctx, x, scale, shift, res, act, slope, eps, out_dtype):
        x = to_nhwc(x)
        if res is not None:
            res = to_nhwc(res)
        y, mean, rstd = _instnorm_fwd(x, scale, shift, res, act, slope, eps, out_dtype)
        ctx.act, ctx.slope, ctx.has_res, ctx.io = act, slope, res is not None, out_dtype is not None
        ctx.save_for_backward(x, scale, shift, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, scale, shift, mean, rstd = ctx.saved_tensors
        gy = to_nhwc(gy)
        dx, dscale, dshift = _instnorm_bwd(x, gy, scale, shift, mean, rstd, ctx.act, ctx.slope, ctx.io)
        has_aff = scale is not None
        return (dx, dscale if has_aff else None, dshift if has_aff else None, (gy.clone() if _DEBUG_CLONE else gy) if ctx.has_res else None,
                None, None, None, None)


def instance_norm_act(x, scale=None, shift=None, res=None, act=ACT_NONE, slope=0.0, eps=1e-5):
    """act((x - mean)/sqrt(var+eps) * scale[n,c] + shift[n,c]) (+ res)."""
    return _InstNormFn.apply(x, scale, shift, res, act, slope, eps, None)


# ------------------------------------------------------------------------------------------
# batch norm (norm_type="batch"): nn.BatchNorm2d and CBBNorm2d (csrc/norm_batch.hip)
# ------------------------------------------------------------------------------------------
def _bn_check(x, training, what):
    n, c, h, w = x.shape
    if c % 4:
        raise _lib.SrganHipError(f"{what}: C = {c} is not a multiple of 4 (the batch-norm kernels read channels four at a time)")
    if training and n * h * w <= 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size {}".format(list(x.shape)))


def _bn_buffers(running_mean, running_var, num_batches_tracked, training, momentum):
    """(running_mean, running_var, counter, cumulative, momentum) as the kernels take them: the buffers only where they are read or
    updated (F.batch_norm: updated in training when given, read in eval)."""
    if running_mean is None:
        return None, None, None, 0, 0.0
    cumulative = momentum is None
    if cumulative and num_batches_tracked is None:
        raise ValueError("batch norm with momentum=None needs num_batches_tracked")
    return running_mean, running_var, num_batches_tracked, int(cumulative), 0.0 if cumulative else float(momentum)


def _bn_stats(n, c, device):
    mean = torch.empty(c, dtype=torch.float32, device=device)
    return mean, torch.empty_like(mean), *(torch.empty(n * c, dtype=torch.float32, device=device) for _ in range(3))


class _BatchNormFn(Function):
    """act((x - mu_c) * r_c * weight + bias) with batch statistics (training) or the running ones.  Saves x and the statistics
    the forward used -- never the running buffers, which later forwards move on the device.  The weight is held by reference and
    read when backward RUNS (nn.BatchNorm2d's autograd saves it by reference: the stale-graph rule of the convolutions); the
    activation mask comes from the forward's own folded coefficients a / b."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps, act, slope):
        _require_gpu(x, "batch_norm")
        x = to_nhwc(x)
        n, c, h, w = x.shape
        _bn_check(x, training, "batch_norm")
        rm, rv, nbt, cumulative, mom = _bn_buffers(running_mean, running_var, num_batches_tracked, training, momentum)
        if not training and rm is None:
            raise ValueError("batch_norm: eval mode needs running statistics")
        lib = _lib.load()
        y = torch.empty_like(x)
        mean, rstd, m, a, b = _bn_stats(n, c, x.device)
        nb = lib.srgan_batchnorm_workspace(n, h * w, c)
        ws = workspace(x.device, nb)
        _lib.check(lib.srgan_batchnorm_fwd(_ptr(x), _ptr(weight), _ptr(bias), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(m), _ptr(a),
                                           _ptr(b), _ptr(rm), _ptr(rv), _ptr(nbt), n, h * w, c, int(bool(training)), mom, cumulative,
                                           float(eps), act, float(slope), _ptr(ws), nb, _stream()), "batchnorm_fwd")
        ctx.act, ctx.slope, ctx.training = act, slope, bool(training)
        ctx.has_affine = weight is not None
        ctx.weight = weight                    # by reference: read at backward time
        ctx.save_for_backward(x, mean, rstd, m, a, b)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, mean, rstd, m, a, b = ctx.saved_tensors
        gy = to_nhwc(gy)
        n, c, h, w = x.shape
        lib = _lib.load()
        dx = torch.empty_like(x)
        dweight = torch.empty(c, dtype=torch.float32, device=x.device)
        dbias = torch.empty_like(dweight)
        nb = lib.srgan_batchnorm_workspace(n, h * w, c)
        ws = workspace(x.device, nb)
        _lib.check(lib.srgan_batchnorm_bwd(_ptr(x), _ptr(gy), _ptr(ctx.weight), _ptr(mean), _ptr(rstd), _ptr(m), _ptr(a), _ptr(b), _ptr(dx),
                                           _ptr(dweight), _ptr(dbias), n, h * w, c, int(ctx.training), ctx.act, float(ctx.slope),
                                           _ptr(ws), nb, _stream()), "batchnorm_bwd")
        if not ctx.has_affine:
            dweight = dbias = None
        return dx, dweight, dbias, None, None, None, None, None, None, None, None


def batch_norm_act(x, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum=0.1, eps=1e-5,
                   act=ACT_NONE, slope=0.0, sync=False):
    """nn.BatchNorm2d + activation: act((x - mu_c) / sqrt(var_c + eps) * weight + bias).  training: batch statistics, and the
    running buffers (if given) are updated on the device; otherwise the running buffers are used.  sync: in training mode under a
    process group, the statistics of every rank's images (two all-gathers per call, forward and backward)."""
    if _synced(sync, training):
        return _SyncBatchNormFn.apply(x, weight, bias, running_mean, running_var, num_batches_tracked, momentum, eps, act, slope)
    return _BatchNormFn.apply(x, weight, bias, running_mean, running_var, num_batches_tracked, bool(training), momentum, eps,
                              act, slope)


class _CbbNormFn(Function):
    """CBBNorm2d: act((x - mu_nc) * r_c * scale[n,c] + shift[n,c]) (+ res), r_c from the batch (training) or running variance.
    scale / shift: CBIN's affine (cbin_affine / PrecomputedCon), whose backward takes dscale / dshift unchanged."""

    @staticmethod
    def forward(ctx, x, scale, shift, running_mean, running_var, num_batches_tracked, training, momentum, eps, act, slope, res):
        _require_gpu(x, "cbb_norm")
        x = to_nhwc(x)
        n, c, h, w = x.shape
        _bn_check(x, training, "cbb_norm")
        rm, rv, nbt, cumulative, mom = _bn_buffers(running_mean, running_var, num_batches_tracked, training, momentum)
        if not training and rm is None:
            raise ValueError("cbb_norm: eval mode needs running statistics")
        if res is not None:
            res = to_nhwc(res)
        scale, shift = _dense2d(scale), _dense2d(shift)
        lib = _lib.load()
        y = torch.empty_like(x)
        mean, rstd, m, a, b = _bn_stats(n, c, x.device)
        nb = lib.srgan_batchnorm_workspace(n, h * w, c)
        ws = workspace(x.device, nb)
        _lib.check(lib.srgan_cbbnorm_fwd(_ptr(x), _ptr(scale), _ptr(shift), _ptr(res), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(m),
                                         _ptr(a), _ptr(b), _ptr(rm), _ptr(rv), _ptr(nbt), n, h * w, c, int(bool(training)), mom,
                                         cumulative, float(eps), act, float(slope), _ptr(ws), nb, _stream()), "cbbnorm_fwd")
        ctx.act, ctx.slope, ctx.training, ctx.has_res = act, slope, bool(training), res is not None
        ctx.save_for_backward(x, scale, mean, rstd, m, a, b)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, scale, mean, rstd, m, a, b = ctx.saved_tensors
        gy = to_nhwc(gy)
        n, c, h, w = x.shape
        lib = _lib.load()
        dx = torch.empty_like(x)
        dscale = torch.empty(n, c, dtype=torch.float32, device=x.device)
        dshift = torch.empty_like(dscale)
        nb = lib.srgan_batchnorm_workspace(n, h * w, c)
        ws = workspace(x.device, nb)
        _lib.check(lib.srgan_cbbnorm_bwd(_ptr(x), _ptr(gy), _ptr(scale), _ptr(mean), _ptr(rstd), _ptr(m), _ptr(a), _ptr(b),
                                         _ptr(dx), _ptr(dscale), _ptr(dshift), n, h * w, c, int(ctx.training), ctx.act,
                                         float(ctx.slope), _ptr(ws), nb, _stream()), "cbbnorm_bwd")
        return (dx, dscale, dshift, None, None, None, None, None, None, None, None,
                (gy.clone() if _DEBUG_CLONE else gy) if ctx.has_res else None)


def cbb_norm_act(x, scale, shift, running_mean, running_var, num_batches_tracked, training, momentum=0.1, eps=1e-5,
                 act=ACT_NONE, slope=0.0, res=None, sync=False):
    """CBBNorm2d + activation (+ residual): act((x - mu_nc) / sqrt(var_c + eps) * scale[n,c] + shift[n,c]) (+ res), the reference's
    (F.batch_norm(x) - avgpool(F.batch_norm(x)) + tanh(Linear(c))) * weight + bias.  sync: as batch_norm_act."""
    if _synced(sync, training):
        return _SyncCbbNormFn.apply(x, scale, shift, running_mean, running_var, num_batches_tracked, momentum, eps, act, slope, res)
    return _CbbNormFn.apply(x, scale, shift, running_mean, running_var, num_batches_tracked, bool(training), momentum, eps, act,
                            slope, res)


# ---- data parallel: statistics of the global batch (dp.sync_batch_stats) -----------------------------------
def _sync_geometry(x, what):
    """(N_global, n0) of this rank's x: rank r holds images [r * N_local, (r + 1) * N_local) of the global batch, every rank the
    same number (the layout of everything in srgan_amd.dp)."""
    from . import dp
    n, c, h, w = x.shape
    ng = n * dp.world_size()
    if c % 4:
        raise _lib.SrganHipError(f"{what}: C = {c} is not a multiple of 4 (the batch-norm kernels read channels four at a time)")
    if ng * h * w <= 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size {}".format([ng, c, h, w]))
    return ng, n * dp.rank()


def _sync_exchange_buffer(lib, x, ng, with_scale):
    """A fresh buffer per call (caching allocator: stream-ordered, so nothing is shared with the side stream the second
    discriminator scale runs on), and the size the kernels check it against."""
    n, c, h, w = x.shape
    nb = lib.srgan_batchnorm_sync_exchange_bytes(ng, n, h * w, c, int(with_scale))
    if not nb:
        raise _lib.SrganHipError("batchnorm_sync: " + lib.srgan_last_error().decode(errors="replace"))
    return torch.empty(nb // 4, dtype=torch.float32, device=x.device), nb


def _sync_forward(ctx, cbb, x, p0, p1, res, running_mean, running_var, num_batches_tracked, momentum, eps, act, slope):
    """Phase 1 (this rank's slab partials into its chunk), the all-gather, phase 2 (merge over the global batch + apply)."""
    from . import dp
    what = "cbb_norm" if cbb else "batch_norm"
    _require_gpu(x, what)
    x = to_nhwc(x)
    n, c, h, w = x.shape
    ng, n0 = _sync_geometry(x, what)
    rm, rv, nbt, cumulative, mom = _bn_buffers(running_mean, running_var, num_batches_tracked, True, momentum)
    lib = _lib.load()
    y = torch.empty_like(x)
    mean, rstd, m, a, b = _bn_stats(n, c, x.device)
    buf, nb = _sync_exchange_buffer(lib, x, ng, False)
    _lib.check(lib.srgan_batchnorm_sync_fwd_partial(_ptr(x), _ptr(buf), nb, ng, n0, n, h * w, c, _stream()), "batchnorm_sync_fwd_partial")
    dp.all_gather_chunks(buf, what + ".forward")
    tail = (_ptr(rm), _ptr(rv), _ptr(nbt), _ptr(buf), nb, ng, n0, n, h * w, c, mom, cumulative, float(eps), act, float(slope), _stream())
    if cbb:
        _lib.check(lib.srgan_cbbnorm_sync_fwd_apply(_ptr(x), _ptr(p0), _ptr(p1), _ptr(res), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(m),
                                                    _ptr(a), _ptr(b), *tail), "cbbnorm_sync_fwd_apply")
    else:
        _lib.check(lib.srgan_batchnorm_sync_fwd_apply(_ptr(x), _ptr(p0), _ptr(p1), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(m), _ptr(a),
                                                      _ptr(b), *tail), "batchnorm_sync_fwd_apply")
    ctx.act, ctx.slope, ctx.geometry = act, slope, (ng, n0)
    return x, y, mean, rstd, m, a, b


def _sync_backward(ctx, cbb, x, gy, scale, weight, mean, rstd, m, a, b):
    """Phase 1 (this rank's {sum g, sum g * xh} partials, CBB: and its scale rows), the all-gather, phase 2 (combine + dx).
    Returns dx and the parameter gradients of the LOCAL images."""
    from . import dp
    what = "cbb_norm" if cbb else "batch_norm"
    gy = to_nhwc(gy)
    n, c, h, w = x.shape
    ng, n0 = ctx.geometry
    lib = _lib.load()
    dx = torch.empty_like(x)
    d0 = torch.empty((n, c) if cbb else (c,), dtype=torch.float32, device=x.device)      # dscale / dweight
    d1 = torch.empty_like(d0)                                                           # dshift / dbias
    buf, nb = _sync_exchange_buffer(lib, x, ng, cbb)
    _lib.check(lib.srgan_batchnorm_sync_bwd_partial(_ptr(x), _ptr(gy), _ptr(scale), _ptr(rstd), _ptr(m), _ptr(a), _ptr(b), _ptr(buf),
                                                    nb, ng, n0, n, h * w, c, ctx.act, float(ctx.slope), _stream()),
               "batchnorm_sync_bwd_partial")
    dp.all_gather_chunks(buf, what + ".backward")
    wb = lib.srgan_batchnorm_sync_workspace(n, c)
    ws = workspace(x.device, wb)
    tail = (_ptr(mean), _ptr(rstd), _ptr(m), _ptr(a), _ptr(b), _ptr(buf), nb, _ptr(dx), _ptr(d0), _ptr(d1), ng, n0, n, h * w, c, ctx.act,
            float(ctx.slope), _ptr(ws), wb, _stream())
    if cbb:
        _lib.check(lib.srgan_cbbnorm_sync_bwd_apply(_ptr(x), _ptr(gy), *tail), "cbbnorm_sync_bwd_apply")
    else:
        _lib.check(lib.srgan_batchnorm_sync_bwd_apply(_ptr(x), _ptr(gy), _ptr(weight), *tail), "batchnorm_sync_bwd_apply")
    return gy, dx, d0, d1


class _SyncBatchNormFn(Function):
    """_BatchNormFn in training mode with the statistics of every rank's images (same kept semantics: the weight by reference)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, num_batches_tracked, momentum, eps, act, slope):
        x, y, mean, rstd, m, a, b = _sync_forward(ctx, False, x, weight, bias, None, running_mean, running_var, num_batches_tracked,
                                                  momentum, eps, act, slope)
        ctx.has_affine = weight is not None
        ctx.weight = weight                    # by reference: read at backward time
        ctx.save_for_backward(x, mean, rstd, m, a, b)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, mean, rstd, m, a, b = ctx.saved_tensors
        gy, dx, dweight, dbias = _sync_backward(ctx, False, x, gy, None, ctx.weight, mean, rstd, m, a, b)
        if not ctx.has_affine:
            dweight = dbias = None
        return dx, dweight, dbias, None, None, None, None, None, None, None


class _SyncCbbNormFn(Function):
    """_CbbNormFn in training mode with r_c from every rank's images."""

    @staticmethod
    def forward(ctx, x, scale, shift, running_mean, running_var, num_batches_tracked, momentum, eps, act, slope, res):
        if res is not None:
            res = to_nhwc(res)
        scale, shift = _dense2d(scale), _dense2d(shift)
        x, y, mean, rstd, m, a, b = _sync_forward(ctx, True, x, scale, shift, res, running_mean, running_var, num_batches_tracked,
                                                  momentum, eps, act, slope)
        ctx.has_res = res is not None
        ctx.save_for_backward(x, scale, mean, rstd, m, a, b)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, scale, mean, rstd, m, a, b = ctx.saved_tensors
        gy, dx, dscale, dshift = _sync_backward(ctx, True, x, gy, scale, None, mean, rstd, m, a, b)
        return (dx, dscale, dshift, None, None, None, None, None, None, None,
                (gy.clone() if _DEBUG_CLONE else gy) if ctx.has_res else None)


def _synced(sync, training):
    """The synced path is taken in training mode under a process group (dp.is_distributed()); otherwise no collective is issued."""
    if not (sync and training):
        return False
    from . import dp
    return dp.is_distributed()


class _NormActConvFn(Function):
    """conv3x3(act(instance_norm(x) * scale + shift), weight) for a 32x32 map feeding an F(4x4,3x3) layer, without the
    normalised tensor: the norm kernel writes the convolution's transformed-input (V) image directly
    (``srgan_instnorm_fwd_v``), the multiply runs on it (``srgan_conv2d_fwd_from_v``) and the weight gradient re-uses it
    (``srgan_conv2d_wgrad_v``).  Backward = the three kernels of the unfused chain: input gradient of the convolution, its
    weight gradient, instance-norm backward.  Same kept semantics as _Conv2dFn (weight by reference, read at backward time)."""

    @staticmethod
    def forward(ctx, x, scale, shift, weight, act, slope, eps):
        lib = _lib.load()
        x = to_nhwc(x)
        n, c, h, w = x.shape
        o = weight.shape[0]
        desc = _conv_desc(n, h, w, c, h, w, o, 3, 3, 1, 1, PAD_ZERO, weight)
        hit, scratch = _packed(desc, weight, 0, ACT_NONE)
        keep = None
        if ctx.needs_input_grad[3]:
            nv = lib.srgan_conv2d_wgrad_v_bytes(ctypes.byref(desc))
            if nv:
                keep = torch.empty(max(nv, scratch), dtype=torch.uint8, device=x.device)
        v = keep if keep is not None else workspace(x.device, scratch)
        mean = torch.empty(n * c, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        _lib.check(lib.srgan_instnorm_fwd_v(ctypes.byref(desc), _ptr(x), _ptr(scale), _ptr(shift), _ptr(mean), _ptr(rstd), _ptr(v),
                                            v.numel(), float(eps), act, float(slope), _stream()), "instnorm_fwd_v")
        y = nhwc_empty(n, o, h, w, x.device)
        _lib.check(lib.srgan_conv2d_fwd_from_v(ctypes.byref(desc), _ptr(v), _ptr(hit.buf), None, _ptr(y), ACT_NONE, 0.0, _stream()),
                   "conv2d_fwd_from_v")
        ctx.desc, ctx.weight, ctx.v_image = desc, weight, keep
        ctx.act, ctx.slope, ctx.eps = act, slope, eps
        ctx.save_for_backward(x, scale, shift, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, scale, shift, mean, rstd = ctx.saved_tensors
        gy = to_nhwc(gy)
        weight = ctx.weight
        dw = None
        if ctx.needs_input_grad[3]:
            def launch(dd, dw, db, ws, nb):
                hx = None
                if ctx.v_image is None:   # no V kept (layer outside the F(4x4,3x3) weight-gradient geometry): recompute the normalised input
                    hx = _InstNormFn.apply(x.detach(), scale, shift, None, ctx.act, ctx.slope, ctx.eps, None)
                _run_conv_wgrad(dd, hx, gy, dw, None, ws, nb, ctx.v_image)

            dw, _ = _wgrad_to_sink(ctx.desc, (weight,), launch)
        dx = dscale = dshift = None
        if ctx.needs_input_grad[0] or (scale is not None and ctx.needs_input_grad[1]):
            dh = torch.empty_like(x)
            _run_conv_dgrad(ctx.desc, gy, weight, dh)
            dx, dscale, dshift = _instnorm_bwd(x, dh, scale, shift, mean, rstd, ctx.act, ctx.slope)
            if scale is None:
                dscale = dshift = None
        return dx, dscale, dshift, dw, None, None, None


class _ResBlockFn(Function):
    """SingleResidualBlock (pyfiles/model.py:196-201) as ONE autograd node on 32x32 maps whose convolutions run on F(4x4,3x3):

        y1 = c1(x);  y2 = c2(relu(cbin1(y1)));  out = cbin2(y2) + x

    Forward: c1 keeps its transformed input V0; cbin1 + ReLU is written straight as c2's transformed input V1
    (``srgan_instnorm_fwd_v``); cbin2 + skip in the slab norm kernel.  Backward: each norm backward writes the two transforms of
    its result -- the input-gradient kernel's image and the weight-gradient kernel's Z image -- instead of the result
    (``srgan_instnorm_bwd_vz``), the multiplies run on them (``srgan_conv2d_dgrad_from_v`` / ``srgan_conv2d_wgrad_vz`` with V1 /
    V0), and the skip path's gradient is added in c1's input-gradient epilogue.  Six launches fewer than the chain and the
    gradients w.r.t. y1 / y2 are never written or re-read.  Weights are held by reference and read at backward time (stale-graph
    semantics of SURVEY.md Appendix C-1), the packed operands come from the packed-weight scope."""

    @staticmethod
    def forward(ctx, x, s1, h1, s2, h2, w1, w2, eps):
        lib = _lib.load()
        x = to_nhwc(x)
        n, c, h, w = x.shape
        dev = x.device
        d1 = _conv_desc(n, h, w, c, h, w, w1.shape[0], 3, 3, 1, 1, PAD_ZERO, w1)
        d2 = _conv_desc(n, h, w, w1.shape[0], h, w, w2.shape[0], 3, 3, 1, 1, PAD_ZERO, w2)
        need_w = ctx.needs_input_grad[5] or ctx.needs_input_grad[6]
        hit1, sc1 = _packed(d1, w1, 0, ACT_NONE)
        hit2, sc2 = _packed(d2, w2, 0, ACT_NONE)
        v0 = torch.empty(max(sc1, 16), dtype=torch.uint8, device=dev) if need_w else workspace(dev, sc1)
        y1 = nhwc_empty(n, w1.shape[0], h, w, dev)
        _lib.check(lib.srgan_conv2d_fwd_packed(ctypes.byref(d1), _ptr(x), _ptr(hit1.buf), None, _ptr(y1), ACT_NONE, 0.0, _ptr(v0), sc1,
                                               _stream()), "conv2d_fwd_packed")
        v1 = torch.empty(max(sc2, 16), dtype=torch.uint8, device=dev) if need_w else workspace(dev, sc2)
        c1 = w1.shape[0]
        mean1 = torch.empty(n * c1, dtype=torch.float32, device=dev)
        rstd1 = torch.empty_like(mean1)
        _lib.check(lib.srgan_instnorm_fwd_v(ctypes.byref(d2), _ptr(y1), _ptr(s1), _ptr(h1), _ptr(mean1), _ptr(rstd1), _ptr(v1), sc2,
                                            float(eps), ACT_RELU, 0.0, _stream()), "instnorm_fwd_v")
        y2 = nhwc_empty(n, w2.shape[0], h, w, dev)
        _lib.check(lib.srgan_conv2d_fwd_from_v(ctypes.byref(d2), _ptr(v1), _ptr(hit2.buf), None, _ptr(y2), ACT_NONE, 0.0, _stream()),
                   "conv2d_fwd_from_v")
        out, mean2, rstd2 = _instnorm_fwd(y2, s2, h2, x, ACT_NONE, 0.0, eps)
        ctx.d1, ctx.d2, ctx.w1, ctx.w2 = d1, d2, w1, w2
        ctx.v0, ctx.v1 = (v0, v1) if need_w else (None, None)
        ctx.save_for_backward(y1, y2, s1, h1, s2, h2, mean1, rstd1, mean2, rstd2)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        y1, y2, s1, h1, s2, h2, mean1, rstd1, mean2, rstd2 = ctx.saved_tensors
        g = to_nhwc(g)
        n, c2, h, w = y2.shape
        c1 = y1.shape[1]
        dev = g.device
        d1, d2, w1, w2 = ctx.d1, ctx.d2, ctx.w1, ctx.w2
        st = _stream()

        def norm_bwd_vz(desc, y, gup, sc, sh, mean, rstd, act, ch):
            vb = lib.srgan_conv2d_packed_scratch(ctypes.byref(desc), 1)
            zb = lib.srgan_instnorm_bwd_vz_z_bytes(ctypes.byref(desc))
            vimg = torch.empty(vb, dtype=torch.uint8, device=dev)
            zimg = torch.empty(zb, dtype=torch.uint8, device=dev)
            dsc = torch.empty(n, ch, dtype=torch.float32, device=dev)
            dsh = torch.empty_like(dsc)
            _lib.check(lib.srgan_instnorm_bwd_vz(ctypes.byref(desc), _ptr(y), _ptr(gup), _ptr(sc), _ptr(sh), _ptr(mean), _ptr(rstd),
                                                 _ptr(dsc), _ptr(dsh), _ptr(vimg), vb, _ptr(zimg), zb, act, 0.0, st), "instnorm_bwd_vz")
            return vimg, zimg, dsc, dsh

        def wgrad_vz(desc, weight, v_fwd, zimg):
            return _wgrad_to_sink(desc, (weight,), lambda dd, dw, db, ws, nb: _lib.check(
                lib.srgan_conv2d_wgrad_vz(ctypes.byref(dd), _ptr(v_fwd), _ptr(zimg), _ptr(dw), _ptr(ws), nb, st), "conv2d_wgrad_vz"))[0]

        def dgrad_from_v(desc, weight, vimg, res, ch):
            hit, _ = _packed(desc, weight, 1, ACT_NONE)
            dx = nhwc_empty(n, ch, h, w, dev)
            _lib.check(lib.srgan_conv2d_dgrad_from_v(ctypes.byref(desc), _ptr(vimg), _ptr(hit.buf), _ptr(res), _ptr(dx), st),
                       "conv2d_dgrad_from_v")
            return dx

        # cbin2 backward -> c2's two images; c2 weight gradient (with V1) and input gradient
        vimg, zimg, ds2, dh2 = norm_bwd_vz(d2, y2, g, s2, h2, mean2, rstd2, ACT_NONE, c2)
        dw2 = wgrad_vz(d2, w2, ctx.v1, zimg) if (ctx.needs_input_grad[6] and ctx.v1 is not None) else None
        dh = dgrad_from_v(d2, w2, vimg, None, c1)
        # cbin1 + ReLU backward -> c1's two images; c1 weight gradient (with V0); input gradient + the skip path's gradient
        vimg, zimg, ds1, dh1 = norm_bwd_vz(d1, y1, dh, s1, h1, mean1, rstd1, ACT_RELU, c1)
        dw1 = wgrad_vz(d1, w1, ctx.v0, zimg) if (ctx.needs_input_grad[5] and ctx.v0 is not None) else None
        dx = dgrad_from_v(d1, w1, vimg, g, d1.I) if ctx.needs_input_grad[0] else None
        return dx, ds1, dh1, ds2, dh2, dw1, dw2, None


class _ResBlockBf16Fn(Function):
    """SingleResidualBlock (pyfiles/model.py:196-201) in the bf16 compute mode as ONE autograd node whose INTERMEDIATES live in
    HBM as bf16:

        y1 = c1(x) [bf16];  h = relu(cbin1(y1)) [bf16];  y2 = c2(h) [bf16];  out = cbin2(y2) + x [fp32]

    and in the backward  dy2 = cbin2'(y2, g) [bf16];  dh = c2^T(dy2) [bf16];  dy1 = (relu . cbin1)'(y1, dh) [bf16];
    dx = c1^T(dy1) + g [fp32].  The residual stream (x, out, g, dx), the statistics, the scale / shift gradients, the weight
    gradients and the master weights stay fp32; every product is bf16 x bf16 with fp32 accumulation on the LDS-resident-patch
    kernels of csrc/conv_halo16.hip (which read a bf16 tensor without the fp32 -> bf16 conversion and at half the bytes), the
    norms are the single-pass slab kernels with bf16 I/O.  Against the unfused bf16-mode chain the conv outputs are rounded to
    bf16 before their statistics are taken (as under autocast), the normalised activation and the conv-output gradients are
    rounded once instead of on every read.  Weights are held by reference and read at backward time (stale-graph semantics,
    SURVEY.md Appendix C-1)."""

    @staticmethod
    def forward(ctx, x, s1, h1, s2, h2, w1, w2, eps):
        lib = _lib.load()
        x = to_nhwc(x)
        n, c, h, w = x.shape
        dev = x.device
        st = _stream()
        d = _conv_desc(n, h, w, c, h, w, c, 3, 3, 1, 1, PAD_ZERO, w1)
        d2 = _conv_desc(n, h, w, c, h, w, c, 3, 3, 1, 1, PAD_ZERO, w2)
        hit1, _ = _packed(d, w1, 0, ACT_NONE)
        hit2, _ = _packed(d2, w2, 0, ACT_NONE)
        y1, y2 = (nhwc_empty(n, c, h, w, dev, torch.bfloat16) for _ in range(2))
        _lib.check(lib.srgan_halo16_conv(ctypes.byref(d), 0, _ptr(x), 0, _ptr(hit1.buf), None, _ptr(y1), 1, st), "halo16_conv")
        # (the slab kernels on maps of <= 1024 pixels, the two-pass kernels with 16-bit I/O on the 64 x 64 trunk maps of 256 x 256)
        hh, mean1, rstd1 = _instnorm_fwd(y1, s1, h1, None, ACT_RELU, 0.0, eps, torch.bfloat16)
        _lib.check(lib.srgan_halo16_conv(ctypes.byref(d2), 0, _ptr(hh), 1, _ptr(hit2.buf), None, _ptr(y2), 1, st), "halo16_conv")
        out, mean2, rstd2 = _instnorm_fwd(y2, s2, h2, x, ACT_NONE, 0.0, eps, torch.float32)
        ctx.d1, ctx.d2, ctx.w1, ctx.w2 = d, d2, w1, w2
        ctx.save_for_backward(x, y1, hh, y2, s1, h1, s2, h2, mean1, rstd1, mean2, rstd2)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x, y1, hh, y2, s1, h1, s2, h2, mean1, rstd1, mean2, rstd2 = ctx.saved_tensors
        g = to_nhwc(g)
        st = _stream()
        d1, d2, w1, w2 = ctx.d1, ctx.d2, ctx.w1, ctx.w2
        dy2, ds2, dh2 = _instnorm_bwd(y2, g, s2, h2, mean2, rstd2, ACT_NONE, 0.0, io=True)
        dw2 = _io_wgrad(_PatchRoute, d2, w2, hh, dy2) if ctx.needs_input_grad[6] else None
        hit2, _ = _packed(d2, w2, 1, ACT_NONE)
        dh = torch.empty_like(dy2)
        _lib.check(lib.srgan_halo16_conv(ctypes.byref(d2), 1, _ptr(dy2), 1, _ptr(hit2.buf), None, _ptr(dh), 1, st), "halo16_conv")
        dy1, ds1, dh1 = _instnorm_bwd(y1, dh, s1, h1, mean1, rstd1, ACT_RELU, 0.0, io=True)
        dw1 = _io_wgrad(_PatchRoute, d1, w1, x, dy1) if ctx.needs_input_grad[5] else None
        dx = None
        if ctx.needs_input_grad[0]:
            hit1, _ = _packed(d1, w1, 1, ACT_NONE)
            dx = torch.empty_like(g)
            _lib.check(lib.srgan_halo16_conv(ctypes.byref(d1), 1, _ptr(dy1), 1, _ptr(hit1.buf), _ptr(g), _ptr(dx), 0, st), "halo16_conv")
        return dx, ds1, dh1, ds2, dh2, dw1, dw2, None


# ---- bf16 activation storage outside the residual trunk ----------------------------------------------------------------
# In the bf16 mode, inside a packed-weight scope, the tensors BETWEEN the layers of four chains live in HBM as bf16; the residual
# stream, the statistics, the weight gradients and the master weights stay fp32:
#   generator down / up path (pyfiles/model.py:212-215, 227-231, 245-246), 4x4 / stride-2 convolutions and their norms:
#     norm0 out (fp32 -> bf16) -> down1 (bf16 -> bf16) -> norm1 (bf16 -> bf16) -> down2 (bf16 -> bf16) -> norm2 (bf16 -> fp32) -> trunk
#     trunk out (fp32) -> up0 (fp32 -> bf16) -> norm (bf16 -> bf16) -> up1 (bf16 -> bf16) -> norm (bf16 -> fp32) -> RGB head
#   style-encoder block (pyfiles/model.py:413-437; reflect-padded 3x3 convolutions on 62 / 31 / 15 / 7-pixel maps):
#     x (fp32, residual stream) -> norm1 (fp32 -> bf16) -> conv1 (bf16 -> bf16) -> norm2 (bf16 -> bf16) -> conv2 (bf16 -> bf16)
#       -> AvgPool2d (bf16 -> fp32) -> + shortcut (fp32)
#   discriminator trunk (pyfiles/model.py:302-309): [conv 4x4 / stride 2 without bias -> LeakyReLU] x num_cls with no norm between,
#     each tensor written by one convolution's epilogue and read by the next one's gather;
#   RGB ends: the generator's 7x7 input and output layers, whose 64-channel side may be bf16 (the 3-channel side is fp32).
# The convolutions round their operands to bf16 anyway, so a bf16 norm OUTPUT changes no product; a bf16 conv OUTPUT is what
# torch.autocast stores (its statistics are then taken from the rounded values, as in the residual-block node above).  The
# gradients take the types of the tensors they belong to.  One Function (_ConvBf16Fn) serves every such convolution; a ROUTE names
# the C entry family that runs it: the LDS-resident-patch kernels (csrc/conv_halo16.hip: halo16s / halo16t / halo16s2_wgrad with
# IN16 / OUT16) for the generator, the implicit GEMM with 64-deep K tiles and the vector weight-gradient kernel (csrc/
# conv_igemm.hip: igemm16_kernel, csrc/conv_wgrad.hip: wgrad_kernel<.., IO16>; with fp32 tensors those layers are bound by their own result and by the fp32 -> bf16 conversion
# on the way into LDS, profiles/LOG.md round 4) for the encoder, whichever kernel serves the direction (srgan_conv2d_io_*) for the
# discriminator and the RGB ends.  The norms are the instance-norm kernels with 16-bit I/O (srgan_instnorm_fwd_io / _bwd_io).
STORAGE_BF16 = True               # tests switch it off to compare against the fp32-tensor chain
_NO_D_IO16 = _lib.ab("SRGAN_NO_D_IO16")          # A/B (experiment build only): the discriminators on fp32 tensors
_NO_RGB_IO16 = _lib.ab("SRGAN_NO_RGB_IO16")      # A/B (experiment build only): fp32 tensors around the generator's 7x7 RGB layers
_NO_CONV_IO16 = _lib.ab("SRGAN_NO_CONV_IO16")      # A/B (experiment build only): the encoder's blocks on fp32 tensors


def _is16(t):
    return 1 if t.dtype == torch.bfloat16 else 0


def _to16(t):
    return t if t.dtype == torch.bfloat16 else t.to(torch.bfloat16)


def _io_gate(weight):
    """What every bf16-tensor convolution needs: storage switch on, packed-weight scope, bf16 mode, a device weight."""
    return bool(STORAGE_BF16 and _pack_cache_on and get_compute_dtype() == "bf16" and weight.is_cuda)


def s2_io_applicable(n, ci, hi, wi, co, weight, transposed):
    """True when a 4x4 / stride-2 / pad-1 Conv2d (ci -> co, hi x wi -> half) -- or, transposed=True, the ConvTranspose2d
    (ci -> co, hi x wi -> double) -- can take / write bf16 tensors: bf16 mode, packed-weight scope, all three directions on the
    patch kernels."""
    if not _io_gate(weight):
        return False
    if tuple(weight.shape[2:]) != (4, 4):
        return False
    if transposed:          # conv C of _ConvTranspose2dFn: input = y-space [n, co, 2 hi, 2 wi], output = x-space
        desc = _conv_desc(n, 2 * hi, 2 * wi, co, hi, wi, ci, 4, 4, 2, 1, PAD_ZERO, weight)
    else:
        if hi % 2 or wi % 2:
            return False
        desc = _conv_desc(n, hi, wi, ci, hi // 2, wi // 2, co, 4, 4, 2, 1, PAD_ZERO, weight)
    return bool(_lib.load().srgan_halo16s2_applicable(ctypes.byref(desc)))


def conv_act_io_applicable(n, ci, hi, wi, weight, act, k=4, stride=2, pad=1):
    """True when a Conv2d without bias followed by `act` can take and write bf16 tensors in all three directions (bf16 mode,
    packed-weight scope; ``srgan_conv2d_io_applicable``): the 4x4 / stride-2 / pad-1 layers of the discriminator trunks, and --
    (k, stride, pad) = (7, 1, 3), act none -- the generator's RGB input and output layers, whose 64-channel side may be bf16."""
    if not _io_gate(weight):
        return False
    if (_NO_D_IO16 and k == 4) or (_NO_RGB_IO16 and k == 7):
        return False
    if tuple(weight.shape[2:]) != (k, k) or (stride == 2 and (hi % 2 or wi % 2)):
        return False
    ho, wo = (hi + 2 * pad - k) // stride + 1, (wi + 2 * pad - k) // stride + 1
    desc = _conv_desc(n, hi, wi, ci, ho, wo, weight.shape[0], k, k, stride, pad, PAD_ZERO, weight)
    return bool(_lib.load().srgan_conv2d_io_applicable(ctypes.byref(desc), act))


def conv_io_applicable(n, ci, hi, wi, weight, pad, pad_mode):
    """True when a stride-1 Conv2d without bias (ci -> weight.shape[0], hi x wi) can take and write bf16 tensors in all three
    directions: bf16 mode, packed-weight scope, every direction on the generic bf16 kernels."""
    if not _io_gate(weight) or _NO_CONV_IO16:
        return False
    co, _, kh, kw = weight.shape
    ho, wo = hi + 2 * pad - kh + 1, wi + 2 * pad - kw + 1
    if ho < 1 or wo < 1:
        return False
    desc = _conv_desc(n, hi, wi, ci, ho, wo, co, kh, kw, 1, pad, pad_mode, weight)
    return bool(_lib.load().srgan_igemm16_io_applicable(ctypes.byref(desc), ACT_NONE))


def norm_io_applicable(n, c, h, w):
    return bool(STORAGE_BF16 and get_compute_dtype() == "bf16" and _lib.load().srgan_instnorm_io_applicable(n, h * w, c))


# The routes: ``what`` names the public wrapper in error messages, ``scratch`` says whether the family takes the packed operand's
# per-call scratch, ``conv(desc, kind, src, hit, dst, act, slope, ws, nb)`` runs conv C forward (kind 0) or its input gradient
# (kind 1) and ``wgrad(dd, xin, dy, dw, ws, nb)`` its weight gradient from C's input side and output side, fp32 or bf16.
class _PatchRoute:
    """srgan_halo16_conv / srgan_halo16_wgrad: the generator's down / up path (and the bf16 residual-block node)."""
    what, scratch = "conv2d_s2_io", False

    @staticmethod
    def conv(desc, kind, src, hit, dst, act, slope, ws, nb):
        _lib.check(_lib.load().srgan_halo16_conv(ctypes.byref(desc), kind, _ptr(src), _is16(src), _ptr(hit.buf), None, _ptr(dst),
                                                 _is16(dst), _stream()), "halo16_conv")

    @staticmethod
    def wgrad(dd, xin, dy, dw, ws, nb):
        _lib.check(_lib.load().srgan_halo16_wgrad(ctypes.byref(dd), _ptr(xin), _is16(xin), _ptr(dy), _is16(dy), _ptr(dw), _ptr(ws), nb,
                                                  _stream()), "halo16_wgrad")


class _GenericRoute:
    """srgan_igemm16_conv / srgan_igemm16_wgrad: the style encoder's blocks."""
    what, scratch = "conv2d_io", True

    @staticmethod
    def conv(desc, kind, src, hit, dst, act, slope, ws, nb):
        _lib.check(_lib.load().srgan_igemm16_conv(ctypes.byref(desc), kind, _ptr(src), _is16(src), _ptr(hit.buf), None, _ptr(dst),
                                                  _is16(dst), act, slope, _ptr(ws), nb, _stream()), "igemm16_conv")

    @staticmethod
    def wgrad(dd, xin, dy, dw, ws, nb):
        # both operands as bf16 tensors (the kernel rounds them to bf16 anyway; an fp32 side -- a block boundary -- is rounded by
        # one elementwise pass here)
        x16, g16 = _to16(xin), _to16(dy)
        _lib.check(_lib.load().srgan_igemm16_wgrad(ctypes.byref(dd), _ptr(x16), _ptr(g16), _ptr(dw), _ptr(ws), nb, _stream()),
                   "igemm16_wgrad")


class _AnyRoute:
    """srgan_conv2d_io_fwd / srgan_conv2d_io_dgrad on whatever kernel serves the direction, srgan_halo16_wgrad: the discriminator
    trunks and the RGB ends."""
    what, scratch = "conv2d_act_io", True
    wgrad = staticmethod(_PatchRoute.wgrad)      # (halo16s2_wgrad_kernel takes bf16 x / dy)

    @staticmethod
    def conv(desc, kind, src, hit, dst, act, slope, ws, nb):
        lib = _lib.load()
        if kind == 0:
            _lib.check(lib.srgan_conv2d_io_fwd(ctypes.byref(desc), _ptr(src), _is16(src), _ptr(hit.buf), None, _ptr(dst), _is16(dst), act,
                                               slope, _ptr(ws), nb, _stream()), "conv2d_io_fwd")
        else:
            _lib.check(lib.srgan_conv2d_io_dgrad(ctypes.byref(desc), _ptr(src), _is16(src), _ptr(hit.buf), _ptr(dst), _is16(dst), _ptr(ws),
                                                 nb, _stream()), "conv2d_io_dgrad")


def _io_operand(route, desc, kind, weight, act=ACT_NONE):
    """-> (packed operand, scratch workspace, its bytes) for ``route.conv`` of direction ``kind``; (.., None, 0) when the route
    takes no scratch or the operand wants none."""
    hit, scratch = _packed(desc, weight, kind, act)
    if not (route.scratch and scratch):
        return hit, None, 0
    return hit, workspace(weight.device, scratch), scratch


def _io_wgrad(route, desc, weight, xin, dy):
    return _wgrad_to_sink(desc, (weight,), lambda dd, dw, db, ws, nb: route.wgrad(dd, xin, dy, dw, ws, nb))[0]


class _ConvBf16Fn(Function):
    """Conv2d without bias (+ activation in the epilogue) -- or, ``transposed``, the ConvTranspose2d that is the input-gradient
    form of the conv C whose weight is w viewed as [O = Cin][I = Cout] (as _ConvTranspose2dFn) -- in the bf16 mode with fp32 or
    bf16 tensors on either side, on ``route``.  Backward: an activation's derivative is applied to the incoming gradient by one
    16-bit elementwise pass whose result -- always bf16: both kernels that read it round it to bf16 anyway -- feeds the
    input-gradient and the weight-gradient kernel; dx has x's type.  The weight is held by reference and read at backward time."""

    @staticmethod
    def forward(ctx, x, weight, route, transposed, k, stride, pad, pad_mode, act, slope, out_bf16):
        x = to_nhwc(x)
        n, i, hi, wi = x.shape
        kh, kw = k
        o, i2 = weight.shape[1 if transposed else 0], weight.shape[0 if transposed else 1]
        if i != i2:
            raise _lib.SrganHipError(f"{'conv_transpose2d_io' if transposed else route.what}: input has {i} channels, weight expects {i2}")
        if transposed:      # conv C: input = y-space [n, o, ho, wo], output = x-space [n, i, hi, wi]
            ho, wo = (hi - 1) * stride - 2 * pad + kh, (wi - 1) * stride - 2 * pad + kw
            desc = _conv_desc(n, ho, wo, o, hi, wi, i, kh, kw, stride, pad, pad_mode, weight)
        else:
            ho, wo = (hi + 2 * pad - kh) // stride + 1, (wi + 2 * pad - kw) // stride + 1
            desc = _conv_desc(n, hi, wi, i, ho, wo, o, kh, kw, stride, pad, pad_mode, weight)
        hit, ws, nb = _io_operand(route, desc, int(transposed), weight, act)
        y = nhwc_empty(n, o, ho, wo, x.device, torch.bfloat16 if out_bf16 else torch.float32)
        route.conv(desc, int(transposed), x, hit, y, act, float(slope), ws, nb)
        ctx.desc, ctx.weight, ctx.route, ctx.transposed, ctx.act, ctx.slope = desc, weight, route, transposed, act, slope
        ctx.save_for_backward(x, y if act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y = ctx.saved_tensors
        g = gy = to_nhwc(gy)
        weight = ctx.weight
        if ctx.act != ACT_NONE:
            g = torch.empty_like(gy, dtype=torch.bfloat16)          # (keeps gy's NHWC-dense strides: no copy)
            _lib.check(_lib.load().srgan_act_bwd_io(_ptr(y), _is16(y), _ptr(gy), _is16(gy), _ptr(g), 1, gy.numel(), ctx.act,
                                                    float(ctx.slope), _stream()), "act_bwd_io")
        dx = dw = None
        if ctx.needs_input_grad[0]:
            hit, ws, nb = _io_operand(ctx.route, ctx.desc, int(not ctx.transposed), weight)
            dx = torch.empty_like(x)
            ctx.route.conv(ctx.desc, int(not ctx.transposed), g, hit, dx, ACT_NONE, 0.0, ws, nb)
        if ctx.needs_input_grad[1]:      # C's input side is y-space when transposed
            dw = _io_wgrad(ctx.route, ctx.desc, weight, *((g, x) if ctx.transposed else (x, g)))
        return dx, dw, None, None, None, None, None, None, None, None, None


def conv2d_s2_io(x, weight, out_bf16):
    return _ConvBf16Fn.apply(x, weight, _PatchRoute, False, (4, 4), 2, 1, PAD_ZERO, ACT_NONE, 0.0, bool(out_bf16))


def conv_transpose2d_io(x, weight, out_bf16):
    return _ConvBf16Fn.apply(x, weight, _PatchRoute, True, (4, 4), 2, 1, PAD_ZERO, ACT_NONE, 0.0, bool(out_bf16))


def conv2d_io(x, weight, padding=0, pad_mode=PAD_ZERO, out_bf16=True):
    return _ConvBf16Fn.apply(x, weight, _GenericRoute, False, weight.shape[2:], 1, padding, pad_mode, ACT_NONE, 0.0, bool(out_bf16))


def conv2d_act_io(x, weight, act, slope, out_bf16, k=4, stride=2, pad=1):
    return _ConvBf16Fn.apply(x, weight, _AnyRoute, False, (k, k), stride, pad, PAD_ZERO, act, slope, bool(out_bf16))


def instance_norm_act_io(x, scale, shift, act=ACT_NONE, slope=0.0, eps=1e-5, out_bf16=False):
    """instance_norm_act with an fp32 or bf16 input and a bf16 or fp32 output (no residual); dx has x's type."""
    return _InstNormFn.apply(x, scale, shift, None, act, slope, eps, torch.bfloat16 if out_bf16 else torch.float32)


class _AvgPool2IoFn(Function):
    """AvgPool2d(2, 2) with an fp32 or bf16 input and a bf16 or fp32 output; dx has x's type."""

    @staticmethod
    def forward(ctx, x, out_bf16):
        x = to_nhwc(x)
        n, c, h, w = x.shape
        y = nhwc_empty(n, c, h // 2, w // 2, x.device, torch.bfloat16 if out_bf16 else torch.float32)
        _lib.check(_lib.load().srgan_avgpool2_fwd_io(_ptr(x), _is16(x), _ptr(y), _is16(y), n, h, w, c, _stream()), "avgpool2_fwd_io")
        ctx.shape, ctx.x_dtype = (n, c, h, w), x.dtype
        return y

    @staticmethod
    def backward(ctx, gy):
        n, c, h, w = ctx.shape
        gy = to_nhwc(gy)
        dx = nhwc_empty(n, c, h, w, gy.device, ctx.x_dtype)
        _lib.check(_lib.load().srgan_avgpool2_bwd_io(_ptr(gy), _is16(gy), _ptr(dx), _is16(dx), n, h, w, c, _stream()), "avgpool2_bwd_io")
        return dx, None


def avgpool2_io(x, out_bf16=False):
    return _AvgPool2IoFn.apply(x, bool(out_bf16))


RESBLOCK_BF16_STORAGE = True      # tests/test_ops_gpu.py switches the bf16-storage node off to compare it with the unfused chain


def res_block_bf16_fusable(x, w1, w2, s1, s2):
    """True when ``residual_block_bf16`` applies: bf16 compute mode, packed-weight scope, affine (scale, shift) pairs, both
    convolutions 3x3 square-channel layers on the LDS-resident-patch kernels, a map the slab norm kernels hold."""
    if not (_pack_cache_on and get_compute_dtype() == "bf16" and x.is_cuda and x.dim() == 4 and s1 is not None and s2 is not None):
        return False
    if not RESBLOCK_BF16_STORAGE:
        return False
    n, c, h, w = x.shape
    if tuple(w1.shape) != (c, c, 3, 3) or tuple(w2.shape) != (c, c, 3, 3):
        return False
    lib = _lib.load()
    if not lib.srgan_instnorm_io_applicable(n, h * w, c):
        return False
    desc = _conv_desc(n, h, w, c, h, w, c, 3, 3, 1, 1, PAD_ZERO, w1)
    return bool(lib.srgan_halo16_applicable(ctypes.byref(desc)))


def residual_block_bf16(x, s1, h1, s2, h2, w1, w2, eps=1e-5):
    """cbin2(c2(relu(cbin1(c1(x))))) + x in the bf16 mode with bf16 intermediates -- see _ResBlockBf16Fn."""
    return _ResBlockBf16Fn.apply(x, s1, h1, s2, h2, w1, w2, eps)


def res_block_fusable(x, w1, w2, s1, s2):
    """True when ``residual_block`` applies: packed-weight scope, 32x32 map, affine (scale, shift) pairs present, both
    convolutions 3x3 square-channel layers whose forward, input gradient and weight gradient all dispatch to F(4x4,3x3)."""
    if not (_pack_cache_on and x.is_cuda and x.dim() == 4 and s1 is not None and s2 is not None):
        return False
    if _lib.ab("SRGAN_NO_RESBLOCK_FUSION"):
        return False
    n, c, h, w = x.shape
    if (h, w) != (32, 32) or tuple(w1.shape) != (c, c, 3, 3) or tuple(w2.shape) != (c, c, 3, 3):
        return False
    lib = _lib.load()
    for wt in (w1, w2):
        desc = _conv_desc(n, h, w, c, h, w, c, 3, 3, 1, 1, PAD_ZERO, wt)
        if not (lib.srgan_instnorm_conv_v_applicable(ctypes.byref(desc)) and lib.srgan_instnorm_bwd_vz_applicable(ctypes.byref(desc))
                and lib.srgan_conv2d_wgrad_v_bytes(ctypes.byref(desc))):
            return False
    return True


def residual_block(x, s1, h1, s2, h2, w1, w2, eps=1e-5):
    """cbin2(c2(relu(cbin1(c1(x))))) + x with (scale, shift) = (s1, h1), (s2, h2) -- see _ResBlockFn."""
    return _ResBlockFn.apply(x, s1, h1, s2, h2, w1, w2, eps)


def norm_act_conv_fusable(x, weight):
    """True when ``instance_norm_act_conv`` applies: packed-weight scope, 32x32 map, the conv dispatches to F(4x4,3x3)."""
    if not (_pack_cache_on and x.is_cuda and x.dim() == 4 and weight.dim() == 4 and weight.shape[2] == 3 and weight.shape[3] == 3):
        return False
    if _lib.ab("SRGAN_NO_NORM_CONV_FUSION"):
        return False
    n, c, h, w = x.shape
    if (h, w) != (32, 32) or weight.shape[1] != c:
        return False
    desc = _conv_desc(n, h, w, c, h, w, weight.shape[0], 3, 3, 1, 1, PAD_ZERO, weight)
    return bool(_lib.load().srgan_instnorm_conv_v_applicable(ctypes.byref(desc)))


def instance_norm_act_conv(x, scale, shift, weight, act=ACT_NONE, slope=0.0, eps=1e-5):
    """conv2d(act(instance_norm(x) * scale[n,c] + shift[n,c]), weight, stride 1, pad 1) -- see _NormActConvFn."""
    return _NormActConvFn.apply(x, scale, shift, weight, act, slope, eps)


class _CbinAffineFn(Function):
    @staticmethod
    def forward(ctx, c, W, b, gamma, beta):
        _require_gpu(c, "cbin condition vector")
        c = _dense2d(c)
        n, nc = c.shape
        ch = W.shape[0]
        t = torch.empty(n, ch, dtype=torch.float32, device=c.device)
        scale = torch.empty_like(t)
        shift = torch.empty_like(t)
        _lib.check(_lib.load().srgan_cbin_affine_fwd(_ptr(c), _ptr(W), _ptr(b), _ptr(gamma), _ptr(beta), _ptr(t),
                                                     _ptr(scale), _ptr(shift), n, ch, nc, _stream()), "cbin_affine_fwd")
        ctx.W = W                      # Linear weight: by reference (read at backward time)
        ctx.save_for_backward(c, t, scale)
        return scale, shift

    @staticmethod
    def backward(ctx, dscale, dshift):
        c, t, scale = ctx.saved_tensors
        W = ctx.W
        n, nc = c.shape
        ch = W.shape[0]
        dev = c.device
        if dscale is None:
            dscale = torch.zeros(n, ch, dtype=torch.float32, device=dev)
        if dshift is None:
            dshift = torch.zeros(n, ch, dtype=torch.float32, device=dev)
        dgamma = torch.empty(ch, dtype=torch.float32, device=dev)
        dbeta = torch.empty_like(dgamma)
        dW = torch.empty(ch, nc, dtype=torch.float32, device=dev)
        db = torch.empty_like(dgamma)
        dc = torch.empty(n, nc, dtype=torch.float32, device=dev)
        ws = workspace(dev, n * ch * 4)
        # gamma as seen by the forward = row 0 of the saved scale (the reference multiplies by a
        # repeat()-copy of gamma made at forward time, model.py:64)
        _lib.check(_lib.load().srgan_cbin_affine_bwd(_ptr(c), _ptr(W), _ptr(scale), _ptr(t), _ptr(_dense2d(dscale)),
                                                     _ptr(_dense2d(dshift)), _ptr(dgamma), _ptr(dbeta), _ptr(dW), _ptr(db),
                                                     _ptr(dc), n, ch, nc, _ptr(ws), n * ch * 4, _stream()),
                   "cbin_affine_bwd")
        return dc, dW, db, dgamma, dbeta


def cbin_affine(c, W, b, gamma, beta):
    """-> (scale[N,C], shift[N,C]) with scale = gamma, shift = tanh(c W^T + b)*gamma + beta."""
    return _CbinAffineFn.apply(c, W, b, gamma, beta)


def _cbin_table(records, device):
    """Host records (ctypes buffers) -> one device array (kernel-argument upload: capturable, nothing to keep alive)."""
    return upload_small(b"".join(bytes(r) for r in records), device)


class _CbinAffineMultiFn(Function):
    """cbin_affine of L layers in one launch (backward: two).  params = (W_1, b_1, gamma_1, beta_1, ..., W_L, ...);
    returns (scale_1, shift_1, ..., scale_L, shift_L).  Same kept semantics as _CbinAffineFn: the Linear weights are held by
    reference and read at backward time, gamma in backward is the forward-time copy (row 0 of scale)."""

    @staticmethod
    def forward(ctx, c, *params):
        _require_gpu(c, "cbin condition vector")
        lib = _lib.load()
        c = _dense2d(c)
        n, nc = c.shape
        L = len(params) // 4
        chs = [params[4 * l].shape[0] for l in range(L)]
        dev = c.device
        outs, ts, recs = [], [], []
        nb = lib.srgan_cbin_rec_bytes()
        for l in range(L):
            W, b, g, be = params[4 * l: 4 * l + 4]
            t = torch.empty(n, chs[l], dtype=torch.float32, device=dev)
            scale = torch.empty_like(t)
            shift = torch.empty_like(t)
            rec = (ctypes.c_char * nb)()
            _lib.check(lib.srgan_cbin_rec_fill(ctypes.byref(rec), _ptr(W), _ptr(b), _ptr(g), _ptr(be), _ptr(t), _ptr(scale),
                                               _ptr(shift), None, None, None, None, None, None, None, chs[l]), "cbin_rec_fill")
            recs.append(rec)
            ts.append(t)
            outs += [scale, shift]
        table = _cbin_table(recs, dev)
        _lib.check(lib.srgan_cbin_affine_multi_fwd(_ptr(c), _ptr(table), L, n, max(chs), nc, _stream()), "cbin_affine_multi_fwd")
        ctx.Ws = [params[4 * l] for l in range(L)]          # by reference: read at backward time
        ctx.params = params                                 # the parameter objects (gradient sink: see fused_param_grads)
        ctx.chs = chs
        ctx.save_for_backward(c, *ts, *outs[0::2])
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        lib = _lib.load()
        saved = ctx.saved_tensors
        L = len(ctx.chs)
        c, ts, scales = saved[0], saved[1:1 + L], saved[1 + L:1 + 2 * L]
        n, nc = c.shape
        dev = c.device
        nb = lib.srgan_cbin_rec_bytes()
        zeros = None
        res, recs = [], []
        da = workspace(dev, n * sum(ctx.chs) * 4).view(torch.float32)
        off = 0
        for l in range(L):
            ch = ctx.chs[l]
            dscale, dshift = grads[2 * l], grads[2 * l + 1]
            if dscale is None or dshift is None:
                if zeros is None:
                    zeros = torch.zeros(n, max(ctx.chs), dtype=torch.float32, device=dev)
                dscale = zeros if dscale is None else dscale
                dshift = zeros if dshift is None else dshift
            dscale, dshift = _dense2d(dscale), _dense2d(dshift)
            slots = _sink_slots(*ctx.params[4 * l: 4 * l + 4]) if all(ctx.needs_input_grad[1 + 4 * l: 5 + 4 * l]) else None
            if slots is not None:
                (dW, db, dgamma, dbeta), acc = slots
            else:
                acc = False
                dgamma = torch.empty(ch, dtype=torch.float32, device=dev)
                dbeta = torch.empty_like(dgamma)
                dW = torch.empty(ch, nc, dtype=torch.float32, device=dev)
                db = torch.empty_like(dgamma)
            rec = (ctypes.c_char * nb)()
            _lib.check(lib.srgan_cbin_rec_fill(ctypes.byref(rec), _ptr(ctx.Ws[l]), None, _ptr(scales[l]), None, _ptr(ts[l]), None,
                                               None, _ptr(dscale), _ptr(dshift), _ptr(dgamma), _ptr(dbeta), _ptr(dW), _ptr(db),
                                               da.data_ptr() + off * 4, ch), "cbin_rec_fill")
            if acc:
                _lib.check(lib.srgan_cbin_rec_set_accumulate(ctypes.byref(rec), 1), "cbin_rec_set_accumulate")
            off += n * ch
            recs.append((rec, dscale, dshift))
            res += [None] * 4 if slots is not None else [dW, db, dgamma, dbeta]
        table = _cbin_table([r[0] for r in recs], dev)
        dc = torch.empty(n, nc, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        _lib.check(lib.srgan_cbin_affine_multi_bwd(_ptr(c), _ptr(table), L, n, max(ctx.chs), nc, _ptr(dc), _stream()),
                   "cbin_affine_multi_bwd")
        return (dc, *res)


def cbin_affine_multi(c, layer_params):
    """layer_params: [(W, b, gamma, beta), ...] -> [(scale, shift), ...], one launch for all layers."""
    flat = [p for lp in layer_params for p in lp]
    out = _CbinAffineMultiFn.apply(c, *flat)
    return [(out[2 * l], out[2 * l + 1]) for l in range(len(layer_params))]


# ------------------------------------------------------------------------------------------
# pointwise / pools / heads
# ------------------------------------------------------------------------------------------
class _TanhFn(Function):
    @staticmethod
    def forward(ctx, x):
        _require_gpu(x, "tanh")
        x = to_nhwc(x) if x.dim() == 4 else x.contiguous()
        y = torch.empty_like(x)
        _lib.check(_lib.load().srgan_tanh_fwd(_ptr(x), _ptr(y), x.numel(), _stream()), "tanh_fwd")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gy = to_nhwc(gy) if y.dim() == 4 else gy.contiguous()      # (y.sum().backward() hands over a stride-0 gradient)
        dx = torch.empty_like(y)
        _lib.check(_lib.load().srgan_tanh_bwd(_ptr(y), _ptr(gy), _ptr(dx), y.numel(), _stream()), "tanh_bwd")
        return dx


def tanh(x):
    return _TanhFn.apply(x)


class _ActFn(Function):
    @staticmethod
    def forward(ctx, x, act, slope):
        _require_gpu(x, "activation")
        x = to_nhwc(x) if x.dim() == 4 else x.contiguous()
        y = torch.empty_like(x)
        _lib.check(_lib.load().srgan_act_fwd(_ptr(x), _ptr(y), x.numel(), act, float(slope), _stream()), "act_fwd")
        ctx.act, ctx.slope = act, slope
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gy = to_nhwc(gy) if y.dim() == 4 else gy.contiguous()
        return _act_bwd(y, gy, ctx.act, ctx.slope), None, None


def activation(x, act, slope=0.0):
    return _ActFn.apply(x, act, slope)


class _AddFn(Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = to_nhwc(a), to_nhwc(b)
        y = torch.empty_like(a)
        _lib.check(_lib.load().srgan_add(_ptr(a), _ptr(b), _ptr(y), a.numel(), _stream()), "add")
        return y

    @staticmethod
    def backward(ctx, gy):
        return gy, gy


def add(a, b):
    return _AddFn.apply(a, b)


def _pool_fn(fwd_name, bwd_name, out_hw):
    class _Pool(Function):
        @staticmethod
        def forward(ctx, x):
            x = to_nhwc(x)
            n, c, h, w = x.shape
            ho, wo = out_hw(h, w)
            y = nhwc_empty(n, c, ho, wo, x.device)
            _lib.check(getattr(_lib.load(), fwd_name)(_ptr(x), _ptr(y), n, h, w, c, _stream()), fwd_name)
            ctx.shape = (n, c, h, w)
            return y

        @staticmethod
        def backward(ctx, gy):
            n, c, h, w = ctx.shape
            gy = to_nhwc(gy)
            dx = nhwc_empty(n, c, h, w, gy.device)
            _lib.check(getattr(_lib.load(), bwd_name)(_ptr(gy), _ptr(dx), n, h, w, c, _stream()), bwd_name)
            return dx
    return _Pool


_AvgPool3s2 = _pool_fn("srgan_avgpool3s2_fwd", "srgan_avgpool3s2_bwd", lambda h, w: ((h - 1) // 2 + 1, (w - 1) // 2 + 1))
_AvgPool2 = _pool_fn("srgan_avgpool2_fwd", "srgan_avgpool2_bwd", lambda h, w: (h // 2, w // 2))


def avgpool3s2(x):
    """AvgPool2d(3, stride=2, padding=1, count_include_pad=False)."""
    return _AvgPool3s2.apply(x)


def avgpool2(x):
    """AvgPool2d(2, 2)."""
    return _AvgPool2.apply(x)


class _LreluGapFn(Function):
    @staticmethod
    def forward(ctx, x, slope):
        x = to_nhwc(x)
        n, c, h, w = x.shape
        y = torch.empty(n, c, dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().srgan_lrelu_gap_fwd(_ptr(x), _ptr(y), n, h * w, c, float(slope), _stream()), "lrelu_gap_fwd")
        ctx.slope = slope
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        n, c, h, w = x.shape
        dx = torch.empty_like(x)
        _lib.check(_lib.load().srgan_lrelu_gap_bwd(_ptr(x), _ptr(_dense2d(gy)), _ptr(dx), n, h * w, c, float(ctx.slope),
                                                   _stream()), "lrelu_gap_bwd")
        return dx, None


def lrelu_global_avgpool(x, slope):
    """LeakyReLU(slope) followed by AdaptiveAvgPool2d(1), flattened to [N, C]."""
    return _LreluGapFn.apply(x, slope)


class _LinearFn(Function):
    @staticmethod
    def forward(ctx, x, W, b):
        _require_gpu(x, "linear")
        x = _dense2d(x)
        m, k = x.shape
        n = W.shape[0]
        y = torch.empty(m, n, dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().srgan_linear_fwd(_ptr(x), _ptr(W), _ptr(b), _ptr(y), m, n, k, _stream()), "linear_fwd")
        ctx.W, ctx.has_bias = W, b is not None
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        W = ctx.W
        m, k = x.shape
        n = W.shape[0]
        gy = _dense2d(gy)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        need_w = ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
        dW = torch.empty(n, k, dtype=torch.float32, device=x.device) if need_w else None
        db = torch.empty(n, dtype=torch.float32, device=x.device) if (need_w and ctx.has_bias) else None
        _lib.check(_lib.load().srgan_linear_bwd(_ptr(x), _ptr(W), _ptr(gy), _ptr(dx), _ptr(dW), _ptr(db), m, n, k, _stream()),
                   "linear_bwd")
        return dx, dW, db


def linear(x, W, b=None):
    return _LinearFn.apply(x, W, b)


# ------------------------------------------------------------------------------------------
# fused losses (value + gradient in one launch)
# ------------------------------------------------------------------------------------------
class _MseConstFn(Function):
    @staticmethod
    def forward(ctx, o, target, weight):
        _require_gpu(o, "mse_const")
        o = o if (o.is_contiguous() or is_nhwc_dense(o)) else o.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=o.device)
        d_o = torch.empty_like(o)
        _lib.check(_lib.load().srgan_mse_const(_ptr(o), o.numel(), float(target), float(weight), _ptr(loss), _ptr(d_o),
                                               _stream()), "mse_const")
        ctx.save_for_backward(d_o)
        return loss

    @staticmethod
    def backward(ctx, g):
        (d_o,) = ctx.saved_tensors
        return d_o * g, None, None


def mse_const(o, target, weight=1.0):
    """weight * mean((o - target)^2)."""
    return _MseConstFn.apply(o, target, weight)


class _SoftmaxMseFn(Function):
    @staticmethod
    def forward(ctx, z, label, weight):
        _require_gpu(z, "softmax_mse")
        z = _dense2d(z)
        b, nc = z.shape
        label = label.to(device=z.device, dtype=torch.int64).contiguous()
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        q = torch.empty_like(z)
        dz = torch.empty_like(z)
        _lib.check(_lib.load().srgan_softmax_mse(_ptr(z), _ptr(label), b, nc, float(weight), _ptr(q), _ptr(loss), _ptr(dz),
                                                 _stream()), "softmax_mse")
        ctx.save_for_backward(dz)
        ctx.mark_non_differentiable(q)
        return loss, q

    @staticmethod
    def backward(ctx, g, _gq):
        (dz,) = ctx.saved_tensors
        return dz * g, None, None


def softmax_mse(z, label, weight=1.0):
    """-> (weight * mean((softmax(z) - onehot(label))^2), softmax(z))."""
    return _SoftmaxMseFn.apply(z, label, weight)


# Criterion kinds of the fused loss kernels (SRGAN_CRIT_* of srgan_hip.h): nn.MSELoss, or the slot's binary cross-entropy
# (nn.BCEWithLogitsLoss on the discriminator's raw maps, nn.BCELoss on class probabilities).  losses.criterion_kind maps modules.
CRIT_MSE, CRIT_BCE = 0, 1


def _crit_kind(kind, who):
    if kind not in (CRIT_MSE, CRIT_BCE):
        raise ValueError(f"{who}: kind is ops.CRIT_MSE (0) or ops.CRIT_BCE (1), got {kind!r}")
    return int(kind)


class _CritConstFn(Function):
    @staticmethod
    def forward(ctx, o, target, weight, kind):
        _require_gpu(o, "crit_const")
        o = o if (o.is_contiguous() or is_nhwc_dense(o)) else o.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=o.device)
        d_o = torch.empty_like(o)
        _lib.check(_lib.load().srgan_crit_const(_ptr(o), o.numel(), float(target), float(weight), kind, _ptr(loss), _ptr(d_o),
                                                _stream()), "crit_const")
        ctx.save_for_backward(d_o)
        return loss

    @staticmethod
    def backward(ctx, g):
        (d_o,) = ctx.saved_tensors
        return d_o * g, None, None, None


def crit_const(o, target, weight=1.0, kind=CRIT_MSE):
    """weight * criterion(o, full_like(o, target)): mean((o - target)^2) (CRIT_MSE, the arithmetic of ``mse_const``) or
    nn.BCEWithLogitsLoss on the raw logits o (CRIT_BCE; any real target)."""
    return _CritConstFn.apply(o, target, weight, _crit_kind(kind, "crit_const"))


class _SoftmaxCritFn(Function):
    @staticmethod
    def forward(ctx, z, label, weight, kind):
        _require_gpu(z, "softmax_crit")
        z = _dense2d(z)
        b, nc = z.shape
        label = label.to(device=z.device, dtype=torch.int64).contiguous()
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        q = torch.empty_like(z)
        dz = torch.empty_like(z)
        _lib.check(_lib.load().srgan_softmax_crit(_ptr(z), _ptr(label), b, nc, float(weight), kind, _ptr(q), _ptr(loss),
                                                  _ptr(dz), _stream()), "softmax_crit")
        ctx.save_for_backward(dz)
        ctx.mark_non_differentiable(q)
        return loss, q

    @staticmethod
    def backward(ctx, g, _gq):
        (dz,) = ctx.saved_tensors
        return dz * g, None, None, None


def softmax_crit(z, label, weight=1.0, kind=CRIT_MSE):
    """-> (weight * criterion(softmax(z), onehot(label)), softmax(z)): nn.MSELoss (CRIT_MSE, the arithmetic of ``softmax_mse``)
    or nn.BCELoss with its -100 log clamp and 1e-12 gradient floor (CRIT_BCE)."""
    return _SoftmaxCritFn.apply(z, label, weight, _crit_kind(kind, "softmax_crit"))


class _SoftmaxXentFn(Function):
    @staticmethod
    def forward(ctx, z, label, weight):
        _require_gpu(z, "softmax_xent")
        z = _dense2d(z)
        b, nc = z.shape
        label = label.to(device=z.device, dtype=torch.int64).contiguous()
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        dz = torch.empty_like(z)
        _lib.check(_lib.load().srgan_softmax_xent(_ptr(z), _ptr(label), b, nc, float(weight), _ptr(loss), _ptr(dz),
                                                  _stream()), "softmax_xent")
        ctx.save_for_backward(dz)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dz,) = ctx.saved_tensors
        return dz * g, None, None


def softmax_xent(z, label, weight=1.0):
    """weight * mean cross-entropy of row-softmax(z) against integer labels (nn.CrossEntropyLoss semantics)."""
    return _SoftmaxXentFn.apply(z, label, weight)


class _L1MeanFn(Function):
    @staticmethod
    def forward(ctx, a, b, weight):
        _require_gpu(a, "l1_mean")
        if a.dim() == 4:
            a, b = to_nhwc(a), to_nhwc(b)
        else:
            a, b = a.contiguous(), b.contiguous()
        lib = _lib.load()
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        da = torch.empty_like(a) if need_a else None
        db = torch.empty_like(b) if need_b else None
        nb = lib.srgan_l1_workspace(a.numel())
        ws = workspace(a.device, nb)
        _lib.check(lib.srgan_l1_mean(_ptr(a), _ptr(b), a.numel(), float(weight), _ptr(loss), _ptr(da), _ptr(db), _ptr(ws),
                                     nb, _stream()), "l1_mean")
        ctx.save_for_backward(da, db)
        return loss

    @staticmethod
    def backward(ctx, g):
        da, db = ctx.saved_tensors
        return (da * g if da is not None else None, db * g if db is not None else None, None)


def l1_mean(a, b, weight=1.0):
    """weight * mean(|a - b|)."""
    return _L1MeanFn.apply(a, b, weight)


class _LatentLossFn(Function):
    @staticmethod
    def forward(ctx, mu, n_batch, target, bins, range_max, sigma, w_bkl, w_corr, w_hist):
        _require_gpu(mu, "latent_losses")
        mu = _dense2d(mu)
        b, d = mu.shape
        vals = torch.empty(4, dtype=torch.float32, device=mu.device)
        dmu = torch.empty_like(mu)
        corr = torch.empty(d, d, dtype=torch.float32, device=mu.device)
        _lib.check(_lib.load().srgan_latent_losses(_ptr(mu), b, d, float(n_batch), _ptr(target), bins, float(range_max),
                                                   float(sigma), float(w_bkl), float(w_corr), float(w_hist), _ptr(vals),
                                                   _ptr(dmu), _ptr(corr), _stream()), "latent_losses")
        ctx.save_for_backward(dmu)
        total, parts = vals[3], vals[:3]
        ctx.mark_non_differentiable(parts, corr)
        return total, parts, corr

    @staticmethod
    def backward(ctx, g, _gp, _gc):
        (dmu,) = ctx.saved_tensors
        return (dmu * g,) + (None,) * 8


def latent_losses(mu, n_batch, hist_target, w_bkl, w_corr, w_hist, bins=50, range_max=10.0, sigma=0.2):
    """-> (w_bkl*bKL + w_corr*corr + w_hist*hist, tensor([bKL, corr, hist]), Pearson matrix [d,d])."""
    return _LatentLossFn.apply(mu, n_batch, hist_target, bins, range_max, sigma, w_bkl, w_corr, w_hist)


class _MsePairFn(Function):
    @staticmethod
    def forward(ctx, a, b, weight):
        _require_gpu(a, "mse_pair")
        a, b = a.contiguous(), b.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        _lib.check(_lib.load().srgan_mse_pair(_ptr(a), _ptr(b), a.numel(), float(weight), _ptr(loss), _ptr(da), _ptr(db),
                                              _stream()), "mse_pair")
        ctx.save_for_backward(da, db)
        return loss

    @staticmethod
    def backward(ctx, g):
        da, db = ctx.saved_tensors
        return (da * g if da is not None else None, db * g if db is not None else None, None)


def mse_pair(a, b, weight=1.0):
    """weight * mean((a - b)^2) for two small tensors of equal shape."""
    return _MsePairFn.apply(a, b, weight)


class _CritPairFn(Function):
    @staticmethod
    def forward(ctx, a, b, weight, kind):
        _require_gpu(a, "crit_pair")
        if kind == CRIT_BCE and ctx.needs_input_grad[1]:
            raise _lib.SrganHipError("crit_pair: nn.BCELoss has no gradient w.r.t. its targets on the HIP path")
        a, b = a.contiguous(), b.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        _lib.check(_lib.load().srgan_crit_pair(_ptr(a), _ptr(b), a.numel(), float(weight), kind, _ptr(loss), _ptr(da), _ptr(db),
                                               _stream()), "crit_pair")
        ctx.save_for_backward(da, db)
        return loss

    @staticmethod
    def backward(ctx, g):
        da, db = ctx.saved_tensors
        return (da * g if da is not None else None, db * g if db is not None else None, None, None)


def crit_pair(a, b, weight=1.0, kind=CRIT_MSE):
    """weight * criterion(a, b) for two small tensors of equal shape: nn.MSELoss (CRIT_MSE, the arithmetic of ``mse_pair``) or
    nn.BCELoss of the probabilities a against the targets b (CRIT_BCE; the targets take no gradient)."""
    return _CritPairFn.apply(a, b, weight, _crit_kind(kind, "crit_pair"))


# ---- LeCam regularisation of the discriminator (srgan_amd.lecam; extension, no counterpart in the reference) ----
LC_MAX_SCALES = 4              # anchors per group in the record


def lc_state_new(device, weight, decay, start):
    """Device-resident record {weight, decay, start, updates, a_real[4], a_fake[4], penalty, applied}, all but the settings at zero."""
    return _record_new(_lib.LcState, device, "lc_state_init", float(weight), float(decay), int(start))


def lc_state_set(state, weight, decay, start):
    """Rewrite the three settings between steps; the counter and the anchors stay (a recorded step reads the record)."""
    _record_call("lc_state_set", state, float(weight), float(decay), int(start))


def lc_state_restore(state, updates, a_real, a_fake):
    """Write a checkpoint's count of anchor updates and the anchors (four per group) between steps; everything else stays."""
    a_real, a_fake = [float(v) for v in a_real], [float(v) for v in a_fake]
    if len(a_real) != LC_MAX_SCALES or len(a_fake) != LC_MAX_SCALES:
        raise _lib.SrganHipError(f"lc_state_restore: {len(a_real)} / {len(a_fake)} anchors ({LC_MAX_SCALES} per group)")
    arr = ctypes.c_float * LC_MAX_SCALES
    _record_call("lc_state_restore", state, int(updates), arr(*a_real), arr(*a_fake))


def lc_state_read(state):
    """The record as a dict (the anchors as lists of four floats); synchronises the current stream."""
    rec = _record_read(_lib.LcState, state)
    rec["a_real"], rec["a_fake"] = list(rec["a_real"]), list(rec["a_fake"])
    return rec


def _lecam_arg(lecam, who):
    """``None``, or ``(record, clamp)`` as ``(record, 0 / 1)``"""
    if lecam is None:
        return None
    state, clamp = lecam
    if not torch.is_tensor(state) or state.dtype != torch.uint8 or state.numel() != ctypes.sizeof(_lib.LcState):
        raise _lib.SrganHipError(f"{who}: lecam = (record, clamp) with a record of lc_state_new")
    return state, int(bool(clamp))


def _lecam_launch(lib, lecam, o, d_o, per, rows, pairs, rows_first, vals, i_total, i_out):
    """``srgan_lecam`` behind a loss launch that left its total at ``vals[i_total]`` and ``d_o``: three values to ``vals[i_out:]``"""
    state, clamp = lecam
    if state.device != vals.device:
        raise _lib.SrganHipError("lecam: the record lives on another device than the maps")
    S = len(o)
    arr = ctypes.c_void_p * S
    _lib.check(lib.srgan_lecam(arr(*[t.data_ptr() for t in o]), per, S, rows, pairs, rows_first, clamp, vals.data_ptr() + 4 * i_total,
                               vals.data_ptr() + 4 * i_out, arr(*[t.data_ptr() for t in d_o]), _ptr(state), _stream()), "lecam")


class _DLossesFn(Function):
    @staticmethod
    def forward(ctx, label, rows_first, t_first, t_rest, w_class, n_scales, gan_kind, class_kind, lecam, *tensors):
        outs, logits = tensors[:n_scales], tensors[n_scales:]
        lib = _lib.load()
        dev = outs[0].device
        rows = outs[0].shape[0]
        o = [t if (t.is_contiguous() or is_nhwc_dense(t)) else t.contiguous() for t in outs]
        for t in o:
            _require_gpu(t, "d_losses")
            if t.dim() == 4 and t.shape[1] != 1:
                raise _lib.SrganHipError("d_losses: LSGAN maps must have one channel")
        z = [_dense2d(t) for t in logits]
        nc = z[0].shape[1] if z else 0
        d_o = [torch.empty_like(t) for t in o]
        dz = [torch.empty_like(t) for t in z]
        vals = torch.empty(4 if lecam is None else 7, dtype=torch.float32, device=dev)
        S = n_scales
        arr = ctypes.c_void_p * S
        per = (ctypes.c_longlong * S)(*[t.numel() // rows for t in o])
        if label is not None:
            label = label.to(device=dev, dtype=torch.int64).contiguous()
        _lib.check(lib.srgan_d_losses_crit(arr(*[t.data_ptr() for t in o]), per, arr(*[t.data_ptr() for t in z]) if z else None, S,
                                           rows, int(rows_first), int(nc), _ptr(label), float(t_first), float(t_rest),
                                           float(w_class), gan_kind, class_kind, _ptr(vals), arr(*[t.data_ptr() for t in d_o]),
                                           arr(*[t.data_ptr() for t in dz]) if z else None, _stream()), "d_losses")
        ctx.save_for_backward(*d_o, *dz)
        if lecam is not None:
            # the LeCam term on the same maps, its gradient added into d_o: vals[4:7] = [R, weight R, total + weight R]
            _lecam_launch(lib, lecam, o, d_o, per, rows, rows, int(rows_first), vals, 3, 4)
            total, parts = vals[6], vals[:6]
        else:
            total, parts = vals[3], vals[:3]
        ctx.mark_non_differentiable(parts)
        return total, parts

    @staticmethod
    def backward(ctx, g, _gp):
        grads = torch._foreach_mul(list(ctx.saved_tensors), g)      # one multi-tensor launch
        return (None,) * 9 + tuple(grads)


def d_losses(outs, logits, label, rows_first, t_first, t_rest, w_class, gan_kind=CRIT_MSE, class_kind=CRIT_MSE, lecam=None):
    """Every loss of one discriminator evaluation in one launch -> (total, tensor([gan_first, class, gan_rest])):
    the first ``rows_first`` rows against ``t_first`` (+ softmax / class loss against ``label``), the rest against ``t_rest``;
    total = gan_first + w_class * class + gan_rest, each term the mean over the scales (util.py:457-468).  ``gan_kind``:
    nn.MSELoss (LSGAN, the default) or nn.BCEWithLogitsLoss on the maps; ``class_kind``: nn.MSELoss or nn.BCELoss on softmax(z).
    ``lecam``: ``(record, clamp)`` (``lc_state_new``) adds the LeCam term in a second launch inside the same autograd node:
    -> (total + weight R while the term is applied, tensor([gan_first, class, gan_rest, total, R, weight R or 0])); the first rows
    are the real ones, its gradient rides the buffers the backward scales anyway."""
    logits = list(logits) if logits else []
    return _DLossesFn.apply(label, rows_first, t_first, t_rest, w_class, len(outs), _crit_kind(gan_kind, "d_losses"),
                            _crit_kind(class_kind, "d_losses"), _lecam_arg(lecam, "d_losses"), *outs, *logits)


class _LincombFn(Function):
    @staticmethod
    def forward(ctx, weights, *terms):
        n = len(terms)
        dev = terms[0].device
        terms = [t.reshape(()) for t in terms]
        out = torch.empty((), dtype=torch.float32, device=dev)
        w = (ctypes.c_float * n)(*[float(v) for v in weights])
        _lib.check(_lib.load().srgan_lincomb((ctypes.c_void_p * n)(*[t.data_ptr() for t in terms]), w, n, _ptr(out), _stream()),
                   "lincomb")
        ctx.weights, ctx.dev = [float(v) for v in weights], dev
        ctx.keep = terms                  # the launch reads them asynchronously
        return out

    @staticmethod
    def backward(ctx, g):
        n = len(ctx.weights)
        dx = torch.empty(n, dtype=torch.float32, device=ctx.dev)
        w = (ctypes.c_float * n)(*ctx.weights)
        _lib.check(_lib.load().srgan_lincomb_bwd(w, n, _ptr(g.contiguous()), _ptr(dx), _stream()), "lincomb_bwd")
        return (None,) + tuple(dx[i] if ctx.needs_input_grad[1 + i] else None for i in range(n))


def lincomb(pairs):
    """sum of weight * scalar over [(0-dim device tensor, python float), ...] (<= 16 terms) in one launch; differentiable."""
    pairs = [(t, w) for t, w in pairs if t is not None]
    if len(pairs) > 16:
        return lincomb([(lincomb(pairs[:16]), 1.0)] + pairs[16:])
    for t, _ in pairs:
        _require_gpu(t, "lincomb")
    return _LincombFn.apply([w for _, w in pairs], *[t for t, _ in pairs])


class _KlNormalFn(Function):
    @staticmethod
    def forward(ctx, mu, logvar, weight):
        _require_gpu(mu, "kl_normal")
        mu, logvar = mu.contiguous(), logvar.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=mu.device)
        dmu = torch.empty_like(mu) if ctx.needs_input_grad[0] else None
        dlv = torch.empty_like(logvar) if ctx.needs_input_grad[1] else None
        _lib.check(_lib.load().srgan_kl_normal(_ptr(mu), _ptr(logvar), mu.numel(), float(weight), _ptr(loss), _ptr(dmu), _ptr(dlv),
                                               _stream()), "kl_normal")
        ctx.save_for_backward(dmu, dlv)
        return loss

    @staticmethod
    def backward(ctx, g):
        dmu, dlv = ctx.saved_tensors
        return (dmu * g if dmu is not None else None, dlv * g if dlv is not None else None, None)


def kl_normal(mu, logvar, weight=1.0):
    """weight * -0.5 * sum(1 + logvar - mu^2 - exp(logvar)): the conventional KL term (util_notebook.py:630-634), value and
    both gradients in one launch."""
    return _KlNormalFn.apply(mu, logvar, weight)


class _SoftHistFn(Function):
    @staticmethod
    def forward(ctx, x, bins, lo, hi, sigma):
        _require_gpu(x, "soft_histogram")
        x = x.contiguous()
        lib = _lib.load()
        h = torch.empty(bins, dtype=torch.float32, device=x.device)
        nb = lib.srgan_soft_histogram_workspace(x.numel(), bins)
        ws = workspace(x.device, nb)
        _lib.check(lib.srgan_soft_histogram_fwd(_ptr(x), x.numel(), bins, float(lo), float(hi), float(sigma), _ptr(h),
                                                _ptr(ws), nb, _stream()), "soft_histogram_fwd")
        ctx.cfg = (bins, lo, hi, sigma)
        ctx.save_for_backward(x)
        return h

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        bins, lo, hi, sigma = ctx.cfg
        dx = torch.empty_like(x)
        _lib.check(_lib.load().srgan_soft_histogram_bwd(_ptr(x), _ptr(g.contiguous()), x.numel(), bins, float(lo), float(hi),
                                                        float(sigma), _ptr(dx), _stream()), "soft_histogram_bwd")
        return dx, None, None, None, None


def soft_histogram(x, bins, lo, hi, sigma):
    """Gaussian-kernel soft histogram of a 1-D sample (differentiable)."""
    return _SoftHistFn.apply(x, bins, lo, hi, sigma)


def adam_step_(p, g, m, v, lr, beta1, beta2, eps, step):
    """In-place torch-1.4 Adam on dense buffers, through raw pointers (no autograd version bump)."""
    _require_gpu(p, "adam")
    _lib.check(_lib.load().srgan_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), float(lr), float(beta1),
                                           float(beta2), float(eps), int(step), _stream()), "adam_step")


# ---- device records: state a recorded step reads, written by the host between steps (csrc/records.h; layouts: _lib.*State) ------
def capturing():
    """Is the current stream recording a hipGraph?  (Never without a GPU.)  Records, workspaces and tables are made and rewritten
    between steps only: their owners refuse while this holds."""
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def refuse_in_capture(what):
    """RuntimeError(what) while the current stream records: the caller allocates or rewrites what a recording points at."""
    if capturing():
        raise RuntimeError(what)


def _record_call(entry, state, *args):
    """``srgan_<entry>(state, *args, stream)``: one write of a record on the current stream"""
    _lib.check(getattr(_lib.load(), "srgan_" + entry)(_ptr(state), *args, _stream()), entry)


def _record_new(layout, device, init, *args):
    """A record of ``layout`` on ``device``, written by its ``init`` entry"""
    st = torch.empty(ctypes.sizeof(layout), dtype=torch.uint8, device=device)
    _record_call(init, st, *args)
    return st


def _record_read(layout, state):
    """The record as a dict of its fields, pads left out; synchronises the current stream."""
    torch.cuda.current_stream(state.device).synchronize()
    rec = layout.from_buffer_copy(state.cpu().numpy().tobytes())
    return {name: getattr(rec, name) for name, _ in layout._fields_ if not name.startswith("_")}


class RecordOwner:
    """What the owners of one device record (``self.state``, of ``self.layout``) share: it is made at the first use, never inside
    a hipGraph capture, and a recording bakes its address in."""

    state = None

    def _make_record(self, new, *args):
        refuse_in_capture(f"{type(self).__name__}: the device record would be allocated inside a hipGraph capture; run one eager "
                          "step first")
        self.state = new(*args)

    def _record_ptr(self):
        return self.state.data_ptr() if self.state is not None else 0

    def _record_field(self, name):
        """A float field of the record as a device scalar (a copy; no synchronisation)."""
        return self.state.view(torch.float32)[getattr(self.layout, name).offset // 4].clone()

    def graph_keepalive(self):
        return [self.state] if self.state is not None else []


def adam_state_new(device, lr, beta1, beta2, eps, steps_done):
    """Device-resident Adam record {t, lr, betas, eps, derived step size} seeded with ``steps_done`` completed steps."""
    return _record_new(_lib.AdamState, device, "adam_state_init", float(lr), float(beta1), float(beta2), float(eps), int(steps_done))


def adam_state_set_lr(state, lr):
    _record_call("adam_state_set_lr", state, float(lr))


def adam_multi_dev_(table_dev, n_tensors, max_numel, state):
    """t += 1 on the device, then one launch of torch-1.4 Adam over the tensors of the pointer table (hipGraph-capturable:
    no host value is baked into the launches)."""
    _lib.check(_lib.load().srgan_adam_multi_dev(_ptr(table_dev), int(n_tensors), int(max_numel), _ptr(state), _stream()),
               "adam_multi_dev")


def adam_multi_step_(table_dev, n_tensors, max_numel, lr, beta1, beta2, eps, step):
    """One launch of torch-1.4 Adam over a list of tensors described by a device pointer table (see optim.Adam)."""
    _lib.check(_lib.load().srgan_adam_multi(_ptr(table_dev), int(n_tensors), int(max_numel), float(lr), float(beta1),
                                            float(beta2), float(eps), int(step), _stream()), "adam_multi")


# ---- device-side gradient guard (optim.Adam.enable_grad_guard; extension, no counterpart in the reference) ---------------------
GRAD_GUARD_CHUNK = 4096        # elements per partial of grad_guard_reduce_ (the unit of a reduce table's chunk0 prefix sums)


def _max_norm_arg(max_norm):
    """None -> +inf (no clipping); anything else must be a finite-or-inf float > 0 (the C ABI refuses the rest)."""
    return float("inf") if max_norm is None else float(max_norm)


def grad_guard_state_new(device, max_norm=None):
    """Device-resident record {max_norm, norm, scale, skip, steps, skipped, clipped, pad} with the counters at zero."""
    return _record_new(_lib.GuardState, device, "grad_guard_state_init", _max_norm_arg(max_norm))


def grad_guard_state_set_max_norm(state, max_norm):
    _record_call("grad_guard_state_set_max_norm", state, _max_norm_arg(max_norm))


def grad_guard_state_set_counters(state, steps, skipped, clipped):
    """Write the cumulative counters between steps (resume from a checkpoint); the threshold and the last step's decision stay."""
    _record_call("grad_guard_state_set_counters", state, int(steps), int(skipped), int(clipped))


def grad_guard_state_read(state):
    """The record as a dict; synchronises the current stream (the only host read of the guard)."""
    rec = _record_read(_lib.GuardState, state)
    return dict(rec, max_norm=None if rec["max_norm"] == float("inf") else rec["max_norm"], skip=bool(rec["skip"]))


def grad_guard_workspace_bytes(total_chunks):
    n = int(_lib.load().srgan_grad_guard_workspace(int(total_chunks)))
    if n == 0:
        _lib.check(-1, "grad_guard_workspace")
    return n


def grad_guard_table(grads, device, out=None):
    """Reduce table of a list of contiguous fp32 gradient tensors: three 64-bit words {g, numel, chunk0} per non-empty tensor.
    Returns (device table, n_records, total_chunks)."""
    rows, at, n = [], 0, 0
    for g in grads:
        _require_gpu(g, "grad_guard")
        if not g.is_contiguous():
            raise _lib.SrganHipError("grad_guard: gradients must be contiguous")
        if g.numel():
            rows.extend((g.data_ptr(), g.numel(), at))
            at += -(-g.numel() // GRAD_GUARD_CHUNK)
            n += 1
    if not rows:
        raise _lib.SrganHipError("grad_guard: no gradient elements")
    return upload_small(struct.pack(f"{len(rows)}q", *rows), device, out=out), n, at


def grad_guard_reduce_(table_dev, n_records, total_chunks, ws, state):
    """Two launches: one fp32 partial of sum g^2 per 4096-element chunk of the table's tensors into ``ws``, then the partials
    summed in double in a fixed order and norm / scale / skip / the counters written into the guard record.  hipGraph-capturable;
    nothing comes back to the host."""
    _lib.check(_lib.load().srgan_grad_guard_reduce(_ptr(table_dev), int(n_records), int(total_chunks), _ptr(ws),
                                                   ws.numel() * ws.element_size(), _ptr(state), _stream()), "grad_guard_reduce")


def adam_multi_dev_guard_(table_dev, n_tensors, max_numel, state, guard_state):
    """``adam_multi_dev_`` behind a guard record: t += 1 as always; no store when the record says skip, else the update on
    g * scale (the gradients are not written)."""
    _lib.check(_lib.load().srgan_adam_multi_dev_guard(_ptr(table_dev), int(n_tensors), int(max_numel), _ptr(state),
                                                      _ptr(guard_state), _stream()), "adam_multi_dev_guard")


# ---- exponential moving average of the sampling weights (srgan_amd.ema; extension, no counterpart in the reference) --------
def ema_state_new(device, decay, ramp, n_done):
    """Device-resident record {n, ramp, decay, c} seeded with ``n_done`` completed updates."""
    return _record_new(_lib.EmaState, device, "ema_state_init", float(decay), int(bool(ramp)), int(n_done))


def ema_state_init(state, decay, ramp, n_done):
    """(Re-)seed an existing record in place: a captured step that points at it keeps pointing at it."""
    _record_call("ema_state_init", state, float(decay), int(bool(ramp)), int(n_done))


def ema_state_set_decay(state, decay):
    _record_call("ema_state_set_decay", state, float(decay))


def ema_state_read(state):
    """The record as a dict; synchronises the current stream."""
    return _record_read(_lib.EmaState, state)


def ema_chunk():
    """Elements per work item of ``ema_multi_dev_`` (the unit of a table's chunk0 prefix sums)."""
    return int(_lib.load().srgan_ema_chunk())


def ema_multi_dev_(table_dev, n_records, total_chunks, state):
    """n += 1 and c = 1 - d_n on the device, then ONE launch over the records {dst, src, numel, kind, chunk0} of the table:
    dst += c * (src - dst) (kind 0) or dst <- src bit for bit (kind 1).  hipGraph-capturable; writes through raw pointers."""
    _lib.check(_lib.load().srgan_ema_multi_dev(_ptr(table_dev), int(n_records), int(total_chunks), _ptr(state), _stream()),
               "ema_multi_dev")


# ---- spectral normalisation of conv weights (srgan_amd.spectral; extension, no counterpart in the reference) ----------------
SPECTRAL_REC_WORDS = 16        # 64-bit words per record: {W, W_sn, u, v, sigma, O, K} + seven words srgan_spectral_plan fills


def spectral_table(layers, device):
    """``layers``: [(W ptr, W_sn ptr, u ptr, v ptr, sigma ptr, O, K)] -> (device table, host plan, workspace).  The library checks
    the records and fills in the work lists' prefix sums and the workspace offsets; the table is uploaded once."""
    lib = _lib.load()
    if lib.srgan_spectral_record_bytes() != 8 * SPECTRAL_REC_WORDS:
        raise _lib.SrganHipError("spectral_table: record layout mismatch")
    rows = []
    for rec in layers:
        rows.extend(tuple(int(x) for x in rec) + (0,) * (SPECTRAL_REC_WORDS - len(rec)))
    host = (ctypes.c_char * (8 * len(rows))).from_buffer_copy(struct.pack(f"{len(rows)}Q", *rows))
    plan = (ctypes.c_char * lib.srgan_spectral_plan_bytes())()
    _lib.check(lib.srgan_spectral_plan(ctypes.byref(host), len(layers), ctypes.byref(plan)), "spectral_plan")
    nbytes = lib.srgan_spectral_workspace(ctypes.byref(plan))
    if nbytes == 0:
        _lib.check(-1, "spectral_workspace")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return upload_small(bytes(host), device), plan, ws


def spectral_refresh_(table_dev, plan, ws, iterate=True, n_power_iterations=1, eps=1e-12):
    """sigma and W_sn = W / sigma of every record, after ``n_power_iterations`` power iterations on (u, v) (``iterate``) or from
    the stored (u, v): 4 n + 1 / 3 launches whatever the number of layers.  hipGraph-capturable; writes through raw pointers."""
    _lib.check(_lib.load().srgan_spectral_refresh(_ptr(table_dev), ctypes.byref(plan), int(bool(iterate)), int(n_power_iterations),
                                                  float(eps), _ptr(ws), ws.numel(), _stream()), "spectral_refresh")


def spectral_project_(table_dev, plan, grads_dev, ws):
    """G <- (G - <G, W_sn> u v^T) / sigma in place for the gradient pointers of ``grads_dev`` (one 64-bit word per record, 0 = no
    gradient): 2 launches."""
    _lib.check(_lib.load().srgan_spectral_project(_ptr(table_dev), ctypes.byref(plan), _ptr(grads_dev), _ptr(ws), ws.numel(),
                                                  _stream()), "spectral_project")


# ---- differentiable augmentation of the discriminator's inputs (srgan_amd.augment; extension, no counterpart in the reference) ----
AUG_COLOR, AUG_TRANSLATION, AUG_CUTOUT = 1, 2, 4
AUG_ROW = 8                    # floats per table row: [b, s, a, ty, tx, cy, cx, 0]


def _aug_args(what, xs, table, flags, cut):
    """checked (sources, table, flags, (cut_h, cut_w), (n, h, w)) of one launch"""
    xs = [to_nhwc(x) for x in xs]
    for x in xs:
        _require_gpu(x, what)
        if x.shape[1] != 3 or x.shape[1:] != xs[0].shape[1:]:
            raise _lib.SrganHipError(f"{what}: images of shape {tuple(x.shape)} (three channels, one size for all sources)")
    n = sum(x.shape[0] for x in xs)
    _require_gpu(table, what + " table")
    if tuple(table.shape) != (n, AUG_ROW) or not table.is_contiguous():
        raise _lib.SrganHipError(f"{what}: table of shape {tuple(table.shape)}, a contiguous [{n}, {AUG_ROW}] expected")
    flags = int(flags)
    if flags & ~7:
        raise _lib.SrganHipError(f"{what}: flags = {flags} (colour 1, translation 2, cutout 4)")
    return xs, table, flags, (int(cut[0]), int(cut[1])), (n, xs[0].shape[2], xs[0].shape[3])


def _aug_workspace(lib, flags, n, h, w, device):
    """partial sums of the colour group: (buffer or None, bytes)"""
    if not flags & AUG_COLOR:
        return None, 0
    nb = lib.srgan_diffaugment_workspace(n, h, w)
    if nb == 0:
        _lib.check(-1, "diffaugment_workspace")
    return workspace(device, nb), nb


def _aug_fwd(xs, table, flags, cut, geom, gated=False):
    n, h, w = geom
    lib = _lib.load()
    y = nhwc_empty(n, 3, h, w, xs[0].device)
    ws, nb = _aug_workspace(lib, flags, n, h, w, y.device)
    x1 = xs[1] if len(xs) > 1 else None
    fwd = lib.srgan_diffaugment_fwd_gated if gated else lib.srgan_diffaugment_fwd
    _lib.check(fwd(_ptr(xs[0]), xs[0].shape[0], _ptr(x1), x1.shape[0] if x1 is not None else 0, _ptr(table), _ptr(y), 3, h, w, flags, cut[0],
                   cut[1], _ptr(ws), nb, _stream()), "diffaugment_fwd_gated" if gated else "diffaugment_fwd")
    return y


class _DiffAugmentFn(Function):
    @staticmethod
    def forward(ctx, x, table, flags, cut, gated=False):
        xs, table, flags, cut, geom = _aug_args("diffaugment", [x], table, flags, cut)
        ctx.save_for_backward(table)
        ctx.aug = (flags, cut, geom, bool(gated))
        return _aug_fwd(xs, table, flags, cut, geom, bool(gated))

    @staticmethod
    def backward(ctx, gy):
        (table,) = ctx.saved_tensors
        flags, cut, (n, h, w), gated = ctx.aug
        gy = to_nhwc(gy)
        lib = _lib.load()
        gx = nhwc_empty(n, 3, h, w, gy.device)
        ws, nb = _aug_workspace(lib, flags, n, h, w, gy.device)
        bwd = lib.srgan_diffaugment_bwd_gated if gated else lib.srgan_diffaugment_bwd
        _lib.check(bwd(_ptr(gy), _ptr(table), _ptr(gx), n, 3, h, w, flags, cut[0], cut[1], _ptr(ws), nb, _stream()),
                   "diffaugment_bwd_gated" if gated else "diffaugment_bwd")
        return gx, None, None, None, None


def diffaugment(x, table, flags, cut, gated=False):
    """DiffAugment of a batch ``x[N, 3, H, W]``: colour, then translation, then cutout, whichever of them ``flags`` names
    (AUG_COLOR | AUG_TRANSLATION | AUG_CUTOUT), from one device row ``[b, s, a, ty, tx, cy, cx, 0]`` of ``table[N, 8]`` per sample
    and the cutout window ``cut = (ch, cw)``.  Differentiable in ``x`` only.  Two launches each way with colour on, one without;
    hipGraph-capturable.  ``gated``: slot 7 of a row is a skip mask (an exact float in 0..7, the bits of ``flags``; ``ada_gate``
    writes it) and a group whose bit is set is not applied to that sample, forward and backward: the sample comes out bit for bit
    as the ungated pass gives it with ``flags & ~mask``."""
    return _DiffAugmentFn.apply(x, table, flags, cut, gated)


def diffaugment_cat(xs, table, flags, cut, gated=False):
    """``diffaugment`` of the batch ``cat_batch(xs)`` (one or two sources) written in the same pass -- the discriminator update's
    real and fake halves.  Forward only: an input that requires grad is refused."""
    if not 1 <= len(xs) <= 2:
        raise _lib.SrganHipError(f"diffaugment_cat: {len(xs)} sources (one or two)")
    if any(x.requires_grad for x in xs):
        raise _lib.SrganHipError("diffaugment_cat: an input requires grad; this form has no backward (detach it, or use diffaugment)")
    with torch.no_grad():
        xs, table, flags, cut, geom = _aug_args("diffaugment_cat", list(xs), table, flags, cut)
        return _aug_fwd(xs, table, flags, cut, geom, bool(gated))


# ---- adaptive discriminator augmentation: p on the device (srgan_amd.ada; extension, no counterpart in the reference) -----------
ADA_ROW = 16                   # floats per row the gate reads: [a stage's table row (slots 0..6), -, one uniform per gated group, ...]
ADA_MAX_SCALES = 4


def ada_state_new(device, p, target, step, p_max, interval):
    """Device-resident record {p, target, step, p_max, interval, seen, n_pos, n_neg, n_total, adjustments, last_r}, counters 0."""
    return _record_new(_lib.AdaState, device, "ada_state_init", float(p), float(target), float(step), float(p_max), int(interval))


def ada_state_set(state, target, step, p_max, interval, p=None):
    """Rewrite target, step, p_max, interval and (``p`` given) p between steps; the counters stay (a recorded step reads the
    record)."""
    _record_call("ada_state_set", state, float(target), float(step), float(p_max), int(interval), 0 if p is None else 1,
                 0.0 if p is None else float(p))


def ada_state_set_counters(state, seen, n_pos, n_neg, n_total, adjustments, last_r):
    """Write the heuristic's counters between steps (resume from a checkpoint); p and the settings stay."""
    _record_call("ada_state_set_counters", state, int(seen), int(n_pos), int(n_neg), int(n_total), int(adjustments), float(last_r))


def ada_state_read(state):
    """The record as a dict; synchronises the current stream."""
    return _record_read(_lib.AdaState, state)


def ada_gate(rows, state, n_groups=3):
    """One launch, for any augmentation stage: device rows ``[n, 16]`` (the stage's table row in slots 0..6, the uniforms of its
    ``n_groups`` gated groups -- 3 for DiffAugment (the default), 4 for the geometric stage, 1 to 4 -- from slot 8 on) and the record's p -> the
    table ``[n, 8]`` of the gated ``diffaugment`` / ``geom_augment``: slots 0..6 copied, slot 7 the skip mask whose bit
    g < ``n_groups`` is set iff ``not u_g < p``.  hipGraph-capturable."""
    _require_gpu(rows, "ada_gate rows")
    if rows.dim() != 2 or rows.shape[1] != ADA_ROW or not rows.is_contiguous() or rows.shape[0] == 0:
        raise _lib.SrganHipError(f"ada_gate: rows of shape {tuple(rows.shape)}, a contiguous [n, {ADA_ROW}] expected")
    table = torch.empty(rows.shape[0], AUG_ROW, dtype=torch.float32, device=rows.device)
    _lib.check(_lib.load().srgan_ada_gate(_ptr(rows), _ptr(state), _ptr(table), rows.shape[0], int(n_groups), _stream()), "ada_gate")
    return table


def ada_observe_(outs, rows_first, thr, state):
    """One launch of one workgroup: counts ``v > thr`` / ``v < thr`` / all over the first ``rows_first`` rows of the
    discriminator's maps ``outs`` (fp32, what ``d_losses`` reads in both compute modes) into the record and, every ``interval``-th
    call, moves p.  hipGraph-capturable; nothing comes back to the host."""
    S = len(outs)
    if not 1 <= S <= ADA_MAX_SCALES:
        raise _lib.SrganHipError(f"ada_observe: {S} scales (1 to {ADA_MAX_SCALES})")
    o = []
    for t in outs:
        t = t.detach()
        _require_gpu(t, "ada_observe")
        if t.dim() == 4 and t.shape[1] != 1:
            raise _lib.SrganHipError("ada_observe: the maps must have one channel")
        if t.shape[0] < rows_first:
            raise _lib.SrganHipError(f"ada_observe: a map of {t.shape[0]} rows, {rows_first} real rows asked for")
        o.append(t if (t.is_contiguous() or is_nhwc_dense(t)) else t.contiguous())
    per = (ctypes.c_longlong * S)(*[t.numel() // t.shape[0] for t in o])
    _lib.check(_lib.load().srgan_ada_observe((ctypes.c_void_p * S)(*[t.data_ptr() for t in o]), per, S, int(rows_first), float(thr),
                                             _ptr(state), _stream()), "ada_observe")


# ---- geometric augmentation of the discriminator's inputs (srgan_amd.augment.GeometricAugment; extension) ------------------------
GEOM_FLIP, GEOM_ROT90, GEOM_SCALE, GEOM_ROTATE = 1, 2, 4, 8
GEOM_ROW = 8                   # floats per table row: [fx, k, zoom, cos, sin, 0, 0, mask]


def _geom_args(what, x, table, flags):
    x = to_nhwc(x)
    _require_gpu(x, what)
    if x.shape[1] != 3:
        raise _lib.SrganHipError(f"{what}: images of shape {tuple(x.shape)} (three channels)")
    _require_gpu(table, what + " table")
    if tuple(table.shape) != (x.shape[0], GEOM_ROW) or not table.is_contiguous():
        raise _lib.SrganHipError(f"{what}: table of shape {tuple(table.shape)}, a contiguous [{x.shape[0]}, {GEOM_ROW}] expected")
    flags = int(flags)
    if flags & ~15:
        raise _lib.SrganHipError(f"{what}: flags = {flags} (flip 1, rot90 2, scale 4, rotate 8)")
    return x, flags


class _GeomAugmentFn(Function):
    @staticmethod
    def forward(ctx, x, table, flags, gated=False):
        x, flags = _geom_args("geom_augment", x, table, flags)
        n, _, h, w = x.shape
        ctx.save_for_backward(table)
        ctx.geom = (flags, (n, h, w), bool(gated))
        y = nhwc_empty(n, 3, h, w, x.device)
        _lib.check(_lib.load().srgan_geom_augment_fwd(_ptr(x), _ptr(table), _ptr(y), n, 3, h, w, flags, int(bool(gated)), _stream()),
                   "geom_augment_fwd")
        return y

    @staticmethod
    def backward(ctx, gy):
        (table,) = ctx.saved_tensors
        flags, (n, h, w), gated = ctx.geom
        gy = to_nhwc(gy)
        gx = nhwc_empty(n, 3, h, w, gy.device)
        _lib.check(_lib.load().srgan_geom_augment_bwd(_ptr(gy), _ptr(table), _ptr(gx), n, 3, h, w, flags, int(gated), _stream()),
                   "geom_augment_bwd")
        return gx, None, None, None


def geom_augment(x, table, flags, gated=False):
    """Geometric augmentation of a batch ``x[N, 3, H, W]``: x-flip, 90-degree turns, isotropic scale and rotation, whichever of them
    ``flags`` names (GEOM_FLIP | GEOM_ROT90 | GEOM_SCALE | GEOM_ROTATE), as one bilinear affine warp per sample from one device row
    ``[fx, k, zoom, cos, sin, 0, 0, mask]`` of ``table[N, 8]``; pixels outside the image read 0.  Differentiable in ``x`` only (the
    adjoint is a gather: no atomics, a fixed order).  One launch each way; hipGraph-capturable.  ``flags == 0`` returns ``x``.
    ``gated``: slot 7 of a row is a skip mask (an exact float in 0..15, the bits of ``flags``; ``ada_gate`` writes it) and the
    sample comes out bit for bit as the ungated pass gives it with ``flags & ~mask``."""
    if int(flags) == 0:
        return x
    return _GeomAugmentFn.apply(x, table, flags, gated)


# ---- R1 gradient penalty on real samples (srgan_amd.r1; extension, no counterpart in the reference) ----------------------------
R1_CHUNK = 4096                # floats of a sample per partial sum of |g|^2


def r1_state_new(device, gamma, every, n):
    """Device-resident record {gamma, every, c, penalty, mean_sq_norm, updates, n, pad}, c = gamma * every / n, counters at zero."""
    return _record_new(_lib.R1State, device, "r1_state_init", float(gamma), int(every), int(n))


def r1_state_set(state, gamma, every, n):
    """Rewrite gamma, every, n and c between steps; the counters stay (a recorded step reads the record)."""
    _record_call("r1_state_set", state, float(gamma), int(every), int(n))


def r1_state_set_updates(state, updates):
    """Write the count of penalised updates between steps (resume from a checkpoint); everything else stays."""
    _record_call("r1_state_set_updates", state, int(updates))


def r1_state_read(state):
    """The record as a dict; synchronises the current stream (the only host read of the penalty)."""
    return _record_read(_lib.R1State, state)


def r1_workspace_bytes(n, h, w):
    nb = int(_lib.load().srgan_r1_workspace(int(n), int(h), int(w)))
    if nb == 0:
        _lib.check(-1, "r1_workspace")
    return nb


def r1_seed_(h1, h2, state, u0, ws):
    """One launch: ``u0 = c * (h1 + pool^T(h2))`` and one partial of ``sum g^2`` per 4096 floats of a sample into ``ws``
    (``h1``, ``u0``: [N, 3, H, W]; ``h2``: [N, 3, (H - 1) // 2 + 1, (W - 1) // 2 + 1]; NHWC-dense fp32).  hipGraph-capturable."""
    for t, what in ((h1, "r1_seed h1"), (h2, "r1_seed h2"), (u0, "r1_seed u0")):
        _require_gpu(t, what)
        if not is_nhwc_dense(t):
            raise _lib.SrganHipError(f"{what}: an NHWC-dense tensor expected")
    n, c, h, w = h1.shape
    if tuple(u0.shape) != (n, c, h, w) or tuple(h2.shape) != (n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1):
        raise _lib.SrganHipError(f"r1_seed: h1 {tuple(h1.shape)}, h2 {tuple(h2.shape)}, u0 {tuple(u0.shape)} do not belong together")
    _lib.check(_lib.load().srgan_r1_seed(_ptr(h1), _ptr(h2), _ptr(state), _ptr(u0), n, c, h, w, _ptr(ws),
                                         ws.numel() * ws.element_size(), _stream()), "r1_seed")


def r1_finalize_(ws, n, h, w, state):
    """One workgroup: the partials of ``r1_seed_`` summed in double in a fixed order; mean_sq_norm, penalty and updates written
    into the record.  hipGraph-capturable; nothing comes back to the host."""
    _lib.check(_lib.load().srgan_r1_finalize(_ptr(ws), ws.numel() * ws.element_size(), int(n), int(h), int(w), _ptr(state),
                                             _stream()), "r1_finalize")


# ---- balanced consistency regularisation of the discriminator (srgan_amd.consistency; extension, no counterpart in the reference) ----
CR_FLIP, CR_TRANSLATION = 1, 2
CR_ROW = 8                     # floats per table row: [fx, ty, tx, 0, 0, 0, 0, 0]
CR_MAX_PAIRS = 1024            # SRGAN_CR_MAX_PAIRS of include/srgan_hip.h: the fused loss stages the row means in LDS


def cr_pairs(xs, table, flags):
    """The rows D reads in a consistency-regularised update, in ONE launch: ``xs`` (one or two batches ``[n_i, 3, H, W]``, n rows
    together) -> ``y[2n, 3, H, W]`` whose rows ``[0, n)`` are a bit copy of ``cat_batch(xs)`` and whose row ``n + r`` is ``T`` of row
    ``r``: an x-flip, then an integer translation with zeros shifted in, from one device row ``[fx, ty, tx, 0, ...]`` of
    ``table[n, 8]``, whichever of the two ``flags`` names (CR_FLIP | CR_TRANSLATION).  Forward only: an input that requires grad
    is refused.  hipGraph-capturable."""
    if not 1 <= len(xs) <= 2:
        raise _lib.SrganHipError(f"cr_pairs: {len(xs)} sources (one or two)")
    if any(x.requires_grad for x in xs):
        raise _lib.SrganHipError("cr_pairs: an input requires grad; the pair builder has no backward (detach it)")
    with torch.no_grad():
        xs = [to_nhwc(x) for x in xs]
        for x in xs:
            _require_gpu(x, "cr_pairs")
            if x.dim() != 4 or x.shape[1] != 3 or x.shape[1:] != xs[0].shape[1:] or x.dtype != torch.float32:
                raise _lib.SrganHipError(f"cr_pairs: images of shape {tuple(x.shape)}, {x.dtype} (float32, three channels, one size "
                                         "for all sources)")
        n = sum(x.shape[0] for x in xs)
        _require_gpu(table, "cr_pairs table")
        if tuple(table.shape) != (n, CR_ROW) or not table.is_contiguous() or table.dtype != torch.float32:
            raise _lib.SrganHipError(f"cr_pairs: table of shape {tuple(table.shape)}, a contiguous float32 [{n}, {CR_ROW}] expected")
        flags = int(flags)
        if flags & ~3:
            raise _lib.SrganHipError(f"cr_pairs: flags = {flags} (flip 1, translation 2)")
        _, _, h, w = xs[0].shape
        y = nhwc_empty(2 * n, 3, h, w, xs[0].device)
        x1 = xs[1] if len(xs) > 1 else None
        _lib.check(_lib.load().srgan_cr_pairs_fwd(_ptr(xs[0]), xs[0].shape[0], _ptr(x1), x1.shape[0] if x1 is not None else 0,
                                                  _ptr(table), _ptr(y), 3, h, w, flags, _stream()), "cr_pairs_fwd")
        return y


def cr_state_new(device, lambda_real, lambda_fake, every):
    """Device-resident record {lambda_real, lambda_fake, every, cr_real, cr_fake, updates, pad, pad}, counters at zero."""
    return _record_new(_lib.CrState, device, "cr_state_init", float(lambda_real), float(lambda_fake), int(every))


def cr_state_set(state, lambda_real, lambda_fake, every):
    """Rewrite the weights and every between steps; the counters stay (a recorded step reads the record)."""
    _record_call("cr_state_set", state, float(lambda_real), float(lambda_fake), int(every))


def cr_state_set_updates(state, updates):
    """Write the count of penalised updates between steps (resume from a checkpoint); everything else stays."""
    _record_call("cr_state_set_updates", state, int(updates))


def cr_state_read(state):
    """The record as a dict; synchronises the current stream."""
    return _record_read(_lib.CrState, state)


class _DLossesCrFn(Function):
    @staticmethod
    def forward(ctx, label, rows_first, t_first, t_rest, w_class, n_scales, gan_kind, class_kind, state, pairs_first, lecam, *tensors):
        outs, logits = tensors[:n_scales], tensors[n_scales:]
        lib = _lib.load()
        dev = outs[0].device
        rows = outs[0].shape[0]
        if rows % 2:
            raise _lib.SrganHipError(f"d_losses_cr: maps of {rows} rows; 2 * pairs expected (ops.cr_pairs builds them)")
        o = [t if (t.is_contiguous() or is_nhwc_dense(t)) else t.contiguous() for t in outs]
        for t in o:
            _require_gpu(t, "d_losses_cr")
            if t.dim() == 4 and t.shape[1] != 1:
                raise _lib.SrganHipError("d_losses_cr: the GAN maps must have one channel")
        z = [_dense2d(t) for t in logits]
        nc = z[0].shape[1] if z else 0
        d_o = [torch.empty_like(t) for t in o]
        dz = [torch.empty_like(t) for t in z]
        vals = torch.empty(7 if lecam is None else 10, dtype=torch.float32, device=dev)
        S = n_scales
        arr = ctypes.c_void_p * S
        per = (ctypes.c_longlong * S)(*[t.numel() // rows for t in o])
        if label is not None:
            label = label.to(device=dev, dtype=torch.int64).contiguous()
        _lib.check(lib.srgan_d_losses_cr(arr(*[t.data_ptr() for t in o]), per, arr(*[t.data_ptr() for t in z]) if z else None, S, rows,
                                         int(rows_first), int(nc), _ptr(label), float(t_first), float(t_rest), float(w_class),
                                         gan_kind, class_kind, _ptr(vals), arr(*[t.data_ptr() for t in d_o]),
                                         arr(*[t.data_ptr() for t in dz]) if z else None, rows // 2, int(pairs_first), _ptr(state),
                                         _stream()), "d_losses_cr")
        ctx.save_for_backward(*d_o, *dz)
        if lecam is not None:
            # the LeCam term on the front rows, on top of total_with_cr: vals[7:10] = [R, weight R, total_with_cr + weight R]
            _lecam_launch(lib, lecam, o, d_o, per, rows, rows // 2, int(rows_first), vals, 6, 7)
            total_cr, parts = vals[9], vals[:9]
        else:
            total_cr, parts = vals[6], vals[:6]
        ctx.mark_non_differentiable(parts)
        return total_cr, parts

    @staticmethod
    def backward(ctx, g, _gp):
        grads = torch._foreach_mul(list(ctx.saved_tensors), g)      # one multi-tensor launch
        return (None,) * 11 + tuple(grads)


def d_losses_cr(outs, logits, label, rows_first, t_first, t_rest, w_class, state, gan_kind=CRIT_MSE, class_kind=CRIT_MSE,
                pairs_first=None, lecam=None):
    """``d_losses`` of a consistency-regularised discriminator evaluation, in one launch: the maps hold ``2 P`` rows, row ``r + P``
    the partner ``cr_pairs`` made of row ``r``.  The front ``P`` rows get what ``d_losses`` computes for ``P`` rows; on top come
    ``cr_g = mean_s mean_{r in g} (m_s(r) - m_s(r + P))^2`` over the pairs ``[0, pairs_first)`` (g = first, weight ``lambda_real *
    every`` of the device record ``state``) and the rest (``lambda_fake * every``), ``m_s`` the patch mean of scale s's map
    (``pairs_first``: ``rows_first`` by default).  -> (total_with_cr, tensor([gan_first, class, gan_rest, total, cr_first,
    cr_rest])): the first is what to back-propagate, the six others carry no gradient.  The record takes the two unweighted terms
    and counts the call.  ``lecam``: ``(record, clamp)`` adds the LeCam term of the front ``P`` rows (``rows_first`` of them real)
    in a second launch inside the same autograd node: the first result gains ``weight R`` while the term is applied, the values
    become the six above followed by ``[total_with_cr, R, weight R or 0]``; the back rows' gradient is not touched."""
    logits = list(logits) if logits else []
    return _DLossesCrFn.apply(label, rows_first, t_first, t_rest, w_class, len(outs), _crit_kind(gan_kind, "d_losses_cr"),
                              _crit_kind(class_kind, "d_losses_cr"), state, rows_first if pairs_first is None else pairs_first,
                              _lecam_arg(lecam, "d_losses_cr"), *outs, *logits)


# ---- mode-seeking regularisation of the generator (srgan_amd.diversity; extension, no counterpart in the reference) ----
MS_FORMS = {"msgan": 0, "dsgan": 1}
MS_CHUNK = 4096                # kMsChunk of csrc/diversity.hip: floats of one row per partial sum


def ms_state_new(device, weight, eps, tau):
    """Device-resident record {weight, eps, tau, ms, weighted, d_image, d_latent, updates}, the last five at zero."""
    return _record_new(_lib.MsState, device, "ms_state_init", float(weight), float(eps), float(tau))


def ms_state_set(state, weight, eps, tau):
    """Rewrite the settings between steps; the values and the counter stay (a recorded step reads the record)."""
    _record_call("ms_state_set", state, float(weight), float(eps), float(tau))


def ms_state_restore(state, updates, ms, d_image, d_latent):
    """Write a checkpoint's counter and last values between steps; the settings (and ``weighted``, until the next loss) stay."""
    _record_call("ms_state_restore", state, int(updates), float(ms), float(d_image), float(d_latent))


def ms_state_read(state):
    """The record as a dict; synchronises the current stream."""
    return _record_read(_lib.MsState, state)


def _ms_rows_of(t, what):
    """An operand of the mode-seeking kernels as dense rows: NHWC-dense 4-d (a row slice of a larger batch included) or contiguous."""
    _require_gpu(t, what)
    if t.dim() < 2:
        raise _lib.SrganHipError(f"{what}: a tensor of shape {tuple(t.shape)}; [B, ...] expected")
    if t.dim() == 4:
        return to_nhwc(t)
    return t if t.is_contiguous() else t.contiguous()


def _ms_pair(a, b, what):
    a, b = _ms_rows_of(a, what), _ms_rows_of(b, what)
    if a.shape != b.shape or a.device != b.device:
        raise _lib.SrganHipError(f"{what}: operands of shape {tuple(a.shape)} and {tuple(b.shape)}")
    rows = a.shape[0]
    return a, b, rows, a.numel() // rows


def _ms_partials(a, b, rows, e, what):
    lib = _lib.load()
    nb = lib.srgan_ms_workspace(rows, e)
    if nb == 0:
        raise _lib.SrganHipError(f"{what}: {rows} rows of {e} floats (both > 0, a row under 2^31 - 4096 floats)")
    ws = workspace(a.device, nb)
    _lib.check(lib.srgan_ms_rows(_ptr(a), _ptr(b), rows, e, _ptr(ws), nb, _stream()), "ms_rows")
    return ws, nb


class _ModeSeekingFn(Function):
    @staticmethod
    def forward(ctx, i1, i2, z1, z2, state, form):
        a, b, rows, e = _ms_pair(i1, i2, "mode_seeking")
        _require_gpu(z1, "mode_seeking")
        _require_gpu(z2, "mode_seeking")
        z1, z2 = _dense2d(z1), _dense2d(z2)
        if z1.dim() != 2 or z1.shape != z2.shape or z1.shape[0] != rows:
            raise _lib.SrganHipError(f"mode_seeking: latents of shape {tuple(z1.shape)} and {tuple(z2.shape)} for {rows} images")
        ws, nb = _ms_partials(a, b, rows, e, "mode_seeking")
        vals = torch.empty(2, dtype=torch.float32, device=a.device)
        coef = torch.empty(rows, dtype=torch.float32, device=a.device)
        _lib.check(_lib.load().srgan_ms_finish(_ptr(ws), nb, _ptr(z1), _ptr(z2), rows, e, z1.shape[1], form, _ptr(state), _ptr(vals),
                                               _ptr(coef), _stream()), "ms_finish")
        ctx.save_for_backward(a, b, coef)
        ctx.geom = (rows, e)
        weighted, unweighted = vals[0], vals[1]
        ctx.mark_non_differentiable(unweighted)
        return weighted, unweighted

    @staticmethod
    def backward(ctx, g, _gu):
        a, b, coef = ctx.saved_tensors
        rows, e = ctx.geom
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        d1 = torch.empty_like(a) if need1 else None
        d2 = torch.empty_like(b) if need2 else None
        if need1 or need2:
            g = g.to(torch.float32).contiguous()
            _lib.check(_lib.load().srgan_ms_grad(_ptr(a), _ptr(b), _ptr(coef), _ptr(g), _ptr(d1), _ptr(d2), rows, e, _stream()),
                       "ms_grad")
        return d1, d2, None, None, None, None


def mode_seeking(i1, i2, z1, z2, record, form="msgan"):
    """The mode-seeking term of two translations ``i1``, ``i2`` [B, C, H, W] of the same sources under the latent codes ``z1``,
    ``z2`` [B, d]: ``form="msgan"``: ``dz / (dI + eps dz)`` with ``dI``, ``dz`` the batch means of ``|i1 - i2|`` and ``|z1 - z2|``
    (MSGAN's ``1 / (dI / dz + eps)``); ``form="dsgan"``: ``-mean_i min(r_i, tau)``, ``r_i`` the per-row ratio of the two means.
    ``weight``, ``eps`` and ``tau`` are read from the device ``record`` (``ms_state_new``), which takes the values and counts the
    call.  -> (weight * ms, ms) as device scalars: the first is differentiable in ``i1`` and ``i2`` independently (either may not
    require a gradient: nothing is computed for it), the second carries no gradient; none goes to the latents.  Two launches
    forward, one backward; no atomics, a fixed order of every sum.  hipGraph-capturable."""
    if form not in MS_FORMS:
        raise _lib.SrganHipError(f"mode_seeking: form = {form!r} (one of {sorted(MS_FORMS)})")
    return _ModeSeekingFn.apply(i1, i2, z1.detach(), z2.detach(), record, MS_FORMS[form])


def rowwise_l1(a, b):
    """Per-row ``mean |a - b|`` of two batches of the same shape -> float64 ``[B]``, on the reduction pass of the mode-seeking
    kernels (one launch; a row's float32 partial sums of 4096 terms are then added and divided in float64, so a row whose sums are
    exact gives the exact mean).  No gradient."""
    with torch.no_grad():
        a, b, rows, e = _ms_pair(a.detach(), b.detach(), "rowwise_l1")
        ws, _ = _ms_partials(a, b, rows, e, "rowwise_l1")
        nchunk = -(-e // MS_CHUNK)
        part = ws[:rows * nchunk * 4].view(torch.float32).view(rows, nchunk)
        # (a tensor divisor: dividing by a Python scalar multiplies by its rounded reciprocal on the device)
        return part.to(torch.float64).sum(1) / torch.full((), float(e), dtype=torch.float64, device=a.device)


# ---- structural similarity and PSNR (srgan_amd.structural; extension, no counterpart in the reference) ----
SSIM_MIN_WINDOW, SSIM_MAX_WINDOW = 3, 11       # kSsMinWindow, kSsMaxWindow of csrc/ssim_math.h
SSIM_MAX_CHANNELS = 3                          # kSsMaxC of csrc/ssim.hip
SSIM_TILE = (8, 32)                            # kSsTH, kSsTW: valid positions (forward) / input pixels (gradient) per workgroup


def ssim_taps(window, sigma):
    """The ``window`` taps of the Gaussian of ``sigma`` as Python floats that hold fp32 values: computed and normalised in double on
    the host, rounded to fp32 (csrc/ssim_math.h).  Needs no GPU."""
    if isinstance(window, bool) or not isinstance(window, int):
        raise _lib.SrganHipError(f"ssim_taps: window must be an odd integer in [{SSIM_MIN_WINDOW}, {SSIM_MAX_WINDOW}], got {window!r}")
    arr = (ctypes.c_float * SSIM_MAX_WINDOW)()
    _lib.check(_lib.load().srgan_ssim_taps(window, float(sigma), arr), "ssim_taps")
    return tuple(float(v) for v in arr[:window])


def ss_state_new(device, weight, c1, c2):
    """Device-resident record {weight, c1, c2, term, weighted, updates}, the last three at zero."""
    return _record_new(_lib.SsState, device, "ssim_state_init", float(weight), float(c1), float(c2))


def ss_state_set(state, weight, c1, c2):
    """Rewrite the settings between steps; the last values and the counter stay (a recorded step reads the record)."""
    _record_call("ssim_state_set", state, float(weight), float(c1), float(c2))


def ss_state_restore(state, updates, term, weighted):
    """Write a checkpoint's counter and last values between steps; the settings stay."""
    _record_call("ssim_state_restore", state, int(updates), float(term), float(weighted))


def ss_state_read(state):
    """The record as a dict; synchronises the current stream."""
    return _record_read(_lib.SsState, state)


def _ssim_pair(x, y, what):
    for t in (x, y):
        if not torch.is_tensor(t) or t.dim() != 4:
            raise _lib.SrganHipError(f"{what}: images [N, C, H, W] expected")
        if t.dtype != torch.float32:
            raise _lib.SrganHipError(f"{what}: fp32 images only, got {t.dtype} (the generator's RGB output is fp32 in both compute "
                                     "modes; convert anything else with .float())")
        _require_gpu(t, what)
    if x.shape != y.shape or x.device != y.device:
        raise _lib.SrganHipError(f"{what}: images of shape {tuple(x.shape)} and {tuple(y.shape)}")
    return to_nhwc(x), to_nhwc(y)


class _SsimFn(Function):
    @staticmethod
    def forward(ctx, x, y, state, taps, c1, c2):
        x, y = _ssim_pair(x, y, "ssim")
        if state is not None and (not torch.is_tensor(state) or state.dtype != torch.uint8
                                  or state.numel() != ctypes.sizeof(_lib.SsState) or state.device != x.device):
            raise _lib.SrganHipError("ssim: the record is None or one of ss_state_new on the images' device")
        lib = _lib.load()
        n, c, h, w = x.shape
        window = len(taps)
        need_x, need_y = int(ctx.needs_input_grad[0]), int(ctx.needs_input_grad[1])
        nb = lib.srgan_ssim_workspace(n, c, h, w, window, need_x, need_y)
        if nb == 0:
            raise _lib.SrganHipError(f"ssim: images of shape {tuple(x.shape)} under a window of {window} taps: "
                                     + lib.srgan_last_error().decode(errors="replace"))
        ws = workspace(x.device, nb)
        tarr = (ctypes.c_float * window)(*taps)
        vals = torch.empty(2, dtype=torch.float32, device=x.device)
        values = torch.empty(n, dtype=torch.float32, device=x.device)
        _lib.check(lib.srgan_ssim_map(_ptr(x), _ptr(y), n, c, h, w, window, tarr, _ptr(state), float(c1), float(c2), need_x, need_y,
                                      _ptr(ws), nb, _stream()), "ssim_map")
        _lib.check(lib.srgan_ssim_finish(_ptr(ws), nb, n, c, h, w, window, _ptr(state), _ptr(vals), _ptr(values), _stream()),
                   "ssim_finish")
        # the gradient of weight * term here, with the maps still in the workspace; the backward scales it (as l1_mean)
        dx = torch.empty_like(x) if need_x else None
        dy = torch.empty_like(y) if need_y else None
        if need_x or need_y:
            _lib.check(lib.srgan_ssim_grad(_ptr(x), _ptr(y), n, c, h, w, window, tarr, _ptr(ws), nb, _ptr(state), None, _ptr(dx),
                                           _ptr(dy), _stream()), "ssim_grad")
        ctx.save_for_backward(dx, dy)
        weighted, term = vals[0], vals[1]
        ctx.mark_non_differentiable(term, values)
        return weighted, term, values

    @staticmethod
    def backward(ctx, g, _gt, _gv):
        dx, dy = ctx.saved_tensors
        return (dx * g if dx is not None else None, dy * g if dy is not None else None, None, None, None, None)


def ssim(x, y, state, taps, c1=4e-4, c2=3.6e-3):
    """Structural similarity of two fp32 image batches [N, C, H, W] (C <= 3) under the separable window ``taps`` (``ssim_taps``), valid
    positions only -> (weight * term, term, per-sample values [N]) with ``term = 1 - mean SSIM``: the first is differentiable in
    ``x`` and ``y`` independently (either may not require a gradient: nothing is computed for it), the other two carry none.
    ``weight``, ``c1`` and ``c2`` are read from the device record ``state`` (``ss_state_new``), which takes the values and counts the
    call; ``state=None``: weight 1, the arguments ``c1``, ``c2`` (defaults: k1 = 0.01, k2 = 0.03, data range 2).  Two launches
    without a gradient, three with (the gradient is formed in the forward; the backward multiplies by the incoming scalar); no
    atomics, a fixed order of every sum.  hipGraph-capturable.  Any dtype but fp32 is refused."""
    return _SsimFn.apply(x, y, state, tuple(taps), c1, c2)


def psnr(x, y, data_range=2.0):
    """Per-sample ``10 log10(data_range^2 / mse)`` of two fp32 batches of one shape -> float64 ``[N]`` on the device (``+inf`` where the
    rows are equal): fp32 partial sums of 4096 squared differences, added and divided in float64.  No gradient."""
    with torch.no_grad():
        for t in (x, y):
            _require_gpu(t, "psnr")
        if x.shape != y.shape or x.dim() < 2:
            raise _lib.SrganHipError(f"psnr: operands of shape {tuple(x.shape)} and {tuple(y.shape)}")
        a, b, rows, e = _ms_pair(x.detach(), y.detach(), "psnr")
        lib = _lib.load()
        nb = lib.srgan_psnr_workspace(rows, e)
        if nb == 0:
            raise _lib.SrganHipError(f"psnr: {rows} rows of {e} floats: " + lib.srgan_last_error().decode(errors="replace"))
        ws = workspace(a.device, nb)
        out = torch.empty(rows, dtype=torch.float64, device=a.device)
        _lib.check(lib.srgan_psnr(_ptr(a), _ptr(b), rows, e, float(data_range), _ptr(out), _ptr(ws), nb, _stream()), "psnr")
        return out
