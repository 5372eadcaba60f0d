"""Yardsticks of the instance-norm / CBIN tests (csrc/norm.hip): float64 references, seeded case lists, the error measure and a
pure-Python restatement of the dispatch of srgan_instnorm_fwd / _bwd / _fwd_io / _bwd_io.  No GPU code:
tests/test_norm_refs_cpu.py pins what is in here (the restated dispatch against the launches the library really makes),
tests/test_norm_kernels_gpu.py holds the HIP kernels to it.

Error measure and bound are those of tests/small_common.py: max |a - ref| relative to max |ref| of the float64 reference,
bounded by ``max(8 * e32, gamma(L))`` -- e32 the error of the SAME formulas in float32 on the CPU, L the longest sequential
float32 accumulation feeding one output on the kernel path the case takes (``path_L`` below, derived from the loops).  The bound
is never scaled by a condition number: e32 carries the conditioning.  A tensor stored as bf16 adds half a bf16 ulp of max |ref|
(``bf16_store``); pass-through gradients are compared exactly.

References: the plain formulas of SURVEY.md Appendix F.1 written out in torch (never F.instance_norm), gradients by autograd in
the same dtype.  A bf16 input is rounded first: the reference consumes the rounded values, which are exact in float64.
"""
import functools
import math
import os

import torch
import torch.nn.functional as F

from tests.small_common import (ACT_LRELU, ACT_NONE, ACT_RELU, ceil_div, check as _check, gamma, rel_err, rnd, run,  # noqa: F401
                                yardstick)

EPS = 1e-5
SLOPE = 0.2
KINK_FACTOR = 64
KINK_SHARE_MAX = 0.01


# ---- the dispatch of csrc/norm.hip, restated ---------------------------------------------------------------------------------------
NORM_CH = 32
APPLY_BLOCK_CAP = 8192


def slab_fast(N, HW, C):
    return C % 32 == 0 and HW <= 1024 and N * (C // 32) >= 128


def pow2_fast(C, HW):
    return C >= 4 and 1024 % C == 0 and HW * C // 4 < 2 ** 30


def plan_split(N, HW, C):
    blocks, S = N * ceil_div(C, NORM_CH), 1
    while blocks * S < 1024 and HW // (S * 2) >= 64:
        S *= 2
    return S, ceil_div(HW, S)


def slab_R(HW, pixels_per_pass=64):
    """Rows a thread of a slab kernel holds: 64 pixels per pass (in_fwd_slab, in_bwd_slab), 128 (in_fwd_slab8)."""
    rows = ceil_div(HW, pixels_per_pass)
    sizes = (1, 2, 4, 8, 16) if pixels_per_pass == 64 else (1, 2, 4, 8)
    return next((R for R in sizes if rows <= R), sizes[-1])


def apply_grid(hwc4, N):
    return max(1, min(ceil_div(hwc4, 256), max(1, 2048 // max(1, N))))


def capped_blocks(total, width):
    """(blocks launched, True when the 8192-block cap bites) of in_apply<V4> / in_bwd_apply<V4>: width 4 or 1 elements per thread."""
    want = ceil_div(total // width, 256)
    return min(want, APPLY_BLOCK_CAP), want > APPLY_BLOCK_CAP


def features(shape, x16=False):
    """What one call of this shape exercises -- the vocabulary of the cases' ``want`` claims."""
    N, C, H, W = shape
    HW = H * W
    if slab_fast(N, HW, C):
        return dict(kind="slab", R=slab_R(HW), R8=slab_R(HW, 128), remap=N % 8 == 0, ragged=HW % 64 != 0, full=HW == 1024)
    S, rps = plan_split(N, HW, C)
    stats = "scalar" if C % 4 else ("v8" if x16 and C % 64 == 0 else "v4")
    lanes = 8 if stats == "scalar" else 32
    f = dict(kind="two-pass", stats=stats, S=S, rps=rps, ragged_rps=S * rps != HW, empty_last_split=(S - 1) * rps >= HW)
    # rows one thread of one split sums: the 4-row unrolled loop runs while four are left, the tail takes the rest
    counts = {ceil_div(max(0, min(HW, (s + 1) * rps) - s * rps - ty), lanes) for s in range(S) for ty in range(lanes)}
    f["L"] = (ceil_div(rps, lanes) + lanes + S)
    if stats != "scalar":
        f["stats_main"] = any(n >= 4 for n in counts)
        f["stats_tail"] = any(n % 4 for n in counts)
        f["stats_main_then_tail"] = any(n >= 4 and n % 4 for n in counts)
    total = N * HW * C
    if pow2_fast(C, HW):
        hwc4 = HW * C // 4
        G = apply_grid(hwc4, N)
        step = G * 256
        per_thread = {ceil_div(max(0, hwc4 - j), step) for j in (0, step - 1)}
        f.update(finish="pow2", G=G, one_block=G == 1, apply_main=any(n >= 4 for n in per_thread),
                 apply_tail=any(n % 4 for n in per_thread), apply_main_then_tail=any(n >= 4 and n % 4 for n in per_thread))
    else:
        width = 1 if C % 4 else 4
        blocks, capped = capped_blocks(total, width)
        f.update(finish="apply4" if width == 4 else "apply1", blocks=blocks, capped=capped)
    return f


def path_L(shape, x16=False, y16=False, backward=False):
    """Longest sequential float32 accumulation feeding one output.  Slab kernels: R rows in a thread, the shuffle steps of a
    wave, the waves through LDS -- R + 3 + 8 (in_fwd_slab), R8 + 4 + 8 (in_fwd_slab8), R + 4 + 4 (in_bwd_slab); a gradient also
    rests on the forward's statistics, so the backward takes the larger of the two.  Two-pass: ceil(rps / lanes) rows in a thread,
    the lanes of the workgroup through LDS (32, or 8 in the scalar kernels), the S splits in the finish -- the same loops in both
    directions."""
    f = features(shape, x16)
    if f["kind"] == "slab":
        fwd = f["R8"] + 4 + 8 if (x16 or y16) else f["R"] + 3 + 8
        return max(fwd, f["R"] + 4 + 4) if backward else fwd
    return f["L"]


def _k(name, targs, grid):
    return (name, tuple(int(t) for t in targs), tuple(grid))


def launch_plan(shape, backward, io=None):
    """[(kernel, template arguments, grid)] of one out-of-place call.  ``io``: None = srgan_instnorm_fwd / _bwd, else
    (x_bf16, y_bf16) of srgan_instnorm_fwd_io, (x_bf16, dy_bf16) of srgan_instnorm_bwd_io."""
    N, C, H, W = shape
    HW = H * W
    a16, b16 = io if io is not None else (False, False)
    S, rps = plan_split(N, HW, C)
    if slab_fast(N, HW, C):
        if backward:
            return [_k("in_bwd_slab", (slab_R(HW), a16, b16, a16), (C // 16, N, 1))]
        if a16 or b16:
            return [_k("in_fwd_slab8", (slab_R(HW, 128), a16, b16), (C // 32, N, 1))]
        return [_k("in_fwd_slab", (slab_R(HW), 0, 0), (C // 32, N, 1))]
    g = (ceil_div(C, NORM_CH), S, N)
    if io is not None:
        assert C % 4 == 0 and pow2_fast(C, HW), "srgan_instnorm_io_applicable"
    if C % 4:
        plan = [_k("in_bwd_partial" if backward else "in_stats_partial", (), g)]
    elif a16 and C % 64 == 0:
        plan = [_k("in_bwd_partial_v8", (b16,), (C // 64, S, N))] if backward else [_k("in_stats_partial_v8", (), (C // 64, S, N))]
    else:
        plan = [_k("in_bwd_partial_v4", (a16, b16), g)] if backward else [_k("in_stats_partial_v4", (a16,), g)]
    if pow2_fast(C, HW):
        g2 = (apply_grid(HW * C // 4, N), N, 1)
        return plan + [_k("in_bwd_apply_pow2", (a16, b16, a16), g2) if backward else _k("in_apply_pow2", (a16, b16), g2)]
    plan.append(_k("in_bwd_final" if backward else "in_stats_final", (), (ceil_div(N * C, 256), 1, 1)))
    width = 1 if C % 4 else 4
    blocks, _ = capped_blocks(N * HW * C, width)
    return plan + [_k("in_bwd_apply" if backward else "in_apply", (width == 4,), (blocks, 1, 1))]


# ---- references ----------------------------------------------------------------------------------------------------------------------
def _act(z, act):
    return {ACT_NONE: z, ACT_RELU: torch.relu(z), ACT_LRELU: F.leaky_relu(z, SLOPE)}[act]


def pre_activation(x, scale, shift):
    """mu = <x>, v = <(x - mu)^2> (biased), x_hat = (x - mu) (v + eps)^-1/2, z = x_hat * scale + shift."""
    mu = x.mean(dim=(2, 3), keepdim=True)
    var = ((x - mu) ** 2).mean(dim=(2, 3), keepdim=True)
    z = (x - mu) / torch.sqrt(var + EPS)
    if scale is not None:
        z = z * scale[:, :, None, None] + shift[:, :, None, None]
    return z


def norm_ref(act):
    def fn(x, scale, shift, res):
        y = _act(pre_activation(x, scale, shift), act)
        return y if res is None else y + res
    return fn


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def bf16_store(ref64):
    """Half a bf16 ulp of max |ref|, relative to max |ref|: what one round-to-nearest store of the tensor may add.  bf16 keeps 8
    significant bits, so for max |ref| in [2^k, 2^(k+1)) the ulp is 2^(k-7) and the term lies between 2^-9 (max |ref| at the top
    of its binade) and 2^-8 (at the bottom); a flat 2^-9 is below what a correctly rounded store can meet."""
    m = float(ref64.detach().abs().max())
    return 2.0 ** (math.floor(math.log2(m)) - 8) / m if m > 0 else 0.0


def check(kernel, what, got, ref64, ref32, L, extra=0.0):
    """small_common.check; ``extra`` (a bf16-stored tensor: bf16_store(ref64)) is added to the bound."""
    if not extra:
        return _check(kernel, what, got, ref64, ref32, L)
    e32, err, g = rel_err(ref32, ref64), rel_err(got, ref64), gamma(L)
    bound = max(8 * e32, g) + extra
    if os.environ.get("SRGAN_TEST_LOG"):
        print(f"small {kernel} | {what} | e32 {e32:.3e} gamma {g:.3e} +{extra:.3e} err {err:.3e} err/bound {err / bound:.3f}")
    assert err <= bound, f"{kernel} {what}: error {err:.3e} > max(8 * e32 = {8 * e32:.3e}, gamma = {g:.3e}) + {extra:.3e}"


def forward_bound(y64, y32, L):
    return max(8 * rel_err(y32, y64), gamma(L))


def kink_mask(z64, fwd_bound):
    """True where the upstream gradient is kept: |z| >= tau = 64 * (forward bound) * max |z| in float64.  Nearer to 0 the
    kernel's ReLU / LeakyReLU mask may legitimately differ from the reference's, and one flip moves dshift / dscale by a whole
    term."""
    tau = KINK_FACTOR * fwd_bound * float(z64.abs().max())
    return z64.abs() >= tau


# ---- instance-norm shape cases ---------------------------------------------------------------------------------------------------------
def _case(shape, want, grid="full", note=""):
    return dict(name="x".join(map(str, shape)), shape=shape, want=want, grid=grid, note=note)


# grid: "full" = affine x skip x activation; "fold" (>= 1 M elements) = two of the four (affine, skip) combinations per activation,
# all four over the three activations (param_grid); "cap" (the large-cap cases with hundreds of splits) = affine + skip once:
# forward LeakyReLU, backward without activation (L of these paths is in the hundreds to a thousand, so the kink window of the
# bound would zero more than 1 % of the gradient); "capact" (beyond a cap with few splits) = affine + skip with LeakyReLU, both ways
FP32_CASES = [
    # slab kernels (in_fwd_slab<R> / in_bwd_slab<R>); L = R + 4 + 8
    _case((32, 128, 7, 9), dict(kind="slab", R=1, ragged=True, remap=True)),
    _case((16, 256, 10, 10), dict(kind="slab", R=2, ragged=True, remap=True)),
    _case((64, 64, 15, 15), dict(kind="slab", R=4, ragged=True, remap=True)),
    _case((64, 64, 20, 20), dict(kind="slab", R=8, ragged=True, remap=True), "fold"),
    _case((16, 256, 32, 32), dict(kind="slab", R=16, full=True, remap=True), "fold"),
    _case((12, 352, 31, 31), dict(kind="slab", R=16, ragged=True, remap=False), "fold"),      # N % 8 != 0: the plain grid
    _case((127, 32, 8, 8), dict(kind="two-pass", stats="v4", finish="pow2", S=1)),            # N * C/32 = 127: just below the gate
    # two-pass, scalar statistics (in_stats_partial, in_stats_final, in_apply<false>); L = ceil(rps / 8) + 8 + S
    _case((2, 6, 5, 5), dict(kind="two-pass", stats="scalar", finish="apply1", S=1, capped=False)),
    _case((3, 3, 37, 41), dict(kind="two-pass", stats="scalar", finish="apply1", S=16, ragged_rps=True, capped=False)),
    _case((1, 6, 600, 600), dict(kind="two-pass", stats="scalar", finish="apply1", S=1024, capped=True), "cap"),
    # two-pass, float4 statistics; L = ceil(rps / 32) + 32 + S
    _case((2, 12, 9, 9), dict(kind="two-pass", stats="v4", finish="apply4", S=1, capped=False)),
    _case((3, 96, 40, 40), dict(kind="two-pass", stats="v4", finish="apply4", S=16, stats_main=True, stats_tail=True, capped=False)),
    _case((2, 96, 220, 200), dict(kind="two-pass", stats="v4", finish="apply4", S=256, capped=True), "cap"),
    # beyond the caps with few splits (L = 68 and 44): the mask recomputation of in_bwd_apply in the grid-stride remainder
    _case((64, 6, 75, 75), dict(kind="two-pass", stats="scalar", finish="apply1", S=16, capped=True), "capact"),
    _case((128, 72, 31, 31), dict(kind="two-pass", stats="v4", finish="apply4", S=4, capped=True), "capact"),
    _case((2, 16, 9, 9), dict(kind="two-pass", stats="v4", finish="pow2", S=1, G=2, apply_main=False)),   # last block partial
    # statistics: 288 rows per split, 9 per thread -- two rounds of the unrolled loop, then the tail, in every thread
    _case((64, 64, 48, 48), dict(kind="two-pass", stats="v4", finish="pow2", S=8, G=32, apply_main_then_tail=True,
                                 stats_main_then_tail=True), "fold"),
    _case((1, 4, 82, 100), dict(kind="two-pass", stats="v4", finish="pow2", S=128, rps=65, empty_last_split=True)),
    # S = 32, rps = 128: the full splits run the unrolled loop alone (4 rows per thread); in the ragged last split (119 rows) the
    # lanes below 23 run the unrolled loop and the others the tail.  (rps never exceeds 128 while blocks * S < 1024 ends the
    # doubling; one thread running the loop AND the tail is the 48 x 48 case above.)
    _case((2, 8, 61, 67), dict(kind="two-pass", stats="v4", finish="pow2", S=32, rps=128, ragged_rps=True, stats_main=True,
                               stats_tail=True)),
    _case((2, 1024, 33, 35), dict(kind="two-pass", stats="v4", finish="pow2", S=16), "fold"),
]

# srgan_instnorm_fwd_io / _bwd_io: every (x, y) pairing but fp32 -> fp32 (x_bf16, y_bf16); dy has y's type and dx has x's
IO_PAIRINGS = [(False, True), (True, False), (True, True)]
IO_CASES = [
    _case((3, 64, 40, 40), dict(kind="two-pass", stats="v8", finish="pow2", S=16)),        # in_stats_partial_v8 / in_bwd_partial_v8
    _case((3, 32, 40, 40), dict(kind="two-pass", stats="v4", finish="pow2", S=16)),        # _v4<true>
    _case((32, 128, 8, 16), dict(kind="slab", R8=1, R=2)),                                 # in_fwd_slab8<R>; backward in_bwd_slab<R>
    _case((16, 256, 15, 15), dict(kind="slab", R8=2, R=4)),
    _case((64, 64, 20, 20), dict(kind="slab", R8=4, R=8)),
    _case((16, 256, 31, 31), dict(kind="slab", R8=8, R=16)),
]

IO_COMBOS = [(True, ACT_RELU), (False, ACT_LRELU), (True, ACT_NONE)]      # (affine, activation); the 16-bit entry takes no skip tensor

_COMBOS = [(True, True), (True, False), (False, False), (False, True)]      # (affine, skip)


def param_grid(case, act):
    """(affine, skip) combinations one test of ``case`` with activation ``act`` runs."""
    if case["grid"] == "full":
        return list(_COMBOS)
    if case["grid"] == "fold":      # act 0: (1, 1), (0, 0); act 1: (1, 0), (0, 1); act 2: (0, 0), (1, 1)
        return [_COMBOS[act % 4], _COMBOS[(act + 2) % 4]]
    return [(True, True)]


def case_params(shape, affine, with_res):
    n, c = shape[:2]
    scale = 1 + 0.3 * rnd(n, c, seed=2) if affine else None
    shift = 0.5 * rnd(n, c, seed=3) if affine else None
    res = rnd(*shape, seed=5) if with_res else None
    return scale, shift, res


def default_input(shape):
    return rnd(*shape, seed=1) * 2 + 0.5


def upstream(shape):
    return rnd(*shape, seed=4)


def kink_keep(x, scale, shift, res, act, L):
    """kink_mask of one case, from the references alone: the forward bound is that of y."""
    inputs = (x, scale, shift, res)
    y64, y32 = (run(norm_ref(act), inputs, (False,) * 4, None, dt)[0] for dt in (torch.float64, torch.float32))
    z64 = pre_activation(x.double(), None if scale is None else scale.double(), None if shift is None else shift.double())
    return kink_mask(z64, forward_bound(y64, y32, L))


def norm_yardstick(x, scale, shift, res, act, L, gout):
    """((float64 results, float32 results), upstream gradient with the kink window zeroed): results are
    [y, dx, (dscale, dshift), (dres)] in input order."""
    needs = (True, scale is not None, shift is not None, res is not None)
    if act != ACT_NONE:
        gout = gout * kink_keep(x, scale, shift, res, act, L)
    return yardstick(norm_ref(act), (x, scale, shift, res), needs, gout), gout


# ---- hostile inputs ----------------------------------------------------------------------------------------------------------------------
HOSTILE_SHAPES = [(2, 8, 64, 64), (2, 6, 40, 40), (64, 64, 15, 15)]       # two-pass pow2, two-pass scalar, slab
HOSTILE_BIG = ((2, 8, 128, 128), "outlier_first")
SIGMA, CENTRE = 0.1, 0.3


def _narrow(shape):
    return rnd(*shape, seed=1) * SIGMA + CENTRE


def _outlier_first(shape):
    x = _narrow(shape)
    x[:, :, 0, 0] = CENTRE + 100 * SIGMA
    return x


def _outlier_last(shape):
    x = _narrow(shape)
    x[:, :, -1, -1] = CENTRE + 100 * SIGMA
    return x


def _row_offset(shape):
    x = _narrow(shape)
    x[:, :, 0, :] += 8 * SIGMA
    return x


def _constant_channel(shape):
    x = default_input(shape)
    x[:, 1] = 0.3
    return x


HOSTILE_INPUTS = {
    "default": default_input,                                       # randn * 2 + 0.5
    "offset_mean": lambda shape: rnd(*shape, seed=1) * 0.25 + 16,
    "constant_channel": _constant_channel,                          # zero variance in one channel of every image
    "outlier_first": _outlier_first,                                # pixel (0, 0) 100 sigma away: the two-pass kernels' shift sample
    "outlier_last": _outlier_last,
    "row_offset": _row_offset,                                      # first image row 8 sigma up
}
OUTLIER_FIRST = "outlier_first"
HOSTILE_CASES = [(shape, kind) for shape in HOSTILE_SHAPES for kind in HOSTILE_INPUTS] + [HOSTILE_BIG]


def hostile_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else v


# ---- CBIN affine ---------------------------------------------------------------------------------------------------------------------------
CBIN_N = (1, 7, 64, 65, 130)            # lanes stride over the batch above 64
CBIN_C = (1, 6, 24, 64, 257)            # one to many waves per block, the ch >= C tail
CBIN_NUM_CON = (1, 12, 16)
CBIN_NUM_CON_REFUSED = 17
# 17 layers of mixed widths: the second pass of the l0 loop of cbin_affine_multi_bwd_c holds one layer
CBIN_MULTI_WIDTHS = (24, 64, 256, 1, 6, 257, 64, 128, 24, 32, 100, 64, 256, 7, 16, 64, 33)
CBIN_MULTI_NO_SCALE_GRAD = 5            # this layer's scale output takes no gradient


def cbin_params(C, num_con, seed):
    return ((rnd(C, num_con, seed=seed) * 0.3), rnd(C, seed=seed + 1) * 0.1, 1 + 0.2 * rnd(C, seed=seed + 2), 0.1 * rnd(C, seed=seed + 3))


def cbin_ref(c, W, b, gam, bet):
    """F.1: t = tanh(c W^T + b); scale = gamma (per sample), shift = t * gamma + beta."""
    t = torch.tanh(c @ W.t() + b)
    return gam[None, :].expand(c.shape[0], -1), t * gam + bet


def cbin_L_params(N, visits=1):
    return visits * (ceil_div(N, 64) + 6)


def cbin_L_dc(C, layers=0):
    return ceil_div(C, 64) + 6 + layers


@functools.lru_cache(maxsize=None)
def cbin_yardstick(N, C, num_con):
    """(inputs, float64 results, float32 results) of the loss (scale * g1).sum() + (shift * g2).sum(): results are
    [scale, shift, dc, dW, db, dgamma, dbeta]."""
    c = rnd(N, num_con, seed=1)
    params = cbin_params(C, num_con, 10)
    g1, g2 = rnd(N, C, seed=6), rnd(N, C, seed=7)
    out = []
    for dt in (torch.float64, torch.float32):
        xs = [t.detach().clone().to(dt).requires_grad_(True) for t in (c, *params)]
        scale, shift = cbin_ref(*xs)
        grads = torch.autograd.grad((scale * g1.to(dt)).sum() + (shift * g2.to(dt)).sum(), xs)
        out.append([scale.detach(), shift.detach(), *grads])
    return (c, params, g1, g2), out[0], out[1]
