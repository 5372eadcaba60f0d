"""Yardsticks of the batch-norm / CBB tests (csrc/norm_batch.hip): float64 references, seeded case lists, the error measure and a
pure-Python restatement of the kernels' plans (bn_plan, stream_grid).  No GPU code: tests/test_bn_refs_cpu.py pins what is in
here, tests/test_bn_kernels_gpu.py holds the HIP kernels to it through the C ABI.

Error measure and bound are those of tests/small_common.py: max |a - ref| relative to max |ref| of the float64 reference,
bounded by ``max(8 * e32, gamma(L))`` -- e32 the error of the SAME formulas in float32 on the CPU, L the longest sequential
float32 accumulation feeding one output (``path_L`` below, derived from the loops).  No measured number enters the bound.  The
``channel_scales`` input (channels seven decades apart) is measured per channel: every channel's error relative to that
channel's own maximum, the worst channel held to the bound (``check_channels``).

References: the formulas of the header comment of norm_batch.hip and DESIGN.md section 7 written out in torch (never
F.batch_norm), gradients by autograd in the same dtype.  Where the float64 pre-activation lies within rounding of an
activation's kink the upstream gradient is zero (norm_common.kink_mask).
"""
import os

import torch

from tests import norm_common as nc
from tests.small_common import ACT_LRELU, ACT_NONE, ACT_RELU, ceil_div, check, gamma, rel_err, rnd  # noqa: F401
from tests.syncbn_common import BN_CH, bn_plan

EPS = 1e-5
SLOPE = 0.2
MOMENTUM = 0.1
NBT0 = 3                 # num_batches_tracked before the first call
CALLS = 3                # consecutive forwards of one case (the same input: the buffers and the counter move on)
KINK_SHARE_MAX = nc.KINK_SHARE_MAX
ACTS = (ACT_NONE, ACT_RELU, ACT_LRELU)


# ---- the plans of csrc/norm_batch.hip, restated ---------------------------------------------------------------------------------------
def stream_grid(N, HWC):
    """Workgroups per image of bn_apply / bn_bwd_dx (stream_grid of norm_batch.hip): one float4 per lane if that takes fewer,
    about 2048 over the batch otherwise.  The grid changes no result (the passes are elementwise and stride by their own grid),
    and srgan_batchnorm_workspace does not depend on it, so this restatement cannot be observed through the C ABI without a launch
    log; tests/test_bn_refs_cpu.py pins its constants (256 lanes, 2048 workgroups) on three hand-computed grids and against the
    source text."""
    return max(1, min(ceil_div(HWC // 4, 256), max(1, 2048 // N)))


def features(shape):
    """What one call of this shape exercises -- the vocabulary of the cases' ``want`` claims."""
    N, C, H, W = shape
    HW = H * W
    S, rps = bn_plan(N, HW, C)
    f = dict(S=S, rps=rps, ragged_rps=S * rps != HW, empty_last_slab=(S - 1) * rps >= HW)
    # rows one thread (ty = 0 .. 31) of one non-empty slab sums: bn_stats_partial's 4-row unrolled loop runs while four are left,
    # the tail takes the rest
    counts = {ceil_div(max(0, min(HW, (s + 1) * rps) - s * rps - ty), 32) for s in range(S) if s * rps < HW for ty in range(32)}
    f["rows"] = max(counts)
    f["stats_main"] = any(n >= 4 for n in counts)
    f["stats_tail"] = any(n % 4 for n in counts)
    f["stats_main_then_tail"] = any(n >= 4 and n % 4 for n in counts)
    f["idle_rows"] = 0 in counts
    f["channel_tail"] = C % BN_CH != 0
    f["channel_blocks"] = ceil_div(C, BN_CH)
    f["lane_trips"] = ceil_div(N, 64)
    hwc4 = HW * C // 4
    G = stream_grid(N, HW * C)
    f["G"] = G
    f["apply_trips"] = ceil_div(hwc4, G * 256)
    f["apply_ragged"] = hwc4 % (G * 256) != 0
    f["one_partial_block"] = G == 1 and hwc4 < 256
    f["block_per_image"] = N > 2048              # 2048 / N == 0: one workgroup per image whatever its size
    return f


def path_L(shape, backward=False):
    """Longest sequential float32 accumulation feeding one output.  Forward: the rows one thread of bn_stats_partial sums, the 32
    partials a lane adds from LDS, the S slabs and the ceil(N / 64) images one lane of bn_finalize merges, the six shuffle steps
    of the wave.  Backward: bn_bwd_partial and bn_bwd_combine run the same loops; a gradient also rests on the forward's
    statistics, so the backward takes the larger of the two."""
    f = features(shape)
    fwd = f["rows"] + 32 + f["S"] + f["lane_trips"] + 6
    bwd = f["rows"] + 32 + f["S"] + f["lane_trips"] + 6
    return max(fwd, bwd) if backward else fwd


# ---- references ----------------------------------------------------------------------------------------------------------------------
MODES = ("tracked", "cumulative", "untracked", "eval")      # momentum 0.1 / momentum None / no buffers / running statistics


def variant_id(v):
    cbb, mode, flag, act = v
    return f"{'cbb' if cbb else 'bn'} {mode} {('res' if cbb else 'affine')}={int(flag)} act={act}"


def _c4(t):
    return t[None, :, None, None]


def _nc4(t):
    return t[:, :, None, None]


def forward(inp, v, dtype, grad=True):
    """One forward by the plain formulas, in ``dtype``.  v = (cbb, mode, flag, act): flag is `affine` for BN and `res` for CBB.
      mu_c, var_c: biased mean / variance over (n, h, w) -- eval: the running buffers; r_c = (var_c + eps)^-1/2
      BN : y = act((x - mu_c) r_c gamma + beta);  CBB: y = act((x - mu_nc) r_c scale[n,c] + shift[n,c]) (+ res)
    Returns the kernels' outputs (y, mean, rstd, the folded m / a / b of y = act((x - m) a + b)), the pre-activation z, the
    running buffers and the counter after each of CALLS calls (``bufs``), and the leaves for ``gradients``."""
    cbb, mode, flag, act = v
    x = inp["x"].detach().to(dtype).requires_grad_(grad)
    n, c, h, w = x.shape
    M = n * h * w
    if cbb:
        p0, p1 = inp["scale"].to(dtype), inp["shift"].to(dtype)
    elif flag:
        p0, p1 = inp["weight"].to(dtype), inp["bias"].to(dtype)
    else:                                    # no affine: gamma = 1, beta = 0 (exact), so that the sums the kernel writes have a reference
        p0, p1 = torch.ones(c, dtype=dtype), torch.zeros(c, dtype=dtype)
    p0, p1 = p0.detach().clone().requires_grad_(grad), p1.detach().clone().requires_grad_(grad)
    rm = rv = None
    if mode != "untracked":
        rm, rv = inp["rm"].to(dtype), inp["rv"].to(dtype)
    if mode == "eval":
        mu, var = rm, rv
    else:
        xc = x.transpose(0, 1).reshape(c, M)      # a channel's values in one row: the float32 run sums them pairwise
        mu = xc.mean(dim=1)
        var = ((xc - mu[:, None]) ** 2).mean(dim=1)
    rstd = 1.0 / torch.sqrt(var + EPS)
    if cbb:
        m = x.mean(dim=(2, 3))
        z = (x - _nc4(m)) * _c4(rstd) * _nc4(p0) + _nc4(p1)
        a, b = rstd[None, :] * p0, p1
    else:
        m = mu[None, :].expand(n, c)
        z = (x - _c4(mu)) * _c4(rstd) * _c4(p0) + _c4(p1)
        a, b = (rstd * p0)[None, :].expand(n, c), p1[None, :].expand(n, c)
    y = nc._act(z, act)
    if cbb and flag:
        y = y + inp["res"].to(dtype)
    bufs = []
    if mode in ("tracked", "cumulative"):    # F.batch_norm's update: unbiased variance; momentum=None: f = 1 / (count + 1)
        nbt, var_u = NBT0, var.detach() * (M / (M - 1))
        for _ in range(CALLS):
            f = MOMENTUM if mode == "tracked" else 1.0 / (nbt + 1)
            rm, rv, nbt = (1 - f) * rm + f * mu.detach(), (1 - f) * rv + f * var_u, nbt + 1
            bufs.append((rm, rv, nbt))
    out = dict(y=y, z=z.detach(), mean=mu.detach(), rstd=rstd.detach(), m=m.detach(), a=a.detach(), b=b.detach(), bufs=bufs)
    out["leaves"] = (x, p0, p1)
    return out


def gradients(fwd, gy):
    """dx and the parameter gradients (d0 = dweight / dscale, d1 = dbias / dshift) by autograd, added to ``fwd``; y detached."""
    y = fwd["y"]
    dx, d0, d1 = torch.autograd.grad(y, fwd.pop("leaves"), gy.to(y.dtype))
    fwd.update(y=y.detach(), dx=dx, d0=d0, d1=d1)
    return fwd


def kink_keep(f64, f32, act, L):
    """norm_common.kink_mask from the references alone: the forward bound is that of y."""
    return nc.kink_mask(f64["z"], nc.forward_bound(f64["y"].detach(), f32["y"].detach(), L))


def yardstick(inp, v, shape, backward=True):
    """(float64 results, float32 results, upstream gradient with the kink window zeroed)."""
    f64, f32 = forward(inp, v, torch.float64, backward), forward(inp, v, torch.float32, backward)
    gy = None
    if backward:
        gy = inp["gy"]
        if v[3] != ACT_NONE:
            gy = gy * kink_keep(f64, f32, v[3], path_L(shape))
        gradients(f64, gy), gradients(f32, gy)
    else:
        for f in (f64, f32):
            f.pop("leaves")
            f["y"] = f["y"].detach()
    return f64, f32, gy


def kink_share(inp, v, shape):
    """Share of the upstream gradient the kink window zeroes."""
    if v[3] == ACT_NONE:
        return 0.0
    f64, f32 = forward(inp, v, torch.float64, False), forward(inp, v, torch.float32, False)
    return 1.0 - float(kink_keep(f64, f32, v[3], path_L(shape)).double().mean())


def default_input(shape):
    return nc.default_input(shape)


def case_inputs(shape, x=None):
    """float32 CPU tensors (the kernels see exactly these values); the parameters and the initial running buffers are fixed."""
    n, c, h, w = shape
    return dict(x=default_input(shape) if x is None else x, gy=rnd(*shape, seed=4), res=rnd(*shape, seed=5),
                weight=1 + 0.3 * rnd(c, seed=2), bias=0.5 * rnd(c, seed=3),
                scale=1 + 0.3 * rnd(n, c, seed=12), shift=0.5 * rnd(n, c, seed=13),
                rm=0.2 * rnd(c, seed=7) + 0.5, rv=1 + 0.5 * rnd(c, seed=8).abs())


# ---- per-channel measure ---------------------------------------------------------------------------------------------------------------
def channel_errs(a, ref):
    """rel_err over each channel separately: [N, C, H, W] over (n, h, w), [N, C] over n, [C] per element."""
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if a.dim() > 1:
        a, ref = a.transpose(0, 1).flatten(1), ref.transpose(0, 1).flatten(1)
    else:
        a, ref = a[:, None], ref[:, None]
    err = (a - ref).abs().amax(dim=1) / ref.abs().amax(dim=1).clamp_min(1e-30)
    return torch.where(torch.isfinite(a).all(dim=1), err, torch.full_like(err, float("inf")))


def check_channels(kernel, what, got, ref64, ref32, L):
    """small_common.check channel by channel: every channel's error within max(8 * its own e32, gamma(L))."""
    e32, err, g = channel_errs(ref32, ref64), channel_errs(got, ref64), gamma(L)
    bound = torch.clamp_min(8 * e32, g)
    ratio = err / bound
    worst = int(ratio.argmax())
    if os.environ.get("SRGAN_TEST_LOG"):
        print(f"small {kernel} | {what} | e32 {float(e32[worst]):.3e} gamma {g:.3e} err {float(err[worst]):.3e} "
              f"err/bound {float(ratio[worst]):.3f} (channel {worst})")
    assert bool((err <= bound).all()), (f"{kernel} {what}: channel {worst} error {float(err[worst]):.3e} > "
                                        f"max(8 * e32 = {8 * float(e32[worst]):.3e}, gamma = {g:.3e})")


# ---- shape cases ---------------------------------------------------------------------------------------------------------------------
FOLD_ABOVE = 1_000_000
MAX_ELEMENTS = 10_500_000


def _case(shape, want, note=""):
    n, c, h, w = shape
    return dict(name="x".join(map(str, shape)), shape=shape, want=want, grid="fold" if n * c * h * w > FOLD_ABOVE else "full", note=note)


CASES = [
    _case((2, 4, 1, 1), dict(S=1, rps=1, idle_rows=True, stats_main=False, one_partial_block=True), "one pixel per image"),
    _case((1, 4, 5, 7), dict(S=1, G=1, one_partial_block=True, apply_trips=1), "a single partial apply block"),
    _case((3, 36, 9, 9), dict(S=1, channel_tail=True, channel_blocks=2, stats_tail=True, stats_main=False)),
    _case((1, 4, 82, 100), dict(S=128, rps=65, empty_last_slab=True, ragged_rps=True)),
    # S = 32, rps = 128: the full slabs run the unrolled loop alone; in the ragged last slab (119 rows) the lanes below 23 run the
    # unrolled loop and the others the tail
    _case((2, 8, 61, 67), dict(S=32, rps=128, ragged_rps=True, stats_main=True, stats_tail=True, stats_main_then_tail=False)),
    _case((64, 64, 12, 12), dict(S=2, lane_trips=1, channel_tail=False, channel_blocks=2)),
    _case((65, 8, 12, 12), dict(S=2, lane_trips=2)),                    # lane 0 merges images 0 and 64
    _case((130, 36, 16, 16), dict(S=4, rps=64, lane_trips=3, channel_tail=True, channel_blocks=2)),
    _case((130, 8, 32, 32), dict(S=8, rps=128, lane_trips=3, stats_main=True, stats_tail=False)),
    # the single-slab plan of large-batch training: N * ceil(C / 32) >= 1024
    _case((1024, 4, 12, 12), dict(S=1, rps=144, stats_main_then_tail=True, lane_trips=16)),
    _case((1024, 4, 48, 48), dict(S=1, rps=2304, rows=72, G=2, apply_trips=5, apply_ragged=True, lane_trips=16)),
    _case((2049, 4, 2, 2), dict(S=1, G=1, block_per_image=True, lane_trips=33, one_partial_block=True)),
    _case((32, 256, 20, 20), dict(S=4, rps=100, G=64, apply_trips=2, apply_ragged=True, channel_blocks=8)),
]

# (cbb, mode, flag): flag = affine (BN) / res (CBB)
FULL_GRID = [(cbb, mode, flag) for cbb in (False, True) for mode in MODES for flag in (True, False)]
# above FOLD_ABOVE elements: two per activation; over the three activations every mode, both kinds under batch and under running
# statistics, BN with and without affine, CBB with and without residual (tests/test_bn_refs_cpu.py holds this)
FOLD_GRID = {
    ACT_NONE: [(False, "tracked", True), (True, "eval", True)],
    ACT_RELU: [(True, "cumulative", False), (False, "untracked", False)],
    ACT_LRELU: [(False, "eval", True), (True, "tracked", True)],
}


def variants(case, act):
    """The (cbb, mode, flag, act) one test of ``case`` with activation ``act`` runs."""
    return [(*g, act) for g in (FULL_GRID if case["grid"] == "full" else FOLD_GRID[act])]


# ---- hostile inputs ------------------------------------------------------------------------------------------------------------------
HOSTILE_SHAPES = [(4, 8, 64, 64), (65, 8, 12, 12), (1024, 4, 48, 48)]
CHANNEL_SCALES, OUTLIER_FIRST = "channel_scales", "outlier_first"


def _channel_scales(shape):
    """Channel c multiplied by 10 ** (c % 7 - 3): a fault confined to the small channels is invisible relative to the tensor's max."""
    c = shape[1]
    return default_input(shape) * _c4(torch.tensor([10.0 ** (i % 7 - 3) for i in range(c)]))


HOSTILE_INPUTS = dict(nc.HOSTILE_INPUTS)
HOSTILE_INPUTS[CHANNEL_SCALES] = _channel_scales
HOSTILE_CASES = [(shape, kind) for shape in HOSTILE_SHAPES for kind in HOSTILE_INPUTS]
E32_MAX = 1e-5


def hostile_variants(shape):
    """Forward + backward without an activation for both kinds; below FOLD_ABOVE elements also the forward alone with an
    activation (tests/test_norm_kernels_gpu.py's treatment).  (variant, backward)."""
    n, c, h, w = shape
    out = [((False, "tracked", True, ACT_NONE), True), ((True, "tracked", True, ACT_NONE), True)]
    if n * c * h * w <= FOLD_ABOVE:
        out += [((False, "tracked", True, ACT_LRELU), False), ((True, "tracked", True, ACT_RELU), False)]
    return out


# ---- synced entries ------------------------------------------------------------------------------------------------------------------
# (N_global, N_local, C, H, W)
SYNC_CASES = [
    (8, 4, 64, 32, 32),
    (4, 1, 8, 16, 16),
    (65, 65, 8, 12, 12),             # a world of one
    (130, 65, 8, 12, 12),
    (130, 13, 36, 16, 16),           # ten chunks, channel tail
    (130, 13, 260, 4, 4),            # N_local * C / 4 = 845 lanes of bn_sync_pack_scale: four workgroups, the last ragged
    (130, 65, 8, 32, 32),            # the local plan (S = 16) is not the global one (S = 8)
]
SYNC_PLANS_DIFFER = (130, 65, 8, 32, 32)
# training mode only: (cbb, mode, flag, act)
SYNC_VARIANTS = [(False, "tracked", True, ACT_NONE), (False, "cumulative", False, ACT_LRELU), (False, "untracked", True, ACT_RELU),
                 (True, "tracked", False, ACT_RELU), (True, "cumulative", True, ACT_NONE), (True, "untracked", True, ACT_LRELU)]


def sync_id(case):
    return "g{}_l{}_{}x{}x{}".format(*case)


def sync_shape(case):
    ng, nl, c, h, w = case
    return (ng, c, h, w)
