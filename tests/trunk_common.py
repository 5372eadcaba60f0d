"""Yardsticks of the fused residual-trunk tests: the instance-norm kernels of csrc/conv_wino43.hip that write the transformed
images of the F(4x4,3x3) layer next to them (in_fwd_slab_v16_kernel, in_bwd_slab_vz_kernel) and the multiply kernels that run on
those images (wino43_kernel on a ready V image, wino43_wgrad_kernel on a ready Z image) -- the entries srgan_instnorm_fwd_v,
srgan_conv2d_fwd_from_v, srgan_instnorm_bwd_vz, srgan_conv2d_dgrad_from_v and srgan_conv2d_wgrad_vz of include/srgan_hip.h.
No GPU code: tests/test_trunk_refs_cpu.py pins what is in here (the restated sizes and applicability against the library's host
functions, the kink window, the reference against oracle/nets.py), tests/test_trunk_kernels_gpu.py holds the kernels to it.

Three compositions, each against float64 (e32 = the same formulas in float32 on the CPU):
  forward          y  = act2(conv3x3(act(z)) + bias), z = pre_activation(x, scale, shift); mean and rstd of x
  input gradient   dx = conv_dgrad(dy) + res, dy = the norm's backward of the upstream gradient; dscale, dshift
  weight gradient  dw = conv_wgrad(x_conv, dy)
Convolution results are held by conv_common.check (max(BOUND[what], 8 * e32)), statistics and dscale / dshift by
norm_common.check (max(8 * e32, gamma(L))).  Every tensor handed to an entry is the test's own, the upstream gradient included:
it is zero where the float64 pre-activation lies within rounding of the activation's kink (norm_common.kink_keep), so no
comparison has to tolerate a flipped mask.  The backward takes mean / rstd from the float64 reference rounded to float32, so it
does not rest on the forward kernel.

All maps are 32 x 32, all layers 3x3 / stride 1 / zero pad 1; (N, I, O) = batch, input and output channels of the convolution.
The forward norm runs over the I channels of the convolution's input, the backward norm over the O channels of its output."""
import functools

import torch

from tests import conv_common as cc
from tests import norm_common as nc
from tests.norm_common import ACT_LRELU, ACT_NONE, ACT_RELU, EPS, SLOPE, ceil_div      # noqa: F401
from tests.small_common import act_ref

HW = 32
MAX_ELEMS = 2 << 20

# Longest sequential float32 accumulation feeding one statistic, from the loops of in_fwd_slab_v16_kernel / in_bwd_slab_vz_kernel
# (as norm_common.path_L derives it for the slab kernels of norm.hip): a thread sums R = 16 rows (1024 pixels over 64 pixel rows
# of 4 lanes each), slab_sum43_q4 adds four shuffle steps (xor 4, 8, 16, 32: the lanes that share a channel quad) and then the
# partial sums of the four waves from LDS -- 16 + 4 + 4.  The backward's two plane sums take the same route.
L = 16 + 4 + 4


# ---- host geometry of csrc/conv_wino43.hip / conv_wino.hip / conv_dispatch.hip, restated ------------------------------------------
W4T, W4C, W4BLK = 64, 8, 36 * 512       # tiles per workgroup, reduce channels per chunk, floats of one (tile block, chunk) image


def wino43_scratch_floats(T, C):
    return ceil_div(T, W4T) * (C // W4C) * W4BLK


def v_bytes(N, C):
    """The V image of N images of 8 x 8 tiles with C reduce channels: srgan_conv2d_packed_scratch(d, 0) with C = I, (d, 1) with C = O."""
    return wino43_scratch_floats(N * (HW // 4) * (HW // 4), C) * 4


def z_bytes(N, O):
    """srgan_instnorm_bwd_vz_z_bytes: [O / 32][ntc = 8 N tile chunks][36 positions][256] floats."""
    return (O // 32) * 8 * N * 36 * 256 * 4


def f43(N, C, Nn):
    """wino_variant == 3 with the size thresholds off (SRGAN_WINOGRAD_THRESHOLD_SCALE=0) for a 3x3 / stride-1 / zero-pad-1 layer on
    a 32 x 32 map: C reduce channels, Nn result channels (kind 0: C = I, Nn = O; kind 1: C = O, Nn = I)."""
    return (C % 16 == 0 and C >= 32 and Nn >= 32 and Nn % 4 == 0 and N * HW * HW * C < 2 ** 29      # wino_variant's gate
            and Nn % 32 == 0 and C % 32 == 0)                                                       # the F(4x4,3x3) branch


def wgrad_geometry(N, I, O):
    """wino43_wgrad_geometry: None when not applicable, else ntc, splits, chunks per split and whether `++cps` ran."""
    if not f43(N, I, O) or I % 64 != 0 or O % 32 != 0:
        return None
    T = N * (HW // 4) * (HW // 4)
    ntc = ceil_div(T, 64) * 8
    tiles = (O // 32) * (I // 64)
    splits = max(1, 256 // tiles)
    cps = max(2, ceil_div(ntc, splits))
    bumped = ntc % cps == 1
    if bumped:
        cps += 1                          # the last split needs two chunks too
    splits = ceil_div(ntc, cps)
    if ntc < 2 or ntc - (splits - 1) * cps < 2:
        return None
    g = dict(ntc=ntc, splits=splits, cps=cps, bumped=bumped, v_bytes=v_bytes(N, I), z_bytes=z_bytes(N, O))
    return g if g["v_bytes"] < 2 ** 32 and g["z_bytes"] < 2 ** 32 else None


def conv_v_applicable(N, I, O):
    """srgan_instnorm_conv_v_applicable: 32 x 32 map, I % 32 == 0, the forward dispatches to F(4x4,3x3)."""
    return I % 32 == 0 and f43(N, I, O)


def bwd_vz_applicable(N, I, O):
    """srgan_instnorm_bwd_vz_applicable: O % 32 == 0, the input gradient dispatches to F(4x4,3x3), the weight gradient has its
    geometry."""
    return O % 32 == 0 and f43(N, O, I) and wgrad_geometry(N, I, O) is not None


def wgrad_v_bytes(N, I, O):
    g = wgrad_geometry(N, I, O)
    return g["v_bytes"] if g else 0


def packed_scratch(N, I, O, kind):
    """srgan_conv2d_packed_scratch of a layer that runs on F(4x4,3x3) in that direction (every case below does)."""
    assert f43(N, I, O) if kind == 0 else f43(N, O, I)
    return v_bytes(N, I if kind == 0 else O)


# ---- cases ----------------------------------------------------------------------------------------------------------------------
# grid: "full" = {none, ReLU, LeakyReLU} x {affine, no affine}; an integer k = two of the six, COMBOS[k] and COMBOS[k + 3], so that
# the three values of k together meet all six (the "fold" of norm_common.param_grid)
COMBOS = [(ACT_NONE, True), (ACT_RELU, False), (ACT_LRELU, True), (ACT_NONE, False), (ACT_RELU, True), (ACT_LRELU, False)]


def _case(nio, grid, why):
    return dict(name="x".join(map(str, nio)), nio=nio, grid=grid, why=why)


FWD_CASES = [
    _case((1, 32, 32), "full", "the minimum: two 16-channel slabs, plain grid"),
    _case((3, 96, 64), "full", "I % 64 != 0: six slabs, chunk index slab * 2 + (quad >> 1) over an odd pair count"),
    _case((8, 64, 32), 0, "the (N & 7) == 0 XCD remap with one group of eight images"),
    _case((16, 128, 96), 2, "the remap with two groups, three output tiles"),
    _case((5, 256, 256), 1, "trunk width, N % 8 != 0"),
]
BWD_CASES = [
    _case((1, 64, 32), "full", "the minimum: ntc = 8, four splits of two chunks"),
    _case((2, 64, 128), "full", "I != O: the norm and the Z image run over O = 128, the skip tensor has I = 64 channels"),
    _case((2, 128, 64), 0, "I != O the other way round"),
    _case((8, 64, 64), 2, "the XCD remap"),
    _case((11, 128, 128), 0, "ntc = 88: cps 3 -> 4 through the `++cps` branch, 22 splits"),
    _case((5, 256, 256), 1, "trunk width"),
]
# what wino43_wgrad_geometry gives for the backward cases: (ntc, splits, chunks per split, `++cps` taken)
BWD_GEOMETRY = {(1, 64, 32): (8, 4, 2, False), (2, 64, 128): (16, 8, 2, False), (2, 128, 64): (16, 8, 2, False),
                (8, 64, 64): (64, 32, 2, False), (11, 128, 128): (88, 22, 4, True), (5, 256, 256): (40, 8, 5, False)}
BUMP_PAIRS = [(64, 32), (64, 64), (128, 128), (128, 64), (64, 128), (256, 256)]      # (I, O) pairs searched for the `++cps` branch
BUMP_CASE = (11, 128, 128)

# the epilogue of srgan_conv2d_fwd_from_v: (case, activation of the norm, affine, activation after conv + bias)
EPILOGUE_CASES = [((3, 96, 64), ACT_RELU, True, ACT_RELU), ((8, 64, 32), ACT_NONE, False, ACT_LRELU)]
# the weight gradient with the V image that srgan_instnorm_fwd_v wrote (the v1 of the residual block: norm output feeding c2):
# (case, activation and affine of the norm in front of the convolution; behind it: ReLU, affine)
V_FROM_NORM_CASE = ((2, 64, 128), ACT_RELU, True)

# hostile inputs of the norm: shape of the normalised tensor -> (forward case, backward case)
HOSTILE_SHAPES = {(2, 32, 32, 32): ((2, 32, 32), (2, 64, 32)), (8, 64, 32, 32): ((8, 64, 64), (8, 64, 64))}


def _near_eps(shape):
    """Per-channel variance about 9e-6, beside eps = 1e-5: eps decides rstd to tens of percent."""
    return nc.rnd(*shape, seed=1) * 3e-3 + 0.3


NEAR_EPS = "near_eps"
HOSTILE_INPUTS = dict(nc.HOSTILE_INPUTS, **{NEAR_EPS: _near_eps})
HOSTILE_CASES = [(shape, kind) for shape in HOSTILE_SHAPES for kind in HOSTILE_INPUTS]
# as tests/test_norm_kernels_gpu.py treats them: forward with each activation, backward without one (both with affine parameters)
HOSTILE_FWD_ACTS = (ACT_RELU, ACT_LRELU)


def combos(case):
    g = case["grid"]
    return list(COMBOS) if g == "full" else [COMBOS[g], COMBOS[g + 3]]


def runs(cases):
    return [(c["nio"], act, affine) for c in cases for act, affine in combos(c)]


def run_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def case10(N, I, O, bias=False):
    return cc.full(N, I, HW, HW, O, 3, 1, 1, False, bias)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def norm_input(shape, kind="default"):
    return HOSTILE_INPUTS[kind](shape)


def affine_params(N, C, affine):
    """(scale, shift) as norm_common.case_params makes them, or (None, None)."""
    return nc.case_params((N, C, HW, HW), affine, False)[:2]


def weight(I, O):
    return cc.inputs(case10(1, I, O))[1]


def bias_of(O):
    return cc.inputs(case10(1, 32, O, True))[2]


def conv_input(N, I):
    return cc.rnd(N, I, HW, HW, seed=6)


def skip_gradient(N, I):
    return cc.rnd(N, I, HW, HW, seed=5)


def _to(t, dtype):
    return None if t is None else t.detach().to(dtype)


# ---- references -----------------------------------------------------------------------------------------------------------------
def plane_stats(x):
    """(mean, rstd) [N * C] in x's type: biased variance, rstd = (var + eps)^-1/2."""
    mu = x.mean(dim=(2, 3), keepdim=True)
    var = ((x - mu) ** 2).mean(dim=(2, 3))
    return mu.flatten(), (1.0 / torch.sqrt(var + EPS)).flatten()


def forward_ref(x, scale, shift, w, bias, act, epilogue_act, dtype):
    """(y, mean, rstd) = (act2(conv3x3(act(pre_activation(x, scale, shift))) + bias), statistics of x) in `dtype`."""
    xv = _to(x, dtype)
    h = nc.norm_ref(act)(xv, _to(scale, dtype), _to(shift, dtype), None)
    y = act_ref(epilogue_act, SLOPE)(cc.conv_ref(h, _to(w, dtype), _to(bias, dtype), 1, 1, False))
    return (y,) + plane_stats(xv)


def backward_ref(y, gup, scale, shift, w, x_conv, act, dtype):
    """dict(dy, dscale, dshift, dx, dw) in `dtype`: the norm's backward of `gup` at the norm input `y` (autograd of
    norm_common.norm_ref; without affine parameters dscale / dshift are the sums the kernel still writes: the gradients at
    scale = 1, shift = 0, which leave every value unchanged), then the convolution's two gradients of dy."""
    N, O = y.shape[:2]
    yv = _to(y, dtype).requires_grad_(True)
    sc = (_to(scale, dtype) if scale is not None else torch.ones(N, O, dtype=dtype)).requires_grad_(True)
    sh = (_to(shift, dtype) if shift is not None else torch.zeros(N, O, dtype=dtype)).requires_grad_(True)
    out = nc.norm_ref(act)(yv, sc, sh, None)
    dy, dscale, dshift = torch.autograd.grad(out, [yv, sc, sh], _to(gup, dtype))
    I = w.shape[1]
    _, dx, dw, _ = cc.reference(case10(N, I, O), x_conv, w, None, dy, dtype)
    return dict(dy=dy, dscale=dscale, dshift=dshift, dx=dx, dw=dw)


def masked_upstream(y, scale, shift, act):
    """The upstream gradient of the norm over `y`, zero inside the kink window of `act` (norm_common.kink_keep)."""
    gup = nc.upstream(tuple(y.shape))
    return gup if act == ACT_NONE else gup * nc.kink_keep(y, scale, shift, None, act, L)


@functools.lru_cache(maxsize=2)
def forward_yardstick(nio, act, affine, epilogue_act=ACT_NONE, with_bias=False, kind="default"):
    """(inputs, float64 results, float32-CPU results) of the forward composition; results are (y, mean, rstd)."""
    torch.set_num_threads(16)
    N, I, O = nio
    x = norm_input((N, I, HW, HW), kind)
    scale, shift = affine_params(N, I, affine)
    w, bias = weight(I, O), (bias_of(O) if with_bias else None)
    refs = [forward_ref(x, scale, shift, w, bias, act, epilogue_act, dt) for dt in (torch.float64, torch.float32)]
    return dict(x=x, scale=scale, shift=shift, w=w, bias=bias), refs[0], refs[1]


@functools.lru_cache(maxsize=2)
def backward_yardstick(nio, act, affine, kind="default", v_from_norm=None):
    """(inputs, float64 results, float32-CPU results) of the two backward compositions; results are backward_ref's, plus
    dx_res = dx + res.  mean / rstd among the inputs are the float64 statistics rounded to float32.  v_from_norm = (act, affine):
    the convolution's input is that norm of x0, which the test hands to srgan_instnorm_fwd_v instead of the convolution's input
    to srgan_conv2d_fwd_packed; x_conv is then the float64 / float32 normalised tensor of each reference."""
    torch.set_num_threads(16)
    N, I, O = nio
    y = norm_input((N, O, HW, HW), kind)
    scale, shift = affine_params(N, O, affine)
    gup = masked_upstream(y, scale, shift, act)
    w, res = weight(I, O), skip_gradient(N, I)
    mean, rstd = (t.float() for t in plane_stats(y.double()))
    inp = dict(y=y, gup=gup, scale=scale, shift=shift, w=w, res=res, mean=mean, rstd=rstd)
    if v_from_norm is None:
        inp["x_conv"] = conv_input(N, I)
        x_of = lambda dt: inp["x_conv"]
    else:
        act0, affine0 = v_from_norm
        inp["act0"] = act0
        inp["x0"] = nc.default_input((N, I, HW, HW))
        inp["scale0"], inp["shift0"] = affine_params(N, I, affine0)
        x_of = lambda dt: nc.norm_ref(act0)(_to(inp["x0"], dt), _to(inp["scale0"], dt), _to(inp["shift0"], dt), None)
    refs = []
    for dt in (torch.float64, torch.float32):
        r = backward_ref(y, gup, scale, shift, w, x_of(dt), act, dt)
        r["dx_res"] = r["dx"] + res.to(dt)
        refs.append(r)
    return inp, refs[0], refs[1]
