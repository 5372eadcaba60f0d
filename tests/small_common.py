"""Yardsticks of the small-kernel tests (csrc/losses.hip, csrc/pointwise.hip): float64 references, seeded case lists and the
error measure.  No GPU code: tests/test_small_refs_cpu.py pins what is in here, tests/test_small_kernels_gpu.py holds the HIP
kernels to it.

Error measure (the one of ``close`` in test_ops_gpu.py): max |a - ref| over the tensor, relative to max |ref| of the float64
reference.  A comparison is bounded by ``max(8 * e32, gamma)``:

  e32    the error, by the same measure, of the SAME formulas run in float32 on the CPU -- the reference sets the bar;
  gamma  (L + 16) * 2^-23, L the longest sequential float32 sum one thread performs for that output (stated per case);
  8      the different summation order and expf / logf implementations.
"""
import functools
import math
import os

import torch
import torch.nn.functional as F

from oracle import losses as ol

EPS32 = 2.0 ** -23
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2


def gamma(L):
    return (L + 16) * EPS32


def ceil_div(a, b):
    return -(-a // b)


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def rel_err(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if not bool(torch.isfinite(a).all()):
        return math.inf
    return float((a - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def check(kernel, what, got, ref64, ref32, L):
    """Hold ``got`` (the HIP kernel's tensor) to the float64 reference; with SRGAN_TEST_LOG set, print the figures first."""
    e32, err, g = rel_err(ref32, ref64), rel_err(got, ref64), gamma(L)
    bound = max(8 * e32, g)
    if os.environ.get("SRGAN_TEST_LOG"):
        print(f"small {kernel} | {what} | e32 {e32:.3e} gamma {g:.3e} err {err:.3e} err/bound {err / bound:.3f}")
    assert err <= bound, f"{kernel} {what}: error {err:.3e} > max(8 * e32 = {8 * e32:.3e}, gamma = {g:.3e})"


def run(fn, inputs, needs, gout=None, dtype=torch.float32, device="cpu"):
    """fn on copies of ``inputs`` (floating tensors cast to dtype, everything moved to device) -> [out, grads w.r.t. the inputs
    flagged in ``needs``], all detached."""
    xs = []
    for x, n in zip(inputs, needs):
        if torch.is_tensor(x) and x.is_floating_point():
            x = x.detach().to(device=device, dtype=dtype).requires_grad_(n)
        elif torch.is_tensor(x):
            x = x.to(device)
        xs.append(x)
    y = fn(*xs)
    outs = [y.detach()]
    wrt = [x for x, n in zip(xs, needs) if n]
    if wrt:
        g = None if gout is None else gout.to(device=y.device, dtype=y.dtype)
        outs += [t.detach() for t in torch.autograd.grad(y, wrt, g)]
    return outs


def yardstick(fn, inputs, needs, gout=None):
    """(float64 results, float32-CPU results) of the reference formulas."""
    return run(fn, inputs, needs, gout, torch.float64), run(fn, inputs, needs, gout, torch.float32)


# ---- latent losses -----------------------------------------------------------------------------------------------------------
ALL_W = ((10.0, 100.0, 100.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
# bins = 1: p = h / S is identically 1, so the histogram term's gradient is identically 0 and a float32 evaluation of it is
# rounding noise over a reference of zero -- not a comparison; the term is checked there inside the weighted sum only (its
# value is d * log(1 / (1 + 1e-8)) ~ -1e-8 d in float64 and 0 in any float32 evaluation: e32 = 1 says so)
NO_HIST_ALONE = ALL_W[:3]


def _lat(name, B, d, n_batch, bins=50, range_max=10.0, sigma=0.2, s=1.0, seed=0, weights=ALL_W):
    return dict(name=name, B=B, d=d, n_batch=n_batch, bins=bins, range_max=range_max, sigma=sigma, s=s, seed=seed, weights=weights)


# mu = randn * s + 0.3; the seeds are the first for which the case is well conditioned (test_small_refs_cpu.py checks it);
# B >= d + 2 everywhere (below that the Pearson matrix is singular)
LATENT_CASES = [
    _lat("b4_d2", 4, 2, 4, seed=0),
    _lat("b7_d5_bins7", 7, 5, 7, bins=7, range_max=4.0, sigma=0.5, seed=0),
    _lat("b32_d8", 32, 8, 32, seed=0),
    _lat("b32_d8_bins1", 32, 8, 32, bins=1, range_max=2.0, sigma=1.0, seed=0, weights=NO_HIST_ALONE),
    _lat("b64_d8_n32", 64, 8, 32, s=4.0, seed=0),                        # the data-parallel shape: B gathered, n_batch local
    _lat("b33_d3_n40_bins64", 33, 3, 40, bins=64, seed=0),
    _lat("b257_d16", 257, 16, 257, s=4.0, seed=0),
    _lat("b300_d3_bins7", 300, 3, 300, bins=7, range_max=4.0, sigma=0.5, seed=0),
]
LATENT_LIMIT_CASE = _lat("b1024_d16_limit", 1024, 16, 1024, seed=0)      # B * d = 16384, the documented limit
LATENT_PUBLIC_CASE = _lat("b40_d6_public", 40, 6, 40, seed=0)            # through losses.corrcoef / corrcoef_loss / histogram_imitation


def latent_inputs(case):
    mu = rnd(case["B"], case["d"], seed=case["seed"]) * case["s"] + 0.3
    target = ol.analytic_hist_target(case["bins"], case["range_max"], case["sigma"])
    return mu, target


def latent_terms(mu, n_batch, target, bins, range_max, sigma, dtype):
    """The three terms by the formulas of oracle/losses.py in ``dtype``: (values [3], their gradients w.r.t. mu [3][B, d],
    Pearson matrix [d, d], per-column histogram mass S [d])."""
    mu = mu.detach().to(dtype).requires_grad_(True)
    hi = ol.HistogramImitation(bins, range_max, sigma, target=target.detach().cpu().to(dtype))
    terms = (ol.batch_kl(mu, n_batch), ol.corr_loss(mu.t()), hi.loss(mu))
    grads = [torch.autograd.grad(t, mu, retain_graph=True)[0] for t in terms]
    mass = torch.stack([ol.soft_histogram(mu.detach()[:, j], bins, -float(range_max), float(range_max), sigma).sum()
                        for j in range(mu.shape[1])])
    return torch.stack([t.detach() for t in terms]), grads, ol.corrcoef(mu.detach().t()), mass


def latent_combine(terms, w):
    """(total, dmu) of the weighted sum over the terms whose weight is not zero -- a term that is not asked for is not computed."""
    vals, grads = terms[0], terms[1]
    total, dmu = torch.zeros((), dtype=vals.dtype), torch.zeros_like(grads[0])
    for i in range(3):
        if w[i] != 0.0:
            total, dmu = total + w[i] * vals[i], dmu + w[i] * grads[i]
    return total, dmu


@functools.lru_cache(maxsize=None)
def _latent_yardstick(name):
    case = next(c for c in LATENT_CASES + [LATENT_LIMIT_CASE, LATENT_PUBLIC_CASE] if c["name"] == name)
    mu, target = latent_inputs(case)
    args = (mu, case["n_batch"], target, case["bins"], case["range_max"], case["sigma"])
    return latent_terms(*args, torch.float64), latent_terms(*args, torch.float32)


def latent_yardstick(case):
    return _latent_yardstick(case["name"])


def conditioning(case):
    """(min and max of the off-diagonal |r|, smallest column standard deviation, smallest histogram mass S) in float64."""
    mu, _ = latent_inputs(case)
    _, _, R, mass = latent_yardstick(case)[0]
    off = R[~torch.eye(R.shape[0], dtype=torch.bool)].abs()
    return float(off.min()), float(off.max()), float(mu.double().std(dim=0).min()), float(mass.min())


# the three deliberately degenerate inputs (exempt from the conditioning rule): (32, 8) samples of the golden shape
def degenerate_far_column():
    """Column 3 lies wholly beyond 13: every expf of its histogram underflows in float32 (S = 0)."""
    mu = rnd(32, 8, seed=11) + 0.3
    mu[:, 3] = mu[:, 3] + 20.0
    assert float(mu[:, 3].min()) > 13.0
    return mu


def degenerate_constant_column():
    """Column 2 is constant (inside the histogram range): zero variance, log(0) in batch-KL and 0 / 0 in the correlation."""
    mu = rnd(32, 8, seed=12) + 0.3
    mu[:, 2] = 1.25
    return mu


def degenerate_identical_columns():
    """Column 5 repeats column 1: an off-diagonal r of exactly +-1 up to rounding (the clamp)."""
    mu = rnd(32, 8, seed=13) + 0.3
    mu[:, 5] = mu[:, 1]
    return mu


# ---- the other loss kernels ------------------------------------------------------------------------------------------------------
KL_NORMAL_CASES = [(n, w) for n in (1, 63, 255, 256, 257, 512, 5000) for w in (1.0, 0.1)]


def kl_normal_inputs(n):
    mu = rnd(n, seed=100 + n)
    logvar = torch.rand(n, generator=torch.Generator().manual_seed(200 + n)) * 12.0 - 8.0      # [-8, 4]
    return mu, logvar


def kl_normal_ref(weight):
    return lambda mu, logvar: weight * ol.conventional_kl(mu, logvar)


L1_SIZES = (1, 2047, 2048, 2049, 300001, 2200003)
L1_WEIGHT = 5.0


def l1_blocks(n):
    return max(1, min(1024, ceil_div(n, 2048)))


def l1_inputs(n):
    a, b = rnd(n, seed=300 + n % 1000), rnd(n, seed=301 + n % 1000)
    b[3::7] = a[3::7]                       # exact zeros in a - b: the gradient there is 0, as in torch
    return a, b


def l1_ref(a, b):
    return L1_WEIGHT * F.l1_loss(a, b)


HIST_A, HIST_B = (-10.0, 10.0, 0.2), (-3.0, 5.0, 0.7)
SOFT_HIST_CASES = [        # n, bins, (lo, hi, sigma)
    (1, 50, HIST_A),
    (255, 1, HIST_B),
    (255, 64, HIST_A),
    (65537, 100, HIST_A),   # 257 blocks asked, 256 launched: the forward's cap plus stride; two blocks in the final kernel
    (100000, 50, HIST_A),   # the constructor's own sample size
    (300001, 64, HIST_B),   # beyond the backward's 1024-block cap
]


def soft_hist_blocks(n):
    return max(1, min(256, ceil_div(n, 256)))


def soft_hist_inputs(n, bins):
    x = rnd(n, seed=400 + bins) * 3.0
    x[::50] += 15.0                          # samples outside either range
    g = torch.linspace(0.5, 1.5, bins) * (1.0 - 2.0 * (torch.arange(bins) % 2))
    return x, g


def soft_hist_ref(x, g, bins, lo, hi, sigma, dtype, chunk=32768):
    """oracle/losses.py's soft_histogram summed over chunks of the sample (the histogram is additive over samples), and the
    gradient of (h * g).sum() -- chunked so that the [bins, n] kernel matrix never exists whole."""
    x, g = x.to(dtype), g.to(dtype)
    h, dx = torch.zeros(bins, dtype=dtype), []
    for i in range(0, x.numel(), chunk):
        xc = x[i:i + chunk].clone().requires_grad_(True)
        hc = ol.soft_histogram(xc, bins, lo, hi, sigma)
        dx.append(torch.autograd.grad(hc, xc, g)[0])
        h += hc.detach()
    return h, torch.cat(dx)


XENT_CASES = [(1, 2, 1.0), (256, 4, 1.0), (257, 4, 1.0), (300, 10, 0.3), (5, 1, 1.0)]      # B, classes, weight


def xent_inputs(B, nc):
    z = rnd(B, nc, seed=500 + B) * 2.0
    label = torch.randint(0, nc, (B,), generator=torch.Generator().manual_seed(600 + B))
    return z, label


def xent_ref(weight):
    return lambda z, label: weight * F.cross_entropy(z, label)


# n terms; slot i = which underlying scalar term i reads (a repeated slot = one tensor passed twice: its gradient is the sum)
LINCOMB_CASES = [
    dict(n=1, slots=[0], no_grad=()),
    dict(n=16, slots=list(range(15)) + [2], no_grad=(4,)),
    dict(n=17, slots=list(range(17)), no_grad=()),
    dict(n=33, slots=list(range(30)) + [0, 17, 29], no_grad=(20,)),
]


def lincomb_inputs(case):
    n = case["n"]
    x = rnd(max(case["slots"]) + 1, seed=700 + n).double()
    w = rnd(n, seed=701 + n).double()
    w[1::5] = 0.0                            # zero weights
    return x, w


def lincomb_ref(case, dtype, gout=1.0):
    x, w = lincomb_inputs(case)
    x, w = x.to(dtype), w.to(dtype)
    out = torch.zeros((), dtype=dtype)
    for i, s in enumerate(case["slots"]):
        out = out + w[i] * x[s]
    grad = torch.zeros_like(x)
    for i, s in enumerate(case["slots"]):
        grad[s] += w[i] * gout
    return out, grad


# ---- pointwise kernels -------------------------------------------------------------------------------------------------------------
POOL3_SHAPES = [(2, 3, 16, 16), (1, 5, 12, 9), (3, 4, 1, 1), (2, 2, 2, 5), (1, 3, 128, 128)]
POOL2_SHAPES = [(2, 3, 6, 8), (1, 5, 7, 9), (2, 4, 2, 3), (1, 3, 13, 2), (1, 2, 64, 66)]       # even and odd: torch floors
GAP_SHAPES = [(3, 1024, 4, 4), (5, 7, 1, 1), (2, 100, 3, 5)]
GAP_SLOPE = 0.2
LINEAR_CASES = [(m, k, n, bias) for (m, k, n) in ((1, 1024, 8), (64, 1024, 8), (6, 100, 1), (3, 1, 5)) for bias in (True, False)]
LAYOUT_SHAPES = [(2, 33, 5, 7), (1, 3, 128, 128), (3, 64, 1, 1), (2, 1, 9, 9), (1, 256, 31, 31)]
POINTWISE_BIG = 8192 * 256 + 77          # one element more than the grid cap covers in one pass, and a ragged tail
POINTWISE_TINY = 5
ACTS = [(ACT_NONE, 0.0), (ACT_RELU, 0.0), (ACT_LRELU, 0.2), (ACT_LRELU, 0.01)]


def pool3_ref(x):
    return F.avg_pool2d(x, 3, 2, 1, count_include_pad=False)


def pool2_ref(x):
    return F.avg_pool2d(x, 2)


def gap_ref(x):
    return F.adaptive_avg_pool2d(F.leaky_relu(x, GAP_SLOPE), 1).flatten(1)


def act_ref(act, slope):
    return {ACT_NONE: lambda x: x * 1.0, ACT_RELU: F.relu, ACT_LRELU: lambda x: F.leaky_relu(x, slope)}[act]


def pointwise_input(n, seed):
    x = rnd(n, seed=seed)
    x[::11] = 0.0                            # exact zeros: the activation's kink
    return x
