"""GPU: the loss and pointwise kernels (csrc/losses.hip, csrc/pointwise.hip) against float64 over their whole domain -- the
shapes at which grid-stride loops, multi-block partial sums, ragged 32x32 tiles, more rows than threads and the dynamic LDS
size come into play.  References, cases and the error measure live in tests/small_common.py (pinned without a GPU by
tests/test_small_refs_cpu.py).  Every comparison is bounded by max(8 * e32, gamma): e32 the float32-CPU error of the same
formulas computed here, gamma = (L + 16) * 2^-23 with L the longest sequential float32 sum of one thread; SRGAN_TEST_LOG=1
prints the three figures of every comparison.  Pure selects and copies are compared exactly."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import small_common as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from srgan_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(scope="module")
def hl():
    from srgan_amd import losses
    return losses


def hip(fn, inputs, needs, gout=None):
    return sc.run(fn, inputs, needs, gout, torch.float32, "cuda")


def held(kernel, what, got, yard, L, names):
    """Every tensor of ``got`` (output, then gradients) against the (float64, float32-CPU) pair of small_common.yardstick."""
    ref64, ref32 = yard
    assert len(got) == len(ref64) == len(names)
    for g, r64, r32, name in zip(got, ref64, ref32, names):
        sc.check(kernel, f"{what} {name}", g, r64, r32, L[name] if isinstance(L, dict) else L)


# ---- latent losses -------------------------------------------------------------------------------------------------------------
def _latent_hip(ops, mu, n_batch, target, w, bins, range_max, sigma):
    mud = mu.cuda().requires_grad_(True)
    total, parts, corr = ops.latent_losses(mud, n_batch, target.cuda(), w[0], w[1], w[2], bins, range_max, sigma)
    (dmu,) = torch.autograd.grad(total, mud)
    return total.detach(), parts, corr, dmu


def _check_latent_case(ops, case):
    mu, target = sc.latent_inputs(case)
    t64, t32 = sc.latent_yardstick(case)
    L = max(case["B"], case["bins"])
    for w in case["weights"]:
        total, parts, corr, dmu = _latent_hip(ops, mu, case["n_batch"], target, w, case["bins"], case["range_max"], case["sigma"])
        what = f"{case['name']} w={w}"
        for i, name in enumerate(("bkl", "corr", "hist")):        # vals[0..2] are the raw parts whatever the weights
            sc.check("latent_losses", f"{what} {name}", parts[i], t64[0][i], t32[0][i], L)
        (tot64, d64), (tot32, d32) = sc.latent_combine(t64, w), sc.latent_combine(t32, w)
        sc.check("latent_losses", f"{what} total", total, tot64, tot32, L)
        sc.check("latent_losses", f"{what} dmu", dmu, d64, d32, L)     # one weight alone: that term's float64 gradient alone
        sc.check("latent_losses", f"{what} pearson", corr, t64[2], t32[2], L)


def test_latent_losses_at_the_element_limit(ops):
    """B * d = 16384, the documented limit: about 76 KB of dynamic LDS in one workgroup.  Run first and on its own."""
    _check_latent_case(ops, sc.LATENT_LIMIT_CASE)
    from srgan_amd._lib import SrganHipError
    with pytest.raises(SrganHipError, match="B\\*d<=16384"):           # one row more is refused before any launch
        ops.latent_losses(torch.zeros(1025, 16).cuda(), 1025, torch.full((50,), 0.02).cuda(), 1.0, 1.0, 1.0)


@pytest.mark.parametrize("case", sc.LATENT_CASES, ids=[c["name"] for c in sc.LATENT_CASES])
def test_latent_losses(ops, case):
    _check_latent_case(ops, case)


def test_latent_public_entry_points(ops, hl):
    """losses.corrcoef / corrcoef_loss / histogram_imitation.loss on a shape other than the golden one."""
    case = sc.LATENT_PUBLIC_CASE
    mu, _ = sc.latent_inputs(case)
    t64, t32 = sc.latent_yardstick(case)
    B = case["B"]
    sc.check("latent_losses", "losses.corrcoef", hl.corrcoef(mu.t().cuda()), t64[2], t32[2], B)
    md = mu.t().contiguous().cuda().requires_grad_(True)
    v = hl.corrcoef_loss(md, "cuda")
    sc.check("latent_losses", "losses.corrcoef_loss", v, t64[0][1], t32[0][1], B)
    sc.check("latent_losses", "losses.corrcoef_loss grad", torch.autograd.grad(v, md)[0].t(), t64[1][1], t32[1][1], B)
    torch.manual_seed(5)
    hi = hl.histogram_imitation("cuda", bins=24, range_max=6, sigma=0.4, target_num=3000)
    tgt = hi.target.detach().cpu()
    args = (mu, B, tgt, 24, 6.0, 0.4)
    h64, h32 = sc.latent_terms(*args, torch.float64), sc.latent_terms(*args, torch.float32)
    xd = mu.cuda().requires_grad_(True)
    v = hi.loss(xd)
    sc.check("latent_losses", "histogram_imitation.loss", v, h64[0][2], h32[0][2], B)
    sc.check("latent_losses", "histogram_imitation.loss grad", torch.autograd.grad(v, xd)[0], h64[1][2], h32[1][2], B)


def test_latent_degenerate_far_column_under_batch_kl_alone(ops):
    """trainer.py runs batch-KL alone (w_corr = w_hist = 0) when corr_enc and hist are off.  A column wholly beyond the
    histogram range has S = 0 in float32 (h / S is NaN); the term is not asked for and must not reach total or dmu."""
    mu = sc.degenerate_far_column()
    target = torch.full((50,), 1.0 / 50)
    w = (10.0, 0.0, 0.0)
    total, _, _, dmu = _latent_hip(ops, mu, 32, target, w, 50, 10.0, 0.2)
    assert bool(torch.isfinite(total)) and bool(torch.isfinite(dmu).all()), (total, dmu)
    yard = sc.yardstick(lambda m: 10.0 * sc.ol.batch_kl(m, 32), [mu], [True])
    held("latent_losses", "far column, batch-KL alone", [total, dmu], yard, 32, ("total", "dmu"))


def test_latent_degenerate_constant_column_under_histogram_imitation(ops, hl):
    """histogram_imitation.loss (w_bkl = w_corr = 0) on a sample with a constant column: log(0) and 0 / 0 in the two terms it
    does not want; the float64 HistogramImitation.loss is finite (S != 0: the constant lies inside the range)."""
    mu = sc.degenerate_constant_column()
    torch.manual_seed(0)
    hi = hl.histogram_imitation("cuda", target_num=5000)
    ref = sc.ol.HistogramImitation(target=hi.target.detach().cpu())
    xd = mu.cuda().requires_grad_(True)
    v = hi.loss(xd)
    (g,) = torch.autograd.grad(v, xd)
    assert bool(torch.isfinite(v)) and bool(torch.isfinite(g).all()), (v, g)
    yard = sc.yardstick(lambda m: ref.loss(m), [mu], [True])
    held("latent_losses", "constant column, histogram alone", [v.detach(), g], yard, 50, ("total", "dmu"))


def test_latent_degenerate_identical_columns_under_histogram_alone(ops):
    mu = sc.degenerate_identical_columns()
    target = sc.ol.analytic_hist_target()
    w = (0.0, 0.0, 3.0)
    total, _, _, dmu = _latent_hip(ops, mu, 32, target, w, 50, 10.0, 0.2)
    assert bool(torch.isfinite(total)) and bool(torch.isfinite(dmu).all()), (total, dmu)
    ref = sc.ol.HistogramImitation(target=target)
    yard = sc.yardstick(lambda m: 3.0 * ref.loss(m), [mu], [True])
    held("latent_losses", "identical columns, histogram alone", [total, dmu], yard, 50, ("total", "dmu"))


def test_latent_nonzero_weights_keep_the_recorded_bits(ops, golden_dir):
    """With all three weights non-zero the zero-weight selects change no bit: vals, dmu and the Pearson matrix at the golden
    (32, 8) inputs equal the arrays recorded from the build before the selects (tests/golden/make_latent_parent_bits.py)."""
    gold = np.load(os.path.join(golden_dir, "losses.npz"))
    rec = np.load(os.path.join(golden_dir, "latent_losses_parent_bits.npz"))
    tgt = torch.from_numpy(gold["hist_target_seed0"])
    for name in ("randn1234", "sin"):
        total, parts, corr, dmu = _latent_hip(ops, torch.from_numpy(gold[f"{name}_mu"]), 32, tgt, (10.0, 100.0, 100.0), 50, 10.0, 0.2)
        vals = torch.cat([parts, total.reshape(1)]).cpu().numpy()
        for key, got in (("vals", vals), ("dmu", dmu.cpu().numpy()), ("corr", corr.cpu().numpy())):
            assert np.array_equal(got.view(np.uint32), rec[f"{name}_{key}"].view(np.uint32)), (name, key)


# ---- the other loss kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,weight", sc.KL_NORMAL_CASES)
def test_kl_normal(ops, n, weight):
    inputs = sc.kl_normal_inputs(n)
    yard = sc.yardstick(sc.kl_normal_ref(weight), inputs, [True, True])
    got = hip(lambda m, lv: ops.kl_normal(m, lv, weight), inputs, [True, True])
    held("kl_normal", f"n={n} w={weight}", got, yard, {"loss": sc.ceil_div(n, 256), "dmu": 1, "dlogvar": 1}, ("loss", "dmu", "dlogvar"))


@pytest.mark.parametrize("n", sc.L1_SIZES)
def test_l1_mean(ops, n):
    inputs = sc.l1_inputs(n)
    L = sc.ceil_div(n, sc.l1_blocks(n) * 256)
    variants = (([True, True], ("loss", "da", "db")), ([True, False], ("loss", "da")), ([False, True], ("loss", "db")))
    for needs, names in variants[:1] if n > 1000000 else variants:      # a null da / db does not depend on the size
        yard = sc.yardstick(sc.l1_ref, inputs, needs)
        got = hip(lambda a, b: ops.l1_mean(a, b, sc.L1_WEIGHT), inputs, needs)
        held("l1_mean", f"n={n} needs={needs}", got, yard, {"loss": L, "da": 1, "db": 1}, names)
        zero = (inputs[0] == inputs[1])
        for g in got[1:]:
            assert zero.any() or n == 1
            assert bool((g.cpu()[zero] == 0).all())                  # sign(0) = 0, as in torch


@pytest.mark.parametrize("n,bins,cfg", sc.SOFT_HIST_CASES)
def test_soft_histogram(ops, n, bins, cfg):
    lo, hi, sigma = cfg
    x, g = sc.soft_hist_inputs(n, bins)
    h64, dx64 = sc.soft_hist_ref(x, g, bins, lo, hi, sigma, torch.float64)
    h32, dx32 = sc.soft_hist_ref(x, g, bins, lo, hi, sigma, torch.float32)
    h, dx = hip(lambda t: ops.soft_histogram(t, bins, lo, hi, sigma), [x], [True], g)
    blocks = sc.soft_hist_blocks(n)
    what = f"n={n} bins={bins} cfg={cfg}"
    sc.check("soft_histogram", what + " h", h, h64, h32, max(sc.ceil_div(n, blocks * 256), blocks))
    sc.check("soft_histogram", what + " dx", dx, dx64, dx32, bins)


@pytest.mark.parametrize("B,nc,weight", sc.XENT_CASES)
def test_softmax_xent(ops, B, nc, weight):
    inputs = sc.xent_inputs(B, nc)
    yard = sc.yardstick(sc.xent_ref(weight), inputs, [True, False])
    got = hip(lambda z, lab: ops.softmax_xent(z, lab, weight), inputs, [True, False])
    held("softmax_xent", f"B={B} nc={nc} w={weight}", got, yard, {"loss": sc.ceil_div(B, 256) + nc, "dz": nc}, ("loss", "dz"))


@pytest.mark.parametrize("case", sc.LINCOMB_CASES, ids=[f"n{c['n']}" for c in sc.LINCOMB_CASES])
def test_lincomb(ops, case):
    x, w = sc.lincomb_inputs(case)
    terms = [x[s].float().cuda().requires_grad_(s not in case["no_grad"]) for s in range(x.numel())]
    out = ops.lincomb([(terms[s], float(w[i])) for i, s in enumerate(case["slots"])])
    out.backward(torch.tensor(1.5).cuda())
    (o64, g64), (o32, g32) = sc.lincomb_ref(case, torch.float64, 1.5), sc.lincomb_ref(case, torch.float32, 1.5)
    sc.check("lincomb", f"n={case['n']} out", out.detach(), o64, o32, case["n"])
    keep = torch.tensor([s not in case["no_grad"] for s in range(x.numel())])
    for s in case["no_grad"]:
        assert terms[s].grad is None
    got = torch.stack([t.grad.cpu() if t.grad is not None else torch.zeros(()) for t in terms])
    sc.check("lincomb", f"n={case['n']} grads", got[keep], g64[keep], g32[keep], 2)


# ---- pointwise kernels -------------------------------------------------------------------------------------------------------------
def _unary(ops_fn, ref_fn, kernel, shape, seed, L, inputs=None):
    x = sc.rnd(*shape, seed=seed) if inputs is None else inputs
    g = sc.rnd(*ref_fn(x).shape, seed=seed + 1)
    yard = sc.yardstick(ref_fn, [x], [True], g)
    got = hip(ops_fn, [x], [True], g)
    held(kernel, f"{tuple(shape)}", got, yard, L, ("y", "dx"))
    return got


@pytest.mark.parametrize("shape", sc.POOL3_SHAPES)
def test_avgpool3s2(ops, shape):
    _unary(ops.avgpool3s2, sc.pool3_ref, "avgpool3s2", shape, 800, 9)


@pytest.mark.parametrize("shape", sc.POOL2_SHAPES)
def test_avgpool2(ops, shape):
    _, dx = _unary(ops.avgpool2, sc.pool2_ref, "avgpool2", shape, 810, 4)
    h, w = shape[2], shape[3]
    dx = dx.cpu()
    assert bool((dx[:, :, h - h % 2:, :] == 0).all()) and bool((dx[:, :, :, w - w % 2:] == 0).all())   # the dropped row / column


@pytest.mark.parametrize("shape", sc.GAP_SHAPES)
def test_lrelu_global_avgpool(ops, shape):
    _unary(lambda x: ops.lrelu_global_avgpool(x, sc.GAP_SLOPE), sc.gap_ref, "lrelu_gap", shape, 820, shape[2] * shape[3])


@pytest.mark.parametrize("m,k,n,bias", sc.LINEAR_CASES)
def test_linear(ops, m, k, n, bias):
    x, W = sc.rnd(m, k, seed=830), sc.rnd(n, k, seed=831) / max(k, 1) ** 0.5
    g = sc.rnd(m, n, seed=833)
    inputs, names = [x, W], ["y", "dx", "dW"]
    if bias:
        inputs.append(sc.rnd(n, seed=832))
        names.append("db")
    yard = sc.yardstick(lambda *a: F.linear(*a), inputs, [True] * len(inputs), g)
    got = hip(lambda *a: ops.linear(*a), inputs, [True] * len(inputs), g)
    L = {"y": sc.ceil_div(k, 64) + 6, "dx": n, "dW": m, "db": m}
    held("linear", f"M={m} K={k} N={n} bias={bias}", got, yard, L, names)


@pytest.mark.parametrize("shape", sc.LAYOUT_SHAPES)
def test_layout_repacks_are_exact(ops, shape):
    x = sc.rnd(*shape, seed=840)
    xd = ops.to_nhwc(x.cuda())
    assert ops.is_nhwc_dense(xd) and xd.shape == x.shape
    assert torch.equal(xd.permute(0, 2, 3, 1).contiguous().cpu(), x.permute(0, 2, 3, 1).contiguous())   # the NHWC memory itself
    back = ops.to_nchw(xd)
    assert back.is_contiguous() and torch.equal(back.cpu(), x)


def _pointwise_inputs(n):
    if n == sc.POINTWISE_TINY:
        return sc.pointwise_input(n, 850)
    return sc.pointwise_input(n, 851)


@pytest.mark.parametrize("n", [sc.POINTWISE_TINY, sc.POINTWISE_BIG])
@pytest.mark.parametrize("act,slope", sc.ACTS)
def test_activation(ops, n, act, slope):
    """Selects and one multiply by the slope -- the single rounding torch makes: exact, forward and backward."""
    x = _pointwise_inputs(n)
    g = sc.rnd(n, seed=852)
    ref = sc.run(sc.act_ref(act, slope), [x], [True], g, torch.float32)
    got = hip(lambda t: ops.activation(t, act, slope), [x], [True], g)
    assert torch.equal(got[0].cpu(), ref[0]) and torch.equal(got[1].cpu(), ref[1])


@pytest.mark.parametrize("n", [sc.POINTWISE_TINY, sc.POINTWISE_BIG])
def test_tanh(ops, n):
    x = _pointwise_inputs(n) * 2.0
    g = sc.rnd(n, seed=853)
    yard = sc.yardstick(torch.tanh, [x], [True], g)
    held("tanh", f"n={n}", hip(ops.tanh, [x], [True], g), yard, 1, ("y", "dx"))


@pytest.mark.parametrize("n", [sc.POINTWISE_TINY, sc.POINTWISE_BIG])
def test_add(ops, n):
    a, b = sc.rnd(1, 1, 1, n, seed=854), sc.rnd(1, 1, 1, n, seed=855)
    g = sc.rnd(1, 1, 1, n, seed=856)
    got = hip(ops.add, [a, b], [True, True], g)
    assert torch.equal(got[0].cpu(), a + b)                          # one rounding, the same as torch's
    assert torch.equal(got[1].cpu(), g) and torch.equal(got[2].cpu(), g)


def test_pointwise_backward_accepts_an_expanded_gradient(ops):
    """y.sum().backward() hands the backward a stride-0 gradient; the kernels read dense memory."""
    x = sc.pointwise_input(300, 857)
    for fn, ref in ((ops.tanh, torch.tanh), (lambda t: ops.activation(t, ops.ACT_LRELU, 0.2), lambda t: F.leaky_relu(t, 0.2))):
        xd = x.cuda().requires_grad_(True)
        fn(xd).sum().backward()
        xr = x.double().requires_grad_(True)
        ref(xr).sum().backward()
        assert sc.rel_err(xd.grad, xr.grad) <= sc.gamma(1)
