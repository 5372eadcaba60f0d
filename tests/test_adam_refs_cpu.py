"""CPU: the yardstick of tests/test_adam_kernels_gpu.py checked without a GPU -- the float64 restatement of tests/adam_common.py
against oracle.trainer.Adam14, a float32 emulation of the kernel's expression against the derived bounds on every input set the
GPU file uses, the restated tick against a 60-digit computation, and the layout of the sentinel slots."""
import decimal
import math

import numpy as np
import pytest
import torch

from tests import adam_common as ac
from tests.adam_common import f32


# ---- 1. the restatement is Adam ------------------------------------------------------------------------------------------------------
def _adam14_run(betas, lr, eps, p0, grads):
    from oracle.trainer import Adam14
    p = torch.from_numpy(p0.copy()).requires_grad_(True)             # float64 tensors: Adam14 computes in double
    opt = Adam14([p], lr=lr, betas=betas, eps=eps)
    out = []
    for g in grads:
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[id(p)]
        out.append((p.data.numpy().copy(), st["m"].numpy().copy(), st["v"].numpy().copy()))
    return out


def _rel(a, b, scale=0.0):
    """worst |a - b| relative to max(|b|, scale, 1e-300) (scale: the largest |p| of the trajectory so far, so that what five
    steps accumulate is not measured against the remainder of an update that cancels p)"""
    return float(np.max(np.abs(a - b) / np.maximum(np.maximum(np.abs(b), scale), 1e-300)))


@pytest.mark.parametrize("lr,beta1,beta2,eps", ac.HYPERS)
def test_restatement_with_torch14_hyper_parameters_is_adam14(lr, beta1, beta2, eps):
    """On float64 tensors Adam14 multiplies by the double 1 - beta, so the float32 complement of torch 1.4 can only be compared
    at betas whose complement IS a float32 number: beta* = 1 - float32(1 - beta), exact in double, |beta* - beta| <= U (1 - beta).  With
    beta*, float32(1 - beta*) from the double and the bias corrections from the double betas, five steps agree to 1e-13."""
    rng = np.random.default_rng(3)
    n = 257
    b1, b2 = 1.0 - float(f32(1.0 - beta1)), 1.0 - float(f32(1.0 - beta2))
    for b, beta in ((b1, beta1), (b2, beta2)):
        assert float(f32(1.0 - b)) == 1.0 - b and abs(b - beta) <= ac.U * (1.0 - beta)
    p0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n) for _ in range(5)]
    want = _adam14_run((b1, b2), lr, eps, p0, grads)
    p, m, v = p0, np.zeros(n), np.zeros(n)
    worst, seen = 0.0, np.abs(p0)
    for t, g in enumerate(grads, 1):
        s = ac.adam_f64(p, g, m, v, **ac.torch14_scalars(t, lr, b1, b2, eps))
        worst = max(worst, _rel(s.p, want[t - 1][0], seen), _rel(s.m, want[t - 1][1]), _rel(s.v, want[t - 1][2]))
        seen = np.maximum(seen, np.abs(s.p))
        p, m, v = s.p, s.m, s.v
    print(f"restatement vs Adam14 over 5 steps: worst relative difference {worst:.2e}")
    assert worst <= 1e-13


@pytest.mark.parametrize("lr,beta1,beta2,eps", ac.HYPERS)
def test_restatement_at_the_nominal_betas_is_adam14_with_the_double_complement(lr, beta1, beta2, eps):
    """the same five lines at the betas as written: Adam14 in double takes 1 - beta in double, and so does this call"""
    rng = np.random.default_rng(4)
    n = 257
    p0 = 1e-3 * rng.standard_normal(n)
    grads = [rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n) for _ in range(5)]
    want = _adam14_run((beta1, beta2), lr, eps, p0, grads)
    p, m, v = p0, np.zeros(n), np.zeros(n)
    seen = np.abs(p0)
    for t, g in enumerate(grads, 1):
        hp = dict(ac.torch14_scalars(t, lr, beta1, beta2, eps), omb1=1.0 - beta1, omb2=1.0 - beta2)
        s = ac.adam_f64(p, g, m, v, **hp)
        assert max(_rel(s.p, want[t - 1][0], seen), _rel(s.m, want[t - 1][1]), _rel(s.v, want[t - 1][2])) <= 1e-13
        seen = np.maximum(seen, np.abs(s.p))
        p, m, v = s.p, s.m, s.v
    # and the float32 complement is within one float32 rounding of it
    for beta in (beta1, beta2):
        assert abs(float(f32(1.0 - beta)) - (1.0 - beta)) <= ac.U * (1.0 - beta)


# ---- 2. the reference alone holds the bound --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def layout():
    return ac.main_layout()


@pytest.mark.parametrize("hyper", range(len(ac.HYPERS)))
def test_float32_emulation_stays_inside_the_bounds_on_the_gpu_inputs(layout, hyper):
    """every (steps_done, step) of tests/test_adam_kernels_gpu.py, once as drawn and once on float32(g * scale) of the clipped run"""
    lr, beta1, beta2, eps = ac.HYPERS[hyper]
    b1, b2, e = ac.kernel_scalars(beta1, beta2, eps)
    worst = dict(p=0.0, m=0.0, v=0.0)
    for steps_done in ac.STEPS_DONE:
        for scale in (None, f32(0.37)):
            x = ac.draw(layout, ac.case_seed(hyper, steps_done))
            p, m, v = x["p"], x["m"], x["v"]
            for k in (1, 2):
                g = x["g"] if k == 1 else ac.redraw_g(layout, ac.case_seed(hyper, steps_done) + 1)
                if scale is not None:
                    g = g * scale
                    assert g.dtype == np.float32
                ss, isb = ac.tick(steps_done + k, lr, beta1, beta2)
                s = ac.restate(p, g, m, v, b1, b2, e, ss, isb)
                with np.errstate(over="raise", invalid="raise", divide="raise"):
                    p, m, v = ac.emulate_f32(p, g, m, v, b1, b2, e, ss, isb)
                r = ac.ratios(p, m, v, s)
                worst = {q: max(worst[q], r[q]) for q in worst}
                assert max(r.values()) <= 1.0, (steps_done, k, scale, r)
                normal = (v >= 2.0 ** -126) | (v == 0)
                assert normal.all() and np.array_equal(v == 0, (g == 0) & (s.v == 0))       # v' is subnormal nowhere
                if beta1 == 0.0:
                    assert np.array_equal(m.view(np.int32), g.view(np.int32))
    print(f"fp32 emulation, hyper {ac.HYPERS[hyper]}: worst error / bound  p {worst['p']:.3f}  m {worst['m']:.3f}  v {worst['v']:.3f}")
    assert min(r for q, r in worst.items() if not (q == "m" and beta1 == 0.0)) > 0.25       # the bounds are not idle either


def test_inputs_cover_what_the_cases_need(layout):
    x = ac.draw(layout, 1)
    g, m, v, p = x["g"], x["m"], x["v"], x["p"]
    assert ((g == 0) & (v != 0)).any() and ((g == 0) & (v == 0) & (m != 0)).any() and ((g == 0) & (v == 0) & (m == 0)).any()
    assert (p == 0).sum() > 50000 and ((p != 0) & (np.abs(p) <= 1e-3)).sum() > 50000 and (np.abs(p) > 0.5).sum() > 20000
    nz = np.abs(g[g != 0])
    assert nz.min() < 1e-11 and nz.max() > 1e15 and np.isfinite(g).all()
    assert (v >= 0).all() and float(v.max()) < 1e32
    # per record: one magnitude
    big = int(np.argmax(layout.n))
    seg = np.abs(g[layout.first[big] + 3:layout.first[big + 1]])
    assert seg.max() / seg.min() < 1e4


def test_layout_of_the_slots(layout):
    n = layout.n
    assert sorted(set(n[4:4 + 2 * len(ac.SIZES)])) == sorted(ac.SIZES) and (n[:4] == ac.MIXED_N).all()
    assert len(n) == 4 + 2 * len(ac.SIZES) + ac.N_TINY and set(n[-ac.N_TINY:]) == set(range(1, 8))
    for i, q in enumerate(ac.QUANTITIES):                # exactly one of p, g, m, v off the 16-byte grid in records 0..3
        assert [layout.start[r][i] % 4 for r in ac.QUANTITIES] == [1 if r == q else 0 for r in ac.QUANTITIES]
    sized = slice(4, 4 + 2 * len(ac.SIZES))
    assert list(layout.start["p"][sized] % 4) == [0] * len(ac.SIZES) + [1] * len(ac.SIZES)
    empty = [i for i in range(len(n)) if n[i] == 0]
    assert len(empty) == 2 and all(0 < i < len(n) - 1 and n[i - 1] > 0 and n[i + 1] > 0 for i in empty)
    assert {int(s) % 4 for s in layout.start["g"][-ac.N_TINY:]} == {0, 1, 2, 3}             # back to back: every alignment
    host = layout.fill("m", np.zeros(int(n.sum()), dtype=np.float32))
    assert layout.guards_intact("m", host) and (host == f32(ac.GUARD)).sum() == layout.total["m"] - n.sum()
    for at in (int(layout.start["m"][0]) - 1, int(layout.start["m"][5] + n[5]), layout.total["m"] - 1):
        broken = host.copy()
        broken[at] = 0.0
        assert not layout.guards_intact("m", broken)


# ---- 3. the tick ---------------------------------------------------------------------------------------------------------------------
def _nearest_f32(x):
    """the float32 nearest to the Decimal x > 0"""
    c = f32(float(x))
    cands = [np.nextafter(c, f32(0)), c, np.nextafter(c, f32(np.inf))]
    return min(cands, key=lambda f: abs(decimal.Decimal(float(f)) - x))


@pytest.mark.parametrize("beta1,beta2", [(0.5, 0.999), (0.9, 0.999)])
@pytest.mark.parametrize("t", [1, 2, 10, 1000, 100000])
def test_tick_against_sixty_digits(t, beta1, beta2):
    lr = 1e-3
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        D = decimal.Decimal
        b1, b2, lr32 = D(float(f32(beta1))), D(float(f32(beta2))), D(float(f32(lr)))       # Decimal(float) is exact
        want_ss = _nearest_f32(lr32 / (1 - b1 ** t))
        want_isb = _nearest_f32(1 / (1 - b2 ** t).sqrt())
    ss, isb = ac.tick(t, lr, beta1, beta2)
    assert isinstance(ss, np.float32) and isinstance(isb, np.float32)
    assert ss == want_ss and isb == want_isb, (t, ss, want_ss, isb, want_isb)


def test_tick_literals():
    ss, isb = ac.tick(1, 1e-3, 0.5, 0.999)
    assert ss == f32(1e-3) * f32(2) and abs(float(isb) - 31.62298) < 1e-5                # 1 / sqrt(0.00099998713)
    ss, isb = ac.tick(100000, 1e-3, 0.5, 0.999)
    assert ss == f32(1e-3) and isb == f32(1)
    ss, isb = ac.tick(2, 2e-4, 0.9, 0.999)
    want = 2e-4 / (1.0 - float(f32(0.9)) ** 2)
    assert abs(float(ss) - want) <= 2 * ac.U * want and abs(float(isb) - 1 / math.sqrt(1 - 0.999 ** 2)) < 3e-4
    ss, isb = ac.tick(7, 1e-3, 0.0, 0.99)
    assert ss == f32(1e-3)                                                               # beta1 = 0: no bias, 0^t = 0


def test_the_numbers_quoted_for_float32_betas():
    """what the float32 betas of the record cost against the doubles of torch 1.4"""
    b2 = float(f32(0.999))

    def isb(beta, t):
        return 1.0 / math.sqrt(1.0 - beta ** t)
    rel = {t: isb(b2, t) / isb(0.999, t) - 1.0 for t in (1, 1000, 5000, 100000)}
    assert abs(rel[1] - 6.44e-6) < 5e-9 and abs(rel[1000] - 3.75e-6) < 5e-9 and abs(rel[5000] - 2.18e-7) < 5e-9
    assert abs(rel[100000]) < 1e-15
    omb_kernel, omb_torch = f32(1) - f32(0.999), f32(1.0 - 0.999)
    assert abs(float(omb_kernel) - 0.00099998713) < 5e-12 and abs(float(omb_torch) - 0.00100000005) < 5e-12
    assert abs((float(omb_torch) - float(omb_kernel)) / 1e-3 - 1.29e-5) < 5e-8
    c = ac.deviation_constant(0.999)
    assert abs(c - 1.29e-5) < 5e-8 and ac.deviation_constant(0.5) == 0.0
    assert float(omb_kernel) == 1.0 - b2                             # 1.f - b is exact (Sterbenz): the complement carries d whole


# ---- 4. the trajectory bound -----------------------------------------------------------------------------------------------------------
def test_trajectory_bound_holds_for_the_float32_emulation():
    """20 steps from zero at (0.5, 0.999): the float32 emulation of the kernel stays inside the bound against the torch-1.4
    trajectory, and the part of the bound that is not rounding is c sum |upd|"""
    lr, beta1, beta2, eps = ac.HYPERS[0]
    rng = np.random.default_rng(8)
    n = 4099
    mag = 10.0 ** rng.uniform(-6, 3, n)
    grads = [(mag * rng.standard_normal(n)).astype(np.float32) for _ in range(20)]
    want, rounding, total = ac.trajectory(grads, lr, beta1, beta2, eps)
    b1, b2, e = ac.kernel_scalars(beta1, beta2, eps)
    p, m, v = (np.zeros(n, dtype=np.float32) for _ in range(3))
    for t, g in enumerate(grads, 1):
        p, m, v = ac.emulate_f32(p, g, m, v, b1, b2, e, *ac.tick(t, lr, beta1, beta2))
    c = ac.deviation_constant(beta2) + ac.deviation_constant(beta1)
    bound = rounding + c * total
    share = np.abs(p.astype(np.float64) - want) / bound
    print(f"emulated distance to torch 1.4 after 20 steps: worst share of the bound {share.max():.3f}; c = {c:.3e}; "
          f"rounding part / bound = {float((rounding / bound).min()):.3f} .. {float((rounding / bound).max()):.3f}")
    assert share.max() <= 1.0 and abs(c - 1.29e-5) < 5e-8
