"""CPU: the yardsticks of tests/test_small_kernels_gpu.py are pinned here, without a GPU -- the float64 references reproduce
the reference project's recorded numbers, every latent-loss case is well conditioned, the degenerate ones are finite in
float64, and the error measure rejects what it should."""
import os

import numpy as np
import pytest
import torch

from oracle import losses as ol
from tests import small_common as sc


def test_float64_references_reproduce_the_recorded_latent_losses(golden_dir):
    """tests/golden/losses.npz: values and per-term gradients the reference project computed in float32.  The float64
    restatement agrees with them within the bound the GPU tests use (max(8 * e32, gamma), B = 32 rows per sum)."""
    gold = np.load(os.path.join(golden_dir, "losses.npz"))
    target = torch.from_numpy(gold["hist_target_seed0"])
    for name in ("randn1234", "sin"):
        args = (torch.from_numpy(gold[f"{name}_mu"]), 32, target, 50, 10.0, 0.2)
        t64, t32 = sc.latent_terms(*args, torch.float64), sc.latent_terms(*args, torch.float32)
        for i, key in enumerate(("dbkl", "dcorr", "dhist")):
            sc.check("golden", f"{name} vals[{i}]", torch.tensor(gold[f"{name}_vals"][i]), t64[0][i], t32[0][i], 32)
            sc.check("golden", f"{name} {key}", torch.from_numpy(gold[f"{name}_{key}"]), t64[1][i], t32[1][i], 32)
        sc.check("golden", f"{name} pearson", torch.from_numpy(np.corrcoef(gold[f"{name}_mu"].astype(np.float64).T)), t64[2], t32[2], 32)


def test_float64_soft_histogram_reproduces_the_recorded_target(golden_dir):
    """hist_target_seed0: the reference constructor's draw of 100 000 samples through GaussianHistogram, in float32."""
    gold = np.load(os.path.join(golden_dir, "losses.npz"))
    torch.manual_seed(0)
    sample = torch.randn(100000, 1)[:, 0]
    g = torch.ones(50)
    (h64, _), (h32, _) = (sc.soft_hist_ref(sample, g, 50, -10.0, 10.0, 0.2, dt) for dt in (torch.float64, torch.float32))
    # the recorded target is one float32 evaluation (its sum over 100 000 samples is torch's pairwise one: L = 50 bins for the
    # normaliser dominates)
    sc.check("golden", "hist_target_seed0", torch.from_numpy(gold["hist_target_seed0"]), h64 / h64.sum() + 1e-8, h32 / h32.sum() + 1e-8, 50)
    # chunking the sample changes nothing but the summation order
    whole = ol.soft_histogram(sample.double())
    assert sc.rel_err(h64, whole) <= 1e-13


ALL_LATENT = sc.LATENT_CASES + [sc.LATENT_LIMIT_CASE, sc.LATENT_PUBLIC_CASE]


def test_latent_case_list_covers_what_it_claims():
    shapes = {(c["B"], c["d"], c["n_batch"]) for c in ALL_LATENT}
    assert {(4, 2, 4), (7, 5, 7), (32, 8, 32), (64, 8, 32), (33, 3, 40), (257, 16, 257), (300, 3, 300), (1024, 16, 1024)} <= shapes
    assert {c["bins"] for c in ALL_LATENT} >= {1, 7, 50, 64}
    assert any((c["range_max"], c["sigma"]) != (10.0, 0.2) for c in ALL_LATENT)
    assert sc.LATENT_LIMIT_CASE["B"] * sc.LATENT_LIMIT_CASE["d"] == 16384
    for c in ALL_LATENT:
        assert c["B"] >= c["d"] + 2 and 2 <= c["d"] <= 16 and 1 <= c["bins"] <= 64 and c["B"] * c["d"] <= 16384, c["name"]
        assert set(c["weights"]) >= set(sc.ALL_W[:3])
        assert c["weights"] == sc.ALL_W or c["bins"] == 1, c["name"]     # the histogram term alone everywhere it has a gradient
    assert len({c["name"] for c in ALL_LATENT}) == len(ALL_LATENT)


@pytest.mark.parametrize("case", ALL_LATENT, ids=[c["name"] for c in ALL_LATENT])
def test_latent_cases_are_well_conditioned(case):
    """A condition on the INPUTS: the +-1 clamp and the kink of |r| are not in play, no column is near-constant and every
    column has histogram mass -- so a float32 evaluation differs from float64 by rounding, not by a branch."""
    r_min, r_max, sd_min, mass_min = sc.conditioning(case)
    assert 1e-4 <= r_min and r_max <= 0.9, (r_min, r_max)
    assert sd_min >= 0.1, sd_min
    assert mass_min >= 1e-3, mass_min
    t64, t32 = sc.latent_yardstick(case)
    assert all(bool(torch.isfinite(t).all()) for t in (t64[0], *t64[1], t64[2], t32[0], *t32[1], t32[2]))


def test_degenerate_inputs_are_finite_in_float64():
    """What the three degenerate GPU cases are held to exists: the float64 term that IS asked for is finite on each input."""
    far = sc.degenerate_far_column().double().requires_grad_(True)
    v = ol.batch_kl(far, 32)
    assert bool(torch.isfinite(v)) and bool(torch.isfinite(torch.autograd.grad(v, far)[0]).all())
    # ... and the term that is NOT asked for is what float32 cannot evaluate there: the column's histogram mass underflows
    mass32 = ol.soft_histogram(far.detach().float()[:, 3]).sum()
    assert float(mass32) == 0.0 and float(ol.soft_histogram(far.detach()[:, 3]).sum()) > 0.0
    hi = ol.HistogramImitation(target=ol.analytic_hist_target())
    for make in (sc.degenerate_constant_column, sc.degenerate_identical_columns):
        x = make().double().requires_grad_(True)
        v = hi.loss(x)
        assert bool(torch.isfinite(v)) and bool(torch.isfinite(torch.autograd.grad(v, x)[0]).all())
    const = sc.degenerate_constant_column().double()
    assert not bool(torch.isfinite(ol.batch_kl(const, 32)))              # log(0): the term histogram_imitation.loss does not want
    assert float(ol.corrcoef(sc.degenerate_identical_columns().double().t())[1, 5]) > 1.0 - 1e-12


def test_error_measure_has_teeth():
    ref = torch.linspace(-2.0, 3.0, 64, dtype=torch.float64)
    f32 = ref.float()
    sc.check("measure", "float32 rounding", f32, ref, f32, 1)
    assert sc.rel_err(ref * (1 + 1e-3), ref) == pytest.approx(1e-3, rel=1e-6)
    for bad in (ref * (1 + 1e-4), ref + 3e-5, torch.where(ref > 2.9, torch.full_like(ref, float("nan")), ref)):
        with pytest.raises(AssertionError):
            sc.check("measure", "wrong", bad, ref, f32, 64)
    assert sc.gamma(32) == 48 * 2.0 ** -23


def test_references_of_the_other_kernels():
    """Closed forms the float64 restatements must give, and the case lists hold the sizes at which the kernels change path."""
    mu, lv = torch.tensor([0.5, -1.0]).double(), torch.tensor([0.0, 1.0]).double()
    assert float(sc.kl_normal_ref(0.1)(mu, lv)) == pytest.approx(0.1 * -0.5 * ((1 - 0.25 - 1) + (2 - 1 - np.e)))
    a, b = sc.l1_inputs(2049)
    assert int((a == b).sum()) == len(range(3, 2049, 7))
    assert [sc.l1_blocks(n) for n in sc.L1_SIZES] == [1, 1, 1, 2, 147, 1024]
    assert [sc.soft_hist_blocks(c[0]) for c in sc.SOFT_HIST_CASES] == [1, 1, 1, 256, 256, 256]
    assert any(c[0] > 1024 * 256 for c in sc.SOFT_HIST_CASES) and any(c[1] > 64 for c in sc.SOFT_HIST_CASES)
    x, _ = sc.soft_hist_inputs(255, 64)
    assert float(x.max()) > 10.0 and float(x.min()) < -3.0                 # samples outside either range
    for case in sc.LINCOMB_CASES:
        x, w = sc.lincomb_inputs(case)
        out, grad = sc.lincomb_ref(case, torch.float64, 2.0)
        assert float(out) == pytest.approx(float((w * x[case["slots"]]).sum()))
        assert float(grad.sum()) == pytest.approx(2.0 * float(w.sum()))
        assert bool((w == 0).any()) or case["n"] == 1
        # |out| is not a cancelled remainder of its terms: the float32 evaluation stays within gamma of float64
        assert sc.rel_err(sc.lincomb_ref(case, torch.float32)[0], out) <= sc.gamma(case["n"])
    assert sc.POINTWISE_BIG > 8192 * 256
    x = torch.tensor([[[[1.0, 3.0, 5.0], [7.0, 9.0, 11.0], [2.0, 4.0, 6.0]]]]).double()
    assert sc.pool2_ref(x).flatten().tolist() == [5.0]
    assert sc.pool3_ref(x).flatten().tolist() == [5.0, 7.0, 5.5, 7.5]
