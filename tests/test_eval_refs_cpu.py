"""CPU: the yardsticks of tests/eval_common.py, which tests/test_eval_kernels_gpu.py holds csrc/evaluation.hip to.
The emulation of the distance kernel's fp32 order meets the derived bound on every case (so the bound can be met); without the
compensation it breaks the bound at the sensitivity case (so the case tests the compensation); the k-th, PRDC and end-to-end
case lists contain what their tests claim to exercise."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import evaluation as oe
from tests import eval_common as ec

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "style-restricted_gan_amd", "csrc", "evaluation.hip")


def test_constants_follow_the_source():
    src = open(HIP).read()
    assert re.search(r"PD_T = 64, PD_K = (\d+)", src).group(1) == str(ec.PD_K)
    assert re.search(r"constexpr int KTH_MAX = (\d+)", src).group(1) == str(ec.KTH_MAX)
    assert "16384" in src and ec.POOL_GRID_CAP == 16384 * 256


@pytest.mark.parametrize("case", ec.DIST_CASES, ids=lambda c: c["name"])
def test_emulation_meets_the_distance_bound(case):
    x, y = case["make"]()
    bad, ratio = ec.dist_violations(ec.dist_emulated(x, y), ec.dist_ref64(x, y))
    assert bad == 0 and ratio < 1.0, (case["name"], bad, ratio)


def test_distance_cases_cover_what_the_issue_lists():
    ns, ms, ds = zip(*ec.DIST_SHAPES)
    assert set(ns) == set(ms) == {1, 63, 64, 65, 129} and set(ds) == {1, 3, 15, 16, 17, 4101}
    assert {(-(-n // 64), -(-m // 64)) for n, m, _ in ec.DIST_SHAPES} >= {(1, 1), (1, 2), (2, 1), (2, 2), (1, 3), (3, 1), (3, 3)}
    x, y = ec._offset_case()["make"]()
    assert x.min() > 990 and y.min() > 990
    for d in (17, 4101):
        x, y = ec._near_case(d)["make"]()
        near = np.diag(ec.dist_ref64(x[:63], y))
        assert 0.3e-4 < near.min() and near.max() < 3e-4 and np.abs(x).max() > 1


def test_float64_reference_is_the_oracles():
    x, y = ec._cloud(65, 63, 17, 1)
    assert np.allclose(ec.dist_ref64(x, y), oe.pairwise_distance(x, y), rtol=1e-13, atol=0)


def test_emulation_is_exact_on_integer_coordinates():
    x, y, want = ec.exact_case()
    known = want >= 0
    assert known.sum() == 60 and set(np.unique(want[known])) >= {3.0, 5.0, 13.0, 25.0, 41.0}
    assert np.array_equal(ec.dist_ref64(x, y)[known], want[known])
    assert np.array_equal(ec.dist_emulated(x, y)[known], want[known].astype(np.float32))


def test_sensitivity_case_needs_the_compensation():
    """D = 2^20 separates the two: measured err / bound 0.08 compensated, 6.5 plain (48 of 64 elements beyond the bound)."""
    x, y, ref = ec.sensitivity_case()
    bad, ratio = ec.dist_violations(ec.dist_emulated(x, y, compensated=True), ref)
    assert bad == 0 and ratio < 1.0, (bad, ratio)
    bad, ratio = ec.dist_violations(ec.dist_emulated(x, y, compensated=False), ref)
    assert bad > 0 and ratio > 1.0, (bad, ratio)


def test_dist_violations_counts_what_it_should():
    ref = np.asarray([[0.0, 1.0, 2.0]])
    assert ec.dist_violations(np.asarray([[0.0, 1.0, 2.0]], np.float32), ref) == (0, 0.0)
    assert ec.dist_violations(np.asarray([[1e-30, 1.0, 2.0]], np.float32), ref)[0] == 1            # 0 must stay 0
    assert ec.dist_violations(np.asarray([[0.0, 1.0 + 14 * ec.U, 2.0]], np.float32), ref)[0] == 1
    assert ec.dist_violations(np.asarray([[0.0, 1.0 + 12 * ec.U, 2.0]], np.float32), ref)[0] == 0
    assert ec.dist_violations(np.asarray([[0.0, np.nan, 2.0]], np.float32), ref)[0] == 1


# ---- k-th smallest --------------------------------------------------------------------------------------------------------------------
def test_kth_rows_contain_the_hard_cases():
    assert ec.KTH_M == (1, 16, 17, 63, 64, 65, 1025) and {1, 16} <= set(ec.KTH_M)       # M == k at k = 1 and k = 16
    for m in ec.KTH_M:
        rows = dict(ec.kth_rows(m))
        assert all(r.shape == (m,) and r.dtype == np.float32 for r in rows.values())
        assert np.isinf(rows["every third +inf"]).any() and np.isinf(rows["one finite"]).sum() == m - 1
        assert len(np.unique(rows["three values"])) <= 3 and len(np.unique(rows["all equal"])) == 1
        assert ("lane 63" in rows) == (m >= 64) and "lane 0" in rows
        for c in (0, 63):
            row = rows.get(f"lane {c}")
            if row is None:
                continue
            k = min(ec.KTH_MAX, len(range(c, m, ec.WAVE)))
            assert set(np.argsort(row, kind="stable")[:k] % ec.WAVE) == {c}             # the k smallest: one lane's columns
    assert len(range(63, 1025, 64)) == 16 and len(range(0, 1025, 64)) == 17               # a full register list in both lanes
    assert any(m < ec.WAVE for m in ec.KTH_M)                                            # lanes with an empty list


def test_kth_ref_is_the_oracles_kth_value():
    for m in (17, 1025):
        stack = np.stack([r for _, r in ec.kth_rows(m)])
        for k in (1, 5, 16):
            assert np.array_equal(ec.kth_ref(stack, k), oe.kth_value(stack, k))


# ---- PRDC -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", ec.PRDC_SHAPES)
def test_prdc_matrix_cases_are_decisive(n, m):
    """Expected values of the three named cases; the tie cases change under <= (so a kernel that wrote <= fails them)."""
    cases = {c[0]: c for c in ec.prdc_matrix_cases(n, m)}
    _, d, rr, rf, k = cases["all inside"]
    assert np.array_equal(ec.prdc_formulas(d, rr, rf, k), np.asarray([1, 1, n / k, 1], np.float32))
    _, d, rr, rf, k = cases["none inside"]
    assert np.array_equal(ec.prdc_formulas(d, rr, rf, k), np.zeros(4, np.float32))
    _, d, rr, rf, k = cases["ties only"]
    assert (d == rr[:, None]).all() and (d == rf[None, :]).all()
    assert np.array_equal(ec.prdc_formulas(d, rr, rf, k), np.zeros(4, np.float32))
    assert np.array_equal(ec.prdc_formulas(d, rr, rf, k, np.less_equal), np.asarray([1, 1, n / k, 1], np.float32))
    for name, d, rr, rf, k in cases.values():
        assert set(np.unique(d)) <= set(range(10)) and set(np.unique(2 * rr)) | set(np.unique(2 * rf)) <= set(range(19))
        want = ec.prdc_formulas(d, rr, rf, k)
        ref = oe_from_matrix(d, rr, rf, k)
        assert np.array_equal(want, ref), name
        if name.startswith("single"):
            assert np.array_equal(want, np.asarray([1 / m, 1 / n, 1 / (k * m), 1 / n], np.float64).astype(np.float32)), name
    if n * m > 1:
        _, d, rr, rf, k = cases["mixed"]
        ties = [bool((d == rr[:, None]).any()), bool((d == rf[None, :]).any())]
        assert all(ties) if min(n, m) > 1 else any(ties)
        assert not np.array_equal(ec.prdc_formulas(d, rr, rf, k), ec.prdc_formulas(d, rr, rf, k, np.less_equal))


def oe_from_matrix(d, r_real, r_fake, k):
    """The body of oracle.evaluation.compute_prdc after its distances and radii, as written there."""
    d, r_real, r_fake = d.astype(np.float64), r_real.astype(np.float64), r_fake.astype(np.float64)
    inside_real = d < r_real[:, None]
    out = [inside_real.any(axis=0).mean(), (d < r_fake[None, :]).any(axis=1).mean(),
           (1.0 / float(k)) * inside_real.sum(axis=0).mean(), (d.min(axis=1) < r_real).mean()]
    return np.asarray(out, np.float64).astype(np.float32)


def test_prdc_shapes_cross_the_block_borders():
    assert ec.PRDC_SHAPES == [(1, 1), (1, 300), (300, 1), (257, 300), (64, 64)]
    assert any(m > 256 for _, m in ec.PRDC_SHAPES) and any(n > 256 for n, _ in ec.PRDC_SHAPES)


@pytest.mark.parametrize("case", ec.E2E_CASES, ids=lambda c: "n{}_m{}_d{}_k{}".format(*c))
def test_end_to_end_cases_have_no_near_tie(case):
    """In float64 no distance lies within 24 * 2^-24 (relative) of a radius it is compared with, so distances and radii that
    are each within 12 * 2^-24 decide every comparison alike.  The oracle's own distances give the same four numbers."""
    real, fake, want, margin = ec.e2e_reference(case)
    assert margin > ec.MARGIN_ULPS * ec.U, margin / ec.U
    ref = oe.compute_prdc(real, fake, case[3])
    ref = np.asarray([ref["precision"], ref["recall"], ref["density"], ref["coverage"]], np.float64).astype(np.float32)
    assert np.array_equal(want, ref)
    assert 0 < want[0] and 0 < want[2] and 0 < want[1]       # not a degenerate pair of sets


def test_end_to_end_cases_cover_what_the_issue_lists():
    assert any(n != m for n, m, *_ in ec.E2E_CASES) and any(d == 4096 for _, _, d, *_ in ec.E2E_CASES)
    assert any(k + 1 == m for _, m, _, k, _ in ec.E2E_CASES)                             # a radius that is the row's maximum


# ---- max pool -------------------------------------------------------------------------------------------------------------------------
def test_pool_reference_and_inputs():
    n, c, h, w = ec.POOL_BIG
    assert n * (h // 2) * (w // 2) * (c // 4) > ec.POOL_GRID_CAP and n * c * h * w * 4 < 270e6
    assert any(s[2] % 2 and s[3] % 2 for s in ec.POOL_SHAPES)
    x = ec.pool_input((1, 4, 7, 9), "-inf")
    ref = ec.pool_ref(x)
    assert ref.shape == (1, 3, 4, 4) and bool(torch.isinf(ref).any())
    assert bool((ec.pool_ref(ec.pool_input((2, 8, 6, 10), "negative")) < 0).all())
    x = ec.pool_input((1, 4, 4, 4), "normal")
    x[0, 1, 1, 2] = float("nan")
    ref = ec.pool_ref(x)
    assert bool(torch.isnan(ref[0, 0, 0, 2])) and int(torch.isnan(ref).sum()) == 1       # torch propagates: the reference does
    assert ec.same_with_nan(ref, ref.clone()) and not ec.same_with_nan(ref, torch.nan_to_num(ref, nan=0.0))
