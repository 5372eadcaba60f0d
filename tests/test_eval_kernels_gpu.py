"""GPU: the evaluation kernels (csrc/evaluation.hip) against exact references, through the C ABI on guarded memory -- every
output and workspace lies between two regions of pattern bytes that must be intact after every call, and the workspace has
exactly the bytes srgan_prdc_workspace returns.  References, case lists and the derivation of the distance bound live in
tests/eval_common.py (pinned without a GPU by tests/test_eval_refs_cpu.py).
  pairwise distances   |got - ref64| <= 12 * 2^-24 * ref64 per element, 0 where ref64 == 0
  k-th smallest        equality with np.sort(row)[k - 1]
  PRDC statistics      equality with the four formulas in float64 -> float32
  compute_prdc         equality with the oracle where float64 proves that no comparison is within the distances' error
  max pool             equality with torch.nn.functional.max_pool2d, NaN included
SRGAN_TEST_LOG=1 prints the worst err / bound of every distance case."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import eval_common as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from srgan_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(scope="module")
def lib():
    from srgan_amd import _lib
    return _lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def run_dist(ops, lib, x, y, same=False, skew=0):
    """srgan_pairwise_dist on guarded memory -> the matrix on the host.  ``same``: x is passed as y too."""
    ar = ec.Arena()
    n, d = x.shape
    xd = ar.put(x, "x", skew=skew)
    yd = xd if same else ar.put(y, "y", skew=skew)
    m = n if same else y.shape[0]
    out = ar.out((n, m), "dist")
    lib.check(lib.load().srgan_pairwise_dist(_p(xd), n, _p(yd), m, d, _p(out), ops._stream()), "pairwise_dist")
    torch.cuda.synchronize()
    ar.intact("pairwise_dist")
    return out.cpu().numpy()


def hold_dist(got, ref64, what):
    bad, ratio = ec.dist_violations(got, ref64)
    if os.environ.get("SRGAN_TEST_LOG"):
        print(f"eval pairwise_dist | {what} | err/bound {ratio:.3f}")
    assert bad == 0, f"{what}: {bad} elements beyond {ec.DIST_ULPS} * 2^-24 relative (worst err / bound {ratio:.3f})"


@pytest.mark.parametrize("case", ec.DIST_CASES, ids=lambda c: c["name"])
def test_pairwise_dist_per_element(ops, lib, case):
    x, y = case["make"]()
    hold_dist(run_dist(ops, lib, x, y), ec.dist_ref64(x, y), case["name"])


def test_pairwise_dist_exact_on_integer_coordinates(ops, lib):
    """Squared distances that are perfect squares of small integers: every fp32 step is exact, so is the result."""
    x, y, want = ec.exact_case()
    got = run_dist(ops, lib, x, y)
    known = want >= 0
    assert np.array_equal(got[known], want[known].astype(np.float32))
    hold_dist(got, ec.dist_ref64(x, y), "integer coordinates")


@pytest.mark.parametrize("n,d", [(65, 17), (129, 4101)])
def test_pairwise_dist_of_a_set_with_itself(ops, lib, n, d):
    """x passed as y: the diagonal is exactly 0 and the matrix exactly symmetric ((a - b)^2 == (b - a)^2 term by term)."""
    x, _ = ec._cloud(n, 1, d, 11)
    x = x + np.float32(3.0)
    got = run_dist(ops, lib, x, None, same=True)
    assert np.array_equal(np.diag(got), np.zeros(n, np.float32))
    assert np.array_equal(got, got.T)
    hold_dist(got, ec.dist_ref64(x, x), "self distances")


def test_pairwise_dist_unaligned_inputs(ops, lib):
    """Both input pointers one float past a 16-byte boundary."""
    x, y = ec._cloud(65, 63, 17, 12)
    got = run_dist(ops, lib, x, y, skew=4)
    assert np.array_equal(got, run_dist(ops, lib, x, y))
    hold_dist(got, ec.dist_ref64(x, y), "unaligned")


def test_pairwise_dist_compensation_is_needed_and_works(ops, lib):
    """N = M = 8, D = 2^20: the plain fp32 sum of the 65536 chunk sums breaks the bound on the CPU emulation
    (tests/test_eval_refs_cpu.py), so a kernel that lost its compensation fails here."""
    x, y, ref = ec.sensitivity_case()
    hold_dist(run_dist(ops, lib, x, y), ref, f"sensitivity D = {ec.SENS_D}")


# ---- k-th smallest --------------------------------------------------------------------------------------------------------------------
def run_kth(ops, lib, rows, k):
    ar = ec.Arena()
    n, m = rows.shape
    d = ar.put(rows, "rows")
    out = ar.out((n,), "kth")
    lib.check(lib.load().srgan_kth_smallest_rows(_p(d), n, m, k, _p(out), ops._stream()), "kth_smallest_rows")
    torch.cuda.synchronize()
    ar.intact("kth_smallest_rows")
    return out.cpu().numpy()


@pytest.mark.parametrize("m", ec.KTH_M)
def test_kth_smallest_is_exact(ops, lib, m):
    """Every row kind alone (N = 1) and in groups of five (N = 5: one full workgroup of four waves and one wave of the next),
    every k in 1 .. min(16, M) -- M == k included."""
    rows = ec.kth_rows(m)
    stack = np.stack([r for _, r in rows])
    fives = [np.arange(s, s + 5) % len(rows) for s in range(0, len(rows), 5)]
    for k in range(1, min(ec.KTH_MAX, m) + 1):
        want = ec.kth_ref(stack, k)
        for i, (name, row) in enumerate(rows):
            got = run_kth(ops, lib, row[None, :], k)
            assert np.array_equal(got, want[i:i + 1]), (m, k, name, got, want[i])
        for idx in fives:
            got = run_kth(ops, lib, stack[idx], k)
            assert np.array_equal(got, want[idx]), (m, k, [rows[i][0] for i in idx], got, want[idx])


# ---- PRDC from a given matrix ---------------------------------------------------------------------------------------------------------
def run_prdc(ops, lib, dist, r_real, r_fake, k, short=0):
    ar = ec.Arena()
    n, m = dist.shape
    L = lib.load()
    nb = L.srgan_prdc_workspace(n, m)
    assert nb == (2 * n + m) * 4
    d, rr, rf = ar.put(dist, "dist"), ar.put(r_real, "r_real"), ar.put(r_fake, "r_fake")
    out, ws = ar.out((4,), "out4"), ar.raw(nb, "workspace")
    code = L.srgan_prdc_from_dist(_p(d), n, m, _p(rr), _p(rf), k, _p(out), _p(ws), nb - short, ops._stream())
    torch.cuda.synchronize()
    ar.intact("prdc_from_dist")
    return code, out.cpu().numpy(), ws


@pytest.mark.parametrize("n,m", ec.PRDC_SHAPES)
def test_prdc_from_a_given_matrix(ops, lib, n, m):
    for name, dist, r_real, r_fake, k in ec.prdc_matrix_cases(n, m):
        code, got, _ = run_prdc(ops, lib, dist, r_real, r_fake, k)
        lib.check(code, "prdc_from_dist")
        want = ec.prdc_formulas(dist, r_real, r_fake, k)
        assert np.array_equal(got, want), (name, got, want)


def test_prdc_workspace_too_small_is_an_error(ops, lib):
    name, dist, r_real, r_fake, k = ec.prdc_matrix_cases(64, 64)[0]
    code, got, ws = run_prdc(ops, lib, dist, r_real, r_fake, k, short=1)
    assert code != 0 and b"workspace too small" in lib.load().srgan_last_error()
    assert bool((ws == ec.PATTERN).all()) and bool((torch.as_tensor(got).view(torch.uint8) == ec.PATTERN).all())   # nothing ran


# ---- compute_prdc end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.E2E_CASES, ids=lambda c: "n{}_m{}_d{}_k{}".format(*c))
def test_compute_prdc_equals_the_oracle(case):
    """No comparison of the algorithm is within 24 * 2^-24 relative in float64 (asserted by the CPU test), so the fp32 distances
    and radii (12 * 2^-24 each) decide every one of them as float64 does: the four numbers are the oracle's."""
    from oracle import evaluation as oe
    from srgan_amd.evaluation import compute_prdc
    real, fake, want, margin = ec.e2e_reference(case)
    assert margin > ec.MARGIN_ULPS * ec.U
    got = compute_prdc(real, fake, case[3])
    got = np.asarray([got["precision"], got["recall"], got["density"], got["coverage"]], np.float32)
    ref = oe.compute_prdc(real, fake, case[3])
    ref = np.asarray([ref["precision"], ref["recall"], ref["density"], ref["coverage"]], np.float64).astype(np.float32)
    assert np.array_equal(want, ref)                      # the formulas of eval_common are the oracle's
    assert np.array_equal(got, ref), (got, ref)


# ---- max pool -------------------------------------------------------------------------------------------------------------------------
def run_pool(ops, lib, x):
    """srgan_maxpool2_fwd on the NHWC tensor [n, h, w, c] -> the device output [n, h/2, w/2, c]."""
    ar = ec.Arena()
    n, h, w, c = x.shape
    xd = ar.put(x, "x")
    out = ar.out((n, h // 2, w // 2, c), "y")
    lib.check(lib.load().srgan_maxpool2_fwd(_p(xd), _p(out), n, h, w, c, ops._stream()), "maxpool2_fwd")
    torch.cuda.synchronize()
    ar.intact("maxpool2_fwd")
    return out


@pytest.mark.parametrize("kind", ["normal", "negative", "-inf", "+inf"])
def test_maxpool2_equals_torch(ops, lib, kind):
    for shape in ec.POOL_SHAPES:
        x = ec.pool_input(shape, kind)
        assert torch.equal(run_pool(ops, lib, x).cpu(), ec.pool_ref(x)), (kind, shape)


def test_maxpool2_beyond_the_grid_cap(ops, lib):
    """More items than the 16384 workgroups of 256 lanes cover in one pass: the grid-stride loop runs."""
    n, c, h, w = ec.POOL_BIG
    assert n * (h // 2) * (w // 2) * (c // 4) > ec.POOL_GRID_CAP
    x = ec.pool_input(ec.POOL_BIG, "normal")
    got = run_pool(ops, lib, x)
    assert torch.equal(got, ec.pool_ref(x).cuda())


@pytest.mark.parametrize("pos", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_maxpool2_propagates_nan(ops, lib, pos):
    """nn.MaxPool2d gives NaN for a window that holds one, wherever it stands; the other windows are untouched."""
    for shape in ((1, 4, 7, 9), (2, 8, 6, 10)):
        x = ec.pool_input(shape, "normal")
        x[:, pos[0]::4, pos[1]::6, ::3] = float("nan")          # some windows, some channels
        x[0, 2 + pos[0], 2 + pos[1], 1] = float("nan")          # with +inf in the same window
        x[0, 2 + (1 - pos[0]), 2 + (1 - pos[1]), 1] = float("inf")
        want = ec.pool_ref(x)
        assert bool(torch.isnan(want).any()) and not bool(torch.isnan(want).all())
        assert ec.same_with_nan(run_pool(ops, lib, x).cpu(), want), (pos, shape)
