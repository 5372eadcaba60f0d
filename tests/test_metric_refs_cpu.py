"""CPU: the yardsticks of the set-metric tests (tests/metric_common.py) and the host-side pieces of the feature -- the float64
references against independent computations, ``kid_subsets``, the pairing schedule and rotation of csrc/metric_math.h run by a
stand-alone host program, the measured Frechet tolerance, the bounds' power to reject wrong estimators, and the argument checks of
the Python functions."""
import collections
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import metric_common as mc

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- 1. the Frechet reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2,d", [(50, 60, 8), (40, 40, 20), (200, 150, 64), (33, 130, 16), (400, 350, 300)], ids=str)
def test_fd_ref64_equals_the_sqrtm_formula(n1, n2, d):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrtm(S1 S2) with scipy, both covariances of full rank (N > D), to 1e-8 relative"""
    from scipy.linalg import sqrtm
    r = np.random.default_rng([21, n1, n2, d])
    x = r.standard_normal((n1, d)) * (0.5 + r.random((1, d)))
    y = r.standard_normal((n2, d)) @ (np.eye(d) + 0.3 * r.standard_normal((d, d)) / np.sqrt(d)) + 0.4
    c1, c2 = np.atleast_2d(np.cov(x, rowvar=False)), np.atleast_2d(np.cov(y, rowvar=False))
    diff = x.mean(axis=0) - y.mean(axis=0)
    want = diff @ diff + np.trace(c1) + np.trace(c2) - 2.0 * np.trace(sqrtm(c1 @ c2)).real
    got = mc.fd_ref64(x, y)
    assert abs(got - want) <= 1e-8 * abs(want), (got, want)


# ---- 2. the KID reference -------------------------------------------------------------------------------------------------------------
def test_kid_ref64_on_three_points_by_hand():
    """D = 2, k(u, v) = (u . v / 2 + 1)^3.  x: dots 0, 1, 1 -> k = 1, 3.375, 3.375, off-diagonal sum 2 * 7.75 = 15.5.
    y: dots 0, 2, 2 -> k = 1, 8, 8, sum 2 * 17 = 34.  x . y: rows (2, 0, 1), (0, 2, 1), (2, 2, 2) -> k rows (8, 1, 3.375),
    (1, 8, 3.375), (8, 8, 8), sum 48.75.  kid = (15.5 + 34) / 6 - 2 * 48.75 / 9."""
    x = np.asarray([[1, 0], [0, 1], [1, 1]], np.float32)
    y = np.asarray([[2, 0], [0, 2], [1, 1]], np.float32)
    want = 49.5 / 6.0 - 97.5 / 9.0
    for table in ([[0, 1, 2]], [[2, 0, 1]]):
        ix = np.asarray(table, np.int32)
        sums, kid = mc.kid_ref64(x, y, ix, ix)
        assert sums.tolist() == [[15.5, 34.0, 48.75]]
        assert abs(kid - want) <= 1e-15
    # two subsets of two points: {x0, x1} with {y0, y2} and {x2, x0} with {y1, y1'}: the mean of the two estimates
    ix, iy = np.asarray([[0, 1], [2, 0]], np.int32), np.asarray([[0, 2], [1, 2]], np.int32)
    sums, kid = mc.kid_ref64(x, y, ix, iy)
    assert sums.tolist() == [[2.0, 16.0, 8 + 3.375 + 1 + 3.375], [6.75, 16.0, 8 + 8 + 1 + 3.375]]
    assert abs(kid - 0.5 * ((18.0 / 2 - 2 * 15.75 / 4) + (22.75 / 2 - 2 * 20.375 / 4))) <= 1e-15


# ---- 3. kid_subsets -------------------------------------------------------------------------------------------------------------------
def test_kid_subsets():
    from srgan_amd.evaluation import kid_subsets
    ix, iy = kid_subsets(50, 70, 9, 20, seed=3)
    assert ix.shape == iy.shape == (9, 20) and ix.dtype == iy.dtype == np.int32
    for tab, n in ((ix, 50), (iy, 70)):
        assert tab.min() >= 0 and tab.max() < n
        assert all(len(set(row.tolist())) == 20 for row in tab)
    jx, jy = kid_subsets(50, 70, 9, 20, seed=3)
    assert np.array_equal(ix, jx) and np.array_equal(iy, jy)
    kx, _ = kid_subsets(50, 70, 9, 20, seed=4)
    assert not np.array_equal(ix, kx)
    assert np.array_equal(ix[4], np.random.default_rng([3, 4, 0]).choice(50, 20, replace=False))
    assert np.array_equal(iy[8], np.random.default_rng([3, 8, 1]).choice(70, 20, replace=False))
    sx, sy = kid_subsets(13, 70, 2, 1000, seed=0)           # m = the smaller set: every row a permutation of it
    assert sx.shape == sy.shape == (2, 13) and sorted(sx[1].tolist()) == list(range(13))


# ---- 4. csrc/metric_math.h through a stand-alone host program -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = os.path.join(str(tmp_path_factory.mktemp("metric_host")), "metric_host_check")
    inc = os.path.join(os.path.dirname(HERE), "style-restricted_gan_amd", "csrc")
    built = subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-I" + inc, os.path.join(HERE, "metric_host_check.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return [line.split() for line in r.stdout.splitlines()]


def test_pairing_schedule_of_the_header(host_program):
    """every even n' in 2..132: each unordered pair exactly once per sweep, no index twice within a round, i < j; the numpy
    restatement the emulation uses gives the same pairs"""
    rounds = collections.defaultdict(list)
    for tag, np_, rnd, slot, i, j in _run(host_program, "pairs", 2, 132):
        assert tag == "P"
        rounds[(int(np_), int(rnd))].append((int(slot), int(i), int(j)))
    assert sorted({k[0] for k in rounds}) == list(range(2, 133, 2))
    for n in range(2, 133, 2):
        seen = collections.Counter()
        for rnd in range(n - 1):
            slots = sorted(rounds[(n, rnd)])
            assert [s for s, _, _ in slots] == list(range(n // 2))
            used = [v for _, i, j in slots for v in (i, j)]
            assert sorted(used) == list(range(n)), (n, rnd)             # every index once: none twice within the round
            assert all(i < j for _, i, j in slots)
            seen.update((i, j) for _, i, j in slots)
            ii, jj = mc.jacobi_pairs(n, rnd)
            assert [(int(a), int(b)) for a, b in zip(ii, jj)] == [(i, j) for _, i, j in slots]
        assert len(seen) == n * (n - 1) // 2 and set(seen.values()) == {1}, n
    # the phantom of an odd count is index n' - 1, which only ever sits in slot 0 as j
    for (n, rnd), slots in rounds.items():
        assert [s for s, i, j in slots if n - 1 in (i, j)] == [0] and sorted(slots)[0][2] == n - 1


def test_rotation_formula_of_the_header(host_program):
    zetas = [0.0, 1e-30, -1e-30, 1.0, -1.0, 1e30, -1e30, 8191.5, -8192.0, 3e38]
    rows = _run(host_program, "rot", *zetas)
    assert len(rows) == len(zetas)
    for (tag, z, t, c, s), zeta in zip(rows, zetas):
        z, t, c, s = (float.fromhex(v) for v in (z, t, c, s))
        assert tag == "R" and z == float(np.float32(zeta))
        assert all(np.isfinite(v) for v in (t, c, s)), (zeta, t, c, s)
        assert abs(c * c + s * s - 1.0) <= 2 * mc.U, (zeta, c, s)
        assert abs(t) <= 1.0 and c > 0
        if zeta != 0:
            assert (t > 0) == (zeta > 0) or t == 0.0, (zeta, t)
            assert t != 0.0 or abs(zeta) >= 1e30
        else:
            assert t == 1.0                                              # +0: the positive root, 45 degrees
        # the smaller root of t^2 + 2 zeta t - 1 = 0, in float64
        want = np.copysign(1.0, z) / (abs(z) + np.hypot(1.0, z))
        if abs(z) >= 1e38:
            continue
        assert abs(t - want) <= 4 * mc.U * abs(want) + 1e-45, (zeta, t, want)
    (tag, k), = _run(host_program, "poly3", 6.0, 4)
    assert tag == "K" and float.fromhex(k) == 2.5 ** 3


# ---- 5. the measured tolerance --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.FD_NAMES)
def test_emulation_converges_and_meets_the_committed_tolerance(name):
    sweeps, rotated, ratio = mc.fd_measure(name)
    print(f"metric fd emulation | {name} | sweeps {sweeps} | ratio {ratio:.3e}")
    assert rotated == 0 and sweeps <= mc.FD_EMUL_SWEEPS, (sweeps, rotated)
    assert ratio <= mc.FD_TOL / 4, ratio
    assert mc.FD_TOL == 4 * mc.FD_WORST_RATIO


def test_orientation_rule_puts_the_smaller_set_on_the_rows():
    """33 x 130 and 130 x 33 (the same pair swapped) give the same W [33, 130], bit for bit: n = min(n1, n2) vectors of length
    L = max(n1, n2).  The other orientation -- 130 vectors that span at most 33 directions, 97 of them zero after the sweeps --
    reaches the same nuclear norm only through the zero-direction rule, and no more accurately (printed, not asserted)."""
    x, y, ref = mc.fd_case("33x130x257 relu")
    x2, y2, ref2 = mc.fd_case("130x33x257 relu swapped")
    assert np.array_equal(x, y2) and np.array_equal(y, x2)
    w, w2 = mc.fd_w_emulated(x, y), mc.fd_w_emulated(x2, y2)
    assert w.shape == (33, 130) and np.array_equal(w, w2)
    assert abs(ref["fd"] - ref2["fd"]) <= 1e-12 * ref["scale"] and abs(ref["nuclear"] - ref2["nuclear"]) <= 1e-12 * ref["nuclear"]
    _, sweeps, rotated, nuclear = mc.jacobi_emulated(np.ascontiguousarray(w.T))
    print(f"metric fd emulation | 130 vectors of length 33 | sweeps {sweeps} | last {rotated} | "
          f"ratio {abs(2 * (nuclear - ref['nuclear'])) / ref['scale']:.3e}")


def test_emulated_w_matches_the_float64_matrix():
    x, y, ref = mc.fd_case("65x63x130 shifted scaled")
    w = mc.fd_w_emulated(x, y)
    assert w.shape == (63, 65) and w.dtype == np.float32
    nuc = np.linalg.svd(w.astype(np.float64), compute_uv=False).sum()
    assert abs(nuc - ref["nuclear"]) <= 1e-5 * ref["nuclear"]


# ---- 6. the bounds are not vacuous ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 65])
def test_kid_bound_rejects_wrong_estimators(m):
    x, y = mc.kid_inputs(m + 5, m + 9, 257)
    ix, iy = mc.kid_tables(m + 5, m + 9, 3, m)
    sums, kid = mc.kid_ref64(x, y, ix, iy)
    bsums, bkid = mc.kid_bound(x, y, ix, iy)
    assert (bsums > 0).all() and bkid > 0
    assert (bsums <= 1e-4 * np.abs(sums)).all() and bkid <= 1e-4 * np.abs(sums[:, 2]).mean() / (m * m)
    for mutation in ("include_diagonal", "biased_m", "no_div"):
        wsums, wkid = mc.kid_ref64(x, y, ix, iy, **{mutation: True})
        assert abs(wkid - kid) > bkid, mutation
        if mutation != "biased_m":
            assert (np.abs(wsums - sums)[:, :2] > bsums[:, :2]).all(), mutation
    # and the fp32 arithmetic it was derived for stays inside: the kernel's epilogue restated on a float64 Gram rounded to fp32
    d = x.shape[1]
    for s in range(ix.shape[0]):
        xs, ys = x[ix[s]].astype(np.float64), y[iy[s]].astype(np.float64)
        g = (xs @ ys.T).astype(np.float32)
        v = g / np.float32(d) + np.float32(1)
        got = (v * v * v).astype(np.float64).sum()
        assert abs(got - sums[s, 2]) <= bsums[s, 2]


def test_gram_and_stats_bounds_are_tight_enough_to_catch_a_wrong_kernel():
    a, b = mc.gram_inputs(65, 33, 257)
    ref, bound = mc.gram_ref64(a, b), mc.gram_bound(a, b)
    assert (bound > 0).all()
    dropped = mc.gram_ref64(a[:, :-1], b[:, :-1])                      # the last feature left out
    assert (np.abs(dropped - ref) > bound).mean() > 0.95
    ai, bi = mc.gram_integer_inputs(65, 33, 4101)
    assert np.abs(mc.gram_ref64(ai, bi)).max() < 2 ** 24 and (np.abs(ai) @ np.abs(bi).T).max() < 2 ** 24
    x = mc.stats_inputs(65, 17, "offset")
    mean, cen, tr = mc.stats_ref64(x)
    biased = tr * 64.0 / 65.0                                           # the covariance divided by N
    assert abs(biased - tr) > mc.trace_bound(x)
    m32 = x.mean(axis=0, dtype=np.float32)                              # a float32 running mean at offset 1000
    assert (mc.mean_bound(x) < 1e-4).all() and (mc.mean_bound(x) >= mc.U * 990).all()
    assert np.abs(m32 - mean).max() < 1e-2


# ---- 7. the argument checks come before the library ------------------------------------------------------------------------------------
def test_argument_checks_raise_before_any_library_call(monkeypatch):
    from srgan_amd import _lib, evaluation as ev

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    f = np.zeros
    with pytest.raises(ValueError, match="4096"):
        ev.compute_frechet_distance(f((4097, 3), np.float32), f((4100, 3), np.float32))
    with pytest.raises(ValueError, match="fewer than 2"):
        ev.compute_frechet_distance(f((1, 3), np.float32), f((5, 3), np.float32))
    with pytest.raises(ValueError, match="fewer than 2"):
        ev.compute_frechet_distance(f((5, 3), np.float32), f((1, 3), np.float32))
    with pytest.raises(ValueError, match="dimensions differ"):
        ev.compute_frechet_distance(f((5, 3), np.float32), f((5, 4), np.float32))
    with pytest.raises(ValueError, match="dimensions differ"):
        ev.compute_kid(f((5, 3), np.float32), f((5, 4), np.float32))
    with pytest.raises(ValueError, match="at least 2"):
        ev.compute_kid(f((1, 3), np.float32), f((5, 3), np.float32))
    with pytest.raises(ValueError, match="at least 2"):
        ev.compute_kid(f((5, 3), np.float32), f((5, 3), np.float32), max_subset_size=1)
    with pytest.raises(ValueError, match="num_subsets"):
        ev.compute_kid(f((5, 3), np.float32), f((5, 3), np.float32), num_subsets=0)
    with pytest.raises(ValueError, match="matrices"):
        ev.compute_kid(f((5,), np.float32), f((5, 3), np.float32))
    # a larger set above the limit is fine as long as the smaller one is not: the check passes and the library is reached
    with pytest.raises(AssertionError, match="before the arguments"):
        ev.compute_frechet_distance(f((4, 3), np.float32), f((5000, 3), np.float32))
    for name in ("compute_frechet_distance", "compute_kid", "kid_subsets"):
        assert name in ev.__all__
    for name in ("get_fd", "get_kid", "get_metrics"):
        assert callable(getattr(ev.GAN_evaluation, name))


def test_abi_lists_the_metric_entries():
    from srgan_amd import _lib
    header = open(os.path.join(os.path.dirname(HERE), "include", "srgan_hip.h")).read()
    for name in ("srgan_gram_f32", "srgan_feature_stats_workspace", "srgan_feature_stats", "srgan_kid_workspace", "srgan_kid_poly3",
                 "srgan_jacobi_workspace", "srgan_jacobi_sweep", "srgan_nuclear_from_rows"):
        assert name in _lib.SIGNATURES and name + "(" in header
