"""Yardsticks of the set-metric tests (csrc/metrics.hip, csrc/metric_math.h): float64 references written from the published
definitions, the derived error bounds, a numpy float32 emulation of the Jacobi sweep and the seeded case lists.
tests/test_metric_refs_cpu.py pins what is in here without a GPU, tests/test_metric_kernels_gpu.py and
tests/test_metric_api_gpu.py hold the HIP kernels to it.  u = 2^-24 throughout; no measured number enters a derived bound.

Gram, per entry.  The kernel's entry is the fp32 fma chain over the D features: |got - ref64| <= (D + 1) u sum_k |a_k b_k|
(``gram_bound``).  On small-integer inputs every partial sum is an integer below 2^24: equality.

Means (``mean_bound``).  u |mean64| for the one fp32 rounding of the float64 mean, plus N 2^-53 mean|x| for the float64 sum of N
terms and the division.

Centred matrix and trace (``centred_bound``, ``trace_bound``).  With d = x - mean64 and r = sqrt(N - 1): the kernel forms
fl(fl(x - mean32) / fl(r)).  |d' - d| <= dm + u (|d| + dm) =: dd (mean error dm, one rounded subtraction); the rounded root and
the rounded division are two relative errors: |a' - d / r| <= (dd + 2.01 u (|d| + dd)) / r =: da.  a'^2 is exact in float64, so
|trace' - trace| <= sum (2 |a| da + da^2) + N D 2^-53 trace (the float64 sum).

KID (``kid_bound``).  Per entry, with g the float64 Gram entry, dG its Gram bound and v = g / D + 1: the epilogue is
fl(fl(g' / D) + 1) cubed by two rounded products.  The division contributes u (|g| + dG) / D, the addition u |v'|:
dv = (dG / D + u (|g| + dG) / D + u |v|) / (1 - u), and |k' - v^3| <= 3 (|v| + dv)^2 dv + 2.01 u (|v| + dv)^3.  To first order
this is 3 v^2 dG / D + c u |v^3| with c = 5 (three from the rounded addition through the cube, two from the two products), plus
3 v^2 u |g| / D for the rounded division, which c u |v^3| does not cover where g / D is near -1.  The bound of a sum is the sum
of its entries' bounds (the diagonal left out where the sum leaves it out) plus m^2 2^-53 sum |k| for the float64 additions; the
bound of the estimate combines the three with the estimator's weights.

Frechet distance.  One-sided Jacobi has no tight closed-form forward bound, so FD_TOL is measured, on the CPU, from
``jacobi_emulated`` -- the kernel's schedule, skip rule and rotation in numpy float32 -- over FD_CASES: the worst
|2 (nuclear_emulated - nuclear_64)| / S with S = |mu1 - mu2|^2 + tr S1 + tr S2, times 4 (the kernel's shuffle / LDS order inside
the three dot products differs from numpy's pairwise sums, and its W comes from an fp32 Gram).  The GPU result is held to
|fd_gpu - fd_ref64| <= FD_TOL * S, never to itself.  tests/test_metric_refs_cpu.py re-measures every case against FD_TOL / 4.
"""
import functools

import numpy as np

from tests.eval_common import Arena  # noqa: F401  (the guarded device memory of the C-ABI tests)

U = 2.0 ** -24
EPS32 = np.float32(2.0 ** -23)
FD_MAX_SWEEPS = 30               # compute_frechet_distance's default cap
FD_EMUL_SWEEPS = 16              # the emulation converges within this on every case (a condition on the case list)
# measured by fd_measure() over FD_CASES (table per case: DESIGN.md 7); the worst ratio stands beside the constant
FD_WORST_RATIO = 1.1e-5          # 1.089e-05 on "128x128x256 self", rounded up to two digits
FD_TOL = 4 * FD_WORST_RATIO


def _rng(*key):
    return np.random.default_rng(list(key))


# ---- Gram -----------------------------------------------------------------------------------------------------------------------------
GRAM_SHAPES = [(1, 1), (63, 65), (64, 64), (65, 129), (129, 33)]
GRAM_D = [1, 15, 16, 17, 257, 4101]


def gram_inputs(na, nb, d, seed=1):
    r = _rng(11, na, nb, d, seed)
    return r.standard_normal((na, d)).astype(np.float32), (r.standard_normal((nb, d)) * 1.3 + 0.2).astype(np.float32)


def gram_integer_inputs(na, nb, d, seed=2):
    """Entries in -8..8: |partial sums| <= 64 d < 2^24 for d <= 4101, every fp32 step exact."""
    r = _rng(12, na, nb, d, seed)
    return r.integers(-8, 9, (na, d)).astype(np.float32), r.integers(-8, 9, (nb, d)).astype(np.float32)


def gram_ref64(a, b):
    return np.asarray(a, np.float64) @ np.asarray(b, np.float64).T


def gram_bound(a, b):
    d = np.asarray(a).shape[1]
    return (d + 1) * U * (np.abs(np.asarray(a, np.float64)) @ np.abs(np.asarray(b, np.float64)).T)


# ---- feature statistics ---------------------------------------------------------------------------------------------------------------
STATS_N = [2, 3, 64, 65, 1025]
STATS_D = [1, 17, 4101]


def stats_inputs(n, d, kind="plain", seed=3):
    r = _rng(13, n, d, seed)
    x = (r.standard_normal((n, d)) * (0.5 + r.random((1, d))) + r.standard_normal((1, d))).astype(np.float32)
    if kind == "offset":
        x = x + np.float32(1000.0)
    elif kind == "constant column":
        x[:, d // 2] = np.float32(3.25)
    return x


def stats_ref64(x):
    """(mean [D], A = (x - mean) / sqrt(N - 1) [N, D], trace of the unbiased covariance) in float64."""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=0)
    a = (x - mean) / np.sqrt(x.shape[0] - 1.0)
    return mean, a, float((a * a).sum())


def mean_bound(x):
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    return U * np.abs(x.mean(axis=0)) + n * 2.0 ** -53 * np.abs(x).mean(axis=0)


def centred_bound(x):
    """Per entry of A."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    dm = mean_bound(x)[None, :]
    d = np.abs(x - x.mean(axis=0))
    dd = dm + U * (d + dm)
    return (dd + 2.01 * U * (d + dd)) / np.sqrt(n - 1.0)


def trace_bound(x):
    x = np.asarray(x, np.float64)
    _, a, tr = stats_ref64(x)
    da = centred_bound(x)
    return float((2 * np.abs(a) * da + da * da).sum() + x.size * 2.0 ** -53 * tr)


# ---- KID ------------------------------------------------------------------------------------------------------------------------------
KID_M = [2, 63, 64, 65, 130]
KID_SUBSETS = [1, 7]
KID_D = [16, 257, 4101]


def kid_inputs(n_real, n_fake, d, seed=4):
    """Features of order 1 per coordinate, so that g / D is of order 1 and the cube matters; the fake set is shifted."""
    r = _rng(14, n_real, n_fake, d, seed)
    return (np.abs(r.standard_normal((n_real, d))) * 1.2).astype(np.float32), \
        (np.abs(r.standard_normal((n_fake, d)) * 1.1 + 0.3)).astype(np.float32)


def kid_tables(n_real, n_fake, num_subsets, m, seed=5):
    """Subset tables drawn here (not by the code under test): no repeat within a row."""
    r = _rng(15, n_real, n_fake, num_subsets, m, seed)
    ix = np.stack([r.choice(n_real, m, replace=False) for _ in range(num_subsets)]).astype(np.int32)
    iy = np.stack([r.choice(n_fake, m, replace=False) for _ in range(num_subsets)]).astype(np.int32)
    return ix, iy


def kid_ref64(x, y, ix, iy, include_diagonal=False, biased_m=False, no_div=False):
    """(sums [S, 3], kid): for every subset the off-diagonal sum of k(x, x), of k(y, y) and the full sum of k(x, y),
    k(u, v) = (u . v / D + 1)^3, and the mean over the subsets of (Sxx + Syy) / (m (m - 1)) - 2 Sxy / m^2.  Float64, row by row.
    The three switches are the mutations a vacuous bound would let through (tests/test_metric_refs_cpu.py)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    d = x.shape[1]
    div = 1.0 if no_div else float(d)
    s_count, m = ix.shape
    sums = np.zeros((s_count, 3), np.float64)
    total = 0.0
    for s in range(s_count):
        xs, ys = x[ix[s]], y[iy[s]]
        sxx = syy = sxy = 0.0
        for i in range(m):
            kxx = (xs @ xs[i] / div + 1.0) ** 3
            kyy = (ys @ ys[i] / div + 1.0) ** 3
            kxy = (ys @ xs[i] / div + 1.0) ** 3
            sxx += kxx.sum() - (0.0 if include_diagonal else kxx[i])
            syy += kyy.sum() - (0.0 if include_diagonal else kyy[i])
            sxy += kxy.sum()
        sums[s] = sxx, syy, sxy
        off = m * m if biased_m else m * (m - 1)
        total += (sxx + syy) / off - 2.0 * sxy / (m * m)
    return sums, total / s_count


def _poly3_bound(a, b, skip_diag):
    """Sum over the entries of the bound on fl((g' / D + 1)^3) for the rows a, b (float64 views of fp32 data)."""
    d = a.shape[1]
    g = a @ b.T
    dg = (d + 1) * U * (np.abs(a) @ np.abs(b).T)
    v = np.abs(g / d + 1.0)
    dv = (dg / d + U * (np.abs(g) + dg) / d + U * v) / (1.0 - U)
    e = 3.0 * (v + dv) ** 2 * dv + 2.01 * U * (v + dv) ** 3
    k = v ** 3
    if skip_diag:
        np.fill_diagonal(e, 0.0)
        np.fill_diagonal(k, 0.0)
    return float(e.sum() + e.size * 2.0 ** -53 * k.sum())


def kid_bound(x, y, ix, iy):
    """(bounds of the sums [S, 3], bound of the estimate), float64, from the inputs alone."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    s_count, m = ix.shape
    b = np.zeros((s_count, 3), np.float64)
    total = 0.0
    for s in range(s_count):
        xs, ys = x[ix[s]], y[iy[s]]
        b[s] = _poly3_bound(xs, xs, True), _poly3_bound(ys, ys, True), _poly3_bound(xs, ys, False)
        total += (b[s, 0] + b[s, 1]) / (m * (m - 1)) + 2.0 * b[s, 2] / (m * m)
    sums, _ = kid_ref64(x, y, ix, iy)
    scale = (np.abs(sums[:, :2]).sum() / (m * (m - 1)) + 2.0 * np.abs(sums[:, 2]).sum() / (m * m)) / s_count
    return b, total / s_count + 8 * (s_count + 4) * 2.0 ** -53 * scale        # (the float64 combination of 3 S terms)


# ---- Frechet distance -----------------------------------------------------------------------------------------------------------------
def fd_ref64(x, y, return_terms=False):
    """pytorch-fid's calculate_frechet_distance in float64: means, unbiased covariances by np.cov, and tr sqrt(S1 S2) as the
    nuclear norm of A1 A2^T (np.linalg.svd), A = (X - mean) / sqrt(N - 1).  tests/test_metric_refs_cpu.py checks the identity
    against scipy.linalg.sqrtm."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    mu1, mu2 = x.mean(axis=0), y.mean(axis=0)
    c1, c2 = np.atleast_2d(np.cov(x, rowvar=False)), np.atleast_2d(np.cov(y, rowvar=False))
    a1 = (x - mu1) / np.sqrt(x.shape[0] - 1.0)
    a2 = (y - mu2) / np.sqrt(y.shape[0] - 1.0)
    nuclear = float(np.linalg.svd(a1 @ a2.T, compute_uv=False).sum())
    diff = mu1 - mu2
    terms = dict(mean_term=float(diff @ diff), trace_real=float(np.trace(c1)), trace_fake=float(np.trace(c2)), nuclear=nuclear)
    terms["scale"] = terms["mean_term"] + terms["trace_real"] + terms["trace_fake"]          # S of the tolerance
    terms["fd"] = terms["scale"] - 2.0 * nuclear
    return terms if return_terms else terms["fd"]


def jacobi_pairs(npad, rnd):
    """The round-robin schedule of csrc/metric_math.h restated: (I, J) of the npad / 2 slots of round ``rnd``, I < J."""
    q = npad - 1
    k = np.arange(1, npad // 2)
    a = np.concatenate([[q], (rnd + k) % q])
    b = np.concatenate([[rnd], (rnd - k + q) % q])
    return np.minimum(a, b), np.maximum(a, b)


def jacobi_emulated(w, max_sweeps=FD_MAX_SWEEPS):
    """csrc/metrics.hip's sweeps in numpy float32: the same schedule, skip rule (|g| <= 4 eps sqrt(a) sqrt(b), or
    sqrt(a) sqrt(b) <= eps^2 |W|_F^2) and rotation (zeta = (b - a) / (2 g), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) with
    the root read as |zeta| from 2^13 on, c = 1 / sqrt(1 + t^2), s = c t); the pairs of a round are disjoint and run at once.
    The dot products are numpy's float32 sums.  Stops after the first sweep that rotates nothing.
    Returns (W, sweeps run, rotations of the last sweep, nuclear norm = sum of the row norms in float64)."""
    w = np.array(w, np.float32)
    n = w.shape[0]
    npad = n + (n & 1)
    f = np.float32
    sweeps, rotated = 0, -1
    while sweeps < max_sweeps:
        frob2 = f((w.astype(np.float64) ** 2).sum())
        rotated = 0
        for rnd in range(npad - 1):
            i, j = jacobi_pairs(npad, rnd)
            real = j < n
            i, j = i[real], j[real]
            wi, wj = w[i], w[j]
            a = (wi * wi).sum(axis=1, dtype=f)
            b = (wj * wj).sum(axis=1, dtype=f)
            g = (wi * wj).sum(axis=1, dtype=f)
            sab = np.sqrt(a) * np.sqrt(b)
            act = (np.abs(g) > f(4) * EPS32 * sab) & (sab > EPS32 * EPS32 * frob2)
            if not act.any():
                continue
            i, j, wi, wj, a, b, g = i[act], j[act], wi[act], wj[act], a[act], b[act], g[act]
            with np.errstate(over="ignore", divide="ignore"):
                zeta = (b - a) / (f(2) * g)
                az = np.abs(zeta)
                root = np.where(az >= f(8192), az, np.sqrt(az * az + f(1)))
                t = np.copysign(f(1), zeta) / (az + root)
            c = f(1) / np.sqrt(t * t + f(1))
            s = c * t
            w[i] = c[:, None] * wi - s[:, None] * wj
            w[j] = s[:, None] * wi + c[:, None] * wj
            rotated += int(act.sum())
        sweeps += 1
        if rotated == 0:
            break
    nuclear = float(np.sqrt((w.astype(np.float64) ** 2).sum(axis=1)).sum())
    return w, sweeps, rotated, nuclear


def fd_w_emulated(x, y):
    """The matrix the sweeps work on, as the kernels form it up to the Gram's summation order: fp32 means of float64 sums, fp32
    centring and scaling, the product rounded to fp32; the smaller set carries the rows (n = min, L = max)."""
    def centred(v):
        v = np.asarray(v, np.float32)
        mean = v.astype(np.float64).mean(axis=0).astype(np.float32)
        return ((v - mean) / np.sqrt(np.float32(v.shape[0] - 1))).astype(np.float32)
    a1, a2 = centred(x), centred(y)
    p, q = (a1, a2) if a1.shape[0] <= a2.shape[0] else (a2, a1)
    return (p.astype(np.float64) @ q.astype(np.float64).T).astype(np.float32)


def _relu_features(n, d, r, latent=48):
    return np.maximum(r.standard_normal((n, latent)) @ (r.standard_normal((latent, d)) / np.sqrt(latent)) + 0.1, 0.0)


def _fd_iid():
    r = _rng(16, 0)
    return r.standard_normal((64, 96)), r.standard_normal((64, 96))


def _fd_shifted():
    r = _rng(16, 1)
    return r.standard_normal((65, 130)), r.standard_normal((63, 130)) * 1.7 + 0.8


def _fd_relu_33_130():
    r = _rng(16, 2)
    return _relu_features(33, 257, r), _relu_features(130, 257, r) * 1.2


def _fd_relu_130_33():
    x, y = _fd_relu_33_130()
    return y, x


def _fd_two_rows():
    r = _rng(16, 3)
    return r.standard_normal((2, 40)), r.standard_normal((64, 40)) + 0.5


def _fd_rank8():
    r = _rng(16, 4)
    basis = r.standard_normal((8, 70))
    return r.standard_normal((127, 8)) @ basis, (r.standard_normal((129, 8)) * 0.8) @ basis + 0.3


def _fd_self():
    r = _rng(16, 5)
    x = r.standard_normal((128, 256)) * (0.2 + r.random((1, 256)))
    return x, x


def _fd_relu_256():
    r = _rng(16, 6)
    return _relu_features(256, 1024, r, latent=256), _relu_features(256, 1024, r, latent=256) * 0.9 + 0.05


FD_CASES = [("64x64x96 iid", _fd_iid), ("65x63x130 shifted scaled", _fd_shifted), ("33x130x257 relu", _fd_relu_33_130),
            ("130x33x257 relu swapped", _fd_relu_130_33), ("2x64x40", _fd_two_rows), ("127x129x70 rank 8", _fd_rank8),
            ("128x128x256 self", _fd_self), ("256x256x1024 relu", _fd_relu_256)]
FD_NAMES = [name for name, _ in FD_CASES]


@functools.lru_cache(maxsize=None)
def fd_case(name):
    """(x fp32, y fp32, fd_ref64's terms): computed once, shared, not to be modified."""
    x, y = dict(FD_CASES)[name]()
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    return x, y, fd_ref64(x, y, return_terms=True)


@functools.lru_cache(maxsize=None)
def fd_measure(name):
    """(sweeps of the emulation, rotations of its last sweep, |2 (nuclear_emulated - nuclear_64)| / S) of one case."""
    x, y, ref = fd_case(name)
    _, sweeps, rotated, nuclear = jacobi_emulated(fd_w_emulated(x, y))
    return sweeps, rotated, abs(2.0 * (nuclear - ref["nuclear"])) / ref["scale"]


if __name__ == "__main__":             # python -m tests.metric_common: the table of DESIGN.md 7
    for case_name in FD_NAMES:
        print("%-28s sweeps %2d  last %d  ratio %.3e" % ((case_name,) + fd_measure(case_name)))
