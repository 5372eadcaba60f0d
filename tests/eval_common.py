"""Yardsticks of the evaluation-kernel tests (csrc/evaluation.hip): float64 references, a numpy emulation of the distance
kernel's float32 order, seeded case lists and the guarded device memory of the C-ABI tests.  tests/test_eval_refs_cpu.py pins
what is in here without a GPU, tests/test_eval_kernels_gpu.py holds the HIP kernels to it.

Pairwise distances.  Bound per element: |got - ref64| <= DIST_ULPS * 2^-24 * ref64, got == 0 where ref64 == 0.  DIST_ULPS = 12
is derived from the kernel's operations, with u = 2^-24, as relative error on the sum of squares:
  2u   the rounded subtraction x - y, squared (every term (d (1 + e))^2, |e| <= u)
  16u  the 16-term fma chain of one chunk (n u for a chain of n non-negative terms)
  2u   the compensated (Kahan) sum of the chunk sums (2u + O(n u^2))
20u in all; the square root halves it and sqrtf adds its own rounding, bounded here by 2u: 12u.  No measured number enters.
``dist_emulated`` repeats the kernel's order (fp32 subtract, fma per chunk of 16, Kahan over the chunks, sqrt); its
``compensated=False`` form adds the chunk sums plainly, which the sensitivity case must show to break the bound.

k-th smallest, PRDC statistics, max pool: exact references (np.sort, the four formulas of prdc 0.2 in float64, torch's
max_pool2d), held to equality.
"""
import functools

import numpy as np
import torch

from oracle import evaluation as oe

U = 2.0 ** -24
DIST_ULPS = 12
PD_K = 16                  # features per chunk of pairwise_dist_kernel
KTH_MAX = 16               # register slots per lane of kth_smallest_rows_kernel
WAVE = 64
GUARD, PATTERN = 4096, 0xA5


# ---- guarded device memory ------------------------------------------------------------------------------------------------------------
class Arena:
    """The device memory of one scenario: every buffer has ``guard`` pattern bytes in front of it and behind it."""

    def __init__(self):
        self.bufs = []

    def raw(self, nbytes, what, guard=GUARD, skew=0):
        """``skew``: the payload starts that many bytes past the 4 KiB boundary (a pointer that is not 16-byte aligned)."""
        guard = -(-guard // GUARD) * GUARD
        buf = torch.full((guard + skew + nbytes + guard,), PATTERN, dtype=torch.uint8, device="cuda")
        self.bufs.append((buf, guard + skew, nbytes, what))
        return buf[guard + skew:guard + skew + nbytes]

    def out(self, shape, what, dtype=torch.float32, guard=GUARD):
        """An output; its bytes start as the pattern (0xA5A5A5A5 is no value a test expects)."""
        numel = int(np.prod(shape, dtype=np.int64))
        return self.raw(numel * torch.empty((), dtype=dtype).element_size(), what, guard).view(dtype).view(tuple(shape))

    def put(self, a, what, guard=GUARD, skew=0):
        """An input: the host array's values, dense."""
        t = torch.as_tensor(np.ascontiguousarray(a)) if not torch.is_tensor(a) else a.detach().contiguous()
        d = self.raw(t.numel() * t.element_size(), what, guard, skew)
        d.copy_(t.reshape(-1).view(torch.uint8))
        return d if skew else d.view(t.dtype).view(t.shape)        # a skewed payload stays a byte view: only its address is used

    def intact(self, when):
        for buf, lead, nbytes, what in self.bufs:
            ok = bool((buf[:lead] == PATTERN).all()) and bool((buf[lead + nbytes:] == PATTERN).all())
            assert ok, f"{when}: bytes written outside the {nbytes} bytes of {what}"


# ---- pairwise distances ---------------------------------------------------------------------------------------------------------------
def dist_ref64(x, y):
    """sqrt(sum (x - y)^2) of the float32 inputs in float64, row by row (no |x|^2 + |y|^2 - 2xy)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = np.empty((x.shape[0], y.shape[0]), np.float64)
    for i in range(x.shape[0]):
        out[i] = np.sqrt(((x[i][None, :] - y) ** 2).sum(axis=1))
    return out


def dist_emulated(x, y, compensated=True):
    """pairwise_dist_kernel's order in float32 on the CPU: d = x - y rounded, part = fma(d, d, part) over the 16 features of a
    chunk (features past D read as 0), the chunk sums added with Kahan compensation (``compensated=False``: plainly), sqrt.
    The fma is d * d + part in float64 (the product of two float32 is exact there) rounded once more to float32."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    (n, d), m = x.shape, y.shape[0]
    chunks = -(-d // PD_K)
    xp = np.zeros((n, chunks * PD_K), np.float32)
    yp = np.zeros((m, chunks * PD_K), np.float32)
    xp[:, :d], yp[:, :d] = x, y
    xp, yp = xp.reshape(n, chunks, PD_K), yp.reshape(m, chunks, PD_K)
    acc, comp = np.zeros((n, m), np.float32), np.zeros((n, m), np.float32)
    step = max(1, (1 << 22) // (n * m))                      # chunks per slab of the [n, m, chunks] working set
    for c0 in range(0, chunks, step):
        xs, ys = xp[:, c0:c0 + step], yp[:, c0:c0 + step]
        part = np.zeros((n, m, xs.shape[1]), np.float32)
        for k in range(PD_K):
            diff = (xs[:, None, :, k] - ys[None, :, :, k]).astype(np.float64)       # float32 subtraction, then widened
            part = (diff * diff + part).astype(np.float32)
        for c in range(part.shape[2]):
            if compensated:
                yk = part[:, :, c] - comp
                t = acc + yk
                comp = (t - acc) - yk
                acc = t
            else:
                acc = acc + part[:, :, c]
    return np.sqrt(acc)


def dist_violations(got, ref64):
    """(number of elements beyond the bound, worst err / bound over the elements with ref64 > 0)."""
    got = np.asarray(got, np.float64)
    zero = ref64 == 0
    bad = int((got[zero] != 0).sum())
    ratio = 0.0
    if (~zero).any():
        r = np.abs(got[~zero] - ref64[~zero]) / (DIST_ULPS * U * ref64[~zero])
        bad += int((~(r <= 1.0)).sum())                      # a NaN counts
        ratio = float(np.nanmax(r)) if np.isfinite(r).any() else float("inf")
    return bad, ratio


def _rng(*key):
    return np.random.default_rng(list(key))


def _cloud(n, m, d, seed):
    r = _rng(seed, n, m, d)
    return r.standard_normal((n, d)).astype(np.float32), (r.standard_normal((m, d)) * 1.1 + 0.15).astype(np.float32)


def _shape_case(n, m, d):
    return dict(name=f"shape {n}x{m}x{d}", make=lambda: _cloud(n, m, d, 1))


def _offset_case():
    def make():
        x, y = _cloud(65, 63, 17, 2)
        return x + np.float32(1000.0), y + np.float32(1000.0)
    return dict(name="offset +1000", make=make)


def _near_case(d):
    def make():
        r = _rng(3, d)
        x = r.standard_normal((65, d)).astype(np.float32)
        y = (x[:63].astype(np.float64) + 1e-4 / np.sqrt(d) * r.standard_normal((63, d))).astype(np.float32)
        return x, y                                        # y[j] lies about 1e-4 from x[j], coordinates of order 1
    return dict(name=f"neighbours 1e-4 apart, D = {d}", make=make)


# N, M in {1, 63, 64, 65, 129} crossed raggedly (every value on both sides, every pair of tile counts), D over its values
DIST_SHAPES = [(1, 1, 1), (1, 129, 3), (129, 1, 15), (63, 64, 16), (64, 65, 17), (65, 63, 4101), (129, 129, 17), (64, 64, 16),
               (63, 129, 1), (65, 1, 3), (1, 63, 15), (129, 65, 16), (64, 63, 4101), (65, 65, 15)]
DIST_CASES = [_shape_case(*s) for s in DIST_SHAPES] + [_offset_case(), _near_case(17), _near_case(4101)]

# (x, y, exact distances): integer coordinates whose squared distances are perfect squares -- every fp32 step is exact
_TRIPLES = [(3, 4, 5), (5, 12, 13), (8, 15, 17), (7, 24, 25), (20, 21, 29), (9, 40, 41)]
_QUADS = [(1, 2, 2, 3), (2, 3, 6, 7), (1, 4, 8, 9), (4, 4, 7, 9), (2, 6, 9, 11), (6, 6, 7, 11)]


def exact_case(d=19):
    """x: 5 integer base points; y: each base point plus a Pythagorean offset spread over the feature axis (so that the
    non-zero terms fall into different chunks).  Returns (x, y, dist) with dist exact integers where known, else -1."""
    r = _rng(4, d)
    x = r.integers(-50, 50, (5, d)).astype(np.float32)
    ys, want = [], []
    for legs in _TRIPLES + _QUADS:
        for i in range(x.shape[0]):
            off = np.zeros(d, np.float32)
            pos = r.choice(d, len(legs) - 1, replace=False)
            off[pos] = np.asarray(legs[:-1], np.float32) * r.choice([-1.0, 1.0], len(legs) - 1)
            ys.append(x[i] + off)
            want.append((i, legs[-1]))
    y = np.stack(ys)
    dist = np.full((x.shape[0], y.shape[0]), -1.0)
    for j, (i, v) in enumerate(want):
        dist[i, j] = v
    return x, y, dist


SENS_N, SENS_D = 8, 1 << 20


@functools.lru_cache(maxsize=None)
def sensitivity_case():
    """N = M = 8 at D = 2^20 (65536 chunk sums): the plain float32 sum of the chunk sums drifts past the bound, the compensated
    one does not (tests/test_eval_refs_cpu.py asserts both halves on the emulation)."""
    x, y = _cloud(SENS_N, SENS_N, SENS_D, 5)
    return x, y, dist_ref64(x, y)


# ---- k-th smallest --------------------------------------------------------------------------------------------------------------------
KTH_M = (1, 16, 17, 63, 64, 65, 1025)


def lane_row(m, c, r):
    """The min(16, columns of lane c) smallest values all in the columns j = c mod 64, in descending column order so that every
    insertion shifts the lane's whole list; everything else far above.  None where lane c has no column."""
    cols = np.arange(c, m, WAVE)[:KTH_MAX]
    if len(cols) == 0:
        return None
    row = (100.0 + r.random(m) * 10).astype(np.float32)
    row[cols] = np.arange(len(cols), 0, -1, dtype=np.float32)
    return row


def kth_rows(m):
    """[(name, float32 row of length m)]"""
    r = _rng(6, m)
    rows = [("ascending", np.arange(m, dtype=np.float32)), ("descending", np.arange(m, 0, -1).astype(np.float32)),
            ("all equal", np.full(m, 7.0, np.float32)), ("three values", r.choice(np.asarray([1.0, 2.0, 3.0], np.float32), m)),
            ("random", r.standard_normal(m).astype(np.float32))]
    for c in (0, 63):
        row = lane_row(m, c, r)
        if row is not None:
            rows.append((f"lane {c}", row))
    some = r.standard_normal(m).astype(np.float32)
    some[::3] = np.inf
    rows.append(("every third +inf", some))
    one = np.full(m, np.inf, np.float32)
    one[m // 2] = -2.5
    rows.append(("one finite", one))
    return rows


def kth_ref(rows, k):
    return np.sort(np.asarray(rows), axis=-1)[..., k - 1]


# ---- PRDC from a given matrix ---------------------------------------------------------------------------------------------------------
PRDC_SHAPES = [(1, 1), (1, 300), (300, 1), (257, 300), (64, 64)]


def prdc_formulas(d, r_real, r_fake, k, less=np.less):
    """The four formulas of prdc 0.2 in float64 -> float32 (``less``: the comparison; np.less_equal is what a wrong kernel does)."""
    d, r_real, r_fake = np.asarray(d, np.float64), np.asarray(r_real, np.float64), np.asarray(r_fake, np.float64)
    inside = less(d, r_real[:, None])
    precision = inside.any(axis=0).mean()
    recall = less(d, r_fake[None, :]).any(axis=1).mean()
    density = (1.0 / float(k)) * inside.sum(axis=0).mean()
    coverage = less(d.min(axis=1), r_real).mean()
    return np.asarray([precision, recall, density, coverage], np.float64).astype(np.float32)


def prdc_matrix_cases(n, m):
    """[(name, dist [n, m], r_real [n], r_fake [m], k)]: small-integer distances, integer and half-integer radii."""
    r = _rng(7, n, m)
    f = np.float32
    ones_n, ones_m = np.ones(n, f), np.ones(m, f)
    mixed = r.integers(1, 5, (n, m)).astype(f)
    cases = [("all inside", mixed, 5 * ones_n, 5 * ones_m, 1),
             ("none inside", mixed, 0.5 * ones_n, 0.5 * ones_m, 5),
             ("ties only", np.full((n, m), 2.0, f), 2 * ones_n, 2 * ones_m, 2),
             # about a quarter of the comparisons are ties d == r, the others fall on both sides
             ("mixed", mixed, r.integers(2, 9, n).astype(f) / 2, r.integers(2, 9, m).astype(f) / 2, 3),
             # sparse: one row in ten and one column in ten can count at all, the ends of both axes among them
             ("sparse", mixed, np.where(np.arange(n) % 10 == (n - 1) % 10, 2.5, 1.0).astype(f),
              np.where(np.arange(m) % 10 == (m - 1) % 10, 1.5, 0.5).astype(f), 4)]
    # one element inside, at the corners and on both sides of the 256-column / 256-row block borders
    for i, j in sorted({(0, 0), (n - 1, m - 1), (n - 1, min(256, m - 1)), (min(256, n - 1), 0), (0, min(255, m - 1))}):
        d = np.full((n, m), 9.0, f)
        d[i, j] = 1.0
        cases.append((f"single ({i}, {j})", d, 2 * ones_n, 1.5 * ones_m, 1))
    return cases


# ---- compute_prdc end to end ----------------------------------------------------------------------------------------------------------
MARGIN_ULPS = 2 * DIST_ULPS            # a distance and a radius each carry DIST_ULPS
# (n, m, d, k, seed): the seeds are chosen so that in float64 no comparison is closer than the margin (the CPU test asserts it)
E2E_CASES = [(128, 100, 4096, 5, 0), (65, 300, 64, 3, 0), (300, 257, 16, 5, 0), (17, 16, 4096, 15, 0)]


def e2e_features(n, m, d, k, seed):
    """Two overlapping clouds whose samples differ in scale, so that the distances do not concentrate at high d."""
    r = _rng(8, n, m, d, k, seed)
    real = r.standard_normal((n, d)) * np.exp(0.4 * r.standard_normal((n, 1)))
    fake = (r.standard_normal((m, d)) * 1.1 + 0.15) * np.exp(0.4 * r.standard_normal((m, 1)))
    return real.astype(np.float32), fake.astype(np.float32)


@functools.lru_cache(maxsize=None)
def e2e_reference(case):
    """(real, fake, the oracle's four numbers, the smallest |d - r| / max(d, r) over every comparison the algorithm makes)."""
    n, m, d, k, seed = case
    real, fake = e2e_features(*case)
    dist = dist_ref64(real, fake)
    r_real = oe.kth_value(dist_ref64(real, real), k + 1)
    r_fake = oe.kth_value(dist_ref64(fake, fake), k + 1)
    gap_r = np.abs(dist - r_real[:, None]) / np.maximum(dist, r_real[:, None])
    gap_f = np.abs(dist - r_fake[None, :]) / np.maximum(dist, r_fake[None, :])
    want = prdc_formulas(dist, r_real, r_fake, k)
    return real, fake, want, float(min(gap_r.min(), gap_f.min()))


# ---- max pool -------------------------------------------------------------------------------------------------------------------------
POOL_GRID_CAP = 16384 * 256           # items (four channels of one output pixel) one pass of the capped grid covers
POOL_BIG = (1, 4, 4098, 4098)         # 2049 * 2049 = 4198401 items > POOL_GRID_CAP: the grid-stride loop runs; 268 MB of input
POOL_SHAPES = [(2, 8, 6, 10), (1, 4, 7, 9), (3, 12, 5, 5), (1, 4, 2, 2), (2, 64, 15, 13)]


def pool_input(shape, kind, seed=9):
    """NHWC float32 tensor [n, h, w, c]."""
    n, c, h, w = shape
    x = torch.randn(n, h, w, c, generator=torch.Generator().manual_seed(seed + sum(shape)))
    if kind == "negative":
        x = -x.abs() - 0.5
    elif kind == "-inf":
        x[:, ::2, ::3, :] = float("-inf")
        x[:, :2, :2, 0] = float("-inf")            # one window of nothing but -inf
    elif kind == "+inf":
        x[:, 1::2, ::2, :] = float("inf")
    return x


def pool_ref(x_nhwc):
    return torch.nn.functional.max_pool2d(x_nhwc.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()


def same_with_nan(a, b):
    """Equality that wants a NaN exactly where the other has one."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a),
                                                                      torch.where(nb, torch.zeros_like(b), b))
