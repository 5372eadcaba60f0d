"""GPU: the set-metric kernels (csrc/metrics.hip) through the C ABI on guarded memory -- every input, output and workspace lies
between two regions of pattern bytes that must be intact after every call, and every workspace has exactly the bytes its
``*_workspace`` entry returns.  References, bounds (derived, u = 2^-24) and case lists: tests/metric_common.py, pinned without a GPU
by tests/test_metric_refs_cpu.py.
  Gram STORE     |got - ref64| <= (D + 1) u sum |a b| per entry; equality on integers, under transposition and with index tables
  statistics     means, centred matrix and trace within their bounds; a constant column exactly
  KID            the three sums of every subset and the estimate within the derived bound of kid_ref64 on the same tables
  Frechet chain  |fd - fd_ref64| <= FD_TOL * S with the measured FD_TOL (4 x the CPU emulation's worst), at most 30 sweeps
SRGAN_TEST_LOG=1 prints the worst err / bound and the sweep counts."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import metric_common as mc

pytestmark = pytest.mark.gpu
LOG = bool(os.environ.get("SRGAN_TEST_LOG"))


@pytest.fixture(scope="module")
def L():
    from srgan_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(L, code, what):
    assert code == 0, f"{what}: code {code}: {L.srgan_last_error().decode(errors='replace')}"


def _untouched(t):
    """an output still holds the arena's pattern bytes"""
    return bool((t.contiguous().view(torch.uint8) == 0xA5).all())


# ---- Gram -----------------------------------------------------------------------------------------------------------------------------
def run_gram(L, a, b, ia=None, ib=None, same=False):
    ar = mc.Arena()
    ad = ar.put(a, "a")
    bd = ad if same else ar.put(b, "b")
    iad = None if ia is None else ar.put(np.asarray(ia, np.int32), "idx_a")
    ibd = None if ib is None else ar.put(np.asarray(ib, np.int32), "idx_b")
    na = a.shape[0] if ia is None else len(ia)
    nb = b.shape[0] if ib is None else len(ib)
    out = ar.out((na, nb), "gram")
    _ok(L, L.srgan_gram_f32(_p(ad), a.shape[0], _p(iad), na, _p(bd), b.shape[0], _p(ibd), nb, a.shape[1], _p(out), _st()), "gram_f32")
    torch.cuda.synchronize()
    ar.intact("gram_f32")
    return out.cpu().numpy()


@pytest.mark.parametrize("d", mc.GRAM_D)
@pytest.mark.parametrize("na,nb", mc.GRAM_SHAPES, ids=str)
def test_gram_store_per_entry(L, na, nb, d):
    a, b = mc.gram_inputs(na, nb, d)
    got = run_gram(L, a, b).astype(np.float64)
    ref, bound = mc.gram_ref64(a, b), mc.gram_bound(a, b)
    ratio = float((np.abs(got - ref) / bound).max())
    if LOG:
        print(f"metric gram | {na}x{nb}x{d} | err/bound {ratio:.3f}")
    assert (np.abs(got - ref) <= bound).all(), ratio
    # transposing the arguments gives the exact transpose (the chain a_k b_k, k ascending, does not know which factor is which)
    assert np.array_equal(run_gram(L, b, a), got.T.astype(np.float32))


@pytest.mark.parametrize("na,nb,d", [(65, 129, 17), (63, 65, 4101), (1, 1, 1), (129, 33, 16)], ids=str)
def test_gram_store_exact_on_integers(L, na, nb, d):
    a, b = mc.gram_integer_inputs(na, nb, d)
    got = run_gram(L, a, b)
    assert np.array_equal(got.astype(np.float64), mc.gram_ref64(a, b))
    # an asymmetric probe: A = identity rows picks out B's columns, so a swapped row / column map cannot pass
    eye = np.eye(64, d, dtype=np.float32)
    assert np.array_equal(run_gram(L, eye, b), b[:, :64].T.copy() if d >= 64 else np.pad(b.T, ((0, 64 - d), (0, 0))))


@pytest.mark.parametrize("d", [17, 4101])
def test_gram_store_with_index_tables(L, d):
    a, b = mc.gram_inputs(70, 40, d)
    r = np.random.default_rng([31, d])
    ia = np.concatenate([np.arange(69, -1, -1), r.integers(0, 70, 60), [5, 5, 5]]).astype(np.int32)       # reversed, repeated: 133 rows
    ib = np.concatenate([r.integers(0, 40, 64), [39, 0, 39]]).astype(np.int32)                             # 67 rows
    got = run_gram(L, a, b, ia, ib)
    assert got.shape == (133, 67)
    assert np.array_equal(got, run_gram(L, a[ia], b[ib]))
    assert np.array_equal(run_gram(L, a, b, ia, None), run_gram(L, a[ia], b))
    # an index outside the matrix reads as a row of zeros, never as memory
    bad = ia.copy()
    bad[[0, 70, 132]] = [-1, 70, 2 ** 31 - 1]
    wild = run_gram(L, a, b, bad, ib)
    keep = np.ones(133, bool)
    keep[[0, 70, 132]] = False
    assert np.array_equal(wild[keep], got[keep]) and not wild[~keep].any()


def test_gram_bad_arguments_write_nothing(L):
    ar = mc.Arena()
    a = ar.put(np.ones((4, 3), np.float32), "a")
    out = ar.out((4, 4), "gram")
    assert L.srgan_gram_f32(_p(a), 4, None, 4, _p(a), 4, None, 4, 0, _p(out), _st()) == -1 and b"D = 0" in L.srgan_last_error()
    assert L.srgan_gram_f32(_p(a), 4, None, 5, _p(a), 4, None, 4, 3, _p(out), _st()) == -1
    assert L.srgan_gram_f32(None, 4, None, 4, _p(a), 4, None, 4, 3, _p(out), _st()) == -1
    torch.cuda.synchronize()
    ar.intact("gram_f32 errors")
    assert _untouched(out)


# ---- statistics -----------------------------------------------------------------------------------------------------------------------
def run_stats(L, x, short=0):
    ar = mc.Arena()
    n, d = x.shape
    xd = ar.put(x, "x")
    mean, a = ar.out((d,), "mean"), ar.out((n, d), "centred")
    trace = ar.out((1,), "trace", dtype=torch.float64)
    nb = L.srgan_feature_stats_workspace(n, d)
    ws = ar.raw(max(nb - short, 1), "workspace")
    code = L.srgan_feature_stats(_p(xd), n, d, _p(mean), _p(a), _p(trace), _p(ws), nb - short, _st())
    torch.cuda.synchronize()
    ar.intact("feature_stats")
    return code, mean, a, trace


def hold_stats(L, x, what):
    code, mean, a, trace = run_stats(L, x)
    _ok(L, code, "feature_stats")
    mean, a, trace = mean.cpu().numpy().astype(np.float64), a.cpu().numpy().astype(np.float64), float(trace.item())
    rm, ra, rt = mc.stats_ref64(x)
    bm, ba, bt = mc.mean_bound(x), mc.centred_bound(x), mc.trace_bound(x)
    if LOG:
        print(f"metric stats | {what} | mean {np.max(np.abs(mean - rm) / bm):.3f} centred {np.max(np.abs(a - ra) / ba):.3f} "
              f"trace {abs(trace - rt) / bt:.3f} (err / bound)")
    assert (np.abs(mean - rm) <= bm).all(), what
    assert (np.abs(a - ra) <= ba).all(), what
    assert abs(trace - rt) <= bt, (what, trace, rt, bt)
    return mean, a, trace


@pytest.mark.parametrize("d", mc.STATS_D)
@pytest.mark.parametrize("n", mc.STATS_N)
def test_feature_stats(L, n, d):
    hold_stats(L, mc.stats_inputs(n, d), f"{n}x{d}")


def test_feature_stats_above_the_row_block_cap(L):
    """4100 rows: more than 64 blocks of 64 rows, so the column sums run as 64 blocks of 65 rows (the last one short)"""
    hold_stats(L, mc.stats_inputs(4100, 3), "4100x3")


def test_feature_stats_at_an_offset_and_on_a_constant_column(L):
    hold_stats(L, mc.stats_inputs(65, 17, "offset"), "offset +1000")
    hold_stats(L, mc.stats_inputs(1025, 17, "offset"), "offset +1000, 1025 rows")
    x = mc.stats_inputs(65, 17, "constant column")
    mean, a, _ = hold_stats(L, x, "constant column")
    assert mean[8] == 3.25 and not a[:, 8].any()


def test_feature_stats_bad_arguments_write_nothing(L):
    x = mc.stats_inputs(64, 17)
    code, mean, a, trace = run_stats(L, x, short=1)
    assert code == -1 and b"workspace too small" in L.srgan_last_error()
    assert _untouched(mean) and _untouched(a) and _untouched(trace)
    ar = mc.Arena()
    xd, out, tr = ar.put(x, "x"), ar.out((64, 17), "out"), ar.out((1,), "trace", dtype=torch.float64)
    ws = ar.raw(1 << 16, "workspace")
    assert L.srgan_feature_stats(_p(xd), 1, 17, _p(out), _p(out), _p(tr), _p(ws), 1 << 16, _st()) == -1 and b"N = 1" in L.srgan_last_error()
    assert L.srgan_feature_stats(_p(xd), 64, 0, _p(out), _p(out), _p(tr), _p(ws), 1 << 16, _st()) == -1 and b"D = 0" in L.srgan_last_error()
    assert L.srgan_feature_stats_workspace(1, 17) == 0 and L.srgan_feature_stats_workspace(64, 0) == 0
    torch.cuda.synchronize()
    ar.intact("feature_stats errors")
    assert _untouched(out) and _untouched(tr) and _untouched(ws)


# ---- KID ------------------------------------------------------------------------------------------------------------------------------
def run_kid(L, x, y, ix, iy, short=0, same=False, m=None, n_real=None, n_fake=None, d=None):
    ar = mc.Arena()
    xd = ar.put(x, "x")
    yd = xd if same else ar.put(y, "y")
    ixd = ar.put(ix, "idx_x")
    iyd = ixd if same else ar.put(iy, "idx_y")
    s, mm = ix.shape
    m = mm if m is None else m
    sums = ar.out((s, 3), "sums", dtype=torch.float64)
    kid = ar.out((1,), "kid", dtype=torch.float64)
    nb = L.srgan_kid_workspace(s, mm)
    ws = ar.raw(max(nb - short, 1), "workspace")
    code = L.srgan_kid_poly3(_p(xd), x.shape[0] if n_real is None else n_real, _p(yd), y.shape[0] if n_fake is None else n_fake,
                             x.shape[1] if d is None else d, _p(ixd), _p(iyd), s, m, _p(sums), _p(kid), _p(ws), nb - short, _st())
    torch.cuda.synchronize()
    ar.intact("kid_poly3")
    return code, sums, kid


@pytest.mark.parametrize("d", mc.KID_D)
@pytest.mark.parametrize("subsets", mc.KID_SUBSETS)
@pytest.mark.parametrize("m", mc.KID_M)
def test_kid_sums_and_estimate(L, m, subsets, d):
    n_real, n_fake = m + 7, m + 2                                    # sets of different sizes, both larger than the subsets
    x, y = mc.kid_inputs(n_real, n_fake, d)
    ix, iy = mc.kid_tables(n_real, n_fake, subsets, m)
    code, sums, kid = run_kid(L, x, y, ix, iy)
    _ok(L, code, "kid_poly3")
    sums, kid = sums.cpu().numpy(), float(kid.item())
    rs, rk = mc.kid_ref64(x, y, ix, iy)
    bs, bk = mc.kid_bound(x, y, ix, iy)
    if LOG:
        print(f"metric kid | m {m} S {subsets} D {d} | sums {np.max(np.abs(sums - rs) / bs):.3f} kid {abs(kid - rk) / bk:.3f} (err / bound)")
    assert (np.abs(sums - rs) <= bs).all(), (sums, rs, bs)
    assert abs(kid - rk) <= bk, (kid, rk, bk)


def test_kid_of_a_set_with_itself_is_symmetric_bit_for_bit(L):
    x, _ = mc.kid_inputs(140, 140, 257)
    ix, _ = mc.kid_tables(140, 140, 7, 130)
    code, sums, kid = run_kid(L, x, x, ix, ix, same=True)
    _ok(L, code, "kid_poly3")
    sums = sums.cpu().numpy()
    assert np.array_equal(sums[:, 0], sums[:, 1])
    rs, rk = mc.kid_ref64(x, x, ix, ix)
    bs, bk = mc.kid_bound(x, x, ix, ix)
    assert (np.abs(sums - rs) <= bs).all() and abs(float(kid.item()) - rk) <= bk


def test_kid_bad_arguments_write_nothing(L):
    x, y = mc.kid_inputs(70, 66, 16)
    ix, iy = mc.kid_tables(70, 66, 2, 65)
    for kw, msg in ((dict(short=1), b"workspace too small"), (dict(m=1), b"m = 1"), (dict(n_fake=64), b"exceeds a set"),
                    (dict(n_real=64), b"exceeds a set"), (dict(d=0), b"D = 0")):
        code, sums, kid = run_kid(L, x, y, ix, iy, **kw)
        assert code == -1 and msg in L.srgan_last_error(), (kw, L.srgan_last_error())
        assert _untouched(sums) and _untouched(kid), kw
    assert L.srgan_kid_workspace(2, 1) == 0 and L.srgan_kid_workspace(0, 65) == 0
    assert L.srgan_kid_workspace(2, 65) == 3 * 2 * 4 * 8


# ---- Jacobi, nuclear norm and the whole Frechet chain -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fd_chain(name):
    """The chain compute_frechet_distance runs, entry by entry on guarded memory: statistics of both sets, the Gram STORE into W
    (the smaller set on the rows), sweeps until one rotates nothing (at most FD_MAX_SWEEPS), the nuclear norm.
    -> dict(fd, mean_term, trace_real, trace_fake, nuclear, sweeps, last, w_shape).  Computed once per case."""
    from srgan_amd import _lib
    L = _lib.load()
    x, y, _ = mc.fd_case(name)
    ar = mc.Arena()
    d = x.shape[1]
    stats = []
    for v, tag in ((x, "real"), (y, "fake")):
        n = v.shape[0]
        vd = ar.put(v, tag)
        mean, a = ar.out((d,), tag + " mean"), ar.out((n, d), tag + " centred")
        trace = ar.out((1,), tag + " trace", dtype=torch.float64)
        nb = L.srgan_feature_stats_workspace(n, d)
        ws = ar.raw(nb, tag + " stats workspace")
        _ok(L, L.srgan_feature_stats(_p(vd), n, d, _p(mean), _p(a), _p(trace), _p(ws), nb, _st()), "feature_stats")
        stats.append((mean, a, trace))
    torch.cuda.synchronize()
    ar.intact("feature_stats")
    (m1, a1, t1), (m2, a2, t2) = stats
    p, q = (a1, a2) if a1.shape[0] <= a2.shape[0] else (a2, a1)
    n, length = p.shape[0], q.shape[0]
    w = ar.out((n, length), "W")
    _ok(L, L.srgan_gram_f32(_p(p), n, None, n, _p(q), length, None, length, d, _p(w), _st()), "gram_f32")
    nb = L.srgan_jacobi_workspace(n)
    ws = ar.raw(nb, "jacobi workspace")
    count = ar.out((1,), "rotations", dtype=torch.int32)
    sweeps, last = 0, -1
    while sweeps < mc.FD_MAX_SWEEPS:
        _ok(L, L.srgan_jacobi_sweep(_p(w), n, length, _p(count), _p(ws), nb, _st()), "jacobi_sweep")
        torch.cuda.synchronize()
        ar.intact(f"jacobi_sweep {sweeps}")
        sweeps += 1
        last = int(count.item())
        if last == 0:
            break
    nuc = ar.out((1,), "nuclear", dtype=torch.float64)
    _ok(L, L.srgan_nuclear_from_rows(_p(w), n, length, _p(nuc), _p(ws), nb, _st()), "nuclear_from_rows")
    torch.cuda.synchronize()
    ar.intact("nuclear_from_rows")
    diff = m1.cpu().numpy().astype(np.float64) - m2.cpu().numpy().astype(np.float64)
    out = dict(mean_term=float(diff @ diff), trace_real=float(t1.item()), trace_fake=float(t2.item()), nuclear=float(nuc.item()),
               sweeps=sweeps, last=last, w_shape=(n, length))
    out["fd"] = out["mean_term"] + out["trace_real"] + out["trace_fake"] - 2.0 * out["nuclear"]
    # the rows are orthogonal now: the nuclear norm is the sum of their norms
    rows = w.cpu().numpy().astype(np.float64)
    out["row_norm_sum"] = float(np.sqrt((rows * rows).sum(axis=1)).sum())
    return out


@pytest.mark.parametrize("name", mc.FD_NAMES)
def test_frechet_chain(L, name):
    x, y, ref = mc.fd_case(name)
    got = fd_chain(name)
    tol = mc.FD_TOL * ref["scale"]
    print(f"metric fd | {name} | sweeps {got['sweeps']} | fd {got['fd']:.9g} ref {ref['fd']:.9g} | err / tol {abs(got['fd'] - ref['fd']) / tol:.3f}")
    assert got["w_shape"] == (min(x.shape[0], y.shape[0]), max(x.shape[0], y.shape[0]))
    assert got["sweeps"] <= mc.FD_MAX_SWEEPS and got["last"] == 0, (got["sweeps"], got["last"])
    assert abs(got["fd"] - ref["fd"]) <= tol, (got, ref)
    assert abs(got["nuclear"] - got["row_norm_sum"]) <= 1e-12 * got["row_norm_sum"]
    if x is y or np.array_equal(x, y):
        assert abs(got["fd"]) <= tol, got["fd"]


def test_frechet_chain_swapped_sets_give_the_same_nuclear_norm(L):
    a, b = fd_chain("33x130x257 relu"), fd_chain("130x33x257 relu swapped")
    _, _, ref = mc.fd_case("33x130x257 relu")
    assert a["w_shape"] == b["w_shape"] == (33, 130)
    assert abs(2.0 * (a["nuclear"] - b["nuclear"])) <= mc.FD_TOL * ref["scale"]
    assert abs(a["fd"] - b["fd"]) <= mc.FD_TOL * ref["scale"]
    assert a["trace_real"] == b["trace_fake"] and a["trace_fake"] == b["trace_real"]


def test_nuclear_from_rows_and_a_sweep_over_orthogonal_rows(L):
    """rows that are orthogonal already (disjoint supports), an odd count: the sweep rotates nothing and changes nothing, the
    nuclear norm is the sum of the row norms; a zero row is left alone (the zero-direction rule)"""
    r = np.random.default_rng([33])
    w = np.zeros((7, 300), np.float32)
    for i in range(6):                                         # row 6 stays zero
        w[i, i * 50:(i + 1) * 50] = r.standard_normal(50).astype(np.float32) * 10.0 ** (i - 3)
    ar = mc.Arena()
    wd = ar.put(w, "W")
    nb = L.srgan_jacobi_workspace(7)
    assert nb == 16 + 7 * 8 + 4 * 4
    ws = ar.raw(nb, "jacobi workspace")
    count = ar.out((1,), "rotations", dtype=torch.int32)
    nuc = ar.out((1,), "nuclear", dtype=torch.float64)
    _ok(L, L.srgan_jacobi_sweep(_p(wd), 7, 300, _p(count), _p(ws), nb, _st()), "jacobi_sweep")
    _ok(L, L.srgan_nuclear_from_rows(_p(wd), 7, 300, _p(nuc), _p(ws), nb, _st()), "nuclear_from_rows")
    torch.cuda.synchronize()
    ar.intact("jacobi_sweep / nuclear_from_rows")
    assert int(count.item()) == 0 and np.array_equal(wd.cpu().numpy(), w)
    want = np.sqrt((w.astype(np.float64) ** 2).sum(axis=1)).sum()
    assert abs(float(nuc.item()) - want) <= 1e-13 * want


def test_jacobi_rotates_one_pair_as_the_formula_says(L):
    """n = 2: one round, one pair; the rotated rows are orthogonal and keep the Frobenius norm, the count is 1, then 0"""
    r = np.random.default_rng([34])
    w = r.standard_normal((2, 1000)).astype(np.float32)
    w[1] += 0.5 * w[0]
    ar = mc.Arena()
    wd = ar.put(w, "W")
    nb = L.srgan_jacobi_workspace(2)
    ws = ar.raw(nb, "jacobi workspace")
    count = ar.out((1,), "rotations", dtype=torch.int32)
    counts = []
    for _ in range(3):
        _ok(L, L.srgan_jacobi_sweep(_p(wd), 2, 1000, _p(count), _p(ws), nb, _st()), "jacobi_sweep")
        torch.cuda.synchronize()
        ar.intact("jacobi_sweep")
        counts.append(int(count.item()))
    got = wd.cpu().numpy().astype(np.float64)
    assert counts[0] == 1 and counts[-1] == 0, counts
    na, nb2 = np.linalg.norm(got[0]), np.linalg.norm(got[1])
    # the last sweep saw |g| <= 4 eps |w0| |w1| on its fp32 dot product, itself within (4 per-thread terms + 6 shuffle steps +
    # 3 wave sums + 1) u sum |x y| <= 7 eps |w0| |w1| of the true one
    assert abs(got[0] @ got[1]) <= 12 * 2.0 ** -23 * na * nb2
    sv = np.linalg.svd(w.astype(np.float64), compute_uv=False)
    assert np.allclose(sorted([na, nb2]), sorted(sv), rtol=1e-5, atol=0)


def test_jacobi_bad_arguments_write_nothing(L):
    w = np.ones((5, 40), np.float32)
    ar = mc.Arena()
    wd = ar.put(w, "W")
    nb = L.srgan_jacobi_workspace(5)
    ws = ar.raw(nb, "jacobi workspace")
    count = ar.out((1,), "rotations", dtype=torch.int32)
    nuc = ar.out((1,), "nuclear", dtype=torch.float64)
    assert L.srgan_jacobi_sweep(_p(wd), 5, 40, _p(count), _p(ws), nb - 1, _st()) == -1 and b"workspace too small" in L.srgan_last_error()
    assert L.srgan_jacobi_sweep(_p(wd), 1, 40, _p(count), _p(ws), nb, _st()) == -1 and b"n = 1" in L.srgan_last_error()
    assert L.srgan_jacobi_sweep(_p(wd), 5, 0, _p(count), _p(ws), nb, _st()) == -1
    assert L.srgan_nuclear_from_rows(_p(wd), 5, 40, _p(nuc), _p(ws), nb - 1, _st()) == -1
    assert L.srgan_nuclear_from_rows(_p(wd), 0, 40, _p(nuc), _p(ws), nb, _st()) == -1
    assert L.srgan_jacobi_workspace(0) == 0
    torch.cuda.synchronize()
    ar.intact("jacobi errors")
    assert _untouched(count) and _untouched(nuc) and _untouched(ws) and np.array_equal(wd.cpu().numpy(), w)
