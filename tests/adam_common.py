"""Shared by the Adam tests: the float64 restatement of one update of the kernel family of csrc/pointwise.hip (adam_kernel,
adam_multi_kernel, adam_tick_kernel + adam_multi_dev_kernel / adam_multi_dev_guard_kernel), the derived bounds, and the inputs.

Restatement of one step.  The float32 arrays p, g, m, v are widened exactly; beta1, beta2, eps, step_size and inv_sqrt_bc2 are the
float32 numbers the kernel holds, widened; omb = float32(1) - float32(beta) as the kernel forms it.  In float64:
    m' = beta1 m + omb1 g        v' = beta2 v + omb2 g^2        den = sqrt(v') inv_sqrt_bc2 + eps
    upd = step_size m' / den     p' = p - upd
``tick`` restates adam_tick_kernel: betas and lr as float32, widened; 1 - beta^t in double; step_size = lr / bc1 and
inv_sqrt_bc2 = 1 / sqrt(bc2) rounded to float32 once each.

Bounds, U = 2^-24 (one float32 rounding is a relative error of at most U; float32 division and square root are correctly
rounded on this path).  Contraction into a fused multiply-add only removes roundings, so the uncontracted expression is counted.
  m'   fl(fl(beta1 m) + fl(omb1 g)): each term is rounded twice, once by its product and once by the sum:
       |dm'| <= ((1 + U)^2 - 1) (|beta1 m| + |omb1 g|)                                   = 2 U (...) to first order
  v'   fl(fl(beta2 v) + fl(fl(omb2 g) g)): the g term is rounded three times, the v term twice, and every term is >= 0:
       |dv'| <= ((1 + U)^3 - 1) v'                                                       = 3 U v' to first order
  p'   the kernel divides ITS m' by a denominator made of ITS v'.  sqrt halves the 3 U of v' (1.5 U); the root, the product with
       inv_sqrt_bc2 and the sum with eps round once each (the terms are >= 0): den is off by 4.5 U.  The quotient and the product
       with step_size round once each: 6.5 U |upd| to first order, plus step_size |dm'| / den for the numerator.  The subtraction
       rounds once: U |p'|.  The constant is taken as 8: the 1.5 U of room covers every second-order term (they are below
       100 U^2) with a margin that does not depend on what a device returns.
       |dp'| <= U |p'| + 8 U |upd| + step_size bound(m') / den
Each bound has a floor of 2^-149, the spacing of the subnormal numbers (one product that underflows).  The inputs of ``draw`` keep
v' normal except where g = v = 0, which is exact.  With |p| ~ 1 the term U |p'| hides a relative error of the update below about
6e-5, so every tensor carries elements with p = 0 and |p| <= 1e-3: there the bound is about 8 U of the update itself.

Distance to torch 1.4 (``trajectory``).  torch 1.4 takes the hyper-parameters as Python doubles: with float32 tensors the
complement enters as float32(1 - beta) and the bias corrections come from the double betas, where the kernel holds b = float32(beta)
and derives 1.f - b and 1 - b^t from it.  With d = b - beta and c = |d| / (1 - beta):
  * 1.f - b is exact for beta >= 0.5 (Sterbenz) and equals (1 - beta)(1 - d / (1 - beta)): every increment of v is off by c;
    the power b^k of the k later decays is off by k d / beta, of the OPPOSITE sign and smaller as long as t (1 - beta) <= beta: v is
    off by at most c (+ U for the rounding of float32(1 - beta)), its root by c / 2;
  * 1 - b^t against 1 - beta^t: |b^t - beta^t| <= t |d| max(b, beta)^(t-1) and 1 - beta^t >= t beta^(t-1) (1 - beta) (mean value
    theorem), so bc2 is off by c and inv_sqrt_bc2 by c / 2.
The two places add up to c on the denominator, hence c on the update, for beta2; the same count for beta1 (numerator and bc1)
gives c1 = |float32(beta1) - beta1| / (1 - beta1), which is 0 at beta1 = 0.5.  (In the product sqrt(v) inv_sqrt_bc2 the two halves
have opposite signs, so the observed distance is far below c; the bound does not use that.)  The roundings that differ besides --
float32(lr), the quotient lr / bc1, inv_sqrt_bc2 and float32(eps), one each -- add 4 U |upd| per step.
The rounding of the device's own trajectory against the float64 trajectory with the kernel's numbers accumulates as
  em_t = (1 + U)^2 beta1 em_(t-1) + ((1 + U)^2 - 1)(|beta1 m| + |omb1 g|)         (the moments do not depend on p here)
  rv_t = (1 + U)^(3 t) - 1                                                        (relative, all terms >= 0)
  ep_t = ep_(t-1) + U |p_t| + (rv_t / 2 - 1.5 U + 8 U) |upd_t| + step_size em_t / den_t
so that  |p_dev - p_torch14| <= ep_T + 4 U sum |upd| + (c + c1) sum |upd|."""
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
G2 = (1.0 + U) ** 2 - 1.0
G3 = (1.0 + U) ** 3 - 1.0
P_FACTOR = 8.0

GUARD = 1.5e30
HYPERS = [(1e-3, 0.5, 0.999, 1e-8), (2e-4, 0.9, 0.999, 1e-8), (1e-3, 0.0, 0.99, 1e-3)]        # (lr, beta1, beta2, eps)
STEPS_DONE = [0, 1, 9, 999, 99999]
SIZES = [0, 1, 3, 4095, 4096, 4097, 8197, 40000]
MIXED_N = 8197
N_TINY = 300
STRIDE_N = 2049 * 4096 + 5
QUANTITIES = "pgmv"

f32 = np.float32


# ---- the hyper-parameters --------------------------------------------------------------------------------------------------------
def tick(t, lr, beta1, beta2):
    """adam_tick_kernel at step t: (step_size, inv_sqrt_bc2) as float32"""
    b1, b2, lr = float(f32(beta1)), float(f32(beta2)), float(f32(lr))
    bc1 = 1.0 - b1 ** int(t)
    bc2 = 1.0 - b2 ** int(t)
    return f32(lr / bc1), f32(1.0 / math.sqrt(bc2))


def kernel_scalars(beta1, beta2, eps):
    """the float32 numbers of the record"""
    return f32(beta1), f32(beta2), f32(eps)


def torch14_scalars(t, lr, beta1, beta2, eps):
    """torch 1.4 with float32 tensors, its hyper-parameters Python doubles: the betas and eps as they are, the complement
    float32(1 - beta) from the double, the bias corrections from the double betas -> the keyword arguments of ``adam_f64``"""
    return dict(beta1=float(beta1), beta2=float(beta2), omb1=float(f32(1.0 - beta1)), omb2=float(f32(1.0 - beta2)), eps=float(eps),
                step_size=lr / (1.0 - beta1 ** int(t)), inv_sqrt_bc2=1.0 / math.sqrt(1.0 - beta2 ** int(t)))


def deviation_constant(beta):
    """c of the module docstring"""
    return abs(float(f32(beta)) - beta) / (1.0 - beta)


# ---- one step ----------------------------------------------------------------------------------------------------------------------
class Step:
    """p, m, v after the step, upd and den, all float64; bp, bm, bv: the bounds of the module docstring (kernel numbers only)"""
    __slots__ = ("p", "m", "v", "upd", "den", "bp", "bm", "bv")


def adam_f64(p, g, m, v, beta1, beta2, omb1, omb2, eps, step_size, inv_sqrt_bc2):
    """the five lines of Adam in float64, every scalar as given"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    s = Step()
    s.m = beta1 * m + omb1 * g
    s.v = beta2 * v + omb2 * (g * g)
    s.den = np.sqrt(s.v) * inv_sqrt_bc2 + eps
    s.upd = step_size * s.m / s.den
    s.p = p - s.upd
    return s


def restate(p, g, m, v, beta1, beta2, eps, step_size, inv_sqrt_bc2):
    """one step with the kernel's numbers -- float32 arrays and float32 scalars, widened exactly -- and its bounds"""
    for a in (p, g, m, v):
        assert a.dtype == np.float32
    for x in (beta1, beta2, eps, step_size, inv_sqrt_bc2):
        assert isinstance(x, np.float32), type(x)
    omb1, omb2 = f32(1) - beta1, f32(1) - beta2                      # float32 arithmetic, as the kernel's 1.f - beta
    b1, b2, o1, o2, ss = float(beta1), float(beta2), float(omb1), float(omb2), float(step_size)
    s = adam_f64(p, g, m, v, b1, b2, o1, o2, float(eps), ss, float(inv_sqrt_bc2))
    m64, g64 = m.astype(np.float64), g.astype(np.float64)
    s.bm = np.maximum(G2 * (np.abs(b1 * m64) + np.abs(o1 * g64)), TINY)
    s.bv = np.maximum(G3 * s.v, TINY)
    s.bp = np.maximum(U * np.abs(s.p) + P_FACTOR * U * np.abs(s.upd) + ss * s.bm / s.den, TINY)
    return s


def emulate_f32(p, g, m, v, beta1, beta2, eps, step_size, inv_sqrt_bc2):
    """the kernel's expression in float32 numpy, one rounding per operation (no contraction) -> p', m', v'"""
    for x in (beta1, beta2, eps, step_size, inv_sqrt_bc2):
        assert isinstance(x, np.float32), type(x)
    mi = beta1 * m + (f32(1) - beta1) * g
    vi = beta2 * v + (f32(1) - beta2) * g * g
    pi = p - step_size * (mi / (np.sqrt(vi) * inv_sqrt_bc2 + eps))
    assert mi.dtype == vi.dtype == pi.dtype == np.float32
    return pi, mi, vi


def ratios(got_p, got_m, got_v, s):
    """worst |error| / bound of the three quantities over every element (0 for an empty set)"""
    out = {}
    for name, got, want, bound in (("p", got_p, s.p, s.bp), ("m", got_m, s.m, s.bm), ("v", got_v, s.v, s.bv)):
        r = np.abs(got.astype(np.float64) - want) / bound
        assert not np.isnan(r).any(), name
        out[name] = float(r.max()) if r.size else 0.0
    return out


def ulps_apart(a, b):
    """distance of two positive float32 numbers in units of the last place"""
    return abs(int(f32(a).view(np.int32)) - int(f32(b).view(np.int32)))


# ---- the records and their places ----------------------------------------------------------------------------------------------
class Layout:
    """Where every record's p, g, m and v lie in one buffer per quantity.  A slot is n + 8 elements (rounded up to a multiple of
    four, so that every slot starts 16-byte aligned) filled with GUARD, the record at offset 4 (aligned) or 1 (not).  ``n``: sizes
    in record order; ``start[q]``: first element of each record in the buffer of q; ``idx[q]``: every element of every record, in
    record order; ``total[q]``: elements of the buffer."""

    def __init__(self, slots):
        """slots: [(sizes, {q: offset})] -- the records of one slot lie back to back (one size: an ordinary slot)"""
        self.n = np.array([n for sizes, _ in slots for n in sizes], dtype=np.int64)
        self.first = np.concatenate([[0], np.cumsum(self.n)])          # of each record in the flat element order
        self.start, self.idx, self.total = {}, {}, {}
        for q in QUANTITIES:
            at, starts = 0, []
            for sizes, offs in slots:
                assert offs[q] in (1, 4)
                pos = at + offs[q]
                for n in sizes:
                    starts.append(pos)
                    pos += n
                at += -(-(sum(sizes) + 8) // 4) * 4
            self.start[q] = np.array(starts, dtype=np.int64)
            self.idx[q] = np.concatenate([np.arange(s, s + n) for s, n in zip(starts, self.n)]).astype(np.int64)
            self.total[q] = at
            outside = np.ones(at, dtype=bool)
            outside[self.idx[q]] = False
            assert outside.sum() == at - self.n.sum() and outside[0] and outside[-1]      # no overlap, sentinels at both ends

    def __len__(self):
        return len(self.n)

    def fill(self, q, values):
        """the host image of the buffer of q: sentinels, and ``values`` (flat, record order) in the records"""
        host = np.full(self.total[q], GUARD, dtype=np.float32)
        host[self.idx[q]] = values
        return host

    def guards_intact(self, q, host):
        outside = np.ones(self.total[q], dtype=bool)
        outside[self.idx[q]] = False
        return bool((host[outside] == f32(GUARD)).all())


def same(off):
    return {q: off for q in QUANTITIES}


def main_layout():
    """the records of the op-level cases: four of 8197 elements with exactly ONE of p, g, m, v off the 16-byte grid; every size
    at offset 4 and at offset 1 (the empty records lie between others); 300 tensors of 1..7 elements back to back"""
    slots = [([MIXED_N], dict(same(4), **{q: 1})) for q in QUANTITIES]
    slots += [([n], same(off)) for off in (4, 1) for n in SIZES]
    slots.append(([int(n) for n in np.random.default_rng(11).integers(1, 8, N_TINY)], same(4)))
    lay = Layout(slots)
    assert len(lay) == 4 + 2 * len(SIZES) + N_TINY
    return lay


def draw(lay, seed, mags=None):
    """float32 p, g, m, v for every element of the layout, flat in record order.  One gradient magnitude per record between 1e-12
    and 1e15 (or ``mags``) with |g| >= 1e-3 of it, m ~ 0.3 and v ~ 0.01 of its square (> 0); p cycles through N(0, 1), 0 and |p| <= 1e-3
    element by element; in records of 8 elements or more the first three elements have g = 0, g = v = 0 and g = v = m = 0."""
    rng = np.random.default_rng(seed)
    n_rec, n_all = len(lay), int(lay.n.sum())
    n_big = n_rec - N_TINY if n_rec > N_TINY else n_rec
    if mags is None:
        mags = np.concatenate([rng.permutation(10.0 ** np.linspace(-12, 15, n_big)),
                               rng.permutation(10.0 ** np.linspace(-12, 15, n_rec - n_big))])
    assert len(mags) == n_rec
    mag = np.repeat(mags, lay.n)
    z = rng.standard_normal(n_all)
    g = mag * np.where(z < 0, -1.0, 1.0) * np.maximum(np.abs(z), 1e-3)
    m = 0.3 * mag * rng.standard_normal(n_all)
    v = mag * mag * (1e-4 + 0.01 * rng.random(n_all))
    kind = np.arange(n_all) % 3
    p = np.where(kind == 0, rng.standard_normal(n_all), np.where(kind == 1, 0.0, 1e-3 * rng.uniform(-1, 1, n_all)))
    for first, n in zip(lay.first[:-1], lay.n):
        if n >= 8:
            g[first:first + 3] = 0.0
            v[first + 1:first + 3] = 0.0
            m[first + 2] = 0.0
    return dict(p=p.astype(np.float32), g=g.astype(np.float32), m=m.astype(np.float32), v=v.astype(np.float32))


def case_seed(hyper, steps_done):
    """seed of the inputs of one (index into HYPERS, steps_done) case; the second step's gradients use the next one"""
    return 1000 * hyper + 2 * STEPS_DONE.index(steps_done) + 100


def redraw_g(lay, seed, mags=None):
    """new gradients, with the same zeros, for the second step"""
    return draw(lay, seed, mags)["g"]


# ---- the distance to torch 1.4 -----------------------------------------------------------------------------------------------------
def trajectory(grads, lr, beta1, beta2, eps):
    """From p = m = v = 0 over the gradients of ``grads`` (one float32 array per step) -> (p of the float64 trajectory with the
    torch-1.4 hyper-parameters, the rounding part of the bound, sum |upd|), see the module docstring."""
    n = grads[0].size
    b1, b2, e = kernel_scalars(beta1, beta2, eps)
    o1 = float(f32(1) - b1)
    pk, mk, vk = (np.zeros(n, dtype=np.float64) for _ in range(3))
    pt, mt, vt = (np.zeros(n, dtype=np.float64) for _ in range(3))
    em, ep, total = np.zeros(n), np.zeros(n), np.zeros(n)
    for t, g in enumerate(grads, 1):
        assert t * (1.0 - beta2) <= beta2
        ss, isb = tick(t, lr, beta1, beta2)
        g64 = g.astype(np.float64)
        em = (1.0 + G2) * float(b1) * em + G2 * (np.abs(float(b1) * mk) + np.abs(o1 * g64))
        k = adam_f64(pk, g, mk, vk, float(b1), float(b2), o1, float(f32(1) - b2), float(e), float(ss), float(isb))
        pk, mk, vk = k.p, k.m, k.v
        rv = (1.0 + U) ** (3 * t) - 1.0
        with np.errstate(invalid="ignore", divide="ignore"):
            ep = ep + U * np.abs(pk) + (rv / 2 - 1.5 * U + P_FACTOR * U) * np.abs(k.upd) + float(ss) * em / k.den
        w = adam_f64(pt, g, mt, vt, **torch14_scalars(t, lr, beta1, beta2, eps))
        pt, mt, vt = w.p, w.m, w.v
        total = total + np.abs(w.upd)
    return pt, ep + 4 * U * total, total
