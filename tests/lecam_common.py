"""Shared by the tests of LeCam regularisation (srgan_amd.lecam, csrc/lecam.hip): a torch restatement of one ``srgan_lecam`` call in
any dtype (float64 is the reference, float32 on the CPU the rounding yardstick), the case lists, a numpy float32 emulation of the
kernel's summation order, the derived error bounds, and the CPU train-step oracle with the term.

One call, on maps o_s [rows, per_s] whose front P rows are what D reads (the first B1 real, the other B2 = P - B1 generated), a
record {weight, decay, start, updates, a_real[S], a_fake[S]}, the gradient buffers d_o_s and the incoming total:

    means     m_R,s / m_F,s over the real / generated elements
    anchors   n = updates, d = 0 if n == 0 else decay:  a <- d a + (1 - d) m; any of the 2S means not finite: none moves, n stays;
              an empty group has no mean, its anchor stays
    term      R = (1 / S) sum_s [ mean_real phi(o - a_F,s)^2 + mean_fake phi(a_R,s - o)^2 ], updated anchors, detached; an empty
              group's half is left out; phi = identity, or relu (clamp)
    gradient  active = weight != 0 and n >= start: d_o += d (weight R) / d o on the front rows; otherwise d_o keeps its bits
    vals      [R, weight R if active else 0, total_in + that]

Bounds (convention of tests/test_small_kernels_gpu.py: (depth of the longest add chain + 16) * 2^-23, times the magnitudes involved).
A thread of lecam_kernel adds the elements of its quads t, t + 256, ... into one accumulator: L = 4 ceil(ceil(N / 4) / 256) adds for
N = P per_s front elements, then 6 butterfly levels and 4 waves, which the + 16 covers.  With M = max |o| and u = 2^-23:

    anchor after call c      |err| <= (L + 16 + 3 c) u M        a mean of values within M; the recurrence is a convex combination, so
                                                                it passes the means' error on and adds three roundings of values
                                                                within M per call.  THE BOUND SCALES WITH max |o|: maps at +1000
                                                                with unit spread have anchors good to 1000 (L + 16) u, not to
                                                                (L + 16) u of their spread.
    phi                      E = anchor bound + u max |phi|     one subtraction; relu is 1-Lipschitz
    R                        2 E sqrt(2 R) + 2 E^2 + (L + 16) u R      (sum over the 2S group means of 2 |phi| E + E^2, Cauchy-Schwarz;
                                                                        then squares, sums and the divisions)
    d_o increment            k (E + 4 u max |phi|) + u max |d_o after|  k = 2 weight / (S n_g); the last term is the rounding of the
                                                                        add into the pre-filled buffer
    weight R, the total      weight err(R) + u weight R (+ u |total|)
"""
import math

import numpy as np
import torch

from oracle import nets
from oracle import trainer as otrainer

EPS32 = 2.0 ** -23
MAX_SCALES = 4

# (S, P, B1, per, rows): the issue's list.  63 / 64 / 65: the 16-byte path cannot, can, cannot run; B1 = 0 / B1 = P: the empty groups;
# (2, 33, 16, 1000): 32 trips per thread; the last: rows = 2 P, the back rows and their d_o must keep every bit.
SHAPES = [(1, 2, 1, 1, 2), (2, 3, 1, 5, 3), (2, 7, 3, 63, 7), (2, 7, 3, 64, 7), (2, 7, 3, 65, 7), (4, 5, 2, 9, 5), (2, 5, 0, 9, 5),
          (2, 5, 5, 9, 5), (2, 33, 16, 1000, 33), (2, 6, 3, 20, 12)]


def per_rows(S, per):
    """per_s of every scale: the first as given, the following ones smaller (an odd second scale), never below 1"""
    return [max(1, per // (1 << s) + (s % 2)) if s else per for s in range(S)]


def make_maps(S, P, per, rows, seed, shift=0.3, spread=0.7):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(rows, p, generator=g) * spread + shift for p in per_rows(S, per)]


def new_record(weight, decay, start, S):
    """the record's fields the restatement needs, as the device reads them: float32 settings"""
    return dict(weight=float(np.float32(weight)), decay=float(np.float32(decay)), start=int(start), updates=0, a_real=[0.0] * S,
                a_fake=[0.0] * S)


def phi(x, clamp):
    return torch.relu(x) if clamp else x


def term(outs, a_real, a_fake, P, B1, clamp):
    """R of maps ``outs`` (differentiable in them) against constant anchors"""
    S = len(outs)
    R = outs[0].new_zeros(())
    for s, o in enumerate(outs):
        f = o.reshape(o.shape[0], -1)[:P]
        if B1 > 0:
            R = R + (phi(f[:B1] - a_fake[s], clamp) ** 2).mean() / S
        if P - B1 > 0:
            R = R + (phi(a_real[s] - f[B1:], clamp) ** 2).mean() / S
    return R


def grad_closed(outs, a_real, a_fake, P, B1, clamp):
    """d R / d o_s in closed form: +2 / (S n1) phi(o - a_F,s) on a real element, -2 / (S n2) phi(a_R,s - o) on a generated one, zero on
    the back rows"""
    S, res = len(outs), []
    for s, o in enumerate(outs):
        o2 = o.detach().reshape(o.shape[0], -1)
        per = o2.shape[1]
        g = torch.zeros_like(o2)
        if B1 > 0:
            g[:B1] = 2.0 / (S * B1 * per) * phi(o2[:B1] - a_fake[s], clamp)
        if P - B1 > 0:
            g[B1:P] = -2.0 / (S * (P - B1) * per) * phi(a_real[s] - o2[B1:P], clamp)
        res.append(g.reshape(o.shape))
    return res


def call(outs, rec, P, B1, clamp, total_in, dtype):
    """One ``srgan_lecam`` in ``dtype`` on the CPU -> (vals [3], [the increment of d_o per scale], the new record, the 2S means).
    ``rec`` is not modified."""
    S = len(outs)
    o = [t.detach().cpu().to(dtype).reshape(t.shape[0], -1) for t in outs]
    cast = lambda v: torch.tensor(v, dtype=dtype)
    a_r, a_f = [cast(v) for v in rec["a_real"]], [cast(v) for v in rec["a_fake"]]
    n, B2 = rec["updates"], P - B1
    m_r = [t[:B1].mean() if B1 > 0 else None for t in o]
    m_f = [t[B1:P].mean() if B2 > 0 else None for t in o]
    ok = all(bool(torch.isfinite(m)) for m in m_r + m_f if m is not None)
    d = cast(0.0 if n == 0 else rec["decay"])
    if ok:
        a_r = [d * a + (1 - d) * m if m is not None else a for a, m in zip(a_r, m_r)]
        a_f = [d * a + (1 - d) * m if m is not None else a for a, m in zip(a_f, m_f)]
    w = cast(rec["weight"])
    active = rec["weight"] != 0 and n >= rec["start"]
    R = term(o, a_r, a_f, P, B1, clamp)
    incr = [w * g if active else torch.zeros_like(g) for g in grad_closed(o, a_r, a_f, P, B1, clamp)]
    total_in = cast(total_in)
    wr = w * R if active else cast(0.0)
    vals = torch.stack([R, wr, total_in + wr if active else total_in])
    new = dict(rec, updates=n + (1 if ok else 0), a_real=[float(a) for a in a_r], a_fake=[float(a) for a in a_f],
               penalty=float(R), applied=int(active))
    return vals, incr, new, (m_r, m_f)


# ---- the kernel's summation order in numpy float32 ---------------------------------------------------------------------------------
def chain_depth(n_front):
    """L: adds of one thread's accumulator over N front elements"""
    return 4 * -(-(-(-n_front // 4)) // 256)


def emulate_sums(front, n1):
    """(sum of front[:n1], sum of front[n1:]) in float32 in lecam_kernel's order: quad q = e // 4 belongs to thread q % 256, which adds
    its elements ascending into one accumulator per sum; the 64 lanes of a wave by the xor butterfly 32, 16, ... 1; the four waves
    ascending onto 0.  (Adding the +0.0 this emulation puts where a thread has no element changes no bit of a sum that starts at
    +0.0.)"""
    x = np.asarray(front, dtype=np.float32).ravel()
    N = x.size
    trips = -(-(-(-N // 4)) // 256)
    idx = np.arange(trips * 256 * 4)
    padded = np.zeros(trips * 256 * 4, dtype=np.float32)
    padded[:N] = x
    out = []
    for mask in (idx < n1, (idx >= n1) & (idx < N)):
        v = np.where(mask, padded, np.float32(0.0)).reshape(trips, 256, 4)
        acc = np.zeros(256, dtype=np.float32)
        for t in range(trips):
            for k in range(4):
                acc = (acc + v[t, :, k]).astype(np.float32)
        w = acc.reshape(4, 64)
        lanes = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            w = (w + w[:, lanes ^ off]).astype(np.float32)
        total = np.float32(0.0)
        for i in range(4):
            total = np.float32(total + w[i, 0])
        out.append(total)
    return out


# ---- the bounds of the module docstring --------------------------------------------------------------------------------------------
def anchor_bound(L, c, M):
    return (L + 16 + 3 * c) * EPS32 * M


def term_bound(L, E, R):
    return 2 * E * math.sqrt(2 * R) + 2 * E * E + (L + 16) * EPS32 * R


def grad_bound(k, E, max_phi, max_after):
    return k * (E + 4 * EPS32 * max_phi) + EPS32 * max_after


# ---- the train-step oracle with the term ---------------------------------------------------------------------------------------------
class LeCamOracle(otrainer.SRGANOracle):
    """``SRGANOracle`` whose every discriminator update moves the anchors and back-propagates errD + weight * R once ``updates >=
    start``; errD and the trace are unchanged, ``trace["errD_lecam"]`` lists R per update."""

    def __init__(self, *args, weight=0.3, decay=0.99, start=0, clamp=False, **kwargs):
        super().__init__(*args, **kwargs)
        self.lc = None
        self.lc_settings = (weight, decay, start)
        self.clamp = bool(clamp)

    def update_D(self):
        otrainer._zero(self.D)
        self.target_image, self.c_rand = self._translate(self.label["target"], self.source)
        out, cls = nets.discriminator(self.D, self.source, self.n_class)
        real = otrainer.losses.lsgan(out, 1.0)
        dom = otrainer.losses.class_mse(cls, self._onehot(self.label["source"]))
        out_f, _ = nets.discriminator(self.D, self.target_image.detach(), self.n_class)
        fake = otrainer.losses.lsgan(out_f, 0.0)
        errD = real + dom * self.lbd["class"] + fake
        if self.lc is None:
            self.lc = new_record(*self.lc_settings, len(out))
        B = self.source.shape[0]
        maps = [torch.cat([a.reshape(B, -1), b.reshape(B, -1)], 0) for a, b in zip(out, out_f)]
        _, _, new, _ = call(maps, self.lc, 2 * B, B, self.clamp, 0.0, maps[0].dtype)
        R = term(maps, new["a_real"], new["a_fake"], 2 * B, B, self.clamp)
        total = errD + self.lc["weight"] * R if new["applied"] else errD
        self.lc = new
        self.trace.setdefault("errD_lecam", []).append(float(R.detach()))
        total.backward()
        self.trace.setdefault("errD_iters", []).append(float(errD.detach()))
        self.trace.setdefault("errD_parts", []).append((float(real.detach()), float(dom.detach()), float(fake.detach())))
        if self.capture_grads:
            self.trace.setdefault("gradD", []).append({k: p.grad.clone() for k, p in self.D.items()})
        self.optD.step()
        return errD.detach()


LC_WEIGHT = 10.0            # the train tests' weight: large enough that the term's gradient is not lost beside errD's
