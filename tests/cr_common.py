"""Shared by the tests of balanced consistency regularisation (srgan_amd.consistency, csrc/consistency.hip): torch restatements of the
transform T and of the fused loss in any dtype (float64 is the reference, float32 on the CPU gives the rounding yardstick e32), the
case lists, and the CPU train-step oracle with the consistency terms.

T (per row, table row [fx, ty, tx, 0, ...]; flags: flip 1, translation 2): ``flip`` along the columns, then zero ``pad`` + slice --
T(x)[i, j] = xf[i - ty, j - tx] inside the image, else 0.  The table is read as the kernel reads it: truncated, clamped (fx into
{0, 1}, |ty| <= h - 1, |tx| <= w - 1), non-finite reads 0.

Loss: maps o_s [2P, per_s], logits z_s [2P, nc]; the front P rows carry ``d_losses``' terms, cr_g = mean_s mean_{r in g} (m_s(r) -
m_s(r + P))^2 with m_s the row mean, and total_with_cr = total + every * (lambda_real * cr_first + lambda_fake * cr_rest), a term with
a zero weight or an empty group left out."""
import itertools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import nets
from oracle import trainer as otrainer

EPS32 = 2.0 ** -23
FLIP, TRANSLATION = 1, 2
MAX_PAIRS = 1024                      # SRGAN_CR_MAX_PAIRS of include/srgan_hip.h


# ---- the transform -------------------------------------------------------------------------------------------------------------------
def table_ints(table, flags, h, w):
    """[(fx, ty, tx)] per row, as the kernel reads a float32 table"""
    out = []
    for row in np.asarray(table, dtype=np.float32):
        def rd(v, lo, hi):
            if not np.isfinite(v):
                return 0
            return int(min(max(math.trunc(float(v)), lo), hi))
        fx = rd(row[0], 0, 1) if flags & FLIP else 0
        ty = rd(row[1], -(h - 1), h - 1) if flags & TRANSLATION else 0
        tx = rd(row[2], -(w - 1), w - 1) if flags & TRANSLATION else 0
        out.append((fx, ty, tx))
    return out


def transform(x, table, flags):
    """T of every row of x [n, 3, h, w] (any dtype; values are copied, never computed with)"""
    n, _, h, w = x.shape
    rows = []
    for xi, (fx, ty, tx) in zip(x, table_ints(table, flags, h, w)):
        xf = torch.flip(xi, dims=(2,)) if fx else xi
        padded = F.pad(xf, (w, w, h, h))                    # zeros all round: every shift up to the image's size is a slice
        rows.append(padded[:, h - ty:2 * h - ty, w - tx:2 * w - tx])
    return torch.stack(rows)


def pairs_ref(xs, table, flags):
    """what ops.cr_pairs writes: [cat(xs) | T(cat(xs))]"""
    x = torch.cat(list(xs), 0)
    return torch.cat([x, transform(x, table, flags)], 0)


# pair-builder shapes (n0, n1, h, w): one source / two, 3 w % 4 != 0 (17 x 23: the scalar path), more than one item per image and a
# grid-stride (128 x 128: 12 items per image), one-pixel-high images
PAIR_SHAPES = [(1, 0, 16, 16), (3, 2, 17, 23), (2, 2, 128, 128), (5, 0, 1, 7)]


def translation_radius(size, ratio=0.125):
    return int(size * ratio + 0.5)


def pair_tables(n, h, w, seed):
    """{name: float32 table [n, 8]}: no shift, +-r, a shift far past the image (clamped to one line short of its size: one row and one
    column survive), flip on and off, and hostile rows (NaN, +-1e30, -0.0, fractions, junk in the unused slots)"""
    ry, rx = translation_radius(h), translation_radius(w)
    g = torch.Generator().manual_seed(seed)
    out = {}
    t = torch.zeros(n, 8)
    out["zero"] = t.clone()
    t[:, 0] = 1.0
    out["flip_only"] = t.clone()
    for name, sy, sx, fx in (("plus_r", ry, rx, 0.0), ("minus_r", -ry, -rx, 1.0)):
        t = torch.zeros(n, 8)
        t[:, 0], t[:, 1], t[:, 2] = fx, float(sy), float(sx)
        out[name] = t
    t = torch.zeros(n, 8)
    t[:, 0] = (torch.arange(n) % 2).float()
    t[:, 1], t[:, 2] = float(3 * h + 5), float(-(3 * w + 5))
    out["past_the_image"] = t
    t = torch.zeros(n, 8)
    t[:, 0] = (torch.rand(n, generator=g) < 0.5).float()
    t[:, 1] = torch.randint(-ry, ry + 1, (n,), generator=g).float()
    t[:, 2] = torch.randint(-rx, rx + 1, (n,), generator=g).float()
    out["drawn"] = t
    hostile = torch.tensor([[float("nan"), float("nan"), float("nan")], [1e30, 1e30, -1e30], [-1e30, -1e30, 1e30],
                            [-0.0, -0.0, -0.0], [0.9, 1.9, -1.9], [float("inf"), float("-inf"), float("inf")], [7.0, 0.5, -0.5]])
    t = torch.full((n, 8), float("nan"))
    t[:, :3] = hostile[torch.arange(n) % hostile.shape[0]]
    out["hostile"] = t
    return out


def pair_images(n, h, w, seed):
    """float32 images with -0.0, +-Inf and NaNs of several payloads planted: a copy must keep every bit"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, h, w, generator=g) * 2 - 1
    flat = x.view(torch.int32).flatten()
    idx = torch.randperm(flat.numel(), generator=g)[:min(8, flat.numel())]
    planted = torch.tensor([-2147483648, 0x7FC00001, 0x7F800123, -4194304 + 77, 0x7F800000, -8388608, 1, 0x007FFFFF], dtype=torch.int32)
    flat[idx] = planted[:idx.numel()]
    return x


# ---- the fused loss --------------------------------------------------------------------------------------------------------------
def _gan(kind, o, target):
    t = torch.full_like(o, target)
    return F.binary_cross_entropy_with_logits(o, t) if kind else F.mse_loss(o, t)


def _cls(kind, z, label):
    q = torch.softmax(z, 1)
    y = F.one_hot(label.long(), z.shape[1]).to(z.dtype)
    return F.binary_cross_entropy(q, y) if kind else F.mse_loss(q, y)


def loss_vals(outs, logits, label, rows_first, t_first, t_rest, w_class, lam_real, lam_fake, every, gan_kind, class_kind, pairs_first):
    """-> the seven values of srgan_d_losses_cr as 0-dim tensors of the inputs' dtype (differentiable in outs and logits)"""
    S, P = len(outs), outs[0].shape[0] // 2
    zero = outs[0].new_zeros(())
    first, rest, cls, cr1, cr2 = zero, zero, zero, zero, zero
    for s, o in enumerate(outs):
        o = o.reshape(2 * P, -1)
        if rows_first > 0:
            first = first + _gan(gan_kind, o[:rows_first], t_first) / S
        if P - rows_first > 0:
            rest = rest + _gan(gan_kind, o[rows_first:P], t_rest) / S
        m = o.mean(1)
        d = m[:P] - m[P:]
        if pairs_first > 0:
            cr1 = cr1 + (d[:pairs_first] ** 2).mean() / S
        if P - pairs_first > 0:
            cr2 = cr2 + (d[pairs_first:] ** 2).mean() / S
        if logits:
            cls = cls + _cls(class_kind, logits[s][:rows_first], label[:rows_first]) / S
    total = first + w_class * cls + rest
    c1, c2 = lam_real * every, lam_fake * every
    with_cr = total
    if c1 != 0 and pairs_first > 0:
        with_cr = with_cr + c1 * cr1
    if c2 != 0 and P - pairs_first > 0:
        with_cr = with_cr + c2 * cr2
    return [first, cls, rest, total, cr1, cr2, with_cr]


def cr_grad_closed(outs, lam_real, lam_fake, every, pairs_first):
    """the consistency terms' share of d total_with_cr / d o_s, in closed form: 2 c_g / (S B_g per_s) (m_s(r) - m_s(r + P)) at every
    element of front row r, the negative at row r + P"""
    S, P = len(outs), outs[0].shape[0] // 2
    res = []
    for o in outs:
        o2 = o.detach().reshape(2 * P, -1)
        per = o2.shape[1]
        m = o2.mean(1)
        d = m[:P] - m[P:]
        k = torch.zeros(P, dtype=o2.dtype)
        if pairs_first > 0:
            k[:pairs_first] = 2 * lam_real * every / (S * pairs_first * per)
        if P - pairs_first > 0:
            k[pairs_first:] = 2 * lam_fake * every / (S * (P - pairs_first) * per)
        g = (k * d)[:, None].expand(P, per)
        res.append(torch.cat([g, -g], 0).reshape(o.shape))
    return res


def loss_run(inputs, dtype, **kw):
    """the restated scalar and its autograd gradients -> (vals [7], [d_o per scale], [dz per scale]) in ``dtype`` on the CPU"""
    outs = [o.detach().cpu().to(dtype).requires_grad_(True) for o in inputs["outs"]]
    logits = [z.detach().cpu().to(dtype).requires_grad_(True) for z in inputs["logits"]]
    vals = loss_vals(outs, logits, inputs["label"].cpu(), **kw)
    grads = torch.autograd.grad(vals[6], outs + logits, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, outs + logits)]
    return torch.stack([v.detach() for v in vals]), grads[:len(outs)], grads[len(outs):]


# P: one pair, fewer pairs than threads, 257: more rows than the 256 threads, 1024: SRGAN_CR_MAX_PAIRS.  per_row: the tier-T maps,
# one-element maps, a long row with an odd second scale.  The longest sequential fp32 sum of one thread of d_losses_cr_kernel is the
# GAN sum of the front rows, thread t adding elements t, t + 256, ...: L = ceil(P * max(per_row) / 256) (+ 6 butterfly levels and 4
# waves, which the bound's + 16 covers); the row means add ceil(per / 64) per lane, the pair sums at most 4.
LOSS_P = [1, 3, 8, 257, 1024]
LOSS_PER_ROW = [(49, 9), (1, 1), (1000, 7)]
KINDS = [(0, 0), (1, 0), (0, 1), (1, 1)]          # (gan_kind, class_kind): 0 MSE, 1 BCE


def loss_L(P, per_row):
    return -(-P * max(per_row) // 256)


def loss_cases():
    """[(P, per_row, pairs_first, gan_kind, class_kind, with_class)]: every P x per_row x pairs_first, the kinds and the class heads
    rotating through them; then every kind pair with and without class heads at P = 8"""
    out = []
    for i, (P, per, which) in enumerate(itertools.product(LOSS_P, LOSS_PER_ROW, range(3))):
        gk, ck = KINDS[i % 4]
        out.append((P, per, (0, P // 2, P)[which], gk, ck, bool((i // 4) % 2 == 0)))
    for (gk, ck), with_class in itertools.product(KINDS, (False, True)):
        out.append((8, (49, 9), 4, gk, ck, with_class))
    return out


def loss_inputs(P, per_row, with_class, seed, nc=4):
    g = torch.Generator().manual_seed(seed)
    outs = [torch.randn(2 * P, per, generator=g) * 0.7 + 0.3 for per in per_row]
    logits = [torch.randn(2 * P, nc, generator=g) for _ in per_row] if with_class else []
    label = torch.randint(0, nc, (2 * P,), generator=g)
    return dict(outs=outs, logits=logits, label=label)


# ---- the train-step oracle with the consistency terms -----------------------------------------------------------------------------
def scores(out):
    """[S, N]: the patch mean of every scale's GAN map"""
    return torch.stack([o.mean(dim=(1, 2, 3)) for o in out])


class CROracle(otrainer.SRGANOracle):
    """``SRGANOracle`` whose discriminator update i back-propagates errD + every * (lambda_real * cr_real + lambda_fake * cr_fake) iff
    i % every == 0; errD and the trace are unchanged, ``trace["errD_cr"]`` lists (cr_real, cr_fake) of the penalised updates.  The T
    tables come from a ``srgan_amd.consistency.ConsistencyPairs`` seeded like the trainer's: real rows' table, then fake rows'."""

    def __init__(self, *args, lambda_real=10.0, lambda_fake=10.0, every=1, policy="flip,translation", translation=0.125, seed=None,
                 **kwargs):
        from srgan_amd.consistency import ConsistencyPairs
        super().__init__(*args, **kwargs)
        self.lambda_real, self.lambda_fake, self.every = float(lambda_real), float(lambda_fake), int(every)
        self.pairs = ConsistencyPairs(policy, translation, seed)
        self._i = 0

    def train(self, source_image, label, capture_grads=False):
        self._i = 0
        return super().train(source_image, label, capture_grads)

    def update_D(self):
        otrainer._zero(self.D)
        self.target_image, self.c_rand = self._translate(self.label["target"], self.source)
        fake_in = self.target_image.detach()
        out, cls = nets.discriminator(self.D, self.source, self.n_class)
        real = otrainer.losses.lsgan(out, 1.0)
        dom = otrainer.losses.class_mse(cls, self._onehot(self.label["source"]))
        out_f, _ = nets.discriminator(self.D, fake_in, self.n_class)
        fake = otrainer.losses.lsgan(out_f, 0.0)
        errD = real + dom * self.lbd["class"] + fake
        total = errD
        if self._i % self.every == 0:
            n, _, h, w = self.source.shape
            flags = self.pairs.flags
            t_real, t_fake = self.pairs.draw(n, h, w), self.pairs.draw(n, h, w)
            out_tr, _ = nets.discriminator(self.D, transform(self.source, t_real, flags), self.n_class)
            out_tf, _ = nets.discriminator(self.D, transform(fake_in, t_fake, flags), self.n_class)
            cr_real = ((scores(out) - scores(out_tr)) ** 2).mean()
            cr_fake = ((scores(out_f) - scores(out_tf)) ** 2).mean()
            self.trace.setdefault("errD_cr", []).append((float(cr_real.detach()), float(cr_fake.detach())))
            total = errD + self.every * (self.lambda_real * cr_real + self.lambda_fake * cr_fake)
        self._i += 1
        total.backward()
        self.trace.setdefault("errD_iters", []).append(float(errD))
        self.trace.setdefault("errD_parts", []).append((float(real), float(dom), float(fake)))
        if self.capture_grads:
            self.trace.setdefault("gradD", []).append({k: p.grad.clone() for k, p in self.D.items()})
        self.optD.step()
        return errD.detach()


# the weight of the train tests: Adam divides the scale of a gradient out, so a consistency term much smaller than errD leaves D within
# close_params of the plain step after K = 2 updates.  tests/test_cr_refs_cpu.py holds the oracle to "at this weight the term acts".
LAMBDA_ACTS = 1.0e4
CR_SEED = 23
