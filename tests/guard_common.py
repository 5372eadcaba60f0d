"""Shared by the gradient-guard tests: the float64 restatement of the norm, the derived bounds, and small op / trainer helpers.

Restatement:  ref = sqrt(sum(float64(g)^2)) over every element of every gradient tensor of the call.
Bound:  |norm_dev - ref| <= ((D + 1) / 2 + 2) * 2^-24 * ref  with D = 24, the documented add depth of one 4096-element chunk
(16 serial adds per thread + 8 tree levels).  Terms: one rounding per square and D adds on non-negative terms give a relative
error of at most (D + 1) * 2^-24 on S (the double sum of the partials adds nothing visible), the square root halves it, one
rounding of the root to float32, one of slack.  The scale min(1, max_norm / (norm + 1e-6f)) adds the rounding of the sum and of
the quotient: ((D + 1) / 2 + 4) * 2^-24 relative to max_norm / (ref + 1e-6).  Everything else the tests check is bit-equality."""
import struct

import numpy as np
import torch

from tests.ema_common import assert_same, live_state, make_trainer, twin_state  # noqa: F401  (re-exported)

D = 24
U = 2.0 ** -24
NORM_FACTOR = (D + 1) / 2 + 2
SCALE_FACTOR = (D + 1) / 2 + 4


def ref_norm(grads):
    """sqrt(sum g^2) in float64 over tensors or arrays"""
    s = 0.0
    for g in grads:
        a = g.detach().cpu().numpy() if torch.is_tensor(g) else np.asarray(g)
        a = a.astype(np.float64).ravel()
        s += float(np.dot(a, a))
    return float(np.sqrt(s))


def norm_bound(ref):
    return NORM_FACTOR * U * ref


def scale_bound(want):
    return SCALE_FACTOR * U * want


def f32_bits(x):
    return struct.unpack("I", struct.pack("f", x))[0]


# ---- op level --------------------------------------------------------------------------------------------------------------
def slot(n, off, values=None):
    """a float32 tensor of n elements ``off`` elements into a larger device buffer (off = 4: 16-byte aligned, off = 1: not)"""
    base = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    view = base[off:off + n]
    if values is not None:
        view.copy_(torch.as_tensor(values, dtype=torch.float32))
    return view


class Reducer:
    """record + table + workspace for a fixed list of gradient tensors, as optim.Adam keeps them"""

    def __init__(self, grads, max_norm=None):
        from srgan_amd import ops
        self.ops, self.grads = ops, grads
        dev = torch.device("cuda")
        self.state = ops.grad_guard_state_new(dev, max_norm)
        self.table, self.n, self.chunks = ops.grad_guard_table(grads, dev)
        self.ws = torch.empty(ops.grad_guard_workspace_bytes(self.chunks), dtype=torch.uint8, device=dev)

    def reduce(self):
        self.ops.grad_guard_reduce_(self.table, self.n, self.chunks, self.ws, self.state)
        return self.stats()

    def stats(self):
        return self.ops.grad_guard_state_read(self.state)


class AdamSet:
    """p, g, m, v of several sizes / alignments with one device Adam record and pointer table (one cohort of optim.Adam)"""

    def __init__(self, shapes, seed, steps_done=0, lr=1e-3, g_scale=1.0):
        from srgan_amd import ops
        self.ops = ops
        rng = np.random.default_rng(seed)
        self.p, self.g, self.m, self.v = [], [], [], []
        for n, off in shapes:
            self.p.append(slot(n, off, rng.standard_normal(n)))
            self.g.append(slot(n, off, rng.standard_normal(n) * g_scale))
            self.m.append(slot(n, off, rng.standard_normal(n) * 0.1))
            self.v.append(slot(n, off, rng.random(n) * 0.01))
        self.lr, self.steps_done = lr, steps_done
        self._bind()

    def _bind(self):
        dev = torch.device("cuda")
        rows = []
        for p, g, m, v in zip(self.p, self.g, self.m, self.v):
            rows.extend((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()))
        self.table = self.ops.upload_small(struct.pack(f"{len(rows)}q", *rows), dev)
        self.state = self.ops.adam_state_new(dev, self.lr, 0.5, 0.999, 1e-8, self.steps_done)
        self.max_numel = max(p.numel() for p in self.p)

    def clone(self, steps_done=None, g=None):
        """a deep copy with the same alignment of every tensor; ``g`` replaces the gradients' values"""
        twin = object.__new__(AdamSet)
        twin.ops, twin.lr = self.ops, self.lr
        twin.steps_done = self.steps_done if steps_done is None else steps_done

        def dup(ts):
            return [slot(t.numel(), 4 if t.data_ptr() % 16 == 0 else 1, t) for t in ts]
        twin.p, twin.m, twin.v = dup(self.p), dup(self.m), dup(self.v)
        twin.g = dup(self.g if g is None else g)
        twin._bind()
        return twin

    def t(self):
        """the Adam record's step counter, read from the device"""
        return struct.unpack("i", self.state.cpu().numpy().tobytes()[:4])[0]

    def step_plain(self):
        self.ops.adam_multi_dev_(self.table, len(self.p), self.max_numel, self.state)

    def step_guarded(self, reducer):
        reducer.reduce()
        self.ops.adam_multi_dev_guard_(self.table, len(self.p), self.max_numel, self.state, reducer.state)

    def snapshot(self):
        return [[t.clone() for t in ts] for ts in (self.p, self.m, self.v)]

    def assert_equals(self, other, what):
        mine = self.snapshot()
        theirs = other.snapshot() if isinstance(other, AdamSet) else other
        for name, a, b in zip("pmv", mine, theirs):
            for i, (x, y) in enumerate(zip(a, b)):
                assert torch.equal(x, y), f"{what}: {name}[{i}] ({x.numel()} elements) differs"


# ---- trainer level ---------------------------------------------------------------------------------------------------------
OPT_STEPS = {"G": 2, "D": 2, "E": 1}      # optimiser steps of one train() at k = 2: k for D, both phases for G, phase 1 for E


def batch_of(seed, batch=4, size=128, poison=None):
    """the synthetic batch of ``seed``; ``poison``: a non-finite value written into ONE pixel of sample 0"""
    from oracle import trainer as otrainer
    x, label = otrainer.synthetic_batch(batch, size, 4, seed=seed)
    if poison is not None:
        x[0, 1, 5, 7] = poison
    return x, label


def train_on(sg, x, label):
    return [float(v) for v in sg.train(x.cuda(), {"source": label["source"].cuda(), "target": label["target"]})]


def run(sg, first_seed, n, batch=4, poison_at=(), between=None):
    """n train steps on the batches of first_seed, first_seed + 1, ...; the steps listed in ``poison_at`` get a NaN pixel;
    ``between(sg, s)`` runs after step s.  The step's noise comes from the global CPU generator, seeded here."""
    torch.manual_seed(first_seed)
    out = []
    for s in range(n):
        x, label = batch_of(first_seed + s, batch, poison=float("nan") if s in poison_at else None)
        out.append(train_on(sg, x, label))
        if between is not None:
            between(sg, s)
    return np.array(out)


def split_steps(state):
    """live_state() -> (tensors without the step counts, the step counts as ints)"""
    tensors = {k: v for k, v in state.items() if not k.endswith(".step")}
    counts = {k: int(v) for k, v in state.items() if k.endswith(".step")}
    return tensors, counts


def all_finite(state):
    return all(bool(torch.isfinite(v).all()) for v in state.values() if v.is_floating_point())
