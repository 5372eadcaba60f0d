"""Shared by the checkpoint tests: the two runs every GPU case compares, and what "the same state" means.

Run A:  seed, build, train ``n1`` steps, ``save_checkpoint``, train ``n2`` more steps on fixed batches.
Run B:  build the same networks from ANOTHER fill seed, seed the CPU generator differently (so the histogram target, the
        spectral-norm vectors and the noise stream all start elsewhere), ``load_checkpoint``, train the same ``n2`` batches.
The bound is bit-identity: the three returned losses and every entry of ``loss_terms`` of each of the ``n2`` steps, and
``final_state`` at the end.  No tolerance anywhere.  Builders and comparers come from tests/ema_common.py and tests/guard_common.py.
"""
import numpy as np
import torch

from tests.ema_common import assert_same, live_state, make_trainer, twin_state  # noqa: F401  (re-exported)
from tests.guard_common import batch_of

BATCH, K, SIZE = 4, 2, 128          # tier T: the smallest size at which the second discriminator scale still has an output for R1
FIRST_SEED = 700                    # the batch of step s is batch_of(FIRST_SEED + s)


def train_row(sg, seed, batch=BATCH, size=SIZE, n_class=4):
    """one train step on the batch of ``seed`` -> ([3 returned losses], {loss term: value}) as Python floats (exact: float32)"""
    if n_class == 4:
        x, label = batch_of(seed, batch, size)
    else:
        from oracle import trainer as otrainer
        x, label = otrainer.synthetic_batch(batch, size, n_class, seed=seed)
    res = sg.train(x.cuda(), {"source": label["source"].cuda(), "target": label["target"]})
    return [float(v) for v in res], {k: float(v) for k, v in sg.loss_terms.items()}


def train_rows(sg, first, n, between=None, **kw):
    """steps first .. first + n - 1; ``between(sg, i)`` runs after the i-th of them"""
    rows = []
    for i in range(n):
        rows.append(train_row(sg, FIRST_SEED + first + i, **kw))
        if between is not None:
            between(sg, i)
    return rows


def step_schedulers(sg, i):
    """one scheduler step after the first step of a continuation: the scheduler state and the lr push to the device records"""
    if i == 0:
        for sche in (sg.scheG, sg.scheD, sg.scheE):
            for s in (sche if isinstance(sche, list) else [sche]):
                s.step()


def assert_rows_equal(a, b, what):
    assert len(a) == len(b), what
    for s, ((la, ta), (lb, tb)) in enumerate(zip(a, b)):
        assert la == lb, f"{what}: returned losses of step {s}: {la} != {lb}"
        assert ta.keys() == tb.keys(), f"{what}: loss_terms of step {s}: {sorted(ta)} != {sorted(tb)}"
        for k in ta:
            assert ta[k] == tb[k], f"{what}: loss_terms[{k!r}] of step {s}: {ta[k]!r} != {tb[k]!r}"


def _opts(sg):
    out = []
    for n in ("G", "D", "E"):
        opt = getattr(sg, "opt" + n)
        out += [(f"{n}{i}", o) for i, o in enumerate(opt)] if isinstance(opt, list) else [(n, opt)]
    return out


def final_state(sg):
    """{name: tensor} of everything a resumed run must agree on: parameters and buffers of G / D / E, every Adam moment and step
    count, the learning rates, the histogram target, the EMA copies and their update count, the CPU generator, the DiffAugment
    generator."""
    if isinstance(sg.D, list):
        out = {}
        nets = [("G", sg.G), ("E", sg.E)] + [(f"D{i}", d) for i, d in enumerate(sg.D)]
        for n, net in nets:
            out.update({f"{n}.{k}": v.detach().clone() for k, v in net.state_dict().items()})
        for n, opt in _opts(sg):
            for i, p in enumerate(q for g in opt.param_groups for q in g["params"]):
                for key, v in (opt.state.get(p) or {}).items():
                    out[f"opt{n}.{i}.{key}"] = v.detach().clone() if torch.is_tensor(v) else torch.tensor(v)
    else:
        out = live_state(sg)
    for n, opt in _opts(sg):
        out[f"lr.{n}"] = torch.tensor([g["lr"] for g in opt.param_groups], dtype=torch.float64)
    if getattr(sg, "hi", None) is not None:
        out["hist_target"] = sg.hi.target.detach().clone()
    if getattr(sg, "_ema", None) is not None:
        out.update({"ema." + k: v for k, v in twin_state(sg).items()})
        out["ema.updates"] = torch.tensor(sg.ema_updates)
    out["rng.torch"] = torch.get_rng_state()
    if getattr(sg, "augment", None) is not None:
        out["rng.augment"] = sg.augment.generator.get_state()
    return out


def assert_state_equal(a, b, what):
    assert a.keys() == b.keys(), f"{what}: {sorted(set(a) ^ set(b))}"
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].cpu(), b[k].cpu()), f"{what}: {k} differs"


def step_counts_are_ints(sg):
    return all(type(st["step"]) is int for _, opt in _opts(sg) for st in opt.state.values() if st)


def run_a(build, path, n1, n2, between=None, at_save=None, **kw):
    """-> (trainer, rows of the n2 steps after the save, final_state).  ``build()`` makes the trainer with everything on;
    ``at_save(sg)`` looks at it when the file is written."""
    sg = build()
    torch.manual_seed(FIRST_SEED)            # the step's noise comes from the global CPU generator
    train_rows(sg, 0, n1, **kw)
    sg.save_checkpoint(path)
    if at_save is not None:
        at_save(sg)
    rows = train_rows(sg, n1, n2, between, **kw)
    return sg, rows, final_state(sg)


def run_b(build, path, n1, n2, between=None, **kw):
    """``build()`` makes the bare trainer from another fill; the CPU generator is somewhere else when the file is loaded"""
    sg = build()
    torch.manual_seed(424242)
    np.random.seed(7)
    report = sg.load_checkpoint(path)
    assert report.missing == [] and report.unexpected == [], report
    rows = train_rows(sg, n1, n2, between, **kw)
    return sg, rows, final_state(sg)
