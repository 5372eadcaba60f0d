"""Shared by the EMA tests: the float64 restatement of the update, the derived bound, and small trainer helpers (copies of
those in tests/test_graph_gpu.py).

Restatement, for update number n = 1, 2, ...:
    d = float32(min(decay, (1 + n) / (10 + n)) if ramp else decay);  c = float32(1) - d (float32 arithmetic);
    e = e + float(c) * (p - e)   in float64.
Bound: the device evaluates fl(e + fl(c * fl(p - e))), at most three roundings per update.  With M = max(|p|, |e|) over the
run, |p - e| <= 2M, so one update adds at most (2 + 2 + 1) * 2^-24 * M and earlier error is multiplied by 1 - c <= 1: after T
updates |e_dev - e_ref| <= 5 * T * 2^-24 * M elementwise.  Everything else the tests check is bit-equality."""
import numpy as np
import torch
import torch.nn as nn


def decay_ref(n, decay, ramp):
    return np.float32(min(decay, (1 + n) / (10 + n)) if ramp else decay)


def restate(e, p, n, decay, ramp):
    """One update, number ``n``: e, p array-likes -> float64 array."""
    c = np.float32(1) - decay_ref(n, decay, ramp)
    e = np.asarray(e, dtype=np.float64)
    return e + float(c) * (np.asarray(p, dtype=np.float64) - e)


def bound(T, M):
    return 5 * T * 2.0 ** -24 * M


def np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def param_snapshot(net):
    return {k: np64(v) for k, v in net.named_parameters()}


def check_within_bound(twin, e_ref, T, M, what):
    """every parameter of ``twin`` against the restated float64 trajectory ``e_ref`` ({name: array}); ``M``: {name: max(|p|, |e|)
    of that tensor over the run}"""
    worst = 0.0
    for k, v in twin.named_parameters():
        err, lim = float(np.abs(np64(v) - e_ref[k]).max()), bound(T, M[k])
        worst = max(worst, err / lim if lim > 0 else 0.0)
        assert err <= lim, f"{what}.{k}: |e_dev - e_ref| = {err:.3e} > 5*T*2^-24*M = {lim:.3e} (T={T}, M={M[k]:.3e})"
    print(f"{what}: worst error / bound = {worst:.3f} (T={T})")


def make_trainer(tier="T", batch=4, k=2, seed=2, nets=None, opts=(None, None, None)):
    from oracle import trainer as otrainer
    from srgan_amd.trainer import SRGAN_training
    from tests.common import build_hip_nets
    G, D, E = nets if nets is not None else build_hip_nets(tier)
    torch.manual_seed(seed)
    sg = SRGAN_training([G, D, E], list(opts), [nn.MSELoss(), nn.MSELoss()], dict(otrainer.DEFAULT_LBD), k, "cuda", np.eye(4),
                        batch, "mu", 8)
    sg.opt_sche_initialization()
    return sg


def one_step(sg, batch, seed, size=128):
    from oracle import trainer as otrainer
    x, label = otrainer.synthetic_batch(batch, size, 4, seed=seed)
    return [float(v) for v in sg.train(x.cuda(), {"source": label["source"].cuda(), "target": label["target"]})]


def steps(sg, batch, n, first_seed, size=128, after=None):
    """n train steps; the step's noise comes from the global CPU generator, so it is seeded here"""
    torch.manual_seed(first_seed)
    out = []
    for s in range(n):
        out.append(one_step(sg, batch, first_seed + s, size))
        if after is not None:
            after(sg, s)
    return np.array(out)


def live_state(sg):
    """parameters and buffers of G / D / E and every Adam moment, cloned"""
    out = {f"{n}.{k}": v.detach().clone() for n, net in (("G", sg.G), ("D", sg.D), ("E", sg.E)) for k, v in net.state_dict().items()}
    for n, opt in (("G", sg.optG), ("D", sg.optD), ("E", sg.optE)):
        for i, p in enumerate(q for g in opt.param_groups for q in g["params"]):
            for key, v in (opt.state.get(p) or {}).items():
                out[f"opt{n}.{i}.{key}"] = v.detach().clone() if torch.is_tensor(v) else torch.tensor(v)
    return out


def twin_state(sg):
    out = {}
    for n, net in (("G", sg.G_ema), ("E", sg.E_ema)):
        if net is not None:
            out.update({f"{n}.{k}": v.detach().clone() for k, v in net.state_dict().items()})
    return out


def assert_same(a, b, what=""):
    assert a.keys() == b.keys(), what
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what} {k}"
