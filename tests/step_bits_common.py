"""Shared by tests/golden/make_step_parent_bits.py and tests/test_train_gpu.py: the five ``SRGAN_training`` configurations whose
eager steps tests/golden/train_step_parent_bits.npz records bit for bit, and the routine that runs one of them and returns
what the fixture holds.  Public API only, plus ``tests.common.build_hip_nets``, ``tests.batch_common.batch_fill`` and
``oracle.trainer.synthetic_batch``."""
import ctypes
import hashlib
import json

import numpy as np
import torch
import torch.nn as nn

from oracle import trainer as otrainer
from tests.common import build_hip_nets

# tier T, 128x128 (H and W multiples of 16, as the R1 penalty needs), batch 4: the smallest shapes the trajectory tests run at
BATCH, SIZE, FIRST_SEED = 4, 128, 300
LBD = dict(otrainer.DEFAULT_LBD, KL=0.1)
#        name          k  steps
CASES = {"plain":      (3, 3),      # phase 1 pair path, KL term, phase 2's per-sample fused branch, batched k-1 translations
         "all_on":     (3, 4),      # spectral D, gradient guard, EMA, DiffAugment, R1 on updates 0 and 2
         "batch_norm": (2, 2),      # no pair path, phase 2's batch-statistics branch, running-buffer order
         "generic":    (2, 2),      # D without forward_logits: _d_losses, phase 2's generic branch
         "latent":     (2, 2)}      # encoded_feature="latent"
WITH_LAUNCH_COUNTS = ("plain", "all_on")     # also the cases the test repeats in graph mode


class PlainD(nn.Module):
    """A discriminator without ``forward_logits`` (as tests/test_criteria_gpu.py::_PlainD): the trainer leaves the fused paths."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return self.inner(x)


def make_trainer(case):
    from srgan_amd import model, spectral
    from srgan_amd.trainer import SRGAN_training
    k, _ = CASES[case]
    if case == "batch_norm":
        from oracle import params
        from tests.batch_common import batch_fill
        G = batch_fill(model.SingleGenerator(3, 4, 2, 2, 1, "batch", num_con=12), 0).cuda()
        E = batch_fill(model.Encoder(3, 8, 4, 4, "batch", 4, "cuda"), 2).cuda()
        D = model.SingleDiscriminator_solo_multi(3, 4, 2, 4, "batch", 4)
        D.load_state_dict(params.fill(params.discriminator_spec(nch_in=3, nch=4, reduce=2, num_cls=4, n_class=4), 1))
        D = D.cuda()
    else:
        G, D, E = build_hip_nets("T")
    if case == "generic":
        D = PlainD(D)
    torch.manual_seed(0)
    np.random.seed(0)
    sg = SRGAN_training([G, D, E], [None, None, None], [nn.MSELoss(), nn.MSELoss()], dict(LBD), k, "cuda", np.eye(4), BATCH,
                        "latent" if case == "latent" else "mu", 8)
    sg.opt_sche_initialization()
    if case == "all_on":
        torch.manual_seed(17)          # u0 / v0 of the power iteration come from the CPU default generator
        spectral.spectral_norm(sg.D)
        sg.enable_grad_guard(max_norm=1.0)
        sg.enable_ema()
        sg.enable_diffaugment(seed=9)
        sg.enable_r1(gamma=10, every=2)
    return sg


def _digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _launch_counts(lib):
    from srgan_amd import _lib
    out = {}
    for kid in range(lib.srgan_prof_num_kernels()):
        ms, n, fl = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double()
        _lib.check(lib.srgan_prof_collect(kid, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)), "prof_collect")
        if n.value:
            out[lib.srgan_prof_kernel_name(kid).decode()] = int(n.value)
    return out


def run_case(case, graph=False):
    """-> (float32 matrix [steps, 3 returned losses + sorted loss_terms], meta): meta = {"digests": {tensor name: sha256},
    "r1_stats", "grad_guard_stats" (None where off), "launches": {kernel: count} of the last eager step (None in graph mode, where
    the launch timer is off, and for the cases that do not record it)}."""
    from srgan_amd import _lib, spectral
    k, steps = CASES[case]
    sg = make_trainer(case)
    if graph:
        sg.enable_graph()
    count = case in WITH_LAUNCH_COUNTS and not graph
    lib = _lib.load()
    torch.manual_seed(FIRST_SEED)      # the step's noise comes from the global CPU generator (tests/test_graph_gpu.py::_steps)
    rows, launches = [], None
    for s in range(steps):
        x, label = otrainer.synthetic_batch(BATCH, SIZE, 4, seed=FIRST_SEED + s)
        if count and s == steps - 1:
            torch.cuda.synchronize()
            lib.srgan_prof_enable(1)
        res = sg.train(x.cuda(), {"source": label["source"].cuda(), "target": label["target"]})
        if count and s == steps - 1:
            torch.cuda.synchronize()
            lib.srgan_prof_enable(0)
            launches = _launch_counts(lib)
        rows.append([float(v) for v in res] + [float(sg.loss_terms[t]) for t in sorted(sg.loss_terms)])
    if graph:
        assert sg.graph_active
    digests = {}
    nets = [("G", sg.G), ("D", sg.D), ("E", sg.E)]
    if case == "all_on":
        nets += [("G_ema", sg.G_ema), ("E_ema", sg.E_ema)]
    for name, net in nets:
        for key, v in net.state_dict().items():
            digests[f"{name}.{key}"] = _digest(v)
    for name, opt in (("optG", sg.optG), ("optD", sg.optD), ("optE", sg.optE)):
        for i, p in enumerate(q for g in opt.param_groups for q in g["params"]):
            st = opt.state.get(p) or {}
            for mom in ("exp_avg", "exp_avg_sq"):
                if mom in st:
                    digests[f"{name}.{i}.{mom}"] = _digest(st[mom])
    if case == "all_on":
        sig = spectral.sigmas(sg.D)
        digests["D.sigma"] = hashlib.sha256(np.array([sig[n] for n in sorted(sig)], dtype=np.float64).tobytes()).hexdigest()
    meta = {"digests": digests, "launches": launches,
            "r1_stats": sg.r1_stats() if case == "all_on" else None,
            "grad_guard_stats": sg.grad_guard_stats() if case == "all_on" else None}
    return np.array(rows, dtype=np.float32), json.loads(json.dumps(meta))
