"""Shared by tests/test_criteria_gpu.py and tests/golden/make_golden_criteria.py: the criterion pairs, the float64 PyTorch-CPU
references of the fused loss kernels, the error bounds and the trainer runs (each made once per session and left unchanged)."""
import functools

import numpy as np
import torch
import torch.nn as nn

ULP = 2.0 ** -24          # half a unit in the last place of a float32 in [1, 2)
RTOL = 1e-5               # a few ulp per expf / log1pf / division, <= 16 serial + 8 tree additions per value; a wrong formula is >= 1e-3

PAIRS = {"bce": (nn.BCEWithLogitsLoss, nn.BCELoss), "bcelogits_mse": (nn.BCEWithLogitsLoss, nn.MSELoss),
         "mse_bce": (nn.MSELoss, nn.BCELoss), "mse": (nn.MSELoss, nn.MSELoss)}

# seeds of oracle.params.fill for the networks of the SingleGAN fixtures (tests/golden/make_golden.py::run_singlegan)
SG_FILL = {"G": 20, "D0": 21, "D1": 22, "E": 25}
SG_BASE = {"class": 0.0, "cycle": 5.0, "idt": 5.0, "reg": 0.5, "idt_reg": 0.0, "KL": 0.1, "batch_KL": 0.0, "corr_enc": 0.0, "hist": 0.0}


def criteria(pair):
    gan, cls = PAIRS[pair]
    return [gan(), cls()]


def load_singlegan_params(gold):
    """{"G.<key>": float32 array, ...} of singlegan_T_b8_k1_bce.npz, which stores every parameter as its distance from the
    deterministic fill in float32 bit patterns (int32: lossless, and small numbers compress)."""
    from oracle import params as oparams
    out = {}
    for full in gold.files:
        if "_ulps." not in full:
            continue
        name, key = full.split("_ulps.", 1)
        fill = oparams.fill_array(key, tuple(gold[full].shape), SG_FILL[name]).astype(np.float32)
        out[f"{name}.{key}"] = (fill.view(np.int32) + gold[full]).view(np.float32)
    return out


# ---- bounds -------------------------------------------------------------------------------------------------------------------
def check_value(got, ref, what):
    got, ref = (float(v.detach()) if torch.is_tensor(v) else float(v) for v in (got, ref))
    assert np.isfinite(got), (what, got)
    print(f"{what}: value {got:.9g} ref {ref:.9g} rel {abs(got - ref) / max(abs(ref), 1e-300):.3e}")
    assert abs(got - ref) <= RTOL * abs(ref), (what, got, ref)


def check_grad(got, ref, floor, what):
    """|got - ref| <= 1e-5 |ref| + floor, element by element (floor: a few ulp of the gradient's scale weight / n)."""
    got = got.detach().double().cpu().flatten()
    ref = ref.detach().double().cpu().flatten()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    if got.numel() == 0:
        return
    excess = (got - ref).abs() - (RTOL * ref.abs() + floor)
    worst = int(excess.argmax())
    print(f"{what}: worst element got {float(got[worst]):.9g} ref {float(ref[worst]):.9g} floor {floor:.3e} "
          f"max err / floor {float((got - ref).abs().max()) / max(floor, 1e-300):.3f}")
    assert float(excess.max()) <= 0.0, (what, float(got[worst]), float(ref[worst]), floor)


# ---- float64 references: PyTorch-CPU's own criteria ---------------------------------------------------------------------------
def ref_gan(kind, o, target, weight):
    """weight * criterion(o, full_like(o, target)) in float64 -> (value, d value / d o)."""
    x = o.detach().double().cpu().requires_grad_(True)
    crit = nn.BCEWithLogitsLoss() if kind else nn.MSELoss()
    v = weight * crit(x, torch.full_like(x, target))
    v.backward()
    return v.detach(), x.grad


def ref_class(kind, z, label, weight, dtype=torch.float64):
    """weight * criterion(softmax(z), onehot(label)) -> (value, softmax, d value / d z)."""
    x = z.detach().to(dtype).cpu().requires_grad_(True)
    q = torch.softmax(x, 1)
    y = torch.nn.functional.one_hot(label.cpu().long(), x.shape[1]).to(dtype)
    crit = nn.BCELoss() if kind else nn.MSELoss()
    v = weight * crit(q, y)
    v.backward()
    return v.detach(), q.detach(), x.grad


# ---- trainer runs ---------------------------------------------------------------------------------------------------------------
def make_trainer(pair, k=2, batch=4, nets=None, ref_label=None):
    from oracle import trainer as otrainer
    from srgan_amd.trainer import SRGAN_training
    from tests.common import build_hip_nets
    G, D, E = nets if nets is not None else build_hip_nets("T")
    sg = SRGAN_training([G, D, E], [None, None, None], criteria(pair) if isinstance(pair, str) else pair,
                        dict(otrainer.DEFAULT_LBD), k, "cuda", np.eye(4) if ref_label is None else ref_label, batch, "mu", 8)
    sg.opt_sche_initialization()
    return sg


def train_steps(sg, steps, batch=4, graph_flags=None):
    from oracle import trainer as otrainer
    traj = []
    for s in range(steps):
        x, label = otrainer.synthetic_batch(batch, 128, 4, seed=100 + s)
        out = sg.train(x.cuda(), {"source": label["source"].cuda(), "target": label["target"]})
        traj.append([float(v) for v in out])
        if graph_flags is not None:
            graph_flags.append(bool(sg.graph_active))
    return np.array(traj)


@functools.lru_cache(maxsize=None)
def tier_t_run(pair, steps=3, dtype="fp32", graph=False):
    """The run of tests/golden/make_golden_criteria.py::run_train on the HIP path (tier T, batch 4, k 2, seed 0), once per
    session -> (trainer, losses[steps][3], graph_active after each step)."""
    from srgan_amd import ops
    ops.set_compute_dtype(dtype)
    try:
        from tests.common import build_hip_nets
        nets = build_hip_nets("T")         # (before the seeding: the constructors draw their default initialisation)
        torch.manual_seed(0)
        np.random.seed(0)
        sg = make_trainer(pair, nets=nets)
        if graph:
            sg.enable_graph()
        flags = []
        traj = train_steps(sg, steps, graph_flags=flags)
    finally:
        ops.set_compute_dtype("fp32")
    traj.setflags(write=False)
    return sg, traj, tuple(flags)
