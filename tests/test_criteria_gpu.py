"""GPU: nn.BCEWithLogitsLoss / nn.BCELoss on the fused loss kernels (csrc/losses.hip, SRGAN_CRIT_BCE) -- every kernel against
PyTorch-CPU's own criteria in float64 on the same inputs, the MSE kinds bit for bit against the entry points they replace, and
the trainer against trajectories of the reference run with these criteria (tests/golden/make_golden_criteria.py).

Bounds (tests/criteria_common.py): a value within 1e-5 relative (each term carries a few ulp of expf / log1pf, the sums are
<= 16 serial + 8 tree additions; a wrong formula is off by >= 1e-3); a gradient element within 1e-5 |ref| + 4 * 2^-24 * scale,
scale = weight / n being the size of the largest gradient element (sigmoid(x) - t and the softmax Jacobian's terms are
differences of numbers <= 1, each rounded to 2^-24)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.common import close, close_params
from tests.criteria_common import (RTOL, SG_BASE, ULP, check_grad, check_value, load_singlegan_params, make_trainer, ref_class,
                                   ref_gan, tier_t_run, train_steps)

pytestmark = pytest.mark.gpu

MSE, BCE = 0, 1
FIXED_LOGITS = [-120.0, -88.0, -20.0, 0.0, 1e-3, 20.0, 88.0, 120.0]


@pytest.fixture(scope="module")
def ops():
    from srgan_amd import ops as hops
    return hops


def _logits(*shape, seed):
    """N(0, 2): standard deviation 2 (logit gaps up to ~12 in the larger cases)."""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * 2.0


# ---- 1. crit_const ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1.0, 0.0, 0.9])
@pytest.mark.parametrize("n", [1, 9, 196, 256, 257, "fixed"])
def test_crit_const_bce_vs_float64(ops, n, t):
    x = torch.tensor(FIXED_LOGITS) if n == "fixed" else _logits(n, seed=n)
    w = 0.7
    xd = x.cuda().requires_grad_(True)
    v = ops.crit_const(xd, t, w, BCE)
    v.backward()
    ref_v, ref_g = ref_gan(BCE, x, t, w)
    check_value(v, ref_v, f"crit_const n={n} t={t}")
    check_grad(xd.grad, ref_g, 4 * ULP * w / x.numel(), f"crit_const d_o n={n} t={t}")


@pytest.mark.parametrize("t", [1.0, 0.0, 0.9])
def test_get_loss_D_bce_two_scales_vs_float64(ops, t):
    """4*7*7 + 4*3*3 as two calls: the discriminator's two maps through losses.get_loss_D (mean over the scales)."""
    from srgan_amd import losses
    o = [_logits(4, 1, 7, 7, seed=1), _logits(4, 1, 3, 3, seed=2)]
    od = [a.cuda().requires_grad_(True) for a in o]
    v = losses.get_loss_D(od, t, nn.BCEWithLogitsLoss())
    v.backward()
    refs = [ref_gan(BCE, a, t, 0.5) for a in o]
    check_value(v, sum(r[0] for r in refs), f"get_loss_D t={t}")
    for a, (_, g) in zip(od, refs):
        check_grad(a.grad, g, 4 * ULP * 0.5 / a.numel(), f"get_loss_D d_o {tuple(a.shape)} t={t}")


# ---- 2. softmax_crit -------------------------------------------------------------------------------------------------------------
def _check_softmax_crit(ops, z, lab, w, what, dtype=torch.float64):
    zd = z.cuda().requires_grad_(True)
    v, q = ops.softmax_crit(zd, lab.cuda(), w, BCE)
    v.backward()
    ref_v, ref_q, ref_g = ref_class(BCE, z, lab, w, dtype)
    check_value(v, ref_v, what)
    assert torch.isfinite(q).all()
    np.testing.assert_allclose(q.detach().cpu().double().numpy(), ref_q.double().numpy(), rtol=RTOL, atol=1e-37, err_msg=what + " q")
    check_grad(zd.grad, ref_g, 4 * ULP * w / z.numel(), what + " dz")
    return v, zd.grad, ref_v, ref_g


@pytest.mark.parametrize("B,nc", [(1, 2), (4, 4), (7, 4), (64, 4), (300, 4), (5, 16)])
def test_softmax_crit_bce_vs_float64(ops, B, nc):
    z = _logits(B, nc, seed=10 * B + nc)
    for off in range(nc):                                    # every class used as a label
        lab = (torch.arange(B) + off) % nc
        _check_softmax_crit(ops, z, lab, 0.7, f"softmax_crit B={B} nc={nc} off={off}")


def test_softmax_crit_bce_saturated_rows_vs_pytorch_fp32(ops):
    """Logit gaps of exactly 120 and 130: exp(-120) is 0 in float32, q is exactly 0 / 1.  nn.BCELoss's -100 clamp makes each
    saturated element with the wrong target cost 100 and its 1e-12 floor makes the gradient finite -- through the softmax
    Jacobian it is all zeros.  Against PyTorch-CPU float32 softmax -> BCELoss (in float64 q is not 0 / 1 at these gaps)."""
    z = torch.tensor([[0.0, 120.0], [0.0, 120.0], [130.0, 0.0], [130.0, 0.0], [-5.0, 125.0]])
    lab = torch.tensor([0, 1, 0, 1, 0])
    v, dz, ref_v, ref_g = _check_softmax_crit(ops, z, lab, 1.0, "saturated nc=2", torch.float32)
    assert float(ref_v) == pytest.approx((200.0 + 0.0 + 0.0 + 200.0 + 200.0) / 10.0)      # 100 per saturated element
    assert not ref_g.any() and not dz.any()
    z4 = torch.tensor([[0.0, 120.0, 0.0, 0.0], [130.0, 0.0, 0.0, 0.0], [1.0, 2.0, 3.0, 133.0]])
    for lab4 in ([1, 1, 3], [0, 0, 0], [2, 3, 1]):
        v, dz, ref_v, ref_g = _check_softmax_crit(ops, z4, torch.tensor(lab4), 2.5, f"saturated nc=4 {lab4}", torch.float32)
        assert not ref_g.any() and not dz.any()


def test_softmax_crit_bce_tiny_probabilities_vs_float64(ops):
    """Logit gaps of 60: q = e^-60 is tiny but normal, 1 - q rounds to 1 (in float32 and in float64), so the large class is a
    saturated element for nn.BCELoss while the small one is not; mixed with ordinary rows."""
    z = _logits(8, 4, seed=3)
    z[1] = torch.tensor([0.0, 60.0, 0.0, 0.0])
    z[4] = torch.tensor([60.0, 0.0, 60.0, 0.0])
    z[6] = torch.tensor([-30.0, -30.0, 30.0, -30.0])
    for off in range(4):
        _check_softmax_crit(ops, z, (torch.arange(8) + off) % 4, 0.7, f"gap 60 off={off}")
    z2 = torch.tensor([[0.0, 60.0], [60.0, 0.0]])
    for lab in ([0, 0], [1, 1]):
        _check_softmax_crit(ops, z2, torch.tensor(lab), 1.0, f"gap 60 nc=2 {lab}")


# ---- 3. crit_pair ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 1200])
def test_crit_pair_bce_vs_float64(ops, n):
    g = torch.Generator().manual_seed(n)
    a = torch.rand(n, generator=g)
    a[:8] = torch.tensor([0.0, 1.0, 0.0, 1.0, 1e-8, 1.0 - 2.0 ** -24, 0.5, 1e-30])
    b = (torch.rand(n, generator=g) < 0.5).float()
    b[:4] = torch.tensor([0.0, 1.0, 1.0, 0.0])               # exact 0 / 1 against the right and the wrong target
    w = 0.7
    ad = a.view(-1, 4).cuda().requires_grad_(True)
    v = ops.crit_pair(ad, b.view(-1, 4).cuda(), w, BCE)
    v.backward()
    x = a.double().requires_grad_(True)
    ref_v = w * nn.BCELoss()(x, b.double())
    ref_v.backward()
    check_value(v, ref_v, f"crit_pair n={n}")
    check_grad(ad.grad, x.grad, 4 * ULP * w / n, f"crit_pair da n={n}")
    from srgan_amd._lib import SrganHipError
    with pytest.raises(SrganHipError, match="targets"):
        ops.crit_pair(a.cuda(), b.cuda().requires_grad_(True), w, BCE)


def test_get_domainloss_D_bce_vs_float64(ops):
    from srgan_amd import losses
    z = [_logits(4, 4, seed=5), _logits(4, 4, seed=6)]
    lab = torch.tensor([0, 3, 1, 2])
    qd = [torch.softmax(a, 1).cuda().requires_grad_(True) for a in z]
    v = losses.get_domainloss_D(qd, torch.eye(4)[lab].cuda(), nn.BCELoss())
    v.backward()
    ref, grads = 0.0, []
    for a in qd:
        x = a.detach().cpu().double().requires_grad_(True)
        r = 0.5 * nn.BCELoss()(x, torch.eye(4).double()[lab])
        r.backward()
        ref, grads = ref + r.detach(), grads + [x.grad]
    check_value(v, ref, "get_domainloss_D")
    for a, g in zip(qd, grads):
        check_grad(a.grad, g, 4 * ULP * 0.5 / 16, "get_domainloss_D dq")


# ---- 4. d_losses -----------------------------------------------------------------------------------------------------------------
def _d_inputs(scales, rows):
    maps = [_logits(rows, 1, 7, 7, seed=40 + rows), _logits(rows, 1, 3, 3, seed=50 + rows)][:scales]
    logits = [_logits(rows, 4, seed=60 + rows), _logits(rows, 4, seed=70 + rows)][:scales]
    return maps, logits, (torch.arange(rows) * 3 + 1) % 4


@pytest.mark.parametrize("rows,split", [(2, "none"), (2, "half"), (2, "all"), (8, "none"), (8, "half"), (8, "all")])
@pytest.mark.parametrize("scales", [1, 2])
@pytest.mark.parametrize("gk,ck", [(MSE, MSE), (MSE, BCE), (BCE, MSE), (BCE, BCE)])
def test_d_losses_kinds_vs_float64_composition(ops, gk, ck, scales, rows, split):
    """vals, every d_o and every dz of the one-launch kernel against criterion(first rows, t_first) + w_class * class loss +
    criterion(rest, t_rest), each the mean over the scales of PyTorch-CPU's float64 criterion.  dz floors: 4 * 2^-24 * scale
    for the BCE class kind (as softmax_crit); (nc + 4) * 2^-24 * scale for the MSE kind, whose Jacobian q (dq - sum q dq) is
    nc + 3 rounded operations on numbers <= scale = 2 w / (rows_first nc)."""
    rows_first = {"none": 0, "half": rows // 2, "all": rows}[split]
    maps, logits, lab = _d_inputs(scales, rows)
    if rows_first == 0:
        logits = []                                          # no class head
    ws = 1.0 / scales
    t_first, t_rest = 1.0, 0.0
    for w_class in (0.0, 1.0, 2.5):
        od = [m.cuda().requires_grad_(True) for m in maps]
        zd = [z.cuda().requires_grad_(True) for z in logits]
        total, parts = ops.d_losses(od, zd, lab[:rows].cuda() if zd else None, rows_first, t_first, t_rest, w_class, gk, ck)
        total.backward()
        what = f"d_losses kinds=({gk},{ck}) S={scales} rows={rows} first={rows_first} w={w_class}"
        ref = [0.0, 0.0, 0.0]
        for s in range(scales):
            n1, n2 = rows_first * maps[s][0].numel(), (rows - rows_first) * maps[s][0].numel()
            if n1:                                           # (one floor per part: its own n)
                v, g = ref_gan(gk, maps[s][:rows_first], t_first, ws)
                ref[0] = ref[0] + v
                check_grad(od[s].grad[:rows_first], g, 4 * ULP * ws / n1, what + f" d_o[{s}] first")
            if n2:
                v, g = ref_gan(gk, maps[s][rows_first:], t_rest, ws)
                ref[2] = ref[2] + v
                check_grad(od[s].grad[rows_first:], g, 4 * ULP * ws / n2, what + f" d_o[{s}] rest")
            if zd:
                v, _, gz = ref_class(ck, logits[s][:rows_first], lab[:rows_first], ws)
                ref[1] = ref[1] + v
                scale = ws * w_class / (rows_first * 4)
                floor = 4 * ULP * scale if ck == BCE else (4 + 4) * ULP * 2 * scale
                check_grad(zd[s].grad[:rows_first], gz * w_class, floor, what + f" dz[{s}]")
                assert not zd[s].grad[rows_first:].any(), what                  # rows without a class loss: exactly zero
        for i, name in enumerate(("first", "class", "rest")):
            if float(ref[i]) == 0.0:
                assert float(parts[i]) == 0.0, (what, name)
            else:
                check_value(parts[i], ref[i], f"{what} {name}")
        check_value(total, ref[0] + w_class * ref[1] + ref[2], what + " total")


@pytest.mark.parametrize("rows_first", [0, 4, 8])
def test_mse_kinds_are_the_previous_entry_points_bit_for_bit(ops, rows_first):
    """Kinds (MSE, MSE) of d_losses against the ``srgan_d_losses`` entry point itself, and crit_const / softmax_crit / crit_pair
    with kind MSE against mse_const / softmax_mse / mse_pair: the same bits, values and gradients."""
    from srgan_amd import _lib
    lib = _lib.load()
    maps, logits, lab = _d_inputs(2, 8)
    if rows_first == 0:
        logits = []
    od = [m.cuda().requires_grad_(True) for m in maps]
    zd = [z.cuda().requires_grad_(True) for z in logits]
    labd = lab.cuda()
    total, parts = ops.d_losses(od, zd, labd if zd else None, rows_first, 1.0, 0.0, 2.5, MSE, MSE)
    total.backward()
    d_o = [torch.empty_like(m) for m in od]
    dz = [torch.empty_like(z) for z in zd]
    vals = torch.empty(4, device="cuda")
    arr = ctypes.c_void_p * 2
    ptrs = lambda ts: arr(*[t.data_ptr() for t in ts]) if ts else None      # noqa: E731
    per = (ctypes.c_longlong * 2)(49, 9)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.srgan_d_losses(ptrs([m.detach() for m in od]), per, ptrs([z.detach() for z in zd]), 2, 8, rows_first, 4 if zd else 0,
                                  labd.data_ptr() if zd else None, 1.0, 0.0, 2.5, vals.data_ptr(), ptrs(d_o), ptrs(dz), stream),
               "d_losses")
    assert torch.equal(vals[:3], parts) and torch.equal(vals[3], total.detach())
    for a, b in zip(od + zd, d_o + dz):
        assert torch.equal(a.grad, b)

    def both(f_new, f_old, *inputs):
        outs = []
        for f in (f_new, f_old):
            leaves = [t.clone().requires_grad_(True) for t in inputs]
            v = f(*leaves)
            v = v[0] if isinstance(v, tuple) else v
            v.backward()
            outs.append([v.detach()] + [t.grad for t in leaves])
        for a, b in zip(*outs):
            assert torch.equal(a, b)

    x = od[0].detach()
    both(lambda o: ops.crit_const(o, 0.9, 0.5, MSE), lambda o: ops.mse_const(o, 0.9, 0.5), x)
    z = _logits(8, 4, seed=60 + 8).cuda()
    both(lambda t: ops.softmax_crit(t, labd, 0.5, MSE), lambda t: ops.softmax_mse(t, labd, 0.5), z)
    q, y = torch.softmax(z, 1), torch.eye(4, device="cuda")[labd]
    both(lambda a, b: ops.crit_pair(a, b, 0.5, MSE), lambda a, b: ops.mse_pair(a, b, 0.5), q, y)


# ---- 5. trajectories against the reference ---------------------------------------------------------------------------------------
def test_bce_trajectory_vs_reference_tier_T(golden_dir):
    gold = np.load(os.path.join(golden_dir, "train_T_b4_k2_bce.npz"))
    sg, traj, _ = tier_t_run("bce")
    print("bce/bce losses", traj.tolist(), "rel", (np.abs(traj - gold["losses"]) / np.abs(gold["losses"])).max())
    close(sg.hi.target, gold["hist_target"], 1e-5, what="hist target")
    np.testing.assert_allclose(traj, gold["losses"], rtol=1e-3)
    for net_name, net, n_opt in (("G", sg.G, 2 * 3), ("D", sg.D, 2 * 3), ("E", sg.E, 3)):
        for key, v in net.state_dict().items():
            close_params(v, gold[f"{net_name}.{key}"], 1e-4, n_opt, what=f"{net_name}.{key}")
    # the criterion really reached the kernels: the discriminator loss is not the LSGAN run's
    mse = np.load(os.path.join(golden_dir, "train_T_b4_k2.npz"))["losses"]
    assert np.abs(traj[:, 1] - mse[:, 1]).min() > 1e-2


@pytest.mark.parametrize("pair", ["bcelogits_mse", "mse_bce"])
def test_mixed_criteria_trajectory_vs_reference_tier_T(golden_dir, pair):
    gold = np.load(os.path.join(golden_dir, "train_T_b4_k2_mixed.npz"))
    _, traj, _ = tier_t_run(pair)
    print(pair, "losses", traj.tolist(), "rel", (np.abs(traj - gold[pair]) / np.abs(gold[pair])).max())
    np.testing.assert_allclose(traj, gold[pair], rtol=1e-3)


def test_singlegan_bce_trajectory_vs_reference(golden_dir):
    from oracle import params, trainer as otrainer
    from srgan_amd import model
    from srgan_amd.trainer import SingleGAN_training
    gold = np.load(os.path.join(golden_dir, "singlegan_T_b8_k1_bce.npz"))
    gold_params = load_singlegan_params(gold)
    G = model.SingleGenerator(3, 4, 2, 2, 1, "instance", num_con=10)
    G.load_state_dict(params.fill(params.generator_spec(3, 4, 2, 2, 1, 10), 20))
    D = []
    for i in range(2):
        d = model.SingleDiscriminator_original_multi(3, 4, 2, 4, "instance")
        d.load_state_dict(params.fill(params.discriminator_original_spec(3, 4, 2, 4), 21 + i))
        D.append(d.cuda())
    E = model.Encoder_original(3, 8, 4, 4, "instance", 2, "cuda")
    E.load_state_dict(params.fill(params.encoder_original_spec(3, 8, 4, 4, 2), 25))
    G.cuda(), E.cuda()
    torch.manual_seed(0)
    np.random.seed(0)
    k, steps = 1, 3
    sg = SingleGAN_training([G, D, E], [None, None, None], [nn.BCEWithLogitsLoss(), nn.BCELoss()], dict(SG_BASE), k, "cuda", np.eye(2),
                            8, (0, 1), 8, "latent", False)
    sg.opt_sche_initialization()
    traj = []
    for s in range(steps):
        x, label = otrainer.synthetic_batch(8, 64, 2, seed=200 + s)
        out = sg.train(x.cuda(), {"source": label["source"].cuda(), "target": label["target"]})
        traj.append([float(v) for v in out])
    np.testing.assert_allclose(np.array(traj), gold["losses"], rtol=1e-3)
    for name_, net, n_opt in (("G", sg.G, 2 * steps), ("D0", sg.D[0], k * steps), ("D1", sg.D[1], k * steps), ("E", sg.E, steps)):
        for key, v in net.state_dict().items():
            close_params(v, gold_params[f"{name_}.{key}"], 1e-4, n_opt, what=f"{name_}.{key}")


# ---- 6. graph --------------------------------------------------------------------------------------------------------------------
def test_bce_graph_replay_is_bit_identical_to_eager():
    eager, ref, _ = tier_t_run("bce", 4)
    sg, got, active = tier_t_run.__wrapped__("bce", 4, "fp32", True)
    assert all(active[2:]) and not active[0], active          # replaying from the third step at the latest
    np.testing.assert_array_equal(got, ref)
    ref_state = {f"{n}.{k}": v for n, net in (("G", eager.G), ("D", eager.D), ("E", eager.E)) for k, v in net.state_dict().items()}
    for n, net in (("G", sg.G), ("D", sg.D), ("E", sg.E)):
        for k, v in net.state_dict().items():
            assert torch.equal(v, ref_state[f"{n}.{k}"]), (n, k)
    sg.disable_graph()


# ---- 7. generic path -------------------------------------------------------------------------------------------------------------
class _PlainD(nn.Module):
    """A discriminator without ``forward_logits``: the trainer leaves the fused paths and goes through the criteria's own entry
    points (get_loss_D -> crit_const, get_domainloss_D -> crit_pair on the probabilities)."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return self.inner(x)


def test_bce_generic_path_agrees_with_the_fused_path():
    from tests.common import build_hip_nets
    _, fused, _ = tier_t_run("bce")
    G, D, E = build_hip_nets("T")
    torch.manual_seed(0)
    np.random.seed(0)
    sg = make_trainer("bce", nets=(G, _PlainD(D), E))
    assert not sg._fused_paths()
    got = train_steps(sg, 1)
    print("generic", got.tolist(), "fused", fused[:1].tolist())
    np.testing.assert_allclose(got[0], fused[0], rtol=1e-5)


def test_unsupported_gan_criterion_raises_from_train():
    from oracle import trainer as otrainer
    sg = make_trainer([nn.L1Loss(), nn.MSELoss()])
    x, label = otrainer.synthetic_batch(4, 128, 4, seed=100)
    with pytest.raises(NotImplementedError, match="nn.MSELoss"):
        sg.train(x.cuda(), {"source": label["source"].cuda(), "target": label["target"]})


# ---- 8. bf16 mode ----------------------------------------------------------------------------------------------------------------
# largest relative loss deviation of the 3-step BCE / BCE trajectory in the bf16 mode from the reference's fp32 run, x 1.5
# (measured on the MI355X: 1.42e-4, errD of the second step)
BF16_TRAJ_BOUND_BCE = 2.15e-4


def test_bce_trajectory_bf16_mode_tracks_the_reference(golden_dir):
    """The loss kernels read fp32 heads in the bf16 mode too; the deviation is bf16 rounding of the conv operands (at tier-T
    widths the layers with >= 32 channels)."""
    gold = np.load(os.path.join(golden_dir, "train_T_b4_k2_bce.npz"))
    _, traj, _ = tier_t_run("bce", 3, "bf16")
    assert np.isfinite(traj).all()
    rel = np.abs(traj - gold["losses"]) / np.abs(gold["losses"])
    print("bf16 bce/bce: largest relative loss deviation", float(rel.max()), rel.max(1).tolist())
    assert float(rel.max()) <= BF16_TRAJ_BOUND_BCE, (float(rel.max()), rel.max(1))
