"""GPU: norm_type="batch" -- nn.BatchNorm2d / CBBNorm2d on the HIP path (csrc/norm_batch.hip, ops.batch_norm_act /
ops.cbb_norm_act, model.BatchNorm2d / CBBNorm2d) against a float64 torch CPU restatement, the reference-generated goldens
(tests/golden/modules_batch_T.npz, train_T_b4_k2_batch.npz, inference_batch_T.npz) and itself (determinism, graph replay);
full-width G / E in fp32 and the bf16 mode inside the packed-weight scope, where only the batch-norm gates keep the fused
instance-norm paths off."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import trainer as otrainer
from tests.batch_common import batch_fill, module_inputs, objective_E, objective_G
from tests.common import close, close_grad, close_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from srgan_amd import ops
    assert torch.cuda.is_available()
    return ops


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def fp32(t):
    """float64 values the fp32 kernels see exactly (the restatement then differs by the kernels' arithmetic only)"""
    return t.float().double()


def act_ref(z, act, slope):
    return {0: z, 1: torch.relu(z), 2: F.leaky_relu(z, slope)}[act]


def ref_batch_norm(x, w, b, rm, rv, nbt, training, momentum, act, slope, cbb=False, scale=None, shift=None, res=None):
    """float64 restatement of nn.BatchNorm2d / the reference's _CBBNorm.forward (model.py:118-140) + activation (+ residual);
    updates rm / rv / nbt (float64 / int copies) as torch does."""
    f = 0.0
    if training and rm is not None:
        nbt[0] += 1
        f = 1.0 / nbt[0] if momentum is None else momentum
    out = F.batch_norm(x, rm, rv, None if cbb else w, None if cbb else b, training or rm is None, f, 1e-5)
    if cbb:
        out = (out - out.mean((2, 3), keepdim=True)) * scale[:, :, None, None] + shift[:, :, None, None]
    y = act_ref(out, act, slope)
    return y + res if res is not None else y


def run_case(ops, shape, cbb, act, training=True, momentum=0.1, track=True, calls=1, offset=0.0, seed=1, with_res=False):
    n, c, h, w = shape
    slope = 0.2
    x = fp32(rnd(*shape, seed=seed) * 1.5 + 0.3 + offset).requires_grad_(True)
    gam = fp32(1 + 0.25 * rnd(c, seed=seed + 1)).requires_grad_(True)
    bet = fp32(0.1 * rnd(c, seed=seed + 2)).requires_grad_(True)
    sc = fp32(1 + 0.25 * rnd(n, c, seed=seed + 3)).requires_grad_(True)
    sh = fp32(0.3 * rnd(n, c, seed=seed + 4)).requires_grad_(True)
    res = fp32(rnd(*shape, seed=seed + 5)) if with_res else None
    gy = fp32(rnd(*shape, seed=seed + 6))
    rm = fp32(0.2 * rnd(c, seed=seed + 7)) if track else None
    rv = fp32(1 + 0.5 * rnd(c, seed=seed + 8).abs()) if track else None
    nbt = [3]
    dev = dict(device="cuda", dtype=torch.float32)
    rmd = rm.to(**dev) if track else None
    rvd = rv.to(**dev) if track else None
    nbtd = torch.tensor(3, dtype=torch.long, device="cuda") if track else None
    for i in range(calls):
        last = i == calls - 1
        xd = x.detach().to(**dev).requires_grad_(True)
        gd, bd = gam.detach().to(**dev).requires_grad_(True), bet.detach().to(**dev).requires_grad_(True)
        scd, shd = sc.detach().to(**dev).requires_grad_(True), sh.detach().to(**dev).requires_grad_(True)
        if cbb:
            y = ops.cbb_norm_act(xd, scd, shd, rmd, rvd, nbtd if (training and track) else None, training or not track, momentum,
                                 1e-5, act, slope, res.to(**dev) if with_res else None)
        else:
            y = ops.batch_norm_act(xd, gd, bd, rmd, rvd, nbtd if (training and track) else None, training or not track, momentum,
                                   1e-5, act, slope)
        yr = ref_batch_norm(x if last else x.detach(), gam, bet, rm, rv, nbt, training, momentum, act, slope, cbb, sc, sh, res)
    y.backward(gy.to(**dev))
    yr.backward(gy)
    close(y, yr, 2e-5, what="y")
    # over ~1e6 elements and more, an activation whose pre-activation lies within fp32 rounding of zero takes the other branch
    # here and there (a sparse, large difference of dx and of its channel's parameter gradient): common.close_grad tells these
    # from a broad error
    cmp = close_grad if n * h * w * c >= 1 << 18 and act else close
    cmp(xd.grad, x.grad, 1e-4, what="dx")
    if cbb:
        cmp(scd.grad, sc.grad, 1e-4, what="dscale")
        cmp(shd.grad, sh.grad, 1e-4, what="dshift")
    else:
        cmp(gd.grad, gam.grad, 1e-4, what="dgamma")
        cmp(bd.grad, bet.grad, 1e-4, what="dbeta")
    if track:
        close(rmd, rm, 1e-5, 1e-6, what="running_mean")
        close(rvd, rv, 1e-5, 1e-6, what="running_var")
        assert int(nbtd) == nbt[0]
    return [t for t in (y, xd.grad, gd.grad, bd.grad, scd.grad, shd.grad, rmd, rvd, nbtd) if t is not None]


def _net_shapes(H, B):
    """(shape, cbb, act) of every norm of tier-F G (CBB down / residual with ReLU, BN up with ReLU) and E (BN with LeakyReLU 0.2),
    and Encoder_original's CBB blocks (LeakyReLU 0.2)."""
    out = [((B, 64, H, H), True, 1), ((B, 128, H // 2, H // 2), True, 1), ((B, 256, H // 4, H // 4), True, 1),
           ((B, 128, H // 2, H // 2), False, 1), ((B, 64, H, H), False, 1)]
    he = (H + 2 - 7) // 2 + 1
    c = 64
    for _ in range(4):
        out += [((B, c, he, he), False, 2), ((B, c, he, he), True, 2)]
        c, he = 2 * c, he // 2
    return out


SHAPES = sorted(set(_net_shapes(128, 32) + _net_shapes(256, 16) + [((4, 4, 128, 128), True, 1), ((4, 8, 64, 64), False, 1),
                                                                    ((4, 16, 32, 32), True, 0), ((3, 64, 3, 3), False, 2),
                                                                    ((1, 8, 16, 16), True, 1), ((1, 4, 5, 7), False, 2)]))


@pytest.mark.parametrize("shape,cbb,act", SHAPES)
def test_ops_match_float64_restatement(ops, shape, cbb, act):
    run_case(ops, shape, cbb, act, with_res=cbb and act == 0)


@pytest.mark.parametrize("cbb", [False, True])
@pytest.mark.parametrize("momentum", [0.1, None])
@pytest.mark.parametrize("shape", [(4, 16, 32, 32), (32, 64, 64, 64)])
def test_running_buffers_after_three_calls(ops, cbb, momentum, shape):
    run_case(ops, shape, cbb, 1, momentum=momentum, calls=3)


@pytest.mark.parametrize("cbb", [False, True])
@pytest.mark.parametrize("shape", [(4, 16, 32, 32), (16, 128, 31, 31)])
def test_eval_mode_and_untracked(ops, cbb, shape):
    run_case(ops, shape, cbb, 2, training=False)                 # running statistics, buffers untouched
    run_case(ops, shape, cbb, 2, track=False)                    # batch statistics, no buffers
    run_case(ops, shape, cbb, 2, training=False, track=False)    # track_running_stats=False: batch statistics in eval too


@pytest.mark.parametrize("cbb", [False, True])
def test_offset_by_100_input(ops, cbb):
    """E[x^2] - E[x]^2 in fp32 over the batch would lose the variance of data offset by 100."""
    run_case(ops, (16, 64, 32, 32), cbb, 1, offset=100.0)
    run_case(ops, (2, 32, 128, 128), cbb, 1, offset=100.0, momentum=None, calls=2)


def test_one_value_per_channel_in_training_is_an_error(ops):
    x = torch.randn(1, 8, 1, 1, device="cuda")
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ops.batch_norm_act(x, None, None, None, None, None, True)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ops.cbb_norm_act(x, torch.ones(1, 8, device="cuda"), torch.zeros(1, 8, device="cuda"), None, None, None, True)
    rm, rv = torch.zeros(8, device="cuda"), torch.ones(8, device="cuda")
    y = ops.batch_norm_act(x, None, None, rm, rv, None, False)        # eval mode: fine
    close(y, x.cpu() / np.sqrt(1 + 1e-5), 1e-6)


def test_bad_channel_count_is_an_error(ops):
    from srgan_amd import _lib
    x = torch.randn(2, 6, 4, 4, device="cuda")
    with pytest.raises(_lib.SrganHipError, match="not a multiple of 4"):
        ops.batch_norm_act(x, None, None, None, None, None, True)
    with pytest.raises(_lib.SrganHipError, match="not a multiple of 4"):
        ops.cbb_norm_act(x, torch.ones(2, 6, device="cuda"), torch.zeros(2, 6, device="cuda"), None, None, None, True)


@pytest.mark.parametrize("training", [True, False])
def test_batch_norm_weight_read_at_backward_time(ops, training):
    """nn.BatchNorm2d's autograd holds the weight by reference: a backward through a graph recorded before an optimiser step (the
    reference's phase-2 backward through the kept target_image graph) uses the UPDATED weight.  The activation mask stays the
    forward's."""
    n, c, h, w = 4, 16, 16, 16
    x = fp32(rnd(n, c, h, w, seed=1) * 1.5 + 0.3).requires_grad_(True)
    gam = fp32(1 + 0.25 * rnd(c, seed=2)).requires_grad_(True)
    bet = fp32(0.1 * rnd(c, seed=3)).requires_grad_(True)
    rm, rv = fp32(0.2 * rnd(c, seed=4)), fp32(1 + 0.5 * rnd(c, seed=5).abs())
    gy = fp32(rnd(n, c, h, w, seed=6))
    dev = dict(device="cuda", dtype=torch.float32)
    xd, gd, bd = (t.detach().to(**dev).requires_grad_(True) for t in (x, gam, bet))
    y = ops.batch_norm_act(xd, gd, bd, rm.to(**dev), rv.to(**dev), None, training, 0.1, 1e-5, ops.ACT_RELU, 0.0)
    yr = torch.relu(F.batch_norm(x, rm.clone(), rv.clone(), gam, bet, training, 0.1, 1e-5))
    with torch.no_grad():                      # an optimiser step between forward and backward (through .data: no version bump)
        gam.data.mul_(1.5).add_(0.1)
        gd.data.mul_(1.5).add_(0.1)
    yr.backward(gy)
    y.backward(gy.to(**dev))
    close(y, yr.detach(), 2e-5, what="y")
    close(xd.grad, x.grad, 1e-4, what="dx")
    close(gd.grad, gam.grad, 1e-4, what="dgamma")
    close(bd.grad, bet.grad, 1e-4, what="dbeta")


@pytest.mark.parametrize("cbb", [False, True])
def test_deterministic(ops, cbb):
    """Bit-identical output, input and parameter gradients and running buffers from two identical call sequences."""
    outs = []
    for _ in range(2):
        torch.cuda.synchronize()
        outs.append(run_case(ops, (32, 64, 64, 64), cbb, 1, momentum=None, calls=2))
    assert len(outs[0]) == len(outs[1]) == 7
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)


# ---- modules against the reference (tests/golden/modules_batch_T.npz) ----------------------------------------------------------
def _hip_modules():
    from srgan_amd import model
    G = batch_fill(model.SingleGenerator(3, 4, 2, 2, 1, "batch", num_con=12), 0).cuda()
    E = batch_fill(model.Encoder(3, 8, 4, 4, "batch", 4, "cuda"), 2).cuda()
    Eo = batch_fill(model.Encoder_original(3, 8, 4, 4, "batch", 4, "cuda"), 3).cuda()
    return G, E, Eo


def _pool8(t):
    from srgan_amd import ops
    return F.avg_pool2d(ops.to_nchw(t.detach()).cpu(), 8)


def test_modules_vs_reference_golden(golden_dir):
    gold = np.load(os.path.join(golden_dir, "modules_batch_T.npz"))
    xs, c_g, c_e = module_inputs()
    G, E, Eo = _hip_modules()
    tol = 2e-4
    for name, net in (("G", G), ("E", E), ("Eo", Eo)):
        net.train()
        for i, x in enumerate(xs):
            net.zero_grad()
            xi = x.cuda().requires_grad_(True)
            if name == "G":
                y = net(xi, c_g.cuda())
                s = objective_G(y)
                close(_pool8(y), gold[f"G{i}_y_pool8"], tol, what=f"G{i} y")
            else:
                torch.manual_seed(3)
                res = net(xi) if name == "E" else net(xi, c_e.cuda())
                s = objective_E(res)
                close(res[1], gold[f"{name}{i}_mu"], tol, what=f"{name}{i} mu")
                close(res[2], gold[f"{name}{i}_logvar"], tol, what=f"{name}{i} logvar")
            s.backward()
            # (the generator's ReLUs: a mask flip against the reference's CPU arithmetic moves its channel through the batch
            # statistics -- common.close_grad; the encoders' LeakyReLU keeps the plain bound)
            cmp = (lambda a, b, what: close_grad(a, b, tol, what=what)) if name == "G" else \
                (lambda a, b, what: close(a, b, tol, 1e-6, what=what))
            cmp(_pool8(xi.grad), gold[f"{name}{i}_dx_pool8"], what=f"{name}{i} dx")
            for k, p in net.named_parameters():
                cmp(p.grad, gold[f"{name}{i}_grad.{k}"], what=f"{name}{i} grad {k}")
        for k, v in net.state_dict().items():
            if "running" in k or "num_batches" in k:
                if "num_batches" in k:
                    assert int(v) == int(gold[f"{name}_buf.{k}"]), k
                else:
                    close(v, gold[f"{name}_buf.{k}"], tol, 1e-6, what=f"{name} {k}")
        net.eval()
        with torch.no_grad():
            if name == "G":
                close(_pool8(net(xs[0].cuda(), c_g.cuda())), gold["G_eval_y_pool8"], tol, what="G eval")
            else:
                torch.manual_seed(3)
                res = net(xs[0].cuda()) if name == "E" else net(xs[0].cuda(), c_e.cuda())
                close(res[1], gold[f"{name}_eval_mu"], tol, what=f"{name} eval mu")
                close(res[2], gold[f"{name}_eval_logvar"], tol, what=f"{name} eval logvar")


# ---- full width, inside the packed-weight scope: the fused instance-norm paths would apply here -------------------------------
def _bn64(x, P, B, prefix):
    """nn.BatchNorm2d in training mode (batch statistics; B's running buffers updated as torch does)"""
    return F.batch_norm(x, B[prefix + ".running_mean"], B[prefix + ".running_var"], P[prefix + ".weight"], P[prefix + ".bias"],
                        True, 0.1, 1e-5)


def _cbb64(x, c, P, B, prefix):
    """the reference's _CBBNorm.forward (model.py:118-140) in training mode"""
    out = F.batch_norm(x, B[prefix + ".running_mean"], B[prefix + ".running_var"], None, None, True, 0.1, 1e-5)
    t = torch.tanh(F.linear(c, P[prefix + ".ConBias.0.weight"], P[prefix + ".ConBias.0.bias"]))
    g, b = P[prefix + ".weight"].view(1, -1, 1, 1), P[prefix + ".bias"].view(1, -1, 1, 1)
    return (out - out.mean((2, 3), keepdim=True) + t[:, :, None, None]) * g + b


def _generator64(P, B, x, c, n_res=6):
    """SingleGenerator(3, 64, 2, 2, n_res, "batch") in float64 (model.py:188-249)"""
    x = torch.relu(_cbb64(F.conv2d(x, P["down_convs.0.weight"], None, 1, 3), c, P, B, "down_cnorms.0"))
    for i in (1, 2):
        x = torch.relu(_cbb64(F.conv2d(x, P[f"down_convs.{i}.weight"], None, 2, 1), c, P, B, f"down_cnorms.{i}"))
    for j in range(n_res):
        h = torch.relu(_cbb64(F.conv2d(x, P[f"resBlocks.{j}.c1.weight"], None, 1, 1), c, P, B, f"resBlocks.{j}.cn1"))
        x = _cbb64(F.conv2d(h, P[f"resBlocks.{j}.c2.weight"], None, 1, 1), c, P, B, f"resBlocks.{j}.cn2") + x
    for i in (0, 1):
        x = torch.relu(_bn64(F.conv_transpose2d(x, P[f"up_convs.{i}.weight"], None, 2, 1), P, B, f"up_norms.{i}"))
    return torch.tanh(F.conv2d(x, P["up_convs.2.weight"], None, 1, 3))


def _encoder64(P, B, x):
    """Encoder(3, 8, 64, 4, "batch") in float64 (model.py:401-496): mu, logvar, class output"""
    from oracle import nets as onets
    h = F.conv2d(x, P["first_layer.weight"], P["first_layer.bias"], 2, 1)
    for b in range(4):
        h = onets._enc_block(P, b, h, lambda t, b=b: _bn64(t, P, B, f"layers.{b}.norm1"),
                             lambda t, b=b: _bn64(t, P, B, f"layers.{b}.norm2"))
    feat = F.leaky_relu(h, 0.2).mean(dim=(2, 3))
    return (F.linear(feat, P["fcmean.weight"], P["fcmean.bias"]), F.linear(feat, P["fcvar.weight"], P["fcvar.bias"]),
            F.linear(feat, P["fcclass.weight"], P["fcclass.bias"]))


def _full_width_nets():
    from srgan_amd import model
    G = batch_fill(model.SingleGenerator(3, 64, 2, 2, 6, "batch", num_con=12), 3)
    E = batch_fill(model.Encoder(3, 8, 64, 4, "batch", 4, "cuda"), 4)
    return G, E


def _hip_full_width(mode, x, c, w):
    """G and E forward + backward on the HIP path in compute mode `mode`, inside ops.pack_cache() (the trainer's scope); checks
    first that the fused instance-norm paths WOULD be taken at this geometry, so that only the batch-norm gates keep them off."""
    from srgan_amd import model, ops
    G, E = _full_width_nets()
    G.cuda()
    E.cuda()
    ops.set_compute_dtype(mode)
    try:
        with ops.pack_cache():
            if mode == "fp32" and x.shape[0] >= 8:   # the norm -> conv V-image path of the residual blocks (32 x 32 trunk)
                probe = ops.to_nhwc(torch.zeros(x.shape[0], 256, 32, 32, device="cuda"))
                assert ops.norm_act_conv_fusable(probe, G.resBlocks[0].c2.weight)
            elif mode == "bf16" and x.shape[0] >= 8:   # the 16-bit storage of the encoder blocks and the generator's down path
                n = x.shape[0]
                served = []
                for b, (ch, hw) in enumerate(((64, 62), (128, 31), (256, 15))):
                    blk, xe = E.layers[b], ops.to_nhwc(torch.zeros(n, ch, hw, hw, device="cuda"))
                    served.append(model._block_io16(xe, blk.conv1, blk.cmp[0]))      # (asked as for an instance-norm block)
                    assert not model._block_io16(xe, blk.conv1, blk.cmp[0], blk.norm1)
                probe = torch.empty((n, 64, 128, 128), device="meta")
                served.append(G.down_convs[1].s2_io_applicable(probe) and ops.norm_io_applicable(n, 128, 64, 64))
                assert any(served), served
            xg = x.cuda()
            y = G(xg, c.cuda())
            (y * w.cuda()).sum().backward()
            xe = x.cuda()
            _, mu, lv, cls, _ = E(xe)
            (mu.sum() + (lv ** 2).sum() + cls.sum()).backward()
        torch.cuda.synchronize()
    finally:
        ops.set_compute_dtype("fp32")
    return G, E, ops.to_nchw(y.detach()).cpu(), mu.detach().cpu(), lv.detach().cpu(), cls.detach().cpu()


@pytest.mark.parametrize("batch", [2, 8])
def test_full_width_batch_modules_vs_float64_restatement(batch):
    """G and E at full width, 128 x 128 (32 x 32 residual trunk), fp32 and the bf16 mode, against float64 restatements:
    outputs, every parameter gradient and running buffer (fp32); the bf16 mode within 1e-2 of fp32.  Batch 8: the smallest at
    which the residual blocks' F(4x4,3x3) layers -- and with them the instance-norm V-image path -- are chosen."""
    x = torch.rand(batch, 3, 128, 128, generator=torch.Generator().manual_seed(1)) * 2 - 1
    c = torch.randn(batch, 12, generator=torch.Generator().manual_seed(2))
    w = torch.randn(batch, 3, 128, 128, generator=torch.Generator().manual_seed(3))
    G0, E0 = _full_width_nets()
    PG = {k: v.detach().double().requires_grad_(True) for k, v in G0.named_parameters()}
    PE = {k: v.detach().double().requires_grad_(True) for k, v in E0.named_parameters()}
    BG = {k: v.detach().double().clone() for k, v in G0.named_buffers()}
    BE = {k: v.detach().double().clone() for k, v in E0.named_buffers()}
    yr = _generator64(PG, BG, x.double(), c.double())
    (yr * w.double()).sum().backward()
    mur, lvr, clsr = _encoder64(PE, BE, x.double())
    (mur.sum() + (lvr ** 2).sum() + clsr.sum()).backward()

    G, E, y, mu, lv, cls = _hip_full_width("fp32", x, c, w)
    close(y, yr.detach(), 2e-4, what="G out")
    for name, t, r in (("mu", mu, mur), ("logvar", lv, lvr), ("cls", cls, clsr)):
        close(t, r.detach(), 2e-4, what="E " + name)
    for net, P, B, tag in ((G, PG, BG, "G"), (E, PE, BE, "E")):
        for k, p in net.named_parameters():
            close_grad(p.grad, P[k].grad, 2e-4, what=f"{tag} grad {k}")
        for k, v in net.named_buffers():
            if k.endswith("num_batches_tracked"):
                assert int(v) == 1, (tag, k)
            else:
                close(v, B[k], 1e-4, 1e-6, what=f"{tag} {k}")

    # the bf16 mode: within 1e-2 of fp32 in relative L2; the largest element error no worse than twice what the bf16 mode costs
    # the instance-norm generator with the same weights and input
    _, _, y16, mu16, lv16, cls16 = _hip_full_width("bf16", x, c, w)
    yi, yi16 = (_instance_generator_out(G0, x, c, mode) for mode in ("fp32", "bf16"))
    max_i = float((yi16 - yi).abs().max()) / float(yi.abs().max())
    for name, a, b in (("G out", y16, y), ("E mu", mu16, mu), ("E logvar", lv16, lv), ("E cls", cls16, cls)):
        l2 = float((a - b).norm()) / max(float(b.norm()), 1e-30)
        mx = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
        print(f"bf16 vs fp32 {name}: rel L2 {l2:.3e}, max {mx:.3e} (instance-norm G max {max_i:.3e})")
        assert l2 <= 1e-2, (name, l2)
        assert name != "G out" or mx <= 2 * max_i + 1e-3, (mx, max_i)


def _instance_generator_out(Gb, x, c, mode):
    """The instance-norm generator with the batch-mode generator's parameters (same keys but the BN affine), in `mode`."""
    from srgan_amd import model, ops
    Gi = model.SingleGenerator(3, 64, 2, 2, 6, "instance", num_con=12)
    params = dict(Gb.named_parameters())
    Gi.load_state_dict({k: params[k].detach() for k in Gi.state_dict()})
    Gi.cuda()
    ops.set_compute_dtype(mode)
    try:
        with ops.pack_cache(), torch.no_grad():
            return ops.to_nchw(Gi(x.cuda(), c.cuda())).cpu()
    finally:
        ops.set_compute_dtype("fp32")


def test_get_samples_vs_reference_golden(golden_dir):
    """inference.get_samples (eval mode: the running statistics stand in) against the reference's (inference_batch_T.npz)."""
    from srgan_amd import model
    from srgan_amd.inference import get_samples
    from tests.batch_common import batch_buffers
    gold = np.load(os.path.join(golden_dir, "inference_batch_T.npz"))
    G = batch_buffers(batch_fill(model.SingleGenerator(3, 4, 2, 2, 1, "batch", num_con=12), 0), 4).cuda()
    E = batch_buffers(batch_fill(model.Encoder(3, 8, 4, 4, "batch", 4, "cuda"), 2), 5).cuda()
    torch.manual_seed(3)
    dataset = [(torch.rand(3, 128, 128) * 2 - 1, int(i % 4)) for i in range(3)]
    assert np.array_equal(np.array([d[1] for d in dataset]), gold["labels"])
    data, label = get_samples(G, E, dataset, 1, latent=gold["latent"], classes=(0, 1, 2, 3), ref_label=np.eye(4), ndim=8,
                              image_type="tensor", batch=2, device="cuda")
    assert np.array_equal(label["source"], gold["source_label"])
    for c in range(4):
        t = data["target"][c]
        t = t.detach().cpu().float() if torch.is_tensor(t) else torch.as_tensor(np.asarray(t)).float()
        close(F.avg_pool2d(t, 4), gold[f"target.{c}.pool4"], 2e-4, what=f"target {c}")
        assert abs(float(t.double().sum()) - float(gold[f"target.{c}.sum"])) <= 2e-4 * float(t.double().abs().sum())
        close(np.concatenate(label["latent"][c], 0), gold[f"mu.{c}"], 2e-4, what=f"mu {c}")
    assert not G.training and all(int(v) == 0 for k, v in G.state_dict().items() if k.endswith("num_batches_tracked"))


# ---- the trainer ------------------------------------------------------------------------------------------------------------------
def _trainer(k=2, batch=4):
    from srgan_amd import model
    from srgan_amd.trainer import SRGAN_training
    from oracle import params
    G, E = batch_fill(model.SingleGenerator(3, 4, 2, 2, 1, "batch", num_con=12), 0), batch_fill(model.Encoder(3, 8, 4, 4, "batch", 4, "cuda"), 2)
    D = model.SingleDiscriminator_solo_multi(3, 4, 2, 4, "batch", 4)
    D.load_state_dict(params.fill(params.discriminator_spec(nch_in=3, nch=4, reduce=2, num_cls=4, n_class=4), 1))
    torch.manual_seed(0)
    np.random.seed(0)
    sg = SRGAN_training([G.cuda(), D.cuda(), E.cuda()], [None, None, None], [nn.MSELoss(), nn.MSELoss()], dict(otrainer.DEFAULT_LBD),
                        k, "cuda", np.eye(4), batch, "mu", 8)
    sg.opt_sche_initialization()
    return sg


def _step(sg, s, batch=4):
    x, label = otrainer.synthetic_batch(batch, 128, 4, seed=100 + s)
    label = {"source": label["source"].cuda(), "target": label["target"]}
    return [float(v) for v in sg.train(x.cuda(), label)]


def _counts(sg):
    return [int(v) for net in (sg.G, sg.E) for k, v in net.state_dict().items() if k.endswith("num_batches_tracked")]


def test_train_trajectory_vs_reference(golden_dir):
    gold = np.load(os.path.join(golden_dir, "train_T_b4_k2_batch.npz"))
    sg = _trainer()
    traj, counts = [], []
    for s in range(4):
        traj.append(_step(sg, s))
        counts.append(_counts(sg))
    np.testing.assert_allclose(np.array(traj), gold["losses"], rtol=1e-3)
    np.testing.assert_array_equal(np.array(counts), gold["num_batches_tracked"])
    for net_name, net, n_opt in (("G", sg.G, 8), ("D", sg.D, 8), ("E", sg.E, 4)):
        for key, v in net.state_dict().items():
            if key.endswith("num_batches_tracked"):
                assert int(v) == int(gold[f"{net_name}.{key}"]), key
            elif "running" in key:
                close(v, gold[f"{net_name}.{key}"], 1e-3, 1e-5, what=f"{net_name}.{key}")
            else:
                close_params(v, gold[f"{net_name}.{key}"], 1e-4, n_opt, what=f"{net_name}.{key}")


def _six_steps(sg):
    """4 train-mode steps, one with G in eval mode, one back in train mode: losses and the state of every network after each."""
    out = []
    for s in range(6):
        sg.G.train(s != 4)
        losses = _step(sg, s)
        out.append((losses, [{k: v.clone() for k, v in net.state_dict().items()} for net in (sg.G, sg.D, sg.E)],
                    sg.graph_active))
    return out


def test_graph_replay_is_bit_identical_to_eager():
    """enable_graph: replay bit-identical to eager, running buffers included; toggling G.eval() / G.train() between steps drops
    the recording (the fingerprint holds every batch norm's mode and momentum) and the results stay those of the eager step."""
    eager = _six_steps(_trainer())
    graph = _six_steps(_trainer().enable_graph())
    assert graph[3][2], "steps 2 and 3 replay the recording"
    for s, ((la, sa, _), (lb, sb, _)) in enumerate(zip(eager, graph)):
        assert la == lb, (s, la, lb)
        for da, db in zip(sa, sb):
            for k in da:
                assert torch.equal(da[k], db[k]), (s, k)
