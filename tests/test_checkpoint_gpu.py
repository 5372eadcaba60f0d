"""GPU: whole-trainer checkpoints resume bit for bit (tests/checkpoint_common.py has the two runs and the comparison).

Every case: tier-T networks, batch 4, k = 2, 128 x 128.  Run A trains, saves and goes on; run B is built from another fill and
another CPU-generator position, loads the file and trains the same batches.  Bit-identity, no tolerance."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.checkpoint_common import (BATCH, FIRST_SEED, K, assert_rows_equal, assert_state_equal, final_state, make_trainer, run_a,
                                     run_b, step_counts_are_ints, step_schedulers, train_rows)

pytestmark = pytest.mark.gpu


def _nets(seed):
    from tests.common import build_hip_nets
    return build_hip_nets("T", seed=seed)


def _plain(fill, seed, graph=False):
    def build():
        sg = make_trainer("T", BATCH, K, seed, nets=_nets(fill))
        return sg.enable_graph() if graph else sg
    return build


def _compare(a, b, what):
    (sg_a, rows_a, state_a), (sg_b, rows_b, state_b) = a, b
    assert_rows_equal(rows_a, rows_b, what)
    assert_state_equal(state_a, state_b, what)
    assert step_counts_are_ints(sg_b), what
    return sg_a, sg_b


# ---- 1. plain step, eager ----------------------------------------------------------------------------------------------------------
def test_plain_eager_resume(tmp_path):
    path = tmp_path / "plain.pt"
    a = run_a(_plain(0, 2), path, 2, 2, step_schedulers)
    b = run_b(_plain(5, 31), path, 2, 2, step_schedulers)
    sg_a, sg_b = _compare(a, b, "plain eager")
    assert sg_b.optG.param_groups[0]["lr"] == pytest.approx(0.95e-4)         # (the scheduler step fell between the two steps)
    # host mirrors and device records: Adam's step counts of the resumed run, read from the device
    import struct
    for opt_a, opt_b, most in ((sg_a.optG, sg_b.optG, 8), (sg_a.optD, sg_b.optD, 8), (sg_a.optE, sg_b.optE, 4)):
        (param_a, cohort_a), (param_b, cohort_b) = opt_a.host_counters(), opt_b.host_counters()
        assert list(param_a.values()) == list(param_b.values()) and max(param_b.values()) == most      # 4 train steps at k = 2
        assert sorted(cohort_a.values()) == sorted(cohort_b.values())
        for co in opt_b._cohorts.values():
            assert struct.unpack("i", co.state.cpu().numpy().tobytes()[:4])[0] == co.steps


# ---- 2. graph mode -----------------------------------------------------------------------------------------------------------------
def test_graph_mode_resume(tmp_path):
    path = tmp_path / "graph.pt"
    a = run_a(_plain(0, 2, graph=True), path, 3, 3, at_save=lambda sg: _assert(sg.graph_active, "run A saves after a replayed step"))
    b = run_b(_plain(5, 31, graph=True), path, 3, 3)
    sg_a, sg_b = _compare(a, b, "graph mode")
    assert sg_a.graph_active and sg_b.graph_active


def _assert(cond, what):
    assert cond, what


# ---- 3. every extension on at once, graph mode ---------------------------------------------------------------------------------
def _counters(sg):
    gg = sg.grad_guard_stats()
    return {"ema": sg.ema_updates, "r1": sg.r1_stats()["updates"],
            "guard": {n: (gg[n]["steps"], gg[n]["skipped"], gg[n]["clipped"]) for n in "GDE"}}


def test_every_extension_resumes_in_graph_mode(tmp_path):
    from srgan_amd import spectral
    path = tmp_path / "all_on.pt"
    saved = {}

    def build_a():
        sg = make_trainer("T", BATCH, K, 2, nets=_nets(0))
        torch.manual_seed(17)                  # u0 / v0 of the power iteration come from the CPU default generator
        spectral.spectral_norm(sg.D)
        sg.enable_ema()
        sg.enable_grad_guard(max_norm=1e-3)    # far below any gradient norm of these networks: every step clips
        sg.enable_diffaugment(seed=9)
        sg.enable_r1(every=2)
        return sg.enable_graph()

    def build_b():
        sg = make_trainer("T", BATCH, K, 31, nets=_nets(5))
        torch.manual_seed(18)
        spectral.spectral_norm(sg.D)           # part of building D; the checkpoint turns everything else on
        return sg.enable_graph()

    a = run_a(build_a, path, 3, 3, at_save=lambda sg: saved.update(_counters(sg)))
    print("counters at the save:", saved)
    assert saved["ema"] == 3 and saved["r1"] == 3
    assert all(saved["guard"][n][0] > 0 and saved["guard"][n][2] > 0 for n in "GDE"), saved    # else the case shows nothing
    b = run_b(build_b, path, 3, 3)
    sg_a, sg_b = _compare(a, b, "all extensions")
    assert sg_a.graph_active and sg_b.graph_active
    assert _counters(sg_a) == _counters(sg_b) and _counters(sg_b)["ema"] == 6 and _counters(sg_b)["r1"] == 6
    assert sg_b._ema.device_updates() == 6                                   # the host mirror and the device record agree
    assert sg_b.grad_guard_stats()["G"]["max_norm"] == float(np.float32(1e-3)) and sg_b.r1_stats()["every"] == 2
    assert spectral.sigmas(sg_a.D) == spectral.sigmas(sg_b.D)


# ---- 4. rollback inside one process that holds a recording -----------------------------------------------------------------------
def test_rollback_drops_the_recording():
    sg = make_trainer("T", BATCH, K, 2, nets=_nets(0)).enable_graph()
    torch.manual_seed(FIRST_SEED)
    train_rows(sg, 0, 2)
    assert sg.graph_active
    sd = sg.state_dict()
    first = train_rows(sg, 2, 2)
    state_first = final_state(sg)
    report = sg.load_state_dict(sd)
    assert report.missing == [] and report.unexpected == []
    assert not sg.graph_active and sg._graph is not None                     # the recording is gone, graph mode stays enabled
    again = train_rows(sg, 2, 2)                                             # eager, then recorded again
    assert sg.graph_active
    assert_rows_equal(first, again, "rollback")
    assert_state_equal(state_first, final_state(sg), "rollback")


# ---- 5. bf16 compute mode ----------------------------------------------------------------------------------------------------------
def test_bf16_mode_resume(tmp_path):
    from srgan_amd import ops
    path = tmp_path / "bf16.pt"
    ops.set_compute_dtype("bf16")
    try:
        a = run_a(_plain(0, 2), path, 2, 2, step_schedulers)
        b = run_b(_plain(5, 31), path, 2, 2, step_schedulers)
        _, sg_b = _compare(a, b, "bf16 mode")
        # fp32 master weights and moments
        assert all(p.dtype == torch.float32 for net in (sg_b.G, sg_b.D, sg_b.E) for p in net.parameters())
        assert all(v.dtype == torch.float32 for opt in (sg_b.optG, sg_b.optD, sg_b.optE) for st in opt.state.values()
                   for k, v in st.items() if k != "step")
        assert torch.load(path, weights_only=True)["config"]["compute_dtype"] == "bf16"
    finally:
        ops.set_compute_dtype("fp32")


# ---- 6. norm_type="batch", eager ---------------------------------------------------------------------------------------------------
def _batch_norm_nets(seed):
    from oracle import params
    from srgan_amd import model
    from tests.batch_common import batch_fill
    G = batch_fill(model.SingleGenerator(3, 4, 2, 2, 1, "batch", num_con=12), seed).cuda()
    E = batch_fill(model.Encoder(3, 8, 4, 4, "batch", 4, "cuda"), seed + 2).cuda()
    D = model.SingleDiscriminator_solo_multi(3, 4, 2, 4, "batch", 4)
    D.load_state_dict(params.fill(params.discriminator_spec(nch_in=3, nch=4, reduce=2, num_cls=4, n_class=4), seed + 1))
    return G, D.cuda(), E


def test_batch_norm_buffers_continue(tmp_path):
    path = tmp_path / "batch.pt"
    a = run_a(lambda: make_trainer("T", BATCH, K, 2, nets=_batch_norm_nets(0)), path, 2, 2)
    b = run_b(lambda: make_trainer("T", BATCH, K, 31, nets=_batch_norm_nets(5)), path, 2, 2)
    sg_a, sg_b = _compare(a, b, "batch norm")
    seen = 0
    for net_a, net_b in ((sg_a.G, sg_b.G), (sg_a.E, sg_b.E)):
        bufs_a, bufs_b = dict(net_a.named_buffers()), dict(net_b.named_buffers())
        assert bufs_a.keys() == bufs_b.keys()
        for k, v in bufs_a.items():
            assert torch.equal(v, bufs_b[k]), k
            if k.endswith("num_batches_tracked"):
                seen += 1
                assert int(v) >= 4, (k, int(v))                              # at least one forward per step, none lost at the resume
    assert seen > 0


# ---- 7. pretrained-E recipe with EMA -----------------------------------------------------------------------------------------------
def _is_head(key):
    return key.startswith(("fcmean", "fcvar"))


def _pretrained_e(fill, seed, ema):
    def build():
        from srgan_amd import optim as hoptim
        G, D, E = _nets(fill)
        keys = [k for k in E.state_dict().keys() if not _is_head(k)]
        E.freeze_melt(keys, "freeze")
        optE = hoptim.Adam(filter(lambda p: p.requires_grad, E.parameters()), lr=1e-3, betas=(0.5, 0.999))
        E.freeze_melt(keys, "melt")
        sg = make_trainer("T", BATCH, K, seed, nets=(G, D, E), opts=(None, None, optE))
        return sg.enable_ema() if ema else sg
    return build


def test_pretrained_encoder_recipe_with_ema(tmp_path):
    path = tmp_path / "pre.pt"
    a = run_a(_pretrained_e(0, 2, True), path, 2, 2)
    b = run_b(_pretrained_e(5, 31, False), path, 2, 2)
    sg_a, sg_b = _compare(a, b, "pretrained E")
    assert sg_b.ema_updates == 4
    for sg in (sg_a, sg_b):
        in_opt = {id(p) for g in sg.optE.param_groups for p in g["params"]}
        live, twin = sg.E.state_dict(), sg.E_ema.state_dict()
        for k, p in sg.E.named_parameters():
            assert (id(p) in in_opt) == _is_head(k), k
            if not _is_head(k):
                assert p not in sg.optE.state and torch.equal(twin[k], live[k]), k      # frozen trunk: no state, copy == live
    # a parameter that had no optimiser state at the save has none after the load
    for opt_a, opt_b in ((sg_a.optG, sg_b.optG), (sg_a.optD, sg_b.optD), (sg_a.optE, sg_b.optE)):
        for pa, pb in zip((p for g in opt_a.param_groups for p in g["params"]), (p for g in opt_b.param_groups for p in g["params"])):
            assert bool(opt_a.state.get(pa)) == bool(opt_b.state.get(pb))


# ---- 8. SingleGAN_training, eager --------------------------------------------------------------------------------------------------
def _singlegan(offset, seed):
    def build():
        from oracle import params
        from srgan_amd import model
        from srgan_amd.trainer import SingleGAN_training
        from tests.criteria_common import SG_BASE, SG_FILL
        G = model.SingleGenerator(3, 4, 2, 2, 1, "instance", num_con=10)
        G.load_state_dict(params.fill(params.generator_spec(3, 4, 2, 2, 1, 10), SG_FILL["G"] + offset))
        D = []
        for i in range(2):
            d = model.SingleDiscriminator_original_multi(3, 4, 2, 4, "instance")
            d.load_state_dict(params.fill(params.discriminator_original_spec(3, 4, 2, 4), SG_FILL[f"D{i}"] + offset))
            D.append(d.cuda())
        E = model.Encoder_original(3, 8, 4, 4, "instance", 2, "cuda")
        E.load_state_dict(params.fill(params.encoder_original_spec(3, 8, 4, 4, 2), SG_FILL["E"] + offset))
        G.cuda(), E.cuda()
        torch.manual_seed(seed)
        sg = SingleGAN_training([G, D, E], [None, None, None], [nn.MSELoss(), nn.MSELoss()], dict(SG_BASE, idt_reg=0.5), K, "cuda",
                                np.eye(2), 8, (0, 1), BATCH, "latent", False)
        sg.opt_sche_initialization()
        return sg
    return build


def test_singlegan_trainer_resume(tmp_path):
    path = tmp_path / "singlegan.pt"
    a = run_a(_singlegan(0, 2), path, 2, 2, step_schedulers, n_class=2)
    b = run_b(_singlegan(40, 31), path, 2, 2, step_schedulers, n_class=2)
    _, sg_b = _compare(a, b, "SingleGAN_training")
    assert isinstance(sg_b.optD, list) and len(sg_b.optD) == 2
    sd = torch.load(path, weights_only=True)
    assert sd["config"]["trainer"] == "SingleGAN_training" and isinstance(sd["D"], list) and len(sd["optD"]) == 2 == len(sd["scheD"])


# ---- 9. the two setters alone ------------------------------------------------------------------------------------------------------
def test_record_setters_write_only_the_counters():
    from srgan_amd import ops
    from srgan_amd._lib import SrganHipError
    dev = torch.device("cuda")
    guard = ops.grad_guard_state_new(dev, 2.5)
    before = ops.grad_guard_state_read(guard)
    ops.grad_guard_state_set_counters(guard, 7, 2, 3)
    assert ops.grad_guard_state_read(guard) == dict(before, steps=7, skipped=2, clipped=3)
    assert before == dict(max_norm=2.5, norm=0.0, scale=1.0, skip=False, steps=0, skipped=0, clipped=0)
    for bad in ((-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        with pytest.raises(SrganHipError, match="grad_guard_state_set_counters"):
            ops.grad_guard_state_set_counters(guard, *bad)
    assert ops.grad_guard_state_read(guard) == dict(before, steps=7, skipped=2, clipped=3)
    ops.grad_guard_state_set_counters(guard, 0, 0, 0)
    assert ops.grad_guard_state_read(guard) == before

    r1 = ops.r1_state_new(dev, 10.0, 2, 4)
    before = ops.r1_state_read(r1)
    assert before == dict(gamma=10.0, every=2, c=5.0, penalty=0.0, mean_sq_norm=0.0, updates=0, n=4)
    ops.r1_state_set_updates(r1, 11)
    assert ops.r1_state_read(r1) == dict(before, updates=11)
    with pytest.raises(SrganHipError, match="r1_state_set_updates"):
        ops.r1_state_set_updates(r1, -1)
    assert ops.r1_state_read(r1) == dict(before, updates=11)
    ops.r1_state_set(r1, 4.0, 2, 8)                      # the other setter keeps the count
    assert ops.r1_state_read(r1) == dict(before, gamma=4.0, c=1.0, n=8, updates=11)


# ---- 10. reference compatibility ---------------------------------------------------------------------------------------------------
def test_networks_in_the_file_keep_the_reference_layout(tmp_path, golden_dir):
    from srgan_amd import model
    from tests.common import TIER_T
    path = tmp_path / "compat.pt"
    sg = _plain(0, 2)()
    torch.manual_seed(FIRST_SEED)
    train_rows(sg, 0, 1)
    sg.save_checkpoint(path)
    ref = json.load(open(os.path.join(golden_dir, "shapes.json")))["T"]
    sd = torch.load(path, weights_only=True)
    for name in "GDE":
        assert [[k, list(v.shape)] for k, v in sd[name].items()] == ref[name], name
        assert all(not v.is_cuda for v in sd[name].values())
    g = TIER_T["G"]
    G = model.SingleGenerator(g["nch_in"], g["nch"], g["reduce"], g["num_cls"], g["res_num"], "instance", num_con=g["num_con"])
    G.load_state_dict(sd["G"], strict=True)
    for k, v in sg.G.state_dict().items():
        assert torch.equal(G.state_dict()[k], v.cpu()), k
