"""CPU: the host side of whole-trainer checkpoints on CPU-constructed trainers (nothing is launched) -- the dict's schema, the
version and config checks, the missing / unexpected report, the two host generators, the atomic save, the refusals."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

LBD = {"class": 1.0, "cycle": 5.0, "idt": 5.0, "reg": 0.5, "idt_reg": 0.5, "KL": 0.0, "batch_KL": 0.0, "corr_enc": 0.0, "hist": 0.0}


def _trainer(criterion=None, k=1, lbd=None, sched_steps=0):
    from srgan_amd import model
    from srgan_amd.trainer import SRGAN_training
    G = model.SingleGenerator(3, 4, 2, 2, 1, "instance", num_con=12)
    D = model.SingleDiscriminator_solo_multi(3, 4, 2, 4, "instance", 4)
    E = model.Encoder(3, 8, 4, 4, "instance", 4, "cpu")
    sg = SRGAN_training([G, D, E], [None, None, None], criterion or [nn.MSELoss(), nn.MSELoss()], dict(lbd or LBD), k, "cpu", np.eye(4),
                        4, "mu", 8)
    sg.opt_sche_initialization()
    for _ in range(sched_steps):
        sg.scheG.step()
    return sg


def _singlegan():
    from srgan_amd import model
    from srgan_amd.trainer import SingleGAN_training
    G = model.SingleGenerator(3, 4, 2, 2, 1, "instance", num_con=10)
    D = [model.SingleDiscriminator_original_multi(3, 4, 2, 4, "instance") for _ in range(2)]
    E = model.Encoder_original(3, 8, 4, 4, "instance", 2, "cpu")
    lbd = {"class": 0, "cycle": 5, "idt": 5, "reg": .5, "idt_reg": 0, "KL": .1, "batch_KL": 0, "corr_enc": 0, "hist": 0}
    sg = SingleGAN_training([G, D, E], [None, None, None], [nn.MSELoss(), nn.MSELoss()], lbd, 1, "cpu", np.eye(2), 8, (0, 1))
    sg.opt_sche_initialization()
    return sg


def _with_adam_state(sg):
    """moments and step counts as a few steps would have left them (written by hand: the step itself is a HIP kernel)"""
    g = torch.Generator().manual_seed(3)
    for opt, steps in ((sg.optG, 6), (sg.optD, 3), (sg.optE, 3)):
        for i, p in enumerate(q for grp in opt.param_groups for q in grp["params"]):
            if i % 5 == 4:
                continue                       # a parameter that never had a gradient keeps no state
            opt.state[p] = {"step": steps, "exp_avg": torch.randn(p.shape, generator=g), "exp_avg_sq": torch.rand(p.shape, generator=g)}
    return sg


def _leaves(obj, where="sd"):
    if isinstance(obj, dict):
        for k, v in obj.items():
            assert type(k) in (int, str), (where, k)
            yield from _leaves(v, f"{where}[{k!r}]")
    elif type(obj) is list:
        for i, v in enumerate(obj):
            yield from _leaves(v, f"{where}[{i}]")
    else:
        yield where, obj


# ---- schema ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [_trainer, _singlegan])
def test_schema_is_cpu_tensors_and_plain_values(tmp_path, make):
    sg = make()
    if make is _trainer:
        _with_adam_state(sg)
        sg.hi = types.SimpleNamespace(target=torch.rand(50))        # (the constructor's own target is made by a HIP kernel)
        sg.enable_diffaugment(seed=4)
        sg.enable_r1(gamma=5.0, every=2)
    sd = sg.state_dict()
    for where, v in _leaves(sd):
        if torch.is_tensor(v):
            assert v.device.type == "cpu" and type(v) is torch.Tensor, where
        else:
            assert v is None or type(v) in (int, float, bool, str), (where, type(v))
    assert sd["version"] == 1 and sd["config"]["trainer"] == type(sg).__name__
    want = {"version", "config", "G", "D", "E", "optG", "optD", "optE", "scheG", "scheD", "scheE", "rng"}
    if make is _trainer:
        want |= {"hist_target", "augment", "r1"}
        assert sd["r1"] == {"gamma": 5.0, "every": 2, "updates": 0, "n": None}
        assert sd["config"]["lbd"] == {k: float(v) for k, v in LBD.items()} and sd["config"]["k"] == 1
        assert (sd["config"]["criterion"], sd["config"]["criterion_class"]) == ("MSELoss", "MSELoss")
        assert sd["optG"]["state"][0]["step"] == 6 and type(sd["optG"]["state"][0]["step"]) is int and 4 not in sd["optG"]["state"]
    else:
        assert isinstance(sd["D"], list) and isinstance(sd["optD"], list) and isinstance(sd["scheD"], list)
    assert set(sd) == want
    # the snapshot shares no storage with the trainer
    p = next(sg.G.parameters())
    key = next(iter(sd["G"]))
    assert sd["G"][key].data_ptr() != p.data_ptr() and list(sd["G"]) == list(sg.G.state_dict())
    assert sd["rng"]["torch"].dtype == torch.uint8 and len(sd["rng"]["numpy"]["keys"]) == 624
    path = tmp_path / "ckpt.pt"
    sg.save_checkpoint(path)
    back = torch.load(path, map_location="cpu", weights_only=True)              # no pickled classes, no numpy arrays
    assert set(back) == want and back["config"] == sd["config"]
    for (wa, a), (wb, b) in zip(_leaves(sd), _leaves(back)):
        assert wa == wb and (torch.equal(a, b) if torch.is_tensor(a) else a == b), wa


def test_round_trip_restores_optimisers_schedulers_target_and_generators(tmp_path):
    a = _with_adam_state(_trainer(sched_steps=2))
    a.hi = types.SimpleNamespace(target=torch.rand(50))
    a.enable_diffaugment("color,cutout", cutout=0.25, seed=4)
    a.augment.draw(4, 16, 16)
    torch.manual_seed(11)
    np.random.seed(12)
    path = tmp_path / "ckpt.pt"
    a.save_checkpoint(path)
    want_torch, want_np, want_aug = torch.randn(5), np.random.rand(5), a.augment.draw(4, 16, 16)

    b = _trainer()
    b.hi = types.SimpleNamespace(target=torch.rand(50))
    torch.manual_seed(99)
    np.random.seed(98)
    report = b.load_checkpoint(path)
    assert report.missing == [] and report.unexpected == []
    assert torch.equal(torch.randn(5), want_torch) and np.array_equal(np.random.rand(5), want_np)
    assert b.augment is not None and (b.augment.policy, b.augment.cutout) == ("color,cutout", 0.25)      # enabled by the checkpoint
    assert torch.equal(b.augment.draw(4, 16, 16), want_aug)
    assert torch.equal(b.hi.target, a.hi.target)
    for n in "GDE":
        for (ka, va), (kb, vb) in zip(getattr(a, n).state_dict().items(), getattr(b, n).state_dict().items()):
            assert ka == kb and torch.equal(va, vb), (n, ka)
    assert b.optG.param_groups[0]["lr"] == a.optG.param_groups[0]["lr"] == pytest.approx(1e-4 * 0.95 ** 2)
    assert b.scheG.last_epoch == 2 and b.scheD.last_epoch == 0
    for opt_a, opt_b in ((a.optG, b.optG), (a.optD, b.optD), (a.optE, b.optE)):
        assert opt_b.param_groups[0]["betas"] == (0.5, 0.999) and isinstance(opt_b.param_groups[0]["betas"], tuple)
        for pa, pb in zip(opt_a.param_groups[0]["params"], opt_b.param_groups[0]["params"]):
            sa, sb = opt_a.state.get(pa), opt_b.state.get(pb)
            assert bool(sa) == bool(sb)                                   # a parameter without state stays without state
            if sa:
                assert type(sb["step"]) is int and sb["step"] == sa["step"]
                for key in ("exp_avg", "exp_avg_sq"):
                    m = sb[key]
                    assert torch.equal(m, sa[key]) and m.dtype == torch.float32 and m.is_contiguous() and m.device == pb.device
        assert opt_b.host_counters()[0] == {id(pb): opt_b.state[pb]["step"] for pb in opt_b.param_groups[0]["params"] if opt_b.state.get(pb)}


def test_adam_load_normalises_what_a_file_may_hand_back():
    from srgan_amd.optim import Adam
    p = nn.Parameter(torch.zeros(4, 3, 2))
    opt = Adam([p], lr=1e-4, betas=(0.5, 0.999))
    sd = {"state": {0: {"step": torch.tensor(5), "exp_avg": torch.ones(2, 3, 4, dtype=torch.float64).permute(2, 1, 0),
                        "exp_avg_sq": torch.ones(4, 3, 2)}},
          "param_groups": [{"lr": 2e-4, "betas": [0.5, 0.999], "eps": 1e-8, "params": [0]}]}
    opt.load_state_dict(sd)
    st = opt.state[p]
    assert type(st["step"]) is int and st["step"] == 5
    assert st["exp_avg"].dtype == torch.float32 and st["exp_avg"].is_contiguous() and st["exp_avg"].shape == p.shape
    assert opt.param_groups[0]["betas"] == (0.5, 0.999) and opt.param_groups[0]["lr"] == 2e-4
    assert opt.host_counters() == ({id(p): 5}, {})                        # no cohort survives: the next step seeds one at 5


# ---- version, config ---------------------------------------------------------------------------------------------------------------
def test_newer_version_is_refused():
    sg = _trainer()
    sd = sg.state_dict()
    sd["version"] = 2
    with pytest.raises(ValueError, match="format version 2"):
        sg.load_state_dict(sd)
    with pytest.raises(ValueError, match="format version 2"):
        sg.load_state_dict(sd, strict=False)
    with pytest.raises(ValueError, match="not a trainer checkpoint"):
        sg.load_state_dict({"G": {}})


@pytest.mark.parametrize("other,field", [(dict(k=2), "k"), (dict(lbd=dict(LBD, cycle=2.5)), "lbd.cycle"),
                                         (dict(criterion=[nn.BCEWithLogitsLoss(), nn.MSELoss()]), "criterion"),
                                         (dict(criterion=[nn.MSELoss(), nn.BCELoss()]), "criterion_class")])
def test_config_mismatch_names_the_field(other, field):
    sd = _trainer().state_dict()
    sg = _trainer(**other)
    before = {k: v.clone() for k, v in sg.G.state_dict().items()}
    with pytest.raises(ValueError, match=r"differs from the trainer's in " + field.replace(".", r"\.") + r"( |$)") as e:
        sg.load_state_dict(sd)
    assert "lbd.idt" not in str(e.value) and "ndim" not in str(e.value)
    assert all(torch.equal(v, before[k]) for k, v in sg.G.state_dict().items())          # refused before anything was written
    report = sg.load_state_dict(sd, strict=False)
    assert report.missing == [] and report.unexpected == []
    assert all(torch.equal(v, sd["G"][k]) for k, v in sg.G.state_dict().items())
    assert sg.k == other.get("k", 1)                                                      # the trainer keeps its own settings


# ---- missing / unexpected ----------------------------------------------------------------------------------------------------------
def test_extension_absent_from_the_checkpoint_is_missing_and_stays_on():
    sd = _trainer().state_dict()
    sg = _trainer()
    sg.enable_diffaugment(seed=4)
    gen = sg.augment.generator.get_state()
    with pytest.raises(ValueError, match="missing in the checkpoint: augment"):
        sg.load_state_dict(sd)
    report = sg.load_state_dict(sd, strict=False)
    assert report.missing == ["augment"] and report.unexpected == []
    assert sg.augment is not None and torch.equal(sg.augment.generator.get_state(), gen)


def test_sections_with_the_keys_of_the_first_format_still_load():
    """``augment``, ``geometry`` and ``ada`` written out as the first release of each wrote them: enabled by the load, nothing
    missing or unexpected, and each stage draws what a stage made from the saved settings and generator state draws"""
    from srgan_amd.augment import DiffAugment, GeometricAugment
    gen_a, gen_g = torch.Generator().manual_seed(21).get_state(), torch.Generator().manual_seed(22).get_state()
    sd = _trainer().state_dict()
    sd["augment"] = {"policy": "color,cutout", "translation": 0.125, "cutout": 0.25, "generator": gen_a.clone()}
    sd["geometry"] = {"policy": "flip,rotate", "scale_std": 0.3, "rotate_max": 0.5, "generator": gen_g.clone()}
    sd["ada"] = {"target": 0.5, "interval": 3, "kimg": 100.0, "p_max": 0.75, "p": 0.25, "seen": 0, "n_pos": 0, "n_neg": 0,
                 "n_total": 0, "adjustments": 0, "last_r": 0.0, "n": None}
    sg = _trainer()
    report = sg.load_state_dict(sd)
    assert report.missing == [] and report.unexpected == []
    assert [type(s) for s in sg._stages()] == [DiffAugment, GeometricAugment]
    assert (sg.augment.policy, sg.augment.translation, sg.augment.cutout) == ("color,cutout", 0.125, 0.25)
    assert (sg.geometry.policy, sg.geometry.scale_std, sg.geometry.rotate_max) == ("flip,rotate", 0.3, 0.5)
    assert (sg._ada.target, sg._ada.interval, sg._ada.kimg, sg._ada.p_max, sg._ada.p) == (0.5, 3, 100.0, 0.75, 0.25)
    old_a, old_g = DiffAugment("color,cutout", 0.125, 0.25), GeometricAugment("flip,rotate", 0.3, 0.5)
    old_a.generator.set_state(gen_a)
    old_g.generator.set_state(gen_g)
    for stage, old, groups in ((sg.augment, old_a, 3), (sg.geometry, old_g, 4)):
        assert torch.equal(stage.draw_fn(4, 16, 12), old.draw(4, 16, 12))
        assert torch.equal(stage.gate_fn(4), torch.rand(4, groups, generator=old.generator, dtype=torch.float32))
    assert sorted(sg.state_dict()["augment"]) == sorted(sd["augment"]) and sorted(sg.state_dict()["geometry"]) == sorted(sd["geometry"])


def test_r1_section_into_singlegan_is_unexpected_not_a_crash():
    sg = _singlegan()
    sd = sg.state_dict()
    sd["r1"] = {"gamma": 10.0, "every": 1, "updates": 3, "n": 4}
    sd["grad_guard"] = {"G": {"max_norm": 1.0, "steps": 2, "skipped": 0, "clipped": 1}}
    with pytest.raises(ValueError, match="unexpected in the checkpoint: r1, grad_guard.G"):
        sg.load_state_dict(sd)
    report = sg.load_state_dict(sd, strict=False)
    assert report.unexpected == ["r1", "grad_guard.G"] and report.missing == []
    # the other way round: a trainer class is part of the config
    with pytest.raises(ValueError, match="trainer"):
        _trainer().load_state_dict(sd)


def test_core_section_absent_is_missing():
    sg = _trainer()
    sd = sg.state_dict()
    del sd["scheD"], sd["optE"]
    with pytest.raises(ValueError, match="missing in the checkpoint: optE, scheD"):
        sg.load_state_dict(sd)
    assert sg.load_state_dict(sd, strict=False).missing == ["optE", "scheD"]


# ---- generators --------------------------------------------------------------------------------------------------------------------
def test_rng_false_leaves_both_generators_out_and_untouched():
    sg = _trainer()
    sd = sg.state_dict(rng=False)
    assert "rng" not in sd
    torch.manual_seed(5)
    np.random.seed(6)
    t, n = torch.get_rng_state(), np.random.get_state()
    report = sg.load_state_dict(sd)
    assert report.missing == [] and report.unexpected == []
    assert torch.equal(torch.get_rng_state(), t)
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), n))


# ---- atomic save -------------------------------------------------------------------------------------------------------------------
def test_failed_save_leaves_the_previous_file(tmp_path, monkeypatch):
    sg = _trainer()
    path = tmp_path / "ckpt.pt"
    sg.save_checkpoint(path)
    old = path.read_bytes()
    real_save = torch.save

    def half_way(obj, f, *args, **kwargs):
        f.write(b"half a checkpoint")
        raise OSError("disk full")

    monkeypatch.setattr(torch, "save", half_way)
    with torch.no_grad():
        next(sg.G.parameters()).add_(1.0)
    with pytest.raises(OSError, match="disk full"):
        sg.save_checkpoint(path)
    assert path.read_bytes() == old and os.listdir(tmp_path) == ["ckpt.pt"]
    monkeypatch.setattr(torch, "save", real_save)
    sg.save_checkpoint(path)                                                 # replaces the existing file
    assert os.listdir(tmp_path) == ["ckpt.pt"] and path.read_bytes() != old
    back = torch.load(path, weights_only=True)
    assert torch.equal(back["G"][next(iter(back["G"]))], next(sg.G.parameters()).detach())


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_load_inside_ema_weights_raises():
    sg = _trainer()
    sd = sg.state_dict()
    # the averaged copies are HIP-side objects; the scope itself only swaps attributes, so a stand-in serves it on the CPU
    sg._ema = types.SimpleNamespace(twins={})
    with sg.ema_weights():
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            sg.load_state_dict(sd)
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            sg.state_dict()
    sg._ema = None
    sg.load_state_dict(sd)
