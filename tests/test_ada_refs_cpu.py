"""CPU: the parts of adaptive discriminator augmentation (srgan_amd.ada, csrc/ada.hip, SRGAN_training.enable_ada) that need no
GPU -- the restated controller of tests/ada_common.py by hand, the gate rule and the slot-7 decoding, validation, the fingerprint,
the trainer's refusals, the draw order, the state dict and the C ABI's argument checks."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ada_common as adc

F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from srgan_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.srgan_last_error().decode()


# ---- the restatement, by hand --------------------------------------------------------------------------------------------------------
def test_controller_by_hand():
    # interval 2: the first update only accumulates, the second adjusts on the counts of both
    st = adc.new_state(0.5, 0.25, 0.125, 0.75, 2)
    adc.controller(st, 6, 2, 10)
    assert (st["seen"], st["n_pos"], st["n_neg"], st["n_total"], st["adjustments"]) == (1, 6, 2, 10, 0) and st["p"] == F32(0.5)
    adc.controller(st, 5, 1, 6)                       # r = (11 - 3) / 16 = 0.5 > 0.25: up
    assert st["last_r"] == F32(0.5) and st["p"] == F32(0.625) and st["adjustments"] == 1
    assert (st["seen"], st["n_pos"], st["n_neg"], st["n_total"]) == (0, 0, 0, 0)
    # r == target: p stays
    st = adc.new_state(0.5, 0.25, 0.125, 0.75, 1)
    adc.controller(st, 5, 3, 8)                       # r = 2 / 8 = 0.25
    assert st["last_r"] == F32(0.25) and st["p"] == F32(0.5) and st["adjustments"] == 1
    # the upper clamp
    st = adc.new_state(0.7, 0.0, 0.125, 0.75, 1)
    adc.controller(st, 4, 0, 4)
    assert st["p"] == F32(0.75) and st["last_r"] == F32(1.0)
    adc.controller(st, 4, 0, 4)
    assert st["p"] == F32(0.75) and st["adjustments"] == 2
    # the lower clamp
    st = adc.new_state(0.1, 0.0, 0.125, 0.75, 1)
    adc.controller(st, 0, 3, 4)                       # r = -0.75 < 0: down, clamped at 0
    assert st["p"] == F32(0.0) and st["last_r"] == F32(-0.75)
    # a NaN counts in n_total only; the threshold itself on neither side
    pos, neg, tot = adc.observe_counts([np.array([[0.5, 0.6, np.nan, -np.inf], [9.0, 9.0, 9.0, 9.0]], dtype=F32)], 1, 0.5)
    assert (pos, neg, tot) == (1, 1, 4)
    pos, neg, tot = adc.observe_counts([np.array([[0.0, -0.0, 1e-45, -1e-45]], dtype=F32)], 1, 0.0)
    assert (pos, neg, tot) == (1, 1, 4)
    assert adc.step_size(4, 1, 0.016) == F32(0.25) and adc.step_size(64, 4, 500.0) == F32(64 * 4 / 500000.0)


def test_gate_rule_and_slot7_by_hand():
    top = F32(1.0) - F32(2.0 ** -24)
    u = np.array([[0.0, 0.25, top], [0.5, np.nan, 0.49999997]], dtype=F32)
    assert adc.gate_masks(u, 0.0).tolist() == [7, 7]                    # p = 0 skips everything (0 < 0 is false)
    assert adc.gate_masks(u, 1.0).tolist() == [0, 2]                    # p = 1 skips nothing but the NaN
    assert adc.gate_masks(u, 0.5).tolist() == [4, 3]                    # u == p skips
    assert adc.gate_masks(u, 2.0 ** -24).tolist() == [6, 7]
    rows = np.arange(32, dtype=F32).reshape(2, 16)
    rows[:, 8:11] = u
    t = adc.gate_rows(rows, 0.5)
    assert t.shape == (2, 8) and np.array_equal(t[:, :7], rows[:, :7]) and t[:, 7].tolist() == [4.0, 3.0]
    assert [adc.slot7_mask(v) for v in (0.0, 5.0, 7.0, 8.0, -1.0, float("nan"), 1e30, -1e30, 6.9)] == [0, 5, 7, 0, 7, 0, 0, 0, 6]


# ---- host logic ----------------------------------------------------------------------------------------------------------------------
def test_validation():
    from srgan_amd import ada
    for bad in (float("nan"), float("inf"), "x", None, True):
        with pytest.raises(ValueError, match="target"):
            ada.AdaptiveP(target=bad)
    for bad in (0, -2, 1.5, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="interval"):
            ada.AdaptiveP(interval=bad)
    for bad in (0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="kimg"):
            ada.AdaptiveP(kimg=bad)
    for p, p_max in ((-0.1, 0.8), (0.9, 0.8), (0.5, 1.5), (float("nan"), 0.8), (0.0, float("nan"))):
        with pytest.raises(ValueError, match="p_max"):
            ada.AdaptiveP(p=p, p_max=p_max)
    a = ada.AdaptiveP()
    assert (a.target, a.interval, a.kimg, a.p, a.p_max) == (0.6, 4, 500.0, 0.0, 0.8)
    assert a.step_size(64) == float(F32(64 * 4 / 500000.0))
    with pytest.raises(ValueError, match="p_max"):
        a.set_p(0.9)
    with pytest.raises(ValueError, match="target"):
        a.set_target(float("nan"))
    a.set_p(0.25)                                     # no device record yet: host state only
    a.set_target(0.5)
    st = a.stats()
    assert st["p"] == 0.25 and st["target"] == 0.5 and st["seen"] == 0 and st["n_total"] == 0 and st["adjustments"] == 0
    from srgan_amd import ops
    assert ada.threshold(ops.CRIT_MSE) == 0.5 and ada.threshold(ops.CRIT_BCE) == 0.0


def test_fingerprint_follows_interval_and_not_p_or_target():
    from srgan_amd import ada
    a = ada.AdaptiveP(interval=4)
    fp = a.fingerprint()
    a.set_p(0.3)
    a.set_target(0.1)
    assert a.fingerprint() == fp
    a.set_interval(2)
    assert a.fingerprint() != fp
    a.set_interval(4)
    assert a.fingerprint() == fp
    assert ada.AdaptiveP(interval=4).fingerprint() != fp          # another object is another recording
    assert a.graph_keepalive() == []


def test_state_dict_round_trip_without_a_record():
    from srgan_amd import ada
    a = ada.AdaptiveP(target=0.4, interval=3, kimg=20.0, p=0.25, p_max=0.5)
    sd = a.state_dict()
    assert sd == dict(target=0.4, interval=3, kimg=20.0, p_max=0.5, p=0.25, seen=0, n_pos=0, n_neg=0, n_total=0, adjustments=0,
                      last_r=0.0, n=None)
    b = ada.AdaptiveP()
    b.load_state_dict(sd)
    assert b.state_dict() == sd and b.state is None
    with pytest.raises(ValueError, match="batch size"):
        b.load_state_dict(dict(sd, seen=1))           # counters need a record, a record needs its batch size
    with pytest.raises(ValueError, match="interval"):
        b.load_state_dict(dict(sd, interval=0))
    assert b.state_dict() == sd                       # a refused load changed nothing


def _cpu_trainer():
    from srgan_amd import model, trainer
    D = model.SingleDiscriminator_solo_multi(3, 4, 2, 4, "instance", 4)
    G = model.SingleGenerator(3, 4, 2, 2, 1, "instance", num_con=12)
    E = model.Encoder(3, 8, 4, 4, "instance", 4, "cpu")
    lbd = dict(**{"class": 1.0}, cycle=5.0, idt=5.0, reg=0.5, idt_reg=0.5, KL=0.0, batch_KL=10.0, corr_enc=100.0, hist=0.0)
    crit = [torch.nn.MSELoss(), torch.nn.MSELoss()]
    return trainer.SRGAN_training([G, D, E], [None, None, None], crit, lbd, 2, "cpu", np.eye(4), batch_size=4, encoded_feature="mu",
                                  ndim=8)


def test_trainer_api_without_a_gpu(monkeypatch):
    from srgan_amd import ada, dp, trainer
    sg = _cpu_trainer()
    assert sg._ada is None and sg.ada_stats() is None
    with pytest.raises(RuntimeError, match="enable_ada"):
        sg.set_ada_p(0.5)
    with pytest.raises(RuntimeError, match="enable_ada"):
        sg.set_ada_target(0.5)
    with pytest.raises(NotImplementedError, match=r"DiffAugment is off.*enable_diffaugment"):
        sg.enable_ada()
    assert sg._ada is None
    sg.enable_diffaugment(policy="", seed=1)
    with pytest.raises(NotImplementedError, match=r"policy is empty.*enable_diffaugment"):
        sg.enable_ada()
    assert sg._ada is None
    sg.enable_diffaugment(seed=1)
    n_ext = len(sg._extensions())
    assert sg.enable_ada(target=0.5, interval=2, kimg=1.0, p=0.1, p_max=0.4) is sg and isinstance(sg._ada, ada.AdaptiveP)
    assert len(sg._extensions()) == n_ext + 1 and sg._extensions().index(sg._ada) == sg._extensions().index(sg.augment) + 1
    assert sg.ada_stats()["p"] == 0.1 and sg.ada_stats()["interval"] == 2
    sg.set_ada_p(0.2)
    sg.set_ada_target(0.3)
    assert sg._ada.p == 0.2 and sg._ada.target == 0.3
    assert "ada" in sg._ckpt_sections()
    for bad in (dict(target=float("nan")), dict(interval=0), dict(kimg=0), dict(p=0.9)):
        with pytest.raises(ValueError):
            sg.enable_ada(**bad)
    sg.disable_ada()
    assert sg._ada is None and sg.augment is not None
    sg.enable_ada()
    sg.disable_diffaugment()                          # nothing left to gate
    assert sg._ada is None and sg.augment is None
    # more than one rank, the generic discriminator path
    sg.enable_diffaugment(seed=1)
    monkeypatch.setattr(dp, "is_distributed", lambda: True)
    with pytest.raises(NotImplementedError, match=r"ranks.*disable_ada"):
        sg.enable_ada()
    monkeypatch.undo()
    sg._fused_paths = lambda: False
    with pytest.raises(NotImplementedError, match=r"fused discriminator pass.*disable_ada"):
        sg.enable_ada()
    assert sg._ada is None
    # the other trainer
    with pytest.raises(NotImplementedError, match="SRGAN_training.enable_ada"):
        trainer.SingleGAN_training.enable_ada(object())


def test_draw_order_table_then_three_uniforms_from_the_augmentations_generator():
    from srgan_amd.augment import DiffAugment
    sg = _cpu_trainer().enable_diffaugment(seed=11)
    sg.enable_ada()
    default_before = torch.get_rng_state()
    rows = [sg._stage_row_draw(sg.augment, 4, 16, 12) for _ in range(3)]
    assert torch.equal(torch.get_rng_state(), default_before)          # the default generator (style noise) is untouched
    ref = DiffAugment(seed=11)
    for r in rows:
        assert tuple(r.shape) == (4, 16) and r.dtype == torch.float32
        table = ref.draw(4, 16, 12)
        u = torch.rand(4, 3, generator=ref.generator, dtype=torch.float32)
        assert torch.equal(r[:, :8], table) and torch.equal(r[:, 8:11], u) and not r[:, 11:].any()
        assert bool(((u >= 0) & (u < 1)).all())
    assert torch.equal(sg.augment.generator.get_state(), ref.generator.get_state())
    # injectable beside draw_fn
    sg.augment.gate_fn = lambda n: torch.full((n, 3), 0.5)
    assert torch.equal(sg._stage_row_draw(sg.augment, 4, 16, 12)[:, 8:11], torch.full((4, 3), 0.5))


def test_with_the_feature_off_the_generator_advances_as_before():
    from srgan_amd.augment import DiffAugment
    sg = _cpu_trainer().enable_diffaugment(seed=12)
    ref = DiffAugment(seed=12)
    for _ in range(3):
        r = sg._stage_row_draw(sg.augment, 4, 16, 12)
        assert tuple(r.shape) == (4, 8) and torch.equal(r, ref.draw(4, 16, 12))
    assert torch.equal(sg.augment.generator.get_state(), ref.generator.get_state())
    sg.enable_ada()
    sg.disable_ada()
    assert torch.equal(sg._stage_row_draw(sg.augment, 4, 16, 12), ref.draw(4, 16, 12))
    assert sg._stage_draws(sg.augment) == 2 * sg.k + 1


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_back_before_any_launch(lib):
    buf = (ctypes.c_char * 4096)()
    b = ctypes.byref(buf)
    nan, inf = float("nan"), float("inf")
    assert lib.srgan_ada_state_bytes() == 56
    good = dict(p=0.1, target=0.6, step=0.01, p_max=0.8, interval=4)
    bad = [dict(target=nan), dict(target=inf), dict(step=-1.0), dict(step=nan), dict(p_max=1.5), dict(p_max=nan), dict(p=0.9),
           dict(p=-0.1), dict(p=nan), dict(interval=0), dict(interval=-3)]
    for change in bad:
        a = dict(good, **change)
        assert lib.srgan_ada_state_init(b, a["p"], a["target"], a["step"], a["p_max"], a["interval"], None) == -1, change
        assert "ada_state_init" in _err(lib)
        assert lib.srgan_ada_state_set(b, a["target"], a["step"], a["p_max"], a["interval"], 1, a["p"], None) == -1, change
        assert "ada_state_set" in _err(lib)
    assert lib.srgan_ada_state_init(None, 0.1, 0.6, 0.01, 0.8, 4, None) == -1 and "ada_state_init" in _err(lib)
    assert lib.srgan_ada_state_set(None, 0.6, 0.01, 0.8, 4, 0, 0.0, None) == -1 and "ada_state_set" in _err(lib)
    cnt = lib.srgan_ada_state_set_counters
    assert cnt(None, 0, 0, 0, 0, 0, 0.0, None) == -1 and "ada_state_set_counters" in _err(lib)
    for seen, pos, neg, tot, adj in ((-1, 0, 0, 0, 0), (0, -1, 0, 1, 0), (0, 0, -1, 1, 0), (0, 3, 3, 5, 0), (0, 0, 0, 0, -1)):
        assert cnt(b, seen, pos, neg, tot, adj, 0.0, None) == -1 and "ada_state_set_counters" in _err(lib)
    p = [ctypes.c_void_p(0x10000000 + (i << 20)) for i in range(3)]
    gate = lib.srgan_ada_gate
    for k in range(3):
        q = list(p)
        q[k] = None
        assert gate(q[0], q[1], q[2], 4, 3, None) == -1 and "null pointer" in _err(lib), k
    assert gate(p[0], p[1], p[2], 0, 3, None) == -1 and "n = 0" in _err(lib)
    assert gate(ctypes.c_void_p(0x10000004), p[1], p[2], 4, 3, None) == -1 and "aligned" in _err(lib)
    assert gate(p[0], p[1], p[0], 4, 3, None) == -1 and "alias" in _err(lib)
    for g in (0, 5, -1):                                                # the uniforms live in slots 8..11: 1 to 4 groups
        assert gate(p[0], p[1], p[2], 4, g, None) == -1 and f"n_groups = {g} (1 to 4)" in _err(lib), g
    obs = lib.srgan_ada_observe
    maps = (ctypes.c_void_p * 5)(*[0x20000000 + (i << 20) for i in range(5)])
    per = (ctypes.c_longlong * 5)(16, 4, 4, 4, 4)
    assert obs(maps, per, 2, 4, 0.5, None, None) == -1 and "null record" in _err(lib)
    assert obs(maps, per, 5, 4, 0.5, b, None) == -1 and "5 scales" in _err(lib)
    assert obs(maps, per, 0, 4, 0.5, b, None) == -1 and "0 scales" in _err(lib)
    assert obs(maps, per, 2, 0, 0.5, b, None) == -1 and "B = 0" in _err(lib)
    assert obs(maps, per, 2, -4, 0.5, b, None) == -1 and "B = -4" in _err(lib)
    assert obs(None, per, 2, 4, 0.5, b, None) == -1 and "null pointer" in _err(lib)
    assert obs(maps, None, 2, 4, 0.5, b, None) == -1 and "null pointer" in _err(lib)
    assert obs(maps, per, 2, 4, nan, b, None) == -1 and "threshold" in _err(lib)
    per0 = (ctypes.c_longlong * 2)(16, 0)
    assert obs(maps, per0, 2, 4, 0.5, b, None) == -1 and "map 1 has 0 elements per row" in _err(lib)
    maps0 = (ctypes.c_void_p * 2)(0x20000000, 0)
    assert obs(maps0, per, 2, 4, 0.5, b, None) == -1 and "map 1 is a null pointer" in _err(lib)
    # the gated augmentation entry points check what the ungated ones check
    q = [ctypes.c_void_p(0x30000000 + (i << 20)) for i in range(4)]
    fwd, bwd = lib.srgan_diffaugment_fwd_gated, lib.srgan_diffaugment_bwd_gated
    assert fwd(q[0], 2, None, 0, q[1], q[2], 4, 8, 8, 7, 4, 4, q[3], 64, None) == -1 and "diffaugment_fwd_gated: C = 4" in _err(lib)
    assert fwd(q[0], 2, None, 0, None, q[2], 3, 8, 8, 7, 4, 4, q[3], 64, None) == -1 and "null pointer" in _err(lib)
    assert fwd(q[0], 2, None, 0, q[1], q[2], 3, 8, 8, 8, 4, 4, q[3], 64, None) == -1 and "flags = 8" in _err(lib)
    assert fwd(q[0], 2, None, 0, q[1], q[2], 3, 8, 8, 1, 4, 4, None, 0, None) == -1 and "null workspace" in _err(lib)
    assert bwd(q[0], q[1], q[2], 0, 3, 8, 8, 7, 4, 4, q[3], 64, None) == -1 and "diffaugment_bwd_gated" in _err(lib)
    assert bwd(q[0], q[1], q[2], 2, 3, 8, 8, 7, 4, 4, q[3], 4, None) == -1 and "workspace" in _err(lib)
