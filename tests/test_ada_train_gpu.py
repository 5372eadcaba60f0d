"""GPU: adaptive discriminator augmentation inside the train step (SRGAN_training.enable_ada) at tier T, 128 x 128, batch 4,
k = 2 -- off means untouched, p pinned at 0 is the plain step and p pinned at 1 the DiffAugment step (bit for bit), the controller's
wiring against the restatement of tests/ada_common.py on the maps D produced, graph mode, checkpoints, the bf16 compute mode and
the refusals.  Every comparison is for equality."""
import numpy as np
import pytest
import torch

from oracle import trainer as otrainer
from tests import ada_common as adc
from tests import augment_common as ac
from tests.checkpoint_common import assert_rows_equal, assert_state_equal, run_a, run_b
from tests.ema_common import assert_same, live_state, make_trainer, one_step, steps

pytestmark = pytest.mark.gpu
BATCH, K, SIZE = 4, 2, 128
SN_SEED = 77
F32 = np.float32
RISE = dict(target=-2.0)           # r >= -1 > target: p rises at every adjustment
FALL = dict(target=2.0)            # r <= 1 < target: p falls


class Feed:
    """hands out fixed tables in the order they are asked for (the injectable ``draw_fn``)"""

    def __init__(self, tables):
        self.tables, self.i = list(tables), 0

    def __call__(self, n, h, w):
        t = self.tables[self.i]
        self.i += 1
        assert tuple(t.shape) == (n, ac.ROW)
        return t.clone()


def _step_tables(seed, n_steps):
    from srgan_amd.augment import DiffAugment
    aug = DiffAugment(seed=seed)
    return [aug.draw(BATCH, SIZE, SIZE) for _ in range(n_steps * (2 * K + 1))]


def _terms(sg):
    return {k: float(v) for k, v in sg.loss_terms.items()}


def _kimg(step, interval=1):
    """the kimg at which p moves by ``step`` per adjustment"""
    return BATCH * interval / (step * 1000.0)


def _record_outs(sg):
    """every ``forward_logits`` of sg.D from now on leaves clones of its maps in the returned list: per step the k discriminator
    updates' first, then phase 1's"""
    D, seen = sg.D, []
    orig = D.forward_logits

    def hooked(x):
        outs, logits = orig(x)
        seen.append([o.detach().clone() for o in outs])
        return outs, logits

    D.forward_logits = hooked
    return seen


def _ada_trainer(seed, aug_seed, extras=False, nets=None, **ada):
    from srgan_amd import spectral
    sg = make_trainer("T", BATCH, K, seed, nets=nets)
    if extras:
        torch.manual_seed(SN_SEED)
        spectral.spectral_norm(sg.D)
        sg.enable_r1()
    return sg.enable_diffaugment(seed=aug_seed).enable_ada(**ada)


def _state(sg, extras):
    out = live_state(sg)
    if extras:
        from tests import sn_common as sn
        out.update(sn.sn_state(sg.D))
    return out


# ---- off, and the two ends of p ------------------------------------------------------------------------------------------------------
def test_enabled_then_disabled_equals_a_diffaugment_trainer_that_never_had_it():
    a = make_trainer("T", BATCH, K, 2).enable_diffaugment(seed=1)
    ref = steps(a, BATCH, 2, 300)
    b = make_trainer("T", BATCH, K, 2).enable_diffaugment(seed=1).enable_ada()
    assert b._ada is not None
    b.disable_ada()
    assert b._ada is None and b.ada_stats() is None
    got = steps(b, BATCH, 2, 300)
    np.testing.assert_array_equal(got, ref)
    assert "ada_p" not in _terms(b) and _terms(a) == _terms(b)
    assert_same(live_state(a), live_state(b))
    assert torch.equal(a.augment.generator.get_state(), b.augment.generator.get_state())


def test_p_pinned_at_0_is_the_plain_step():
    from srgan_amd.augment import DiffAugment
    a = make_trainer("T", BATCH, K, 3)
    ref = steps(a, BATCH, 2, 310)
    b = _ada_trainer(3, 1, p=0.0, p_max=0.0)
    got = steps(b, BATCH, 2, 310)
    np.testing.assert_array_equal(got, ref)
    ta, tb = _terms(a), _terms(b)
    assert set(tb) == set(ta) | {"ada_p"} and all(ta[k] == tb[k] for k in ta) and tb["ada_p"] == 0.0
    assert_same(live_state(a), live_state(b))
    st = b.ada_stats()
    assert st["p"] == 0.0 and st["adjustments"] == (2 * K) // 4 and st["seen"] == (2 * K) % 4
    assert not torch.equal(b.augment.generator.get_state(), DiffAugment(seed=1).generator.get_state())      # it has advanced


def test_p_pinned_at_1_is_the_diffaugment_step():
    tables = _step_tables(21, 2)
    a = make_trainer("T", BATCH, K, 4).enable_diffaugment(seed=0)
    fa = a.augment.draw_fn = Feed(tables)
    ref = steps(a, BATCH, 2, 320)
    b = _ada_trainer(4, 0, p=1.0, p_max=1.0, interval=1, **RISE)
    fb = b.augment.draw_fn = Feed(tables)
    got = steps(b, BATCH, 2, 320)
    assert fa.i == fb.i == 2 * (2 * K + 1)
    np.testing.assert_array_equal(got, ref)
    ta, tb = _terms(a), _terms(b)
    assert set(tb) == set(ta) | {"ada_p"} and all(ta[k] == tb[k] for k in ta) and tb["ada_p"] == 1.0
    assert_same(live_state(a), live_state(b))
    assert b.ada_stats()["p"] == 1.0 and b.ada_stats()["adjustments"] == 2 * K


# ---- the controller's wiring ---------------------------------------------------------------------------------------------------------
def test_p_moves_by_step_per_adjustment_and_is_clamped():
    sg = _ada_trainer(5, 3, interval=1, kimg=_kimg(0.25), p=0.0, p_max=0.6, **RISE)
    seen = _record_outs(sg)
    torch.manual_seed(330)
    one_step(sg, BATCH, 330)
    st = sg.ada_stats()
    assert st["step"] == 0.25 and st["p"] == 0.5 and float(sg.loss_terms["ada_p"]) == 0.5      # 0.25 after the first update, then 0.5
    assert st["adjustments"] == K and st["seen"] == 0 and st["n_total"] == 0 and st["last_r"] >= -1.0
    one_step(sg, BATCH, 331)
    st = sg.ada_stats()
    assert F32(st["p"]) == F32(0.6) and st["adjustments"] == 2 * K                             # 0.75 clamped at p_max
    sg.set_ada_target(FALL["target"])
    sg.set_ada_p(0.5)
    one_step(sg, BATCH, 332)
    assert sg.ada_stats()["p"] == 0.0 and sg.ada_stats()["adjustments"] == 3 * K               # 0.25, then 0
    one_step(sg, BATCH, 333)
    assert sg.ada_stats()["p"] == 0.0 and float(sg.loss_terms["ada_p"]) == 0.0                 # clamped at 0
    # the counts between adjustments: interval 3 at k = 2 leaves the record mid-interval after every step
    per_row = sum(o.numel() // o.shape[0] for o in seen[0])
    assert len(seen[0]) == 2 and all(o.shape[0] == 2 * BATCH and o.dtype == torch.float32 for o in seen[0])
    sg = _ada_trainer(5, 3, interval=3, kimg=_kimg(0.25, 3), p=0.25, **RISE)
    torch.manual_seed(334)
    one_step(sg, BATCH, 334)
    st = sg.ada_stats()                                # two updates seen: one short of the adjustment
    assert (st["seen"], st["adjustments"], st["n_total"]) == (2, 0, BATCH * per_row * 2) and st["p"] == 0.25
    assert st["n_pos"] + st["n_neg"] <= st["n_total"] and st["step"] == 0.25
    one_step(sg, BATCH, 335)
    st = sg.ada_stats()                                # the third update adjusted on B * (P1 + P2) * interval elements and reset
    assert (st["seen"], st["adjustments"], st["n_total"]) == (1, 1, BATCH * per_row) and st["p"] == 0.5


def _restate_steps(sg, seen, st, n_steps, first_seed, thr=0.5):
    """``n_steps`` train steps; after each the device record against the restated controller fed with the maps D produced"""
    for s in range(n_steps):
        one_step(sg, BATCH, first_seed + s)
        calls = seen[s * (K + 1):(s + 1) * (K + 1)]
        assert len(calls) == K + 1
        for outs in calls[:K]:                         # the discriminator updates; phase 1's pass is not observed
            adc.observe(st, [o.cpu().numpy() for o in outs], BATCH, thr)
        adc.same_record(sg.ada_stats(), st)
        assert F32(float(sg.loss_terms["ada_p"])) == st["p"]


def test_last_r_and_p_against_the_maps_d_produced():
    ada = dict(target=0.1, interval=2, kimg=_kimg(0.125, 2), p=0.5, p_max=0.75)
    sg = _ada_trainer(6, 4, **ada)
    seen = _record_outs(sg)
    st = adc.new_state(0.5, 0.1, adc.step_size(BATCH, 2, ada["kimg"]), 0.75, 2)
    torch.manual_seed(340)
    _restate_steps(sg, seen, st, 3, 340)
    assert st["adjustments"] == 3 and -1.0 <= st["last_r"] <= 1.0 and st["p"] != F32(0.5)


def test_bce_criterion_uses_threshold_0():
    import torch.nn as nn
    sg = make_trainer("T", BATCH, K, 6)
    sg.criterion = nn.BCEWithLogitsLoss()
    sg.enable_diffaugment(seed=4).enable_ada(target=0.0, interval=1, kimg=_kimg(0.125), p=0.5)
    seen = _record_outs(sg)
    st = adc.new_state(0.5, 0.0, 0.125, 0.8, 1)
    torch.manual_seed(345)
    _restate_steps(sg, seen, st, 1, 345, thr=0.0)


def test_bf16_compute_mode_step():
    from srgan_amd import ops
    ops.set_compute_dtype("bf16")
    try:
        sg = _ada_trainer(7, 5, target=0.1, interval=1, kimg=_kimg(0.125), p=0.5)
        seen = _record_outs(sg)
        st = adc.new_state(0.5, 0.1, 0.125, 0.8, 1)
        torch.manual_seed(350)
        _restate_steps(sg, seen, st, 1, 350)
        assert all(o.dtype == torch.float32 for outs in seen for o in outs)     # what d_losses reads in this mode too
        assert all(np.isfinite(v) for v in _terms(sg).values())
    finally:
        ops.set_compute_dtype("fp32")
        ops.invalidate_packed()


# ---- graph mode ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extras", [False, True], ids=["plain", "spectral+r1"])
def test_graph_replay_is_bit_identical_to_eager(extras):
    """one eager warm-up step, then three steps of the recording, against four eager steps; p moves at every update"""
    ada = dict(interval=1, kimg=_kimg(1.0 / 16), p=0.25, **RISE)
    eager = _ada_trainer(2, 15, extras, **ada)
    ref = steps(eager, BATCH, 4, 500)
    sg = _ada_trainer(2, 15, extras, **ada).enable_graph()
    got = steps(sg, BATCH, 4, 500)
    assert sg.graph_active and sg._graph.aug is not None and tuple(sg._graph.aug.shape) == (2 * K + 1, BATCH, 16)
    np.testing.assert_array_equal(got, ref)
    assert _terms(sg) == _terms(eager)
    assert_same(_state(eager, extras), _state(sg, extras))
    assert sg.ada_stats() == eager.ada_stats() and sg.ada_stats()["p"] == 0.25 + 4 * K / 16 and sg.ada_stats()["adjustments"] == 4 * K
    assert torch.equal(sg.augment.generator.get_state(), eager.augment.generator.get_state())


def test_set_p_and_target_keep_the_recording_and_a_new_interval_drops_it():
    ps = {}

    def change(t, s):
        ps.setdefault(id(t), []).append(t.ada_stats()["p"])
        if s == 1:
            t.set_ada_p(0.5)
        if s == 2:
            t.set_ada_target(FALL["target"])
        if s == 3:
            t._ada.set_interval(2)

    ada = dict(interval=1, kimg=_kimg(1.0 / 16), p=0.0, **RISE)
    eager = _ada_trainer(3, 16, **ada)
    ref = steps(eager, BATCH, 6, 600, after=change)
    sg = _ada_trainer(3, 16, **ada).enable_graph()
    got = [steps(sg, BATCH, 2, 600, after=change)]
    assert sg.graph_active
    got.append(np.array([one_step(sg, BATCH, 602)]))
    assert sg.graph_active                                # set_ada_p kept the recording ...
    change(sg, 2)
    assert ps[id(sg)][-1] == 0.5 + K / 16                 # ... and the replay read the new p
    got.append(np.array([one_step(sg, BATCH, 603)]))
    assert sg.graph_active                                # set_ada_target kept it too
    change(sg, 3)
    assert ps[id(sg)][-1] == 0.5                          # ... and p fell by K / 16
    got.append(np.array([one_step(sg, BATCH, 604)]))
    assert not sg.graph_active                            # the new interval dropped it: this step ran eagerly
    change(sg, 4)
    got.append(np.array([one_step(sg, BATCH, 605)]))
    assert sg.graph_active                                # ... and the step was recorded again
    change(sg, 5)
    np.testing.assert_array_equal(np.concatenate(got), ref)
    assert ps[id(sg)] == ps[id(eager)]
    assert_same(live_state(eager), live_state(sg))
    assert sg.ada_stats() == eager.ada_stats() and sg.ada_stats()["interval"] == 2


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_checkpoint_resume_mid_interval(tmp_path, graph):
    """saved after 2 steps (4 updates at interval 3: one adjustment made, one update into the next interval, p mid-range), loaded
    into a bare trainer from another fill, 2 more steps: bit-identical to the uninterrupted run"""
    from tests.common import build_hip_nets
    path = tmp_path / "ada.pt"
    saved = {}

    def build_a():
        sg = _ada_trainer(2, 9, nets=build_hip_nets("T", seed=0), interval=3, kimg=_kimg(0.125, 3), p=0.3, **RISE)
        return sg.enable_graph() if graph else sg

    def build_b():
        sg = make_trainer("T", BATCH, K, 31, nets=build_hip_nets("T", seed=5))
        return sg.enable_graph() if graph else sg

    a = run_a(build_a, path, 2, 2, at_save=lambda sg: saved.update(sg.ada_stats()))
    assert saved["adjustments"] == 1 and saved["seen"] == 1 and saved["n_total"] > 0 and 0.3 < saved["p"] < 0.5
    b = run_b(build_b, path, 2, 2)
    (sg_a, rows_a, state_a), (sg_b, rows_b, state_b) = a, b
    assert_rows_equal(rows_a, rows_b, "ada resume")
    assert_state_equal(state_a, state_b, "ada resume")
    assert sg_a.ada_stats() == sg_b.ada_stats() and sg_b.ada_stats()["adjustments"] == 2
    assert sg_b._ada.kimg == sg_a._ada.kimg and sg_b._ada.p_max == 0.8
    assert sg_a.graph_active == sg_b.graph_active == graph


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_way_out(monkeypatch):
    from srgan_amd import dp
    sg = make_trainer("T", BATCH, K, 8).enable_diffaugment(seed=1)
    monkeypatch.setattr(dp, "is_distributed", lambda: True)
    with pytest.raises(NotImplementedError, match=r"ranks.*disable_ada"):
        sg.enable_ada()
    monkeypatch.undo()
    assert sg._ada is None
    sg.enable_ada()
    sg._fused_paths = lambda: False                       # the generic discriminator path, met when the step runs
    x, label = otrainer.synthetic_batch(BATCH, SIZE, 4, seed=1)
    with pytest.raises(NotImplementedError, match=r"fused discriminator pass.*disable_ada"):
        sg.train(x.cuda(), {"source": label["source"].cuda(), "target": label["target"]})
    with pytest.raises(NotImplementedError, match=r"fused discriminator pass.*disable_ada"):
        sg.enable_ada()
