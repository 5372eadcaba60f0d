"""GPU: the geometric augmentation inside the train step (SRGAN_training.enable_geometric_augment) at tier T, 128 x 128, batch 4,
k = 2 -- off means untouched, the step against the CPU oracle whose discriminator reads the float32 restatement of
tests/geom_common.py on the same tables (alone and after the full DiffAugment policy), the style noise and DiffAugment's tables,
graph mode, the adaptive probability at both ends of p, checkpoints, the generic discriminator path and the bf16 compute mode."""
import numpy as np
import pytest
import torch

from oracle import trainer as otrainer
from tests import augment_common as ac
from tests import geom_common as gc
from tests.checkpoint_common import assert_rows_equal, assert_state_equal, run_a, run_b
from tests.common import close_params, oracle_params
from tests.ema_common import assert_same, live_state, make_trainer, one_step, steps
from tests.test_train_gpu import TERM_PAIRS

pytestmark = pytest.mark.gpu
BATCH, K, SIZE = 4, 2, 128
SN_SEED = 77
RISE = dict(target=-2.0)           # r >= -1 > target: p rises at every adjustment


class Feed:
    """hands out fixed tables in the order they are asked for (the injectable ``draw_fn``)"""

    def __init__(self, tables):
        self.tables, self.i = list(tables), 0

    def __call__(self, n, h, w):
        t = self.tables[self.i]
        self.i += 1
        assert tuple(t.shape) == (n, 8)
        return t.clone()


def _geo_tables(seed, n_steps=1, k=K):
    """2k + 1 tables per step in the draw order: per discriminator update real then fake, then phase 1's"""
    from srgan_amd.augment import GeometricAugment
    geo = GeometricAugment(seed=seed)
    return [geo.draw(BATCH, SIZE, SIZE) for _ in range(n_steps * (2 * k + 1))]


def _aug_tables(seed, n_steps=1, k=K):
    from srgan_amd.augment import DiffAugment
    aug = DiffAugment(seed=seed)
    return [aug.draw(BATCH, SIZE, SIZE) for _ in range(n_steps * (2 * k + 1))], aug.cut(SIZE, SIZE)


def _terms(sg):
    return {k: float(v) for k, v in sg.loss_terms.items()}


def _train(sg, x, label):
    return [float(v) for v in sg.train(x.cuda(), {"source": label["source"].cuda(), "target": label["target"]})]


# ---- off is off ----------------------------------------------------------------------------------------------------------------------
def test_enabled_then_disabled_equals_a_fresh_trainer():
    a = make_trainer("T", BATCH, K, 2)
    ref = steps(a, BATCH, 2, 300)
    b = make_trainer("T", BATCH, K, 2)
    b.enable_geometric_augment(seed=1)
    assert b.geometry is not None
    b.disable_geometric_augment()
    assert b.geometry is None
    got = steps(b, BATCH, 2, 300)
    np.testing.assert_array_equal(got, ref)
    assert_same(live_state(a), live_state(b))


def test_empty_policy_is_the_plain_step():
    from srgan_amd.augment import GeometricAugment
    a = make_trainer("T", BATCH, K, 3)
    ref = steps(a, BATCH, 1, 310)
    b = make_trainer("T", BATCH, K, 3).enable_geometric_augment(policy="", seed=1)
    got = steps(b, BATCH, 1, 310)
    np.testing.assert_array_equal(got, ref)
    ta, tb = _terms(a), _terms(b)
    assert ta.keys() == tb.keys() and all(ta[k] == tb[k] for k in ta)
    assert_same(live_state(a), live_state(b))
    assert torch.equal(b.geometry.generator.get_state(), GeometricAugment(seed=1).generator.get_state())      # no draw


# ---- the step against the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_diffaugment", [False, True], ids=["alone", "after-diffaugment"])
def test_step_vs_the_oracle_on_the_restatement(monkeypatch, with_diffaugment):
    """the same injected tables on both sides: the three losses, every loss term and the parameters after the step at the bounds of
    test_train_gpu.step_vs_oracle (1e-3; close_params), and errG_dis more than 1e-4 away from the plain step's"""
    seed, batch_seed = 5, 42
    geo_tables = _geo_tables(31)
    aug_tables, cut = _aug_tables(21)
    x, label = otrainer.synthetic_batch(BATCH, SIZE, 4, seed=batch_seed)
    real_d = otrainer.nets.discriminator
    feed_g, feed_a = Feed(geo_tables), Feed(aug_tables)

    def augmented_d(P, img, n_class):
        n, _, h, w = img.shape
        if with_diffaugment:
            img = ac.restate(img, feed_a(n, h, w), ac.ALL, cut, torch.float32)
        return real_d(P, gc.restate(img, feed_g(n, h, w), gc.ALL, torch.float32), n_class)

    PG, PD, PE = oracle_params("T")
    torch.manual_seed(seed)
    orc = otrainer.SRGANOracle(PG, PD, PE, otrainer.DEFAULT_LBD, K, np.eye(4), BATCH, "mu", 8)
    monkeypatch.setattr(otrainer.nets, "discriminator", augmented_d)
    ref = [float(v) for v in orc.train(x, label)]
    monkeypatch.undo()
    assert feed_g.i == 2 * K + 1 and feed_a.i == (2 * K + 1 if with_diffaugment else 0)

    def hip_step(on):
        sg = make_trainer("T", BATCH, K, seed)
        feeds = []
        if on:
            if with_diffaugment:
                sg.enable_diffaugment(seed=0)
                sg.augment.draw_fn = Feed(aug_tables)
                feeds.append(sg.augment.draw_fn)
            sg.enable_geometric_augment(seed=0)
            sg.geometry.draw_fn = Feed(geo_tables)
            feeds.append(sg.geometry.draw_fn)
        out = _train(sg, x, label)
        assert all(f.i == 2 * K + 1 for f in feeds)
        return sg, out

    sg, out = hip_step(True)
    np.testing.assert_allclose(out, ref, rtol=1e-3)
    t, tr = _terms(sg), orc.trace
    for a, b in TERM_PAIRS:
        assert abs(t[a] - tr[b]) <= 1e-3 * max(abs(tr[b]), 1e-3), (a, t[a], tr[b])
    for j, name in enumerate(("errD_real", "errD_class", "errD_fake")):
        want = tr["errD_parts"][-1][j]
        assert abs(t[name] - want) <= 1e-3 * max(abs(want), 1e-3), (name, t[name], want)
    for net, P, n_opt in ((sg.G, orc.G, 2), (sg.D, orc.D, K), (sg.E, orc.E, 1)):
        for key, v in net.state_dict().items():
            close_params(v, P[key], 1e-4, n_opt, what=key)
    plain, _ = hip_step(False)
    d0 = _terms(plain)["errG_dis"]
    assert abs(t["errG_dis"] - d0) > 1e-4 * abs(d0), (t["errG_dis"], d0)


# ---- noise and draws -----------------------------------------------------------------------------------------------------------------
def test_style_noise_and_diffaugment_tables_are_untouched():
    def run(geometry):
        sg = make_trainer("T", BATCH, K, 4).enable_diffaugment(seed=8)
        if geometry:
            sg.enable_geometric_augment(seed=8)
        seen, tables = [], []

        def noise(*shape):
            seen.append(torch.randn(*shape))
            return seen[-1]

        draw = sg.augment.draw

        def recorded(n, h, w):
            tables.append(draw(n, h, w))
            return tables[-1]

        sg.noise_fn = noise
        sg.augment.draw_fn = recorded
        torch.manual_seed(320)
        one_step(sg, BATCH, 320)
        return seen, tables, torch.get_rng_state(), sg

    off, tab_off, state_off, _ = run(False)
    on, tab_on, state_on, sg = run(True)
    assert len(off) == len(on) == K and all(torch.equal(a, b) for a, b in zip(off, on))
    assert torch.equal(state_off, state_on)          # the reparametrisation noise (normal_ on the default generator) too
    assert len(tab_off) == len(tab_on) == 2 * K + 1 and all(torch.equal(a, b) for a, b in zip(tab_off, tab_on))
    from srgan_amd.augment import GeometricAugment
    ref = GeometricAugment(seed=8)
    for _ in range(2 * K + 1):
        ref.draw(BATCH, SIZE, SIZE)
    assert torch.equal(sg.geometry.generator.get_state(), ref.generator.get_state())      # 2k + 1 geometry tables, nothing else


# ---- graph mode ----------------------------------------------------------------------------------------------------------------------
def _geom_trainer(seed, geo_seed, extras="plain", nets=None, **policy):
    from srgan_amd import spectral
    sg = make_trainer("T", BATCH, K, seed, nets=nets)
    if extras == "all":
        torch.manual_seed(SN_SEED)
        spectral.spectral_norm(sg.D)
        sg.enable_grad_guard()
        sg.enable_ema()
        sg.enable_r1()
    if extras in ("ada", "all"):
        sg.enable_diffaugment(seed=geo_seed + 100).enable_ada(interval=1, kimg=BATCH / (1000.0 / 16), p=0.25, **RISE)
    return sg.enable_geometric_augment(seed=geo_seed, **policy)


def _state(sg, extras):
    out = live_state(sg)
    if extras == "all":
        from tests import sn_common as sn
        from tests.ema_common import twin_state
        out.update(sn.sn_state(sg.D))
        out.update({"ema." + k: v for k, v in twin_state(sg).items()})
    return out


@pytest.mark.parametrize("extras", ["plain", "ada", "all"], ids=["plain", "diffaugment+ada", "ema+guard+spectral+r1+ada"])
def test_graph_replay_is_bit_identical_to_eager(extras):
    """one eager warm-up step, then three steps of the recording, against four eager steps from the same seeds"""
    eager = _geom_trainer(2, 15, extras)
    ref = steps(eager, BATCH, 4, 500)
    sg = _geom_trainer(2, 15, extras).enable_graph()
    got = steps(sg, BATCH, 4, 500)
    width = 16 if extras != "plain" else gc.ROW
    assert sg.graph_active and sg._graph.geom is not None and tuple(sg._graph.geom.shape) == (2 * K + 1, BATCH, width)
    assert (sg._graph.aug is None) == (extras == "plain")
    np.testing.assert_array_equal(got, ref)
    assert _terms(sg) == _terms(eager)
    assert_same(_state(eager, extras), _state(sg, extras))
    assert torch.equal(sg.geometry.generator.get_state(), eager.geometry.generator.get_state())
    if extras != "plain":
        assert sg.ada_stats() == eager.ada_stats() and sg.ada_stats()["p"] == 0.25 + 4 * K / 16


def test_changing_the_policy_drops_the_recording_and_records_again():
    def change(t, s):
        if s == 1:
            if t._graph is not None:
                assert t.graph_active
            t.enable_geometric_augment(policy="flip,scale", scale_std=0.1, seed=31)
        if s == 4:
            t.geometry.policy = "rot90"                   # edited in place: the fingerprint notices

    eager = _geom_trainer(3, 16)
    ref = steps(eager, BATCH, 7, 600, after=change)
    sg = _geom_trainer(3, 16).enable_graph()
    got = [steps(sg, BATCH, 2, 600, after=change)]
    got.append(np.array([one_step(sg, BATCH, 602)]))
    assert not sg.graph_active                            # dropped by the change: this step ran eagerly
    got.append(np.array([one_step(sg, BATCH, 603)]))
    assert sg.graph_active                                # ... and the step was recorded again
    got.append(np.array([one_step(sg, BATCH, 604)]))
    change(sg, 4)
    got.append(np.array([one_step(sg, BATCH, 605)]))
    assert not sg.graph_active
    got.append(np.array([one_step(sg, BATCH, 606)]))
    assert sg.graph_active
    np.testing.assert_array_equal(np.concatenate(got), ref)
    assert_same(live_state(eager), live_state(sg))
    sg.disable_geometric_augment()
    one_step(sg, BATCH, 607)
    one_step(sg, BATCH, 608)
    assert sg.graph_active and sg._graph.geom is None


# ---- the adaptive probability --------------------------------------------------------------------------------------------------------
def test_p_pinned_at_0_is_the_plain_step():
    a = make_trainer("T", BATCH, K, 3)
    ref = steps(a, BATCH, 2, 310)
    b = make_trainer("T", BATCH, K, 3).enable_diffaugment(seed=1).enable_geometric_augment(seed=2).enable_ada(p=0.0, p_max=0.0)
    got = steps(b, BATCH, 2, 310)
    np.testing.assert_array_equal(got, ref)
    ta, tb = _terms(a), _terms(b)
    assert set(tb) == set(ta) | {"ada_p"} and all(ta[k] == tb[k] for k in ta) and tb["ada_p"] == 0.0
    assert_same(live_state(a), live_state(b))
    # set_ada_p(0) on a record that stood elsewhere does the same from the next step on
    c = make_trainer("T", BATCH, K, 3).enable_diffaugment(seed=1).enable_geometric_augment(seed=2)
    c.enable_ada(p=0.5, kimg=1e9, target=0.0)             # (a step of ~0: p stays where it is put)
    c.set_ada_p(0.0)
    np.testing.assert_array_equal(steps(c, BATCH, 2, 310), ref)
    assert_same(live_state(a), live_state(c))


def test_p_pinned_at_1_is_the_ungated_step():
    aug_tables, _ = _aug_tables(21, 2)
    geo_tables = _geo_tables(22, 2)

    def build(ada):
        sg = make_trainer("T", BATCH, K, 4).enable_diffaugment(seed=0).enable_geometric_augment(seed=0)
        if ada:
            sg.enable_ada(p=1.0, p_max=1.0, interval=1, **RISE)
            sg.geometry.gate_fn = lambda n: torch.full((n, 4), 0.999)       # below 1: nothing is skipped
        fa = sg.augment.draw_fn = Feed(aug_tables)
        fg = sg.geometry.draw_fn = Feed(geo_tables)
        return sg, fa, fg

    a, fa, fg = build(False)
    ref = steps(a, BATCH, 2, 320)
    b, fb, fh = build(True)
    got = steps(b, BATCH, 2, 320)
    assert fa.i == fb.i == fg.i == fh.i == 2 * (2 * K + 1)
    np.testing.assert_array_equal(got, ref)
    ta, tb = _terms(a), _terms(b)
    assert set(tb) == set(ta) | {"ada_p"} and all(ta[k] == tb[k] for k in ta) and tb["ada_p"] == 1.0
    assert_same(live_state(a), live_state(b))


# ---- other paths ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_checkpoint_resume_is_bit_identical(tmp_path, graph):
    """saved after 2 steps, loaded into a bare trainer from another fill (the load switches the stage on), 2 more steps:
    bit-identical to the uninterrupted run, the geometry generator included"""
    from tests.common import build_hip_nets
    path = tmp_path / "geom.pt"

    def build_a():
        sg = _geom_trainer(2, 9, "ada", nets=build_hip_nets("T", seed=0), policy="flip,rot90,rotate", rotate_max=0.5)
        return sg.enable_graph() if graph else sg

    def build_b():
        sg = make_trainer("T", BATCH, K, 31, nets=build_hip_nets("T", seed=5))
        return sg.enable_graph() if graph else sg

    (sg_a, rows_a, state_a), (sg_b, rows_b, state_b) = run_a(build_a, path, 2, 2), run_b(build_b, path, 2, 2)
    assert_rows_equal(rows_a, rows_b, "geometry resume")
    assert_state_equal(state_a, state_b, "geometry resume")
    assert sg_b.geometry is not None and (sg_b.geometry.policy, sg_b.geometry.rotate_max) == ("flip,rot90,rotate", 0.5)
    assert torch.equal(sg_a.geometry.generator.get_state(), sg_b.geometry.generator.get_state())
    assert sg_a.ada_stats() == sg_b.ada_stats()
    assert sg_a.graph_active == sg_b.graph_active == graph


def test_generic_discriminator_path_matches_the_fused_one():
    geo_tables = _geo_tables(23)
    aug_tables, _ = _aug_tables(24)
    x, label = otrainer.synthetic_batch(BATCH, SIZE, 4, seed=44)

    def run(fused):
        sg = make_trainer("T", BATCH, K, 6).enable_diffaugment(seed=0).enable_geometric_augment(seed=0)
        fa = sg.augment.draw_fn = Feed(aug_tables)
        fg = sg.geometry.draw_fn = Feed(geo_tables)
        if not fused:
            sg._fused_paths = lambda: False
        torch.manual_seed(330)
        out = _train(sg, x, label)
        assert fa.i == fg.i == 2 * K + 1
        return out, _terms(sg)

    (lf, tf), (lg, tg) = run(True), run(False)
    np.testing.assert_allclose(lg, lf, rtol=1e-5)
    assert tf.keys() == tg.keys()
    for k in tf:
        assert abs(tg[k] - tf[k]) <= 1e-5 * max(abs(tf[k]), 1e-3), (k, tg[k], tf[k])


def test_bf16_compute_mode_step():
    from srgan_amd import ops
    geo_tables = _geo_tables(25)
    x, label = otrainer.synthetic_batch(BATCH, SIZE, 4, seed=46)

    def run():
        sg = make_trainer("T", BATCH, K, 7).enable_geometric_augment(seed=0)
        sg.geometry.draw_fn = Feed(geo_tables)
        torch.manual_seed(340)
        return _train(sg, x, label), _terms(sg)

    ref, _ = run()
    ops.set_compute_dtype("bf16")
    try:
        got, tgot = run()
    finally:
        ops.set_compute_dtype("fp32")
        ops.invalidate_packed()
    assert np.isfinite(got).all() and all(np.isfinite(v) for v in tgot.values())
    np.testing.assert_allclose(got, ref, rtol=1e-2)


def test_singlegan_training_refuses():
    from srgan_amd.trainer import SingleGAN_training
    with pytest.raises(NotImplementedError, match="SRGAN_training.enable_geometric_augment"):
        SingleGAN_training.enable_geometric_augment(object())
