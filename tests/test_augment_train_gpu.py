"""GPU: DiffAugment inside the train step (SRGAN_training.enable_diffaugment) at tier T, 128 x 128, batch 4, k = 2 -- off means
untouched, the step against the CPU oracle whose discriminator reads the float32 restatement of tests/augment_common.py on the
same tables, the style noise, graph mode, the generic discriminator path and the bf16 compute mode."""
import numpy as np
import pytest
import torch

from oracle import trainer as otrainer
from tests import augment_common as ac
from tests.common import close_params, oracle_params
from tests.ema_common import assert_same, live_state, make_trainer, one_step, steps
from tests.test_train_gpu import TERM_PAIRS

pytestmark = pytest.mark.gpu
BATCH, K, SIZE = 4, 2, 128
SN_SEED = 77


class Feed:
    """hands out fixed tables in the order they are asked for (the injectable ``draw_fn``)"""

    def __init__(self, tables):
        self.tables, self.i = list(tables), 0

    def __call__(self, n, h, w):
        t = self.tables[self.i]
        self.i += 1
        assert tuple(t.shape) == (n, ac.ROW)
        return t.clone()


def _step_tables(seed, n_steps=1, k=K):
    """2k + 1 tables per step in the draw order: per discriminator update real then fake, then phase 1's"""
    from srgan_amd.augment import DiffAugment
    aug = DiffAugment(seed=seed)
    return [aug.draw(BATCH, SIZE, SIZE) for _ in range(n_steps * (2 * k + 1))], aug.cut(SIZE, SIZE)


def _terms(sg):
    return {k: float(v) for k, v in sg.loss_terms.items()}


def test_enabled_then_disabled_equals_a_fresh_trainer():
    a = make_trainer("T", BATCH, K, 2)
    ref = steps(a, BATCH, 2, 300)
    b = make_trainer("T", BATCH, K, 2)
    b.enable_diffaugment(seed=1)
    assert b.augment is not None
    b.disable_diffaugment()
    assert b.augment is None
    got = steps(b, BATCH, 2, 300)
    np.testing.assert_array_equal(got, ref)
    assert_same(live_state(a), live_state(b))


def test_empty_policy_is_the_plain_step():
    a = make_trainer("T", BATCH, K, 3)
    ref = steps(a, BATCH, 1, 310)
    b = make_trainer("T", BATCH, K, 3).enable_diffaugment(policy="", seed=1)
    got = steps(b, BATCH, 1, 310)
    np.testing.assert_array_equal(got, ref)
    ta, tb = _terms(a), _terms(b)
    assert ta.keys() == tb.keys() and all(ta[k] == tb[k] for k in ta)
    assert_same(live_state(a), live_state(b))


def test_step_vs_the_oracle_on_the_restatement(monkeypatch):
    """full policy, the same injected tables on both sides: the three losses, every loss term and the parameters after the step at
    the bounds of test_train_gpu.step_vs_oracle (1e-3; close_params), and errG_dis more than 1e-4 away from the plain step's"""
    seed, batch_seed = 5, 42
    tables, cut = _step_tables(21)
    x, label = otrainer.synthetic_batch(BATCH, SIZE, 4, seed=batch_seed)
    real_d = otrainer.nets.discriminator
    feed_o = Feed(tables)

    def augmented_d(P, img, n_class):
        n, _, h, w = img.shape
        return real_d(P, ac.restate(img, feed_o(n, h, w), ac.ALL, cut, torch.float32), n_class)

    PG, PD, PE = oracle_params("T")
    torch.manual_seed(seed)
    orc = otrainer.SRGANOracle(PG, PD, PE, otrainer.DEFAULT_LBD, K, np.eye(4), BATCH, "mu", 8)
    monkeypatch.setattr(otrainer.nets, "discriminator", augmented_d)
    ref = [float(v) for v in orc.train(x, label)]
    monkeypatch.undo()
    assert feed_o.i == 2 * K + 1

    def hip_step(aug):
        sg = make_trainer("T", BATCH, K, seed)
        feed = None
        if aug:
            sg.enable_diffaugment(seed=0)
            feed = sg.augment.draw_fn = Feed(tables)
        out = [float(v) for v in sg.train(x.cuda(), {"source": label["source"].cuda(), "target": label["target"]})]
        assert feed is None or feed.i == 2 * K + 1
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


def test_style_noise_is_untouched():
    def run(aug):
        sg = make_trainer("T", BATCH, K, 4)
        if aug:
            sg.enable_diffaugment(seed=8)
        seen = []

        def noise(*shape):
            seen.append(torch.randn(*shape))
            return seen[-1]

        sg.noise_fn = noise
        torch.manual_seed(320)
        one_step(sg, BATCH, 320)
        return seen, torch.get_rng_state()

    off, state_off = run(False)
    on, state_on = run(True)
    assert len(off) == len(on) == K and all(torch.equal(a, b) for a, b in zip(off, on))
    assert torch.equal(state_off, state_on)          # the reparametrisation noise (normal_ on the default generator) too


def _aug_trainer(seed, aug_seed, extras=False, **policy):
    from srgan_amd import spectral
    sg = make_trainer("T", BATCH, K, seed)
    if extras:
        torch.manual_seed(SN_SEED)
        spectral.spectral_norm(sg.D)
        sg.enable_grad_guard()
    return sg.enable_diffaugment(seed=aug_seed, **policy)


def _state(sg, extras):
    out = live_state(sg)
    if extras:
        from tests import sn_common as sn
        out.update(sn.sn_state(sg.D))
    return out


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "spectral+guard"])
def test_graph_replay_is_bit_identical_to_eager(extras):
    """one eager warm-up step, then three steps of the recording, against four eager steps from the same seeds"""
    eager = _aug_trainer(2, 15, extras)
    ref = steps(eager, BATCH, 4, 500)
    sg = _aug_trainer(2, 15, extras).enable_graph()
    got = steps(sg, BATCH, 4, 500)
    assert sg.graph_active and sg._graph.aug is not None and tuple(sg._graph.aug.shape) == (2 * K + 1, BATCH, ac.ROW)
    np.testing.assert_array_equal(got, ref)
    assert_same(_state(eager, extras), _state(sg, extras))


def test_changing_the_policy_drops_the_recording_and_records_again():
    def change(t, s):
        if s == 1:
            if t._graph is not None:
                assert t.graph_active
            t.enable_diffaugment(policy="color,cutout", cutout=0.25, seed=31)
        if s == 4:
            t.augment.policy = "translation"              # edited in place: the fingerprint notices

    eager = _aug_trainer(3, 16)
    ref = steps(eager, BATCH, 7, 600, after=change)
    sg = _aug_trainer(3, 16).enable_graph()
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
    sg.disable_diffaugment()
    one_step(sg, BATCH, 607)
    one_step(sg, BATCH, 608)
    assert sg.graph_active and sg._graph.aug is None


def test_generic_discriminator_path_matches_the_fused_one():
    tables, _ = _step_tables(23)
    x, label = otrainer.synthetic_batch(BATCH, SIZE, 4, seed=44)

    def run(fused):
        sg = make_trainer("T", BATCH, K, 6).enable_diffaugment(seed=0)
        feed = sg.augment.draw_fn = Feed(tables)
        if not fused:
            sg._fused_paths = lambda: False
        torch.manual_seed(330)
        out = [float(v) for v in sg.train(x.cuda(), {"source": label["source"].cuda(), "target": label["target"]})]
        assert feed.i == 2 * K + 1
        return out, _terms(sg)

    (lf, tf), (lg, tg) = run(True), run(False)
    np.testing.assert_allclose(lg, lf, rtol=1e-5)
    assert tf.keys() == tg.keys()
    for k in tf:
        assert abs(tg[k] - tf[k]) <= 1e-5 * max(abs(tf[k]), 1e-3), (k, tg[k], tf[k])


def test_bf16_compute_mode_step():
    from srgan_amd import ops
    tables, _ = _step_tables(25)
    x, label = otrainer.synthetic_batch(BATCH, SIZE, 4, seed=46)

    def run():
        sg = make_trainer("T", BATCH, K, 7).enable_diffaugment(seed=0)
        sg.augment.draw_fn = Feed(tables)
        torch.manual_seed(340)
        out = [float(v) for v in sg.train(x.cuda(), {"source": label["source"].cuda(), "target": label["target"]})]
        return out, _terms(sg)

    ref, tref = run()
    ops.set_compute_dtype("bf16")
    try:
        got, tgot = run()
    finally:
        ops.set_compute_dtype("fp32")
        ops.invalidate_packed()
    assert np.isfinite(got).all() and all(np.isfinite(v) for v in tgot.values())
    np.testing.assert_allclose(got, ref, rtol=1e-2)
