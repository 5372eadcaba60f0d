"""GPU: the R1 gradient penalty inside the train step (SRGAN_training.enable_r1) at tier T, 128 x 128, batch 4, k = 2 -- the step
against the CPU oracle that adds the penalty by double backward (tests/r1_common.R1Oracle), off means untouched, graph mode, the
device record and the refusals."""
import numpy as np
import pytest
import torch

from oracle import trainer as otrainer
from tests import r1_common as rc
from tests.common import close_params, oracle_params
from tests.ema_common import assert_same, live_state, make_trainer, one_step, steps
from tests.test_train_gpu import TERM_PAIRS

pytestmark = pytest.mark.gpu
BATCH, K, SIZE = 4, 2, 128
GAMMA = 10.0
# Adam divides the scale of a gradient out, so after K = 2 steps a penalty much smaller than errD (gamma = 10 gives 0.01 against
# 1.3) leaves D within close_params of the plain step.  At this gamma the penalty's gradient leads (P is about 10 on the CPU
# oracle), and the oracle's own penalised and plain steps end outside those bounds of each other for every = 1 and every = 2.
GAMMA_ACTS = 1.0e4
SN_SEED = 77


def _terms(sg):
    return {k: float(v) for k, v in sg.loss_terms.items()}


def _cuda_batch(seed):
    x, label = otrainer.synthetic_batch(BATCH, SIZE, 4, seed=seed)
    return x, label, (x.cuda(), {"source": label["source"].cuda(), "target": label["target"]})


@pytest.mark.parametrize("every", [1, 2])
def test_step_vs_the_oracle_with_the_penalty(every):
    """the three losses, every loss term, the penalty and the parameters after the step at the bounds of
    test_train_gpu.step_vs_oracle (1e-3; close_params); every = 2: the penalty on update 0 only, with gamma_eff = 2 gamma; and D
    after the step differs from the plain step's by more than the bound: the penalty acts"""
    seed, batch_seed = 5, 42
    x, label, dev = _cuda_batch(batch_seed)
    PG, PD, PE = oracle_params("T")
    torch.manual_seed(seed)
    orc = rc.R1Oracle(PG, PD, PE, otrainer.DEFAULT_LBD, K, np.eye(4), BATCH, "mu", 8, gamma=GAMMA_ACTS, every=every)
    ref = [float(v) for v in orc.train(x, label)]
    assert len(orc.trace["errD_r1"]) == len([i for i in range(K) if i % every == 0])

    def hip_step(on):
        sg = make_trainer("T", BATCH, K, seed)
        if on:
            sg.enable_r1(gamma=GAMMA_ACTS, every=every)
        out = [float(v) for v in sg.train(*dev)]
        return sg, out

    sg, out = hip_step(True)
    np.testing.assert_allclose(out, ref, rtol=1e-3)
    t, tr = _terms(sg), orc.trace
    for a, b in TERM_PAIRS:
        assert abs(t[a] - tr[b]) <= 1e-3 * max(abs(tr[b]), 1e-3), (a, t[a], tr[b])
    for j, name in enumerate(("errD_real", "errD_class", "errD_fake")):
        want = tr["errD_parts"][-1][j]
        assert abs(t[name] - want) <= 1e-3 * max(abs(want), 1e-3), (name, t[name], want)
    want = tr["errD_r1"][-1]
    assert want > 0 and abs(t["errD_r1"] - want) <= 1e-3 * want, (t["errD_r1"], want)
    stats = sg.r1_stats()
    assert stats["penalty"] == t["errD_r1"] and stats["updates"] == len(tr["errD_r1"]) and stats["every"] == every
    assert stats["gamma"] == GAMMA_ACTS and abs(stats["c"] - GAMMA_ACTS * every / BATCH) <= 1e-6 * stats["c"]
    for net, P, n_opt in ((sg.G, orc.G, 2), (sg.D, orc.D, K), (sg.E, orc.E, 1)):
        for key, v in net.state_dict().items():
            close_params(v, P[key], 1e-4, n_opt, what=key)
    plain, out0 = hip_step(False)
    assert "errD_r1" not in _terms(plain)
    assert out[1] == out0[1]                      # errD of the first update is computed before any penalised gradient is used
    moved = []
    for key in rc.all_weight_keys(PD):
        try:
            close_params(sg.D.state_dict()[key], plain.D.state_dict()[key], 1e-4, K, what=key)
        except AssertionError:
            moved.append(key)
    assert moved, "the penalised step left D within close_params of the plain step: the penalty does not act"


def test_enabled_then_disabled_equals_a_fresh_trainer():
    a = make_trainer("T", BATCH, K, 2)
    ref = steps(a, BATCH, 2, 300)
    b = make_trainer("T", BATCH, K, 2)
    b.enable_r1(gamma=3.0, every=2)
    assert b._r1 is not None and b.r1_stats()["updates"] == 0
    b.disable_r1()
    assert b._r1 is None and b.r1_stats() is None
    got = steps(b, BATCH, 2, 300)
    np.testing.assert_array_equal(got, ref)
    assert_same(live_state(a), live_state(b))
    assert "errD_r1" not in b.loss_terms


def _r1_trainer(seed, extras=False, every=1, ema=False, aug=False):
    from srgan_amd import spectral
    sg = make_trainer("T", BATCH, K, seed)
    if extras:
        torch.manual_seed(SN_SEED)
        spectral.spectral_norm(sg.D)
        sg.enable_grad_guard()
    if ema:
        sg.enable_ema()
    if aug:
        sg.enable_diffaugment(seed=9)
    return sg.enable_r1(gamma=GAMMA, every=every)


def _state(sg, extras):
    out = live_state(sg)
    if extras:
        from tests import sn_common as sn
        out.update(sn.sn_state(sg.D))
    return out


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "ema+guard+spectral+diffaugment"])
def test_graph_replay_is_bit_identical_to_eager(extras):
    """one eager warm-up step, then three steps of the recording, against four eager steps from the same seeds"""
    eager = _r1_trainer(2, extras, ema=extras, aug=extras)
    ref = steps(eager, BATCH, 4, 500)
    sg = _r1_trainer(2, extras, ema=extras, aug=extras).enable_graph()
    got = steps(sg, BATCH, 4, 500)
    assert sg.graph_active
    np.testing.assert_array_equal(got, ref)
    assert_same(_state(eager, extras), _state(sg, extras))
    a, b = eager.r1_stats(), sg.r1_stats()
    assert a == b and a["updates"] == 4 * K and a["penalty"] > 0
    assert float(sg.loss_terms["errD_r1"]) == b["penalty"] == float(eager.loss_terms["errD_r1"])


def test_set_gamma_keeps_the_recording_and_changing_every_drops_it():
    def change(t, s):
        if s == 2:
            if t._graph is not None:
                assert t.graph_active
            t.set_r1_gamma(2.5)
            if t._graph is not None:
                assert t.graph_active                 # gamma is device state
        if s == 4:
            t.enable_r1(gamma=2.5, every=2)

    eager = _r1_trainer(3)
    ref = steps(eager, BATCH, 8, 600, after=change)
    sg = _r1_trainer(3).enable_graph()
    got = [steps(sg, BATCH, 3, 600, after=change)]
    got.append(np.array([one_step(sg, BATCH, 603)]))
    assert sg.graph_active                                # still the first recording, reading the new gamma
    assert sg.r1_stats()["gamma"] == 2.5
    got.append(np.array([one_step(sg, BATCH, 604)]))
    change(sg, 4)
    assert not sg.graph_active                            # another schedule: dropped
    got.append(np.array([one_step(sg, BATCH, 605)]))
    assert not sg.graph_active                            # this step ran eagerly ...
    got.append(np.array([one_step(sg, BATCH, 606)]))
    assert sg.graph_active                                # ... and the step was recorded again
    got.append(np.array([one_step(sg, BATCH, 607)]))
    np.testing.assert_array_equal(np.concatenate(got), ref)
    assert_same(live_state(eager), live_state(sg))
    assert eager.r1_stats() == sg.r1_stats() and sg.r1_stats()["every"] == 2 and sg.r1_stats()["updates"] == 3
    sg.disable_r1()
    one_step(sg, BATCH, 608)
    one_step(sg, BATCH, 609)
    assert sg.graph_active and "errD_r1" not in sg.loss_terms


def test_refusals_name_the_way_out(monkeypatch):
    from srgan_amd import dp, model, ops, r1
    from srgan_amd.trainer import SingleGAN_training
    sg = make_trainer("T", BATCH, K, 4)
    for bad, what in ((dict(gamma=-1.0), "gamma"), (dict(every=0), "every"), (dict(every=1.5), "every")):
        with pytest.raises(ValueError, match=what):
            sg.enable_r1(**bad)
    with pytest.raises(NotImplementedError, match="SRGAN_training.enable_r1"):
        SingleGAN_training.enable_r1(object())
    # more than one rank
    monkeypatch.setattr(dp, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="2 ranks.*disable_r1"):
        sg.enable_r1()
    monkeypatch.undo()
    assert sg._r1 is None
    # the bf16 mode and the image size: when the step runs
    sg.enable_r1()
    _, _, dev = _cuda_batch(50)
    ops.set_compute_dtype("bf16")
    try:
        with pytest.raises(NotImplementedError, match="bf16 compute mode.*set_compute_dtype"):
            sg.train(*dev)
    finally:
        ops.set_compute_dtype("fp32")
        ops.invalidate_packed()
    D = sg.D
    with pytest.raises(NotImplementedError, match="multiples of 16"):
        r1.r1_accumulate(D, torch.zeros(2, 3, 72, 72, device="cuda"), sg._r1)
    other = model.SingleDiscriminator_original_multi(3, 4, 2, 4, "instance", 2).cuda()
    with pytest.raises(NotImplementedError, match="forward_logits / two-scale layout"):
        r1.r1_accumulate(other, torch.zeros(2, 3, 128, 128, device="cuda"), sg._r1)
    # a first use inside a capture must not allocate
    fresh = r1.R1Penalty(1.0, 1)
    g = torch.cuda.CUDAGraph()
    x = torch.zeros(2, 3, 128, 128, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        x = ops.to_nhwc(x)
    torch.cuda.current_stream().wait_stream(s)
    with pytest.raises(RuntimeError, match="inside a hipGraph capture"):
        with torch.cuda.graph(g):
            fresh._ensure(x.device, 2)
