"""GPU: balanced consistency regularisation inside the train step (SRGAN_training.enable_bcr) at tier T, 128 x 128, batch 4, k = 2 --
the step against the CPU oracle with the consistency terms (tests/cr_common.CROracle), off means untouched, the launches of an
unpenalised and of a penalised update, composition with every other extension, graph mode, checkpoints, the bf16 compute mode and the
refusals."""
import numpy as np
import pytest
import torch

from oracle import trainer as otrainer
from tests import ada_common as adc
from tests import cr_common as cc
from tests import r1_common as rc
from tests.checkpoint_common import assert_rows_equal, assert_state_equal, run_a, run_b
from tests.common import close_params, oracle_params
from tests.ema_common import assert_same, live_state, make_trainer, one_step, steps
from tests.step_bits_common import _launch_counts
from tests.test_train_gpu import TERM_PAIRS

pytestmark = pytest.mark.gpu
BATCH, K, SIZE = 4, 2, 128
LAM = cc.LAMBDA_ACTS               # tests/test_cr_refs_cpu.py: at this weight the oracle's D leaves the plain oracle's
SN_SEED = 77
NEW_KERNELS = ("cr_pairs_kernel", "d_losses_cr_kernel")


def _terms(sg):
    return {k: float(v) for k, v in sg.loss_terms.items()}


def _cuda_batch(seed):
    x, label = otrainer.synthetic_batch(BATCH, SIZE, 4, seed=seed)
    return x, label, (x.cuda(), {"source": label["source"].cuda(), "target": label["target"]})


@pytest.mark.parametrize("every", [1, 2])
def test_step_vs_the_oracle_with_the_consistency_terms(every):
    """the three losses, every loss term, the two new terms and the parameters after the step at the bounds of
    test_train_gpu.step_vs_oracle (1e-3; close_params); every = 2: the terms on update 0 only, weighted 2 lambda; and D after the
    step differs from the plain step's by more than the bound: the terms act"""
    seed, batch_seed = 5, 42
    x, label, dev = _cuda_batch(batch_seed)
    PG, PD, PE = oracle_params("T")
    torch.manual_seed(seed)
    orc = cc.CROracle(PG, PD, PE, otrainer.DEFAULT_LBD, K, np.eye(4), BATCH, "mu", 8, lambda_real=LAM, lambda_fake=LAM, every=every,
                      seed=cc.CR_SEED)
    ref = [float(v) for v in orc.train(x, label)]
    n_pen = len([i for i in range(K) if i % every == 0])
    assert len(orc.trace["errD_cr"]) == n_pen

    def hip_step(on):
        sg = make_trainer("T", BATCH, K, seed)
        if on:
            sg.enable_bcr(lambda_real=LAM, lambda_fake=LAM, every=every, seed=cc.CR_SEED)
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
    for j, name in enumerate(("errD_cr_real", "errD_cr_fake")):
        want = tr["errD_cr"][-1][j]
        print(f"every {every} {name}: {t[name]:.9g} oracle {want:.9g} rel {abs(t[name] - want) / want:.3e}")
        assert want > 0 and abs(t[name] - want) <= 1e-3 * want, (name, t[name], want)
    stats = sg.bcr_stats()
    assert stats == dict(lambda_real=LAM, lambda_fake=LAM, every=every, cr_real=t["errD_cr_real"], cr_fake=t["errD_cr_fake"],
                         updates=n_pen)
    for net, P, n_opt in ((sg.G, orc.G, 2), (sg.D, orc.D, K), (sg.E, orc.E, 1)):
        for key, v in net.state_dict().items():
            close_params(v, P[key], 1e-4, n_opt, what=key)
    plain, out0 = hip_step(False)
    assert "errD_cr_real" not in _terms(plain) and plain.bcr_stats() is None
    assert out[1] == out0[1]                      # errD of the first update: the value without the terms, before any of their gradients
    moved = []
    for key in rc.all_weight_keys(PD):
        try:
            close_params(sg.D.state_dict()[key], plain.D.state_dict()[key], 1e-4, K, what=key)
        except AssertionError:
            moved.append(key)
    assert moved, "the regularised step left D within close_params of the plain step: the terms do not act"


def test_enabled_then_disabled_equals_a_fresh_trainer():
    a = make_trainer("T", BATCH, K, 2)
    ref = steps(a, BATCH, 2, 300)
    b = make_trainer("T", BATCH, K, 2)
    b.enable_bcr(lambda_real=3.0, every=2, seed=1)
    assert b.bcr is not None and b.bcr_stats()["updates"] == 0
    b.disable_bcr()
    assert b.bcr is None and b.bcr_stats() is None
    got = steps(b, BATCH, 2, 300)
    np.testing.assert_array_equal(got, ref)
    assert_same(live_state(a), live_state(b))
    assert _terms(a) == _terms(b) and "errD_cr_real" not in b.loss_terms


def _update_launches(sg, index):
    """{kernel: launches} of ONE discriminator update (number ``index`` of a step) of a trainer that has run a step"""
    from srgan_amd import _lib, ops
    lib = _lib.load()
    with ops.pack_cache():
        torch.cuda.synchronize()
        lib.srgan_prof_enable(1)
        try:
            sg.update_D(_index=index)
            torch.cuda.synchronize()
        finally:
            lib.srgan_prof_enable(0)
        return _launch_counts(lib)


@pytest.mark.parametrize("staged", [False, True], ids=["no_stage", "diffaugment+geometry"])
def test_launches_of_an_unpenalised_and_of_a_penalised_update(staged):
    """every = 2: update 1 launches exactly the kernels of the plain update; update 0 the same NUMBER of network launches (on twice
    the rows, so a convolution may take another tile shape), one pair builder -- in place of the concatenation, or behind the last
    stage -- and one fused loss"""
    def build(on):
        sg = make_trainer("T", BATCH, K, 3)
        if staged:
            sg.enable_diffaugment(seed=4).enable_geometric_augment(seed=5)
        if on:
            sg.enable_bcr(every=2, seed=6)
        torch.manual_seed(360)
        one_step(sg, BATCH, 360)
        return sg

    plain, sg = build(False), build(True)
    want = _update_launches(plain, 1)
    assert want and not any(k in want for k in NEW_KERNELS)
    assert _update_launches(sg, 1) == want
    got = _update_launches(sg, 0)
    assert got.pop("cr_pairs_kernel") == 1 and got.pop("d_losses_cr_kernel") == 1
    assert sum(got.values()) == sum(want.values()), (got, want)
    assert sg.bcr_stats()["updates"] == 2                      # update 0 of the step, and the one above


def _record_outs(sg):
    D, seen = sg.D, []
    orig = D.forward_logits

    def hooked(x):
        outs, logits = orig(x)
        seen.append([o.detach().clone() for o in outs])
        return outs, logits

    D.forward_logits = hooked
    return seen


def _everything(seed, bcr=True, every=1, graph=False, nets=None):
    from srgan_amd import spectral
    sg = make_trainer("T", BATCH, K, seed, nets=nets)
    torch.manual_seed(SN_SEED)
    spectral.spectral_norm(sg.D)
    sg.enable_grad_guard(max_norm=1.0)
    sg.enable_ema()
    sg.enable_diffaugment(seed=9).enable_geometric_augment(seed=10)
    sg.enable_ada(target=0.1, interval=1, kimg=BATCH / (0.125 * 1000.0), p=0.5)
    sg.enable_r1(gamma=10.0, every=2)
    if bcr:
        sg.enable_bcr(lambda_real=5.0, lambda_fake=2.0, every=every, seed=11)
    return sg.enable_graph() if graph else sg


def test_composition_with_every_other_extension():
    """DiffAugment + geometric stage + ADA + R1 + spectral norm + gradient guard + EMA + bCR: one step runs; ADA's record is the
    restated controller fed with the FRONT B rows of the maps D produced (4B rows in a penalised update); the other stages' tables
    are what they are without bCR"""
    sg = _everything(7)
    seen = _record_outs(sg)
    st = adc.new_state(0.5, 0.1, 0.125, 0.8, 1)
    torch.manual_seed(370)
    out = one_step(sg, BATCH, 370)
    assert all(np.isfinite(out)) and all(np.isfinite(v) for v in _terms(sg).values())
    assert len(seen) == K + 1 and [o.shape[0] for o in seen[0]] == [4 * BATCH] * 2 and [o.shape[0] for o in seen[K]] == [BATCH] * 2
    for outs in seen[:K]:
        adc.observe(st, [o.cpu().numpy() for o in outs], BATCH, 0.5)
    adc.same_record(sg.ada_stats(), st)
    t = _terms(sg)
    assert t["errD_cr_real"] > 0 and t["errD_cr_fake"] > 0 and t["errD_r1"] > 0
    assert sg.bcr_stats()["updates"] == K and sg.r1_stats()["updates"] == 1
    default_after = torch.get_rng_state()
    other = _everything(7, bcr=False)
    torch.manual_seed(370)
    one_step(other, BATCH, 370)
    assert torch.equal(sg.augment.generator.get_state(), other.augment.generator.get_state())
    assert torch.equal(sg.geometry.generator.get_state(), other.geometry.generator.get_state())
    assert torch.equal(torch.get_rng_state(), default_after)                 # the step's noise stream too
    from srgan_amd.consistency import ConsistencyPairs
    ref = ConsistencyPairs(seed=11)
    for _ in range(2 * K):
        ref.draw(BATCH, SIZE, SIZE)
    assert torch.equal(sg.bcr.stage.generator.get_state(), ref.generator.get_state())          # two tables per penalised update


def _bcr_trainer(seed, every=1, extras=False):
    if extras:
        return _everything(seed, every=every)
    return make_trainer("T", BATCH, K, seed).enable_bcr(lambda_real=5.0, lambda_fake=2.0, every=every, seed=11)


def _state(sg, extras):
    out = live_state(sg)
    if extras:
        from tests import sn_common as sn
        from tests.ema_common import twin_state
        out.update(sn.sn_state(sg.D))
        out.update({"ema." + k: v for k, v in twin_state(sg).items()})
    return out


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "everything_on"])
def test_graph_replay_is_bit_identical_to_eager(extras):
    """one eager warm-up step, then three steps of the recording, against four eager steps from the same seeds"""
    eager = _bcr_trainer(2, 2 if extras else 1, extras)
    ref = steps(eager, BATCH, 4, 500)
    sg = _bcr_trainer(2, 2 if extras else 1, extras).enable_graph()
    got = steps(sg, BATCH, 4, 500)
    assert sg.graph_active
    n_pen = 1 if extras else K
    assert tuple(sg._graph.tables("bcr").shape) == (2 * n_pen, BATCH, 8)
    np.testing.assert_array_equal(got, ref)
    assert _terms(sg) == _terms(eager)
    assert_same(_state(eager, extras), _state(sg, extras))
    a, b = eager.bcr_stats(), sg.bcr_stats()
    assert a == b and a["updates"] == 4 * n_pen and a["cr_real"] > 0
    assert float(sg.loss_terms["errD_cr_real"]) == b["cr_real"] and float(sg.loss_terms["errD_cr_fake"]) == b["cr_fake"]
    assert torch.equal(sg.bcr.stage.generator.get_state(), eager.bcr.stage.generator.get_state())


def test_set_weights_keeps_the_recording_and_a_new_every_drops_it():
    def change(t, s):
        if s == 2:
            if t._graph is not None:
                assert t.graph_active
            t.set_bcr_weights(50.0, 0.0)
            if t._graph is not None:
                assert t.graph_active                 # the weights are device state
        if s == 4:
            t.enable_bcr(lambda_real=50.0, lambda_fake=0.0, every=2, seed=12)

    eager = _bcr_trainer(3)
    ref = steps(eager, BATCH, 8, 600, after=change)
    sg = _bcr_trainer(3).enable_graph()
    got = [steps(sg, BATCH, 3, 600, after=change)]
    got.append(np.array([one_step(sg, BATCH, 603)]))
    assert sg.graph_active                                # still the first recording, reading the new weights
    assert sg.bcr_stats()["lambda_real"] == 50.0 and sg.bcr_stats()["lambda_fake"] == 0.0
    got.append(np.array([one_step(sg, BATCH, 604)]))
    change(sg, 4)
    assert not sg.graph_active                            # another schedule: dropped
    got.append(np.array([one_step(sg, BATCH, 605)]))
    assert not sg.graph_active                            # this step ran eagerly ...
    got.append(np.array([one_step(sg, BATCH, 606)]))
    assert sg.graph_active                                # ... and the step was recorded again
    got.append(np.array([one_step(sg, BATCH, 607)]))
    got = np.concatenate(got)
    np.testing.assert_array_equal(got, ref)
    assert_same(live_state(eager), live_state(sg))
    assert eager.bcr_stats() == sg.bcr_stats() and sg.bcr_stats()["every"] == 2 and sg.bcr_stats()["updates"] == 3
    # the new weights changed the step that followed them: an uninterrupted run from the same seeds ends elsewhere
    same = steps(_bcr_trainer(3), BATCH, 4, 600)
    assert np.array_equal(same[:3], ref[:3]) and not np.array_equal(same[3], ref[3])
    sg.disable_bcr()
    one_step(sg, BATCH, 608)
    one_step(sg, BATCH, 609)
    assert sg.graph_active and "errD_cr_real" not in sg.loss_terms


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_checkpoint_resume_mid_run(tmp_path, graph):
    """saved after 2 steps with everything on (every = 2), loaded into a bare trainer from another fill, 2 more steps: bit-identical
    to the uninterrupted run, the regulariser's generator and count of updates included"""
    from tests.common import build_hip_nets
    path = tmp_path / "bcr.pt"
    saved = {}

    def build_a():
        return _everything(2, every=2, graph=graph, nets=build_hip_nets("T", seed=0))

    def build_b():
        from srgan_amd import spectral
        sg = make_trainer("T", BATCH, K, 31, nets=build_hip_nets("T", seed=5))
        torch.manual_seed(18)
        spectral.spectral_norm(sg.D)           # part of building D; the checkpoint turns everything else on
        return sg.enable_graph() if graph else sg

    a = run_a(build_a, path, 2, 2, at_save=lambda sg: saved.update(sg.bcr_stats()))
    assert saved["updates"] == 2 and saved["every"] == 2
    b = run_b(build_b, path, 2, 2)
    (sg_a, rows_a, state_a), (sg_b, rows_b, state_b) = a, b
    assert_rows_equal(rows_a, rows_b, "bcr resume")
    assert_state_equal(state_a, state_b, "bcr resume")
    assert sg_a.bcr_stats() == sg_b.bcr_stats() and sg_b.bcr_stats()["updates"] == 4
    assert (sg_b.bcr.lambda_real, sg_b.bcr.lambda_fake, sg_b.bcr.stage.policy, sg_b.bcr.stage.translation) == (5.0, 2.0, "flip,translation", 0.125)
    assert torch.equal(sg_a.bcr.stage.generator.get_state(), sg_b.bcr.stage.generator.get_state())
    assert sg_a.graph_active == sg_b.graph_active == graph


def test_bf16_compute_mode_step():
    """maps and images are fp32 in this mode too: the two terms are the restated ones on the maps D produced, at the bound of the
    fused loss (tests/test_cr_kernels_gpu.py), and every loss term is finite"""
    from srgan_amd import ops
    ops.set_compute_dtype("bf16")
    try:
        sg = _bcr_trainer(7)
        seen = _record_outs(sg)
        torch.manual_seed(350)
        out = one_step(sg, BATCH, 350)
        assert all(o.dtype == torch.float32 for outs in seen for o in outs)
        assert all(np.isfinite(out)) and all(np.isfinite(v) for v in _terms(sg).values())
        outs = [o.cpu().double() for o in seen[K - 1]]                       # the step's last penalised update
        assert [o.shape[0] for o in outs] == [4 * BATCH] * 2
        vals = cc.loss_vals(outs, [], None, rows_first=BATCH, t_first=1.0, t_rest=0.0, w_class=0.0, lam_real=5.0, lam_fake=2.0, every=1,
                            gan_kind=0, class_kind=0, pairs_first=BATCH)
        outs32 = [o.float() for o in outs]
        vals32 = cc.loss_vals(outs32, [], None, rows_first=BATCH, t_first=1.0, t_rest=0.0, w_class=0.0, lam_real=5.0, lam_fake=2.0,
                              every=1, gan_kind=0, class_kind=0, pairs_first=BATCH)
        from tests import small_common as sc
        L = cc.loss_L(2 * BATCH, [o[0].numel() for o in outs])
        for i, name in ((4, "errD_cr_real"), (5, "errD_cr_fake"), (0, "errD_real"), (2, "errD_fake")):
            sc.check("d_losses_cr", f"bf16 step {name}", sg.loss_terms[name].reshape(()), vals[i], vals32[i], L)
    finally:
        ops.set_compute_dtype("fp32")
        ops.invalidate_packed()


def test_refusals_name_the_way_out(monkeypatch):
    from srgan_amd import consistency, dp, ops
    from srgan_amd.trainer import SingleGAN_training
    from tests.step_bits_common import PlainD
    sg = make_trainer("T", BATCH, K, 4)
    for bad, what in ((dict(lambda_real=-1.0), "lambda_real"), (dict(lambda_fake=float("nan")), "lambda_fake"), (dict(every=0), "every"),
                      (dict(policy="rot90"), "unknown policy entry"), (dict(translation=-0.5), "translation")):
        with pytest.raises(ValueError, match=what):
            sg.enable_bcr(**bad)
    with pytest.raises(RuntimeError, match="enable_bcr"):
        sg.set_bcr_weights(1.0, 1.0)
    with pytest.raises(NotImplementedError, match="SRGAN_training.enable_bcr"):
        SingleGAN_training.enable_bcr(object())
    monkeypatch.setattr(dp, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="2 ranks.*disable_bcr"):
        sg.enable_bcr()
    monkeypatch.undo()
    assert sg.bcr is None
    # the generic discriminator path: at enable_bcr, and when the step runs
    generic = make_trainer("T", BATCH, K, 4)
    generic.D = PlainD(generic.D)
    with pytest.raises(NotImplementedError, match="fused discriminator pass.*disable_bcr"):
        generic.enable_bcr()
    sg.enable_bcr()
    sg.D = PlainD(sg.D)
    _, _, dev = _cuda_batch(50)
    with pytest.raises(NotImplementedError, match="fused discriminator pass.*disable_bcr"):
        sg.train(*dev)
    # a first use inside a capture must not allocate
    fresh = consistency.BalancedCR()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="inside a hipGraph capture"):
        with torch.cuda.graph(g):
            fresh._ensure(torch.device("cuda"))
    assert ops.get_compute_dtype() == "fp32"
