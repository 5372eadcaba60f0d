"""GPU: mode-seeking regularisation inside the train step (SRGAN_training.enable_mode_seeking) at tier T, 128 x 128, batch 4, k = 2 --
the step against the CPU oracle with the term (tests/ms_common.MSOracle), off means untouched, the launches, the fallback forward,
composition with every other extension, graph mode, checkpoints, the bf16 compute mode, the refusals and the evaluation score."""
import numpy as np
import pytest
import torch

from oracle import trainer as otrainer
from tests import ms_common as mc
from tests.checkpoint_common import assert_rows_equal, assert_state_equal, run_a, run_b
from tests.common import close_params, oracle_params
from tests.ema_common import assert_same, live_state, make_trainer, one_step, steps
from tests.step_bits_common import _launch_counts
from tests.test_train_gpu import TERM_PAIRS

pytestmark = pytest.mark.gpu
BATCH, K, SIZE = 4, 2, 128
SN_SEED = 77
NEW_KERNELS = ("ms_rows_kernel", "ms_finish_kernel", "ms_grad_kernel")


def _terms(sg):
    return {k: float(v) for k, v in sg.loss_terms.items()}


def _cuda_batch(seed):
    x, label = otrainer.synthetic_batch(BATCH, SIZE, 4, seed=seed)
    return x, label, (x.cuda(), {"source": label["source"].cuda(), "target": label["target"]})


def _kw(form):
    return dict(weight=mc.LAMBDA_ACTS[form], form=form, tau=mc.DSGAN_TAU if form == "dsgan" else None, seed=mc.MS_SEED)


@pytest.fixture(scope="module")
def plain_step():
    """the plain HIP step at the oracle test's seeds: (trainer, returned losses, the default generator's state after it)"""
    _, _, dev = _cuda_batch(mc.TRAIN_BATCH_SEED)
    sg = make_trainer("T", BATCH, K, mc.TRAIN_SEED)
    out = [float(v) for v in sg.train(*dev)]
    return sg, out, torch.get_rng_state()


@pytest.mark.parametrize("form", mc.FORMS)
def test_step_vs_the_oracle_with_the_term(plain_step, form):
    """the three losses and every loss term at 1e-3, errG_ms at the tolerance fixed in tests/test_ms_refs_cpu.py, the parameters by
    close_params; errG is the value without the term; G leaves the plain step's G, D's first update does not"""
    x, label, dev = _cuda_batch(mc.TRAIN_BATCH_SEED)
    PG, PD, PE = oracle_params("T")
    torch.manual_seed(mc.TRAIN_SEED)
    orc = mc.MSOracle(PG, PD, PE, otrainer.DEFAULT_LBD, K, np.eye(4), BATCH, "mu", 8, **_kw(form))
    ref = [float(v) for v in orc.train(x, label)]
    sg = make_trainer("T", BATCH, K, mc.TRAIN_SEED)
    sg.enable_mode_seeking(**_kw(form))
    out = [float(v) for v in sg.train(*dev)]
    plain, out0, rng_after = plain_step
    assert torch.equal(torch.get_rng_state(), rng_after)          # the default generator: the same with the feature on and off
    np.testing.assert_allclose(out, ref, rtol=1e-3)
    t, tr = _terms(sg), orc.trace
    for a, b in TERM_PAIRS:
        assert abs(t[a] - tr[b]) <= 1e-3 * max(abs(tr[b]), 1e-3), (a, t[a], tr[b])
    for j, name in enumerate(("errD_real", "errD_class", "errD_fake")):
        want = tr["errD_parts"][-1][j]
        assert abs(t[name] - want) <= 1e-3 * max(abs(want), 1e-3), (name, t[name], want)
    st = sg.mode_seeking_stats()
    print(f"{form}: errG_ms {t['errG_ms']:.9g} oracle {tr['ms']:.9g} rel {abs(t['errG_ms'] - tr['ms']) / abs(tr['ms']):.3e}; "
          f"d_image {st['d_image']:.6g} / {tr['d_image']:.6g}, d_latent {st['d_latent']:.6g} / {tr['d_latent']:.6g}")
    assert abs(t["errG_ms"] - tr["ms"]) <= mc.ERRG_MS_RTOL * abs(tr["ms"])
    assert abs(st["d_image"] - tr["d_image"]) <= 1e-3 * tr["d_image"] and abs(st["d_latent"] - tr["d_latent"]) <= 1e-5 * tr["d_latent"]
    assert st["ms"] == t["errG_ms"] and st["updates"] == 1 and st["form"] == form and st["weight"] == mc.LAMBDA_ACTS[form]
    for net, P, n_opt in ((sg.G, orc.G, 2), (sg.D, orc.D, K), (sg.E, orc.E, 1)):
        for key, v in net.state_dict().items():
            close_params(v, P[key], 1e-4, n_opt, what=key)
    # the returned errG: phase 1's sum WITHOUT the term (bit for bit the plain step's: nothing of the term has been used yet) plus
    # phase 2's, which G's changed step moves -- the first-phase terms are the plain step's bits, and errD / errE are
    t0 = _terms(plain)
    assert "errG_ms" not in t0 and plain.mode_seeking_stats() is None
    for name in ("errG_dis", "errG_class", "errE_bKL", "errE_corr", "errE_hist", "errD_real", "errD_fake"):
        assert t[name] == t0[name], name
    for name in ("errG_cycle", "errG_idt"):            # rows of a 3B batch instead of a 2B one: the same value, not pinned to the bit
        assert abs(t[name] - t0[name]) <= 1e-6 * t0[name], name
    assert out[1] == out0[1] and abs(out[2] - out0[2]) <= 1e-6 * abs(out0[2])
    L = otrainer.DEFAULT_LBD
    p1 = t["errG_dis"] + L["class"] * t["errG_class"] + L["cycle"] * t["errG_cycle"] + L["idt"] * t["errG_idt"]
    p2 = L["reg"] * t["errG_reg"] + L["idt_reg"] * (L["idt"] / L["cycle"]) * t["errG_idt_reg"]
    assert abs(out[0] - (p1 + p2)) <= 1e-5 * abs(out[0])          # the term is not in it (it would add weight * ms = 3.7 / 277)
    assert torch.equal(torch.cat([p.flatten() for p in sg.D.parameters()]), torch.cat([p.flatten() for p in plain.D.parameters()]))
    moved = []
    for key, v in sg.G.state_dict().items():
        try:
            close_params(v, plain.G.state_dict()[key], 1e-4, 2, what=key)
        except AssertionError:
            moved.append(key)
    assert moved, "the regularised step left G within close_params of the plain step: the term does not act"


def test_enabled_then_disabled_equals_a_fresh_trainer():
    a = make_trainer("T", BATCH, K, 2)
    ref = steps(a, BATCH, 2, 300)
    b = make_trainer("T", BATCH, K, 2)
    b.enable_mode_seeking(weight=3.0, seed=1)
    assert b.mode_seeking_stats()["updates"] == 0
    b.disable_mode_seeking()
    assert b.mode_seeking_stats() is None
    got = steps(b, BATCH, 2, 300)
    np.testing.assert_array_equal(got, ref)
    assert_same(live_state(a), live_state(b))
    assert _terms(a) == _terms(b) and "errG_ms" not in b.loss_terms and "mode_seeking" not in b.state_dict(rng=False)


def _step_launches(sg, seed):
    from srgan_amd import _lib
    lib = _lib.load()
    torch.manual_seed(seed)
    torch.cuda.synchronize()
    lib.srgan_prof_enable(1)
    try:
        one_step(sg, BATCH, seed)
        torch.cuda.synchronize()
    finally:
        lib.srgan_prof_enable(0)
    return _launch_counts(lib)


def test_launches_three_new_kernels_and_nothing_else_where_i2_rides_the_batched_forward():
    def build(on):
        sg = make_trainer("T", BATCH, K, 3)
        if on:
            sg.enable_mode_seeking(seed=6)
        torch.manual_seed(360)
        one_step(sg, BATCH, 360)
        return sg

    want = _step_launches(build(False), 361)
    assert want and not any(k in want for k in NEW_KERNELS)
    got = _step_launches(build(True), 361)
    new = {k: got.pop(k) for k in NEW_KERNELS}
    assert new == dict(ms_rows_kernel=1, ms_finish_kernel=1, ms_grad_kernel=1) and sum(new.values()) <= 3
    # every other kernel: the plain step's NUMBER of launches (phase 1's generator pass runs on 3B rows instead of 2B, so a
    # convolution may take another tile shape: the total and every non-convolution kernel are pinned)
    assert sum(got.values()) == sum(want.values()), (got, want)
    free = ("igemm", "wino", "halo", "rgb", "wgrad")
    assert {k: v for k, v in got.items() if not any(f in k for f in free)} == \
        {k: v for k, v in want.items() if not any(f in k for f in free)}


def test_fallback_forward_gives_the_same_term():
    """lbd["idt"] = 0: no batched phase-1 forward, I2 takes a forward of its own; per-sample network and the same kernels, so errG_ms
    of the first step is the same bits as with I2 riding (where idt only adds rows to the batch)"""
    def run(idt, ride=True):
        sg = make_trainer("T", BATCH, K, 4)
        if not idt:
            sg.lbd["idt"] = 0.0
        if not ride:
            sg._ms_rides = lambda nb, src: False
        sg.enable_mode_seeking(seed=8)
        torch.manual_seed(380)
        out = one_step(sg, BATCH, 380)
        assert all(np.isfinite(out))
        return _terms(sg)["errG_ms"], sg.mode_seeking_stats()

    rides, st_r = run(True)
    own, st_o = run(True, ride=False)                            # the 4 GiB guard's fallback, forced
    no_pair, st_n = run(False)                                   # no pair path at all
    print(f"errG_ms riding {rides:.9g}, own forward {own:.9g}, without the pair path {no_pair:.9g}")
    assert abs(own - rides) <= 1e-6 * abs(rides) and abs(no_pair - rides) <= 1e-6 * abs(rides)
    assert st_r["updates"] == st_o["updates"] == st_n["updates"] == 1


def _everything(seed, ms=True, form="msgan", graph=False, nets=None):
    from srgan_amd import spectral
    sg = make_trainer("T", BATCH, K, seed, nets=nets)
    torch.manual_seed(SN_SEED)
    spectral.spectral_norm(sg.D)
    sg.enable_grad_guard(max_norm=1.0)
    sg.enable_ema()
    sg.enable_diffaugment(seed=9).enable_geometric_augment(seed=10)
    sg.enable_ada(target=0.1, interval=1, kimg=BATCH / (0.125 * 1000.0), p=0.5)
    sg.enable_r1(gamma=10.0, every=2)
    sg.enable_bcr(lambda_real=5.0, lambda_fake=2.0, every=2, seed=11)
    if ms:
        sg.enable_mode_seeking(weight=0.5, form=form, tau=2.0 if form == "dsgan" else None, seed=12)
    return sg.enable_graph() if graph else sg


def test_composition_with_every_other_extension():
    """EMA + spectral norm + DiffAugment + geometric stage + ADA + R1 + bCR + gradient guard + mode seeking: one step runs and is
    finite; the other extensions' generators, tables and counters are what they are without mode seeking (D never sees the term)"""
    sg = _everything(7)
    torch.manual_seed(370)
    out = one_step(sg, BATCH, 370)
    assert all(np.isfinite(out)) and all(np.isfinite(v) for v in _terms(sg).values())
    assert _terms(sg)["errG_ms"] > 0 and sg.mode_seeking_stats()["updates"] == 1
    default_after = torch.get_rng_state()
    other = _everything(7, ms=False)
    torch.manual_seed(370)
    one_step(other, BATCH, 370)
    assert torch.equal(torch.get_rng_state(), default_after)
    assert torch.equal(sg.augment.generator.get_state(), other.augment.generator.get_state())
    assert torch.equal(sg.geometry.generator.get_state(), other.geometry.generator.get_state())
    assert torch.equal(sg.bcr.stage.generator.get_state(), other.bcr.stage.generator.get_state())
    assert sg.ada_stats() == other.ada_stats() and sg.r1_stats() == other.r1_stats() and sg.bcr_stats() == other.bcr_stats()
    assert sg.ema_updates == other.ema_updates == 1
    for name in ("errD_real", "errD_fake", "errD_class", "errD_r1", "errD_cr_real", "errD_cr_fake", "ada_p"):
        assert _terms(sg)[name] == _terms(other)[name], name
    from srgan_amd.diversity import ModeSeeking
    ref = ModeSeeking(seed=12)
    ref.draw(BATCH, 8)
    assert torch.equal(sg._ms.generator.get_state(), ref.generator.get_state())         # one draw per step


def _ms_trainer(seed, extras=False, form="msgan"):
    if extras:
        return _everything(seed, form=form)
    return make_trainer("T", BATCH, K, seed).enable_mode_seeking(weight=0.5, form=form, tau=2.0 if form == "dsgan" else None, seed=12)


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
    form = "dsgan" if extras else "msgan"
    eager = _ms_trainer(2, extras, form)
    ref = steps(eager, BATCH, 4, 500)
    sg = _ms_trainer(2, extras, form).enable_graph()
    got = steps(sg, BATCH, 4, 500)
    assert sg.graph_active
    assert tuple(sg._graph.tables("mode_seeking").shape) == (1, BATCH, 8)          # z2: one draw per step, beside the stages' tables
    np.testing.assert_array_equal(got, ref)
    assert _terms(sg) == _terms(eager)
    assert_same(_state(eager, extras), _state(sg, extras))
    a, b = eager.mode_seeking_stats(), sg.mode_seeking_stats()
    assert a == b and a["updates"] == 4 and a["ms"] != 0
    assert float(sg.loss_terms["errG_ms"]) == b["ms"]
    assert torch.equal(sg._ms.generator.get_state(), eager._ms.generator.get_state())


def test_set_weight_keeps_the_recording_and_a_new_form_drops_it():
    def change(t, s):
        if s == 2:
            t.set_mode_seeking_weight(20.0)
            if t._graph is not None:
                assert t.graph_active                 # the weight is device state
        if s == 4:
            t.enable_mode_seeking(weight=20.0, form="dsgan", tau=2.0, seed=13)

    eager = _ms_trainer(3)
    ref = steps(eager, BATCH, 8, 600, after=change)
    sg = _ms_trainer(3).enable_graph()
    got = [steps(sg, BATCH, 3, 600, after=change)]
    got.append(np.array([one_step(sg, BATCH, 603)]))
    assert sg.graph_active and sg.mode_seeking_stats()["weight"] == 20.0          # still the first recording, reading the new weight
    got.append(np.array([one_step(sg, BATCH, 604)]))
    change(sg, 4)
    assert not sg.graph_active                            # another form: dropped
    got.append(np.array([one_step(sg, BATCH, 605)]))
    assert not sg.graph_active                            # this step ran eagerly ...
    got.append(np.array([one_step(sg, BATCH, 606)]))
    assert sg.graph_active                                # ... and the step was recorded again
    got.append(np.array([one_step(sg, BATCH, 607)]))
    got = np.concatenate(got)
    np.testing.assert_array_equal(got, ref)
    assert_same(live_state(eager), live_state(sg))
    assert eager.mode_seeking_stats() == sg.mode_seeking_stats() and sg.mode_seeking_stats()["form"] == "dsgan"
    assert sg.mode_seeking_stats()["updates"] == 3
    # the new weight changed the step that followed it: an uninterrupted run from the same seeds ends elsewhere
    same = steps(_ms_trainer(3), BATCH, 4, 600)
    assert np.array_equal(same[:3], ref[:3]) and not np.array_equal(same[3], ref[3])
    sg.disable_mode_seeking()
    one_step(sg, BATCH, 608)
    one_step(sg, BATCH, 609)
    assert sg.graph_active and "errG_ms" not in sg.loss_terms


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_checkpoint_resume_mid_run(tmp_path, graph):
    """saved after 2 steps with everything on, loaded into a bare trainer from another fill, 2 more steps: bit-identical to the
    uninterrupted run, the regulariser's generator, counter and last values included"""
    from tests.common import build_hip_nets
    path = tmp_path / "ms.pt"
    saved = {}

    def build_a():
        return _everything(2, form="dsgan", graph=graph, nets=build_hip_nets("T", seed=0))

    def build_b():
        from srgan_amd import spectral
        sg = make_trainer("T", BATCH, K, 31, nets=build_hip_nets("T", seed=5))
        torch.manual_seed(18)
        spectral.spectral_norm(sg.D)           # part of building D; the checkpoint turns everything else on
        return sg.enable_graph() if graph else sg

    a = run_a(build_a, path, 2, 2, at_save=lambda sg: saved.update(sg.mode_seeking_stats()))
    assert saved["updates"] == 2 and saved["form"] == "dsgan" and saved["ms"] != 0
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert sd["mode_seeking"]["updates"] == 2 and sd["mode_seeking"]["ms"] == saved["ms"]
    fresh = make_trainer("T", BATCH, K, 31, nets=build_hip_nets("T", seed=5))
    torch.manual_seed(18)
    from srgan_amd import spectral
    spectral.spectral_norm(fresh.D)
    fresh.load_checkpoint(path)
    assert fresh.mode_seeking_stats() == saved            # the record's last values come back before any step
    b = run_b(build_b, path, 2, 2)
    (sg_a, rows_a, state_a), (sg_b, rows_b, state_b) = a, b
    assert_rows_equal(rows_a, rows_b, "mode seeking resume")
    assert_state_equal(state_a, state_b, "mode seeking resume")
    assert sg_a.mode_seeking_stats() == sg_b.mode_seeking_stats() and sg_b.mode_seeking_stats()["updates"] == 4
    assert torch.equal(sg_a._ms.generator.get_state(), sg_b._ms.generator.get_state())
    assert sg_a.graph_active == sg_b.graph_active == graph


def test_checkpoint_without_the_section_loads_as_missing(tmp_path):
    path = tmp_path / "plain.pt"
    a = make_trainer("T", BATCH, K, 2)
    one_step(a, BATCH, 700)
    a.save_checkpoint(path)
    b = make_trainer("T", BATCH, K, 3).enable_mode_seeking(seed=1)
    with pytest.raises(ValueError, match="missing.*mode_seeking"):
        b.load_checkpoint(path)
    rep = b.load_checkpoint(path, strict=False)
    assert rep.missing == ["mode_seeking"] and rep.unexpected == []
    assert b.mode_seeking_stats()["updates"] == 0
    out = one_step(b, BATCH, 701)
    assert all(np.isfinite(out)) and b.mode_seeking_stats()["updates"] == 1


def test_bf16_compute_mode_step():
    """the generator's output is fp32 in this mode too; one step is finite and within the mode's trajectory bound (1e-2 on the three
    losses and every loss term, tests/test_train_gpu.py) of the fp32 step"""
    from srgan_amd import ops

    def run():
        sg = _ms_trainer(7)
        torch.manual_seed(350)
        out = one_step(sg, BATCH, 350)
        assert sg.target_image.dtype == torch.float32
        return out, _terms(sg)

    ref, t32 = run()
    ops.set_compute_dtype("bf16")
    try:
        out, t16 = run()
    finally:
        ops.set_compute_dtype("fp32")
        ops.invalidate_packed()
    assert all(np.isfinite(out)) and all(np.isfinite(v) for v in t16.values())
    np.testing.assert_allclose(out, ref, rtol=1e-2)
    for name, want in t32.items():
        assert abs(t16[name] - want) <= 1e-2 * max(abs(want), 1e-3), (name, t16[name], want)


def test_refusals_name_the_way_out(monkeypatch):
    from srgan_amd import diversity, dp, ops
    from srgan_amd.trainer import SingleGAN_training
    from tests import step_bits_common as sb
    sg = make_trainer("T", BATCH, K, 4)
    for bad, what in ((dict(weight=-1.0), "weight"), (dict(eps=0.0), "eps"), (dict(form="dsgan"), "tau"), (dict(form="hinge"), "form")):
        with pytest.raises(ValueError, match=what):
            sg.enable_mode_seeking(**bad)
    with pytest.raises(RuntimeError, match="enable_mode_seeking"):
        sg.set_mode_seeking_weight(1.0)
    with pytest.raises(NotImplementedError, match="SRGAN_training.enable_mode_seeking"):
        SingleGAN_training.enable_mode_seeking(object())
    monkeypatch.setattr(dp, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="2 ranks.*disable_mode_seeking"):
        sg.enable_mode_seeking()
    monkeypatch.undo()
    assert sg.mode_seeking_stats() is None
    # more than one rank when the step runs
    sg.enable_mode_seeking()
    monkeypatch.setattr(dp, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="2 ranks.*disable_mode_seeking"):
        sg._ms_check()
    monkeypatch.undo()
    bn = sb.make_trainer("batch_norm")
    with pytest.raises(NotImplementedError, match="batch statistics.*disable_mode_seeking"):
        bn.enable_mode_seeking()
    assert bn.mode_seeking_stats() is None
    # a first use inside a capture must not allocate
    fresh = diversity.ModeSeeking()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="inside a hipGraph capture"):
        with torch.cuda.graph(g):
            fresh._ensure(torch.device("cuda"))
    assert ops.get_compute_dtype() == "fp32"


def test_style_diversity_score():
    from srgan_amd import evaluation
    rng = np.random.default_rng(5)
    x = (rng.integers(-8, 9, (3, 4, 3, 16, 16)) / 8.0).astype(np.float32)
    import math
    rows = [np.abs(x[i, n].astype(np.float64) - x[j, n]).mean() for n in range(4) for i in range(3) for j in range(i + 1, 3)]
    want = math.fsum(rows) / len(rows)                 # the exactly rounded sum of the 12 float64 row means, over their number
    assert abs(want - np.mean(rows)) <= 2.0 ** -52 * want
    got = evaluation.compute_style_diversity(torch.tensor(x).cuda())
    assert isinstance(got, float) and got == want
    with pytest.raises(ValueError, match="at least 2"):
        evaluation.compute_style_diversity(torch.tensor(x[:1]).cuda())
    ev = evaluation.GAN_evaluation.__new__(evaluation.GAN_evaluation)
    ev.device = "cuda"
    assert ev.get_diversity(torch.tensor(x)) == got
