"""GPU: LeCam regularisation inside the train step (SRGAN_training.enable_lecam) at tier T, 128 x 128, batch 4, k = 2 -- the step
against the CPU oracle with the term (tests/lecam_common.LeCamOracle), off and inactive mean bit-identical to the plain step, the
launches of an update, composition with every other extension, graph mode across the ``start`` boundary, checkpoints, the bf16
compute mode and the refusals."""
import numpy as np
import pytest
import torch

from oracle import trainer as otrainer
from tests import lecam_common as lc
from tests.checkpoint_common import assert_rows_equal, assert_state_equal, run_a, run_b
from tests.common import close_params, oracle_params
from tests.ema_common import assert_same, live_state, make_trainer, one_step, steps
from tests.step_bits_common import _launch_counts
from tests.test_train_gpu import TERM_PAIRS

pytestmark = pytest.mark.gpu
BATCH, K, SIZE = 4, 2, 128
W = lc.LC_WEIGHT
SN_SEED = 77


def _terms(sg):
    return {k: float(v) for k, v in sg.loss_terms.items()}


def _cuda_batch(seed):
    x, label = otrainer.synthetic_batch(BATCH, SIZE, 4, seed=seed)
    return x, label, (x.cuda(), {"source": label["source"].cuda(), "target": label["target"]})


@pytest.mark.parametrize("clamp", [False, True], ids=["identity", "relu"])
def test_three_steps_vs_the_oracle_with_the_term(clamp):
    """the three losses and every loss term of each of 3 steps, R, the anchors and the parameters after them at the trajectory
    tolerance of test_train_gpu (1e-3; close_params); start = 0"""
    seed, n_steps = 5, 3
    PG, PD, PE = oracle_params("T")
    torch.manual_seed(seed)
    orc = lc.LeCamOracle(PG, PD, PE, otrainer.DEFAULT_LBD, K, np.eye(4), BATCH, "mu", 8, weight=W, decay=0.9, start=0, clamp=clamp)
    refs, traces = [], []
    for step in range(n_steps):                          # the oracle's run first: both draw the noise from the CPU generator
        x, label, _ = _cuda_batch(42 + step)
        refs.append([float(v) for v in orc.train(x, label)])
        traces.append(orc.trace)
    sg = make_trainer("T", BATCH, K, seed).enable_lecam(weight=W, decay=0.9, start=0, clamp=clamp)
    for step in range(n_steps):
        out = [float(v) for v in sg.train(*_cuda_batch(42 + step)[2])]
        np.testing.assert_allclose(out, refs[step], rtol=1e-3, err_msg=f"step {step}")
        t, tr = _terms(sg), traces[step]
        for a, b in TERM_PAIRS:
            assert abs(t[a] - tr[b]) <= 1e-3 * max(abs(tr[b]), 1e-3), (step, a, t[a], tr[b])
        want = tr["errD_lecam"][-1]
        print(f"clamp {clamp} step {step} errD_lecam {t['errD_lecam']:.9g} oracle {want:.9g}")
        assert want > 0 and abs(t["errD_lecam"] - want) <= 1e-3 * want, (step, t["errD_lecam"], want)
    stats = sg.lecam_stats()
    assert stats["updates"] == n_steps * K == orc.lc["updates"] and stats["applied"] == 1 and stats["clamp"] is clamp
    assert stats["penalty"] == t["errD_lecam"]
    for s in range(2):
        for name in ("a_real", "a_fake"):
            want = orc.lc[name][s]
            assert abs(stats[name][s] - want) <= 1e-3 * max(abs(want), 1e-3), (name, s, stats[name][s], want)
    assert stats["a_real"][2:] == [0.0, 0.0] and stats["a_fake"][2:] == [0.0, 0.0]
    for net, P, n_opt in ((sg.G, orc.G, 2 * n_steps), (sg.D, orc.D, K * n_steps), (sg.E, orc.E, n_steps)):
        for key, v in net.state_dict().items():
            close_params(v, P[key], 1e-4, n_opt, what=key, walk=True)


def test_enabled_then_disabled_equals_a_fresh_trainer():
    a = make_trainer("T", BATCH, K, 2)
    ref = steps(a, BATCH, 2, 300)
    b = make_trainer("T", BATCH, K, 2)
    b.enable_lecam(weight=3.0, clamp=True)
    assert b._lecam is not None and b.lecam_stats()["updates"] == 0
    b.disable_lecam()
    assert b._lecam is None and b.lecam_stats() is None
    got = steps(b, BATCH, 2, 300)
    np.testing.assert_array_equal(got, ref)
    assert_same(live_state(a), live_state(b))
    assert _terms(a) == _terms(b) and "errD_lecam" not in b.loss_terms


def test_a_zero_weight_and_the_warm_up_leave_the_plain_steps_bits():
    """weight = 0: every parameter bit-identical to the plain trainer after 2 steps while the anchors moved; start = 3 with k = 2:
    step 1 (updates 0, 1) bit-identical to plain, step 2 (update 3 is applied) differs"""
    plain = make_trainer("T", BATCH, K, 2)
    ref = steps(plain, BATCH, 1, 300)
    state1 = live_state(plain)
    torch.manual_seed(301)
    ref = np.concatenate([ref, [one_step(plain, BATCH, 301)]])
    state2 = live_state(plain)

    zero = make_trainer("T", BATCH, K, 2).enable_lecam(weight=0.0)
    got = steps(zero, BATCH, 1, 300)
    torch.manual_seed(301)
    got = np.concatenate([got, [one_step(zero, BATCH, 301)]])
    np.testing.assert_array_equal(got, ref)
    assert_same(state2, live_state(zero))
    st = zero.lecam_stats()
    assert st["updates"] == 2 * K and st["applied"] == 0 and all(st["a_real"][:2]) and all(st["a_fake"][:2]) and st["penalty"] > 0
    assert float(zero.loss_terms["errD_lecam"]) == st["penalty"]

    warm = make_trainer("T", BATCH, K, 2).enable_lecam(weight=W, start=3)
    got = steps(warm, BATCH, 1, 300)
    np.testing.assert_array_equal(got, ref[:1])
    assert_same(state1, live_state(warm))
    assert warm.lecam_stats()["applied"] == 0 and warm.lecam_stats()["updates"] == 2
    torch.manual_seed(301)
    one_step(warm, BATCH, 301)
    st = warm.lecam_stats()
    assert st["applied"] == 1 and st["updates"] == 4
    now = live_state(warm)
    assert any(not torch.equal(now[k], state2[k]) for k in now if k.startswith("D."))


def _update_launches(sg, index=0):
    """{kernel: launches} of ONE discriminator update of a trainer that has run a step"""
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


def test_the_timed_launches_of_an_update_are_the_plain_updates():
    """the new kernel is untimed by design (as d_losses_kernel): what the launch timer sees must not change, and the list of timed
    kernels is the one tests/test_abi_cpu.py pins"""
    def build(on):
        sg = make_trainer("T", BATCH, K, 3)
        if on:
            sg.enable_lecam(weight=W)
        torch.manual_seed(360)
        one_step(sg, BATCH, 360)
        return sg

    plain, sg = build(False), build(True)
    want = _update_launches(plain)
    assert want and _update_launches(sg) == want
    assert sg.lecam_stats()["updates"] == K + 1
    from srgan_amd import _lib
    lib = _lib.load()
    assert not any("lecam" in lib.srgan_prof_kernel_name(k).decode() for k in range(lib.srgan_prof_num_kernels()))


def _everything(seed, lecam=True, graph=False, nets=None, start=0):
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
    sg.enable_mode_seeking(weight=0.5, seed=12)
    if lecam:
        sg.enable_lecam(weight=W, decay=0.9, start=start, clamp=True)
    return sg.enable_graph() if graph else sg


def test_composition_with_every_other_extension():
    """DiffAugment + geometric stage + ADA + R1 + bCR (every = 2: one update with 4B rows, one with 2B) + spectral norm + mode seeking
    + gradient guard + EMA + LeCam: the run ends finite, errD is the value without the term (update 0 of the step has seen none of
    its gradients: the returned errD of the first update equals the run without LeCam bit for bit), the other features' records
    are what they are without it"""
    sg = _everything(7)
    torch.manual_seed(370)
    x, label, dev = _cuda_batch(370)
    errs = []
    orig = sg.update_D

    def spy(*a, **kw):
        out = orig(*a, **kw)
        errs.append(float(out[0] if isinstance(out, tuple) else out))
        return out

    sg.update_D = spy
    out = [float(v) for v in sg.train(*dev)]
    assert all(np.isfinite(out)) and all(np.isfinite(v) for v in _terms(sg).values())
    t = _terms(sg)
    assert t["errD_lecam"] > 0 and t["errD_cr_real"] > 0 and t["errD_r1"] > 0 and "errG_ms" in t
    st = sg.lecam_stats()
    assert st["updates"] == K and st["applied"] == 1 and st["penalty"] == t["errD_lecam"]
    other = _everything(7, lecam=False)
    errs0, orig0 = [], other.update_D

    def spy0(*a, **kw):
        out = orig0(*a, **kw)
        errs0.append(float(out[0] if isinstance(out, tuple) else out))
        return out

    other.update_D = spy0
    torch.manual_seed(370)
    other.train(*dev)
    assert len(errs) == len(errs0) == K and errs[0] == errs0[0] and errs[1] != errs0[1]
    assert sg.bcr_stats()["updates"] == other.bcr_stats()["updates"] == 1 and sg.r1_stats()["updates"] == 1
    assert torch.equal(sg.augment.generator.get_state(), other.augment.generator.get_state())
    assert torch.equal(sg.bcr.stage.generator.get_state(), other.bcr.stage.generator.get_state())


def _lc_trainer(seed, start=3, clamp=False):
    return make_trainer("T", BATCH, K, seed).enable_lecam(weight=W, decay=0.9, start=start, clamp=clamp)


def test_graph_replay_is_bit_identical_to_eager_across_the_start_boundary():
    """one eager warm-up step (updates 0, 1), then three replays of one recording: start = 3 is crossed inside the first replay by the
    device record alone"""
    eager = _lc_trainer(2)
    ref = steps(eager, BATCH, 4, 500)
    sg = _lc_trainer(2).enable_graph()
    seen = []
    got = steps(sg, BATCH, 4, 500, after=lambda t, s: seen.append((t.graph_active, t.lecam_stats()["applied"], t.lecam_stats()["updates"])))
    assert sg.graph_active
    assert seen == [(False, 0, 2), (True, 1, 4), (True, 1, 6), (True, 1, 8)]
    np.testing.assert_array_equal(got, ref)
    assert _terms(sg) == _terms(eager)
    assert_same(live_state(eager), live_state(sg))
    assert eager.lecam_stats() == sg.lecam_stats()
    assert float(sg.loss_terms["errD_lecam"]) == sg.lecam_stats()["penalty"]
    # the term acted from update 3 on: the plain run from the same seeds ends elsewhere, and agrees on step 1
    plain = steps(make_trainer("T", BATCH, K, 2), BATCH, 2, 500)
    assert np.array_equal(plain[0], ref[0]) and not np.array_equal(plain[1], ref[1])


def test_set_lecam_keeps_the_recording_and_enable_disable_or_a_new_clamp_drop_it():
    def change(t, s):
        if s == 2:
            t.set_lecam(weight=2 * W, decay=0.5)
        if s == 4:
            t.enable_lecam(weight=W, decay=0.9, start=0, clamp=True)

    eager = _lc_trainer(3, start=0)
    ref = steps(eager, BATCH, 7, 600, after=change)
    sg = _lc_trainer(3, start=0).enable_graph()
    active = []

    def change_and_watch(t, s):
        before = t.graph_active
        change(t, s)
        active.append((s, before, t.graph_active))

    got = steps(sg, BATCH, 7, 600, after=change_and_watch)
    # s = 2: set_lecam between replays keeps the recording; s = 4: a new object with another clamp drops it; step 5 runs eagerly,
    # step 6 records again
    assert active == [(0, False, False), (1, True, True), (2, True, True), (3, True, True), (4, True, False), (5, False, False),
                      (6, True, True)]
    np.testing.assert_array_equal(got, ref)
    assert_same(live_state(eager), live_state(sg))
    st = sg.lecam_stats()
    assert st == eager.lecam_stats() and st["clamp"] is True and st["updates"] == 2 * K
    same = steps(_lc_trainer(3, start=0), BATCH, 4, 600)
    assert np.array_equal(same[:3], ref[:3]) and not np.array_equal(same[3], ref[3])        # the new settings changed the next step only
    sg.disable_lecam()
    assert not sg.graph_active
    one_step(sg, BATCH, 608)
    one_step(sg, BATCH, 609)
    assert sg.graph_active and "errD_lecam" not in sg.loss_terms


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_checkpoint_resume_mid_run(tmp_path, graph):
    """saved after 2 steps with everything on (start = 5: the boundary lies AFTER the save), loaded into a bare trainer from another
    fill, 2 more steps: bit-identical to the uninterrupted run, the anchors and the count of updates included"""
    from tests.common import build_hip_nets
    path = tmp_path / "lecam.pt"
    saved = {}

    def build_a():
        return _everything(2, graph=graph, nets=build_hip_nets("T", seed=0), start=5)

    def build_b():
        from srgan_amd import spectral
        sg = make_trainer("T", BATCH, K, 31, nets=build_hip_nets("T", seed=5))
        torch.manual_seed(18)
        spectral.spectral_norm(sg.D)           # part of building D; the checkpoint turns everything else on
        return sg.enable_graph() if graph else sg

    a = run_a(build_a, path, 2, 2, at_save=lambda sg: saved.update(sg.lecam_stats()))
    assert saved["updates"] == 2 * K and saved["applied"] == 0 and all(saved["a_real"][:2])
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert sd["lecam"] == dict(weight=W, decay=0.9, start=5, clamp=True, a_real=saved["a_real"], a_fake=saved["a_fake"], updates=2 * K)
    b = run_b(build_b, path, 2, 2)
    (sg_a, rows_a, state_a), (sg_b, rows_b, state_b) = a, b
    assert_rows_equal(rows_a, rows_b, "lecam resume")
    assert_state_equal(state_a, state_b, "lecam resume")
    assert sg_a.lecam_stats() == sg_b.lecam_stats() and sg_b.lecam_stats()["updates"] == 4 * K and sg_b.lecam_stats()["applied"] == 1
    assert sg_a.graph_active == sg_b.graph_active == graph


def test_bf16_compute_mode_step():
    """the maps are fp32 in this mode too: R is the restated term on the maps D produced in the step's last update, at the kernel
    test's bound, and every loss term is finite"""
    from srgan_amd import ops
    ops.set_compute_dtype("bf16")
    try:
        sg = _lc_trainer(7, start=0)
        D, seen = sg.D, []
        orig = D.forward_logits

        def hooked(x):
            outs, logits = orig(x)
            seen.append([o.detach().clone() for o in outs])
            return outs, logits

        D.forward_logits = hooked
        torch.manual_seed(350)
        out = one_step(sg, BATCH, 350)
        assert all(o.dtype == torch.float32 for outs in seen for o in outs)
        assert all(np.isfinite(out)) and all(np.isfinite(v) for v in _terms(sg).values())
        st = sg.lecam_stats()
        assert st["updates"] == K and st["applied"] == 1
        # replay the K updates' anchors in float64, then the last term
        rec64 = rec32 = lc.new_record(W, 0.9, 0, 2)
        for outs in seen[:K]:
            maps = [o.cpu().reshape(2 * BATCH, -1) for o in outs]
            v64, _, rec64, _ = lc.call(maps, rec64, 2 * BATCH, BATCH, False, 0.0, torch.float64)
            v32, _, rec32, _ = lc.call(maps, rec32, 2 * BATCH, BATCH, False, 0.0, torch.float32)
        L = max(lc.chain_depth(m.numel()) for m in maps)
        M = max(float(m.abs().max()) for m in maps)
        E = lc.anchor_bound(L, K, M) + lc.EPS32 * 2 * M
        bound = max(8 * abs(float(v32[0]) - float(v64[0])), lc.term_bound(L, E, float(v64[0])))
        err = abs(st["penalty"] - float(v64[0]))
        print(f"bf16 step R {st['penalty']:.9g} float64 {float(v64[0]):.9g} err {err:.3e} bound {bound:.3e}")
        assert err <= bound
    finally:
        ops.set_compute_dtype("fp32")
        ops.invalidate_packed()


def test_refusals_name_the_way_out(monkeypatch):
    from srgan_amd import dp, lecam, ops
    from srgan_amd.trainer import SingleGAN_training
    from tests.step_bits_common import PlainD
    sg = make_trainer("T", BATCH, K, 4)
    for bad, what in ((dict(weight=-1.0), "weight"), (dict(weight=float("nan")), "weight"), (dict(decay=1.0), "decay"),
                      (dict(start=-1), "start"), (dict(clamp=2), "clamp")):
        with pytest.raises(ValueError, match=what):
            sg.enable_lecam(**bad)
    with pytest.raises(RuntimeError, match="enable_lecam"):
        sg.set_lecam(weight=1.0)
    with pytest.raises(NotImplementedError, match="SRGAN_training.enable_lecam"):
        SingleGAN_training.enable_lecam(object())
    monkeypatch.setattr(dp, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="2 ranks.*disable_lecam"):
        sg.enable_lecam()
    monkeypatch.undo()
    assert sg._lecam is None
    # the generic discriminator path: at enable_lecam, and when the step runs
    generic = make_trainer("T", BATCH, K, 4)
    generic.D = PlainD(generic.D)
    with pytest.raises(NotImplementedError, match="fused discriminator pass.*disable_lecam"):
        generic.enable_lecam()
    sg.enable_lecam()
    sg.D = PlainD(sg.D)
    _, _, dev = _cuda_batch(50)
    with pytest.raises(NotImplementedError, match="fused discriminator pass.*disable_lecam"):
        sg.train(*dev)
    # a first use inside a capture must not allocate; settings are not written inside one either
    fresh = lecam.LeCam()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="inside a hipGraph capture"):
        with torch.cuda.graph(g):
            fresh._ensure(torch.device("cuda"))
    assert ops.get_compute_dtype() == "fp32"
