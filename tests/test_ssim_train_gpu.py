"""GPU: the structural-similarity term inside the train step (SRGAN_training.enable_ssim) at tier T, 128 x 128, batch 4, k = 2 -- the
step against the CPU oracle with the term (tests/ssim_common.SSIMOracle), the reported term against the float64 restatement at the
kernel bound, off means bit-identical to the plain step, graph mode, checkpoints, the bf16 compute mode, composition with every
other extension and the refusals."""
import numpy as np
import pytest
import torch

from oracle import trainer as otrainer
from tests import ssim_common as sc
from tests.checkpoint_common import assert_rows_equal, assert_state_equal, run_a, run_b
from tests.common import close_params, oracle_params
from tests.ema_common import assert_same, live_state, make_trainer, one_step, steps
from tests.step_bits_common import _launch_counts
from tests.test_train_gpu import TERM_PAIRS

pytestmark = pytest.mark.gpu
BATCH, K, SIZE = 4, 2, 128
W = sc.SS_WEIGHT
SN_SEED = 77


def _terms(sg):
    return {k: float(v) for k, v in sg.loss_terms.items()}


def _cuda_batch(seed):
    x, label = otrainer.synthetic_batch(BATCH, SIZE, 4, seed=seed)
    return x, label, (x.cuda(), {"source": label["source"].cuda(), "target": label["target"]})


def _term_matches(sg, source, image, got, what):
    """the reported term against the float64 restatement on the fp32 images, at the kernel tests' bound"""
    x, y = source.detach().float().cpu(), image.detach().float().cpu()
    want = sc.reference(x, y, grads=False)["term"]
    bound = sc.bounds(x, y, grads=False)["term"]
    print(f"{what}: term {got:.9g} float64 {want:.9g} err {abs(got - want):.3e} bound {bound:.3e}")
    assert abs(got - want) <= bound, (what, got, want, bound)


@pytest.mark.parametrize("on", [("cycle",), ("cycle", "idt")], ids=["cycle", "cycle+idt"])
def test_three_steps_vs_the_oracle_with_the_term(on):
    """the three losses and every loss term of each of 3 steps, the SSIM terms and the parameters after them at the trajectory
    tolerance of test_train_gpu (1e-3; close_params)"""
    seed, n_steps = 5, 3
    PG, PD, PE = oracle_params("T")
    torch.manual_seed(seed)
    orc = sc.SSIMOracle(PG, PD, PE, otrainer.DEFAULT_LBD, K, np.eye(4), BATCH, "mu", 8, weight=W, on=on)
    refs, traces = [], []
    for step in range(n_steps):                          # the oracle's run first: both draw the noise from the CPU generator
        x, label, _ = _cuda_batch(42 + step)
        refs.append([float(v) for v in orc.train(x, label)])
        traces.append(orc.trace)
    sg = make_trainer("T", BATCH, K, seed).enable_ssim(weight=W, on=on)
    for step in range(n_steps):
        x, _, dev = _cuda_batch(42 + step)
        out = [float(v) for v in sg.train(*dev)]
        np.testing.assert_allclose(out, refs[step], rtol=1e-3, err_msg=f"step {step}")
        t, tr = _terms(sg), traces[step]
        for a, b in TERM_PAIRS:
            assert abs(t[a] - tr[b]) <= 1e-3 * max(abs(tr[b]), 1e-3), (step, a, t[a], tr[b])
        for which in ("cycle", "idt"):
            key = f"errG_ssim_{which}"
            if which in on:
                want = tr[f"g_ssim_{which}"]
                print(f"on {on} step {step} {key} {t[key]:.9g} oracle {want:.9g}")
                assert want > 0 and abs(t[key] - want) <= 1e-3 * want, (step, key, t[key], want)
            else:
                assert key not in t
        _term_matches(sg, x, sg.recon_image, t["errG_ssim_cycle"], f"on {on} step {step}")
    stats = sg.ssim_stats()
    assert stats["updates"] == n_steps * len(on) and stats["on"] == on and stats["weight"] == W
    assert stats["term"] == t["errG_ssim_" + on[-1]] and abs(stats["weighted"] - W * stats["term"]) <= 4 * sc.U * W * stats["term"]
    for net, P, n_opt in ((sg.G, orc.G, 2 * n_steps), (sg.D, orc.D, K * n_steps), (sg.E, orc.E, n_steps)):
        for key, v in net.state_dict().items():
            close_params(v, P[key], 1e-4, n_opt, what=key, walk=True)


def _step_launches(sg, seed):
    """{kernel: launches} the launch timer sees in one whole train step"""
    from srgan_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.srgan_prof_enable(1)
    try:
        torch.manual_seed(seed)
        one_step(sg, BATCH, seed)
        torch.cuda.synchronize()
    finally:
        lib.srgan_prof_enable(0)
    return _launch_counts(lib)


def test_off_is_the_plain_step_and_the_term_changes_it():
    a = make_trainer("T", BATCH, K, 2)
    ref = steps(a, BATCH, 2, 300)
    b = make_trainer("T", BATCH, K, 2)
    b.enable_ssim(weight=3.0, on=("cycle", "idt"), window=7)
    assert b._ssim is not None and b.ssim_stats()["updates"] == 0 and b.ssim_stats()["on"] == ("cycle", "idt")
    b.disable_ssim()
    assert b._ssim is None and b.ssim_stats() is None
    got = steps(b, BATCH, 2, 300)
    np.testing.assert_array_equal(got, ref)
    assert_same(live_state(a), live_state(b))
    assert _terms(a) == _terms(b) and not any(k.startswith("errG_ssim") for k in b.loss_terms)
    # the timed launches of a step are the plain step's with the feature off, and with it on (its kernels are untimed by design)
    plain = _step_launches(a, 302)
    assert plain and _step_launches(b, 302) == plain
    c = make_trainer("T", BATCH, K, 2).enable_ssim(weight=W)
    got_c = steps(c, BATCH, 2, 300)
    assert _step_launches(c, 302) == plain
    from srgan_amd import _lib
    lib = _lib.load()
    assert not any("ssim" in lib.srgan_prof_kernel_name(k).decode() for k in range(lib.srgan_prof_num_kernels()))
    # step 1: errD and errE_output are the plain ones (the term is not part of them; errG ends with phase 2's term, taken after the
    # generator's first update, which has seen the term's gradient); step 2 differs throughout
    assert np.array_equal(got_c[0][1:], ref[0][1:]) and got_c[0][0] != ref[0][0] and not np.array_equal(got_c[1], ref[1])
    now = live_state(c)
    plain_state = live_state(a)
    assert any(not torch.equal(now[k], plain_state[k]) for k in now if k.startswith("G."))
    # a zero weight: the term is taken and reported, the parameters are the plain run's
    z = make_trainer("T", BATCH, K, 2).enable_ssim(weight=0.0)
    got_z = steps(z, BATCH, 2, 300)
    np.testing.assert_array_equal(got_z, ref)
    st = z.ssim_stats()
    assert st["updates"] == 2 and st["weighted"] == 0.0 and st["term"] > 0 and float(z.loss_terms["errG_ssim_cycle"]) == st["term"]


def _ss_trainer(seed, on=("cycle", "idt"), **kw):
    return make_trainer("T", BATCH, K, seed).enable_ssim(weight=W, on=on, **kw)


def test_graph_replay_is_bit_identical_to_eager():
    eager = _ss_trainer(2)
    ref = steps(eager, BATCH, 4, 500)
    sg = _ss_trainer(2).enable_graph()
    seen = []
    got = steps(sg, BATCH, 4, 500, after=lambda t, s: seen.append((t.graph_active, t.ssim_stats()["updates"])))
    assert sg.graph_active and seen == [(False, 2), (True, 4), (True, 6), (True, 8)]
    np.testing.assert_array_equal(got, ref)
    assert _terms(sg) == _terms(eager)
    assert_same(live_state(eager), live_state(sg))
    assert eager.ssim_stats() == sg.ssim_stats()
    assert float(sg.loss_terms["errG_ssim_idt"]) == sg.ssim_stats()["term"]
    plain = steps(make_trainer("T", BATCH, K, 2), BATCH, 2, 500)
    assert np.array_equal(plain[0][1:], ref[0][1:]) and not np.array_equal(plain[1], ref[1])


def test_set_ssim_weight_keeps_the_recording_and_enable_disable_or_a_new_window_drop_it():
    def change(t, s):
        if s == 2:
            t.set_ssim_weight(2 * W)
        if s == 4:
            t.enable_ssim(weight=W, on=("cycle",), window=7)

    eager = _ss_trainer(3, on=("cycle",))
    ref = steps(eager, BATCH, 7, 600, after=change)
    sg = _ss_trainer(3, on=("cycle",)).enable_graph()
    active = []

    def change_and_watch(t, s):
        before = t.graph_active
        change(t, s)
        active.append((s, before, t.graph_active))

    got = steps(sg, BATCH, 7, 600, after=change_and_watch)
    # s = 2: the weight is device state and the recording stays; s = 4: a new object with another window drops it; step 5 runs
    # eagerly, step 6 records again
    assert active == [(0, False, False), (1, True, True), (2, True, True), (3, True, True), (4, True, False), (5, False, False),
                      (6, True, True)]
    np.testing.assert_array_equal(got, ref)
    assert_same(live_state(eager), live_state(sg))
    st = sg.ssim_stats()
    assert st == eager.ssim_stats() and st["window"] == 7 and st["updates"] == 2 and st["weight"] == W
    same = steps(_ss_trainer(3, on=("cycle",)), BATCH, 5, 600)
    # the new weight is first read by step 3, whose errG ends with a term taken after the generator's update under it
    assert np.array_equal(same[:3], ref[:3]) and not np.array_equal(same[3], ref[3])
    sg.disable_ssim()
    assert not sg.graph_active
    one_step(sg, BATCH, 608)
    one_step(sg, BATCH, 609)
    assert sg.graph_active and "errG_ssim_cycle" not in sg.loss_terms


def _everything(seed, ssim=True, graph=False, nets=None):
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
    sg.enable_lecam(weight=1.0, decay=0.9)
    sg.enable_mode_seeking(weight=0.5, seed=12)
    if ssim:
        sg.enable_ssim(weight=W, on=("cycle", "idt"), window=7, sigma=1.0)
    return sg.enable_graph() if graph else sg


def test_composition_with_every_other_extension():
    sg = _everything(7)
    rows = steps(sg, BATCH, 3, 370)
    assert np.isfinite(rows).all() and all(np.isfinite(v) for v in _terms(sg).values())
    t = _terms(sg)
    assert 0 < t["errG_ssim_cycle"] < 2 and 0 < t["errG_ssim_idt"] < 2 and "errG_ms" in t and "errD_lecam" in t and t["errD_r1"] > 0
    st = sg.ssim_stats()
    assert st["updates"] == 6 and st["window"] == 7 and st["term"] == t["errG_ssim_idt"]
    # the other features' host-side draws are what they are without the term
    other = _everything(7, ssim=False)
    steps(other, BATCH, 3, 370)
    assert torch.equal(sg.augment.generator.get_state(), other.augment.generator.get_state())
    assert torch.equal(sg._ms.generator.get_state(), other._ms.generator.get_state())
    assert sg.bcr_stats()["updates"] == other.bcr_stats()["updates"] and sg.lecam_stats()["updates"] == other.lecam_stats()["updates"]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_checkpoint_resume_mid_run(tmp_path, graph):
    """saved after 2 steps with everything on, loaded into a bare trainer from another fill, 2 more steps: bit-identical to the
    uninterrupted run, the settings, the count of updates and the last values included"""
    from tests.common import build_hip_nets
    path = tmp_path / "ssim.pt"
    saved = {}

    def build_a():
        return _everything(2, graph=graph, nets=build_hip_nets("T", seed=0))

    def build_b():
        from srgan_amd import spectral
        sg = make_trainer("T", BATCH, K, 31, nets=build_hip_nets("T", seed=5))
        torch.manual_seed(18)
        spectral.spectral_norm(sg.D)           # part of building D; the checkpoint turns everything else on
        return sg.enable_graph() if graph else sg

    a = run_a(build_a, path, 2, 2, at_save=lambda sg: saved.update(sg.ssim_stats()))
    assert saved["updates"] == 4 and saved["term"] > 0
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert sd["ssim"] == dict(weight=W, on=["cycle", "idt"], window=7, sigma=1.0, k1=0.01, k2=0.03, data_range=2.0, updates=4,
                              term=saved["term"], weighted=saved["weighted"])
    b = run_b(build_b, path, 2, 2)
    (sg_a, rows_a, state_a), (sg_b, rows_b, state_b) = a, b
    assert_rows_equal(rows_a, rows_b, "ssim resume")
    assert_state_equal(state_a, state_b, "ssim resume")
    assert sg_a.ssim_stats() == sg_b.ssim_stats() and sg_b.ssim_stats()["updates"] == 8
    assert sg_a.graph_active == sg_b.graph_active == graph
    # loaded right after the save, before any step: the record holds the saved counter and last values
    c = build_b()
    c.load_checkpoint(path)
    assert c.ssim_stats() == saved
    # a trainer without the identity term cannot take the section: refused by name before anything is written
    d = build_b()
    d.lbd["idt"] = 0.0
    before = live_state(d)
    with pytest.raises(ValueError, match=r"identity reconstruction.*lbd\['idt'\] is 0"):
        d.load_checkpoint(path, strict=False)
    assert d._ssim is None and d._ms is None and d.ssim_stats() is None
    assert_same(before, live_state(d))


def test_bf16_compute_mode_step():
    """G's RGB output is fp32 in this mode too: the term is the restated one on the fp32 images, at the kernel tests' bound"""
    from srgan_amd import ops
    ops.set_compute_dtype("bf16")
    try:
        sg = _ss_trainer(7, on=("cycle",))
        torch.manual_seed(350)
        x, _, dev = _cuda_batch(350)
        out = [float(v) for v in sg.train(*dev)]
        assert sg.recon_image.dtype == torch.float32 and sg.target_image.dtype == torch.float32
        assert all(np.isfinite(out)) and all(np.isfinite(v) for v in _terms(sg).values())
        assert sg.ssim_stats()["updates"] == 1
        _term_matches(sg, x, sg.recon_image, float(sg.loss_terms["errG_ssim_cycle"]), "bf16 step")
    finally:
        ops.set_compute_dtype("fp32")
        ops.invalidate_packed()


def test_refusals_name_the_way_out():
    from srgan_amd import ops, structural
    from srgan_amd.trainer import SingleGAN_training
    sg = make_trainer("T", BATCH, K, 4)
    for bad, what in ((dict(weight=-1.0), "weight"), (dict(weight=float("nan")), "weight"), (dict(window=8), "window"),
                      (dict(window=13), "window"), (dict(sigma=0.0), "sigma"), (dict(k2=0.0), "k2"), (dict(data_range=0.0), "data_range"),
                      (dict(on=()), "subset"), (dict(on=("cycle", "reg")), "subset"), (dict(on=("cycle", "cycle")), "subset")):
        with pytest.raises(ValueError, match=what):
            sg.enable_ssim(**bad)
    assert sg._ssim is None
    with pytest.raises(RuntimeError, match="enable_ssim"):
        sg.set_ssim_weight(1.0)
    with pytest.raises(NotImplementedError, match="SRGAN_training.enable_ssim"):
        SingleGAN_training.enable_ssim(object())
    # the identity image does not exist without the identity term
    sg.lbd["idt"] = 0.0
    with pytest.raises(ValueError, match=r"lbd\['idt'\] > 0.*on=\('cycle',\)"):
        sg.enable_ssim(on=("cycle", "idt"))
    sg.enable_ssim(on="cycle")
    assert sg.ssim_stats()["on"] == ("cycle",)
    sg.lbd["idt"] = 5.0
    sg.enable_ssim(on=("idt", "cycle"))
    assert sg.ssim_stats()["on"] == ("cycle", "idt")
    sg.lbd["idt"] = 0.0                                     # switched off behind the trainer's back: the step says so
    _, _, dev = _cuda_batch(50)
    with pytest.raises(RuntimeError, match=r"lbd\['idt'\] > 0.*on=\('cycle',\)"):
        sg.train(*dev)
    # images too small for the window, other dtypes
    small = structural.SSIM(window=11)
    a = torch.zeros(2, 3, 10, 32, device="cuda")
    with pytest.raises(ops._lib.SrganHipError, match="window"):
        small.loss(a, a)
    with pytest.raises(ops._lib.SrganHipError, match="fp32 images only"):
        small.loss(a.to(torch.bfloat16), a.to(torch.bfloat16))
    # a first use inside a capture must not allocate; the weight is not written inside one either
    fresh = structural.SSIM()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="inside a hipGraph capture"):
        with torch.cuda.graph(g):
            fresh._ensure(torch.device("cuda"))
    assert ops.get_compute_dtype() == "fp32"
