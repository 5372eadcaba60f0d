"""GPU: spectral normalisation of the discriminator (srgan_amd.spectral, csrc/spectral.hip) against the float64 restatement of
tests/sn_common.py -- the two multi-tensor operations, a marked module, checkpoints, the train step against the oracle, and
bit-equality of the recorded step, of an idle gradient guard and of a network whose mark was removed."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import nets as onets, trainer as otrainer
from tests import sn_common as sn
from tests.common import build_hip_nets, close, close_grad, close_params, oracle_params
from tests.ema_common import assert_same, live_state, make_trainer, steps

pytestmark = pytest.mark.gpu
SN_SEED = 77


# ---- op level ------------------------------------------------------------------------------------------------------------------
class Table:
    """weights of the given (O, I, kh, kw) with their (W_sn, u, v, sigma) buffers and one device table, as spectral.py keeps them;
    ``off``: elements into a 16-byte aligned buffer (1: every pointer misaligned)"""

    def __init__(self, shapes, seed, off=0):
        from srgan_amd import ops
        self.ops = ops
        g = torch.Generator().manual_seed(seed)

        def dev(t):
            base = torch.zeros(t.numel() + 8, dtype=torch.float32, device="cuda")
            view = base[off:off + t.numel()].view(t.shape)
            view.copy_(t)
            return view

        self.W0, self.u0, self.v0, self.G0 = [], [], [], []
        for i, shp in enumerate(shapes):
            o, k = shp[0], shp[1] * shp[2] * shp[3]
            mag = 10.0 ** (-3 + 5 * i / max(len(shapes) - 1, 1)) if len(shapes) > 1 else 10.0 ** (seed % 6 - 3)   # 1e-3 .. 1e2
            self.W0.append(torch.randn(shp, generator=g) * mag)
            self.u0.append(torch.nn.functional.normalize(torch.randn(o, generator=g), dim=0))
            self.v0.append(torch.nn.functional.normalize(torch.randn(k, generator=g), dim=0))
            self.G0.append(torch.randn(shp, generator=g) / mag)
        self.W = [dev(t) for t in self.W0]
        self.Wsn = [dev(torch.zeros_like(t)) for t in self.W0]
        self.u = [dev(t) for t in self.u0]
        self.v = [dev(t) for t in self.v0]
        self.G = [dev(t) for t in self.G0]
        self.sigma = torch.zeros(len(shapes), dtype=torch.float32, device="cuda")
        rows = [(w.data_ptr(), ws.data_ptr(), u.data_ptr(), v.data_ptr(), self.sigma.data_ptr() + 4 * i, w.shape[0], w[0].numel())
                for i, (w, ws, u, v) in enumerate(zip(self.W, self.Wsn, self.u, self.v))]
        self.table, self.plan, self.ws = ops.spectral_table(rows, torch.device("cuda"))
        self.gtab = ops.upload_small(np.array([g_.data_ptr() for g_ in self.G], dtype=np.uint64).tobytes(), torch.device("cuda"))

    def reset(self):
        for dst, src in zip(self.u + self.v + self.G, self.u0 + self.v0 + self.G0):
            dst.copy_(src)
        for w in self.Wsn:
            w.zero_()
        self.sigma.zero_()
        self.ws.zero_()

    def refresh(self, iterate=True, n=1):
        self.ops.spectral_refresh_(self.table, self.plan, self.ws, iterate, n, sn.EPS)

    def project(self):
        self.ops.spectral_project_(self.table, self.plan, self.gtab, self.ws)

    def snapshot(self):
        torch.cuda.synchronize()
        return [t.detach().clone() for t in self.u + self.v + self.Wsn + self.G] + [self.sigma.clone()]


def _check_table(shapes, seed, n, off, what):
    tab = Table(shapes, seed, off)
    runs = []
    for _ in range(2):                                    # every call twice from the same state: equal bits
        tab.reset()
        tab.refresh(True, n)
        tab.project()
        after = tab.snapshot()
        tab.refresh(False)                                # sigma and W_sn again from the stored (u, v): nothing may move
        runs.append(after + tab.snapshot())
    for a, b in zip(*runs):
        assert torch.equal(a, b), what
    worst = 0.0
    for i, shp in enumerate(shapes):
        u, v, sigma, Wsn = sn.refresh(tab.W0[i], tab.u0[i], tab.v0[i], n)
        want = dict(u=u, v=v, sigma=sigma.reshape(1), W_sn=Wsn, grad=sn.project(tab.G0[i].double(), Wsn, u, v, sigma))
        got = dict(u=tab.u[i], v=tab.v[i], sigma=tab.sigma[i:i + 1], W_sn=tab.Wsn[i], grad=tab.G[i])
        for key in want:
            r = sn.ratio(got[key], want[key])
            worst = max(worst, r)
            assert r <= 1.0, f"{what} layer {i} {shp} {key}: error / (1e-5 * max|ref|) = {r:.3f}"
        # without iteration: sigma = u^T W v and W / sigma of the stored vectors
        s2, W2 = sn.materialize(tab.W0[i].double(), sn.np64(tab.u[i]), sn.np64(tab.v[i]))
        assert sn.ratio(runs[0][len(runs[0]) - 1][i:i + 1], s2.reshape(1)) <= 1.0, (what, i, "sigma without iteration")
    print(f"{what}: worst error / bound = {worst:.4f} (bound 1e-5 * max|ref|)")


@pytest.mark.parametrize("i", range(len(sn.OP_SHAPES)))
def test_one_layer_per_table_against_the_restatement(i):
    shp = sn.OP_SHAPES[i]
    assert (shp[0], shp[1] * shp[2] * shp[3]) == sn.OP_OK[i]
    _check_table([shp], seed=10 + i, n=1, off=0, what=f"{sn.OP_OK[i]}")


@pytest.mark.parametrize("n,off", [(1, 0), (3, 0), (1, 1)])
def test_all_layers_in_one_table_against_the_restatement(n, off):
    """seven layers, magnitudes 1e-3 .. 1e2; n_power_iterations = 3; every pointer 4 bytes off a 16-byte boundary (scalar paths)"""
    _check_table(sn.OP_SHAPES, seed=3, n=n, off=off, what=f"seven layers, n = {n}, offset {off}")


def test_projection_leaves_a_layer_without_gradient_alone():
    tab = Table(sn.OP_SHAPES[:3], seed=5)
    tab.refresh()
    ptrs = [tab.G[0].data_ptr(), 0, tab.G[2].data_ptr()]
    tab.gtab = tab.ops.upload_small(np.array(ptrs, dtype=np.uint64).tobytes(), torch.device("cuda"))
    tab.project()
    torch.cuda.synchronize()
    assert torch.equal(tab.G[1].cpu(), tab.G0[1]) and not torch.equal(tab.G[0].cpu(), tab.G0[0])


# ---- module level ----------------------------------------------------------------------------------------------------------------
def _marked_D(seed=SN_SEED, **kw):
    from srgan_amd import spectral
    _, D, _ = build_hip_nets("T")
    torch.manual_seed(seed)
    return spectral.spectral_norm(D, **kw)


def _module_reference(n=1):
    """oracle.nets.discriminator on the restated W_sn with autograd and the projection -> (outputs, logits-softmax, grads)"""
    _, PD, _ = oracle_params("T")
    torch.manual_seed(SN_SEED)
    st = sn.Restated({k: PD[k] for k in sn.sn_keys(PD)}, n)
    P = {k: (st.Wsn[k].float() if k in st.Wsn else v.clone()).requires_grad_(True) for k, v in PD.items()}
    x, _ = otrainer.synthetic_batch(4, 128, 4, seed=31)
    (o1, o2), (c1, c2) = onets.discriminator(P, x, 4)
    ((o1 ** 2).sum() + o2.sum() + (c1 ** 2).sum() + (c2 ** 2).sum()).backward()
    grads = {k: (st.project(k, P[k].grad).float() if k in st.Wsn else P[k].grad) for k in P}
    return x, st, (o1, o2, c1, c2), grads


def _module_run(D, x):
    from srgan_amd import spectral
    (o1, o2), (c1, c2) = D(x.cuda())
    ((o1 ** 2).sum() + o2.sum() + (c1 ** 2).sum() + (c2 ** 2).sum()).backward()
    spectral.project(D)
    grads = {k.replace("weight_orig", "weight"): p.grad for k, p in D.named_parameters()}
    return (o1, o2, c1, c2), grads


def test_marked_discriminator_vs_oracle_on_the_restated_weights():
    from srgan_amd import spectral
    x, st, want, want_g = _module_reference()
    D = _marked_D()
    got, got_g = _module_run(D, x)
    for name, a, b in zip(("o1", "o2", "c1", "c2"), got, want):
        close(a.reshape(b.shape), b, what=name)
    assert set(got_g) == set(want_g)
    for k in want_g:
        close_grad(got_g[k], want_g[k], what="grad " + k)
    sig = spectral.sigmas(D)
    for k in st.sigma:
        assert sn.ratio(torch.tensor([sig[k[:-len(".weight")]]]), st.sigma[k].reshape(1)) <= 1.0, k
    # train() / eval() change nothing, and neither does a second forward: the iteration belongs to the optimiser step
    before = sn.sn_state(D)
    D.eval()
    D(x.cuda())
    D.train()
    assert_same(before, sn.sn_state(D))


def test_marked_discriminator_bf16_compute_mode():
    """tests/test_modules_gpu.py checks the bf16 mode by bit-equality between two HIP runs and holds no numeric bound for it.  So:
    (a) the marked network equals, bit for bit, a plain HIP network that holds W_sn as its weights (outputs, the gradients of the
    normalised weights and of the biases): the mark changes nothing the convolutions see; (b) the projection of those gradients
    is within the op-level bound of the float64 formula, and sigma / u / v / W_sn are the fp32-mode bits (the spectral kernels are
    fp32 in both modes); (c) against the fp32 oracle the suite's bounds for bf16 conv operands hold: relative L2 2e-2 on the
    outputs (tests/test_ops_gpu.py: 2^-9 per operand, a few sign flips) and 5e-2 on the gradients (ibid.: the activation-mask
    flips of bf16-rounded conv outputs move a gradient by 3e-2 .. 5e-2 of its fp32 value)."""
    from srgan_amd import ops, spectral
    x, st, want, want_g = _module_reference()
    D32 = _marked_D()
    ops.set_compute_dtype("bf16")
    try:
        D = _marked_D()
        assert_same(sn.sn_state(D32), sn.sn_state(D))
        ctl = spectral.controller(D)
        _, plain, _ = build_hip_nets("T")
        with torch.no_grad():
            for name, leaf in zip(ctl.names, ctl.leaves):
                plain.get_submodule(name).weight.copy_(leaf)
        with ops.pack_cache():
            (o1, o2), (c1, c2) = D(x.cuda())
            ((o1 ** 2).sum() + o2.sum() + (c1 ** 2).sum() + (c2 ** 2).sum()).backward()
            pouts = plain(x.cuda())
            ((pouts[0][0] ** 2).sum() + pouts[0][1].sum() + (pouts[1][0] ** 2).sum() + (pouts[1][1] ** 2).sum()).backward()
        for a_, b_ in zip((o1, o2, c1, c2), (pouts[0][0], pouts[0][1], pouts[1][0], pouts[1][1])):
            assert torch.equal(a_, b_)
        raw = {}
        for name, leaf in zip(ctl.names, ctl.leaves):
            m = plain.get_submodule(name)
            assert torch.equal(leaf.grad, m.weight.grad), name
            raw[name + ".weight"] = leaf.grad.detach().clone()
            if m.bias is not None:
                assert torch.equal(D.get_submodule(name).bias.grad, m.bias.grad), name
        spectral.project(D)
        got = (o1, o2, c1, c2)
        got_g = {k.replace("weight_orig", "weight"): p.grad for k, p in D.named_parameters()}
        worst = 0.0
        for i, name in enumerate(ctl.names):
            m = D.get_submodule(name)
            ref = sn.project(sn.np64(raw[name + ".weight"]), sn.np64(ctl.leaves[i]), sn.np64(m.weight_u), sn.np64(m.weight_v),
                             sn.np64(ctl.sigma[i]))
            r = sn.ratio(got_g[name + ".weight"], ref)
            worst = max(worst, r)
            assert r <= 1.0, (name, r)
        print(f"bf16 mode: projection, worst error / (1e-5 * max|ref|) = {worst:.4f}")
    finally:
        ops.set_compute_dtype("fp32")
        ops.invalidate_packed()

    def rel(a, b):
        a, b = sn.np64(a).reshape(b.shape), sn.np64(b)
        return float((a - b).norm() / b.norm())

    eo = {n: rel(a, b) for n, a, b in zip(("o1", "o2", "c1", "c2"), got, want)}
    eg = {k: rel(got_g[k], want_g[k]) for k in want_g}
    print(f"bf16 mode vs fp32 oracle: outputs {max(eo.values()):.3e} (bound 2e-2), gradients {max(eg.values()):.3e} (bound 5e-2)")
    assert max(eo.values()) <= 2e-2, eo
    assert max(eg.values()) <= 5e-2, eg


def test_refusals_that_need_a_marked_network():
    from srgan_amd import spectral
    D = _marked_D()
    with pytest.raises(RuntimeError, match="marked already"):
        spectral.spectral_norm(D)
    with pytest.raises(RuntimeError, match="marked already"):
        spectral.spectral_norm(D.discriminator1)
    _, D2, _ = build_hip_nets("T")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            with pytest.raises(RuntimeError, match="inside a hipGraph capture"):
                spectral.spectral_norm(D2)
            with pytest.raises(RuntimeError, match="inside a hipGraph capture"):
                spectral.remove_spectral_norm(D)
        finally:
            g.capture_end()
    assert "weight" in dict(D2.last_layer1.named_parameters())


# ---- checkpoints -----------------------------------------------------------------------------------------------------------------
def test_state_dict_loads_into_torch_spectral_norm():
    D = _marked_D()
    sd = {k: v.cpu() for k, v in D.state_dict().items()}
    assert not any(k.endswith(".weight") for k in sd)
    ctl = __import__("srgan_amd.spectral", fromlist=["x"]).controller(D)
    for name, m, leaf in zip(ctl.names, ctl.mods, ctl.leaves):
        ref = nn.Conv2d(m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, bias=m.bias is not None)
        torch.nn.utils.spectral_norm(ref)
        mine = {k[len(name) + 1:]: v for k, v in sd.items() if k.startswith(name + ".")}
        want = ref.state_dict()
        assert list(mine) == list(want) and all(mine[k].shape == want[k].shape and mine[k].dtype == want[k].dtype for k in want), name
        ref.load_state_dict(mine, strict=True)
        ref.eval()
        ref(torch.zeros(1, m.in_channels, 16, 16))        # eval mode: the weight from the stored (u, v), no iteration
        assert sn.ratio(leaf, ref.weight.detach()) <= 1.0, name


def _sn_trainer(seed=2, k=2, mark=True, **kw):
    from srgan_amd import spectral
    sg = make_trainer("T", 4, k, seed, **kw)
    if mark:
        torch.manual_seed(SN_SEED)
        spectral.spectral_norm(sg.D)
    return sg


def _full_state(sg):
    out = live_state(sg)
    out.update(sn.sn_state(sg.D))
    return out


def test_save_load_and_one_more_step_is_bit_identical():
    a = _sn_trainer()
    steps(a, 4, 2, 300)
    sd = {k: v.detach().clone() for k, v in a.D.state_dict().items()}
    opt_sd = copy.deepcopy(a.optD.state_dict())              # (state_dict() hands out the live moment tensors)
    ref_loss = steps(a, 4, 1, 400)
    b = _sn_trainer()
    steps(b, 4, 2, 300)                                   # same G / E and optimiser states; D restored from the checkpoint below
    torch.manual_seed(999)
    from srgan_amd import spectral
    spectral.remove_spectral_norm(b.D)
    spectral.spectral_norm(b.D)                           # a FRESH mark: other (u, v), one iteration on the current weights
    b.D.load_state_dict(sd)                               # ... all replaced by the checkpoint, W_sn re-materialised, no iteration
    b.optD.load_state_dict(opt_sd)
    got_loss = steps(b, 4, 1, 400)
    np.testing.assert_array_equal(got_loss, ref_loss)
    assert_same(_full_state(a), _full_state(b))


def test_remove_spectral_norm_leaves_a_plain_network_with_the_same_forward():
    from srgan_amd import spectral
    D = _marked_D()
    x, _ = otrainer.synthetic_batch(4, 128, 4, seed=31)
    params = {id(p) for p in D.parameters()}
    with torch.no_grad():
        before = [t.clone() for pair in D(x.cuda()) for t in pair]
    spectral.remove_spectral_norm(D)
    assert spectral.controller(D) is None and {id(p) for p in D.parameters()} == params      # the same Parameter objects
    _, plain, _ = build_hip_nets("T")
    assert list(D.state_dict()) == list(plain.state_dict())
    with torch.no_grad():
        after = [t for pair in D(x.cuda()) for t in pair]
    for a, b in zip(before, after):
        assert torch.equal(a, b)


# ---- train step ------------------------------------------------------------------------------------------------------------------
def test_trajectory_vs_the_spectral_oracle():
    """tier T, batch 4, k = 2, 4 steps: losses to 1e-3, parameters with close_params (tests/test_train_gpu.py), u / v / sigma to
    1e-3 of their largest element"""
    batch, k, n = 4, 2, 4
    PG, PD, PE = oracle_params("T")
    torch.manual_seed(2)
    orc = sn.SNOracle(PG, PD, PE, otrainer.DEFAULT_LBD, k, np.eye(4), batch, "mu", 8, sn_seed=SN_SEED)
    torch.manual_seed(500)
    ref = []
    for s in range(n):
        x, label = otrainer.synthetic_batch(batch, 128, 4, seed=500 + s)
        ref.append([float(v) for v in orc.train(x, label)])
    sg = _sn_trainer(seed=2, k=k)
    got = steps(sg, batch, n, 500)
    np.testing.assert_allclose(got, np.array(ref), rtol=1e-3)
    for net, P, n_opt in ((sg.G, orc.G, 2 * n), (sg.E, orc.E, n)):
        for key, v in net.state_dict().items():
            close_params(v, P[key], 1e-4, n_opt, what=key)
    sd = sg.D.state_dict()
    for key in PD:
        if key in orc.sn_orig:
            close_params(sd[key + "_orig"], orc.sn_orig[key], 1e-4, k * n, what=key + "_orig")
            close(sd[key + "_u"], orc.sn.u[key], rtol=1e-3, what=key + "_u")
            close(sd[key + "_v"], orc.sn.v[key], rtol=1e-3, what=key + "_v")
        else:
            close_params(sd[key], orc.D[key], 1e-4, k * n, what=key)
    from srgan_amd import spectral
    sig = spectral.sigmas(sg.D)
    for key in orc.sn_orig:
        close(torch.tensor([sig[key[:-len(".weight")]]]), orc.sn.sigma[key].reshape(1), rtol=1e-3, what=key + " sigma")


def test_graph_replay_is_bit_identical_and_a_late_mark_drops_the_recording():
    from srgan_amd import spectral
    eager = _sn_trainer(seed=2)
    ref = steps(eager, 4, 4, 500)
    sg = _sn_trainer(seed=2).enable_graph()
    got = steps(sg, 4, 4, 500)
    assert sg.graph_active
    np.testing.assert_array_equal(got, ref)
    assert_same(_full_state(eager), _full_state(sg))

    # the mark applied AFTER a recording exists: the recording is dropped, the next steps record again and still match
    def mark_after_two(t, s):
        if s == 1:
            if t._graph is not None:
                assert t.graph_active
            torch.manual_seed(SN_SEED)
            spectral.spectral_norm(t.D)
            torch.manual_seed(1234)

    eager2 = _sn_trainer(seed=3, mark=False)
    ref2 = steps(eager2, 4, 5, 600, after=mark_after_two)
    sg2 = _sn_trainer(seed=3, mark=False).enable_graph()
    got2 = steps(sg2, 4, 2, 600, after=mark_after_two)
    from tests.ema_common import one_step
    more = [one_step(sg2, 4, 602)]
    assert not sg2.graph_active                                                     # dropped by the mark: this step ran eagerly
    more += [one_step(sg2, 4, 603), one_step(sg2, 4, 604)]
    assert sg2.graph_active                                                         # ... and the step was recorded again
    np.testing.assert_array_equal(np.concatenate([got2, np.array(more)]), ref2)
    assert_same(_full_state(eager2), _full_state(sg2))


def test_idle_gradient_guard_changes_no_bit():
    a = _sn_trainer(seed=4)
    ref = steps(a, 4, 2, 700)
    b = _sn_trainer(seed=4)
    b.enable_grad_guard()
    got = steps(b, 4, 2, 700)
    np.testing.assert_array_equal(got, ref)
    assert_same(_full_state(a), _full_state(b))
    st = b.grad_guard_stats()["D"]
    assert st["steps"] == 4 and st["skipped"] == 0 and st["norm"] > 0


def test_marked_then_unmarked_trainer_equals_a_never_marked_one():
    from srgan_amd import spectral
    a = make_trainer("T", 4, 2, 5)
    ref = steps(a, 4, 2, 800)
    b = _sn_trainer(seed=5)
    spectral.remove_spectral_norm(b.D)
    _, PD, _ = oracle_params("T")
    b.D.load_state_dict(PD)                               # the weights restored to the originals
    got = steps(b, 4, 2, 800)
    np.testing.assert_array_equal(got, ref)
    assert_same(live_state(a), live_state(b))
