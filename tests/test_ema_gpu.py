"""GPU: the exponential moving average of the sampling weights kept inside the train step (SRGAN_training.enable_ema,
srgan_amd.ema, srgan_ema_multi_dev).  The yardstick is the float64 restatement of tests/ema_common.py with its derived bound
5 * T * 2^-24 * M; everything else is bit-equality."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.ema_common import (assert_same, bound, check_within_bound, live_state, make_trainer, np64, one_step, param_snapshot,
                              restate, steps, twin_state)

pytestmark = pytest.mark.gpu


# ---- 1. op level --------------------------------------------------------------------------------------------------------------
SIZES = [1, 3, 4095, 4096, 4097, 2 ** 20 + 5]
GUARD = 1.5e30


def _slot(n, off, dtype=torch.float32):
    """a tensor of n elements ``off`` elements into a larger buffer whose other elements are sentinels"""
    base = torch.full((n + 8,), GUARD if dtype == torch.float32 else 77, dtype=dtype, device="cuda")
    return base, base[off:off + n]


def _guards_intact(base, off, n):
    g = base.clone()
    g[off:off + n] = base[0]
    return bool((g == base[0]).all())


@pytest.mark.parametrize("ramp", [True, False])
def test_op_level_against_the_restatement(ramp):
    from srgan_amd import ema, ops
    T, decay = 20, 0.999
    rng = np.random.default_rng(5)
    avg, same, cpy = [], [], []                       # averaged records, p == e records, copy records
    for n in SIZES:
        for off in (4, 1):                            # 16-byte aligned; offset by one element (the scalar path)
            eb, e = _slot(n, off)
            pb, p = _slot(n, off)
            e0 = rng.standard_normal(n).astype(np.float32)
            e.copy_(torch.from_numpy(e0))
            avg.append(dict(n=n, off=off, eb=eb, e=e, pb=pb, p=p, ref=e0.astype(np.float64), M=float(np.abs(e0).max())))
    for n, off_e, off_p in ((4097, 4, 4), (5, 1, 4), (8192, 4, 1)):
        eb, e = _slot(n, off_e)
        pb, p = _slot(n, off_p)
        v = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
        e.copy_(v), p.copy_(v)
        same.append(dict(n=n, eb=eb, e=e, off=off_e, p=p, start=e.clone()))
    for n, dtype, off in ((1, torch.int64, 4), (4097, torch.float32, 4), (37, torch.float32, 1)):
        db, d = _slot(n, off, dtype)
        sb, s = _slot(n, off, dtype)
        cpy.append(dict(n=n, off=off, db=db, d=d, s=s, dtype=dtype))
    records = [(r["e"].data_ptr(), r["p"].data_ptr(), r["n"], ema.KIND_AVERAGE) for r in avg + same]
    records += [(r["d"].data_ptr(), r["s"].data_ptr(), r["n"] * r["d"].element_size() // 4, ema.KIND_COPY) for r in cpy]
    table, n_rec, chunks = ema.build_table(records, torch.device("cuda"))
    state = ops.ema_state_new(torch.device("cuda"), decay, ramp, 0)
    for t in range(1, T + 1):
        for r in avg:                                 # p redrawn before each update
            p = rng.standard_normal(r["n"]).astype(np.float32)
            r["p"].copy_(torch.from_numpy(p))
            r["ref"] = restate(r["ref"], p, t, decay, ramp)
            r["M"] = max(r["M"], float(np.abs(p).max()))
        for r in cpy:
            if r["dtype"] == torch.int64:
                src = torch.from_numpy(rng.integers(-2 ** 62, 2 ** 62, r["n"]))
            else:
                src = torch.from_numpy(rng.standard_normal(r["n"]).astype(np.float32))
            r["s"].copy_(src)
            r["want"] = src
        ops.ema_multi_dev_(table, n_rec, chunks, state)
        for r in cpy:
            assert torch.equal(r["d"].cpu(), r["want"]), ("copy record", r["n"], r["dtype"], t)
    n_dev, ramp_dev, decay_dev, c_dev = ema.read_state(state)
    assert n_dev == T and ramp_dev == int(ramp) and decay_dev == np.float32(decay)
    assert np.float32(c_dev) == np.float32(1) - ema.decay_at(T, decay, ramp)
    worst = 0.0
    for r in avg:
        got = np64(r["e"])
        M = max(r["M"], float(np.abs(got).max()))
        err = float(np.abs(got - r["ref"]).max())
        worst = max(worst, err / bound(T, M))
        assert err <= bound(T, M), (r["n"], r["off"], err, bound(T, M))
        assert _guards_intact(r["eb"], r["off"], r["n"]) and _guards_intact(r["pb"], r["off"], r["n"]), (r["n"], r["off"])
    print(f"op level, ramp={ramp}: worst error / bound = {worst:.3f}")
    for r in same:
        assert torch.equal(r["e"], r["start"]) and _guards_intact(r["eb"], r["off"], r["n"]), ("p == e record moved", r["n"])
    for r in cpy:
        assert _guards_intact(r["db"], r["off"], r["n"]), ("copy record wrote outside", r["n"])


def test_wrappers_refuse_bad_arguments_on_the_device():
    from srgan_amd import ops
    from srgan_amd._lib import SrganHipError
    with pytest.raises(SrganHipError, match="ema_state_init"):
        ops.ema_state_new(torch.device("cuda"), 1.0, True, 0)
    st = ops.ema_state_new(torch.device("cuda"), 0.5, True, 0)
    with pytest.raises(SrganHipError, match="ema_state_set_decay"):
        ops.ema_state_set_decay(st, -0.25)


# ---- 2. no existing behaviour changes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,n", [(False, 3), (True, 5)])
def test_live_training_is_bit_identical_with_the_ema_on(graph, n):
    off = make_trainer("T", 4, 2, seed=2)
    on = make_trainer("T", 4, 2, seed=2).enable_ema()
    assert on.G_ema is not None and on.E_ema is not None and off.G_ema is None and off.E_ema is None
    if graph:
        off.enable_graph(), on.enable_graph()
    a, b = steps(off, 4, n, 500), steps(on, 4, n, 500)
    np.testing.assert_array_equal(a, b)                                   # the three returned losses of every step
    assert_same(live_state(off), live_state(on), "EMA on vs off")         # parameters, buffers, Adam moments and step counts
    assert on.ema_updates == n and off.ema_updates == 0
    if graph:
        assert on.graph_active and off.graph_active


# ---- 3. trajectory --------------------------------------------------------------------------------------------------------------
def _amax(v):
    return float(np.abs(v).max())


def _follow(sg, n, first_seed, decay, ramp, n0=0, batch=4):
    """n steps; the restatement applied to snapshots of the live networks -> ({net: {param: e_ref}}, {net: {param: M}})"""
    pairs = [(name, live, twin) for name, live, twin in (("G", sg.G, sg.G_ema), ("E", sg.E, sg.E_ema)) if twin is not None]
    ref = {name: param_snapshot(twin) for name, _, twin in pairs}
    M = {name: {k: _amax(v) for k, v in ref[name].items()} for name, _, _ in pairs}
    torch.manual_seed(first_seed)
    for s in range(n):
        one_step(sg, batch, first_seed + s)
        for name, live, _ in pairs:
            snap = param_snapshot(live)
            ref[name] = {k: restate(ref[name][k], snap[k], n0 + s + 1, decay, ramp) for k in snap}
            M[name] = {k: max(M[name][k], _amax(snap[k])) for k in snap}
    for name, _, twin in pairs:
        M[name] = {k: max(M[name][k], _amax(np64(v))) for k, v in twin.named_parameters()}
    return ref, M


@pytest.mark.parametrize("decay,ramp", [(0.999, True), (0.9, False)])
def test_trajectory_follows_the_restatement(decay, ramp):
    from srgan_amd import ema
    sg = make_trainer("T", 4, 2, seed=3).enable_ema(decay=decay, ramp=ramp)
    assert_same({k: v for k, v in twin_state(sg).items()},
                {k: v for k, v in live_state(sg).items() if k.startswith(("G.", "E."))}, "copies start at the live weights")
    ref, M = _follow(sg, 5, 600, decay, ramp)
    assert sg.ema_updates == 5 and sg._ema.device_updates() == 5
    for name, twin in (("G", sg.G_ema), ("E", sg.E_ema)):
        check_within_bound(twin, ref[name], 5, M[name], f"{name}_ema")
        assert not twin.training and not any(p.requires_grad for p in twin.parameters())
        assert any(not torch.equal(a, b) for a, b in zip(twin.parameters(), getattr(sg, name).parameters()))   # it is an average
    # one network only
    sg2 = make_trainer("T", 4, 2, seed=3).enable_ema(nets=("G",))
    assert sg2.E_ema is None and isinstance(sg2.G_ema, type(sg2.G))
    sg2.disable_ema()
    assert sg2.G_ema is None and sg2.ema_updates == 0
    assert isinstance(ema.decay_at(1, decay, ramp), np.float32)


# ---- 4. graph mode --------------------------------------------------------------------------------------------------------------
def test_graph_replays_update_the_copies_like_eager_steps():
    eager = make_trainer("T", 4, 2, seed=4).enable_ema()
    sg = make_trainer("T", 4, 2, seed=4).enable_ema().enable_graph()
    seen = []
    np.testing.assert_array_equal(steps(eager, 4, 5, 700), steps(sg, 4, 5, 700, after=lambda t, s: seen.append(t.graph_active)))
    assert seen == [False, True, True, True, True]          # step 0 eager, step 1 recorded, 3 replays
    assert_same(twin_state(eager), twin_state(sg), "copies, eager vs graph")
    assert sg.ema_updates == eager.ema_updates == 5 and sg._ema.device_updates() == 5


def test_set_ema_decay_between_replays_keeps_the_recording():
    sg = make_trainer("T", 4, 2, seed=5).enable_ema(decay=0.9, ramp=False).enable_graph()
    steps(sg, 4, 3, 710)
    assert sg.graph_active
    sg.set_ema_decay(0.5)
    assert sg.graph_active
    ref, M = _follow(sg, 1, 720, 0.5, False, n0=3)
    assert sg.graph_active and sg.ema_updates == 4 and sg._ema.device_updates() == 4
    for name, twin in (("G", sg.G_ema), ("E", sg.E_ema)):
        check_within_bound(twin, ref[name], 1, M[name], f"{name}_ema after set_ema_decay")
    # the restatement with the OLD decay is out of reach of the bound: the new decay is what ran
    with pytest.raises(ValueError):
        sg.set_ema_decay(1.0)


def test_enable_ema_after_a_recording_drops_it():
    sg = make_trainer("T", 4, 2, seed=6).enable_graph()
    steps(sg, 4, 3, 730)
    assert sg.graph_active
    sg.enable_ema()
    old = sg._graph.graph
    torch.manual_seed(740)
    for i in range(4):
        one_step(sg, 4, 740 + i)
        assert sg._graph.graph is not old                   # never the recording made without the EMA
        assert sg._ema.device_updates() == i + 1 == sg.ema_updates
        assert sg.graph_active == (i >= 1)                  # eager, then recorded again
    # re-creating the EMA and switching it off drop the recording too
    for change in (sg.enable_ema, sg.disable_ema):
        assert sg.graph_active
        old = sg._graph.graph
        change()
        one_step(sg, 4, 750)
        assert sg._graph.graph is not old and not sg.graph_active
        one_step(sg, 4, 751)
        assert sg.graph_active
    assert sg.G_ema is None and sg.ema_updates == 0


def test_enable_ema_inside_a_capture_raises():
    sg = make_trainer("T", 4, 2, seed=6)
    g = torch.cuda.CUDAGraph()
    warm = torch.ones(8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        warm.add_(1.0)
        with pytest.raises(RuntimeError, match="capture"):
            sg.enable_ema()
    assert sg.G_ema is None


# ---- 5. inference sees the update -------------------------------------------------------------------------------------------------
def _fresh_twins(sg):
    from srgan_amd import model
    from tests.common import TIER_T
    g, e = TIER_T["G"], TIER_T["E"]
    G = model.SingleGenerator(g["nch_in"], g["nch"], g["reduce"], g["num_cls"], g["res_num"], "instance", num_con=g["num_con"])
    E = model.Encoder(e["nch_in"], e["nch_out"], e["nch"], e["num_cls"], "instance", e["num_con"], "cuda")
    G.load_state_dict(sg.G_ema.state_dict())
    E.load_state_dict(sg.E_ema.state_dict())
    return G.cuda().eval(), E.cuda().eval()


def _sample_inputs():
    from oracle import trainer as otrainer
    x, _ = otrainer.synthetic_batch(2, 128, 4, seed=9)
    g = torch.Generator().manual_seed(9)
    code = torch.cat([torch.eye(4)[[1, 2]], torch.randn(2, 8, generator=g)], 1)
    return x.cuda(), code.cuda()


def _mu(E, x):
    return E.fcmean(E.features(x))


def test_forward_of_the_copies_sees_every_update():
    from srgan_amd import ops
    from srgan_amd.inference import GraphedForward
    sg = make_trainer("T", 4, 2, seed=7).enable_ema(decay=0.5, ramp=False)
    x, code = _sample_inputs()
    torch.manual_seed(800)
    with ops.pack_cache():
        one_step(sg, 4, 800)
        with torch.no_grad():                               # cached packed operands of the copies now exist ...
            y1, mu1 = sg.G_ema(x, code).clone(), _mu(sg.E_ema, x).clone()
    gf_live = GraphedForward(lambda a, c: sg.G(a, c), x, code)
    gf_twin = GraphedForward(lambda a, c: sg.G_ema(a, c), x, code)
    with ops.pack_cache():
        with torch.no_grad():
            assert torch.equal(sg.G_ema(x, code), y1) and torch.equal(_mu(sg.E_ema, x), mu1)
        one_step(sg, 4, 801)                                # ... and go stale here
        with torch.no_grad():
            y_in, mu_in = sg.G_ema(x, code).clone(), _mu(sg.E_ema, x).clone()
    with torch.no_grad():
        y_out, mu_out = sg.G_ema(x, code).clone(), _mu(sg.E_ema, x).clone()
        G2, E2 = _fresh_twins(sg)
        y_want, mu_want = G2(x, code), _mu(E2, x)
        with ops.pack_cache():
            y_in2, mu_in2 = sg.G_ema(x, code).clone(), _mu(sg.E_ema, x).clone()
    assert not torch.equal(y1, y_want) and not torch.equal(mu1, mu_want)        # the second update moved the copies
    for got, want, what in ((y_in, y_want, "G_ema inside the step's scope"), (y_out, y_want, "G_ema outside a scope"),
                            (y_in2, y_want, "G_ema inside a new scope"), (mu_in, mu_want, "E_ema mu inside the step's scope"),
                            (mu_out, mu_want, "E_ema mu outside a scope"), (mu_in2, mu_want, "E_ema mu inside a new scope")):
        assert torch.equal(got, want), what
    # a GraphedForward built before the second update: the copy behaves as the live generator does after an optimiser step
    with torch.no_grad():
        live_follows = torch.equal(gf_live(x, code), sg.G(x, code))
        twin_follows = torch.equal(gf_twin(x, code), y_want)
    print(f"GraphedForward built before an update replays the new weights: live {live_follows}, copy {twin_follows}")
    assert twin_follows == live_follows


# ---- 6. ema_weights() -------------------------------------------------------------------------------------------------------------
def test_ema_weights_scope():
    from srgan_amd import inference
    from srgan_amd.losses import class_encode
    sg = make_trainer("T", 4, 2, seed=8).enable_ema(decay=0.5, ramp=False).enable_graph()
    steps(sg, 4, 3, 810)
    assert sg.graph_active
    liveG, liveE = sg.G, sg.E
    before = live_state(sg)
    x, _ = _sample_inputs()
    tgt = torch.tensor([[1], [2]])
    with sg.ema_weights() as scope:
        assert scope is sg and sg.G is sg.G_ema and sg.E is sg.E_ema
        with torch.no_grad():
            img, info = sg.G_transformation(tgt, x, True, x)
            mu = sg.E_ema(x)[1]
            want = sg.G_ema(x, torch.cat([class_encode(tgt, "cuda", np.eye(4)), mu], 1))
        assert torch.equal(info[1], mu) and torch.equal(img, want)
        with torch.no_grad():
            live_img = liveG(x, torch.cat([class_encode(tgt, "cuda", np.eye(4)), liveE(x)[1]], 1))
        assert not torch.equal(img, live_img)
        with pytest.raises(RuntimeError, match="ema_weights"):
            one_step(sg, 4, 820)
        torch.manual_seed(1)
        out = inference.get_output_tensors(sg, [(x[0].cpu(), 1)], 0, (0, 1, 2, 3), random_sample_num=2)
        assert out["target_random"].shape == (2, 3, 128, 128) and torch.isfinite(out["identity"]).all()
    assert sg.G is liveG and sg.E is liveE
    assert_same(before, live_state(sg), "live state across ema_weights()")
    torch.manual_seed(830)
    one_step(sg, 4, 830), one_step(sg, 4, 831)
    assert sg.graph_active and sg.ema_updates == 5 == sg._ema.device_updates()
    sg.disable_ema()
    with pytest.raises(RuntimeError, match="enable_ema"):
        with sg.ema_weights():
            pass


# ---- 7. batch-norm networks ---------------------------------------------------------------------------------------------------------
def test_batch_norm_buffers_are_carried_over():
    from oracle import params
    from srgan_amd import model
    from tests.batch_common import batch_fill
    G = batch_fill(model.SingleGenerator(3, 4, 2, 2, 1, "batch", num_con=12), 0)
    E = batch_fill(model.Encoder(3, 8, 4, 4, "batch", 4, "cuda"), 2)
    D = model.SingleDiscriminator_solo_multi(3, 4, 2, 4, "batch", 4)
    D.load_state_dict(params.fill(params.discriminator_spec(nch_in=3, nch=4, reduce=2, num_cls=4, n_class=4), 1))
    sg = make_trainer(nets=(G.cuda(), D.cuda(), E.cuda()), seed=0).enable_ema()
    torch.manual_seed(100)
    for s in range(3):
        one_step(sg, 4, 100 + s)
        n_buf = 0
        for live, twin in ((sg.G, sg.G_ema), (sg.E, sg.E_ema)):
            assert not any(m.training for m in twin.modules()) and live.training
            tb = dict(twin.named_buffers())
            for k, v in live.named_buffers():
                assert k.endswith(("running_mean", "running_var", "num_batches_tracked"))
                assert v.dtype == tb[k].dtype and torch.equal(v, tb[k]), (s, k)
                n_buf += 1
        assert n_buf > 0 and any(int(v) > 0 for k, v in sg.G_ema.named_buffers() if k.endswith("num_batches_tracked"))
    with torch.no_grad():
        x, code = _sample_inputs()
        assert torch.isfinite(sg.G_ema(x, code)).all()
    for k, v in sg.G.named_buffers():
        assert torch.equal(v, dict(sg.G_ema.named_buffers())[k]), k              # an eval-mode forward of the copy wrote nothing


# ---- 8. pretrained-E recipe -----------------------------------------------------------------------------------------------------------
def test_frozen_trunk_stays_bit_identical_in_the_copy():
    from srgan_amd import optim as hoptim
    from tests.common import build_hip_nets
    G, D, E = build_hip_nets("T")
    heads = [p for k, p in E.named_parameters() if k.startswith(("fcmean", "fcvar"))]
    optE = hoptim.Adam(heads, lr=1e-3, betas=(0.5, 0.999))
    sg = make_trainer(nets=(G, D, E), seed=9, opts=(None, None, optE)).enable_ema()
    start = {k: v.detach().clone() for k, v in E.named_parameters()}
    steps(sg, 4, 3, 840)
    twin = dict(sg.E_ema.named_parameters())
    for k, p in E.named_parameters():
        if k.startswith("fcmean"):                 # the trained head moved, and its copy lags behind it
            assert not torch.equal(p, start[k]) and not torch.equal(twin[k], p), k
        elif k.startswith("fcvar"):                # in optE, but with encoded_feature="mu" and KL = 0 logvar feeds no loss: a
            assert torch.equal(twin[k], p) == torch.equal(p, start[k]), k      # parameter that never moved is exact in the copy
        else:
            assert torch.equal(p, start[k]) and torch.equal(twin[k], p), k


# ---- 9. bf16 mode -----------------------------------------------------------------------------------------------------------------------
def test_bf16_mode_keeps_float32_copies_within_the_bound():
    from srgan_amd import ops
    ops.set_compute_dtype("bf16")
    try:
        sg = make_trainer("T", 4, 2, seed=10).enable_ema()
        ref, M = _follow(sg, 3, 850, 0.999, True)
        for name, twin in (("G", sg.G_ema), ("E", sg.E_ema)):
            assert all(v.dtype == torch.float32 for v in twin.parameters())
            check_within_bound(twin, ref[name], 3, M[name], f"{name}_ema (bf16 mode)")
    finally:
        ops.set_compute_dtype("fp32")


# ---- 10. state round trip ---------------------------------------------------------------------------------------------------------------
def test_state_round_trip():
    whole = make_trainer("T", 4, 2, seed=11).enable_ema()
    steps(whole, 4, 4, 860)

    first = make_trainer("T", 4, 2, seed=11).enable_ema()
    torch.manual_seed(860)
    one_step(first, 4, 860), one_step(first, 4, 861)
    rng = torch.get_rng_state()
    sd = first.ema_state_dict()
    assert sd["updates"] == 2 and sd["decay"] == 0.999 and sd["ramp"] is True and set(sd) == {"G", "E", "updates", "decay", "ramp"}
    assert list(sd["G"]) == list(first.G.state_dict()) and list(sd["E"]) == list(first.E.state_dict())
    second = make_trainer(nets=(first.G, first.D, first.E), seed=11, opts=(first.optG, first.optD, first.optE))
    second.load_ema_state_dict(sd)
    assert second.ema_updates == 2 and second._ema.device_updates() == 2
    torch.set_rng_state(rng)                         # the CPU generator where the two steps left it (make_trainer seeds it)
    one_step(second, 4, 862), one_step(second, 4, 863)
    assert second.ema_updates == whole.ema_updates == 4 and second._ema.device_updates() == 4
    assert_same(twin_state(whole), twin_state(second), "copies after a state round trip")
    # a snapshot, not an alias of the copies
    assert not torch.equal(sd["G"]["down_convs.0.weight"], second.G_ema.state_dict()["down_convs.0.weight"])


# ---- 11. two ranks on the one device over gloo --------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_worker(rank, world, port, out_q, graph):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), SRGAN_DP_DEVICE="0", SRGAN_DP_BACKEND="gloo")
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "style-restricted_gan_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    from oracle import trainer as otrainer
    from srgan_amd import dp
    dp.init_from_env()
    assert dp.world_size() == world and dp.is_distributed()
    gb = 4
    sg = make_trainer("T", gb, 2, seed=0).enable_ema(decay=0.5, ramp=False)
    if graph:
        sg.enable_graph()
    gen = torch.Generator().manual_seed(77)

    def noise(batch, ndim):                          # every rank draws the GLOBAL noise and keeps its rows
        full = torch.randn(batch * world, ndim, generator=gen)
        return full[rank * batch:(rank + 1) * batch].clone()
    sg.noise_fn = noise
    per = gb // world
    torch.manual_seed(5)                             # the reparametrisation noise: the same on both ranks
    for s in range(3):
        x, label = otrainer.synthetic_batch(gb, 128, 4, seed=300 + s)
        sl = slice(rank * per, (rank + 1) * per)
        sg.train(x[sl].cuda(), {"source": label["source"][sl].cuda(), "target": label["target"][sl]})
    twins = {k: v.cpu().numpy().copy() for k, v in twin_state(sg).items()}
    lives = {k: v.cpu().numpy().copy() for k, v in live_state(sg).items() if k.startswith(("G.", "E."))}
    out_q.put((rank, twins, lives, sg.ema_updates, sg._ema.device_updates(), sg.graph_active))
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world, graph, timeout=240):
    """start the rank processes, collect one result per rank and ALWAYS reap them (tests/test_dp_gpu.py)"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q, graph)) for r in range(world)]
    try:
        for p in procs:
            p.start()
        res = sorted([q.get(timeout=timeout) for _ in procs], key=lambda t: t[0])
        for p in procs:
            p.join(timeout=120)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
                if p.is_alive():
                    p.kill()
                    p.join(timeout=10)
    assert [p.exitcode for p in procs] == [0] * world, [p.exitcode for p in procs]
    return res


@pytest.mark.parametrize("graph", [False, True])
def test_two_ranks_hold_identical_copies(graph):
    a, b = _spawn(2, graph)
    assert a[3] == b[3] == 3 and a[4] == b[4] == 3 and a[5] == b[5] == graph
    assert a[1].keys() == b[1].keys() and len(a[1]) > 0
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), ("live weights differ across ranks", k)
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k]), ("copies differ across ranks", k)
    assert any(not np.array_equal(a[1][k], a[2][k]) for k in a[1])       # they are averages, not the live weights
