"""GPU: the device-side gradient guard (optim.Adam.enable_grad_guard, SRGAN_training.enable_grad_guard, srgan_grad_guard_* and
srgan_adam_multi_dev_guard).  The yardstick for the norm is the float64 restatement of tests/guard_common.py with its derived
bound ((D + 1) / 2 + 2) * 2^-24 * ref, D = 24; everything else is bit-equality."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.guard_common import (OPT_STEPS, AdamSet, Reducer, all_finite, assert_same, batch_of, f32_bits, live_state, make_trainer,
                                norm_bound, ref_norm, run, scale_bound, slot, split_steps, train_on, twin_state)

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4095, 4096, 4097, 8197, 40000]
MIXED = [(n, 4) for n in SIZES] + [(4097, 1), (5, 1), (8197, 1)]      # (elements, offset): offset 1 refuses the 16-byte path


# ---- 1. the norm ---------------------------------------------------------------------------------------------------------------
def _norm_sets():
    rng = np.random.default_rng(11)
    mags = 10.0 ** np.linspace(-6, 3, len(SIZES))
    aligned = [slot(n, 4, rng.standard_normal(n) * m) for n, m in zip(SIZES, mags)]
    views = [slot(n, 1, rng.standard_normal(n) * m) for n, m in zip(SIZES, mags[::-1])]
    pool = torch.from_numpy(rng.standard_normal(300 * 7 + 8).astype(np.float32) * 1e-3).cuda()
    tiny, at = [], 0
    for n in rng.integers(1, 8, 300):                # 300 tensors of 1..7 elements, packed: every alignment occurs
        tiny.append(pool[at:at + n])
        at += int(n)
    # more chunks than the launch has blocks (2048): the grid stride
    big = [slot(2049 * 4096 + 5, 4, rng.standard_normal(2049 * 4096 + 5) * 0.03)]
    return {"sizes": aligned, "views": views, "tiny300": tiny, "mixed": aligned + views + tiny, "stride": big}


@pytest.fixture(scope="module")
def norm_sets():
    return _norm_sets()


@pytest.mark.parametrize("which", ["sizes", "views", "tiny300", "mixed", "stride"])
def test_norm_is_within_the_bound_and_repeats_bit_for_bit(norm_sets, which):
    grads = norm_sets[which]
    before = [g.clone() for g in grads]
    ref = ref_norm(grads)
    red = Reducer(grads)
    a = red.reduce()
    b = red.reduce()
    err = abs(a["norm"] - ref)
    print(f"{which}: norm = {a['norm']!r}, ref = {ref!r}, error / bound = {err / norm_bound(ref):.4f}")
    assert err <= norm_bound(ref), (which, a["norm"], ref, err, norm_bound(ref))
    assert f32_bits(a["norm"]) == f32_bits(b["norm"])
    assert a["scale"] == 1.0 and not a["skip"] and (b["steps"], b["skipped"], b["clipped"]) == (2, 0, 0) and a["max_norm"] is None
    assert all(torch.equal(g, g0) for g, g0 in zip(grads, before))


def test_norm_does_not_depend_on_the_load_path(norm_sets):
    """an element has the same owner and slot whether its chunk is read 16 bytes at a time or element by element"""
    aligned = norm_sets["sizes"]
    shifted = [slot(g.numel(), 1, g) for g in aligned]
    assert f32_bits(Reducer(aligned).reduce()["norm"]) == f32_bits(Reducer(shifted).reduce()["norm"])


# ---- 2. inactive = identical -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [None, "above"])
def test_idle_guard_is_bit_identical_to_the_plain_update(max_norm):
    a = AdamSet(MIXED, seed=3)
    b = a.clone()
    ref = ref_norm(a.g)
    red = Reducer(a.g, None if max_norm is None else 1.5 * ref)
    g0 = [g.clone() for g in a.g]
    for _ in range(2):
        a.step_guarded(red)
        b.step_plain()
    a.assert_equals(b, f"idle guard (max_norm={max_norm})")
    st = red.stats()
    assert (st["steps"], st["skipped"], st["clipped"], st["scale"], st["skip"]) == (2, 0, 0, 1.0, False)
    assert a.t() == b.t() == 2 and all(torch.equal(x, y) for x, y in zip(a.g, g0))


# ---- 3. clip -------------------------------------------------------------------------------------------------------------------
def test_clip_scales_the_update_and_leaves_the_gradients():
    a = AdamSet(MIXED, seed=4, g_scale=3.0)
    ref = ref_norm(a.g)
    max_norm = float(np.float32(0.37 * ref))
    red = Reducer(a.g, max_norm)
    g0 = [g.clone() for g in a.g]
    a.step_guarded(red)
    st = red.stats()
    want = max_norm / (ref + 1e-6)
    print(f"clip: scale = {st['scale']!r}, want = {want!r}, error / bound = {abs(st['scale'] - want) / scale_bound(want):.4f}")
    assert abs(st["norm"] - ref) <= norm_bound(ref)
    assert abs(st["scale"] - want) <= scale_bound(want) and st["scale"] < 1.0
    assert (st["steps"], st["skipped"], st["clipped"], st["skip"]) == (1, 0, 1, False) and st["max_norm"] == max_norm
    assert all(torch.equal(x, y) for x, y in zip(a.g, g0)), "the gradient tensors were modified"
    start = AdamSet(MIXED, seed=4, g_scale=3.0)                       # the same start (same seed)
    b = start.clone(g=[g * st["scale"] for g in g0])                  # an fp32 multiply by the read-back value
    b.step_plain()
    a.assert_equals(b, "clipped update vs the plain update on g * scale")
    # raising the threshold between steps: the next step is not clipped
    red.ops.grad_guard_state_set_max_norm(red.state, 2.0 * ref)
    a.step_guarded(red)
    b2 = b.clone(steps_done=1, g=g0)
    b2.step_plain()
    a.assert_equals(b2, "unclipped step after set_max_norm")
    st = red.stats()
    assert (st["steps"], st["clipped"], st["scale"]) == (2, 1, 1.0)


# ---- 4. skip -------------------------------------------------------------------------------------------------------------------
SKIP_SHAPES = [(4096 + 9, 4), (1, 4), (8197, 1), (40, 4)]
POSITIONS = {"first element of the first tensor": (0, 0), "last element of a scalar tail": (0, 4096 + 8), "1-element tensor": (1, 0),
             "misaligned view": (2, 5000)}


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf"), 3e19])
@pytest.mark.parametrize("where", list(POSITIONS))
def test_non_finite_gradient_skips_the_whole_step(where, value):
    where_t, where_i = POSITIONS[where]               # (3e19 is finite: its square overflows float32)
    a = AdamSet(SKIP_SHAPES, seed=6)
    clean = a.g[where_t][where_i].clone()
    a.g[where_t][where_i] = value
    red = Reducer(a.g)
    before = a.snapshot()
    a.step_guarded(red)
    st = red.stats()
    a.assert_equals(before, f"skipped step ({where}, {value})")
    assert st["skip"] and (st["steps"], st["skipped"], st["clipped"]) == (1, 1, 0) and not np.isfinite(st["norm"]), st
    assert a.t() == 1, "the Adam record's t advances on a skipped step"
    # a clean step follows: it updates like the plain kernel at t = 2
    a.g[where_t][where_i] = clean
    b = a.clone(steps_done=1)
    a.step_guarded(red)
    b.step_plain()
    a.assert_equals(b, f"clean step after a skipped one ({where}, {value})")
    st = red.stats()
    assert not st["skip"] and (st["steps"], st["skipped"], st["clipped"]) == (2, 1, 0) and np.isfinite(st["norm"]) and a.t() == 2
    assert any(not torch.equal(x, y) for x, y in zip(a.p, before[0]))


# ---- 5. bad arguments ------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_bad_arguments_on_the_device():
    from srgan_amd import ops
    from srgan_amd._lib import SrganHipError
    dev = torch.device("cuda")
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(SrganHipError, match="grad_guard_state_init"):
            ops.grad_guard_state_new(dev, bad)
    st = ops.grad_guard_state_new(dev, 2.0)
    with pytest.raises(SrganHipError, match="grad_guard_state_set_max_norm"):
        ops.grad_guard_state_set_max_norm(st, -0.5)
    with pytest.raises(SrganHipError, match="grad_guard_workspace"):
        ops.grad_guard_workspace_bytes(0)
    g = torch.ones(5000, device="cuda")
    table, n, chunks = ops.grad_guard_table([g], dev)
    small = torch.zeros(4, dtype=torch.uint8, device="cuda")              # two chunks need 8 bytes
    with pytest.raises(SrganHipError, match="workspace"):
        ops.grad_guard_reduce_(table, n, chunks, small, st)
    with pytest.raises(SrganHipError, match="grad_guard_reduce"):
        ops.grad_guard_reduce_(table, 0, chunks, small, st)
    with pytest.raises(SrganHipError, match="adam_multi_dev_guard"):
        ops.adam_multi_dev_guard_(table, 0, 1, st, st)
    with pytest.raises(SrganHipError, match="contiguous"):
        ops.grad_guard_table([torch.ones(4, 4, device="cuda").t()], dev)
    with pytest.raises(SrganHipError, match="float32"):
        ops.grad_guard_table([torch.ones(4, device="cuda", dtype=torch.float64)], dev)
    read = ops.grad_guard_state_read(st)                                   # nothing was launched on the record
    assert read == dict(max_norm=2.0, norm=0.0, scale=1.0, skip=False, steps=0, skipped=0, clipped=0)
    assert int(small.sum()) == 0


def test_optimiser_level_guard_spans_groups_and_cohorts():
    """one decision for every parameter of the call: a NaN in one group's gradient holds back the other group as well"""
    from srgan_amd import optim
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(n, device="cuda")) for n in (5000, 7, 4096)]
    opt = optim.Adam([{"params": ps[:2]}, {"params": ps[2:], "lr": 1e-2}], lr=1e-3, betas=(0.5, 0.999))
    twin_ps = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    twin = optim.Adam([{"params": twin_ps[:2]}, {"params": twin_ps[2:], "lr": 1e-2}], lr=1e-3, betas=(0.5, 0.999))
    opt.enable_grad_guard(max_norm=None)
    assert opt.grad_guard_fingerprint() is not None and "guard" not in str(opt.state_dict().keys())

    def grads(seed, poison=False):
        g = torch.Generator().manual_seed(seed)
        out = [torch.randn(p.numel(), generator=g).cuda() for p in ps]
        if poison:
            out[2][17] = float("nan")
        return out
    for p, q, g in zip(ps, twin_ps, grads(1)):
        p.grad, q.grad = g.clone(), g.clone()
    opt.step(), twin.step()
    ps[1].grad = twin_ps[1].grad = None               # one parameter sits out from here on: another cohort in group 0
    held = [p.detach().clone() for p in ps]
    bad = grads(2, poison=True)
    ps[0].grad, ps[2].grad = bad[0], bad[2]           # the NaN is in group 1 ...
    opt.step()
    assert all(torch.equal(p.detach(), h) for p, h in zip(ps, held)), "a skipped step wrote a parameter"       # ... group 0 waits too
    st = opt.grad_guard_stats()
    assert st["skip"] and (st["steps"], st["skipped"]) == (2, 1)
    assert opt.state[ps[0]]["step"] == 2 and opt.state[ps[1]]["step"] == 1 and opt.state[ps[2]]["step"] == 2
    # a skipped step is a step that moved nothing: the next clean one equals a plain optimiser's whose counters stand one ahead
    for q in (twin_ps[0], twin_ps[2]):
        twin.state[q]["step"] += 1
    good = grads(3)
    for i in (0, 2):
        ps[i].grad, twin_ps[i].grad = good[i].clone(), good[i].clone()
    opt.step(), twin.step()
    for p, q in zip(ps, twin_ps):
        assert torch.equal(p.detach(), q.detach())
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[p][key], twin.state[q][key])
    opt.set_max_norm(1e-3)
    assert opt.grad_guard_stats()["max_norm"] == float(np.float32(1e-3))
    opt.disable_grad_guard()
    assert opt.grad_guard_fingerprint() is None


# ---- 6. guard on, nothing triggers ---------------------------------------------------------------------------------------------
def _counts(sg):
    return {n: (st["steps"], st["skipped"], st["clipped"]) for n, st in sg.grad_guard_stats().items()}


@pytest.mark.parametrize("graph,n,max_norm", [(False, 3, None), (True, 5, 1e30)])
def test_training_is_bit_identical_with_an_idle_guard(graph, n, max_norm):
    off = make_trainer("T", 4, 2, seed=2)
    on = make_trainer("T", 4, 2, seed=2).enable_grad_guard(max_norm)
    if graph:
        off.enable_graph(), on.enable_graph()
    a, b = run(off, 500, n), run(on, 500, n)
    np.testing.assert_array_equal(a, b)                                   # the three returned losses of every step
    assert_same(live_state(off), live_state(on), "guard on vs off")       # parameters, buffers, Adam moments and step counts
    assert _counts(on) == {k: (n * OPT_STEPS[k], 0, 0) for k in "GDE"}
    assert off.grad_guard_stats() == {"G": None, "D": None, "E": None}
    if graph:
        assert on.graph_active and off.graph_active


def test_bf16_mode_is_bit_identical_with_an_idle_guard():
    from srgan_amd import ops
    ops.set_compute_dtype("bf16")
    try:
        off = make_trainer("T", 4, 2, seed=3)
        on = make_trainer("T", 4, 2, seed=3).enable_grad_guard()
        np.testing.assert_array_equal(run(off, 520, 2), run(on, 520, 2))
        assert_same(live_state(off), live_state(on), "guard on vs off (bf16 mode)")
        assert _counts(on) == {k: (2 * OPT_STEPS[k], 0, 0) for k in "GDE"}
    finally:
        ops.set_compute_dtype("fp32")


# ---- 7. skip in a real step ------------------------------------------------------------------------------------------------------
def test_nan_pixel_skips_the_step_and_training_goes_on():
    sg = make_trainer("T", 4, 2, seed=4).enable_grad_guard().enable_ema()
    bare = make_trainer("T", 4, 2, seed=4)
    run(sg, 600, 2), run(bare, 600, 2)
    snap_t, snap_c = split_steps(live_state(sg))
    c0 = _counts(sg)
    x, label = batch_of(602, poison=float("nan"))
    torch.manual_seed(602)
    losses = train_on(sg, x, label)
    torch.manual_seed(602)
    train_on(bare, x, label)
    after_t, after_c = split_steps(live_state(sg))
    assert_same(snap_t, after_t, "parameters / buffers / moments after a skipped step")
    bare_t, bare_c = split_steps(live_state(bare))
    assert after_c == bare_c and after_c != snap_c                        # the step counts advanced as in a normal step
    c1 = _counts(sg)
    for n in "GDE":
        assert c1[n][0] - c0[n][0] == OPT_STEPS[n] and c1[n][1] - c0[n][1] == OPT_STEPS[n] and c1[n][2] == 0, (n, c0[n], c1[n])
    assert all(st["skip"] for st in sg.grad_guard_stats().values())
    assert not all(np.isfinite(losses)), "the returned losses are not filtered"
    assert all_finite(twin_state(sg)) and sg.ema_updates == 3
    # the input does poison: the unguarded twin's weights are gone
    assert not all_finite({k: v for k, v in bare_t.items() if k.startswith(("G.", "D.", "E."))})
    # a clean fourth step moves the weights and everything is finite
    x, label = batch_of(603)
    losses = train_on(sg, x, label)
    final_t, _ = split_steps(live_state(sg))
    assert np.isfinite(losses).all() and all_finite(final_t) and all_finite(twin_state(sg))
    for net in "GDE":
        moved = [k for k in final_t if k.startswith(net + ".") and not torch.equal(final_t[k], after_t[k])]
        assert moved, f"{net} did not move in the clean step"
    c2 = _counts(sg)
    assert all(c2[n][1] == c1[n][1] and c2[n][0] - c1[n][0] == OPT_STEPS[n] for n in "GDE")


# ---- 8. the same under replay ----------------------------------------------------------------------------------------------------
def test_replayed_step_skips_like_the_eager_one():
    eager = make_trainer("T", 4, 2, seed=5).enable_grad_guard().enable_ema()
    graph = make_trainer("T", 4, 2, seed=5).enable_grad_guard().enable_ema().enable_graph()
    a = run(eager, 700, 5, poison_at=(3,))
    b = run(graph, 700, 5, poison_at=(3,))           # eager, capture, clean replay, NaN replay, clean replay
    assert graph.graph_active
    np.testing.assert_array_equal(a, b)
    assert_same(live_state(eager), live_state(graph), "guarded replay vs guarded eager")
    assert_same(twin_state(eager), twin_state(graph), "copies, guarded replay vs guarded eager")
    assert _counts(eager) == _counts(graph) == {k: (5 * OPT_STEPS[k], OPT_STEPS[k], 0) for k in "GDE"}
    assert eager.grad_guard_stats() == graph.grad_guard_stats()
    assert all_finite(live_state(graph)) and np.isnan(b[3]).any() and np.isfinite(b[4]).all()


# ---- 9. clipping -----------------------------------------------------------------------------------------------------------------
def test_clipping_threshold_changes_between_replays():
    probe = make_trainer("T", 4, 2, seed=6).enable_grad_guard()
    seen = []
    run(probe, 800, 5, between=lambda sg, s: seen.append(sg.grad_guard_stats()["E"]["norm"]))
    # E takes one optimiser step per train(), so its record shows every norm.  G and D get a threshold nothing reaches and stay on
    # the probe's trajectory; E gets one above everything seen after step 1 (a finite threshold that does not clip) and, after
    # step 2, one between the norms the probe saw at steps 3 and 4.  Until E's first clipped step the run IS the probe's, so: if
    # step 3 lies above the threshold it is clipped, otherwise step 4 lies above it and is.
    assert seen[3] != seen[4]
    high, mid = float(np.float32(2.0 * max(seen))), float(np.float32(0.5 * (seen[3] + seen[4])))
    logs = {}

    def between(name):
        log = logs.setdefault(name, [])

        def fn(sg, s):
            if s == 1:
                sg.set_grad_clip({"G": 1e30, "D": 1e30, "E": high})
            if s == 2:
                sg.set_grad_clip(mid, nets=("E",))   # graph run: between two replays
            if s >= 2 and name == "graph":
                assert sg.graph_active
            log.append(sg.grad_guard_stats())
        return fn
    eager = make_trainer("T", 4, 2, seed=6).enable_grad_guard()
    graph = make_trainer("T", 4, 2, seed=6).enable_grad_guard().enable_graph()
    a = run(eager, 800, 5, between=between("eager"))
    b = run(graph, 800, 5, between=between("graph"))
    np.testing.assert_array_equal(a, b)
    assert_same(live_state(eager), live_state(graph), "clipped replay vs clipped eager")
    assert logs["eager"] == logs["graph"]
    log = logs["graph"]
    assert all(log[s][n]["clipped"] == 0 for s in range(5) for n in "GD") and log[4]["G"]["max_norm"] == float(np.float32(1e30))
    threshold = [None, None, high, mid, mid]          # what E's step s ran under
    for s in range(5):
        st, moved = log[s]["E"], log[s]["E"]["clipped"] - (log[s - 1]["E"]["clipped"] if s else 0)
        above = threshold[s] is not None and st["norm"] > threshold[s]
        print(f"step {s}: E norm {st['norm']!r} under {threshold[s]!r}: scale {st['scale']!r}, clipped moved by {moved}")
        assert moved == int(above) and (st["scale"] < 1.0) == above, (s, st)
    assert [log[s]["E"]["norm"] for s in range(4)] == seen[:4]            # unclipped up to step 2, so step 3 saw the probe's weights
    first = 3 if seen[3] > mid else 4
    assert log[first]["E"]["clipped"] == 1 and log[first]["E"]["norm"] == seen[first] and log[2]["E"]["scale"] == 1.0


# ---- 10. recordings --------------------------------------------------------------------------------------------------------------
def test_enabling_the_guard_drops_a_recording_and_records_again():
    sg = make_trainer("T", 4, 2, seed=7).enable_graph()
    twin = make_trainer("T", 4, 2, seed=7)
    torch.manual_seed(900)
    for s in range(3):
        train_on(sg, *batch_of(900 + s))
    assert sg.graph_active
    old = sg._graph.graph
    sg.enable_grad_guard(max_norm={"G": 1e30, "D": None, "E": 1e30})
    train_on(sg, *batch_of(903))
    assert not sg.graph_active                       # one eager step: it sizes the guards' tables
    train_on(sg, *batch_of(904))
    assert sg.graph_active and sg._graph.graph is not old
    sg.set_grad_clip(1e29, nets=("G",))              # device state: the recording stays
    rec = sg._graph.graph
    train_on(sg, *batch_of(905))
    assert sg.graph_active and sg._graph.graph is rec
    assert {n: (st["steps"], st["max_norm"]) for n, st in sg.grad_guard_stats().items()} == {
        "G": (6, float(np.float32(1e29))), "D": (6, None), "E": (3, float(np.float32(1e30)))}
    sg.disable_grad_guard()
    train_on(sg, *batch_of(906))
    assert not sg.graph_active and sg.grad_guard_stats() == {"G": None, "D": None, "E": None}
    train_on(sg, *batch_of(907))
    assert sg.graph_active
    torch.manual_seed(900)
    for s in range(8):
        train_on(twin, *batch_of(900 + s))
    assert_same(live_state(twin), live_state(sg), "guard switched on and off around recordings vs a plain eager run")


def test_enabling_the_guard_inside_a_capture_raises():
    sg = make_trainer("T", 4, 2, seed=8)
    g = torch.cuda.CUDAGraph()
    warm = torch.ones(8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        warm.add_(1.0)
        with pytest.raises(RuntimeError, match="capture"):
            sg.enable_grad_guard()
    assert sg.grad_guard_stats() == {"G": None, "D": None, "E": None}


def test_first_guarded_step_inside_a_capture_raises():
    from srgan_amd import optim
    p = torch.nn.Parameter(torch.randn(100, device="cuda"))
    opt = optim.Adam([p], lr=1e-3)
    p.grad = torch.randn(100, device="cuda")
    opt.step()                                       # the cohort exists; the guard's table does not
    opt.enable_grad_guard()
    g = torch.cuda.CUDAGraph()
    warm = torch.ones(8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        warm.add_(1.0)
        with pytest.raises(RuntimeError, match="capture"):
            opt.step()


def test_foreign_optimiser_is_refused_by_name():
    from tests.common import build_hip_nets
    G, D, E = build_hip_nets("T")
    optD = torch.optim.Adam(D.parameters(), lr=1e-4, betas=(0.5, 0.999))
    sg = make_trainer(nets=(G, D, E), seed=9, opts=(None, optD, None))
    with pytest.raises(TypeError, match=r"optD is torch\.optim\.adam\.Adam"):
        sg.enable_grad_guard()
    assert sg.grad_guard_stats() == {"G": None, "D": None, "E": None}     # nothing half-enabled
    sg.enable_grad_guard(nets=("G", "E"))
    assert sg.grad_guard_stats()["G"] is not None and sg.grad_guard_stats()["D"] is None
    with pytest.raises(ValueError, match="nets"):
        sg.enable_grad_guard(nets=("G", "Q"))
    with pytest.raises(ValueError, match="no entry"):
        sg.enable_grad_guard(max_norm={"G": 1.0}, nets=("G", "E"))


# ---- 11. two ranks on the one device over gloo ---------------------------------------------------------------------------------------
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
    from srgan_amd import dp
    dp.init_from_env()
    assert dp.world_size() == world and dp.is_distributed()
    gb = 4
    sg = make_trainer("T", gb, 2, seed=0).enable_grad_guard()
    if graph:
        sg.enable_graph()
    gen = torch.Generator().manual_seed(77)

    def noise(batch, ndim):                          # every rank draws the GLOBAL noise and keeps its rows
        full = torch.randn(batch * world, ndim, generator=gen)
        return full[rank * batch:(rank + 1) * batch].clone()
    sg.noise_fn = noise
    per = gb // world
    torch.manual_seed(5)                             # the reparametrisation noise: the same on both ranks
    snap = None
    for s in range(3):
        if s == 2:
            snap = {k: v.cpu().numpy().copy() for k, v in split_steps(live_state(sg))[0].items()}
        x, label = batch_of(300 + s, gb, poison=float("nan") if s == 2 else None)      # the NaN pixel is in sample 0: rank 0's shard
        sl = slice(rank * per, (rank + 1) * per)
        assert bool(torch.isnan(x[sl]).any()) == (s == 2 and rank == 0)
        sg.train(x[sl].cuda(), {"source": label["source"][sl].cuda(), "target": label["target"][sl]})
    lives = {k: v.cpu().numpy().copy() for k, v in split_steps(live_state(sg))[0].items()}
    out_q.put((rank, snap, lives, _counts(sg), sg.graph_active))
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
def test_two_ranks_skip_together(graph):
    a, b = _spawn(2, graph)
    want = {k: (3 * OPT_STEPS[k], OPT_STEPS[k], 0) for k in "GDE"}
    assert a[3] == b[3] == want and a[4] == b[4] == graph
    assert a[1].keys() == a[2].keys() == b[2].keys() and len(a[2]) > 0
    # batch-norm-free tier: every tensor of the state is a parameter or a moment, and none of them moved on either rank
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), ("weights differ across ranks", k)
        assert np.array_equal(a[2][k], a[1][k]) and np.array_equal(b[2][k], b[1][k]), ("a skipped step moved", k)
        assert np.isfinite(a[2][k]).all(), k
