"""GPU: every Adam entry of csrc/pointwise.hip -- adam_multi_dev_ (adam_tick_kernel + adam_multi_dev_kernel), adam_multi_dev_guard_
with an idle and with a clipping guard, adam_multi_step_ (adam_multi_kernel) and adam_step_ (adam_kernel) -- held to the float64
restatement of tests/adam_common.py, one step at a time from the device's own read-back state, inside the bounds derived there.
Every element of every record is compared; the buffers are the sentinel slots of tests/test_ema_gpu.py laid out in one allocation
per quantity (adam_common.Layout), so that a store outside a record is seen wherever it lands."""
import ctypes
import struct

import numpy as np
import pytest
import torch

from tests import adam_common as ac
from tests.adam_common import f32

pytestmark = pytest.mark.gpu

ENTRIES = ["multi_dev", "guard_idle", "guard_clip", "multi_step", "single"]
CLIP = 0.37                     # max_norm of the clipping guard, as a share of the first step's gradient norm


def _dev():
    return torch.device("cuda")


# ---- records on the device ------------------------------------------------------------------------------------------------------
class Records:
    """the buffers of a Layout on the device, the pointer table over them and the views of every record"""

    def __init__(self, lay, values):
        from srgan_amd import ops
        self.ops, self.lay = ops, lay
        self.buf = {q: torch.from_numpy(lay.fill(q, values[q])).to(_dev()) for q in ac.QUANTITIES}
        assert all(b.data_ptr() % 16 == 0 for b in self.buf.values())
        self.view = {q: [self.buf[q][s:s + n] for s, n in zip(lay.start[q], lay.n)] for q in ac.QUANTITIES}
        rows = []
        for i, n in enumerate(lay.n):
            rows.extend([self.view[q][i].data_ptr() for q in ac.QUANTITIES] + [int(n)])
        self.table = ops.upload_small(struct.pack(f"{len(rows)}q", *rows), _dev())
        self.max_numel = int(lay.n.max())

    def set_g(self, g):
        self.buf["g"].copy_(torch.from_numpy(self.lay.fill("g", g)))

    def read(self):
        """{q: host image of the whole buffer}"""
        torch.cuda.synchronize()
        return {q: self.buf[q].cpu().numpy() for q in ac.QUANTITIES}

    def records_of(self, host):
        """{q: the elements of every record, flat in record order}"""
        return {q: host[q][self.lay.idx[q]] for q in ac.QUANTITIES}

    def assert_guards(self, host, what):
        for q in ac.QUANTITIES:
            assert self.lay.guards_intact(q, host[q]), f"{what}: a sentinel around the {q} records was overwritten"


def read_adam_state(state):
    from srgan_amd import _lib
    torch.cuda.synchronize()
    raw = state.cpu().numpy().tobytes()
    assert len(raw) == ctypes.sizeof(_lib.AdamState)
    return _lib.AdamState.from_buffer_copy(raw)


class Guard:
    """record, reduce table and workspace of a gradient guard over the g views (optim.Adam keeps them the same way)"""

    def __init__(self, recs, max_norm):
        ops = recs.ops
        self.ops = ops
        self.state = ops.grad_guard_state_new(_dev(), max_norm)
        self.table, self.n, self.chunks = ops.grad_guard_table(recs.view["g"], _dev())
        self.ws = torch.empty(ops.grad_guard_workspace_bytes(self.chunks), dtype=torch.uint8, device=_dev())

    def reduce(self):
        self.ops.grad_guard_reduce_(self.table, self.n, self.chunks, self.ws, self.state)

    def read(self):
        return self.ops.grad_guard_state_read(self.state)


def _norm64(g):
    g = g.astype(np.float64)
    return float(np.sqrt(np.dot(g, g)))


class Runner:
    """one entry over one set of records: ``step(t)`` runs step t and returns what the restatement needs of it --
    (step_size, inv_sqrt_bc2, scale): the device's own where a record holds them, ``tick`` where the host derived them"""

    def __init__(self, entry, recs, hyper, steps_done, g_first):
        self.entry, self.recs, self.ops = entry, recs, recs.ops
        self.lr, self.beta1, self.beta2, self.eps = hyper
        self.steps_done = steps_done
        self.state = self.guard = None
        if entry in ("multi_dev", "guard_idle", "guard_clip"):
            self.state = self.ops.adam_state_new(_dev(), self.lr, self.beta1, self.beta2, self.eps, steps_done)
        if entry.startswith("guard"):
            self.guard = Guard(recs, None if entry == "guard_idle" else CLIP * _norm64(g_first))

    def step(self, t, g=None):
        """``g``: the gradients of this step (the clipping guard's threshold follows their norm)"""
        r, ops = self.recs, self.ops
        n_rec = len(r.lay)
        scale = None
        if self.entry == "multi_dev":
            ops.adam_multi_dev_(r.table, n_rec, r.max_numel, self.state)
        elif self.guard is not None:
            if self.entry == "guard_clip":
                ops.grad_guard_state_set_max_norm(self.guard.state, CLIP * _norm64(g))
            self.guard.reduce()
            ops.adam_multi_dev_guard_(r.table, n_rec, r.max_numel, self.state, self.guard.state)
            st = self.guard.read()
            assert not st["skip"]
            scale = f32(st["scale"])
            assert scale == 1.0 if self.entry == "guard_idle" else abs(scale - CLIP) < 1e-3, (self.entry, scale)
        elif self.entry == "multi_step":
            ops.adam_multi_step_(r.table, n_rec, r.max_numel, self.lr, self.beta1, self.beta2, self.eps, t)
        else:
            for p, g, m, v in zip(*(r.view[q] for q in ac.QUANTITIES)):
                ops.adam_step_(p, g, m, v, self.lr, self.beta1, self.beta2, self.eps, t)
        want_ss, want_isb = ac.tick(t, self.lr, self.beta1, self.beta2)
        if self.state is None:
            return want_ss, want_isb, scale
        rec = read_adam_state(self.state)
        b1, b2, e = ac.kernel_scalars(self.beta1, self.beta2, self.eps)
        assert rec.step == t, (rec.step, t)
        assert (f32(rec.lr), f32(rec.beta1), f32(rec.beta2), f32(rec.eps)) == (f32(self.lr), b1, b2, e)
        ss, isb = f32(rec.step_size), f32(rec.inv_sqrt_bc2)
        # the device's pow may differ from the host's in the last double bit: one float32 unit in the last place at the most
        assert ac.ulps_apart(ss, want_ss) <= 1 and ac.ulps_apart(isb, want_isb) <= 1, (t, ss, want_ss, isb, want_isb)
        return ss, isb, scale


def check_step(recs, before, hyper, ss, isb, scale, what, worst):
    """the device's state after one step against the restatement of that step from ``before`` (host images read before it)"""
    _, beta1, beta2, eps = hyper
    b1, b2, e = ac.kernel_scalars(beta1, beta2, eps)
    after = recs.read()
    x, y = recs.records_of(before), recs.records_of(after)
    g = x["g"] if scale is None else x["g"] * scale                  # float32(g * scale): one float32 multiply by the read-back scale
    assert g.dtype == np.float32
    s = ac.restate(x["p"], g, x["m"], x["v"], b1, b2, e, ss, isb)
    r = ac.ratios(y["p"], y["m"], y["v"], s)
    for q in r:
        worst[q] = max(worst.get(q, 0.0), r[q])
    assert max(r.values()) <= 1.0, (what, r)
    assert np.array_equal(before["g"].view(np.int32), after["g"].view(np.int32)), f"{what}: the gradients were written"
    recs.assert_guards(after, what)
    if beta1 == 0.0:
        assert np.array_equal(y["m"].view(np.int32), g.view(np.int32)), f"{what}: beta1 = 0 and m' is not g bit for bit"
    return after


@pytest.fixture(scope="module")
def layout():
    return ac.main_layout()


# ---- 1. every entry, every path, every step count ---------------------------------------------------------------------------------
@pytest.mark.parametrize("hyper", range(len(ac.HYPERS)))
@pytest.mark.parametrize("entry", ENTRIES)
def test_every_entry_follows_the_restatement(layout, entry, hyper):
    worst = {}
    for steps_done in ac.STEPS_DONE:
        seed = ac.case_seed(hyper, steps_done)
        x = ac.draw(layout, seed)
        recs = Records(layout, x)
        run = Runner(entry, recs, ac.HYPERS[hyper], steps_done, x["g"])
        before = recs.read()
        g = x["g"]
        for k in (1, 2):
            if k == 2:
                g = ac.redraw_g(layout, seed + 1)                    # the gradients are redrawn between the steps
                recs.set_g(g)
                before = dict(before, g=recs.read()["g"])
            ss, isb, scale = run.step(steps_done + k, g)
            before = check_step(recs, before, ac.HYPERS[hyper], ss, isb, scale, (entry, ac.HYPERS[hyper], steps_done, k), worst)
    print(f"{entry}, {ac.HYPERS[hyper]}: worst error / bound  p {worst['p']:.3f}  m {worst['m']:.3f}  v {worst['v']:.3f}")


# ---- 2. the grid stride ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["multi_dev", "multi_step"])
def test_grid_stride_and_one_block_column_give_the_same_bits(entry):
    """more chunks than the launch has block columns (2048): the stride; with max_numel = 4096 one column walks all of them"""
    lay = ac.Layout([([ac.STRIDE_N], ac.same(4))])
    x = ac.draw(lay, 7, mags=[30.0])
    hyper = ac.HYPERS[0]
    got = []
    try:
        for max_numel in (ac.STRIDE_N, 4096):
            recs = Records(lay, x)
            recs.max_numel = max_numel
            before = recs.read()
            run = Runner(entry, recs, hyper, 9, x["g"])
            ss, isb, scale = run.step(10)
            worst = {}
            after = check_step(recs, before, hyper, ss, isb, scale, (entry, "stride", max_numel), worst)
            print(f"{entry}, {ac.STRIDE_N} elements, max_numel {max_numel}: worst error / bound  p {worst['p']:.3f}  m {worst['m']:.3f}  "
                  f"v {worst['v']:.3f}")
            got.append(after)
            del recs, run, before
        for q in "pmv":
            assert np.array_equal(got[0][q].view(np.int32), got[1][q].view(np.int32)), q
    finally:
        got.clear()
        torch.cuda.empty_cache()


# ---- 3. neighbours do not matter ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [4, 1])
def test_a_record_alone_and_as_record_150_of_301_end_bit_identical(off):
    n = 8197
    tiny = [int(k) for k in np.random.default_rng(5).integers(1, 8, 150)]
    crowd = ac.Layout([(tiny, ac.same(4)), ([n], ac.same(off)), (tiny, ac.same(4))])
    alone = ac.Layout([([n], ac.same(off))])
    assert len(crowd) == 301 and crowd.n[150] == n
    xc = ac.draw(crowd, 21)
    sel = slice(int(crowd.first[150]), int(crowd.first[151]))
    xa = {q: xc[q][sel] for q in ac.QUANTITIES}
    hyper = ac.HYPERS[0]
    rc, ra = Records(crowd, xc), Records(alone, xa)
    for q in ac.QUANTITIES:
        assert rc.view[q][150].data_ptr() % 16 == ra.view[q][0].data_ptr() % 16 == (0 if off == 4 else 4)
    bc, ba = rc.read(), ra.read()
    worst = {}
    for recs, before in ((rc, bc), (ra, ba)):
        run = Runner("multi_dev", recs, hyper, 0, None)
        for t in (1, 2):
            ss, isb, scale = run.step(t)
            before = check_step(recs, before, hyper, ss, isb, scale, ("neighbours", len(recs.lay), t), worst)
    for q in "pmv":
        assert torch.equal(rc.view[q][150], ra.view[q][0]), q
    print(f"neighbours, offset {off}: worst error / bound  p {worst['p']:.3f}  m {worst['m']:.3f}  v {worst['v']:.3f}")


# ---- 4. lr rewritten between steps ----------------------------------------------------------------------------------------------
def test_set_lr_between_steps_changes_the_step_size_and_not_t():
    lay = ac.Layout([([8197], ac.same(4)), ([0], ac.same(4)), ([37], ac.same(1))])
    x = ac.draw(lay, 31, mags=[1e-2, 1.0, 1e4])
    lr, beta1, beta2, eps = hyper = ac.HYPERS[1]
    recs = Records(lay, x)
    run = Runner("multi_dev", recs, hyper, 9, None)
    worst = {}
    before = recs.read()
    ss, isb, _ = run.step(10)
    before = check_step(recs, before, hyper, ss, isb, None, "before set_lr", worst)
    new_lr = 0.35 * lr
    recs.ops.adam_state_set_lr(run.state, new_lr)
    rec = read_adam_state(run.state)
    assert rec.step == 10 and f32(rec.lr) == f32(new_lr) and f32(rec.step_size) == ss      # only lr is written; the tick derives
    run.lr = new_lr
    recs.set_g(ac.redraw_g(lay, 32, mags=[1e4, 1.0, 1e-2]))
    before = dict(before, g=recs.read()["g"])
    ss2, isb2, _ = run.step(11)                                      # asserts step == 11 and the tick at the NEW lr
    assert ss2 != ac.tick(11, lr, beta1, beta2)[0]
    check_step(recs, before, (new_lr, beta1, beta2, eps), ss2, isb2, None, "after set_lr", worst)
    print(f"set_lr: worst error / bound  p {worst['p']:.3f}  m {worst['m']:.3f}  v {worst['v']:.3f}")


# ---- 5. optim.Adam ------------------------------------------------------------------------------------------------------------
def test_optimiser_follows_a_host_replay_of_the_restatement():
    """two groups with different lr, one parameter without a gradient on step 2 only (its cohort splits off by step count),
    ExponentialLR between the steps: every parameter and both moments against the restatement applied to exactly the parameters
    that had a gradient"""
    from srgan_amd import optim as hoptim
    rng = np.random.default_rng(41)
    sizes = [(8197,), (5, 7), (4096,), (1,), (3, 4099)]
    params = [torch.nn.Parameter(torch.from_numpy((rng.standard_normal(s) * (1e-3 if i % 2 else 1.0)).astype(np.float32)).to(_dev()))
              for i, s in enumerate(sizes)]
    lazy = params[2]
    betas, eps = (0.5, 0.999), 1e-8
    opt = hoptim.Adam([dict(params=params[:3], lr=1e-3), dict(params=params[3:], lr=2e-4)], betas=betas, eps=eps)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.7)
    b1, b2, e = ac.kernel_scalars(betas[0], betas[1], eps)
    steps = {id(p): 0 for p in params}
    worst = {}

    def host(t):
        return t.detach().cpu().numpy().ravel().copy()
    for s in range(1, 5):
        lrs = [g["lr"] for g in opt.param_groups]
        state_before = {}
        for gi, group in enumerate(opt.param_groups):
            for p in group["params"]:
                has = not (p is lazy and s == 2)
                p.grad = torch.from_numpy((rng.standard_normal(tuple(p.shape)) * 10.0 ** rng.uniform(-4, 4)).astype(np.float32)).to(_dev()) \
                    if has else None
                st = opt.state.get(p, {})
                zeros = np.zeros(p.numel(), dtype=np.float32)
                state_before[id(p)] = (host(p), host(st["exp_avg"]) if st else zeros, host(st["exp_avg_sq"]) if st else zeros, gi, has)
        opt.step()
        torch.cuda.synchronize()
        for p in params:
            p0, m0, v0, gi, has = state_before[id(p)]
            if not has:
                assert np.array_equal(host(p), p0) and opt.state[p]["step"] == steps[id(p)]
                continue
            steps[id(p)] += 1
            st = opt.state[p]
            assert st["step"] == steps[id(p)]
            # the record of the cohort that stepped p: its group, p among its parameters, the count p now stands at
            mine = [co for key, co in opt._cohorts.items() if key[0] == gi and id(p) in key[1:] and co.steps == steps[id(p)]]
            assert len(mine) == 1
            rec = read_adam_state(mine[0].state)
            ss, isb = f32(rec.step_size), f32(rec.inv_sqrt_bc2)
            want_ss, want_isb = ac.tick(steps[id(p)], lrs[gi], betas[0], betas[1])
            assert rec.step == steps[id(p)] and ac.ulps_apart(ss, want_ss) <= 1 and ac.ulps_apart(isb, want_isb) <= 1
            want = ac.restate(p0, host(p.grad), m0, v0, b1, b2, e, ss, isb)
            r = ac.ratios(host(p), host(st["exp_avg"]), host(st["exp_avg_sq"]), want)
            for q in r:
                worst[q] = max(worst.get(q, 0.0), r[q])
            assert max(r.values()) <= 1.0, (s, tuple(p.shape), r)
        sched.step()
        opt.sync_device()
    assert steps[id(lazy)] == 3 and all(steps[id(p)] == 4 for p in params if p is not lazy)
    assert abs(opt.param_groups[0]["lr"] - 1e-3 * 0.7 ** 4) < 1e-12 and abs(opt.param_groups[1]["lr"] - 2e-4 * 0.7 ** 4) < 1e-12
    # the device records stand where the host mirrors do: one cohort per (group, step count)
    for key, co in opt._cohorts.items():
        rec = read_adam_state(co.state)
        assert rec.step == co.steps and f32(rec.lr) == f32(opt.param_groups[key[0]]["lr"])
    assert sorted(read_adam_state(co.state).step for co in opt._cohorts.values()) == [1, 3, 4, 4]
    print(f"optim.Adam, 4 steps: worst error / bound  p {worst['p']:.3f}  m {worst['m']:.3f}  v {worst['v']:.3f}")


# ---- 6. the distance to torch 1.4 -----------------------------------------------------------------------------------------------
def test_distance_to_torch14_stays_inside_c():
    """20 steps from p = m = v = 0 at (0.5, 0.999): the device against the float64 trajectory with torch 1.4's hyper-parameters.
    |dp| <= accumulated rounding + (c + c1) sum |upd|, c = |float32(beta2) - beta2| / (1 - beta2) ~ 1.29e-5, c1 = 0 at beta1 = 0.5
    (tests/adam_common.py).  This pins what the float32 betas of the record cost, so that it cannot grow."""
    lr, beta1, beta2, eps = hyper = ac.HYPERS[0]
    lay = ac.Layout([([8197], ac.same(4)), ([4099], ac.same(1))])
    n_all = int(lay.n.sum())
    rng = np.random.default_rng(51)
    mag = 10.0 ** rng.uniform(-6, 3, n_all)
    grads = [(mag * rng.standard_normal(n_all)).astype(np.float32) for _ in range(20)]
    zeros = np.zeros(n_all, dtype=np.float32)
    recs = Records(lay, dict(p=zeros, g=grads[0], m=zeros, v=zeros))
    run = Runner("multi_dev", recs, hyper, 0, None)
    for t, g in enumerate(grads, 1):
        recs.set_g(g)
        run.step(t)
    after = recs.read()
    recs.assert_guards(after, "20 steps")
    got = recs.records_of(after)["p"].astype(np.float64)
    want, rounding, total = ac.trajectory(grads, lr, beta1, beta2, eps)
    c = ac.deviation_constant(beta2) + ac.deviation_constant(beta1)
    assert abs(c - 1.29e-5) < 5e-8 and ac.deviation_constant(beta1) == 0.0
    bound = rounding + c * total
    share = np.abs(got - want) / bound
    print(f"distance to torch 1.4 after 20 steps: worst |dp| / bound = {share.max():.4f} (c = {c:.4e}; the rounding part is "
          f"{float((rounding / bound).min()):.3f} .. {float((rounding / bound).max()):.3f} of the bound); "
          f"worst |dp| / sum |upd| = {float((np.abs(got - want) / total).max()):.3e}")
    assert (np.abs(got - want) <= bound).all()
