"""GPU: the kernels of adaptive discriminator augmentation -- the gated forms of csrc/augment.hip against the ungated kernels on
the reduced flags, bit for bit; the gate and observe kernels of csrc/ada.hip against the restatements of tests/ada_common.py, for
equality.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

from tests import ada_common as adc
from tests import augment_common as ac

pytestmark = pytest.mark.gpu
F32 = np.float32

# the switch-overs of csrc/augment.hip (chunk, item, scalar / 16-byte path, grid stride), one shape on either side
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 8, 8), (5, 36, 38), (2, 35, 39), (2, 2, 683), (2, 36, 57), (2, 3, 683), (2049, 4, 4)]
assert all(s in ac.CASES for s in SHAPES + [(4, 128, 128)])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what


def _ungated(x, gy, table, cut):
    """{flags: (y, gx)} of the ungated kernels for every flag set 0..7 (slot 7 of the table zeroed: they do not read it)"""
    from srgan_amd import ops
    t = table.clone()
    t[:, 7] = 0
    out = {}
    for f in range(8):
        leaf = x.clone().requires_grad_(True)
        y = ops.diffaugment(leaf, t, f, cut)
        (gx,) = torch.autograd.grad(y, leaf, gy)
        out[f] = (y.detach(), gx)
    return out


def _gated_case(shape, name, table, cut, rots):
    from srgan_amd import ops
    n, h, w = shape
    x, gy = (t.cuda() for t in ac.inputs(shape))
    x, gy = ops.to_nhwc(x), ops.to_nhwc(gy)
    ref = _ungated(x, gy, table.cuda(), cut)
    for rot in rots:
        masks = (torch.arange(n) + rot) % 8
        t = table.clone()
        t[:, 7] = masks.to(torch.float32)
        t = t.cuda()
        for flags in range(1, 8):
            what = f"{shape} {name} rot {rot} flags {flags}"
            leaf = x.clone().requires_grad_(True)
            y = ops.diffaugment(leaf, t, flags, cut, gated=True)
            (gx,) = torch.autograd.grad(y, leaf, gy)
            ys = [y.detach()]
            if n > 1:                                  # the two-source forward: the same rows from two tensors
                n0 = (n + 1) // 2
                ys.append(ops.diffaugment_cat([x[:n0].clone(), x[n0:].clone()], t, flags, cut, gated=True))
            else:
                ys.append(ops.diffaugment_cat([x], t, flags, cut, gated=True))
            for m in sorted(set(masks.tolist())):
                idx = (masks == m).nonzero().flatten().cuda()
                eff = flags & ~m
                for k, got in enumerate(ys):
                    _same_bits(got[idx], ref[eff][0][idx], f"{what} mask {m} forward {k}")
                _same_bits(gx[idx], ref[eff][1][idx], f"{what} mask {m} backward")
                if eff == 0:                           # all launched groups skipped: bit copies
                    _same_bits(ys[0][idx], x[idx], f"{what} mask {m} copy of x")
                    _same_bits(gx[idx], gy[idx], f"{what} mask {m} copy of gy")


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_gated_equals_ungated_on_the_reduced_flags(shape):
    """every launch flag set 1..7, per-sample masks cycling through 0..7 (rotated so that a small batch still meets all eight),
    forward, backward and the two-source forward, every table of augment_common.tables"""
    n = shape[0]
    rots = range(0, 8, n) if n < 8 else (0,)
    for name, table, cut in ac.tables(shape):
        _gated_case(shape, name, table, cut, rots)


def test_gated_equals_ungated_at_the_workload_shape():
    shape = (4, 128, 128)
    name, table, cut = ac.tables(shape)[-1]           # the drawn table
    _gated_case(shape, name, table, cut, (0, 4))


def test_slot7_garbage_is_clamped_and_masked():
    from srgan_amd import ops
    shape = (5, 36, 38)
    x, gy = (ops.to_nhwc(t.cuda()) for t in ac.inputs(shape))
    _, table, cut = ac.tables(shape)[0]
    garbage = [8.0, -1.0, float("nan"), 1e30, 5.0]
    clean = [float(adc.slot7_mask(v)) for v in garbage]
    assert clean == [0.0, 7.0, 0.0, 0.0, 5.0]
    res = []
    for slot in (garbage, clean):
        t = table.clone()
        t[:, 7] = torch.tensor(slot)
        leaf = x.clone().requires_grad_(True)
        y = ops.diffaugment(leaf, t.cuda(), ac.ALL, cut, gated=True)
        (gx,) = torch.autograd.grad(y, leaf, gy)
        res.append((y.detach(), gx))
    torch.cuda.synchronize()
    _same_bits(res[0][0], res[1][0], "forward")
    _same_bits(res[0][1], res[1][1], "backward")
    ref = _ungated(x, gy, table.cuda(), cut)
    for i, m in enumerate(int(v) for v in clean):
        _same_bits(res[0][0][i], ref[ac.ALL & ~m][0][i], f"forward sample {i}")
        _same_bits(res[0][1][i], ref[ac.ALL & ~m][1][i], f"backward sample {i}")


@pytest.mark.parametrize("shape", [(3, 5, 7), (5, 36, 38), (2, 35, 39)], ids=str)
def test_ungated_kernels_do_not_read_slot7(shape):
    from srgan_amd import ops
    n = shape[0]
    x, gy = (ops.to_nhwc(t.cuda()) for t in ac.inputs(shape))
    for name, table, cut in ac.tables(shape):
        dirty = table.clone()
        dirty[:, 7] = torch.tensor([7.0, float("nan"), 3.0, -1.0, 1e30][:n])
        ref = _ungated(x, gy, table.cuda(), cut)
        for flags in range(8):
            leaf = x.clone().requires_grad_(True)
            y = ops.diffaugment(leaf, dirty.cuda(), flags, cut)
            (gx,) = torch.autograd.grad(y, leaf, gy)
            _same_bits(y.detach(), ref[flags][0], f"{shape} {name} flags {flags} forward")
            _same_bits(gx, ref[flags][1], f"{shape} {name} flags {flags} backward")
            if not flags & ac.COLOR:                   # copy-or-zero: the float32 restatement is exact
                want = ac.restate(x, table, flags, cut, torch.float32)
                assert torch.equal(y.detach().cpu(), want), f"{shape} {name} flags {flags} restatement"


# ---- the gate -----------------------------------------------------------------------------------------------------------------------
TOP = float(F32(1.0) - F32(2.0 ** -24))               # the largest float32 below 1
PS = [0.0, 2.0 ** -24, 0.5, TOP, 1.0]


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_gate_against_the_restatement(n):
    from srgan_amd import ops
    g = torch.Generator().manual_seed(4000 + n)
    for p in PS:
        rows = torch.randn(n, 16, generator=g)
        rows[:, 8:11] = torch.rand(n, 3, generator=g)
        special = [0.0, TOP, p, float("nan"), 2.0 ** -24, 0.5]
        for i in range(n):                             # every special value in every group within the first rows
            rows[i, 8 + i % 3] = special[(i // 3) % len(special)] if i < 3 * len(special) else rows[i, 8 + i % 3]
        rows[0, 0], rows[0, 1], rows[0, 7] = float("nan"), -0.0, 123.0      # copied bit for bit / overwritten
        state = ops.ada_state_new("cuda", p, 0.6, 0.01, 1.0, 4)
        table = ops.ada_gate(rows.cuda(), state)
        want = adc.gate_rows(rows.numpy(), p)
        got = table.cpu().numpy()
        assert got.shape == (n, 8)
        assert np.array_equal(got[:, :7].view(np.int32), rows.numpy()[:, :7].view(np.int32)), (n, p)
        assert np.array_equal(got[:, 7], want[:, 7]), (n, p, got[:8, 7], want[:8, 7])
        if p == 0.0:
            assert (got[:, 7] == 7.0).all()
        if p == 1.0:
            u = rows.numpy()[:, 8:11]
            odd = (np.isnan(u) | (u >= 1.0)).any(axis=1)          # the NaN, and the value equal to p = 1 (outside [0, 1))
            assert (got[~odd, 7] == 0.0).all() and (got[odd, 7] > 0).all()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("n_groups", [1, 2])
def test_gate_of_fewer_groups_against_the_restatement(n_groups, n):
    """the gate reads the first ``n_groups`` uniforms only: every read slot meets exactly 0, exactly p and the largest float32 below
    1; the slots behind them hold what would set a bit if it were read (uniforms, a NaN), and the bits at and above ``n_groups``
    stay clear"""
    from srgan_amd import ops
    g = torch.Generator().manual_seed(4100 + 10 * n + n_groups)
    for p in (0.0, 0.5, 1.0):
        state = ops.ada_state_new("cuda", p, 0.6, 0.01, 1.0, 4)
        special = [0.0, p, TOP]
        for shift in range(len(special)):                  # (a batch of one row still meets every special value)
            rows = torch.randn(n, 16, generator=g)
            rows[:, 8:12] = torch.rand(n, 4, generator=g)
            for i in range(min(n, len(special) * n_groups)):
                rows[i, 8 + i % n_groups] = special[(i // n_groups + shift) % len(special)]
            rows[0, 8 + n_groups:12] = float("nan")
            rows[0, 1], rows[0, 7] = -0.0, 123.0           # copied bit for bit / overwritten
            got = ops.ada_gate(rows.cuda(), state, n_groups).cpu()
            want = torch.from_numpy(adc.gate_rows(rows.numpy(), p, n_groups))
            assert torch.equal(got, want) and torch.equal(_bits(got), _bits(want)), (n, n_groups, p, shift)
            assert (got[:, 7] < (1 << n_groups)).all()
            if p == 0.0:
                assert (got[:, 7] == (1 << n_groups) - 1).all()
        # a three-group call does not read slot 11: whatever it holds (a NaN, values not below p), bit 3 stays clear
        rows[:, 8:11] = torch.rand(n, 3, generator=g)
        rows[:, 11] = torch.where(torch.arange(n) % 2 == 0, float("nan"), 1.5)
        got = ops.ada_gate(rows.cuda(), state, 3).cpu()
        assert torch.equal(got, torch.from_numpy(adc.gate_rows(rows.numpy(), p, 3))) and (got[:, 7] < 8).all()


# ---- observe ------------------------------------------------------------------------------------------------------------------------
OBSERVE_CASES = [(1, [(1, 1)]), (4, [(16, 16), (8, 8)]), (3, [(7, 5), (4, 3)]), (32, [(1, 1), (1, 1)]), (2, [(250, 280)])]
INTERVAL = 3


def _maps(B, sizes, thr, seed):
    """maps [2B, 1, h, w] around the threshold with every special value in the real rows; the rows beyond B would change every
    count if they were read"""
    g = torch.Generator().manual_seed(seed)
    special = [thr, 0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e-45, -1e-45, 1e-39, thr + 1e-7, thr - 1e-7]
    out = []
    for h, w in sizes:
        m = torch.randn(2 * B, 1, h, w, generator=g) * 0.5 + thr
        flat = m[:B].reshape(-1)
        k = min(len(special), flat.numel())
        pos = torch.randperm(flat.numel(), generator=g)[:k]
        flat[pos] = torch.tensor(special[:k])
        m[:B] = flat.reshape(B, 1, h, w)
        m[B:] = torch.where(torch.arange(B * h * w).reshape(B, 1, h, w) % 3 == 0, thr + 5.0, thr - 7.0)
        out.append(m)
    return out


@pytest.mark.parametrize("thr", [0.5, 0.0])
@pytest.mark.parametrize("case", OBSERVE_CASES, ids=[f"B{b}-" + "+".join(f"{h}x{w}" for h, w in s) for b, s in OBSERVE_CASES])
def test_observe_against_the_restatement(case, thr):
    """the record after 1, interval - 1, interval and interval + 1 calls"""
    from srgan_amd import ops
    B, sizes = case
    p0, target, step, p_max = 0.5, 0.05, 0.125, 0.75
    state = ops.ada_state_new("cuda", p0, target, step, p_max, INTERVAL)
    st = adc.new_state(p0, target, step, p_max, INTERVAL)
    adc.same_record(ops.ada_state_read(state), st)
    for call in range(INTERVAL + 1):
        maps = _maps(B, sizes, thr, 5000 + 10 * B + call)
        ops.ada_observe_([m.cuda() for m in maps], B, thr, state)
        adc.observe(st, [m.numpy() for m in maps], B, thr)
        adc.same_record(ops.ada_state_read(state), st)
        if call == INTERVAL - 2:
            assert st["seen"] == INTERVAL - 1 and st["n_total"] == (INTERVAL - 1) * B * sum(h * w for h, w in sizes)
    assert st["adjustments"] == 1 and st["seen"] == 1


def test_observe_moves_p_both_ways_and_holds_it_at_equality():
    from srgan_amd import ops
    cases = [([1.0, -1.0, float("nan"), 0.0], 0.0, 0.5, 0.0),       # r == target: p stays
             ([1.0, 1.0, 1.0, -1.0], 0.0, 0.625, 0.5),              # up
             ([-1.0, -1.0, 1.0, 0.0], 0.0, 0.375, -0.25),           # down
             ([1.0, 1.0, 1.0, 1.0], 0.0, 0.75, 1.0)]                # up twice: clamped at p_max
    for vals, thr, want_p, want_r in cases:
        state = ops.ada_state_new("cuda", 0.5, 0.0, 0.125, 0.75, 1)
        st = adc.new_state(0.5, 0.0, 0.125, 0.75, 1)
        m = torch.tensor(vals + [9.0] * 4).reshape(2, 1, 2, 2)
        for _ in range(3 if want_p == 0.75 else 1):
            ops.ada_observe_([m.cuda()], 1, thr, state)
            adc.observe(st, [m.numpy()], 1, thr)
        got = ops.ada_state_read(state)
        adc.same_record(got, st)
        assert got["p"] == want_p and got["last_r"] == want_r, (vals, got)


def test_state_set_and_set_counters():
    from srgan_amd import ops
    state = ops.ada_state_new("cuda", 0.25, 0.6, 0.01, 0.8, 4)
    ops.ada_state_set_counters(state, 3, 2 ** 40 + 1, 7, 2 ** 41, 9, -0.5)
    got = ops.ada_state_read(state)
    assert (got["seen"], got["n_pos"], got["n_neg"], got["n_total"], got["adjustments"], got["last_r"]) == (3, 2 ** 40 + 1, 7, 2 ** 41, 9, -0.5)
    assert F32(got["p"]) == F32(0.25) and got["interval"] == 4
    ops.ada_state_set(state, 0.1, 0.5, 0.75, 2)                      # p and the counters stay
    got = ops.ada_state_read(state)
    assert (F32(got["p"]), F32(got["target"]), got["step"], got["p_max"], got["interval"]) == (F32(0.25), F32(0.1), 0.5, 0.75, 2)
    assert (got["seen"], got["n_pos"], got["adjustments"]) == (3, 2 ** 40 + 1, 9)
    ops.ada_state_set(state, 0.1, 0.5, 0.75, 2, 0.5)
    assert ops.ada_state_read(state)["p"] == 0.5
