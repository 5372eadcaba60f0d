"""GPU: the geometric-augmentation kernels (csrc/augment_geom.hip through ops.geom_augment; the gate of csrc/ada.hip through
ops.ada_gate) against the restatement of tests/geom_common.py -- forward and backward under max(8 * e32, gamma(L)) per
sample, the permutations, the gated form, bit copies, independence of the batch, the two access paths and the device-side
sanitising bit for bit.  Shapes and tables: geom_common.SHAPES / tables (both sides of every switch-over of the implementation are
in the list)."""
import functools
import itertools

import pytest
import torch

from tests import geom_common as gc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(shape):
    """inputs of a shape, made once and never written"""
    return gc.inputs(shape)


def _run(x, gy, table, flags, gated=False):
    """(y, gx) of the HIP op on device copies of the inputs; checks that neither input was written"""
    from srgan_amd import ops
    xd = x.cuda().requires_grad_(True)
    gd, td = gy.cuda(), table.cuda()
    y = ops.geom_augment(xd, td, flags, gated)
    (gx,) = torch.autograd.grad(y, xd, gd)
    assert y.shape == x.shape and gx.shape == x.shape and (flags == 0 or (ops.is_nhwc_dense(y) and ops.is_nhwc_dense(gx)))
    assert torch.equal(xd.detach().cpu(), x) and torch.equal(gd.cpu(), gy) and torch.equal(td.cpu(), table)
    return y.detach().cpu(), gx.cpu()


def _hold(what, x, gy, table, flags, gated=False):
    y64, g64 = gc.restate_with_grad(x, gy, table, flags, torch.float64, gated)
    y32 = gc.restate(x, table, flags, torch.float32, gated)
    g32 = gc.adjoint_gather(gy, table, flags, torch.float32, gated)
    y, gx = _run(x, gy, table, flags, gated)
    gc.check(f"geom {what} forward", y, y64, y32, gc.L_FWD)
    gc.check(f"geom {what} backward", gx, g64, g32, gc.L_BWD)


@pytest.mark.parametrize("shape", gc.CASES, ids=str)
def test_forward_and_backward_against_the_float64_restatement(shape):
    """random rows under every subset of the four flags, the extreme finite rows, and a gated table with every mask value"""
    x, gy = _case(shape)
    drawn = gc.drawn_table(shape)
    for flags in range(16):
        _hold(f"{shape} drawn flags {flags}", x, gy, drawn, flags)
    for name, table in gc.extreme_tables(shape):
        _hold(f"{shape} {name}", x, gy, table, gc.ALL)
    for name, table in gc.gated_tables(shape):
        _hold(f"{shape} {name} gated", x, gy, table, gc.ALL, gated=True)


@pytest.mark.parametrize("shape", gc.CASES, ids=str)
def test_pure_flip_and_rot90_tables_are_the_cpu_permutation_bit_for_bit(shape):
    x, gy = _case(shape)
    for fx, k, table in gc.pure_tables(shape):
        for flags in (gc.FLIP | gc.ROT90, gc.ALL):
            y, gx = _run(x, gy, table, flags)
            assert torch.equal(y, gc.permutation(x, fx, k)), (shape, fx, k, flags, "forward")
            assert torch.equal(gc.permutation(gx, fx, k), gy), (shape, fx, k, flags, "backward")          # the adjoint is the inverse


@pytest.mark.parametrize("shape", gc.CASES, ids=str)
def test_gated_rows_equal_the_ungated_kernel_with_the_groups_removed(shape):
    """sample n with mask m comes out as the ungated launch with flags & ~m gives it; every group skipped, and flags == 0: bit copies"""
    x, gy = _case(shape)
    for launch in (gc.ALL, gc.FLIP | gc.ROTATE):
        for name, table in gc.gated_tables(shape):
            y, gx = _run(x, gy, table, launch, gated=True)
            masks = table[:, 7].to(torch.int64)
            for m in sorted(set(masks.tolist())):
                rows = masks == m
                yu, gu = _run(x, gy, table, launch & ~m)
                assert torch.equal(y[rows], yu[rows]) and torch.equal(gx[rows], gu[rows]), (shape, name, launch, m)
                if launch & ~m == 0:
                    assert torch.equal(y[rows], x[rows]) and torch.equal(gx[rows], gy[rows]), (shape, name, launch, m)
    y, gx = _run(x, gy, gc.drawn_table(shape), 0)
    assert torch.equal(y, x) and torch.equal(gx, gy)
    # the ungated kernels never read slot 7
    table = gc.gated_tables(shape)[0][1]
    plain = table.clone()
    plain[:, 7] = 0
    ya, ga = _run(x, gy, table, gc.ALL)
    yb, gb = _run(x, gy, plain, gc.ALL)
    assert torch.equal(ya, yb) and torch.equal(ga, gb)


@pytest.mark.parametrize("shape", [s for s in gc.CASES if 2 <= s[0] <= 8], ids=str)
def test_a_sample_depends_neither_on_the_batch_nor_on_its_position(shape):
    from srgan_amd import ops
    x, gy = _case(shape)
    n = shape[0]
    table = gc.extreme_tables(shape)[0][1] if shape[1] * shape[2] > 64 else gc.drawn_table(shape)
    y, gx = _run(x, gy, table, gc.ALL)
    for i in sorted({0, n // 2, n - 1}):                                  # row i alone
        yi, gi = _run(x[i:i + 1], gy[i:i + 1], table[i:i + 1], gc.ALL)
        assert torch.equal(yi[0], y[i]) and torch.equal(gi[0], gx[i]), (shape, i)
    rev = torch.arange(n - 1, -1, -1)                                     # the batch in reverse order
    yr, gr = _run(x[rev], gy[rev], table[rev], gc.ALL)
    assert torch.equal(yr[rev], y) and torch.equal(gr[rev], gx), shape
    # the forward of cat([a, b]) is the cat of the forwards
    cut = n // 2
    both = ops.geom_augment(ops.cat_batch([x[:cut].cuda(), x[cut:].cuda()]), table.cuda(), gc.ALL)
    ya, _ = _run(x[:cut], gy[:cut], table[:cut], gc.ALL)
    yb, _ = _run(x[cut:], gy[cut:], table[cut:], gc.ALL)
    assert torch.equal(both.cpu(), torch.cat([ya, yb])) and torch.equal(both.cpu(), y), shape


def _misaligned(t):
    """a device copy of NCHW tensor t, NHWC-dense, whose storage starts 4 bytes past a 16-byte boundary"""
    n, c, h, w = t.shape
    flat = torch.empty(t.numel() + 4, dtype=torch.float32, device="cuda")
    view = flat[1:1 + t.numel()].view(n, h, w, c)
    view.copy_(t.permute(0, 2, 3, 1))
    out = view.permute(0, 3, 1, 2)
    assert out.data_ptr() % 16 == 4
    return out


@pytest.mark.parametrize("shape", [s for s in gc.CASES if (s[1] * s[2]) % 4 == 0 and s[0] <= 8], ids=str)
def test_the_16_byte_path_equals_the_scalar_path(shape):
    """the same images at an address off 16-byte alignment take the scalar path; both round alike"""
    from srgan_amd import ops
    x, gy = _case(shape)
    tables = [(gc.drawn_table(shape), False), (gc.extreme_tables(shape)[0][1], False), (gc.gated_tables(shape)[0][1], True)]
    for table, gated in tables:
        y, gx = _run(x, gy, table, gc.ALL, gated)
        xm = _misaligned(x).requires_grad_(True)
        ym = ops.geom_augment(xm, table.cuda(), gc.ALL, gated)
        (gm,) = torch.autograd.grad(ym, xm, _misaligned(gy))
        assert torch.equal(ym.detach().cpu(), y) and torch.equal(gm.cpu(), gx), shape


def test_out_of_range_rows_read_as_their_clamped_values(tmp_path):
    """finite rows outside the ranges -- zoom 1e-3 and 1e3, k = 9, fx = 3 -- equal the rows clamped on the host, bit for bit.  The
    stand-alone host sweep of the shared arithmetic (tests/geom_host_sweep.cpp) runs first: the device sees such rows only after it
    has passed."""
    checks, _ = gc.run_host_sweep(tmp_path, sanitize=False)
    assert checks > 10 ** 6
    shape = (4, 16, 12)
    x, gy = _case(shape)
    th = 0.3
    wild = gc.build_table([(3, 9, 1e-3, th), (0, 9, 1e3, -th), (1, 6, 0.4999, 2.0), (2, 5, 2.0001, 0.0)])
    tame = gc.build_table([(1, 1, 0.5, th), (0, 1, 2.0, -th), (1, 2, 0.5, 2.0), (0, 1, 2.0, 0.0)])
    for flags in (gc.ALL, gc.SCALE, gc.ROT90 | gc.FLIP):
        yw, gw = _run(x, gy, wild, flags)
        yt, gt = _run(x, gy, tame, flags)
        assert torch.equal(yw, yt) and torch.equal(gw, gt), flags


def _gate_restated(rows, p):
    """float32 [n, 8]: slots 0..6 copied, slot 7 the mask whose bit g is set iff not (u_g < p)"""
    out = rows[:, :8].clone()
    mask = torch.zeros(rows.shape[0])
    for g in range(4):
        mask += torch.where(rows[:, 8 + g] < p, 0.0, float(1 << g))       # (a NaN compares false: the group is skipped)
    out[:, 7] = mask
    return out


@pytest.mark.parametrize("p", [0.0, 0.3, 1.0])
def test_gate_of_four_groups_against_the_restatement(p):
    import numpy as np
    from srgan_amd import ops
    pf = float(np.float32(p))
    below = max(float(np.nextafter(np.float32(pf), np.float32(-1))), 0.0)          # (uniforms live in [0, 1))
    special = [0.0, pf, below, float(np.nextafter(np.float32(pf), np.float32(2))), float("nan"), 0.999999]
    combos = list(itertools.product(special, repeat=4))                   # every slot meets every special value: 1296 rows
    g = torch.Generator().manual_seed(7)
    rows = torch.zeros(len(combos) + 300, 16)
    rows[:, :8] = torch.randn(rows.shape[0], 8, generator=g)
    rows[:len(combos), 8:12] = torch.tensor(combos, dtype=torch.float32)
    rows[len(combos):, 8:12] = torch.rand(300, 4, generator=g)
    rows[:, 12:] = torch.randn(rows.shape[0], 4, generator=g)             # the unused slots do not matter
    state = ops.ada_state_new(torch.device("cuda"), pf, 0.6, 0.01, 1.0, 4)
    got = ops.ada_gate(rows.cuda(), state, 4).cpu()
    want = _gate_restated(rows, torch.tensor(pf))
    assert torch.equal(got[:, :7], rows[:, :7]) and torch.equal(got, want)
    masks = set(got[:, 7].tolist())
    assert masks == ({15.0} if p == 0.0 else set(float(m) for m in range(16)))
    if p == 1.0:
        assert float(got[len(combos):, 7].max()) == 0.0                   # every uniform in [0, 1) passes
    for n in (1, 255, 257):                                               # the launch's tail
        assert torch.equal(ops.ada_gate(rows[:n].contiguous().cuda(), state, 4).cpu(), want[:n])
