"""GPU: the DiffAugment kernels (csrc/augment.hip through ops.diffaugment / ops.diffaugment_cat) against the restatement of
tests/augment_common.py -- colour on under max(8 * e32, gamma(L)) per sample, colour off bit for bit, independence of the batch
size and of a sample's position, repeatability.  Shapes and tables: augment_common.SHAPES / tables (both sides of every
switch-over point of the implementation are in the list)."""
import functools

import pytest
import torch

from tests import augment_common as ac

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(shape):
    """inputs and tables of a shape, made once and never written"""
    x, gy = ac.inputs(shape)
    return x, gy, ac.tables(shape)


def _run(x, gy, table, flags, cut):
    """(y, gx) of the HIP op on device copies of the inputs; checks that neither input was written"""
    from srgan_amd import ops
    xd = x.cuda().requires_grad_(True)
    gd, td = gy.cuda(), table.cuda()
    y = ops.diffaugment(xd, td, flags, cut)
    (gx,) = torch.autograd.grad(y, xd, gd)
    assert ops.is_nhwc_dense(y) and ops.is_nhwc_dense(gx) and y.shape == x.shape and gx.shape == x.shape
    assert torch.equal(xd.detach().cpu(), x) and torch.equal(gd.cpu(), gy) and torch.equal(td.cpu(), table)
    return y.detach().cpu(), gx.cpu()


@pytest.mark.parametrize("shape", ac.CASES, ids=str)
def test_colour_on_against_the_float64_restatement(shape):
    x, gy, tabs = _case(shape)
    L = ac.seq_len(*shape[1:])
    for name, table, cut in tabs:
        for flags in ((1, 3, 5, 7) if ac.is_small(shape) else (1, 7)):
            y64, g64 = ac.restate_with_grad(x, gy, table, flags, cut, torch.float64)
            y32, g32 = ac.restate_with_grad(x, gy, table, flags, cut, torch.float32)
            y, gx = _run(x, gy, table, flags, cut)
            ac.check(f"{shape} {name} flags {flags} forward", y, y64, y32, L)
            ac.check(f"{shape} {name} flags {flags} backward", gx, g64, g32, L)


@pytest.mark.parametrize("shape", ac.CASES, ids=str)
def test_colour_off_is_bit_equal_to_the_restatement(shape):
    x, gy, tabs = _case(shape)
    for name, table, cut in tabs:
        for flags in (0, 2, 4, 6):
            y32, g32 = ac.restate_with_grad(x, gy, table, flags, cut, torch.float32)
            y, gx = _run(x, gy, table, flags, cut)
            assert torch.equal(y, y32), (shape, name, flags, "forward")
            assert torch.equal(gx, g32), (shape, name, flags, "backward")
            if flags == 0:
                assert torch.equal(y, x) and torch.equal(gx, gy)


@pytest.mark.parametrize("shape", [s for s in ac.CASES if s[0] >= 2], ids=str)
def test_a_sample_depends_neither_on_the_batch_nor_on_its_position(shape):
    from srgan_amd import ops
    x, gy, tabs = _case(shape)
    n = shape[0]
    cutn = n // 2
    for name, table, cut in tabs[-2:]:                       # the whole-image extremes and the drawn rows
        for flags in (7, 6):
            y, gx = _run(x, gy, table, flags, cut)
            # the two-source form against the two halves run on their own
            a, b = x[:cutn].cuda(), x[cutn:].cuda()
            ycat = ops.diffaugment_cat([a, b], table.cuda(), flags, cut)
            assert ops.is_nhwc_dense(ycat) and not ycat.requires_grad
            ya, ga = _run(x[:cutn], gy[:cutn], table[:cutn], flags, cut)
            yb, gb = _run(x[cutn:], gy[cutn:], table[cutn:], flags, cut)
            assert torch.equal(ycat.cpu(), torch.cat([ya, yb])), (shape, name, flags)
            assert torch.equal(y, torch.cat([ya, yb])) and torch.equal(gx, torch.cat([ga, gb])), (shape, name, flags)
            one = ops.diffaugment_cat([x.cuda()], table.cuda(), flags, cut)
            assert torch.equal(one.cpu(), y)
            # row i alone (first, last, one in the middle)
            for i in sorted({0, n // 2, n - 1}):
                yi, gi = _run(x[i:i + 1], gy[i:i + 1], table[i:i + 1], flags, cut)
                assert torch.equal(yi[0], y[i]) and torch.equal(gi[0], gx[i]), (shape, name, flags, i)


@pytest.mark.parametrize("shape", [(3, 5, 7), (4, 128, 128), (2049, 4, 4)], ids=str)
def test_two_runs_are_bit_equal(shape):
    x, gy, tabs = _case(shape)
    name, table, cut = tabs[-1]
    for flags in (7, 1):
        first, second = _run(x, gy, table, flags, cut), _run(x, gy, table, flags, cut)
        assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]), (shape, flags)


def test_layouts_and_refusals():
    from srgan_amd import _lib, ops
    shape = (3, 5, 7)
    x, gy, tabs = _case(shape)
    name, table, cut = tabs[-1]
    y, gx = _run(x, gy, table, 7, cut)
    # an NCHW-contiguous input and gradient: repacked, same values
    xd = x.cuda().contiguous().requires_grad_(True)
    y2 = ops.diffaugment(xd, table.cuda(), 7, cut)
    (g2,) = torch.autograd.grad(y2, xd, gy.cuda().contiguous())
    assert torch.equal(y2.detach().cpu(), y) and torch.equal(g2.cpu(), gx)
    # an image pointer 4 bytes off a 16-byte boundary on a shape that otherwise takes the 16-byte path: the scalar path, same bits
    xs, gs, ts = _case((2, 8, 8))
    _, tab8, cut8 = ts[-1]
    want = _run(xs, gs, tab8, 7, cut8)[0]
    flat = torch.zeros(xs.numel() + 1, device="cuda")
    off = flat[1:].view(2, 8, 8, 3).permute(0, 3, 1, 2)
    off.copy_(xs.cuda())
    assert off.data_ptr() % 16 == 4
    assert torch.equal(ops.diffaugment(off, tab8.cuda(), 7, cut8).cpu(), want)
    with pytest.raises(_lib.SrganHipError, match="three channels"):
        ops.diffaugment(torch.zeros(2, 4, 8, 8, device="cuda"), tab8.cuda(), 7, cut8)
    with pytest.raises(_lib.SrganHipError, match="table of shape"):
        ops.diffaugment(xs.cuda(), tab8.cuda()[:1], 7, cut8)
    with pytest.raises(_lib.SrganHipError, match="flags"):
        ops.diffaugment(xs.cuda(), tab8.cuda(), 8, cut8)
    with pytest.raises(_lib.SrganHipError, match="no CPU fallback"):
        ops.diffaugment(xs, tab8, 7, cut8)
    with pytest.raises(_lib.SrganHipError, match="requires grad"):
        ops.diffaugment_cat([xs.cuda().requires_grad_(True)], tab8.cuda(), 7, cut8)
    with pytest.raises(_lib.SrganHipError, match="one or two"):
        ops.diffaugment_cat([xs.cuda()] * 3, tab8.cuda().repeat(3, 1), 7, cut8)


def test_the_object_draws_uploads_and_applies():
    from srgan_amd.augment import DiffAugment
    x, gy = ac.inputs((4, 16, 12))
    a, b = DiffAugment(seed=3), DiffAugment(seed=3)
    table = b.draw(4, 16, 12)
    xd = x.cuda().requires_grad_(True)
    y = a(xd)
    (gx,) = torch.autograd.grad(y, xd, gy.cuda())
    want = _run(x, gy, table, 7, b.cut(16, 12))
    assert torch.equal(y.detach().cpu(), want[0]) and torch.equal(gx.cpu(), want[1])
    ident = DiffAugment("")
    assert ident(xd) is xd
