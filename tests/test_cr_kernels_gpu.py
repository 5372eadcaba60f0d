"""GPU: the two kernels of csrc/consistency.hip against the restatements of tests/cr_common.py -- the pair builder for bit-equality on
both access paths, the fused loss against float64 with the bound of tests/small_common.check, the two zero-weight bit rules, the empty
group and the device record."""
import ctypes

import pytest
import torch

from tests import cr_common as cc
from tests import small_common as sc

pytestmark = pytest.mark.gpu
GUARD = 1024                       # floats: 4 KiB on either side of y


def _nhwc_flat(x):
    """[n, 3, h, w] -> the NHWC-dense float32 vector a kernel reads"""
    return x.permute(0, 2, 3, 1).contiguous().flatten()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _run_pairs(xs, table, flags, offset):
    """srgan_cr_pairs_fwd on copies of the sources that start ``offset`` floats into their buffers (0: 16-byte aligned, 1: the scalar
    path), y between two guard regions -> (y [2n * E] on the CPU, the two guards)"""
    from srgan_amd import _lib
    lib = _lib.load()
    n, (_, _, h, w) = sum(x.shape[0] for x in xs), xs[0].shape
    E = 3 * h * w
    srcs = []
    for x in xs:
        buf = torch.empty(x.numel() + 4, dtype=torch.float32, device="cuda")
        buf[offset:offset + x.numel()].view(torch.int32).copy_(_nhwc_flat(x).view(torch.int32).cuda())     # bits, not values
        srcs.append(buf)
    sentinel = torch.tensor(0x7FDEAD77, dtype=torch.int32)
    ybuf = torch.empty(2 * GUARD + 2 * n * E + 4, dtype=torch.int32, device="cuda").fill_(sentinel.item()).view(torch.float32)
    y0 = GUARD + offset
    tab = table.to(torch.float32).cuda().contiguous()
    ptr = lambda t, off: ctypes.c_void_p(t.data_ptr() + 4 * off)
    rc = lib.srgan_cr_pairs_fwd(ptr(srcs[0], offset), xs[0].shape[0], ptr(srcs[1], offset) if len(xs) > 1 else None,
                                xs[1].shape[0] if len(xs) > 1 else 0, ctypes.c_void_p(tab.data_ptr()), ptr(ybuf, y0), 3, h, w, flags,
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.srgan_last_error()
    torch.cuda.synchronize()
    out = ybuf.cpu()
    return out[y0:y0 + 2 * n * E], (out[:y0].view(torch.int32), out[y0 + 2 * n * E:].view(torch.int32)), sentinel


@pytest.mark.parametrize("shape", cc.PAIR_SHAPES, ids=str)
def test_pair_builder_is_bit_equal_to_the_restatement(shape):
    n0, n1, h, w = shape
    n = n0 + n1
    xs = [cc.pair_images(m, h, w, seed=10 * m + h) for m in (n0, n1) if m]
    paths = [0, 1] if (3 * w) % 4 == 0 else [0]          # 3 w % 4 != 0 takes the scalar path at any alignment
    for name, table in cc.pair_tables(n, h, w, seed=h + w).items():
        for flags in ((3,) if name not in ("drawn", "hostile") else (3, 1, 2, 0)):
            want = _bits(_nhwc_flat(cc.pairs_ref(xs, table, flags)))
            for offset in paths:
                got, guards, sentinel = _run_pairs(xs, table, flags, offset)
                assert torch.equal(_bits(got), want), (shape, name, flags, offset)
                assert all(bool((g == sentinel).all()) for g in guards), (shape, name, flags, offset, "a guard region was written")
    # the planted -0.0 / NaN payloads are really there, and really copied
    x = torch.cat(xs, 0)
    assert bool(torch.isnan(x).any()) and bool((_bits(x) == -2147483648).any())


def test_past_the_image_leaves_one_line_and_the_front_rows_are_a_copy():
    x = cc.pair_images(2, 16, 16, seed=3).nan_to_num(0.5, 0.5, 0.5).abs() + 1.0          # no zero anywhere
    table = cc.pair_tables(2, 16, 16, seed=1)["past_the_image"]
    from srgan_amd import ops
    y = ops.cr_pairs([x.cuda()], table.cuda(), 3).cpu()
    assert tuple(y.shape) == (4, 3, 16, 16) and torch.equal(y[:2], x)
    t = y[2:]
    assert not t[:, :, :15, :].any() and not t[:, :, :, 1:].any() and bool((t[:, :, 15, 0] != 0).all())    # ty = 15, tx = -15
    assert torch.equal(t[0, :, 15, 0], x[0, :, 0, 15]) and torch.equal(t[1, :, 15, 0], x[1, :, 0, 0])       # row 1 is flipped


def test_ops_cr_pairs_wrapper():
    from srgan_amd import _lib, ops
    a, b = cc.pair_images(2, 16, 16, seed=1), cc.pair_images(1, 16, 16, seed=2)
    table = cc.pair_tables(3, 16, 16, seed=5)["drawn"]
    y = ops.cr_pairs([a.cuda(), b.cuda()], table.cuda(), 3)
    assert tuple(y.shape) == (6, 3, 16, 16) and ops.is_nhwc_dense(y) and not y.requires_grad
    assert torch.equal(_bits(y), _bits(cc.pairs_ref([a, b], table, 3)))
    with pytest.raises(_lib.SrganHipError, match="requires grad"):
        ops.cr_pairs([a.cuda().requires_grad_(True)], table[:2].cuda(), 3)
    with pytest.raises(_lib.SrganHipError, match="table of shape"):
        ops.cr_pairs([a.cuda()], table.cuda(), 3)
    with pytest.raises(_lib.SrganHipError, match="flags = 4"):
        ops.cr_pairs([a.cuda()], table[:2].cuda(), 4)
    with pytest.raises(_lib.SrganHipError, match="sources"):
        ops.cr_pairs([], table.cuda(), 3)


# ---- the fused loss --------------------------------------------------------------------------------------------------------------
LAM_REAL, LAM_FAKE, EVERY, W_CLASS = 3.0, 0.5, 2, 0.7


def _device_loss(inp, state, rows_first, gk, ck, pairs_first):
    from srgan_amd import ops
    outs = [o.cuda().requires_grad_(True) for o in inp["outs"]]
    logits = [z.cuda().requires_grad_(True) for z in inp["logits"]]
    total, parts = ops.d_losses_cr(outs, logits, inp["label"].cuda(), rows_first, 1.0, 0.0, W_CLASS, state, gk, ck, pairs_first)
    assert not parts.requires_grad and tuple(parts.shape) == (6,)
    total.backward()
    vals = torch.cat([parts.detach(), total.detach().reshape(1)]).cpu()
    return vals, [o.grad.cpu() for o in outs], [z.grad.cpu() for z in logits]


@pytest.mark.parametrize("case", cc.loss_cases(), ids=str)
def test_fused_loss_against_float64(case):
    """every vals entry, d_o and dz within max(8 e32, (L + 16) 2^-23) of float64, L = cr_common.loss_L: the longest sequential fp32 sum
    of one thread of d_losses_cr_kernel"""
    from srgan_amd import ops
    P, per_row, pairs_first, gk, ck, with_class = case
    rows_first = (P + 1) // 2
    inp = cc.loss_inputs(P, per_row, with_class, seed=7 * P + pairs_first)
    state = ops.cr_state_new("cuda", LAM_REAL, LAM_FAKE, EVERY)
    vals, d_o, dz = _device_loss(inp, state, rows_first, gk, ck, pairs_first)
    kw = dict(rows_first=rows_first, t_first=1.0, t_rest=0.0, w_class=W_CLASS, lam_real=LAM_REAL, lam_fake=LAM_FAKE, every=EVERY,
              gan_kind=gk, class_kind=ck, pairs_first=pairs_first)
    v64, g64, z64 = cc.loss_run(inp, torch.float64, **kw)
    v32, g32, z32 = cc.loss_run(inp, torch.float32, **kw)
    L = cc.loss_L(P, per_row)
    names = ("gan_first", "class", "gan_rest", "total", "cr_first", "cr_rest", "total_with_cr")
    for i, name in enumerate(names):
        sc.check("d_losses_cr", f"{case} vals[{name}]", vals[i], v64[i], v32[i], L)
    for s in range(len(per_row)):
        sc.check("d_losses_cr", f"{case} d_o[{s}]", d_o[s], g64[s], g32[s], L)
        if with_class:
            sc.check("d_losses_cr", f"{case} dz[{s}]", dz[s], z64[s], z32[s], L)
            assert not dz[s][rows_first:].any()
    if pairs_first == 0:
        assert float(vals[4]) == 0.0                  # an empty group gives 0, not NaN
    if pairs_first == P:
        assert float(vals[5]) == 0.0
    rec = ops.cr_state_read(state)
    assert rec["updates"] == 1 and rec["cr_real"] == float(vals[4]) and rec["cr_fake"] == float(vals[5])


def _plain_prefix(inp, P, rows_first, gk, ck):
    from srgan_amd import ops
    outs = [o[:P].contiguous().cuda().requires_grad_(True) for o in inp["outs"]]
    logits = [z[:P].contiguous().cuda().requires_grad_(True) for z in inp["logits"]]
    total, parts = ops.d_losses(outs, logits, inp["label"][:P].cuda(), rows_first, 1.0, 0.0, W_CLASS, gk, ck)
    total.backward()
    return torch.cat([parts.detach(), total.detach().reshape(1)]).cpu(), [o.grad.cpu() for o in outs], [z.grad.cpu() for z in logits]


@pytest.mark.parametrize("kinds", cc.KINDS, ids=str)
@pytest.mark.parametrize("P,per_row", [(3, (49, 9)), (257, (1000, 7))], ids=str)
def test_zero_weights_give_the_plain_kernels_bits_and_exact_zeros_behind(P, per_row, kinds):
    """with both weights 0: vals[0..3], d_o[s][:P] and dz[s][:P] are srgan_d_losses_crit's bits on the P-row prefix, and the back rows'
    d_o is exactly 0 although those rows hold NaN and Inf"""
    from srgan_amd import ops
    gk, ck = kinds
    rows_first = (P + 1) // 2
    inp = cc.loss_inputs(P, per_row, True, seed=P)
    for o in inp["outs"]:
        o[P:] = float("nan")
        o[P + P // 2:] = float("inf")
    for z in inp["logits"]:
        z[P:] = float("nan")
    want_v, want_o, want_z = _plain_prefix(inp, P, rows_first, gk, ck)
    state = ops.cr_state_new("cuda", 0.0, 0.0, 3)
    vals, d_o, dz = _device_loss(inp, state, rows_first, gk, ck, P // 2)
    assert torch.equal(_bits(vals[:4]), _bits(want_v)) and torch.equal(_bits(vals[6:]), _bits(want_v[3:]))
    for s in range(len(per_row)):
        assert torch.equal(_bits(d_o[s][:P]), _bits(want_o[s])), s
        assert torch.equal(_bits(dz[s][:P]), _bits(want_z[s])), s
        assert not _bits(d_o[s][P:]).any() and not _bits(dz[s][P:]).any(), s           # +0.0 everywhere
    # one weight 0: its group alone is taken out
    ops.cr_state_set(state, 0.0, 2.0, 3)
    for o in inp["outs"]:
        o[P + P // 2:] = 0.25                                                          # group 2's partners are finite again
    vals, d_o, _ = _device_loss(inp, state, rows_first, gk, ck, P // 2)
    assert bool(torch.isfinite(vals[[0, 1, 2, 3, 5, 6]]).all()) and float(vals[6]) > float(vals[3])
    for s in range(len(per_row)):
        assert torch.equal(_bits(d_o[s][:P // 2]), _bits(want_o[s][:P // 2])) and not _bits(d_o[s][P:P + P // 2]).any()
        assert bool(torch.isfinite(d_o[s][P // 2:P]).all()) and bool((d_o[s][P + P // 2:] != 0).any())
    assert ops.cr_state_read(state)["updates"] == 2


def test_record_after_three_calls_and_the_setters():
    from srgan_amd import ops
    state = ops.cr_state_new("cuda", 1.5, 2.5, 2)
    assert ops.cr_state_read(state) == dict(lambda_real=1.5, lambda_fake=2.5, every=2, cr_real=0.0, cr_fake=0.0, updates=0)
    last = None
    for i in range(3):
        inp = cc.loss_inputs(8, (49, 9), True, seed=40 + i)
        last, _, _ = _device_loss(inp, state, 4, 0, 0, 4)
    rec = ops.cr_state_read(state)
    assert rec["updates"] == 3 and rec["cr_real"] == float(last[4]) > 0 and rec["cr_fake"] == float(last[5]) > 0
    assert abs(float(last[6]) - (float(last[3]) + 2 * (1.5 * float(last[4]) + 2.5 * float(last[5])))) <= 1e-5 * float(last[6])
    ops.cr_state_set(state, 0.5, 0.0, 4)                          # rewrites the weights, keeps the counters
    rec2 = ops.cr_state_read(state)
    assert rec2 == dict(rec, lambda_real=0.5, lambda_fake=0.0, every=4)
    ops.cr_state_set_updates(state, 11)
    assert ops.cr_state_read(state) == dict(rec2, updates=11)
    from srgan_amd import _lib
    with pytest.raises(_lib.SrganHipError, match="cr_state_set"):
        ops.cr_state_set(state, -1.0, 0.0, 1)
    inp = cc.loss_inputs(cc.MAX_PAIRS + 1, (1, 1), False, seed=1)
    with pytest.raises(_lib.SrganHipError, match="pairs = 1025"):
        ops.d_losses_cr([o.cuda() for o in inp["outs"]], [], None, 4, 1.0, 0.0, 1.0, state)
    with pytest.raises(_lib.SrganHipError, match="7 rows"):
        ops.d_losses_cr([torch.zeros(7, 4, device="cuda")], [], None, 2, 1.0, 0.0, 1.0, state)
