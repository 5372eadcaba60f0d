"""GPU: the batch-norm and CBB kernels (csrc/norm_batch.hip) against float64 on every path -- every slab plan up to the
single-slab plan of large batches, batches beyond one lane trip of the finalize, every branch of the streaming grid, every
mode (training tracked / untracked / momentum=None, eval), and inputs that are not well-conditioned Gaussians -- called through
the C ABI with the test's own NHWC tensors, so that mean, rstd and the folded coefficients m, a, b are compared too.
References, cases, the restated plans and the error measure live in tests/bn_common.py (pinned without a GPU by
tests/test_bn_refs_cpu.py).  Every comparison is bounded by max(8 * e32, gamma(L)); the counter is compared as an integer.

Every tensor a call reads or writes lies between two guard regions of pattern bytes, the workspace and the exchange buffer
have exactly the bytes the size functions return, and every guard has to be intact after every call.

The synced entries: one process plays every rank in turn -- each rank's partial pass writes its chunk of one exchange buffer,
which then holds what the all-gather would deliver -- and every rank's results are held to torch.equal with the one-process
entries on the whole batch, and to float64.
SRGAN_TEST_LOG=1 prints e32, gamma, err and err / bound of every comparison."""
import os

import pytest
import torch

from tests import bn_common as bn

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 4096, 0xA5
KERNEL = "norm_batch"


@pytest.fixture(scope="module")
def ops():
    from srgan_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(scope="module")
def lib():
    from srgan_amd import _lib
    return _lib


class Arena:
    """The device memory of one scenario: every buffer has ``guard`` pattern bytes in front of it and behind it."""

    def __init__(self):
        self.bufs = []

    def raw(self, nbytes, what, guard=GUARD):
        guard = -(-guard // GUARD) * GUARD                     # keeps the payload 4 KiB-aligned within the allocation
        buf = torch.full((guard + nbytes + guard,), PATTERN, dtype=torch.uint8, device="cuda")
        self.bufs.append((buf, guard, nbytes, what))
        return buf[guard:guard + nbytes]

    def out(self, shape, what, guard=GUARD, dtype=torch.float32):
        """An output: NaN-filled (the counter: its start value comes from ``put``)."""
        numel = int(torch.Size(shape).numel())
        t = self.raw(numel * 4, what, guard).view(dtype).view(shape)
        t.fill_(float("nan"))
        return t

    def put(self, t, what, guard=GUARD):
        """An input (or a buffer the call updates): the CPU tensor's values, dense."""
        if t is None:
            return None
        t = t.detach().contiguous()
        d = self.raw(t.numel() * t.element_size(), what, guard).view(t.dtype).view(t.shape)
        d.copy_(t)
        return d

    def intact(self, when):
        for buf, guard, nbytes, what in self.bufs:
            ok = bool((buf[:guard] == PATTERN).all()) and bool((buf[guard + nbytes:] == PATTERN).all())
            assert ok, f"{when}: bytes written outside the {nbytes} bytes of {what}"


def nhwc(t):
    """NCHW CPU tensor -> the dense NHWC array the kernels read."""
    return t.detach().float().permute(0, 2, 3, 1).contiguous()


def nchw(t):
    """A dense NHWC device array -> the logical NCHW tensor on the CPU."""
    return t.permute(0, 3, 1, 2).cpu()


def _flags(v):
    cbb, mode, flag, act = v
    return dict(training=int(mode != "eval"), cumulative=int(mode == "cumulative"), momentum=bn.MOMENTUM if mode == "tracked" else 0.0,
                tracked=mode in ("tracked", "cumulative"), buffers=mode != "untracked")


def _params(inp, v, rows=slice(None)):
    """(p0, p1, res) of the variant on the CPU: BN weight / bias (None without affine), CBB scale / shift rows and the residual."""
    cbb, mode, flag, act = v
    if cbb:
        return inp["scale"][rows], inp["shift"][rows], nhwc(inp["res"][rows]) if flag else None
    return (inp["weight"], inp["bias"], None) if flag else (None, None, None)


def run_one(ops, lib, shape, inp, v, gy, what):
    """CALLS forwards and (gy given) one backward of the one-process entries on guarded memory -> the outputs on the device."""
    cbb, mode, flag, act = v
    n, c, h, w = shape
    hw, fl = h * w, _flags(v)
    L, P, st = lib.load(), ops._ptr, ops._stream()
    A = Arena()
    x = A.put(nhwc(inp["x"]), "x")
    p0, p1, res = (A.put(t, name) for t, name in zip(_params(inp, v), ("weight / scale", "bias / shift", "res")))
    y = A.out((n, h, w, c), "y")
    mean, rstd = A.out((c,), "mean"), A.out((c,), "rstd")
    m, a, b = A.out((n, c), "m"), A.out((n, c), "a"), A.out((n, c), "b")
    rm, rv = (A.put(inp["rm"], "running_mean"), A.put(inp["rv"], "running_var")) if fl["buffers"] else (None, None)
    nbt = A.put(torch.tensor([bn.NBT0], dtype=torch.int64), "num_batches_tracked")
    ws_bytes = L.srgan_batchnorm_workspace(n, hw, c)
    ws = A.raw(ws_bytes, "workspace")
    out = dict(bufs=[])
    for call in range(bn.CALLS):
        tail = (P(y), P(mean), P(rstd), P(m), P(a), P(b), P(rm), P(rv), P(nbt), n, hw, c, fl["training"], fl["momentum"], fl["cumulative"],
                bn.EPS, act, bn.SLOPE, P(ws), ws_bytes, st)
        if cbb:
            lib.check(L.srgan_cbbnorm_fwd(P(x), P(p0), P(p1), P(res), *tail), "cbbnorm_fwd")
        else:
            lib.check(L.srgan_batchnorm_fwd(P(x), P(p0), P(p1), *tail), "batchnorm_fwd")
        torch.cuda.synchronize()
        A.intact(f"{what} forward {call}")
        out["bufs"].append((rm.clone() if fl["buffers"] else None, rv.clone() if fl["buffers"] else None, int(nbt)))
        if call == 0:
            first = [t.clone() for t in (y, mean, rstd, m, a, b)]
    assert all(torch.equal(t, u) for t, u in zip(first, (y, mean, rstd, m, a, b))), f"{what}: the same call gave other bits"
    out.update(y=y, mean=mean, rstd=rstd, m=m, a=a, b=b)
    if gy is not None:
        dy = A.put(nhwc(gy), "dy")
        dx = A.out((n, h, w, c), "dx")
        d0, d1 = (A.out((n, c) if cbb else (c,), name) for name in ("dscale / dweight", "dshift / dbias"))
        ws2 = A.raw(ws_bytes, "backward workspace")
        tail = (P(mean), P(rstd), P(m), P(a), P(b), P(dx), P(d0), P(d1), n, hw, c, fl["training"], act, bn.SLOPE, P(ws2), ws_bytes, st)
        if cbb:
            lib.check(L.srgan_cbbnorm_bwd(P(x), P(dy), P(p0), *tail), "cbbnorm_bwd")
        else:
            lib.check(L.srgan_batchnorm_bwd(P(x), P(dy), P(p0), *tail), "batchnorm_bwd")
        torch.cuda.synchronize()
        A.intact(f"{what} backward")
        out.update(dx=dx, d0=d0, d1=d1)
    return out


def _cpu(name, t):
    return nchw(t) if name in ("y", "dx") else t.cpu()


def _hold(check, what, name, got, r64, r32, L, inp=None):
    """One tensor against the yardstick.  A gradient whose float64 reference is identically zero has no scale to be relative to
    (CBB with one pixel per image: x is its own mean, dx = alpha g + k with k = -alpha g): the kernel's value is then held to
    gamma(L) of the terms that cancel, max |a| max |dy|."""
    if name == "dx" and float(r64.abs().max()) == 0.0 and float(r32.abs().max()) == 0.0:
        err, bound = float(got.abs().max()), bn.gamma(L) * float(inp[0].abs().max()) * float(inp[1].abs().max())
        if os.environ.get("SRGAN_TEST_LOG"):
            print(f"small {KERNEL} | {what} {name} | zero reference: max |got| {err:.3e} err/bound {err / bound:.3f}")
        assert err <= bound, f"{what} {name}: {err:.3e} > gamma = {bn.gamma(L):.3e} of max |a| max |dy|"
        return
    check(KERNEL, f"{what} {name}", got, r64, r32, L)


def hold_one(ops, lib, shape, inp, v, backward=True, per_channel=False, tag=""):
    """The one-process entries on one variant against the yardstick; returns the device outputs, the upstream gradient and
    the yardstick."""
    f64, f32, gy = bn.yardstick(inp, v, shape, backward)
    what = "x".join(map(str, shape)) + " " + tag + bn.variant_id(v)
    got = run_one(ops, lib, shape, inp, v, gy, what)
    check = bn.check_channels if per_channel else bn.check
    L_f, L_b = bn.path_L(shape), bn.path_L(shape, backward=True)
    fl = _flags(v)
    for name in ("y", "mean", "rstd", "m", "a", "b") + (("dx", "d0", "d1") if backward else ()):
        _hold(check, what, name, _cpu(name, got[name]), f64[name], f32[name], L_b if name in ("dx", "d0", "d1") else L_f,
              (f64["a"], gy) if backward else None)
    for call, (rm, rv, count) in enumerate(got["bufs"]):
        if fl["tracked"]:
            assert count == f64["bufs"][call][2] == bn.NBT0 + call + 1, f"{what}: num_batches_tracked after call {call}"
            check(KERNEL, f"{what} running_mean after call {call}", rm.cpu(), f64["bufs"][call][0], f32["bufs"][call][0], L_f)
            check(KERNEL, f"{what} running_var after call {call}", rv.cpu(), f64["bufs"][call][1], f32["bufs"][call][1], L_f)
        else:                                   # eval mode, or no buffers: nothing moves
            assert count == bn.NBT0, f"{what}: num_batches_tracked moved"
            if fl["buffers"]:
                assert torch.equal(rm.cpu(), inp["rm"]) and torch.equal(rv.cpu(), inp["rv"]), f"{what}: running buffers moved"
    return got, gy, f64, f32


CASE_IDS = [c["name"] for c in bn.CASES]


@pytest.mark.parametrize("act", bn.ACTS)
@pytest.mark.parametrize("case", bn.CASES, ids=CASE_IDS)
def test_one_process_entries(ops, lib, case, act):
    """srgan_batchnorm_fwd / _bwd and srgan_cbbnorm_fwd / _bwd on every variant of the case's grid."""
    inp = bn.case_inputs(case["shape"])
    for v in bn.variants(case, act):
        hold_one(ops, lib, case["shape"], inp, v)


@pytest.mark.parametrize("shape,kind", bn.HOSTILE_CASES, ids=bn.nc.hostile_id)
def test_hostile_inputs(ops, lib, shape, kind):
    """Offset means, a constant channel, a 100-sigma outlier at the first or the last pixel, an offset first row, channels seven
    decades apart (measured per channel): within the same bound as everything else.  bn_stats_partial shifts its sums by the
    slab's first pixel, and under the single-slab plan one such sum runs over the whole image: the 100-sigma first pixel at
    (1024, 4, 48, 48) is the case that would show a cancellation there (DESIGN.md section 7 has the measured figures)."""
    inp = bn.case_inputs(shape, bn.HOSTILE_INPUTS[kind](shape))
    for v, backward in bn.hostile_variants(shape):
        hold_one(ops, lib, shape, inp, v, backward, per_channel=kind == bn.CHANNEL_SCALES, tag=kind + " ")


# ---- the synced entries ----------------------------------------------------------------------------------------------------------------
def run_ranks(ops, lib, case, inp, v, gy, what):
    """Every rank of the case in turn, on guarded memory -> per rank the outputs on the device."""
    cbb, mode, flag, act = v
    ng, nl, c, h, w = case
    hw, fl, world = h * w, _flags(v), ng // nl
    L, P, st = lib.load(), ops._ptr, ops._stream()
    A = Arena()
    wide = ng * c * 4                       # a write displaced by any image of the global batch stays inside the guard
    ranks = []
    for r in range(world):
        rows = slice(r * nl, (r + 1) * nl)
        k = dict(x=A.put(nhwc(inp["x"][rows]), "x"), dy=A.put(nhwc(gy[rows]), "dy"))
        k["p0"], k["p1"], k["res"] = (A.put(t, name) for t, name in zip(_params(inp, v, rows), ("weight / scale", "bias / shift", "res")))
        k["y"], k["dx"] = A.out((nl, h, w, c), "y"), A.out((nl, h, w, c), "dx")
        k["mean"], k["rstd"] = A.out((c,), "mean"), A.out((c,), "rstd")
        k["m"], k["a"], k["b"] = (A.out((nl, c), name, wide) for name in ("m", "a", "b"))
        k["d0"], k["d1"] = (A.out((nl, c) if cbb else (c,), name, wide) for name in ("dscale / dweight", "dshift / dbias"))
        k["rm"], k["rv"] = (A.put(inp["rm"], "running_mean"), A.put(inp["rv"], "running_var")) if fl["buffers"] else (None, None)
        k["nbt"] = A.put(torch.tensor([bn.NBT0], dtype=torch.int64), "num_batches_tracked")
        k["ws_bytes"] = L.srgan_batchnorm_sync_workspace(nl, c)
        k["ws"] = A.raw(k["ws_bytes"], "rank workspace", wide)
        ranks.append(k)
    geo = lambda r: (ng, r * nl, nl, hw, c)                                             # noqa: E731
    fwd_bytes = L.srgan_batchnorm_sync_exchange_bytes(ng, nl, hw, c, 0)
    bwd_bytes = L.srgan_batchnorm_sync_exchange_bytes(ng, nl, hw, c, int(cbb))
    assert fwd_bytes and bwd_bytes
    # the guard is as large as the buffer: an access displaced by up to the whole buffer stays inside the allocation
    xf, xb = A.raw(fwd_bytes, "forward exchange buffer", fwd_bytes), A.raw(bwd_bytes, "backward exchange buffer", bwd_bytes)
    for r, k in enumerate(ranks):
        lib.check(L.srgan_batchnorm_sync_fwd_partial(P(k["x"]), P(xf), fwd_bytes, *geo(r), st), "batchnorm_sync_fwd_partial")
    for r, k in enumerate(ranks):
        tail = (P(k["y"]), P(k["mean"]), P(k["rstd"]), P(k["m"]), P(k["a"]), P(k["b"]), P(k["rm"]), P(k["rv"]), P(k["nbt"]), P(xf),
                fwd_bytes, *geo(r), fl["momentum"], fl["cumulative"], bn.EPS, act, bn.SLOPE, st)
        if cbb:
            lib.check(L.srgan_cbbnorm_sync_fwd_apply(P(k["x"]), P(k["p0"]), P(k["p1"]), P(k["res"]), *tail), "cbbnorm_sync_fwd_apply")
        else:
            lib.check(L.srgan_batchnorm_sync_fwd_apply(P(k["x"]), P(k["p0"]), P(k["p1"]), *tail), "batchnorm_sync_fwd_apply")
    torch.cuda.synchronize()
    A.intact(f"{what} synced forward")
    for r, k in enumerate(ranks):
        lib.check(L.srgan_batchnorm_sync_bwd_partial(P(k["x"]), P(k["dy"]), P(k["p0"]) if cbb else None, P(k["rstd"]), P(k["m"]), P(k["a"]),
                                                     P(k["b"]), P(xb), bwd_bytes, *geo(r), act, bn.SLOPE, st), "batchnorm_sync_bwd_partial")
    for r, k in enumerate(ranks):
        tail = (P(k["mean"]), P(k["rstd"]), P(k["m"]), P(k["a"]), P(k["b"]), P(xb), bwd_bytes, P(k["dx"]), P(k["d0"]), P(k["d1"]), *geo(r),
                act, bn.SLOPE, P(k["ws"]), k["ws_bytes"], st)
        if cbb:
            lib.check(L.srgan_cbbnorm_sync_bwd_apply(P(k["x"]), P(k["dy"]), *tail), "cbbnorm_sync_bwd_apply")
        else:
            lib.check(L.srgan_batchnorm_sync_bwd_apply(P(k["x"]), P(k["dy"]), P(k["p0"]), *tail), "batchnorm_sync_bwd_apply")
    torch.cuda.synchronize()
    A.intact(f"{what} synced backward")
    return ranks


@pytest.mark.parametrize("case", bn.SYNC_CASES, ids=bn.sync_id)
def test_synced_entries(ops, lib, case):
    """Every rank bit-identical to the one-process entries on the concatenated batch (which are held to float64 here as well);
    BN's dweight / dbias are sums over a rank's own images: their sum over the ranks is held to float64."""
    ng, nl, c, h, w = case
    shape = bn.sync_shape(case)
    inp = bn.case_inputs(shape)
    L_b = bn.path_L(shape, backward=True)
    for v in bn.SYNC_VARIANTS:
        cbb = v[0]
        what = bn.sync_id(case) + " " + bn.variant_id(v)
        one, gy, f64, f32 = hold_one(ops, lib, shape, inp, v)
        rm1, rv1, count1 = one["bufs"][0]
        ranks = run_ranks(ops, lib, case, inp, v, gy, what)
        for r, k in enumerate(ranks):
            rows = slice(r * nl, (r + 1) * nl)
            for name in ("y", "dx", "m", "a", "b") + (("d0", "d1") if cbb else ()):
                assert torch.equal(k[name], one[name][rows]), f"{what}: rank {r} {name} differs from one process"
            for name in ("mean", "rstd"):
                assert torch.equal(k[name], one[name]), f"{what}: rank {r} {name} differs from one process"
            assert int(k["nbt"]) == count1, f"{what}: rank {r} num_batches_tracked"
            if rm1 is not None:
                assert torch.equal(k["rm"], rm1) and torch.equal(k["rv"], rv1), f"{what}: rank {r} running buffers differ from one process"
        if not cbb:
            for name in ("d0", "d1"):
                total = torch.stack([k[name].double() for k in ranks]).sum(dim=0)
                bn.check(KERNEL, f"{what} {name} summed over the ranks", total.cpu(), f64[name], f32[name], L_b)
