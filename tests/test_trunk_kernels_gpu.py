"""GPU: the fused norm + F(4x4,3x3) entries of the residual trunk against float64 -- srgan_instnorm_fwd_v + srgan_conv2d_fwd_from_v
(in_fwd_slab_v16_kernel, wino43_kernel on a ready V image), srgan_instnorm_bwd_vz (in_bwd_slab_vz_kernel) + srgan_conv2d_dgrad_from_v
(wino43_kernel<RES>) + srgan_conv2d_wgrad_vz (wino43_wgrad_kernel on a ready Z image), called through ctypes with the test's own
tensors.  References, cases, the restated image sizes and L live in tests/trunk_common.py (pinned without a GPU by
tests/test_trunk_refs_cpu.py).  Convolution results are bounded by conv_common.check (max(BOUND[what], 8 * e32)), statistics and
dscale / dshift by norm_common.check (max(8 * e32, gamma(L))); the upstream gradient is zero inside the activation's kink window,
so nothing here tolerates a flipped mask.  Every V and Z image carries 4 KiB of pattern behind the byte count the ABI states and
the pattern has to survive the call.  SRGAN_TEST_LOG=1 prints e32, err and err / bound of every comparison."""
import contextlib
import ctypes
import os

import pytest
import torch

from tests import conv_common as cc
from tests import norm_common as nc
from tests import trunk_common as tc

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 4096, 0xA5
FWD_V, FROM_V, BWD_VZ = "srgan_instnorm_fwd_v", "srgan_conv2d_fwd_from_v", "srgan_instnorm_bwd_vz"
DGRAD_V, WGRAD_VZ = "srgan_conv2d_dgrad_from_v", "srgan_conv2d_wgrad_vz"


@pytest.fixture(scope="module")
def ops():
    from srgan_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(scope="module")
def lib():
    from srgan_amd import _lib
    return _lib


@contextlib.contextmanager
def forced(ops):
    """A packed-weight scope with the dispatch thresholds off (read per call), so that the small batches take F(4x4,3x3)."""
    os.environ["SRGAN_WINOGRAD_THRESHOLD_SCALE"] = "0"
    ops.invalidate_packed()
    try:
        with ops.pack_cache():
            yield
            torch.cuda.synchronize()
    finally:
        os.environ.pop("SRGAN_WINOGRAD_THRESHOLD_SCALE", None)
        ops.invalidate_packed()


def nhwc(t):
    """The tensor on the device, NHWC-dense with its logical NCHW shape."""
    return t.detach().float().permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)


def dev(t):
    return None if t is None else t.detach().float().contiguous().cuda()


def guarded(nbytes):
    """An image of `nbytes` bytes with GUARD bytes behind it, all pattern."""
    return torch.full((nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")


def assert_guard(buf, nbytes, what):
    assert buf.numel() == nbytes + GUARD and bool((buf[nbytes:] == PATTERN).all()), f"{what}: bytes written beyond the stated {nbytes}"


def conv_desc(ops, lib, nio, wd):
    N, I, O = nio
    return ops._conv_desc(N, tc.HW, tc.HW, I, tc.HW, tc.HW, O, 3, 3, 1, 1, ops.PAD_ZERO, wd)


def run_forward(ops, lib, nio, inp, act, epilogue_act=tc.ACT_NONE):
    """srgan_instnorm_fwd_v into a guarded V image, srgan_conv2d_fwd_from_v on it -> (y, mean, rstd)."""
    N, I, O = nio
    L, P, st = lib.load(), ops._ptr, ops._stream()
    with forced(ops):
        xd, wd = nhwc(inp["x"]), dev(inp["w"])
        scd, shd, bd = dev(inp["scale"]), dev(inp["shift"]), dev(inp["bias"])
        desc = conv_desc(ops, lib, nio, wd)
        d = ctypes.byref(desc)
        assert L.srgan_instnorm_conv_v_applicable(d)
        hit, scratch = ops._packed(desc, wd, 0, epilogue_act)
        assert scratch == L.srgan_conv2d_packed_scratch(d, 0) == tc.packed_scratch(N, I, O, 0)
        v = guarded(scratch)
        mean = torch.full((N * I,), float("nan"), device="cuda")
        rstd = torch.full_like(mean, float("nan"))
        lib.check(L.srgan_instnorm_fwd_v(d, P(xd), P(scd), P(shd), P(mean), P(rstd), P(v), scratch, tc.EPS, act, tc.SLOPE, st), FWD_V)
        y = ops.nhwc_empty(N, O, tc.HW, tc.HW, xd.device)
        lib.check(L.srgan_conv2d_fwd_from_v(d, P(v), P(hit.buf), P(bd), P(y), epilogue_act, tc.SLOPE, st), FROM_V)
    assert_guard(v, scratch, FWD_V + " V image")
    return y, mean, rstd


def hold_forward(ops, lib, nio, act, affine, epilogue_act=tc.ACT_NONE, with_bias=False, kind="default"):
    inp, r64, r32 = tc.forward_yardstick(nio, act, affine, epilogue_act, with_bias, kind)
    y, mean, rstd = run_forward(ops, lib, nio, inp, act, epilogue_act)
    what = f"{tc.run_id(nio)} {kind} act={act} affine={int(affine)} epilogue={epilogue_act} bias={int(with_bias)}"
    cc.check(f"{FWD_V}+{FROM_V} {what}", "y", y, r64[0], r32[0])
    nc.check(FWD_V, f"{what} mean", mean, r64[1], r32[1], tc.L)
    nc.check(FWD_V, f"{what} rstd", rstd, r64[2], r32[2], tc.L)


def run_backward(ops, lib, nio, inp, act):
    """srgan_instnorm_bwd_vz into guarded V and Z images; srgan_conv2d_dgrad_from_v without and with the skip gradient;
    srgan_conv2d_wgrad_vz with the V image the forward kept (srgan_conv2d_fwd_packed with a kept workspace, or
    srgan_instnorm_fwd_v when the case normalises the convolution's input) -> dict(dx, dx_res, dw, dscale, dshift)."""
    N, I, O = nio
    L, P, st = lib.load(), ops._ptr, ops._stream()
    with forced(ops):
        yd, gd, wd = nhwc(inp["y"]), nhwc(inp["gup"]), dev(inp["w"])
        scd, shd, resd = dev(inp["scale"]), dev(inp["shift"]), nhwc(inp["res"])
        mean, rstd = dev(inp["mean"]), dev(inp["rstd"])
        desc = conv_desc(ops, lib, nio, wd)
        d = ctypes.byref(desc)
        assert L.srgan_instnorm_bwd_vz_applicable(d)
        vb, zb = L.srgan_conv2d_packed_scratch(d, 1), L.srgan_instnorm_bwd_vz_z_bytes(d)
        assert vb == tc.packed_scratch(N, I, O, 1) and zb == tc.z_bytes(N, O)
        vimg, zimg = guarded(vb), guarded(zb)
        dsc = torch.full((N, O), float("nan"), device="cuda")
        dsh = torch.full_like(dsc, float("nan"))
        lib.check(L.srgan_instnorm_bwd_vz(d, P(yd), P(gd), P(scd), P(shd), P(mean), P(rstd), P(dsc), P(dsh), P(vimg), vb, P(zimg), zb,
                                          act, tc.SLOPE, st), BWD_VZ)
        hit1, _ = ops._packed(desc, wd, 1, ops.ACT_NONE)
        out = dict(dscale=dsc, dshift=dsh)
        for name, r in (("dx", None), ("dx_res", resd)):
            out[name] = ops.nhwc_empty(N, I, tc.HW, tc.HW, yd.device)
            lib.check(L.srgan_conv2d_dgrad_from_v(d, P(vimg), P(hit1.buf), P(r), P(out[name]), st), DGRAD_V)
        # the forward's V image, kept by the caller as _ResBlockFn.forward keeps v0 / v1
        hit0, sc0 = ops._packed(desc, wd, 0, ops.ACT_NONE)
        assert sc0 == L.srgan_conv2d_wgrad_v_bytes(d) == tc.wgrad_v_bytes(N, I, O) != 0
        v0 = guarded(sc0)
        if "x0" in inp:
            x0, s0, h0 = nhwc(inp["x0"]), dev(inp["scale0"]), dev(inp["shift0"])
            m0 = torch.empty(N * I, device="cuda")
            r0 = torch.empty_like(m0)
            lib.check(L.srgan_instnorm_fwd_v(d, P(x0), P(s0), P(h0), P(m0), P(r0), P(v0), sc0, tc.EPS, inp["act0"], tc.SLOPE, st), FWD_V)
        else:
            xc, y1 = nhwc(inp["x_conv"]), ops.nhwc_empty(N, O, tc.HW, tc.HW, yd.device)
            lib.check(L.srgan_conv2d_fwd_packed(d, P(xc), P(hit0.buf), None, P(y1), ops.ACT_NONE, 0.0, P(v0), sc0, st),
                      "srgan_conv2d_fwd_packed")
        # the weight-gradient workspace as ops._wgrad_to_sink sets it up (outside a gradient sink: a fresh dw, no accumulation)
        out["dw"], _ = ops._wgrad_to_sink(desc, (wd,), lambda dd, dw, db, ws, nb: lib.check(
            L.srgan_conv2d_wgrad_vz(ctypes.byref(dd), P(v0), P(zimg), P(dw), P(ws), nb, st), WGRAD_VZ))
    assert_guard(vimg, vb, BWD_VZ + " V image")
    assert_guard(zimg, zb, BWD_VZ + " Z image")
    assert_guard(v0, sc0, "forward V image")
    return out


def hold_backward(ops, lib, nio, act, affine, kind="default", v_from_norm=None):
    inp, r64, r32 = tc.backward_yardstick(nio, act, affine, kind, v_from_norm)
    got = run_backward(ops, lib, nio, inp, act)
    what = f"{tc.run_id(nio)} {kind} act={act} affine={int(affine)}" + (" V from the norm" if v_from_norm else "")
    # composition 2: the input gradient, without and with the skip path's gradient in the epilogue
    cc.check(f"{BWD_VZ}+{DGRAD_V} {what}", "dx", got["dx"], r64["dx"], r32["dx"])
    cc.check(f"{BWD_VZ}+{DGRAD_V} {what} +res", "dx", got["dx_res"], r64["dx_res"], r32["dx_res"])
    nc.check(BWD_VZ, f"{what} dscale", got["dscale"], r64["dscale"], r32["dscale"], tc.L)
    nc.check(BWD_VZ, f"{what} dshift", got["dshift"], r64["dshift"], r32["dshift"], tc.L)
    # composition 3: the weight gradient from the kept V image and the Z image
    cc.check(f"{BWD_VZ}+{WGRAD_VZ} {what}", "dw", got["dw"], r64["dw"], r32["dw"])


@pytest.mark.parametrize("nio,act,affine", tc.runs(tc.FWD_CASES), ids=tc.run_id)
def test_forward(ops, lib, nio, act, affine):
    """Composition 1: y = conv3x3(act(z)), mean and rstd."""
    hold_forward(ops, lib, nio, act, affine)


@pytest.mark.parametrize("nio,act,affine,epilogue_act", tc.EPILOGUE_CASES, ids=tc.run_id)
def test_forward_bias_and_activation_epilogue(ops, lib, nio, act, affine, epilogue_act):
    """The bias / act arguments of srgan_conv2d_fwd_from_v: y = act2(conv3x3(act(z)) + bias)."""
    hold_forward(ops, lib, nio, act, affine, epilogue_act, True)


@pytest.mark.parametrize("nio,act,affine", tc.runs(tc.BWD_CASES), ids=tc.run_id)
def test_backward(ops, lib, nio, act, affine):
    """Compositions 2 and 3 from one call of srgan_instnorm_bwd_vz, as the residual block uses it: dx (with and without the skip
    gradient), dscale, dshift (written without affine parameters too) and dw."""
    hold_backward(ops, lib, nio, act, affine)


def test_weight_gradient_with_the_v_image_of_the_norm(ops, lib):
    """The v1 of the residual block: srgan_instnorm_fwd_v writes the V image that srgan_conv2d_wgrad_vz multiplies with Z."""
    nio, act0, affine0 = tc.V_FROM_NORM_CASE
    hold_backward(ops, lib, nio, tc.ACT_RELU, True, v_from_norm=(act0, affine0))


@pytest.mark.parametrize("shape,kind", tc.HOSTILE_CASES, ids=nc.hostile_id)
def test_hostile_inputs(ops, lib, shape, kind):
    """Offset means, a constant channel, 100-sigma outliers, an offset row and a variance beside eps through the fused
    statistics: the forward with each activation, the backward without one (tests/test_norm_kernels_gpu.py's treatment)."""
    fwd, bwd = tc.HOSTILE_SHAPES[shape]
    for act in tc.HOSTILE_FWD_ACTS:
        hold_forward(ops, lib, fwd, act, True, kind=kind)
    hold_backward(ops, lib, bwd, tc.ACT_NONE, True, kind=kind)


def test_an_image_one_byte_short_is_refused_before_any_launch(ops, lib):
    """An argument check: each norm entry returns non-zero for a V or Z byte count one below the stated size, srgan_last_error
    names the size function, and neither the images nor the statistics are touched (the buffers themselves have their full size)."""
    nio = N, I, O = 2, 64, 128
    L, P, st = lib.load(), ops._ptr, ops._stream()
    with forced(ops):
        wd = dev(tc.weight(I, O))
        d = ctypes.byref(conv_desc(ops, lib, nio, wd))
        v0, v1, zb = L.srgan_conv2d_packed_scratch(d, 0), L.srgan_conv2d_packed_scratch(d, 1), L.srgan_instnorm_bwd_vz_z_bytes(d)
        x, y, g = (nhwc(tc.norm_input((N, c, tc.HW, tc.HW))) for c in (I, O, O))
        stats = [torch.full((N * O,), 7.0, device="cuda") for _ in range(4)]
        images = [guarded(n) for n in (v0, v1, zb)]
        assert L.srgan_instnorm_fwd_v(d, P(x), None, None, P(stats[0]), P(stats[1]), P(images[0]), v0 - 1, tc.EPS, 1, 0.0, st) != 0
        assert b"srgan_conv2d_packed_scratch" in L.srgan_last_error()
        for vb, zz, name in ((v1 - 1, zb, b"srgan_conv2d_packed_scratch(d, 1)"), (v1, zb - 1, b"srgan_instnorm_bwd_vz_z_bytes")):
            assert L.srgan_instnorm_bwd_vz(d, P(y), P(g), None, None, P(stats[0]), P(stats[1]), P(stats[2]), P(stats[3]), P(images[1]), vb,
                                           P(images[2]), zz, 1, 0.0, st) != 0
            assert name in L.srgan_last_error()
    assert all(bool((s == 7.0).all()) for s in stats) and all(bool((b == PATTERN).all()) for b in images)


def test_a_refused_weight_gradient_leaves_no_open_timer_bracket(ops, lib):
    """srgan_halo16_wgrad refuses bf16 x with fp32 dy (halo16_wgrad_kernel has no such instantiation) before its launch-timer bracket
    opens: the profiling session of the refused call holds no slot of that kernel and every kernel id collects; the accepted call
    (bf16 x, bf16 dy) books exactly one launch with a finite, positive time.  The smallest layer halo16_applicable accepts."""
    N, C, H, W = 1, 64, 4, 32
    L, P, st = lib.load(), ops._ptr, ops._stream()
    names = [L.srgan_prof_kernel_name(k).decode() for k in range(L.srgan_prof_num_kernels())]

    def collect():
        L.srgan_prof_enable(0)
        torch.cuda.synchronize()
        out = {}
        for kid, name in enumerate(names):
            ms, n, fl = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double()
            assert L.srgan_prof_collect(kid, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)) == 0, (name, L.srgan_last_error())
            out[name] = (n.value, ms.value)
        return out

    assert L.srgan_set_compute_mode(1) == 0
    try:
        dw = torch.zeros(C, C, 3, 3, device="cuda")
        desc = ops._conv_desc(N, H, W, C, H, W, C, 3, 3, 1, 1, ops.PAD_ZERO, dw)
        d = ctypes.byref(desc)
        nbytes = L.srgan_conv2d_workspace(d)
        assert nbytes > 0
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        x16 = torch.randn(N, H, W, C, device="cuda").to(torch.bfloat16)
        dy32 = torch.randn(N, H, W, C, device="cuda")
        dy16 = dy32.to(torch.bfloat16)
        L.srgan_prof_enable(1)
        assert L.srgan_halo16_wgrad(d, P(x16), 1, P(dy32), 0, P(dw), P(ws), nbytes, st) != 0
        assert b"not instantiated" in L.srgan_last_error()
        got = collect()
        assert got["halo16_wgrad_kernel"][0] == 0, got
        L.srgan_prof_enable(1)
        lib.check(L.srgan_halo16_wgrad(d, P(x16), 1, P(dy16), 1, P(dw), P(ws), nbytes, st), "srgan_halo16_wgrad")
        got = collect()
        n, ms = got["halo16_wgrad_kernel"]
        assert n == 1 and ms > 0.0 and ms != float("inf") and ms == ms, got
    finally:
        L.srgan_prof_enable(0)
        assert L.srgan_set_compute_mode(0) == 0
