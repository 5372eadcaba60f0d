"""GPU: the convolution kernels no case of tests/test_ops_gpu.py launches -- the 8-wave 256-row implicit-GEMM tiles of the
benchmarked step, the generic 128x128 tile, the row-aligned weight-gradient tiles, the narrow-output instantiations, the masked
epilogues of the transposed Winograd kernels and the 128 -> 256 patch kernels with 16-bit tensors -- against the float64
convolution of tests/conv_common.py: y, dx, dw and db, through ops.conv2d with and without ops.pack_cache() (the io kernels
through ops.conv2d_s2_io).  Which kernel each case launches is pinned on the CPU by tests/test_conv_refs_cpu.py.

In the bf16 compute mode a direction multiplies bf16-rounded operands exactly when its gather is the vector one (the BF16
instantiations of igemm_kernel / wgrad_kernel exist with VEC only): I % 32 == 0 for the forward and the weight gradient,
O % 32 == 0 for the input gradient; a scalar-gather direction is the exact fp32 product in both modes.  The reference follows
that rule (test_conv_refs_cpu.py checks it against the launched instantiations); bounds as in conv_common.check."""
import contextlib
import functools
import os
import re

import pytest
import torch

from tests import conv_common as cc

pytestmark = pytest.mark.gpu

R = cc.bf16_round


@pytest.fixture(scope="module")
def ops():
    from srgan_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(scope="module", autouse=True)
def figures():
    """With SRGAN_TEST_LOG set: the worst error / bound per kernel family at the end of the module."""
    del cc.FIGURES[:]
    yield
    if os.environ.get("SRGAN_TEST_LOG"):
        worst = {}
        for kernel, what, e32, err, bound in cc.FIGURES:
            fam = re.sub(r"<.*", "", kernel.split(" ")[0])
            if fam not in worst or err / bound > worst[fam][0]:
                worst[fam] = (err / bound, kernel, what, e32, err, bound)
        for fam, (ratio, kernel, what, e32, err, bound) in sorted(worst.items()):
            print(f"conv worst {fam} | {kernel} {what} | e32 {e32:.3e} err {err:.3e} bound {bound:.3e} err/bound {ratio:.3f}")


@functools.lru_cache(maxsize=2)       # the packed and the unpacked run of a (case, mode) follow each other and share it
def yardstick(case, mode):
    """inputs, float64 reference and float32-CPU reference (y, dx, dw, db) of a case in a compute mode."""
    torch.set_num_threads(16)
    x, w, b, gy = cc.inputs(case)
    if mode == "fp32":
        return (x, w, b, gy), cc.reference(case, x, w, b, gy, torch.float64), cc.reference(case, x, w, b, gy, torch.float32)
    i, o = case[1], case[4]
    fwd16, dgrad16, wgrad16 = i % 32 == 0, o % 32 == 0, i % 32 == 0
    out = []
    for dtype in (torch.float64, torch.float32):
        y = cc.reference(case, R(x) if fwd16 else x, R(w) if fwd16 else w, b, gy, dtype)[0]
        dx = cc.reference(case, x, R(w) if dgrad16 else w, b, R(gy) if dgrad16 else gy, dtype)[1]
        dw = cc.reference(case, R(x) if wgrad16 else x, w, b, R(gy) if wgrad16 else gy, dtype)[2]
        db = cc.reference(case, x, w, b, gy, dtype)[3]
        out.append((y, dx, dw, db))
    return (x, w, b, gy), out[0], out[1]


_RUNS = [(case, mode, packed) for case, want in cc.KERNEL_CASES for mode in ("fp32", "bf16") if mode in want for packed in (False, True)]


@pytest.mark.parametrize("case,mode,packed", _RUNS, ids=[f"{cc.tag(c)}-{m}-{'packed' if p else 'unpacked'}" for c, m, p in _RUNS])
def test_conv_kernel(ops, case, mode, packed):
    want = dict(cc.KERNEL_CASES)[case][mode]
    label = "+".join(f"{k}" for k in want.values()) + f" {cc.tag(case)} {mode}{' packed' if packed else ''}"
    (x, w, b, gy), ref64, ref32 = yardstick(case, mode)
    s, p, reflect = case[6], case[7], case[8]
    xd, wd = x.detach().cuda().requires_grad_(True), w.detach().cuda().requires_grad_(True)
    bd = b.detach().cuda().requires_grad_(True) if b is not None else None
    ops.invalidate_packed()
    ops.set_compute_dtype(mode)
    try:
        with (ops.pack_cache() if packed else contextlib.nullcontext()):
            y = ops.conv2d(xd, wd, bd, s, p, ops.PAD_REFLECT if reflect else ops.PAD_ZERO)
            y.backward(gy.cuda())
        torch.cuda.synchronize()
    finally:
        ops.set_compute_dtype("fp32")
        ops.invalidate_packed()
    got = (y, xd.grad, wd.grad, bd.grad if b is not None else None)
    for what, g, r64, r32 in zip(("y", "dx", "dw", "db"), got, ref64, ref32):
        if r64 is not None:
            cc.check(label, what, g, r64, r32)


@pytest.mark.parametrize("case,kernel", cc.MASK_CASES, ids=[cc.tag(c) for c, _ in cc.MASK_CASES])
def test_masked_input_gradient(ops, case, kernel):
    """conv(4x4, s2) whose input is the LeakyReLU(0.2) output of its producer: ops.conv2d(..., in_slope=0.2) inside a pack-cache
    scope multiplies the input gradient by 1 or 0.2 after the sign of the input, in the epilogue of the transposed Winograd
    kernel (srgan_conv2d_dgrad_packed_mask; the dispatch thresholds are off so that these small maps take it)."""
    torch.set_num_threads(16)
    x, w, b, gy = cc.inputs(case)
    mask = torch.where(x > 0, torch.ones_like(x), torch.full_like(x, 0.2))
    refs = []
    for dtype in (torch.float64, torch.float32):
        y, dx, dw, _ = cc.reference(case, x, w, b, gy, dtype)
        refs.append((y, dx * mask.to(dtype), dw))
    xd, wd = x.detach().cuda().requires_grad_(True), w.detach().cuda().requires_grad_(True)
    os.environ["SRGAN_WINOGRAD_THRESHOLD_SCALE"] = "0"
    ops.invalidate_packed()
    try:
        with ops.pack_cache():
            y = ops.conv2d(xd, wd, None, case[6], case[7], ops.PAD_ZERO, ops.ACT_NONE, 0.0, 0.2, False)
            y.backward(gy.cuda())
        torch.cuda.synchronize()
    finally:
        os.environ.pop("SRGAN_WINOGRAD_THRESHOLD_SCALE", None)
        ops.invalidate_packed()
    for what, g, r64, r32 in zip(("y", "dx", "dw"), (y, xd.grad, wd.grad), *refs):
        cc.check(f"{kernel} {cc.tag(case)}", what, g, r64, r32)


@pytest.mark.parametrize("kind", [0, 1], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("case,kernel", cc.HALO16_IO_CASES, ids=[cc.tag(c) for c, _ in cc.HALO16_IO_CASES])
def test_halo16_bf16_source_fp32_result(ops, case, kernel, kind):
    """srgan_halo16_conv with a bf16 source, an fp32 result and no skip tensor -- instantiated, reachable through the C ABI and
    used by no Function of srgan_amd.ops, so the entry is called here: forward (kind 0) and input gradient (kind 1) of the
    residual-trunk layers against the float64 convolution of the bf16-rounded operands."""
    import ctypes
    from srgan_amd import _lib
    torch.set_num_threads(16)
    n, c, h, w_ = case[:4]
    x, w, _, gy = cc.inputs(case)
    ref64 = cc.reference(case, R(x), R(w), None, R(gy), torch.float64)
    ref32 = cc.reference(case, R(x), R(w), None, R(gy), torch.float32)
    src = (x if kind == 0 else gy).detach().cuda().permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)      # [N][H][W][C]
    dst = torch.empty((n, h, w_, c), dtype=torch.float32, device="cuda")
    ops.set_compute_dtype("bf16")
    ops.invalidate_packed()
    try:
        with ops.pack_cache():
            wd = w.detach().cuda()
            desc = ops._conv_desc(n, h, w_, c, h, w_, c, 3, 3, 1, 1, ops.PAD_ZERO, wd)
            lib = _lib.load()
            assert lib.srgan_halo16_applicable(ctypes.byref(desc))
            hit, _ = ops._packed(desc, wd, kind, ops.ACT_NONE)
            _lib.check(lib.srgan_halo16_conv(ctypes.byref(desc), kind, ops._ptr(src), 1, ops._ptr(hit.buf), None, ops._ptr(dst), 0,
                                             ops._stream()), "halo16_conv")
        torch.cuda.synchronize()
    finally:
        ops.set_compute_dtype("fp32")
        ops.invalidate_packed()
    what = "y" if kind == 0 else "dx"
    cc.check(f"{kernel} {cc.tag(case)} kind{kind}", what, dst.permute(0, 3, 1, 2), ref64[kind], ref32[kind])


@pytest.mark.parametrize("in16", [False, True])
@pytest.mark.parametrize("out16", [False, True])
def test_stride2_io_kernels(ops, in16, out16):
    """The 128 -> 256 down convolution with fp32 / bf16 tensors on either side (ops.conv2d_s2_io, bf16 mode): forward, input
    gradient and weight gradient against the float64 convolution of the bf16-rounded operands; a bf16 result is the reference
    rounded once more (half a bf16 ulp of its maximum)."""
    torch.set_num_threads(16)
    case = cc.S2_IO_CASE
    n, ci, h, w_, co = case[:5]
    x, w, _, gy = cc.inputs(case)
    ref64 = cc.reference(case, R(x), R(w), None, R(gy), torch.float64)
    ref32 = cc.reference(case, R(x), R(w), None, R(gy), torch.float32)
    b = ",".join("true" if v else "false" for v in (in16, out16))
    label = f"halo16s_kernel<128,256,{b}>+halo16t_kernel<256,128,{','.join(reversed(b.split(',')))}>+halo16s2_wgrad_kernel<32,{b}>"
    ops.set_compute_dtype("bf16")
    ops.invalidate_packed()
    try:
        with ops.pack_cache():
            wd = w.detach().cuda().requires_grad_(True)
            assert ops.s2_io_applicable(n, ci, h, w_, co, wd, False)
            xd = x.detach().cuda().contiguous(memory_format=torch.channels_last)
            xd = (xd.to(torch.bfloat16) if in16 else xd).requires_grad_(True)
            y = ops.conv2d_s2_io(xd, wd, out16)
            assert y.dtype == (torch.bfloat16 if out16 else torch.float32)
            y.backward(gy.cuda().contiguous(memory_format=torch.channels_last).to(y.dtype))
            assert xd.grad.dtype == xd.dtype
        torch.cuda.synchronize()
    finally:
        ops.set_compute_dtype("fp32")
        ops.invalidate_packed()
    cc.check(label, "y", y.float(), ref64[0], ref32[0], stored_bf16=out16)
    cc.check(label, "dx", xd.grad.float(), ref64[1], ref32[1], stored_bf16=in16)
    cc.check(label, "dw", wd.grad, ref64[2], ref32[2])
