"""CPU: the parts of the gradient guard (srgan_grad_guard_* / srgan_adam_multi_dev_guard of the C ABI, optim.Adam's and the
trainer's entry points) that need no GPU -- argument errors before any launch, the reduce table's layout, and the float64
restatement's bound against a simulation of the kernel's documented summation order."""
import ctypes
import struct

import numpy as np
import pytest
import torch

from tests.guard_common import D, NORM_FACTOR, U, ref_norm


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from srgan_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.srgan_last_error().decode()


def test_bad_arguments_return_minus_one_without_a_gpu(lib):
    buf = (ctypes.c_char * 4096)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    inf = float("inf")
    assert lib.srgan_grad_guard_state_bytes() == 32
    for bad in (0.0, -1.0, float("nan"), -inf):
        assert lib.srgan_grad_guard_state_init(b, bad, None) == -1 and "grad_guard_state_init" in _err(lib), bad
        assert lib.srgan_grad_guard_state_set_max_norm(b, bad, None) == -1 and "grad_guard_state_set_max_norm" in _err(lib), bad
    assert lib.srgan_grad_guard_state_init(None, 1.0, None) == -1 and "grad_guard_state_init" in _err(lib)
    assert lib.srgan_grad_guard_state_set_max_norm(None, inf, None) == -1 and "grad_guard_state_set_max_norm" in _err(lib)
    assert lib.srgan_grad_guard_workspace(0) == 0 and "grad_guard_workspace" in _err(lib)
    assert lib.srgan_grad_guard_workspace(-3) == 0 and "grad_guard_workspace" in _err(lib)
    assert lib.srgan_grad_guard_workspace(5) == 20
    reduce = lib.srgan_grad_guard_reduce
    assert reduce(None, 1, 1, b, 4, b, None) == -1 and "grad_guard_reduce" in _err(lib)                  # NULL table
    assert reduce(b, 1, 1, None, 4, b, None) == -1 and "grad_guard_reduce" in _err(lib)                  # NULL workspace
    assert reduce(b, 1, 1, b, 4, None, None) == -1 and "grad_guard_reduce" in _err(lib)                  # NULL record
    assert reduce(b, 0, 1, b, 4, b, None) == -1 and "grad_guard_reduce" in _err(lib)                     # zero records
    assert reduce(b, 1, 0, b, 4, b, None) == -1 and "grad_guard_reduce" in _err(lib)                     # zero chunks
    assert reduce(b, 3, 2, b, 64, b, None) == -1 and "grad_guard_reduce" in _err(lib)                    # fewer chunks than records
    assert reduce(b, 1, 2, b, 7, b, None) == -1 and "workspace" in _err(lib)                             # workspace too small
    guard = lib.srgan_adam_multi_dev_guard
    assert guard(None, 1, 1, b, b, None) == -1 and "adam_multi_dev_guard" in _err(lib)
    assert guard(b, 1, 1, None, b, None) == -1 and "adam_multi_dev_guard" in _err(lib)
    assert guard(b, 1, 1, b, None, None) == -1 and "adam_multi_dev_guard" in _err(lib)
    assert guard(b, 0, 1, b, b, None) == -1 and "adam_multi_dev_guard" in _err(lib)
    assert guard(b, 1, 0, b, b, None) == -1 and "adam_multi_dev_guard" in _err(lib)
    assert all(c == b"\x00" for c in buf)                                                              # nothing was touched


def test_host_side_refusals():
    """what the Python layer refuses before it reaches the library"""
    from srgan_amd import optim
    from srgan_amd.trainer import SRGAN_training
    opt = optim.Adam([torch.nn.Parameter(torch.zeros(3))], lr=1e-3)
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="max_norm"):
            opt.enable_grad_guard(bad)
    with pytest.raises(RuntimeError, match="GPU"):                     # CPU parameters: no fallback
        opt.enable_grad_guard()
    for call in (opt.grad_guard_stats, lambda: opt.set_max_norm(1.0)):
        with pytest.raises(RuntimeError, match="guard is off"):
            call()
    assert opt.grad_guard_fingerprint() is None and opt.graph_keepalive() == []
    assert "guard" not in str(opt.state_dict().keys())
    opt.disable_grad_guard()                                           # off already: nothing to do
    for name in ("enable_grad_guard", "set_grad_clip", "disable_grad_guard", "grad_guard_stats"):
        assert callable(getattr(SRGAN_training, name))


def test_table_layout(lib):
    """three 64-bit words per record {g, numel, chunk0}; chunk0 is the prefix sum of ceil(numel / 4096); empty tensors stay out"""
    from srgan_amd import ops

    class Fake:
        is_cuda, dtype = True, torch.float32

        def __init__(self, ptr, n):
            self._p, self._n = ptr, n

        def is_contiguous(self):
            return True

        def numel(self):
            return self._n

        def data_ptr(self):
            return self._p

    seen = {}
    orig = ops.upload_small
    ops.upload_small = lambda blob, device, out=None: seen.setdefault("blob", bytes(blob))
    try:
        _, n, total = ops.grad_guard_table([Fake(16, 1), Fake(64, 4096), Fake(80, 0), Fake(256, 4097), Fake(1024, 8193)], "cpu")
    finally:
        ops.upload_small = orig
    assert ops.GRAD_GUARD_CHUNK == 4096 and (n, total) == (4, 1 + 1 + 2 + 3)
    assert struct.unpack("12q", seen["blob"]) == (16, 1, 0, 64, 4096, 1, 256, 4097, 2, 1024, 8193, 4)


def _chunk_partial(x):
    """one chunk as the kernel documents it: element e -> thread (e / 4) % 256, slot (e / 1024) * 4 + e % 4; 16 serial
    x * x + acc with ONE rounding each; xor butterfly over 64 lanes; (w0 + w1) + (w2 + w3)"""
    x = np.concatenate([x.astype(np.float32), np.zeros(4096 - x.size, np.float32)]).reshape(4, 256, 4)
    acc = np.zeros(256, np.float64)
    for j in range(4):
        for e in range(4):
            v = x[j, :, e].astype(np.float64)
            acc = (v * v + acc).astype(np.float32).astype(np.float64)     # the product of two floats is exact in double: one rounding
    acc = acc.astype(np.float32).reshape(4, 64)
    o = 32
    while o:
        acc = acc + acc[:, np.arange(64) ^ o]                             # float32 adds
        o >>= 1
    w = acc[:, 0]
    return np.float32(np.float32(w[0] + w[1]) + np.float32(w[2] + w[3]))


def test_documented_summation_order_stays_inside_the_bound():
    """the depth D = 24 the bound is built from: a CPU simulation of the chunk sum over random tensor sets"""
    assert D == 16 + 6 + 2
    rng = np.random.default_rng(0)
    worst = 0.0
    for trial in range(20):
        sizes = rng.choice([1, 3, 4095, 4096, 4097, 8197, 40000], size=4)
        tensors = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 3)).astype(np.float32) for n in sizes]
        S = 0.0
        for t in tensors:
            for c0 in range(0, t.size, 4096):
                S += float(_chunk_partial(t[c0:c0 + 4096]))
        norm, ref = np.float32(np.sqrt(S)), ref_norm(tensors)
        worst = max(worst, abs(float(norm) - ref) / (U * ref))
        assert abs(float(norm) - ref) <= NORM_FACTOR * U * ref, (trial, float(norm), ref)
    print(f"simulated chunk sums: worst error = {worst:.3f} * 2^-24 * ref (bound factor {NORM_FACTOR})")


# ---- launch descriptors (no GPU: tests/hip_shim/launch_shim.c logs them) --------------------------------------------------------
def test_launch_descriptors_within_aql_limits(lib, tmp_path):
    """the three kernels for an optimiser of 300 tensors / 2 * 10^7 elements, and for a single element"""
    import os
    import subprocess
    import sys
    from srgan_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    import isa_tools
    so = str(tmp_path / "launch_shim.so")
    subprocess.run(["gcc", "-shared", "-fPIC", "-O1", "-o", so, os.path.join(here, "hip_shim", "launch_shim.c")], check=True)
    desc = {k["name"]: k for k in isa_tools.kernel_descriptors(_lib.LIB_PATH)}
    log = str(tmp_path / "launches.log")
    env = dict(os.environ, LD_PRELOAD=so, SRGAN_SHIM_LOG=log)
    env.pop("SRGAN_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(here, "hip_shim", "drive_guard.py"), _lib.LIB_PATH, "300", "20000000"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for line in open(log):
        if line.startswith("#"):
            continue
        kname, gx, gy, gz, bx, by, bz, dyn = line.split()
        gx, gy, gz, bx, by, bz, dyn = map(int, (gx, gy, gz, bx, by, bz, dyn))
        short = next((s for s in ("grad_sumsq_partials_kernel", "grad_guard_finalize_kernel", "adam_multi_dev_guard_kernel") if s in kname), None)
        if short is None:
            assert "adam_tick_kernel" in kname, kname            # the unchanged tick is the only other launch
            continue
        k = desc[kname]
        ctx = (kname, (gx, gy, gz), (bx, by, bz))
        assert min(gx, gy, gz, bx, by, bz) >= 1 and (bx, by, bz) == (256, 1, 1) and 256 <= k["max_wg"], ctx
        assert gx * bx < 2 ** 32 and gy < 2 ** 16 and gz < 2 ** 16, ctx
        assert k["lds"] + dyn <= 160 * 1024 and k["scratch"] == 0 and dyn == 0, ctx
        seen.setdefault(short, []).append((gx, gy, gz))
    chunks = -(-(20000000 - sum(1 + i % 7 for i in range(299))) // 4096) + 299
    assert seen["grad_sumsq_partials_kernel"] == [(min(chunks, 2048), 1, 1), (1, 1, 1)]
    assert seen["grad_guard_finalize_kernel"] == [(1, 1, 1), (1, 1, 1)]                       # one workgroup, always
    assert seen["adam_multi_dev_guard_kernel"] == [(2048, 300, 1), (1, 1, 1)]
