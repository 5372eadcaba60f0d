"""Runs under LD_PRELOAD=launch_shim.so (tests/test_grad_guard_cpu.py): calls the gradient guard's entry points of the C ABI --
the reduction and the guarded Adam update -- for an optimiser of <n_tensors> tensors and <total> elements in all (and for one
tiny tensor), with fake device pointers.  Nothing executes; the shim logs every launch descriptor.
usage: drive_guard.py <lib> <n_tensors> <total_elements>"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from drive_batchnorm import FAKE                                               # noqa: E402
from srgan_amd import _lib                                                     # noqa: E402  (ctypes only, no torch)

CHUNK = 4096


def main():
    lib_path, n_tensors, total = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    os.environ["SRGAN_HIP_LIB"] = lib_path
    _lib.LIB_PATH = lib_path
    lib = _lib.load()
    mark = ctypes.CDLL(None).srgan_shim_mark
    mark.argtypes = [ctypes.c_char_p]
    p = ctypes.c_void_p(FAKE)
    # one large tensor and n - 1 small ones, as an encoder with many biases has them
    small = [1 + i % 7 for i in range(n_tensors - 1)]
    sizes = [total - sum(small)] + small
    for name, ns in (("optimiser", sizes), ("one element", [1])):
        chunks = sum(-(-n // CHUNK) for n in ns)
        ws = lib.srgan_grad_guard_workspace(chunks)
        assert ws == 4 * chunks, name
        mark(f"{name}: {len(ns)} tensors, {sum(ns)} elements, {chunks} chunks".encode())
        rc = lib.srgan_grad_guard_reduce(p, len(ns), chunks, p, ws, p, None)
        assert rc == 0, (name, lib.srgan_last_error())
        rc = lib.srgan_adam_multi_dev_guard(p, len(ns), max(ns), p, p, None)
        assert rc == 0, (name, lib.srgan_last_error())


if __name__ == "__main__":
    main()
