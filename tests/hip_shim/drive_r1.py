"""Runs under LD_PRELOAD=launch_shim.so (tests/test_r1_refs_cpu.py): calls the two entry points of csrc/r1.hip -- the seed pass and
the finalize -- at the shapes of tests/test_r1_kernels_gpu.py, the headline batch and a batch past the grid cap, with fake device
pointers.  Nothing executes; the shim logs every launch descriptor.
usage: drive_r1.py <lib>"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from drive_batchnorm import FAKE                                               # noqa: E402
from srgan_amd import _lib                                                     # noqa: E402  (ctypes only, no torch)

SHAPES = ((1, 1, 1), (2, 3, 5), (3, 32, 32), (2, 33, 47), (1, 37, 111), (2, 40, 24), (2, 128, 128), (32, 128, 128), (64, 256, 256))


def main():
    lib_path = sys.argv[1]
    os.environ["SRGAN_HIP_LIB"] = lib_path
    _lib.LIB_PATH = lib_path
    lib = _lib.load()
    mark = ctypes.CDLL(None).srgan_shim_mark
    mark.argtypes = [ctypes.c_char_p]
    p = [ctypes.c_void_p(FAKE + (i << 28)) for i in range(5)]
    for n, h, w in SHAPES:
        ws = lib.srgan_r1_workspace(n, h, w)
        assert ws > 0, (n, h, w)
        mark(f"{n} {h} {w}".encode())
        assert lib.srgan_r1_seed(p[0], p[1], p[2], p[3], n, 3, h, w, p[4], ws, None) == 0, lib.srgan_last_error()
        assert lib.srgan_r1_finalize(p[4], ws, n, h, w, p[2], None) == 0, lib.srgan_last_error()


if __name__ == "__main__":
    main()
