"""Runs under LD_PRELOAD=launch_shim.so (tests/test_geom_refs_cpu.py): calls the three entry points of the geometric augmentation --
the forward and backward warp of csrc/augment_geom.hip, ungated and gated, and the gate of csrc/ada.hip -- at the shapes of
tests/test_geom_kernels_gpu.py and the headline batch, with fake device pointers.  Nothing executes; the shim logs every launch
descriptor.
usage: drive_geom.py <lib>"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from drive_batchnorm import FAKE                                               # noqa: E402
from srgan_amd import _lib                                                     # noqa: E402  (ctypes only, no torch)

SHAPES = ((1, 1, 1), (1, 2, 2), (3, 5, 7), (2, 8, 8), (5, 16, 12), (2, 7, 7), (2, 6, 10), (2, 32, 64), (2, 36, 57), (2, 3, 683),
          (4, 128, 128), (2048, 2, 2), (2049, 2, 2), (64, 128, 128), (64, 256, 256))


def main():
    lib_path = sys.argv[1]
    os.environ["SRGAN_HIP_LIB"] = lib_path
    _lib.LIB_PATH = lib_path
    lib = _lib.load()
    mark = ctypes.CDLL(None).srgan_shim_mark
    mark.argtypes = [ctypes.c_char_p]
    p = [ctypes.c_void_p(FAKE + (i << 32)) for i in range(4)]
    for n, h, w in SHAPES:
        mark(f"{n} {h} {w}".encode())
        for gated in (0, 1):
            assert lib.srgan_geom_augment_fwd(p[0], p[1], p[2], n, 3, h, w, 15, gated, None) == 0, lib.srgan_last_error()
            assert lib.srgan_geom_augment_bwd(p[2], p[1], p[0], n, 3, h, w, 15, gated, None) == 0, lib.srgan_last_error()
        assert lib.srgan_ada_gate(p[0], p[3], p[1], n, 4, None) == 0, lib.srgan_last_error()


if __name__ == "__main__":
    main()
