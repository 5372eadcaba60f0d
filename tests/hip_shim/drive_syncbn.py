"""Runs under LD_PRELOAD=launch_shim.so (tests/test_syncbn_cpu.py): calls the synced batch-norm entry points of the C ABI -- both
phases of the forward and of the backward -- for every norm shape of tier-F G and E with norm_type="batch" at one BASELINE
geometry and one world size, with fake device pointers.  Nothing executes; the shim logs every launch descriptor.
usage: drive_syncbn.py <lib> <H> <N_global> <world>"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from drive_batchnorm import FAKE, norm_shapes                                  # noqa: E402
from srgan_amd import _lib                                                     # noqa: E402  (ctypes only, no torch)


def main():
    lib_path, H, NG, W = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    os.environ["SRGAN_HIP_LIB"] = lib_path
    _lib.LIB_PATH = lib_path
    lib = _lib.load()
    mark = ctypes.CDLL(None).srgan_shim_mark
    mark.argtypes = [ctypes.c_char_p]
    p = ctypes.c_void_p(FAKE)
    NL = NG // W
    for name, N, HW, C, cbb in norm_shapes(H, NG):
        for r in (0, W - 1):
            n0 = r * NL
            nb = lib.srgan_batchnorm_sync_exchange_bytes(N, NL, HW, C, 0)
            nbs = lib.srgan_batchnorm_sync_exchange_bytes(N, NL, HW, C, cbb)
            wb = lib.srgan_batchnorm_sync_workspace(NL, C)
            assert nb and nbs and wb, name
            mark(f"{name} N{N} W{W} rank{r} fwd".encode())
            rc = lib.srgan_batchnorm_sync_fwd_partial(p, p, nb, N, n0, NL, HW, C, None)
            assert rc == 0, (name, lib.srgan_last_error())
            if cbb:
                rc = lib.srgan_cbbnorm_sync_fwd_apply(p, p, p, p, p, p, p, p, p, p, p, p, p, p, nb, N, n0, NL, HW, C, 0.1, 0, 1e-5, 1, 0.0, None)
            else:
                rc = lib.srgan_batchnorm_sync_fwd_apply(p, p, p, p, p, p, p, p, p, p, p, p, p, nb, N, n0, NL, HW, C, 0.0, 1, 1e-5, 2, 0.2, None)
            assert rc == 0, (name, lib.srgan_last_error())
            mark(f"{name} N{N} W{W} rank{r} bwd".encode())
            rc = lib.srgan_batchnorm_sync_bwd_partial(p, p, p if cbb else None, p, p, p, p, p, nbs, N, n0, NL, HW, C, 1, 0.0, None)
            assert rc == 0, (name, lib.srgan_last_error())
            if cbb:
                rc = lib.srgan_cbbnorm_sync_bwd_apply(p, p, p, p, p, p, p, p, nbs, p, p, p, N, n0, NL, HW, C, 1, 0.0, p, wb, None)
            else:
                rc = lib.srgan_batchnorm_sync_bwd_apply(p, p, p, p, p, p, p, p, p, nbs, p, p, p, N, n0, NL, HW, C, 2, 0.2, p, wb, None)
            assert rc == 0, (name, lib.srgan_last_error())


if __name__ == "__main__":
    main()
