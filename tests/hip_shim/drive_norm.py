"""Runs under LD_PRELOAD=launch_shim.so (tests/test_norm_refs_cpu.py): calls the instance-norm entry points of the C ABI for a
list of shapes with fake device pointers.  Nothing executes; the shim logs every launch the host code of csrc/norm.hip makes.
usage: drive_norm.py <lib> <json list of [tag, N, HW, C, null | [a_bf16, b_bf16]]>"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "style-restricted_gan_amd"))
from srgan_amd import _lib                                                     # noqa: E402  (ctypes only, no torch)

FAKE = 0x7000_0000_0000          # "device" pointers: never dereferenced on the host
BIG = 1 << 40


def main():
    lib_path, calls = sys.argv[1], json.loads(sys.argv[2])
    os.environ["SRGAN_HIP_LIB"] = lib_path
    _lib.LIB_PATH = lib_path
    lib = _lib.load()
    mark = ctypes.CDLL(None).srgan_shim_mark
    mark.argtypes = [ctypes.c_char_p]
    p, out = ctypes.c_void_p(FAKE), ctypes.c_void_p(FAKE + BIG)      # out-of-place: the result is another tensor
    for tag, N, HW, C, io in calls:
        ws = lib.srgan_instnorm_workspace(N, HW, C)
        mark(f"{tag} fwd".encode())
        if io is None:
            rc = lib.srgan_instnorm_fwd(p, p, p, None, out, p, p, N, HW, C, 1e-5, 1, 0.0, p, ws, None)
        else:
            rc = lib.srgan_instnorm_fwd_io(p, io[0], p, p, None, out, io[1], p, p, N, HW, C, 1e-5, 1, 0.0, p, ws, None)
        assert rc == 0, (tag, lib.srgan_last_error())
        mark(f"{tag} bwd".encode())
        if io is None:
            rc = lib.srgan_instnorm_bwd(p, p, p, p, p, p, out, p, p, N, HW, C, 1, 0.0, p, ws, None)
        else:       # dy has y's type, dx has x's
            rc = lib.srgan_instnorm_bwd_io(p, io[0], p, io[1], p, p, p, p, out, io[0], p, p, N, HW, C, 1, 0.0, p, ws, None)
        assert rc == 0, (tag, lib.srgan_last_error())


if __name__ == "__main__":
    main()
