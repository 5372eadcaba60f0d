"""Runs under LD_PRELOAD=launch_shim.so (tests/test_batchnorm_cpu.py): calls the batch-norm entry points of the C ABI -- forward in
training and eval mode, backward -- for every norm shape of tier-F G and E with norm_type="batch" at one BASELINE geometry, with
fake device pointers.  Nothing executes; the shim logs every launch descriptor.  usage: drive_batchnorm.py <lib> <H> <B>"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "style-restricted_gan_amd"))
from srgan_amd import _lib                                                     # noqa: E402  (ctypes only, no torch)

FAKE = 0x7000_0000_0000          # "device" pointers: never dereferenced on the host


def norm_shapes(H, B):
    """(name, N, HW, C, cbb) of every norm: the generator's down / residual CBB layers and up-path BN, the encoder blocks' BN and
    Encoder_original's CBB blocks."""
    out = [("G.cn0", B, H * H, 64, 1), ("G.cn1", B, H * H // 4, 128, 1), ("G.cn2", B, H * H // 16, 256, 1),
           ("G.up0", B, H * H // 4, 128, 0), ("G.up1", B, H * H, 64, 0)]
    he, c = (H + 2 - 7) // 2 + 1, 64
    for b in range(4):
        out += [(f"E.l{b}", B, he * he, c, 0), (f"Eo.l{b}", B, he * he, c, 1)]
        c, he = 2 * c, he // 2
    return out


def main():
    lib_path, H, B = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    os.environ["SRGAN_HIP_LIB"] = lib_path
    _lib.LIB_PATH = lib_path
    lib = _lib.load()
    mark = ctypes.CDLL(None).srgan_shim_mark
    mark.argtypes = [ctypes.c_char_p]
    p = ctypes.c_void_p(FAKE)
    for name, N, HW, C, cbb in norm_shapes(H, B):
        nb = lib.srgan_batchnorm_workspace(N, HW, C)
        for training in (1, 0):
            mark(f"{name} N{N} train{training} fwd".encode())
            if cbb:
                rc = lib.srgan_cbbnorm_fwd(p, p, p, p if training else None, p, p, p, p, p, p, p, p, p, N, HW, C, training, 0.1, 0,
                                           1e-5, 1, 0.0, p, nb, None)
            else:
                rc = lib.srgan_batchnorm_fwd(p, p, p, p, p, p, p, p, p, p, p, p, N, HW, C, training, 0.0, 1, 1e-5, 2, 0.2, p, nb, None)
            assert rc == 0, (name, lib.srgan_last_error())
            mark(f"{name} N{N} train{training} bwd".encode())
            if cbb:
                rc = lib.srgan_cbbnorm_bwd(p, p, p, p, p, p, p, p, p, p, p, N, HW, C, training, 1, 0.0, p, nb, None)
            else:
                rc = lib.srgan_batchnorm_bwd(p, p, p, p, p, p, p, p, p, p, p, N, HW, C, training, 2, 0.2, p, nb, None)
            assert rc == 0, (name, lib.srgan_last_error())


if __name__ == "__main__":
    main()
