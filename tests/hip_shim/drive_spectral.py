"""Runs under LD_PRELOAD=launch_shim.so (tests/test_spectral_cpu.py): calls the spectral-normalisation entry points of the C ABI --
a refresh with one power iteration, a refresh without, a projection -- for the twelve conv layers of the full-width discriminator
and for a single 1 x 4096 layer, with fake device pointers.  Nothing executes; the shim logs every launch descriptor.
usage: drive_spectral.py <lib>"""
import ctypes
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from drive_batchnorm import FAKE                                               # noqa: E402
from srgan_amd import _lib                                                     # noqa: E402  (ctypes only, no torch)


def d_layers(nch=64, num_cls=4, n_class=4):
    """(O, K) of SingleDiscriminator_solo_multi(3, nch, 2, num_cls, n_class=n_class) in module order"""
    out = []
    for width in (nch, nch // 2):
        w = [min(width * 2 ** i, width * 8) for i in range(num_cls)]
        out.append((w[0], 3 * 16))
        out += [(w[i], w[i - 1] * 16) for i in range(1, num_cls)]
    dim = min(nch * 2 ** num_cls, nch * 8)
    return out + [(1, dim * 16), (1, dim // 2 * 16), (n_class, dim * 64), (n_class, dim // 2 * 16)]


CASES = (("discriminator", d_layers()), ("one layer", [(1, 4096)]))


def table(layers):
    rows = []
    for i, (o, k) in enumerate(layers):
        base = FAKE + (i << 28)
        rows += [base, base + (1 << 26), base + (2 << 26), base + (3 << 26), FAKE + (15 << 28) + 4 * i, o, k] + [0] * 9
    return (ctypes.c_char * (8 * len(rows))).from_buffer_copy(struct.pack(f"{len(rows)}Q", *rows))


def main():
    lib_path = sys.argv[1]
    os.environ["SRGAN_HIP_LIB"] = lib_path
    _lib.LIB_PATH = lib_path
    lib = _lib.load()
    mark = ctypes.CDLL(None).srgan_shim_mark
    mark.argtypes = [ctypes.c_char_p]
    p = ctypes.c_void_p(FAKE)
    for name, layers in CASES:
        host = table(layers)
        plan = (ctypes.c_char * lib.srgan_spectral_plan_bytes())()
        assert lib.srgan_spectral_plan(ctypes.byref(host), len(layers), ctypes.byref(plan)) == 0, lib.srgan_last_error()
        ws = lib.srgan_spectral_workspace(ctypes.byref(plan))
        assert ws > 0, name
        for what, call in (("refresh", lambda: lib.srgan_spectral_refresh(p, ctypes.byref(plan), 1, 1, 1e-12, p, ws, None)),
                           ("materialise", lambda: lib.srgan_spectral_refresh(p, ctypes.byref(plan), 0, 1, 1e-12, p, ws, None)),
                           ("project", lambda: lib.srgan_spectral_project(p, ctypes.byref(plan), p, p, ws, None))):
            mark(f"{name}: {what}".encode())
            assert call() == 0, (name, what, lib.srgan_last_error())


if __name__ == "__main__":
    main()
