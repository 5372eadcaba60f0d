"""Runs under LD_PRELOAD=launch_shim.so (tests/test_conv_refs_cpu.py): calls every convolution entry point of the C ABI for a
list of layer geometries with fake device pointers, in both compute modes and under both dispatch settings (default, and
SRGAN_WINOGRAD_THRESHOLD_SCALE=0, which the library reads per call).  Nothing executes; the shim logs every launch the host code
of csrc/conv_*.hip makes, one `srgan_shim_mark` per (case, mode, dispatch, entry):  "# <tag> m<mode> <dispatch> <entry>".
usage: drive_conv.py <lib> <json file: list of [tag, N, I, H, W, O, k, stride, pad, reflect, bias]>"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "style-restricted_gan_amd"))
from srgan_amd import _lib                                                     # noqa: E402  (ctypes only, no torch)

FAKE = 0x7000_0000_0000          # "device" pointers: never dereferenced on the host
BIG = 1 << 40
DISPATCH = (("default", None), ("forced", "0"))


def main():
    lib_path, cases = sys.argv[1], json.load(open(sys.argv[2]))
    os.environ["SRGAN_HIP_LIB"] = lib_path
    _lib.LIB_PATH = lib_path
    lib = _lib.load()
    mark_ = ctypes.CDLL(None).srgan_shim_mark
    mark_.argtypes = [ctypes.c_char_p]
    p = ctypes.c_void_p(FAKE)
    for tag, N, I, H, W, O, k, s, pad, reflect, has_bias in cases:
        Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
        d = _lib.ConvDesc(N, H, W, I, Ho, Wo, O, k, k, s, pad, 1 if reflect else 0, I * k * k, k * k, k, 1)
        dref = ctypes.byref(d)
        bias = p if has_bias else None
        for mode in (0, 1):
            assert lib.srgan_set_compute_mode(mode) == 0
            for dname, scale in DISPATCH:
                if scale is None:
                    os.environ.pop("SRGAN_WINOGRAD_THRESHOLD_SCALE", None)
                else:
                    os.environ["SRGAN_WINOGRAD_THRESHOLD_SCALE"] = scale
                where = f"{tag} m{mode} {dname}"

                def mark(entry):
                    mark_(f"{where} {entry}".encode())

                def call(what, rc):
                    assert rc == 0, (where, what, lib.srgan_last_error())

                def scratch(kind):      # as srgan_amd.ops hands it over: a buffer only where the layer asks for one
                    nb = lib.srgan_conv2d_packed_scratch(dref, kind)
                    return (p, nb) if nb else (None, 0)

                mark("fwd")
                call("fwd", lib.srgan_conv2d_fwd(dref, p, p, bias, p, 0, 0.0, p, BIG, None))
                mark("dgrad")
                call("dgrad", lib.srgan_conv2d_dgrad(dref, p, p, p, p, BIG, None))
                mark("wgrad")
                call("wgrad", lib.srgan_conv2d_wgrad(dref, p, p, p, bias, p, BIG, None))
                mark("pack0")
                call("pack0", lib.srgan_conv2d_pack(dref, 0, 0, p, p, BIG, None))
                mark("fwd_packed")
                call("fwd_packed", lib.srgan_conv2d_fwd_packed(dref, p, p, bias, p, 0, 0.0, *scratch(0), None))
                mark("pack1")
                call("pack1", lib.srgan_conv2d_pack(dref, 1, 0, p, p, BIG, None))
                ws, nb = scratch(1)
                mark("dgrad_packed")
                call("dgrad_packed", lib.srgan_conv2d_dgrad_packed(dref, p, p, p, ws, nb, None))
                mark("dgrad_packed_add")
                call("dgrad_packed_add", lib.srgan_conv2d_dgrad_packed_add(dref, p, p, p, ctypes.c_void_p(FAKE + BIG), ws, nb, None))
                mark("dgrad_packed_mask")
                call("dgrad_packed_mask", lib.srgan_conv2d_dgrad_packed_mask(dref, p, p, p, 0.2, ctypes.c_void_p(FAKE + BIG), ws, nb, None))
                if lib.srgan_conv2d_wgrad_v_bytes(dref):
                    mark("wgrad_v")
                    call("wgrad_v", lib.srgan_conv2d_wgrad_v(dref, p, p, p, bias, p, BIG, None))
                # the fused norm + convolution nodes: V / Z images written by the norm kernels, multiply / gradients from them
                if lib.srgan_instnorm_conv_v_applicable(dref):
                    mark("instnorm_fwd_v")
                    call("instnorm_fwd_v", lib.srgan_instnorm_fwd_v(dref, p, p, p, p, p, p, BIG, 1e-5, 1, 0.0, None))
                    mark("fwd_from_v")
                    call("fwd_from_v", lib.srgan_conv2d_fwd_from_v(dref, p, p, bias, p, 0, 0.0, None))
                if lib.srgan_instnorm_bwd_vz_applicable(dref):
                    mark("instnorm_bwd_vz")
                    call("instnorm_bwd_vz", lib.srgan_instnorm_bwd_vz(dref, p, p, p, p, p, p, p, p, p, BIG, p, BIG, 1, 0.0, None))
                    mark("dgrad_from_v")
                    call("dgrad_from_v", lib.srgan_conv2d_dgrad_from_v(dref, p, p, p, ctypes.c_void_p(FAKE + BIG), None))
                    mark("wgrad_vz")
                    call("wgrad_vz", lib.srgan_conv2d_wgrad_vz(dref, p, p, p, p, BIG, None))
                # the entries with 16-bit tensors, over the dtype pairings of drive_launches.py
                if lib.srgan_halo16_applicable(dref):      # the skip gradient of the residual block, added to an fp32 result
                    for i16 in (0, 1):
                        mark(f"halo16_conv_res:in16={i16}")
                        call("halo16_res", lib.srgan_halo16_conv(dref, 1, p, i16, p, p, ctypes.c_void_p(FAKE + BIG), 0, None))
                if lib.srgan_halo16_applicable(dref) or lib.srgan_halo16s2_applicable(dref):
                    for kind in (0, 1):
                        for i16 in (0, 1):
                            for o16 in (0, 1):
                                mark(f"halo16_conv:kind{kind}:in16={i16}:out16={o16}")
                                call("halo16", lib.srgan_halo16_conv(dref, kind, p, i16, p, None, p, o16, None))
                    for x16 in (0, 1):
                        for d16 in (0, 1):
                            if x16 and not d16 and not lib.srgan_halo16s2_applicable(dref):
                                continue                    # (the 3x3 kernel has no bf16 x with fp32 dy; the stride-2 one has)
                            mark(f"halo16_wgrad:x16={x16}:d16={d16}")
                            call("halo16_wgrad", lib.srgan_halo16_wgrad(dref, p, x16, p, d16, p, p, BIG, None))
                if lib.srgan_igemm16_io_applicable(dref, 0):
                    for kind in (0, 1):
                        for i16 in (0, 1):
                            for o16 in (0, 1):
                                mark(f"igemm16_conv:kind{kind}:in16={i16}:out16={o16}")
                                call("igemm16", lib.srgan_igemm16_conv(dref, kind, p, i16, p, None, p, o16, 0, 0.0, p, BIG, None))
                    mark("igemm16_wgrad")
                    call("igemm16_wgrad", lib.srgan_igemm16_wgrad(dref, p, p, p, p, BIG, None))
                for act in (0, 2):
                    if not lib.srgan_conv2d_io_applicable(dref, act):
                        continue
                    ins = (0,) if I == 3 else (0, 1)
                    outs = (0,) if O == 3 else (0, 1)
                    for i16 in ins:
                        for o16 in outs:
                            mark(f"io_fwd:act{act}:in16={i16}:out16={o16}")
                            call("io_fwd", lib.srgan_conv2d_io_fwd(dref, p, i16, p, None, p, o16, act, 0.01, p, BIG, None))
                            mark(f"io_dgrad:act{act}:dy16={o16}:dx16={i16}")
                            call("io_dgrad", lib.srgan_conv2d_io_dgrad(dref, p, o16, p, p, i16, p, BIG, None))
                            # (every layer of these entries takes its weight gradient from srgan_halo16_wgrad, with the tensors' types)
                            mark(f"io_wgrad:act{act}:x16={i16}:d16={o16}")
                            call("io_wgrad", lib.srgan_halo16_wgrad(dref, p, i16, p, o16, p, p, BIG, None))
    os.environ.pop("SRGAN_WINOGRAD_THRESHOLD_SCALE", None)
    lib.srgan_set_compute_mode(0)
    # entries that serve many layers with one launch: every stale packed operand, every queued split-K slab sum
    d = _lib.ConvDesc(2, 8, 8, 32, 8, 8, 32, 3, 3, 1, 1, 0, 32 * 9, 9, 3, 1)
    mark_(b"- m0 default pack_multi")
    assert lib.srgan_conv2d_pack_multi(p, 2, None) == 0, lib.srgan_last_error()
    mark_(b"- m0 default wgrad_deferred")
    assert lib.srgan_wgrad_defer_begin(p, BIG, None) == 0, lib.srgan_last_error()
    assert lib.srgan_set_wgrad_accumulate(2) == 0
    assert lib.srgan_conv2d_wgrad(ctypes.byref(d), p, p, p, None, p, BIG, None) == 0, lib.srgan_last_error()
    assert lib.srgan_set_wgrad_accumulate(0) == 0
    assert lib.srgan_wgrad_defer_end() == 0, lib.srgan_last_error()


if __name__ == "__main__":
    main()
