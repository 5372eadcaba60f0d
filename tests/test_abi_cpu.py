"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/srgan_hip.h declares."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__
    __graft_entry__.build()
    from srgan_amd import _lib
    return _lib


def test_header_symbols_are_exported_and_bound(built_lib):
    header = open(os.path.join(ROOT, "include", "srgan_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(srgan_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 30
    lib = built_lib.load()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in srgan_hip.h but not exported"
    assert declared == set(built_lib.SIGNATURES), declared ^ set(built_lib.SIGNATURES)
    assert lib.srgan_abi_version() == 1


def test_invalid_arguments_are_reported_without_a_gpu(built_lib):
    import ctypes
    lib = built_lib.load()
    d = built_lib.ConvDesc(1, 8, 8, 4, 9, 9, 4, 3, 3, 1, 1, 0, 36, 9, 3, 1)   # wrong Ho/Wo
    assert lib.srgan_conv2d_workspace(ctypes.byref(d)) == 0
    assert b"do not match geometry" in lib.srgan_last_error()
    assert lib.srgan_adam_step(None, None, None, None, 10, 1e-3, 0.5, 0.999, 1e-8, 1, None) == -1
    with pytest.raises(built_lib.SrganHipError, match="adam"):
        built_lib.check(-1, "adam")
    # collectives (csrc/comm.cpp): argument errors come back before RCCL is touched
    assert lib.srgan_allreduce_bucket(None, None, 16, 0, 1, None) == -1 and b"no communicator" in lib.srgan_last_error()
    assert lib.srgan_allgather_rows(None, None, None, 8, None) == -1 and b"no communicator" in lib.srgan_last_error()
    assert lib.srgan_comm_init(None, 2, 0, None) == -1 and lib.srgan_comm_destroy(None) == 0
    assert lib.srgan_comm_available() in (0, 1)
    # round 5: the 16-bit generic-layer entry points, the pools with 16-bit I/O, the reparametrisation kernels
    buf = (ctypes.c_char * 4096)()
    good = built_lib.ConvDesc(2, 8, 8, 64, 8, 8, 64, 3, 3, 1, 1, 1, 64 * 9, 9, 3, 1)
    assert lib.srgan_igemm16_io_applicable(ctypes.byref(d), 0) == 0                # a descriptor that fails validation is "not served"
    assert lib.srgan_igemm16_io_applicable(ctypes.byref(good), 0) == 0             # fp32 compute mode: not served either
    assert lib.srgan_igemm16_conv(ctypes.byref(good), 0, None, 1, None, None, None, 1, 0, 0.0, None, 0, None) != 0
    assert b"null pointer" in lib.srgan_last_error()
    assert lib.srgan_igemm16_conv(ctypes.byref(good), 2, buf, 1, buf, None, buf, 1, 0, 0.0, None, 0, None) != 0
    assert b"kind" in lib.srgan_last_error()
    assert lib.srgan_igemm16_conv(ctypes.byref(good), 0, buf, 1, buf, None, buf, 1, 0, 0.0, None, 0, None) != 0
    assert b"not applicable" in lib.srgan_last_error()                             # (the bf16 mode is off in this process)
    assert lib.srgan_igemm16_wgrad(ctypes.byref(good), None, None, None, None, 0, None) != 0
    assert lib.srgan_avgpool2_fwd_io(buf, 1, buf, 0, 1, 4, 4, 6, None) != 0        # C % 4 != 0
    assert b"C % 4" in lib.srgan_last_error()
    assert lib.srgan_avgpool2_bwd_io(None, 1, buf, 0, 1, 4, 4, 8, None) != 0
    assert lib.srgan_reparam_fwd(None, buf, buf, buf, buf, 256, None) != 0
    assert b"reparam_fwd" in lib.srgan_last_error()
    assert lib.srgan_reparam_bwd(buf, buf, buf, buf, 0, None) != 0
    # round 6: conv + activation with 16-bit tensors -- the discriminator trunks' 4x4 / stride-2 layers and the generator's 7x7
    # RGB layers, whose 3-channel side is fp32 (a bf16 flag there is an argument error, reported before any launch)
    rgb_in = built_lib.ConvDesc(2, 64, 64, 3, 64, 64, 64, 7, 7, 1, 3, 0, 147, 49, 7, 1)
    rgb_out = built_lib.ConvDesc(2, 64, 64, 64, 64, 64, 3, 7, 7, 1, 3, 0, 64 * 49, 49, 7, 1)
    d_c2 = built_lib.ConvDesc(4, 64, 64, 64, 32, 32, 128, 4, 4, 2, 1, 0, 64 * 16, 16, 4, 1)
    for desc in (rgb_in, rgb_out, d_c2):
        assert lib.srgan_conv2d_io_applicable(ctypes.byref(desc), 0) == 0          # fp32 compute mode: not served
    assert lib.srgan_conv2d_io_fwd(ctypes.byref(rgb_in), buf, 0, buf, None, buf, 1, 0, 0.0, None, 0, None) != 0
    assert b"not applicable" in lib.srgan_last_error()
    assert lib.srgan_set_compute_mode(1) == 0
    try:
        assert lib.srgan_conv2d_io_applicable(ctypes.byref(rgb_in), 0) == 1 and lib.srgan_conv2d_io_applicable(ctypes.byref(rgb_out), 0) == 1
        assert lib.srgan_conv2d_io_applicable(ctypes.byref(rgb_in), 2) == 0        # no activation epilogue on the RGB layers
        assert lib.srgan_conv2d_io_applicable(ctypes.byref(d_c2), 2) == 1
        assert lib.srgan_conv2d_io_fwd(ctypes.byref(rgb_in), buf, 1, buf, None, buf, 1, 0, 0.0, None, 0, None) != 0
        assert b"3-channel input of the RGB input layer is fp32" in lib.srgan_last_error()
        assert lib.srgan_conv2d_io_fwd(ctypes.byref(rgb_out), buf, 1, buf, None, buf, 1, 0, 0.0, None, 0, None) != 0
        assert b"3-channel result of the RGB output layer is fp32" in lib.srgan_last_error()
        assert lib.srgan_conv2d_io_dgrad(ctypes.byref(rgb_in), buf, 1, buf, buf, 1, None, 0, None) != 0
        assert b"3-channel input gradient" in lib.srgan_last_error()
        assert lib.srgan_conv2d_io_dgrad(ctypes.byref(rgb_out), buf, 1, buf, buf, 1, None, 0, None) != 0
        assert b"3-channel gradient" in lib.srgan_last_error()
        assert lib.srgan_halo16_wgrad(ctypes.byref(rgb_in), buf, 1, buf, 1, buf, buf, 1 << 30, None) != 0
        assert b"3-channel tensor of an RGB layer is fp32" in lib.srgan_last_error()
        assert lib.srgan_halo16_wgrad(ctypes.byref(rgb_out), buf, 1, buf, 1, buf, buf, 1 << 30, None) != 0
        assert b"3-channel tensor of an RGB layer is fp32" in lib.srgan_last_error()
        assert lib.srgan_conv2d_io_fwd(ctypes.byref(d_c2), None, 1, buf, None, buf, 1, 2, 0.01, None, 0, None) != 0
        assert b"null pointer" in lib.srgan_last_error()
    finally:
        assert lib.srgan_set_compute_mode(0) == 0


def test_instance_norm_entries_refuse_what_they_refused(built_lib):
    """Every refusal of the six instance-norm entries (csrc/norm.hip): -1, the entry's own message, and the order in which the
    conditions are tested.  Fake pointers; every call here is refused before a launch."""
    import ctypes
    lib = built_lib.load()
    x, y, r, g, d, m, s, a, b = (ctypes.cast((ctypes.c_char * 64)(), ctypes.c_void_p) for _ in range(9))
    ws = (ctypes.c_char * 64)()
    SLAB, TWO, ODD = (32, 63, 128), (2, 81, 16), (2, 81, 12)       # slab kernels; two-pass with the pow2 finish; fp32 entries only
    assert lib.srgan_instnorm_slab_applicable(*SLAB) == 1 and lib.srgan_instnorm_slab_applicable(*TWO) == 0
    assert lib.srgan_instnorm_io_applicable(*SLAB) == 1 and lib.srgan_instnorm_io_applicable(*TWO) == 1
    assert lib.srgan_instnorm_io_applicable(*ODD) == 0
    need = {shape: lib.srgan_instnorm_workspace(*shape) for shape in (SLAB, TWO, ODD)}
    assert all(v > 64 for v in need.values())

    def refused(rc, message):
        assert rc == -1 and lib.srgan_last_error() == message.encode(), (rc, lib.srgan_last_error(), message)

    # ---- forward ----
    def fwd(shape, x=x, scale=a, shift=b, res=None, y=y, mean=m, rstd=s, ws=ws, nb=None):
        return lib.srgan_instnorm_fwd(x, scale, shift, res, y, mean, rstd, *shape, 1e-5, 0, 0.0, ws, need[shape] if nb is None else nb, None)

    def slab_fwd(shape, x=x, scale=a, shift=b, res=None, y=y, y16=0, mean=m, rstd=s):
        return lib.srgan_instnorm_slab_fwd_io(x, 1, scale, shift, res, y, y16, mean, rstd, *shape, 1e-5, 0, 0.0, None)

    def fwd_io(shape, x=x, scale=a, shift=b, res=None, y=y, y16=0, mean=m, rstd=s, ws=ws, nb=None):
        return lib.srgan_instnorm_fwd_io(x, 1, scale, shift, res, y, y16, mean, rstd, *shape, 1e-5, 0, 0.0, ws,
                                         need[shape] if nb is None else nb, None)

    for name, call in (("instnorm_fwd", fwd), ("instnorm_slab_fwd_io", slab_fwd), ("instnorm_fwd_io", fwd_io)):
        for shape in (SLAB, TWO) if call is not slab_fwd else (SLAB,):
            for missing in ("x", "y", "mean", "rstd"):
                refused(call(shape, **{missing: None}), name + ": null pointer")
    for shape in ((0, 81, 16), (2, 0, 16), (2, 81, 0)):
        need[shape] = 0
        refused(fwd(shape), "instnorm_fwd: bad shape")
        refused(fwd(shape, shift=None), "instnorm_fwd: bad shape")                         # (tested before the affine pair)
    for shape in (SLAB, TWO, ODD):
        refused(fwd(shape, shift=None), "instnorm_fwd: scale and shift go together")
        refused(fwd(shape, scale=None, ws=None), "instnorm_fwd: scale and shift go together")
        refused(fwd(shape, ws=None), "instnorm_fwd: workspace too small")                  # (on a slab shape too)
        refused(fwd(shape, nb=need[shape] - 1), "instnorm_fwd: workspace too small")
    refused(slab_fwd(SLAB, shift=None), "instnorm_slab_fwd_io: scale and shift go together")
    refused(slab_fwd(TWO, scale=None), "instnorm_slab_fwd_io: scale and shift go together")  # (tested before the shape)
    for shape in (TWO, ODD):
        refused(slab_fwd(shape), "instnorm_slab_fwd_io: shape not served by the slab kernels (srgan_instnorm_slab_applicable)")
        refused(slab_fwd(shape, res=r, y16=1), "instnorm_slab_fwd_io: shape not served by the slab kernels (srgan_instnorm_slab_applicable)")
    refused(slab_fwd(SLAB, res=r, y16=1), "instnorm_slab_fwd_io: the skip tensor is added to an fp32 result only")
    refused(fwd_io(ODD), "instnorm_fwd_io: shape not served (srgan_instnorm_io_applicable)")
    refused(fwd_io(ODD, y=x), "instnorm_fwd_io: shape not served (srgan_instnorm_io_applicable)")
    refused(fwd_io((0, 81, 16)), "instnorm_fwd_io: shape not served (srgan_instnorm_io_applicable)")
    for shape in (SLAB, TWO):
        refused(fwd_io(shape, y=x), "instnorm_fwd_io: in-place calls are not supported")
        refused(fwd_io(shape, res=y), "instnorm_fwd_io: in-place calls are not supported")
        refused(fwd_io(shape, res=y, y16=1), "instnorm_fwd_io: in-place calls are not supported")
        refused(fwd_io(shape, res=r, y16=1), "instnorm_fwd_io: the skip tensor is added to an fp32 result only")
        refused(fwd_io(shape, res=r, y16=1, shift=None, ws=None), "instnorm_fwd_io: the skip tensor is added to an fp32 result only")
    # an io call on a slab shape is the slab entry's from here on: no workspace is asked for, and the slab entry's messages come back
    refused(fwd_io(SLAB, shift=None, ws=None, nb=0), "instnorm_slab_fwd_io: scale and shift go together")
    refused(fwd_io(TWO, shift=None, ws=None, nb=0), "instnorm_fwd_io: scale and shift go together")
    refused(fwd_io(TWO, ws=None), "instnorm_fwd_io: workspace too small (srgan_instnorm_workspace)")
    refused(fwd_io(TWO, nb=need[TWO] - 1), "instnorm_fwd_io: workspace too small (srgan_instnorm_workspace)")

    # ---- backward ----
    def bwd(shape, x=x, dy=g, scale=a, shift=b, mean=m, rstd=s, dx=d, dscale=y, dshift=r, ws=ws, nb=None):
        return lib.srgan_instnorm_bwd(x, dy, scale, shift, mean, rstd, dx, dscale, dshift, *shape, 0, 0.0, ws,
                                      need[shape] if nb is None else nb, None)

    def slab_bwd(shape, x=x, x16=1, dy=g, scale=a, shift=b, mean=m, rstd=s, dx=d, dx16=1, dscale=y, dshift=r):
        return lib.srgan_instnorm_slab_bwd_io(x, x16, dy, 0, scale, shift, mean, rstd, dx, dx16, dscale, dshift, *shape, 0, 0.0, None)

    def bwd_io(shape, x=x, x16=1, dy=g, scale=a, shift=b, mean=m, rstd=s, dx=d, dx16=1, dscale=y, dshift=r, ws=ws, nb=None):
        return lib.srgan_instnorm_bwd_io(x, x16, dy, 0, scale, shift, mean, rstd, dx, dx16, dscale, dshift, *shape, 0, 0.0, ws,
                                         need[shape] if nb is None else nb, None)

    for name, call in (("instnorm_bwd", bwd), ("instnorm_slab_bwd_io", slab_bwd), ("instnorm_bwd_io", bwd_io)):
        for shape in (SLAB, TWO) if call is not slab_bwd else (SLAB,):
            for missing in ("x", "dy", "mean", "rstd", "dx", "dscale", "dshift"):
                refused(call(shape, **{missing: None}), name + ": null pointer")
    for shape in (SLAB, TWO, ODD):
        refused(bwd(shape, shift=None), "instnorm_bwd: scale and shift go together")
        refused(bwd(shape, scale=None, ws=None), "instnorm_bwd: scale and shift go together")
        refused(bwd(shape, ws=None), "instnorm_bwd: workspace too small")
        refused(bwd(shape, nb=need[shape] - 1), "instnorm_bwd: workspace too small")
    refused(slab_bwd(SLAB, shift=None), "instnorm_slab_bwd_io: scale and shift go together")
    refused(slab_bwd(TWO, scale=None), "instnorm_slab_bwd_io: scale and shift go together")
    for shape in (TWO, ODD):
        refused(slab_bwd(shape), "instnorm_slab_bwd_io: shape not served by the slab kernels (srgan_instnorm_slab_applicable)")
        refused(slab_bwd(shape, dx16=0), "instnorm_slab_bwd_io: shape not served by the slab kernels (srgan_instnorm_slab_applicable)")
    refused(slab_bwd(SLAB, dx16=0), "instnorm_slab_bwd_io: the input gradient has the input's type")
    refused(slab_bwd(SLAB, x16=0), "instnorm_slab_bwd_io: the input gradient has the input's type")
    refused(bwd_io(ODD), "instnorm_bwd_io: shape not served (srgan_instnorm_io_applicable)")
    refused(bwd_io(ODD, dx16=0), "instnorm_bwd_io: shape not served (srgan_instnorm_io_applicable)")
    for shape in (SLAB, TWO):
        refused(bwd_io(shape, dx16=0), "instnorm_bwd_io: the input gradient has the input's type")
        refused(bwd_io(shape, x16=0, shift=None, ws=None), "instnorm_bwd_io: the input gradient has the input's type")
    refused(bwd_io(SLAB, shift=None, ws=None, nb=0), "instnorm_slab_bwd_io: scale and shift go together")
    refused(bwd_io(TWO, shift=None, ws=None, nb=0), "instnorm_bwd_io: scale and shift go together")
    refused(bwd_io(TWO, ws=None), "instnorm_bwd_io: workspace too small (srgan_instnorm_workspace)")
    refused(bwd_io(TWO, nb=need[TWO] - 1), "instnorm_bwd_io: workspace too small (srgan_instnorm_workspace)")


def test_launch_timer_kernel_ids_and_names(built_lib):
    """bench.py (is_hbm_kernel, executed_divisor), tests/step_bits_common.py and the scripts under scratch/ select timed kernels by
    these names, and a launch site books its time by position in this list: number, spelling and order are part of the ABI."""
    names = [
        "igemm_kernel<128,128,2,2,gen>", "igemm_kernel<128,128,2,2,vec>", "igemm_kernel<128,64,2,2,gen>", "igemm_kernel<128,64,2,2,vec>",
        "igemm_kernel<128,32,4,1,gen>", "igemm_kernel<128,32,4,1,vec>", "igemm_kernel<64,64,2,2,gen>", "igemm_kernel<64,64,2,2,vec>",
        "wgrad_kernel<gen>", "wgrad_kernel<vec>", "igemm_kernel<256,128,4,2,gen>", "igemm_kernel<256,128,4,2,vec>",
        "igemm_kernel<256,64,4,2,gen>", "igemm_kernel<256,64,4,2,vec>", "wino_kernel", "wino_wgrad_kernel", "wino_kernel<4x4s2>",
        "wino_wgrad_kernel<4x4s2>", "wino43_kernel", "wino43_input_kernel", "rgbin_conv_kernel", "rgb_wgrad_kernel", "wino43_wgrad_kernel",
        "wino43_dy_kernel", "halo16_kernel", "halo16_wgrad_kernel", "halo16s2_wgrad_kernel", "halo16t_kernel", "rgbout_conv_kernel",
        "halo16s_kernel", "in_stats_partial", "in_apply", "in_bwd_partial", "in_bwd_apply", "in_fwd_slab", "in_bwd_slab", "igemm16_kernel",
        "wino42_kernel", "in_fwd_slab_v", "in_bwd_slab_vz", "cr_pairs_kernel", "d_losses_cr_kernel", "ms_rows_kernel", "ms_finish_kernel",
        "ms_grad_kernel"]
    lib = built_lib.load()
    assert lib.srgan_prof_num_kernels() == 45 == len(names)
    assert [lib.srgan_prof_kernel_name(k).decode() for k in range(45)] == names
    assert lib.srgan_prof_kernel_name(-1) == b"" and lib.srgan_prof_kernel_name(45) == b""


def test_product_refuses_cpu_tensors(built_lib):
    import torch
    from srgan_amd import ops
    with pytest.raises(built_lib.SrganHipError, match="no CPU fallback"):
        ops.conv2d(torch.zeros(1, 3, 8, 8), torch.zeros(4, 3, 3, 3))


def test_no_experiment_switch_ships_in_the_product_library(built_lib):
    """wrong-result timing switches (SRGAN_EXP_*), the compile-time ablations (WINO_EXP / RGBOUT_EXP /
    W43_DIAG) and the A/B switches of scratch/ exist only in `make exp` builds (scratch/libsrgan_exp.so).  The product library
    reads three environment variables, all test / debug hooks that change no result: listed here and in DESIGN.md."""
    blob = open(built_lib.LIB_PATH, "rb").read()
    names = set(m.decode() for m in re.findall(rb"SRGAN_[A-Z0-9_]{3,}", blob))
    assert not [n for n in names if n.startswith("SRGAN_EXP")], names
    assert names <= {"SRGAN_WINOGRAD_THRESHOLD_SCALE", "SRGAN_PACK_ITEM_PATH", "SRGAN_DEBUG_REDUCE"}, names
    assert not built_lib.EXPERIMENTS and not built_lib.ab("PATH")        # python-side A/B switches are off next to the product library
    # an ablation flag without -DSRGAN_EXPERIMENTS does not compile (csrc/common.h)
    import subprocess
    src = os.path.join(ROOT, "style-restricted_gan_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "--offload-arch=gfx950", "-DWINO_EXP=5", "-I" + os.path.join(ROOT, "include"),
                        "-I" + src, "-E", "-x", "hip", os.path.join(src, "common.h"), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode != 0 and "experiment builds" in r.stderr


def test_no_buffer_store_with_a_scalar_register_offset_in_the_product_isa(built_lib):
    """VERDICT r5 item 3 / DESIGN.md section 8 (toolchain rules).  On gfx950 with ROCm 7.2 a 16-byte `buffer_store` whose
    soffset operand is an SGPR misplaced data in `wino42_kernel`'s epilogue (profiles/LOG.md, round 5): the compiler's hazard
    recognizer treats a register soffset as "no store-data hazard" and lets the data registers be rewritten right behind the
    store.  The product keeps every buffer store on `soffset = 0` (offsets go into the vector offset); this test disassembles
    every gfx950 code object of the library and fails if a buffer store with any other soffset operand appears.  Loads with an
    SGPR soffset (the gathers, the filter fragments) are unaffected and allowed."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import isa_tools
    isa = isa_tools.disassemble(built_lib.LIB_PATH)
    stores = re.findall(r"^\s*(buffer_(?:store|atomic)\w*)\s+(.*?)(?://.*)?$", isa, flags=re.M)
    assert len(stores) >= 50, len(stores)                       # the F(4x4,2x2) epilogues alone hold ~100
    bad = []
    for op, operands in stores:
        ops = [o.strip() for o in operands.split(",")]
        assert len(ops) >= 4, (op, operands)                    # vdata, vaddr, srsrc, soffset [modifiers]
        soffset = ops[3].split()[0]
        if soffset not in ("0", "off"):
            bad.append((op, operands.strip()))
    assert not bad, bad[:5]
    # the loads are there and do use scalar offsets: the pattern above is looking at the right operand
    loads = re.findall(r"^\s*buffer_load\w*\s+(.*?)(?://.*)?$", isa, flags=re.M)
    # (the LDS-DMA form `buffer_load_dwordx4 vaddr, srsrc, soffset offen lds` has no data operand)
    def soffset(o):
        ops = [t.strip() for t in o.split(",")]
        return (ops[2] if " lds" in " " + ops[-1] else ops[3]).split()[0]
    assert sum(1 for o in loads if re.match(r"s\d+", soffset(o))) > 100
