"""CPU: the yardsticks of the convolution tests (tests/test_ops_gpu.py, tests/test_conv_kernels_gpu.py) are pinned here, without
a GPU -- every hand-picked case launches the kernel tests/conv_common.py claims for it (compared with the launches the library
really makes, logged by tests/hip_shim/launch_shim.c under tests/hip_shim/drive_conv.py: a threshold that moves in choose_tile,
wino_variant, the narrow / halo16 applicability tests or the weight-gradient tile switch fails here instead of silently losing
coverage), the packed entries launch what the unpacked ones do, every kernel of the code objects of csrc/conv_*.hip is launched
by a case a GPU test compares with a reference or is listed as unreachable, and the reference is the oracle's convolution."""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import nets
from tests import conv_common as cc

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import isa_tools                                                               # noqa: E402
from tests.test_launch_plan_cpu import GEOMETRIES                              # noqa: E402

CSRC = os.path.join(HERE, "..", "style-restricted_gan_amd", "csrc")


@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__
    __graft_entry__.build()
    from srgan_amd import _lib
    return _lib.LIB_PATH


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("conv_shim") / "launch_shim.so")
    subprocess.run(["gcc", "-shared", "-fPIC", "-O1", "-o", so, os.path.join(HERE, "hip_shim", "launch_shim.c")], check=True)
    return so


@pytest.fixture(scope="module")
def launches(lib_path, shim, tmp_path_factory):
    """{(case tag, mode, dispatch, entry): [kernel, ...]} of every case of every COVERAGE row, from one run of the driver."""
    cases = [c for _, cs, *_ in cc.COVERAGE for c in cs]
    return cc.drive(lib_path, shim, cases, str(tmp_path_factory.mktemp("conv_launches")))


@pytest.fixture(scope="module")
def conv_kernels(lib_path):
    """Kernel symbols of the code objects built from csrc/conv_*.hip: a code object belongs to them when it holds a kernel that
    one of those sources defines (kernels instantiated from pack_device.h come along with the object that uses them)."""
    defined = set()
    for f in sorted(os.listdir(CSRC)):
        if re.fullmatch(r"conv_\w+\.hip", f):
            defined |= set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", open(os.path.join(CSRC, f)).read()))
    assert len(defined) >= 40, sorted(defined)
    objects = {}
    for k in isa_tools.kernel_descriptors(lib_path):
        objects.setdefault(k["object"], set()).add(cc.kernel_name(k["name"]))
    out = set()
    for names in objects.values():
        if any(n.split("<")[0] in defined for n in names):
            out |= names
    return out


def covered(launches):
    """{kernel: first (test, launch mark) that covers it} over the COVERAGE rows."""
    out = {}
    for test, cases, modes, dispatches, entries in cc.COVERAGE:
        marks = [("-", "m0", "default", e) for e in entries] if not cases else \
            [k for c in cases for m in modes for d in dispatches for k in cc.covered_entries(launches, c, m, d, entries)]
        assert marks, test
        for k in marks:
            for kern in launches[k]:
                out.setdefault(kern, (test, k))
    return out


def test_tables_are_what_the_tests_take():
    assert set(cc.CLAIMS) == set(cc.CONV_CASES) and len(set(cc.CONV_CASES)) == len(cc.CONV_CASES)
    assert cc.RANDOM_CASES == cc._random_conv_cases(48, 20260410) and cc.RANDOM_BF16_CASES == cc._random_bf16_conv_cases(32, 20261004)
    assert len(cc.BF16_MODE_CASES) >= 20
    for case in cc.CONV_CASES:
        want = {"fp32/default", "fp32/forced"} | ({"bf16/default"} if case in cc.BF16_MODE_CASES else set())
        assert set(cc.CLAIMS[case]) == want, case
    for case, want in cc.KERNEL_CASES:       # every tensor of the new GPU cases at or below 16M elements
        n, i, h, w, o, k, s, p = case[:8]
        ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        assert max(n * i * h * w, n * o * ho * wo, o * i * k * k) <= 16 << 20, case
        assert want and set(want) <= {"fp32", "bf16"}


_MODE = {"fp32": "m0", "bf16": "m1"}


@pytest.mark.parametrize("case", cc.CONV_CASES, ids=cc.tag)
def test_hand_picked_case_launches_what_it_claims(case, launches):
    for combo, kernels in cc.CLAIMS[case].items():
        mode, dispatch = combo.split("/")
        got = tuple(cc.main_kernel(launches[(cc.tag(case), _MODE[mode], dispatch, e)]) for e in cc.UNPACKED)
        assert got == tuple(kernels), (combo, got)


@pytest.mark.parametrize("case,want", cc.KERNEL_CASES, ids=[cc.tag(c) for c, _ in cc.KERNEL_CASES])
def test_kernel_case_launches_what_it_claims(case, want, launches):
    for mode, dirs in want.items():
        for direction, kernel in dirs.items():
            for entry in (direction, {"fwd": "fwd_packed", "dgrad": "dgrad_packed", "wgrad": "wgrad"}[direction]):
                ls = launches[(cc.tag(case), _MODE[mode], "default", entry)]
                assert cc.main_kernel(ls) == kernel, (mode, entry, ls)


def test_bf16_mode_rounds_the_operands_of_vector_gathers_only(launches):
    """The rule the references of test_conv_kernels_gpu.py follow in the bf16 mode: BF16 of igemm_kernel<BM, BN, WM, WN, VEC, BF16>
    and of wgrad_kernel<BMc, BNn, WM, WN, VEC, ROWS, BF16, IO16> is set exactly when the direction's reduce channels are a
    multiple of 32 (or the layer runs on igemm16_kernel, bf16 by construction)."""
    n = 0
    for case, want in cc.KERNEL_CASES:
        if "bf16" not in want:
            continue
        i, o = case[1], case[4]
        for entry, rule, flag in (("fwd", i % 32 == 0, 5), ("dgrad", o % 32 == 0, 5), ("wgrad", i % 32 == 0, 6),
                                  ("fwd_packed", i % 32 == 0, 5), ("dgrad_packed", o % 32 == 0, 5)):
            k = cc.main_kernel(launches[(cc.tag(case), "m1", "default", entry)])
            name, args = k.split("<")[0], k.split("<")[1].rstrip(">").split(",")
            assert name in ("igemm_kernel", "wgrad_kernel", "igemm16_kernel"), (case, entry, k)
            assert (name == "igemm16_kernel" or args[flag] == "true") == rule, (case, entry, k)
            n += 1
    assert n >= 40


def test_masked_and_io_cases_launch_what_they_claim(launches):
    for case, kernel in cc.MASK_CASES:
        assert launches[(cc.tag(case), "m0", "forced", "dgrad_packed_mask")] == [kernel]
    for case, kernel in cc.HALO16_IO_CASES:
        for kind in (0, 1):
            assert launches[(cc.tag(case), "m1", "default", f"halo16_conv:kind{kind}:in16=1:out16=0")] == [kernel]
    t = cc.tag(cc.S2_IO_CASE)
    for a in (0, 1):
        for b in (0, 1):
            ab = ",".join("true" if v else "false" for v in (a, b))
            assert launches[(t, "m1", "default", f"halo16_conv:kind0:in16={a}:out16={b}")] == [f"halo16s_kernel<128,256,{ab}>"]
            assert launches[(t, "m1", "default", f"halo16_conv:kind1:in16={a}:out16={b}")] == [f"halo16t_kernel<256,128,{ab}>"]
            assert cc.main_kernel(launches[(t, "m1", "default", f"halo16_wgrad:x16={a}:d16={b}")]) == f"halo16s2_wgrad_kernel<32,{ab}>"


def test_packed_entries_launch_what_the_unpacked_ones_do(launches):
    """include/srgan_hip.h: "srgan_conv2d_fwd / _dgrad are exactly pack-into-workspace + the packed call" -- for every case, both
    compute modes, both dispatch settings.  The epilogue variants of the packed input gradient launch the same kernels, or the
    masked / adding instantiation of the same kernel, or one elementwise pass more."""
    n = 0
    for key, ls in launches.items():
        base = key[:3]
        if key[3] == "fwd":
            assert launches[base + ("pack0",)] + launches[base + ("fwd_packed",)] == ls, key
            n += 1
        if key[3] == "dgrad":
            packed = launches[base + ("dgrad_packed",)]
            assert launches[base + ("pack1",)] + packed == ls, key
            for variant, extra in (("dgrad_packed_add", "add_inplace_kernel"), ("dgrad_packed_mask", "act_bwd_kernel")):
                got = launches[base + (variant,)]
                if got and got[-1] == extra:
                    assert got[:-1] == packed, (key, variant)
                else:       # in the kernel's own epilogue
                    assert [re.sub(r"<.*", "", k) for k in got] == [re.sub(r"<.*", "", k) for k in packed], (key, variant)
            n += 1
    assert n >= 4 * 2 * 200


def test_every_conv_kernel_is_covered_dead_or_deferred(launches, conv_kernels):
    """The ledger: every kernel symbol of the convolution code objects is in exactly one of three groups."""
    assert len(conv_kernels) >= 200
    cov = covered(launches)
    dead, deferred = [k for k, _, _ in cc.DEAD], [k for k, _, _ in cc.DEFERRED]
    assert len(set(dead)) == len(dead) and len(set(deferred)) == len(deferred) and not set(dead) & set(deferred)
    assert set(dead) | set(deferred) <= conv_kernels, sorted((set(dead) | set(deferred)) - conv_kernels)
    assert not set(cov) & (set(dead) | set(deferred)), sorted(set(cov) & (set(dead) | set(deferred)))
    missing = sorted(conv_kernels - set(cov) - set(dead) - set(deferred))
    assert not missing, missing
    # a DEAD entry quotes the dispatch condition from the source it names
    src = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith(".hip")}
    for kernel, quotes, why in cc.DEAD:
        assert quotes and why, kernel
        for q in quotes:
            assert any(q in s for s in src.values()), (kernel, q)
    # nothing no descriptor launches hides behind an entry the driver does not know: whatever any entry launched is a conv
    # kernel or the pointwise activation backward behind srgan_conv2d_dgrad_packed_mask
    launched = {k for ls in launches.values() for k in ls}
    assert launched - conv_kernels <= {"act_bwd_kernel"}, sorted(launched - conv_kernels)


def test_deferred_stays_small():
    for kernel, shape, why in cc.DEFERRED:
        assert not re.match(r"(igemm_kernel|wgrad_kernel|narrow_|wino|rgb)", kernel), kernel
        assert shape and why
    assert len(cc.DEFERRED) <= 4


@pytest.mark.parametrize("name,H,B,ncls", GEOMETRIES)
def test_benchmark_geometry_is_fully_covered(name, H, B, ncls, lib_path, shim, launches, conv_kernels, tmp_path):
    """No kernel any entry of drive_launches.py launches at a benchmark geometry is DEAD or DEFERRED -- so each is launched by a
    case that a GPU test compares with the reference (the ledger above)."""
    log = str(tmp_path / "launches.log")
    env = dict(os.environ, LD_PRELOAD=shim + (":" + os.environ["LD_PRELOAD"] if os.environ.get("LD_PRELOAD") else ""), SRGAN_SHIM_LOG=log)
    env.pop("SRGAN_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "hip_shim", "drive_launches.py"), lib_path, str(H), str(B), str(ncls)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    used = {cc.kernel_name(ln.split()[0]) for ln in open(log) if not ln.startswith("#")}
    assert len(used) >= 40
    off = {k for k, _, _ in cc.DEAD} | {k for k, _, _ in cc.DEFERRED}
    assert not used & off, sorted(used & off)
    cov = covered(launches)
    uncovered = sorted((used & conv_kernels) - set(cov))
    assert not uncovered, uncovered
    if name in ("c3_128_b64", "c4_256_b16"):      # E.l0.shortcut forward on the 8-wave 256x128 tile
        assert "igemm_kernel<256,128,4,2,true,false>" in used
    if name == "c3_128_b64":                      # its input gradient; D0.last / D0.cls input gradient at N = 128
        assert {"igemm_kernel<256,64,4,2,true,false>", "igemm_kernel<128,128,2,2,false,false>"} <= used


def test_the_three_benchmark_kernels_are_launched_by_a_case_of_the_kernel_tests(launches):
    """igemm_kernel<128,128,2,2,false,false> (D0.last / D0.cls input gradient), <256,128,4,2,true,false> (E.l0.shortcut forward) and
    <256,64,4,2,true,false> (its input gradient) at c3_128_b64 (asserted above): no case of test_ops_gpu.py launches them,
    KERNEL_CASES do."""
    cov = covered(launches)
    for k in ("igemm_kernel<128,128,2,2,false,false>", "igemm_kernel<256,128,4,2,true,false>", "igemm_kernel<256,64,4,2,true,false>"):
        assert cov[k][0].startswith("test_conv_kernels_gpu::"), (k, cov[k])


def test_reference_is_the_convolution_of_the_oracle():
    for case in ((2, 5, 9, 11, 7, 3, 1, 1, True, False), (2, 5, 9, 11, 7, 3, 1, 1, False, True), (2, 6, 10, 9, 4, 4, 2, 1, False, False)):
        x, w, b, gy = (t.double() if t is not None else None for t in cc.inputs(case))
        n, i, h, ww, o, k, s, p, reflect, _ = case
        y, dx, dw, db = cc.reference(case, x, w, b, gy)
        if reflect:
            assert cc.rel_err(y, nets._conv3_reflect(x, w)) <= 1e-12
            assert cc.rel_err(y, F.conv2d(F.pad(x, (p, p, p, p), mode="reflect"), w, b, s)) <= 1e-12
        else:
            assert cc.rel_err(y, F.conv2d(x, w, b, s, p)) <= 1e-12
        if (k, s, p, b) == (4, 2, 1, None):       # zero padding: the first layer of the oracle's discriminator trunk (conv + LeakyReLU)
            assert cc.rel_err(F.leaky_relu(y, nets.D_SLOPE), nets._trunk({"d.down_convs.0.weight": w}, "d", x)[0]) <= 1e-12
        # the gradients are those of the same expression, by hand: dw[o,i,ky,kx] = sum dy[n,o,y,x] * xpad[n,i,s y + ky,s x + kx]
        xp = F.pad(x, (p, p, p, p), mode="reflect" if reflect else "constant")
        cols = F.unfold(xp, k, stride=s)                                           # [n, i k k, L]
        dw_hand = torch.einsum("nol,nkl->ok", gy.flatten(2), cols).view(o, i, k, k)
        assert cc.rel_err(dw, dw_hand) <= 1e-12
        if b is not None:
            assert cc.rel_err(db, gy.sum((0, 2, 3))) <= 1e-12
        assert cc.rel_err(dx, torch.autograd.functional.vjp(lambda t: cc.conv_ref(t, w, b, s, p, reflect), x, gy)[1]) <= 1e-12
    # the reference works on copies in either type: the inputs stay leaves outside any graph (a test moves them to the GPU after it)
    x, w, b, gy = cc.inputs((2, 5, 9, 11, 7, 3, 1, 1, False, True))
    for dtype in (torch.float32, torch.float64):
        cc.reference((2, 5, 9, 11, 7, 3, 1, 1, False, True), x, w, b, gy, dtype)
        assert not any(t.requires_grad or t.grad is not None for t in (x, w, b, gy))
    # the bf16-mode variant rounds the two operands of each product and nothing else
    case = (2, 32, 6, 7, 32, 3, 1, 1, False, True)
    x, w, b, gy = cc.inputs(case)
    r = cc.bf16_round
    y, dx, dw, db = cc.reference(case, x, w, b, gy, bf16=True)
    assert cc.rel_err(y, F.conv2d(r(x).double(), r(w).double(), b.double(), 1, 1)) <= 1e-12
    assert cc.rel_err(dx, F.conv_transpose2d(r(gy).double(), r(w).double(), None, 1, 1)) <= 1e-12
    assert cc.rel_err(dw, cc.reference(case, r(x), w, b, r(gy))[2]) <= 1e-12 and cc.rel_err(db, gy.double().sum((0, 2, 3))) <= 1e-12
    assert float((r(x) - x).abs().max()) > 0 and float((r(r(x)) - r(x)).abs().max()) == 0


def test_error_check_holds_and_refuses():
    ref = torch.linspace(-1, 1, 101, dtype=torch.float64)
    ref32 = ref.float()
    cc.check("self", "y", ref + 1.9e-5, ref, ref32)
    cc.check("self", "dw", ref + 4.9e-5, ref, ref32)
    assert cc.bf16_store(ref) == 2.0 ** -8 and cc.bf16_store(ref * 1.999) == 2.0 ** -8 / 1.999      # max |ref| = 1: bottom of its binade
    cc.check("self", "y", ref + 3.9e-3, ref, ref32, stored_bf16=True)
    for what, off in (("y", 2.2e-5), ("dx", 2.2e-5), ("dw", 5.2e-5), ("db", 5.2e-5)):
        with pytest.raises(AssertionError):
            cc.check("self", what, ref + off, ref, ref32)
    with pytest.raises(AssertionError):
        cc.check("self", "y", ref + 4.0e-3, ref, ref32, stored_bf16=True)
    # a long sum whose float32 evaluation is itself 1e-5 off widens the bound to 8 e32 and no further
    cc.check("self", "dw", ref + 7e-5, ref, ref + 1e-5)
    with pytest.raises(AssertionError):
        cc.check("self", "dw", ref + 9e-5, ref, ref + 1e-5)
    del cc.FIGURES[:]
