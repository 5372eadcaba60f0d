"""CPU: the yardsticks of tests/test_norm_kernels_gpu.py are pinned here, without a GPU -- every shape case takes the kernel
path its entry in tests/norm_common.py claims (the restated dispatch is compared with the launches the library really makes,
logged by tests/hip_shim/launch_shim.c: a threshold that moves in csrc/norm.hip fails here instead of silently losing
coverage), the activation-kink window zeroes at most 1 % of any upstream gradient, the hostile inputs are well enough
conditioned for a float32 two-pass evaluation, and the references are the formulas of oracle/nets.py."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import nets
from tests import norm_common as nc

HERE = os.path.dirname(os.path.abspath(__file__))
ALL_CASES = [(c, None) for c in nc.FP32_CASES] + [(c, io) for c in nc.IO_CASES for io in nc.IO_PAIRINGS]


def _tag(case, io):
    return case["name"] + ("" if io is None else f"_x16={int(io[0])}_y16={int(io[1])}")


@pytest.fixture(scope="module")
def launches(tmp_path_factory):
    """{(tag, 'fwd' | 'bwd'): [(kernel, template arguments, grid)]} of every case, from one run of the driver under the shim."""
    import __graft_entry__
    __graft_entry__.build()
    from srgan_amd import _lib
    tmp = tmp_path_factory.mktemp("norm_shim")
    so, log = str(tmp / "launch_shim.so"), str(tmp / "launches.log")
    subprocess.run(["gcc", "-shared", "-fPIC", "-O1", "-o", so, os.path.join(HERE, "hip_shim", "launch_shim.c")], check=True)
    calls = [[_tag(c, io), c["shape"][0], c["shape"][2] * c["shape"][3], c["shape"][1], io and [int(io[0]), int(io[1])]]
             for c, io in ALL_CASES]
    env = dict(os.environ, LD_PRELOAD=so, SRGAN_SHIM_LOG=log)
    env.pop("SRGAN_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "hip_shim", "drive_norm.py"), _lib.LIB_PATH, json.dumps(calls)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out, where = {}, None
    for line in open(log):
        if line.startswith("#"):
            where = tuple(line[1:].split())
            out[where] = []
            continue
        mangled, gx, gy, gz = line.split()[:4]
        m = re.match(r"_ZN5srgan(\d+)", mangled)
        name, rest = mangled[m.end():m.end() + int(m.group(1))], mangled[m.end() + int(m.group(1)):]
        t = re.match(r"I((?:L[ib]\d+E)+)E", rest)
        targs = tuple(int(v) for v in re.findall(r"L[ib](\d+)E", t.group(1))) if t else ()
        out[where].append((name, targs, (int(gx), int(gy), int(gz))))
    return out


@pytest.mark.parametrize("case,io", ALL_CASES, ids=[_tag(c, io) for c, io in ALL_CASES])
def test_case_takes_the_path_it_claims(case, io, launches):
    f = nc.features(case["shape"], x16=io is not None)          # the 16-bit cases claim the route a bf16 input takes
    assert {k: f.get(k) for k in case["want"]} == case["want"], f
    if io is not None:
        N, C, H, W = case["shape"]
        assert nc.slab_fast(N, H * W, C) or (C % 4 == 0 and nc.pow2_fast(C, H * W))        # srgan_instnorm_io_applicable
    assert launches[(_tag(case, io), "fwd")] == nc.launch_plan(case["shape"], False, io)
    assert launches[(_tag(case, io), "bwd")] == nc.launch_plan(case["shape"], True, io)
    N, C, H, W = case["shape"]
    assert N * C * H * W <= 10_500_000


def test_case_list_covers_every_dispatch_path():
    fs = [nc.features(c["shape"]) for c in nc.FP32_CASES]
    slab = [f for f in fs if f["kind"] == "slab"]
    two = [f for f in fs if f["kind"] == "two-pass"]
    assert {f["R"] for f in slab} == {1, 2, 4, 8, 16}
    assert any(f["ragged"] and not f["remap"] for f in slab) and any(f["full"] for f in slab)
    assert {(f["stats"], f["finish"]) for f in two} == {("scalar", "apply1"), ("v4", "apply4"), ("v4", "pow2")}
    assert {(f["finish"], True) for f in two if f.get("capped")} == {("apply1", True), ("apply4", True)}
    for grid in ("cap", "capact"):      # both caps without and with an activation in the backward
        assert {nc.features(c["shape"])["finish"] for c in nc.FP32_CASES if c["grid"] == grid} == {"apply1", "apply4"}
    for c in nc.FP32_CASES:             # a folded case still meets every (affine, skip) combination
        if c["grid"] == "fold":
            assert {ab for act in (0, 1, 2) for ab in nc.param_grid(c, act)} == {(a, b) for a in (0, 1) for b in (0, 1)}
    assert any(f.get("apply_main_then_tail") for f in two) and any(f.get("one_block") or f.get("G") == 2 for f in two)
    assert any(f["empty_last_split"] for f in two) and any(f.get("stats_main_then_tail") for f in two)
    assert (127, 32, 8, 8) in [c["shape"] for c in nc.FP32_CASES] and not nc.slab_fast(127, 64, 32) and nc.slab_fast(128, 64, 32)
    io = [nc.features(c["shape"], x16=True) for c in nc.IO_CASES]
    assert {f["R8"] for f in io if f["kind"] == "slab"} == {1, 2, 4, 8}
    assert {f["stats"] for f in io if f["kind"] == "two-pass"} == {"v4", "v8"}
    assert set(nc.IO_PAIRINGS) == {(False, True), (True, False), (True, True)}


def _grid(case):
    """(affine, skip, activation) combinations whose backward passes through an activation."""
    if case["grid"] == "cap":
        return []
    acts = (nc.ACT_LRELU,) if case["grid"] == "capact" else (nc.ACT_RELU, nc.ACT_LRELU)
    return [(aff, res, act) for act in acts for aff, res in nc.param_grid(case, act)]


@pytest.mark.parametrize("case,io", ALL_CASES, ids=[_tag(c, io) for c, io in ALL_CASES])
def test_kink_window_zeroes_at_most_one_percent(case, io):
    """From the references alone.  With the well-conditioned default input the share is about 0.2 %."""
    shape = case["shape"]
    x = nc.default_input(shape)
    if io is not None:
        x = nc.bf16_round(x) if io[0] else x
        combos = [(aff, False, act) for aff, act in nc.IO_COMBOS if act != nc.ACT_NONE]
    else:
        combos = _grid(case)
    worst = 0.0
    for aff, res, act in combos:
        scale, shift, r = nc.case_params(shape, aff, res)
        keep = nc.kink_keep(x, scale, shift, r, act, nc.path_L(shape, *(io or (False, False))))
        worst = max(worst, 1.0 - float(keep.double().mean()))
    assert worst <= nc.KINK_SHARE_MAX, worst


@pytest.mark.parametrize("shape,kind", nc.HOSTILE_CASES, ids=nc.hostile_id)
def test_hostile_inputs_are_within_reach_of_float32(shape, kind):
    """e32 -- the float32 two-pass evaluation against float64 -- is finite and below the project's 1e-3 parity contract for the
    forward with each activation and for the gradients of the plain forward."""
    x = nc.HOSTILE_INPUTS[kind](shape)
    scale, shift, res = nc.case_params(shape, True, True)
    for act in (nc.ACT_NONE, nc.ACT_RELU, nc.ACT_LRELU):
        needs = (True, True, True, True) if act == nc.ACT_NONE else (False,) * 4
        r64, r32 = nc.yardstick(nc.norm_ref(act), (x, scale, shift, res), needs, nc.upstream(shape) if needs[0] else None)
        for a, b in zip(r32, r64):
            e32 = nc.rel_err(a, b)
            assert e32 < 1e-3, (kind, act, e32)


def test_references_are_the_formulas_of_the_oracle():
    shape = (3, 6, 9, 11)
    x = nc.default_input(shape).double()
    scale, shift, res = (t.double() for t in nc.case_params(shape, True, True))
    sc4, sh4 = scale[:, :, None, None], shift[:, :, None, None]
    assert nc.rel_err(nc.pre_activation(x, None, None), F.instance_norm(x, eps=nc.EPS)) <= 1e-12
    assert nc.rel_err(nc.pre_activation(x, None, None), nets.inorm(x)) <= 1e-12
    for act, fn in ((nc.ACT_NONE, lambda z: z), (nc.ACT_RELU, torch.relu), (nc.ACT_LRELU, lambda z: F.leaky_relu(z, nc.SLOPE))):
        want = fn(F.instance_norm(x, eps=nc.EPS) * sc4 + sh4) + res
        assert nc.rel_err(nc.norm_ref(act)(x, scale, shift, res), want) <= 1e-12
    # CBIN: (IN(x) + tanh(Linear(c))) * gamma + beta of oracle/nets.py = the norm with cbin_ref's scale and shift
    c = nc.rnd(3, 12, seed=1).double()
    W, b, gam, bet = (t.double() for t in nc.cbin_params(6, 12, 10))
    P = {"n.ConBias.0.weight": W, "n.ConBias.0.bias": b, "n.weight": gam, "n.bias": bet}
    cs, ch = nc.cbin_ref(c, W, b, gam, bet)
    assert nc.rel_err(nc.norm_ref(nc.ACT_NONE)(x, cs, ch, None), nets.cbin(x, c, P, "n")) <= 1e-12


def test_cbin_case_lists_reach_the_limits_of_the_kernels():
    """The CBIN cases are chosen against constants of csrc/norm.hip: 16 layers per pass of cbin_affine_multi_bwd_c, 16 style
    conditions at most, 64 lanes striding over the batch.  If one of them moves, the lists have to follow."""
    src = open(os.path.join(HERE, "..", "style-restricted_gan_amd", "csrc", "norm.hip")).read()
    assert "for (int l0 = 0; l0 < n_layers; l0 += 16)" in src and "__shared__ float part[16][16];" in src
    assert len(nc.CBIN_MULTI_WIDTHS) == 16 + 1
    assert src.count("num_con > 0 && num_con <= 16") == 4
    assert max(nc.CBIN_NUM_CON) == 16 and nc.CBIN_NUM_CON_REFUSED == 17
    assert src.count("for (int n = lane; n < N; n += 64)") == 2 and src.count("ch += 64)") == 2
    assert {64, 65} <= set(nc.CBIN_N) and max(nc.CBIN_N) > 128 and {64, 257} <= set(nc.CBIN_C)
