"""CPU: the yardsticks of tests/test_trunk_kernels_gpu.py are pinned here, without a GPU -- the library admits every case (its
pure host functions, called through ctypes with the dispatch thresholds off, agree with the restatement in
tests/trunk_common.py: applicability, V / Z image sizes, the split geometry of the weight gradient), the case list reaches what
each case is there for, the activation-kink window zeroes at most 1 % of any upstream gradient, the hostile inputs are within
reach of float32, an image one byte short is an argument error, and the reference is the composition of oracle/nets.py."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import nets
from tests import conv_common as cc
from tests import norm_common as nc
from tests import trunk_common as tc

ALL_NIO = sorted({c["nio"] for c in tc.FWD_CASES + tc.BWD_CASES} | {nio for pair in tc.HOSTILE_SHAPES.values() for nio in pair})


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from srgan_amd import _lib
    os.environ["SRGAN_WINOGRAD_THRESHOLD_SCALE"] = "0"          # read per call: the small batches take F(4x4,3x3)
    try:
        yield _lib
    finally:
        os.environ.pop("SRGAN_WINOGRAD_THRESHOLD_SCALE", None)


def _desc(_lib, N, I, O):
    return _lib.ConvDesc(N, tc.HW, tc.HW, I, tc.HW, tc.HW, O, 3, 3, 1, 1, 0, I * 9, 9, 3, 1)


def _host(_lib, N, I, O):
    """What the library's host functions say about the layer."""
    L, d = _lib.load(), ctypes.byref(_desc(_lib, N, I, O))
    return dict(conv_v=L.srgan_instnorm_conv_v_applicable(d), bwd_vz=L.srgan_instnorm_bwd_vz_applicable(d),
                wgrad_v=L.srgan_conv2d_wgrad_v_bytes(d), z=L.srgan_instnorm_bwd_vz_z_bytes(d),
                scratch0=L.srgan_conv2d_packed_scratch(d, 0), scratch1=L.srgan_conv2d_packed_scratch(d, 1))


def _restated(N, I, O):
    g = tc.wgrad_geometry(N, I, O)
    return dict(conv_v=int(tc.conv_v_applicable(N, I, O)), bwd_vz=int(tc.bwd_vz_applicable(N, I, O)), wgrad_v=tc.wgrad_v_bytes(N, I, O),
                z=g["z_bytes"] if g else 0, scratch0=tc.packed_scratch(N, I, O, 0), scratch1=tc.packed_scratch(N, I, O, 1))


@pytest.mark.parametrize("nio", ALL_NIO, ids=tc.run_id)
def test_library_admits_the_case_and_states_the_restated_sizes(nio, lib):
    N, I, O = nio
    got, want = _host(lib, N, I, O), _restated(N, I, O)
    assert got == want, (got, want)
    assert got["scratch0"] == tc.wino43_scratch_floats(N * 64, I) * 4 and got["scratch1"] == tc.wino43_scratch_floats(N * 64, O) * 4
    if nio in [c["nio"] for c in tc.FWD_CASES] + [f for f, _ in tc.HOSTILE_SHAPES.values()]:
        assert got["conv_v"] == 1
    if nio in [c["nio"] for c in tc.BWD_CASES] + [b for _, b in tc.HOSTILE_SHAPES.values()]:
        assert got["bwd_vz"] == 1 and got["wgrad_v"] == got["scratch0"] != 0
        assert got["z"] == (O // 32) * 8 * N * 36 * 256 * 4
    # every tensor of the case at or below 2 M elements
    assert max(N * I * tc.HW * tc.HW, N * O * tc.HW * tc.HW, O * I * 9) <= tc.MAX_ELEMS


def test_restatement_follows_the_library_beyond_the_cases(lib):
    """The same comparison over a grid that includes layers the entries refuse: the restated conditions are the library's."""
    n = 0
    for N in (1, 3, 8, 11):
        for I in (32, 48, 64, 96, 128):
            for O in (32, 40, 64, 96):
                if not (tc.f43(N, I, O) and tc.f43(N, O, I)):       # packed_scratch is restated for F(4x4,3x3) layers only
                    h = _host(lib, N, I, O)
                    assert h["conv_v"] == int(tc.conv_v_applicable(N, I, O)) and h["bwd_vz"] == int(tc.bwd_vz_applicable(N, I, O))
                    continue
                assert _host(lib, N, I, O) == _restated(N, I, O), (N, I, O)
                n += 1
    assert n >= 40


def test_cases_reach_what_they_are_there_for(lib):
    h = _host(lib, 3, 96, 64)
    assert h["wgrad_v"] == 0 and h["conv_v"] == 1 and h["bwd_vz"] == 0       # no kept V image: the recompute branch of _NormActConvFn
    for c in tc.BWD_CASES:
        g = tc.wgrad_geometry(*c["nio"])
        assert (g["ntc"], g["splits"], g["cps"], g["bumped"]) == tc.BWD_GEOMETRY[c["nio"]], (c["nio"], g)
        assert g["ntc"] - (g["splits"] - 1) * g["cps"] >= 2
    assert tc.BWD_GEOMETRY[(1, 64, 32)] == (8, 4, 2, False) and tc.BWD_GEOMETRY[tc.BUMP_CASE] == (88, 22, 4, True)
    assert -(-88 // 32) == 3 and 88 % 3 == 1                                  # cps 3 -> 4
    bump = [(N, I, O) for I, O in tc.BUMP_PAIRS for N in range(1, 17) if (tc.wgrad_geometry(N, I, O) or {}).get("bumped")]
    assert bump == [tc.BUMP_CASE]
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "style-restricted_gan_amd", "csrc", "conv_wino.hip")).read()
    assert "if (ntc % cps == 1) ++cps;" in src
    fwd, bwd = [c["nio"] for c in tc.FWD_CASES], [c["nio"] for c in tc.BWD_CASES]
    assert fwd == [(1, 32, 32), (3, 96, 64), (8, 64, 32), (16, 128, 96), (5, 256, 256)]
    assert bwd == [(1, 64, 32), (2, 64, 128), (2, 128, 64), (8, 64, 64), (11, 128, 128), (5, 256, 256)]
    assert any(N % 8 == 0 and N > 8 for N, _, _ in fwd) and any(I != O for _, I, O in bwd) and any(I % 64 for _, I, _ in fwd)
    # the full grid on the two smallest cases of each direction, two combinations on each of the others, all six among them
    every = {(a, b) for a in (tc.ACT_NONE, tc.ACT_RELU, tc.ACT_LRELU) for b in (True, False)}
    for cases in (tc.FWD_CASES, tc.BWD_CASES):
        assert [c["grid"] for c in cases[:2]] == ["full", "full"] and all(set(tc.combos(c)) == every for c in cases[:2])
        rest = [tc.combos(c) for c in cases[2:]]
        assert all(len(r) == 2 for r in rest) and {ab for r in rest for ab in r} == every
    assert {e for *_, e in tc.EPILOGUE_CASES} == {tc.ACT_RELU, tc.ACT_LRELU}
    assert tc.wgrad_v_bytes(*tc.V_FROM_NORM_CASE[0]) and tc.conv_v_applicable(*tc.V_FROM_NORM_CASE[0])
    assert tc.L == 24 and set(tc.HOSTILE_INPUTS) == set(nc.HOSTILE_INPUTS) | {tc.NEAR_EPS}
    assert sorted(cc.TRUNK_CASES) == ALL_NIO                                  # the ledger row of tests/conv_common.py drives these
    for shape, (f, b) in tc.HOSTILE_SHAPES.items():
        assert (f[0], f[1]) == shape[:2] and (b[0], b[2]) == shape[:2]


def test_an_image_one_byte_short_is_an_argument_error(lib):
    """Before any launch: the entries return non-zero and name the size function (no device is touched on the way)."""
    L = lib.load()
    p = ctypes.c_void_p(0x7000_0000_0000)                       # never dereferenced on the host
    N, I, O = 2, 64, 128
    d = ctypes.byref(_desc(lib, N, I, O))
    v0, v1, z = tc.packed_scratch(N, I, O, 0), tc.packed_scratch(N, I, O, 1), tc.z_bytes(N, O)
    assert L.srgan_instnorm_fwd_v(d, p, p, p, p, p, p, v0 - 1, 1e-5, 1, 0.0, None) < 0
    assert b"srgan_conv2d_packed_scratch" in L.srgan_last_error()
    assert L.srgan_instnorm_bwd_vz(d, p, p, p, p, p, p, p, p, p, v1 - 1, p, z, 1, 0.0, None) < 0
    assert b"srgan_conv2d_packed_scratch(d, 1)" in L.srgan_last_error()
    assert L.srgan_instnorm_bwd_vz(d, p, p, p, p, p, p, p, p, p, v1, p, z - 1, 1, 0.0, None) < 0
    assert b"srgan_instnorm_bwd_vz_z_bytes" in L.srgan_last_error()


@pytest.mark.parametrize("nio,act,affine", [r for r in tc.runs(tc.BWD_CASES) if r[1] != tc.ACT_NONE], ids=tc.run_id)
def test_kink_window_zeroes_at_most_one_percent(nio, act, affine):
    """From the float64 reference alone: tau is about 1.6e-3 and the share about 0.1 % at L = 24."""
    N, _, O = nio
    y = tc.norm_input((N, O, tc.HW, tc.HW))
    scale, shift = tc.affine_params(N, O, affine)
    gup = tc.masked_upstream(y, scale, shift, act)
    share = float((gup == 0).double().mean())
    assert 0 < share <= nc.KINK_SHARE_MAX, share


@pytest.mark.parametrize("shape,kind", tc.HOSTILE_CASES, ids=nc.hostile_id)
def test_hostile_inputs_are_within_reach_of_float32(shape, kind):
    """e32 of every result the GPU test holds on this input -- the forward with each activation, the backward without one -- is
    finite and below the project's 1e-3 parity contract; the near-eps input really is decided by eps."""
    fwd, bwd = tc.HOSTILE_SHAPES[shape]
    for act in tc.HOSTILE_FWD_ACTS:
        _, r64, r32 = tc.forward_yardstick(fwd, act, True, kind=kind)
        for a, b in zip(r32, r64):
            assert nc.rel_err(a, b) < 1e-3, (kind, act)
    _, r64, r32 = tc.backward_yardstick(bwd, tc.ACT_NONE, True, kind=kind)
    for k in r64:
        assert nc.rel_err(r32[k], r64[k]) < 1e-3, (kind, k)
    if kind == tc.NEAR_EPS:
        x = tc.norm_input(shape, kind).double()
        var = x.var(dim=(2, 3), unbiased=False)
        assert 0.5 * tc.EPS < float(var.min()) and float(var.max()) < 2 * tc.EPS
        ratio = torch.sqrt(var / (var + tc.EPS))                 # rstd with eps over rstd without
        assert float(ratio.max()) < 0.8


def test_reference_is_the_composition_of_the_oracle():
    """conv3x3(relu(cbin(x))) as oracle/nets.py's generator writes its residual block (CBIN = the norm with cbin_ref's scale and
    shift), the plain instance norm, and the gradients as autograd of that expression."""
    N, I, O = 2, 6, 5
    x = nc.default_input((N, I, 9, 11)).double()
    w = (nc.rnd(O, I, 3, 3, seed=2) / 7).double()
    c = nc.rnd(N, 12, seed=1).double()
    W, b, gam, bet = (t.double() for t in nc.cbin_params(I, 12, 10))
    P = {"n.ConBias.0.weight": W, "n.ConBias.0.bias": b, "n.weight": gam, "n.bias": bet}
    cs, ch = nc.cbin_ref(c, W, b, gam, bet)
    y, mean, rstd = tc.forward_ref(x, cs, ch, w, None, tc.ACT_RELU, tc.ACT_NONE, torch.float64)
    assert nc.rel_err(y, F.conv2d(torch.relu(nets.cbin(x, c, P, "n")), w, None, 1, 1)) <= 1e-12
    y0, _, _ = tc.forward_ref(x, None, None, w, None, tc.ACT_NONE, tc.ACT_NONE, torch.float64)
    assert nc.rel_err(y0, F.conv2d(nets.inorm(x), w, None, 1, 1)) <= 1e-12
    m, v = nets._plane_stats(x)
    assert nc.rel_err(mean, m.flatten()) <= 1e-12 and nc.rel_err(rstd, (1 / torch.sqrt(v + nets.EPS)).flatten()) <= 1e-12
    bias = nc.rnd(O, seed=3).double()
    ye, _, _ = tc.forward_ref(x, cs, ch, w, bias, tc.ACT_RELU, tc.ACT_LRELU, torch.float64)
    assert nc.rel_err(ye, F.leaky_relu(F.conv2d(torch.relu(nets.cbin(x, c, P, "n")), w, bias, 1, 1), tc.SLOPE)) <= 1e-12
    # backward: the norm runs over the convolution's OUTPUT; the gradients are those of the oracle's expression by autograd, with
    # the gradient w.r.t. the norm's input handed to the convolution (backward_ref's formulas do not depend on the map size)
    yn = nc.default_input((N, O, 9, 11)).double()
    gup, xc = nc.upstream((N, O, 9, 11)).double(), nc.rnd(N, I, 9, 11, seed=6).double()
    W2, b2, gam2, bet2 = (t.double() for t in nc.cbin_params(O, 12, 20))
    P2 = {"n.ConBias.0.weight": W2, "n.ConBias.0.bias": b2, "n.weight": gam2, "n.bias": bet2}
    s2, h2 = nc.cbin_ref(c, W2, b2, gam2, bet2)
    yv = yn.clone().requires_grad_(True)
    dy, = torch.autograd.grad(torch.relu(nets.cbin(yv, c, P2, "n")), yv, gup)
    xv, wv = xc.clone().requires_grad_(True), w.clone().requires_grad_(True)
    dx, dw = torch.autograd.grad(F.conv2d(xv, wv, None, 1, 1), [xv, wv], dy)
    r = tc.backward_ref(yn, gup, s2, h2, w, xc, tc.ACT_RELU, torch.float64)
    assert nc.rel_err(r["dy"], dy) <= 1e-12 and nc.rel_err(r["dx"], dx) <= 1e-12 and nc.rel_err(r["dw"], dw) <= 1e-12
    xh = nets.inorm(yn)
    on = (xh * s2[:, :, None, None] + h2[:, :, None, None]) > 0
    assert nc.rel_err(r["dshift"], (gup * on).sum((2, 3))) <= 1e-12 and nc.rel_err(r["dscale"], (gup * on * xh).sum((2, 3))) <= 1e-12
    # without affine parameters the two sums are those at scale = 1, shift = 0, and dy is the plain norm's
    r0 = tc.backward_ref(yn, gup, None, None, w, xc, tc.ACT_LRELU, torch.float64)
    yv = yn.clone().requires_grad_(True)
    dy0, = torch.autograd.grad(F.leaky_relu(nets.inorm(yv), tc.SLOPE), yv, gup)
    m = torch.where(xh > 0, torch.ones_like(xh), torch.full_like(xh, tc.SLOPE))
    assert nc.rel_err(r0["dy"], dy0) <= 1e-12
    assert nc.rel_err(r0["dshift"], (gup * m).sum((2, 3))) <= 1e-12 and nc.rel_err(r0["dscale"], (gup * m * xh).sum((2, 3))) <= 1e-12
