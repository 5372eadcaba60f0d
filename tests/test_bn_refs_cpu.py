"""CPU: the yardsticks of tests/test_bn_kernels_gpu.py are pinned here, without a GPU -- the restated slab plan sizes the
workspace and the exchange buffer exactly as the library does (a threshold that moves in csrc/norm_batch.hip fails here instead
of silently losing coverage), every shape case has the features its entry in tests/bn_common.py claims and the list as a whole
covers every feature value, the references are F.batch_norm in float64 (buffer update included), the activation-kink window
zeroes at most 1 % of any upstream gradient, and the hostile inputs are well conditioned for a float32 evaluation."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import bn_common as bn
from tests.syncbn_common import bn_plan

HERE = os.path.dirname(os.path.abspath(__file__))
CASE_IDS = [c["name"] for c in bn.CASES]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from srgan_amd import _lib
    return _lib


# ---- the restated plan against the library ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bn.CASES, ids=CASE_IDS)
def test_restated_plan_sizes_the_workspace(lib, case):
    """srgan_batchnorm_workspace = the [N][S][C] float2 partials + alpha, k [N][C] + delta [C]: S is observable through it."""
    N, C, H, W = case["shape"]
    S = bn.features(case["shape"])["S"]
    assert lib.load().srgan_batchnorm_workspace(N, H * W, C) - 4 * (2 * N * C + C) == N * S * C * 8
    assert N * C * H * W <= bn.MAX_ELEMENTS


@pytest.mark.parametrize("case", bn.SYNC_CASES, ids=bn.sync_id)
def test_exchange_buffer_follows_the_global_plan(lib, case):
    NG, NL, C, H, W = case
    S, _ = bn_plan(NG, H * W, C)
    L = lib.load()
    assert L.srgan_batchnorm_sync_exchange_bytes(NG, NL, H * W, C, 0) == NG * S * C * 8
    assert L.srgan_batchnorm_sync_exchange_bytes(NG, NL, H * W, C, 1) == NG * S * C * 8 + NG * C * 4
    assert L.srgan_batchnorm_sync_workspace(NL, C) == 4 * (2 * NL * C + C)
    assert NG % NL == 0 and NG * C * H * W <= bn.MAX_ELEMENTS


def test_sync_cases_reach_what_they_are_there_for():
    NG, NL, C, H, W = bn.SYNC_PLANS_DIFFER
    assert bn.SYNC_PLANS_DIFFER in bn.SYNC_CASES and bn_plan(NG, H * W, C) == (8, 128) and bn_plan(NL, H * W, C) == (16, 64)
    # at 64 channels and 32 x 32 pixels both plans stop at the 64-row floor (S = 16), whatever the batch
    assert bn_plan(8, 32 * 32, 64) == bn_plan(4, 32 * 32, 64) == (16, 64)
    assert any(ng == nl for ng, nl, *_ in bn.SYNC_CASES) and any(ng // nl == 10 and c % 32 for ng, nl, c, _, _ in bn.SYNC_CASES)
    assert any(ng > 128 and nl > 64 for ng, nl, *_ in bn.SYNC_CASES)          # a rank's own images take two lane trips
    lanes = [nl * c // 4 for _, nl, c, _, _ in bn.SYNC_CASES]                  # bn_sync_pack_scale: one float4 per lane
    assert any(n > 256 and n % 256 for n in lanes)
    kinds = {(v[0], v[1]) for v in bn.SYNC_VARIANTS}
    assert kinds == {(cbb, mode) for cbb in (False, True) for mode in ("tracked", "cumulative", "untracked")}
    assert {v[3] for v in bn.SYNC_VARIANTS} == set(bn.ACTS)


def test_stream_grid_constants():
    """Three grids by hand: 2304 float4 per image over 1024 images -> 2048 / 1024 = 2 workgroups of 256 lanes; 2049 images ->
    2048 / 2049 = 0, raised to 1; 25600 float4 over 32 images -> min(100, 64)."""
    assert bn.stream_grid(1024, 48 * 48 * 4) == 2
    assert bn.stream_grid(2049, 2 * 2 * 4) == 1
    assert bn.stream_grid(32, 20 * 20 * 256) == 64
    assert bn.stream_grid(1, 5 * 7 * 4) == 1 and bn.stream_grid(1, 82 * 100 * 4) == 33


def test_restatement_quotes_the_source():
    """The loops the case list is chosen against, as csrc/norm_batch.hip spells them.  If one of them moves, bn_common has to
    follow (stream_grid's constants show in no size the ABI reports, so the text is the only place they can be pinned)."""
    src = open(os.path.join(HERE, "..", "style-restricted_gan_amd", "csrc", "norm_batch.hip")).read()
    assert "while (blocks * S < 1024 && HW / (S * 2) >= 64) S *= 2;" in src and "constexpr int BN_CH = 32;" in src
    assert "const long long per_image = ceil_div(HWC / 4, 256);" in src and "const long long want = std::max(1, 2048 / N);" in src
    assert src.count("j += gridDim.x * blockDim.x * 4") == 2
    assert src.count("for (int n = lane; n < N; n += 64)") == 2 and src.count("for (int n = lane; n < Nl; n += 64)") == 2
    assert "for (; r + 96 < r1; r += 128)" in src and src.count("r += 32)") == 2
    assert src.count("for (int o = 32; o > 0; o >>= 1)") == 2 and src.count("for (int i = 0; i < 32; ++i)") == 2


# ---- features --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bn.CASES, ids=CASE_IDS)
def test_case_has_the_features_it_claims(case):
    f = bn.features(case["shape"])
    assert {k: f.get(k) for k in case["want"]} == case["want"], f
    n, c, h, w = case["shape"]
    assert case["grid"] == ("fold" if n * c * h * w > bn.FOLD_ABOVE else "full") and c % 4 == 0


def test_case_list_covers_every_feature():
    fs = [bn.features(c["shape"]) for c in bn.CASES]
    assert {1, 2, 4, 8, 32, 128} <= {f["S"] for f in fs}
    single = [f for f in fs if f["S"] == 1]
    assert any(f["rps"] >= 2304 and f["rows"] >= 8 for f in single)             # several rounds of the unrolled loop in one thread
    assert any(f["stats_main_then_tail"] for f in single) and any(f["idle_rows"] for f in single)
    assert any(f["ragged_rps"] for f in fs) and any(f["empty_last_slab"] for f in fs)
    assert any(f["stats_main"] and f["stats_tail"] and not f["stats_main_then_tail"] for f in fs)      # the loop in some lanes only
    assert any(f["stats_main"] and not f["stats_tail"] for f in fs) and any(f["stats_tail"] and not f["stats_main"] for f in fs)
    assert any(f["channel_tail"] and f["channel_blocks"] > 1 for f in fs) and any(f["channel_blocks"] >= 8 for f in fs)
    assert {1, 2, 3} <= {f["lane_trips"] for f in fs} and max(f["lane_trips"] for f in fs) >= 16
    shapes = [c["shape"][0] for c in bn.CASES]
    assert 64 in shapes and 65 in shapes                                        # the last image of the first trip, the first of the second
    assert any(f["lane_trips"] == 3 and f["channel_tail"] for f in fs)
    # the streaming passes: N > 2048, several trips with a ragged last one, a single partial workgroup, a full single trip
    assert any(f["block_per_image"] for f in fs)
    assert any(f["apply_trips"] >= 5 and f["apply_ragged"] and f["G"] == 2 for f in fs)
    assert any(f["apply_trips"] == 2 and f["G"] > 2 for f in fs)
    assert any(f["one_partial_block"] and not f["block_per_image"] for f in fs)
    assert any(f["apply_trips"] == 1 and not f["apply_ragged"] for f in fs)
    # path_L follows the loops
    assert bn.path_L((1024, 4, 48, 48)) == 72 + 32 + 1 + 16 + 6 and bn.path_L((1, 4, 82, 100)) == 3 + 32 + 128 + 1 + 6
    assert all(bn.path_L(c["shape"], True) >= bn.path_L(c["shape"]) for c in bn.CASES)


def test_variant_grids():
    assert len(bn.FULL_GRID) == len(set(bn.FULL_GRID)) == 16
    assert any(c["grid"] == "fold" for c in bn.CASES) and any(c["grid"] == "full" for c in bn.CASES)
    fold = [g for act in bn.ACTS for g in bn.FOLD_GRID[act]]
    assert {g[1] for g in fold} == set(bn.MODES)
    assert {(g[0], g[1] == "eval") for g in fold} == {(cbb, ev) for cbb in (False, True) for ev in (False, True)}
    assert {(g[0], g[2]) for g in fold} == {(cbb, flag) for cbb in (False, True) for flag in (False, True)}
    big = next(c for c in bn.CASES if c["grid"] == "fold")
    assert [len(bn.variants(big, act)) for act in bn.ACTS] == [2, 2, 2]
    assert set(bn.HOSTILE_INPUTS) == {"default", "offset_mean", "constant_channel", "outlier_first", "outlier_last", "row_offset",
                                      "channel_scales"}
    assert bn.HOSTILE_SHAPES == [(4, 8, 64, 64), (65, 8, 12, 12), (1024, 4, 48, 48)]


# ---- references against PyTorch float64 ------------------------------------------------------------------------------------------------
def _torch_buffers(inp, mode, x, training=True):
    """F.batch_norm's own buffer update over CALLS calls, the way nn.BatchNorm2d drives it."""
    rm, rv, nbt, out = inp["rm"].double().clone(), inp["rv"].double().clone(), bn.NBT0, []
    for _ in range(bn.CALLS):
        nbt += 1
        f = bn.MOMENTUM if mode == "tracked" else 1.0 / nbt
        F.batch_norm(x, rm, rv, None, None, training, f, bn.EPS)
        out.append((rm.clone(), rv.clone(), nbt))
    return out


@pytest.mark.parametrize("shape", [(3, 8, 5, 7), (2, 4, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_references_equal_torch_batch_norm_in_float64(shape):
    inp = bn.case_inputs(shape)
    x = inp["x"].double()
    for mode in bn.MODES:
        for affine in (True, False):
            for act in bn.ACTS:
                v = (False, mode, affine, act)
                got = bn.gradients(bn.forward(inp, v, torch.float64), inp["gy"])
                xt = x.clone().requires_grad_(True)
                w, b = (inp["weight"].double().requires_grad_(True), inp["bias"].double().requires_grad_(True)) if affine else (None, None)
                rm, rv = (None, None) if mode == "untracked" else (inp["rm"].double().clone(), inp["rv"].double().clone())
                out = F.batch_norm(xt, rm, rv, w, b, mode != "eval", bn.MOMENTUM, bn.EPS)
                y = {0: out, 1: torch.relu(out), 2: F.leaky_relu(out, bn.SLOPE)}[act]
                grads = torch.autograd.grad(y, [xt, w, b] if affine else [xt], inp["gy"].double())
                assert bn.rel_err(got["y"], y) <= 1e-12, v
                for name, g in zip(("dx", "d0", "d1"), grads):
                    if shape[2] * shape[3] > 1:      # two values per channel: dx is a difference of equal terms, of the order of eps
                        assert bn.rel_err(got[name], g) <= 1e-12, (v, name)
                if mode in ("tracked", "cumulative"):
                    for (rm_g, rv_g, n_g), (rm_t, rv_t, n_t) in zip(got["bufs"], _torch_buffers(inp, mode, x)):
                        assert n_g == n_t and bn.rel_err(rm_g, rm_t) <= 1e-12 and bn.rel_err(rv_g, rv_t) <= 1e-12, v
                else:
                    assert got["bufs"] == []


def test_cbb_reference_equals_the_restatement_of_the_older_test():
    from tests.test_batchnorm_gpu import ref_batch_norm
    shape = (3, 8, 5, 7)
    inp = bn.case_inputs(shape)
    x = inp["x"].double()
    sc, sh, res = inp["scale"].double(), inp["shift"].double(), inp["res"].double()
    for mode in bn.MODES:
        for with_res in (True, False):
            for act in bn.ACTS:
                v = (True, mode, with_res, act)
                got = bn.forward(inp, v, torch.float64, False)
                rm, rv = (None, None) if mode == "untracked" else (inp["rm"].double().clone(), inp["rv"].double().clone())
                nbt = [bn.NBT0]
                want = ref_batch_norm(x, None, None, rm, rv, nbt, mode != "eval", None if mode == "cumulative" else bn.MOMENTUM, act,
                                      bn.SLOPE, True, sc, sh, res if with_res else None)
                assert bn.rel_err(got["y"], want) <= 1e-12, v
                if mode in ("tracked", "cumulative"):
                    rm_g, rv_g, n_g = got["bufs"][0]
                    assert n_g == nbt[0] and bn.rel_err(rm_g, rm) <= 1e-12 and bn.rel_err(rv_g, rv) <= 1e-12, v
                # the folded coefficients reproduce the pre-activation
                z = (x - got["m"][:, :, None, None]) * got["a"][:, :, None, None] + got["b"][:, :, None, None]
                assert bn.rel_err(z, got["z"]) <= 1e-12


# ---- kink window -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bn.CASES, ids=CASE_IDS)
def test_kink_window_zeroes_at_most_one_percent(case):
    """From the references alone, for every variant whose backward passes through an activation."""
    shape = case["shape"]
    inp = bn.case_inputs(shape)
    worst = max(bn.kink_share(inp, v, shape) for act in (bn.ACT_RELU, bn.ACT_LRELU) for v in bn.variants(case, act))
    assert worst <= bn.KINK_SHARE_MAX, worst


@pytest.mark.parametrize("case", bn.SYNC_CASES, ids=bn.sync_id)
def test_kink_window_of_the_sync_cases(case):
    shape = bn.sync_shape(case)
    inp = bn.case_inputs(shape)
    worst = max(bn.kink_share(inp, v, shape) for v in bn.SYNC_VARIANTS)
    assert worst <= bn.KINK_SHARE_MAX, worst


# ---- conditioning ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind", bn.HOSTILE_CASES, ids=bn.nc.hostile_id)
def test_hostile_inputs_are_well_conditioned_in_float32(shape, kind):
    """e32 -- the float32 run of the reference against float64, by the measure the GPU test uses (per channel for
    channel_scales) -- stays below 1e-5 for every output."""
    inp = bn.case_inputs(shape, bn.HOSTILE_INPUTS[kind](shape))
    for v, backward in bn.hostile_variants(shape):
        f64, f32, _ = bn.yardstick(inp, v, shape, backward)
        names = ["y", "mean", "rstd", "m", "a", "b"] + (["dx", "d0", "d1"] if backward else [])
        for name in names:
            e32 = float(bn.channel_errs(f32[name], f64[name]).max()) if kind == bn.CHANNEL_SCALES else bn.rel_err(f32[name], f64[name])
            assert e32 < bn.E32_MAX, (kind, v, name, e32)
        for (rm32, rv32, _), (rm64, rv64, _) in zip(f32["bufs"], f64["bufs"]):
            for a, b in ((rm32, rm64), (rv32, rv64)):
                e32 = float(bn.channel_errs(a, b).max()) if kind == bn.CHANNEL_SCALES else bn.rel_err(a, b)
                assert e32 < bn.E32_MAX, (kind, v, e32)
