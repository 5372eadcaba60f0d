"""CPU: the parts of the R1 gradient penalty (srgan_amd.r1, csrc/r1.hip, SRGAN_training.enable_r1) that need no GPU -- the two
float64 restatements of tests/r1_common.py pinned to each other, the float32 yardstick, the pool^T divisors against autograd, the
mask condition of the GPU test's seeds, validation and the schedule, the C ABI's argument checks and the launch descriptors."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import nets, params
from tests import r1_common as rc


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from srgan_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.srgan_last_error().decode()


@pytest.fixture(scope="module")
def refs():
    """per pass case: (P, x64, (dW, g, P) of form (a) in float64, of form (b) in float64, of form (b) in float32)"""
    out = {}
    ge = rc.PASS_GAMMA * rc.PASS_EVERY
    for case in rc.PASS_CASES:
        n, h, w, layers, seed = case
        P = rc.pass_params(layers)
        x = rc.real_batch(n, h, w, seed).float().double()
        P64 = rc.cast(P, torch.float64)
        out[case] = (P, x, rc.autograd_form(P64, x, ge), rc.closed_form(P64, x, ge), rc.closed_form(P, x.float(), ge))
    return out


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------
def test_scalar_is_that_of_the_oracle_discriminator():
    P = rc.cast(rc.pass_params(4), torch.float64)
    x = rc.real_batch(2, 128, 128, 3)
    outs, _ = nets.discriminator(P, x, 4)
    assert torch.equal(rc.scalar_S(P, x), sum(o.mean(dim=(1, 2, 3)) for o in outs))


@pytest.mark.parametrize("case", rc.PASS_CASES, ids=lambda c: "x".join(map(str, c[:3])))
def test_closed_form_equals_the_double_backward(refs, case):
    _, _, (dWa, ga, Pa), (dWb, gb, Pb), _ = refs[case]
    assert dWa.keys() == dWb.keys() and len(dWa) == 2 * (case[3] + 1)
    for k in dWa:
        assert float(dWa[k].abs().max()) > 0 and rc.rel_err(dWb[k], dWa[k]) <= 1e-12, k
    assert rc.rel_err(gb, ga) <= 1e-12 and rc.rel_err(Pb, Pa) <= 1e-12 and float(Pa) > 0


@pytest.mark.parametrize("case", rc.PASS_CASES, ids=lambda c: "x".join(map(str, c[:3])))
def test_float32_yardstick_and_mask_condition(refs, case):
    """e32 per tensor (float32 CPU against float64, own masks each) stays at rounding level, and the float32 forward's masks differ
    from float64's only inside the band and in at most 1 % of a layer: the condition the GPU test puts on the device's masks, held
    here for its seeds from the references alone"""
    P, x, _, (dW64, g64, P64), (dW32, g32, P32) = refs[case]
    m32 = rc.own_masks(P, x.float())
    rc.assert_masks_within(P, x, m32, "float32 CPU")
    same = all(torch.equal(a, b) for sa, sb in zip(m32, rc.own_masks(rc.cast(P, torch.float64), x)) for a, b in zip(sa, sb))
    if same:            # equal masks: the float32 closed form differs from float64 by rounding only
        for k in dW64:
            assert rc.rel_err(dW32[k], dW64[k]) <= 64 * rc.EPS32, k
        assert rc.rel_err(g32, g64) <= 64 * rc.EPS32 and rc.rel_err(P32, P64) <= 64 * rc.EPS32


def test_given_masks_are_taken_as_constants(refs):
    case = rc.PASS_CASES[0]
    P, x, _, (dW, g, pen), _ = refs[case]
    P64 = rc.cast(P, torch.float64)
    masks = rc.own_masks(P64, x)
    again = rc.closed_form(P64, x, rc.PASS_GAMMA * rc.PASS_EVERY, masks)
    assert all(torch.equal(again[0][k], dW[k]) for k in dW) and torch.equal(again[1], g)
    masks[0][0] = ~masks[0][0]
    moved = rc.closed_form(P64, x, rc.PASS_GAMMA * rc.PASS_EVERY, masks)
    assert rc.rel_err(moved[1], g) > 1e-3
    with pytest.raises(AssertionError):
        rc.assert_masks_within(P, x, masks, "flipped")


@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (3, 5), (4, 6), (33, 47), (40, 24), (37, 111), (16, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pool_transpose_divisors_against_autograd(hw):
    h, w = hw
    g = torch.Generator().manual_seed(h * 1000 + w)
    h2 = torch.randn(2, 3, (h - 1) // 2 + 1, (w - 1) // 2 + 1, generator=g, dtype=torch.float64)
    x = torch.zeros(2, 3, h, w, dtype=torch.float64, requires_grad=True)
    (ga,) = torch.autograd.grad((F.avg_pool2d(x, 3, 2, 1, count_include_pad=False) * h2).sum(), x)
    assert float((ga - rc.pool_t(h2, h, w)).abs().max()) <= 1e-15 * float(h2.abs().max())
    d = rc.pool_divisors(h, w)
    assert set(d.flatten().tolist()) <= {1.0, 2.0, 3.0, 4.0, 6.0, 9.0}
    if h >= 3 and w >= 3:
        assert set(d.flatten().tolist()) <= {4.0, 6.0, 9.0} and float(d[0, 0]) == 4.0
        # the trailing edge: a full window on odd sizes, a cut one on even sizes
        assert float(d[-1, -1]) == (2.0 if h % 2 else 3.0) * (2.0 if w % 2 else 3.0)


# ---- host logic ----------------------------------------------------------------------------------------------------------------------
def test_validation_and_schedule():
    from srgan_amd import r1
    for bad in (-1.0, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="gamma"):
            r1.R1Penalty(bad, 1)
    for bad in (0, -2, 1.5, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="every"):
            r1.R1Penalty(10.0, bad)
    st = r1.R1Penalty(0.0, 3)
    assert st.gamma == 0.0 and st.every == 3 and st.gamma_eff == 0.0
    assert r1.R1Penalty(2.5, 4).gamma_eff == 10.0
    assert r1.schedule(5, 1) == [True] * 5
    assert r1.schedule(5, 2) == [True, False, True, False, True]
    assert r1.schedule(5, 4) == [True, False, False, False, True]
    assert r1.schedule(2, 2) == [True, False] and r1.schedule(3, 7) == [True, False, False]
    with pytest.raises(ValueError, match="gamma"):
        st.set_gamma(-0.5)
    st.set_gamma(4.0)                     # no device record yet: host state only
    assert st.gamma == 4.0 and st.stats()["updates"] == 0 and st.stats()["penalty"] == 0.0


def test_fingerprint_follows_every_and_not_gamma():
    from srgan_amd import r1
    a = r1.R1Penalty(10.0, 1)
    fp = a.fingerprint()
    a.set_gamma(3.0)
    assert a.fingerprint() == fp
    b = r1.R1Penalty(10.0, 2)
    assert b.fingerprint() != fp and r1.R1Penalty(10.0, 1).fingerprint() != fp          # another object is another recording
    assert a.graph_keepalive() == []


def test_trainer_api_without_a_gpu():
    """enable / disable / set / stats on a trainer whose networks are never run; the refusals that need no step"""
    import numpy as np
    from srgan_amd import model, r1, trainer
    D = model.SingleDiscriminator_solo_multi(3, 4, 2, 4, "instance", 4)
    G = model.SingleGenerator(3, 4, 2, 2, 1, "instance", num_con=12)
    E = model.Encoder(3, 8, 4, 4, "instance", 4, "cpu")
    lbd = dict(**{"class": 1.0}, cycle=5.0, idt=5.0, reg=0.5, idt_reg=0.5, KL=0.0, batch_KL=10.0, corr_enc=100.0, hist=0.0)
    crit = [torch.nn.MSELoss(), torch.nn.MSELoss()]
    sg = trainer.SRGAN_training([G, D, E], [None, None, None], crit, lbd, 2, "cpu", np.eye(4), batch_size=4, encoded_feature="mu", ndim=8)
    assert sg._r1 is None and sg.r1_stats() is None
    with pytest.raises(RuntimeError, match="enable_r1"):
        sg.set_r1_gamma(1.0)
    assert sg.enable_r1(gamma=5.0, every=2) is sg and isinstance(sg._r1, r1.R1Penalty)
    assert sg.r1_stats()["gamma"] == 5.0 and sg.r1_stats()["every"] == 2 and sg.r1_stats()["updates"] == 0
    sg.set_r1_gamma(7.0)
    assert sg._r1.gamma == 7.0
    for bad in (dict(gamma=-1.0), dict(every=0), dict(every=1.5)):
        with pytest.raises(ValueError):
            sg.enable_r1(**bad)
    sg.disable_r1()
    assert sg._r1 is None
    # a discriminator without the two-scale layout
    sg.D = model.SingleDiscriminator_original_multi(3, 4, 2, 4, "instance", 2)
    with pytest.raises(NotImplementedError, match="forward_logits / two-scale layout"):
        sg.enable_r1()
    assert sg._r1 is None
    # the other trainer
    with pytest.raises(NotImplementedError, match="SRGAN_training.enable_r1"):
        trainer.SingleGAN_training.enable_r1(object())
    # image sizes and the bf16 mode are checked when the pass runs
    from srgan_amd import ops
    D2 = model.SingleDiscriminator_solo_multi(3, 4, 2, 4, "instance", 4)
    with pytest.raises(NotImplementedError, match="multiples of 16"):
        r1.check_supported(D2, torch.zeros(2, 3, 72, 64))
    with pytest.raises(NotImplementedError, match="multiples of 16"):
        r1.check_supported(D2, torch.zeros(2, 3, 64, 40))
    assert len(r1.check_supported(D2, torch.zeros(2, 3, 64, 48))) == 2


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_back_before_any_launch(lib):
    buf = (ctypes.c_char * 4096)()
    b = ctypes.byref(buf)
    nan, inf = float("nan"), float("inf")
    assert lib.srgan_r1_state_bytes() == 32
    for fn, name in ((lib.srgan_r1_state_init, "r1_state_init"), (lib.srgan_r1_state_set, "r1_state_set")):
        for gamma, every, n in ((-1.0, 1, 4), (nan, 1, 4), (inf, 1, 4), (1.0, 0, 4), (1.0, -1, 4), (1.0, 1, 0)):
            assert fn(b, gamma, every, n, None) == -1 and name in _err(lib), (name, gamma, every, n)
        assert fn(None, 1.0, 1, 4, None) == -1 and name in _err(lib)
    for n, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (1, 40000, 40000)):
        assert lib.srgan_r1_workspace(n, h, w) == 0 and "r1_workspace" in _err(lib)
    assert lib.srgan_r1_workspace(2, 128, 128) == 2 * 12 * 4 and lib.srgan_r1_workspace(1, 37, 111) == 4 * 4
    assert lib.srgan_r1_workspace(1, 1, 1) == 4 and lib.srgan_r1_workspace(3, 32, 32) == 12
    p = [ctypes.c_void_p(0x10000000 + (i << 20)) for i in range(5)]
    seed = lib.srgan_r1_seed
    assert seed(p[0], p[1], p[2], p[3], 2, 4, 8, 8, p[4], 64, None) == -1 and "3 channels" in _err(lib)
    for k in range(5):
        q = list(p)
        q[k] = None
        assert seed(q[0], q[1], q[2], q[3], 2, 3, 8, 8, q[4], 64, None) == -1 and "null pointer" in _err(lib), k
    assert seed(p[0], p[1], p[2], p[3], 0, 3, 8, 8, p[4], 64, None) == -1 and "geometry" in _err(lib)
    assert seed(p[0], p[1], p[2], p[3], 2, 3, 8, 0, p[4], 64, None) == -1 and "geometry" in _err(lib)
    assert seed(p[0], p[1], p[2], p[3], 2, 3, 128, 128, p[4], 95, None) == -1 and "workspace" in _err(lib)
    assert seed(p[0], p[1], p[2], p[0], 2, 3, 8, 8, p[4], 64, None) == -1 and "alias" in _err(lib)
    assert seed(p[0], p[1], p[2], p[1], 2, 3, 8, 8, p[4], 64, None) == -1 and "alias" in _err(lib)
    assert seed(ctypes.c_void_p(0x10000002), p[1], p[2], p[3], 2, 3, 8, 8, p[4], 64, None) == -1 and "aligned" in _err(lib)
    fin = lib.srgan_r1_finalize
    assert fin(None, 64, 2, 8, 8, p[2], None) == -1 and "null pointer" in _err(lib)
    assert fin(p[4], 64, 2, 8, 8, None, None) == -1 and "null pointer" in _err(lib)
    assert fin(p[4], 64, 2, -8, 8, p[2], None) == -1 and "geometry" in _err(lib)
    assert fin(p[4], 4, 2, 8, 8, p[2], None) == -1 and "workspace" in _err(lib)


# ---- launch descriptors (no GPU: tests/hip_shim/launch_shim.c logs them) -------------------------------------------------------------
def test_launch_descriptors_within_aql_limits_and_launch_counts(lib, tmp_path):
    """one seed launch of min(N * ceil(3 H W / 4096), 2048) workgroups and one finalize workgroup per call, 256 threads each, inside
    the AQL limits, no scratch, no dynamic LDS"""
    from srgan_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    import isa_tools
    so = str(tmp_path / "launch_shim.so")
    subprocess.run(["gcc", "-shared", "-fPIC", "-O1", "-o", so, os.path.join(here, "hip_shim", "launch_shim.c")], check=True)
    desc = {k["name"]: k for k in isa_tools.kernel_descriptors(_lib.LIB_PATH)}
    log = str(tmp_path / "launches.log")
    env = dict(os.environ, LD_PRELOAD=so, SRGAN_SHIM_LOG=log)
    env.pop("SRGAN_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(here, "hip_shim", "drive_r1.py"), _lib.LIB_PATH], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    seen, cur = {}, None
    for line in open(log):
        if line.startswith("#"):
            cur = line[1:].strip()
            seen[cur] = []
            continue
        kname, gx, gy, gz, bx, by, bz, dyn = line.split()
        gx, gy, gz, bx, by, bz, dyn = map(int, (gx, gy, gz, bx, by, bz, dyn))
        short = next((s for s in ("r1_seed_kernel", "r1_finalize_kernel") if s in kname), None)
        assert short is not None, kname
        k = desc[kname]
        ctx = (cur, kname, (gx, gy, gz), (bx, by, bz))
        assert (gy, gz) == (1, 1) and gx >= 1 and (bx, by, bz) == (256, 1, 1) and 256 <= k["max_wg"], ctx
        assert gx * bx < 2 ** 32, ctx
        assert k["lds"] + dyn <= 160 * 1024 and k["scratch"] == 0 and dyn == 0, ctx
        seen[cur].append((short, gx))
    sys.path.insert(0, os.path.join(here, "hip_shim"))
    import drive_r1
    assert len(seen) == len(drive_r1.SHAPES)
    for n, h, w in drive_r1.SHAPES:
        items = n * -(-(3 * h * w) // 4096)
        assert seen[f"{n} {h} {w}"] == [("r1_seed_kernel", min(items, 2048)), ("r1_finalize_kernel", 1)], (n, h, w)
    assert seen["64 256 256"][0][1] == 2048 and seen["2 128 128"][0][1] == 24
