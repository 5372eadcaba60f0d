"""CPU: what the DiffAugment tests measure against (tests/augment_common.py) and the host side of the feature -- the closed-form
gradient against autograd, the float32 restatement against the float64 one, the draws of srgan_amd.augment.DiffAugment, policy
parsing, the refusal of SingleGAN_training, and the C ABI's workspace size and argument checks (the library loads without a GPU)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import augment_common as ac
from tests.small_common import gamma, rel_err

SUBSETS = (0, 1, 2, 3, 4, 5, 6, 7)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from srgan_amd import _lib
    return _lib.load()


def _flag_sets(shape):
    return SUBSETS if ac.is_small(shape) else (ac.COLOR, ac.ALL)


@pytest.mark.parametrize("shape", ac.CASES, ids=str)
def test_closed_form_gradient_equals_autograd_of_the_restatement(shape):
    x, gy = ac.inputs(shape)
    for name, table, cut in ac.tables(shape):
        for flags in _flag_sets(shape):
            _, gx = ac.restate_with_grad(x, gy, table, flags, cut, torch.float64)
            want = ac.closed_form_grad(gy, table, flags, cut)
            assert float(ac.sample_errs(want, gx).max()) <= 1e-12, (shape, name, flags)


@pytest.mark.parametrize("shape", ac.CASES, ids=str)
def test_float32_restatement_stays_within_gamma_of_the_float64_one(shape):
    """L per case: ``augment_common.seq_len`` -- 4 per 1024 floats of the sample up to 16 (the second level adds at most 2 partials
    per thread in the case list and never sets L)"""
    x, gy = ac.inputs(shape)
    L = ac.seq_len(*shape[1:])
    assert L == min(16, 4 * -(-3 * shape[1] * shape[2] // 1024)) and -(-ac.chunks(*shape[1:]) // 256) <= 2
    for name, table, cut in ac.tables(shape):
        for flags in (ac.COLOR, ac.ALL):
            y64, g64 = ac.restate_with_grad(x, gy, table, flags, cut, torch.float64)
            y32, g32 = ac.restate_with_grad(x, gy, table, flags, cut, torch.float32)
            assert float(ac.sample_errs(y32, y64).max()) <= gamma(L), (shape, name, flags, "forward")
            assert float(ac.sample_errs(g32, g64).max()) <= gamma(L), (shape, name, flags, "backward")


def test_restatement_by_hand_on_a_2x2_image():
    """every step spelt out for one sample: brightness, saturation, contrast, a shift by (1, -1), a 1 x 1 window at (0, 1)"""
    x = torch.arange(12, dtype=torch.float64).view(1, 3, 2, 2) / 10
    table = ac.build_table([(0.75, 0.25, 0.5, 1, -1, 0, 1)])
    b, s, a = 0.25, 0.5, 1.0
    x1 = x + b
    m = (x1[:, 0] + x1[:, 1] + x1[:, 2]) / 3
    x2 = (x1 - m) * s + m
    M = x2.sum() / 12
    x3 = (x2 - M) * a + M
    want = torch.zeros_like(x3)
    want[0, :, 0, 1] = x3[0, :, 1, 0]          # y[0, 1] = x3[0 + 1, 1 - 1]; the other three read outside the image
    want[0, :, 0, 1] = 0                       # ... and the 1 x 1 window sits on (0, 1)
    got = ac.restate(x, table, ac.ALL, (1, 1))
    assert torch.equal(got, want)
    got = ac.restate(x, table, ac.COLOR | ac.TRANSLATION, (1, 1))
    assert float((got[0, :, 0, 1] - x3[0, :, 1, 0]).abs().max()) <= 1e-15 and float(got[0, :, 0, 1].abs().min()) > 0.1
    rest = got.clone()
    rest[0, :, 0, 1] = 0
    assert float(rest.abs().max()) == 0.0
    assert abs(float(M) - float(x.mean() + b)) <= 1e-15          # the identity the kernel may use


# ---- draws ---------------------------------------------------------------------------------------------------------------------
def test_draws_stay_in_range_and_reach_both_ends():
    from srgan_amd.augment import DiffAugment
    h, w = 8, 12
    aug = DiffAugment(seed=5)
    state = torch.get_rng_state()
    t = aug.draw(10000, h, w)
    assert torch.equal(torch.get_rng_state(), state)                 # the default generator is not touched
    assert t.dtype == torch.float32 and tuple(t.shape) == (10000, 8) and not t.is_cuda
    b, s, a = t[:, 0], t[:, 1], t[:, 2]
    assert float(b.min()) >= -0.5 and float(b.max()) < 0.5
    assert float(s.min()) >= 0.0 and float(s.max()) < 2.0
    assert float(a.min()) >= 0.5 and float(a.max()) <= 1.5           # (r_c + 0.5 rounds to 1.5 for the last float32 below 1)
    ints = t[:, 3:7]
    assert torch.equal(ints, ints.round())
    sy, sx = ac.window(h, 0.125), ac.window(w, 0.125)                # 1 and 2
    ch, cw = aug.cut(h, w)                                           # 4 and 6: even, so the centre range is size + 1
    assert (sy, sx, ch, cw) == (1, 2, 4, 6)
    for col, lo, hi in ((3, -sy, sy), (4, -sx, sx), (5, 0, h), (6, 0, w)):
        assert float(t[:, col].min()) == lo and float(t[:, col].max()) == hi, (col, lo, hi)
    assert float(t[:, 7].abs().max()) == 0.0
    odd = DiffAugment(cutout=0.625, seed=5).draw(10000, 8, 8)        # window 5: odd, the centre range is the size
    assert float(odd[:, 5].min()) == 0 and float(odd[:, 5].max()) == 7


def test_same_seed_same_tables_and_state_dict_round_trip():
    from srgan_amd.augment import DiffAugment
    a, b = DiffAugment(seed=11), DiffAugment(seed=11)
    assert torch.equal(a.draw(7, 16, 16), b.draw(7, 16, 16))
    assert not torch.equal(a.draw(7, 16, 16), DiffAugment(seed=12).draw(7, 16, 16))
    b.draw(7, 16, 16)
    sd = a.state_dict()
    nxt = a.draw(5, 32, 32)
    c = DiffAugment("color", translation=0.3, cutout=0.1, seed=99)
    sd2 = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
    c.load_state_dict(sd2)
    assert (c.policy, c.translation, c.cutout) == (a.policy, a.translation, a.cutout)
    assert torch.equal(c.draw(5, 32, 32), nxt)
    assert torch.equal(b.draw(5, 32, 32), nxt)
    assert not torch.equal(DiffAugment().draw(4, 8, 8), DiffAugment().draw(4, 8, 8))       # unseeded: fresh entropy each


def test_groups_that_are_off_yield_identity_rows():
    from srgan_amd.augment import DiffAugment
    ident = torch.tensor([0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]).repeat(6, 1)
    assert torch.equal(DiffAugment("", seed=1).draw(6, 16, 16), ident)
    t = DiffAugment("translation", seed=1).draw(6, 16, 16)
    assert torch.equal(t[:, :3], ident[:, :3]) and torch.equal(t[:, 5:], ident[:, 5:]) and float(t[:, 3:5].abs().max()) > 0
    t = DiffAugment("color,cutout", seed=1).draw(6, 16, 16)
    assert torch.equal(t[:, 3:5], ident[:, 3:5]) and not torch.equal(t[:, :3], ident[:, :3])
    # identity rows are the identity of the restatement, whatever the flags say (colour: up to the rounding of (x - m) + m)
    x, _ = ac.inputs((6, 16, 16))
    assert torch.equal(ac.restate(x, ident, ac.TRANSLATION | ac.CUTOUT, (0, 0), torch.float64), x.double())
    assert rel_err(ac.restate(x, ident, ac.ALL, (0, 0), torch.float64), x.double()) <= 1e-15


# ---- host logic ----------------------------------------------------------------------------------------------------------------
def test_policy_parsing():
    from srgan_amd import ops
    from srgan_amd.augment import DiffAugment
    assert (ops.AUG_COLOR, ops.AUG_TRANSLATION, ops.AUG_CUTOUT) == (ac.COLOR, ac.TRANSLATION, ac.CUTOUT) and ops.AUG_ROW == ac.ROW
    assert DiffAugment().flags == 7 and DiffAugment().policy == "color,translation,cutout"
    assert (DiffAugment().translation, DiffAugment().cutout) == (0.125, 0.5)
    assert DiffAugment("").flags == 0
    assert DiffAugment("cutout, color").flags == 5 and DiffAugment("translation").flags == 2
    for bad in ("colour", "color,flip", "color,,cutout", None):
        with pytest.raises(ValueError):
            DiffAugment(bad)
    aug = DiffAugment("color")
    aug.policy = "rotate"                                          # edited in place: refused where it is read
    with pytest.raises(ValueError, match="rotate"):
        aug.flags
    assert DiffAugment(cutout=0.5).cut(5, 7) == (3, 4) and DiffAugment(cutout=1.0).cut(5, 7) == (5, 7)
    assert aug.draw_fn == aug.draw                                 # the injectable draw source defaults to the object's own


def test_trainers_host_side():
    from srgan_amd import model
    from srgan_amd.trainer import SingleGAN_training, SRGAN_training
    from tests.common import TIER_T
    g, d, e = TIER_T["G"], TIER_T["D"], TIER_T["E"]
    G = model.SingleGenerator(g["nch_in"], g["nch"], g["reduce"], g["num_cls"], g["res_num"], "instance", num_con=g["num_con"])
    D = model.SingleDiscriminator_solo_multi(d["nch_in"], d["nch"], d["reduce"], d["num_cls"], "instance", d["n_class"])
    E = model.Encoder(e["nch_in"], e["nch_out"], e["nch"], e["num_cls"], "instance", e["num_con"], "cpu")
    lbd = dict(**{"class": 1.0}, cycle=5.0, idt=5.0, reg=0.5, idt_reg=0.5, KL=0.0, batch_KL=10.0, corr_enc=0.0, hist=0.0)
    crit = [nn.MSELoss(), nn.MSELoss()]
    single = SingleGAN_training([G, D, E], [None] * 3, crit, lbd, 1, "cpu", np.eye(4), 8, [0, 1, 2, 3], singleD=True)
    with pytest.raises(NotImplementedError, match="SingleGAN_training.*SRGAN_training"):
        single.enable_diffaugment()
    sg = SRGAN_training([G, D, E], [None] * 3, crit, lbd, 3, "cpu", np.eye(4), 4, "mu", 8)
    assert sg.augment is None and sg._stage_draws(sg.augment) == 0
    assert sg.enable_diffaugment(policy="color,cutout", translation=0.2, cutout=0.25, seed=3) is sg
    assert (sg.augment.flags, sg.augment.translation, sg.augment.cutout) == (5, 0.2, 0.25) and sg._stage_draws(sg.augment) == 7      # 2k + 1
    with pytest.raises(ValueError):
        sg.enable_diffaugment(policy="colour")
    sg.enable_diffaugment(policy="")
    assert sg.augment is not None and sg._stage_draws(sg.augment) == 0 and not sg._stage_on(sg.augment)                                        # identity
    sg.disable_diffaugment()
    assert sg.augment is None
    from srgan_amd import dp
    orig = dp.world_size
    dp.world_size = lambda: 2
    try:
        sg.enable_diffaugment(seed=1)                                  # a process group does not refuse it
    finally:
        dp.world_size = orig
    # the draw order of a step: the injected source is asked 2k + 1 times for [B, 8]; the eager path uploads what it returns
    calls = []

    def fixed(n, h, w):
        calls.append((n, h, w))
        return torch.full((n, 8), float(len(calls)))

    sg.augment.draw_fn = fixed
    pair = sg._stage_tables(sg.augment, 2, 4, 16, 12)
    one = sg._stage_tables(sg.augment, 1, 4, 16, 12)
    assert calls == [(4, 16, 12)] * 3 and tuple(pair.shape) == (8, 8) and tuple(one.shape) == (4, 8)
    assert torch.equal(pair[:4], torch.full((4, 8), 1.0)) and torch.equal(pair[4:], torch.full((4, 8), 2.0))


def test_workspace_size_and_argument_checks_through_ctypes(lib):
    for n, h, w in ac.CASES:
        assert lib.srgan_diffaugment_workspace(n, h, w) == ac.workspace_bytes(n, h, w), (n, h, w)
    assert lib.srgan_diffaugment_workspace(64, 128, 128) == 4 * 64 * 12
    for bad in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, -2), (1, 1 << 15, (1 << 14) + 1)):
        assert lib.srgan_diffaugment_workspace(*bad) == 0 and b"diffaugment_workspace" in lib.srgan_last_error()
    buf = (ctypes.c_char * 4096)()
    ok = dict(x0=buf, n0=1, x1=None, n1=0, table=buf, y=buf, c=3, h=4, w=4, flags=7, ch=2, cw=2, ws=buf, nb=4096)

    def fwd(**kw):
        a = dict(ok, **kw)
        return lib.srgan_diffaugment_fwd(a["x0"], a["n0"], a["x1"], a["n1"], a["table"], a["y"], a["c"], a["h"], a["w"], a["flags"],
                                         a["ch"], a["cw"], a["ws"], a["nb"], None)

    def bwd(**kw):
        a = dict(ok, **kw)
        return lib.srgan_diffaugment_bwd(a["x0"], a["table"], a["y"], a["n0"], a["c"], a["h"], a["w"], a["flags"], a["ch"], a["cw"],
                                         a["ws"], a["nb"], None)

    for call, name in ((fwd, b"diffaugment_fwd"), (bwd, b"diffaugment_bwd")):
        for kw, word in ((dict(c=4), b"three-channel"), (dict(c=1), b"three-channel"), (dict(x0=None), b"null pointer"),
                         (dict(table=None), b"null pointer"), (dict(y=None), b"null pointer"), (dict(n0=0), b"n0"),
                         (dict(n0=-3), b"n0"), (dict(flags=8), b"flags"), (dict(flags=-1), b"flags"), (dict(ws=None), b"workspace"),
                         (dict(nb=3), b"workspace"), (dict(h=0), b"H ="), (dict(ch=-1), b"cutout window")):
            assert call(**kw) == -1, (name, kw)
            err = lib.srgan_last_error()
            assert name in err and word in err, (name, kw, err)
    # the two-source form: a second pointer without rows, or rows without a pointer
    assert fwd(x1=buf, n1=0) == -1 and fwd(x1=None, n1=2) == -1 and fwd(x1=buf, n1=-1) == -1
