"""CPU: the parts of balanced consistency regularisation (srgan_amd.consistency, csrc/consistency.hip, SRGAN_training.enable_bcr) that
need no GPU -- the restatements of tests/cr_common.py against autograd and by hand, the draws, validation, the fingerprint, the
trainer's interface and refusals, the checkpoint section, the C ABI's argument checks, and the oracle-side "the term acts" condition
of the GPU train test."""
import ctypes
import io

import numpy as np
import pytest
import torch

from tests import cr_common as cc


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from srgan_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.srgan_last_error().decode()


# ---- the restatements ------------------------------------------------------------------------------------------------------------------
def test_transform_by_hand():
    x = torch.arange(2 * 3 * 2 * 3, dtype=torch.float64).reshape(2, 3, 2, 3)
    table = torch.zeros(2, 8)
    table[0, :3] = torch.tensor([1.0, 0.0, 1.0])               # flip, then one column to the right
    table[1, :3] = torch.tensor([0.0, -1.0, 0.0])              # one row up
    y = cc.transform(x, table, 3)
    assert y[0, 0].tolist() == [[0.0, 2.0, 1.0], [0.0, 5.0, 4.0]]
    assert y[1, 0].tolist() == [[21.0, 22.0, 23.0], [0.0, 0.0, 0.0]]
    assert torch.equal(cc.transform(x, table, 0), x)           # both groups off: the identity
    assert cc.transform(x, table, 1)[0, 0].tolist() == [[2.0, 1.0, 0.0], [5.0, 4.0, 3.0]] and torch.equal(cc.transform(x, table, 1)[1], x[1])
    assert torch.equal(cc.transform(x, table, 2)[0, 0], torch.tensor([[0.0, 0.0, 1.0], [0.0, 3.0, 4.0]], dtype=torch.float64))
    # the table as the kernel reads it: truncated, clamped to one line short of the image, non-finite reads 0
    hostile = torch.tensor([[float("nan")] * 8, [1e30, 1e30, -1e30, 0, 0, 0, 0, 0], [0.9, 1.9, -1.9, 0, 0, 0, 0, 0],
                            [-0.0, float("inf"), float("-inf"), 0, 0, 0, 0, 0], [7.0, -0.5, 0.5, 0, 0, 0, 0, 0]])
    assert cc.table_ints(hostile, 3, 4, 5) == [(0, 0, 0), (1, 3, -4), (0, 1, -1), (0, 0, 0), (1, 0, 0)]
    assert cc.table_ints(hostile, 0, 4, 5) == [(0, 0, 0)] * 5
    assert cc.table_ints(hostile[1:2], 3, 1, 7) == [(1, 0, -6)]                 # a one-pixel-high image has no row shift


@pytest.mark.parametrize("case", [c for c in cc.loss_cases() if c[0] <= 8], ids=str)
def test_restated_gradients_equal_autograd_at_float64(case):
    P, per_row, pairs_first, gk, ck, with_class = case
    inp = cc.loss_inputs(P, per_row, with_class, seed=P + pairs_first)
    kw = dict(rows_first=(P + 1) // 2, t_first=1.0, t_rest=0.0, w_class=0.7, every=2, gan_kind=gk, class_kind=ck, pairs_first=pairs_first)
    vals, d_o, dz = cc.loss_run(inp, torch.float64, lam_real=3.0, lam_fake=0.5, **kw)
    vals0, d_o0, dz0 = cc.loss_run(inp, torch.float64, lam_real=0.0, lam_fake=0.0, **kw)
    assert torch.equal(vals[:6], vals0[:6]) and float(vals0[6]) == float(vals0[3])
    B1, B2 = pairs_first, P - pairs_first
    want = float(vals[3]) + 2 * (3.0 * float(vals[4]) * (B1 > 0) + 0.5 * float(vals[5]) * (B2 > 0))
    assert abs(float(vals[6]) - want) <= 1e-14 * abs(want)
    outs64 = [o.double() for o in inp["outs"]]
    for s, g in enumerate(cc.cr_grad_closed(outs64, 3.0, 0.5, 2, pairs_first)):
        diff = d_o[s] - d_o0[s]                                 # autograd's share of the consistency terms
        assert float((diff - g).abs().max()) <= 1e-13 * max(float(g.abs().max()), 1e-30), s
        assert torch.equal(d_o0[s][P:], torch.zeros_like(d_o0[s][P:]))       # back rows: no GAN loss
    for a, b in zip(dz, dz0):
        assert torch.equal(a, b) and not a[kw["rows_first"]:].any()          # the class heads do not enter; back rows carry none


def test_an_empty_group_is_zero_and_a_zero_weight_hides_nan():
    inp = cc.loss_inputs(4, (5, 3), False, seed=1)
    kw = dict(rows_first=2, t_first=1.0, t_rest=0.0, w_class=1.0, every=1, gan_kind=0, class_kind=0)
    vals, _, _ = cc.loss_run(inp, torch.float64, lam_real=2.0, lam_fake=2.0, pairs_first=0, **kw)
    assert float(vals[4]) == 0.0 and float(vals[5]) > 0
    inp["outs"][0][4:] = float("nan")
    vals, d_o, _ = cc.loss_run(inp, torch.float64, lam_real=0.0, lam_fake=0.0, pairs_first=2, **kw)
    assert torch.isfinite(vals[:4]).all() and float(vals[6]) == float(vals[3]) and not d_o[0][4:].any()


# ---- the draws -----------------------------------------------------------------------------------------------------------------------
def test_draw_ranges_off_groups_and_the_default_generator():
    from srgan_amd.consistency import ConsistencyPairs
    st = ConsistencyPairs(seed=3)
    before = torch.get_rng_state()
    t = st.draw(4096, 128, 64)
    assert torch.equal(torch.get_rng_state(), before)                 # the default generator (style noise) is untouched
    assert tuple(t.shape) == (4096, 8) and t.dtype == torch.float32 and not t[:, 3:].any()
    assert set(t[:, 0].tolist()) == {0.0, 1.0} and 0.45 < float(t[:, 0].mean()) < 0.55
    assert set(t[:, 1].tolist()) == set(float(v) for v in range(-16, 17))          # int(128 * 0.125 + 0.5) = 16
    assert set(t[:, 2].tolist()) == set(float(v) for v in range(-8, 9))
    assert ConsistencyPairs(translation=0.3).draw(64, 5, 5)[:, 1:3].abs().max() <= 2  # int(5 * 0.3 + 0.5) = 2
    # a group that is off draws nothing and is the identity: the generator stands where the other group alone leaves it
    flip, ref = ConsistencyPairs("flip", seed=5), torch.Generator().manual_seed(5)
    t = flip.draw(8, 16, 16)
    assert torch.equal(t[:, 0], (torch.rand(8, generator=ref, dtype=torch.float32) < 0.5).float()) and not t[:, 1:].any()
    assert torch.equal(flip.generator.get_state(), ref.get_state())
    none = ConsistencyPairs("", seed=5)
    state = none.generator.get_state()
    assert not none.draw(8, 16, 16).any() and torch.equal(none.generator.get_state(), state) and none.flags == 0
    tr = ConsistencyPairs("translation", seed=5)
    assert not tr.draw(8, 16, 16)[:, 0].any() and tr.flags == 2
    with pytest.raises(ValueError, match="unknown policy entry"):
        ConsistencyPairs("flip,rot90")
    for bad in (-0.1, float("nan"), "x"):
        with pytest.raises(ValueError, match="translation"):
            ConsistencyPairs(translation=bad)
    with pytest.raises(ValueError, match="not gated"):
        st.apply(torch.zeros(1, 3, 4, 4), torch.zeros(1, 8), gated=True)


def _cpu_trainer(k=2):
    from srgan_amd import model, trainer
    D = model.SingleDiscriminator_solo_multi(3, 4, 2, 4, "instance", 4)
    G = model.SingleGenerator(3, 4, 2, 2, 1, "instance", num_con=12)
    E = model.Encoder(3, 8, 4, 4, "instance", 4, "cpu")
    lbd = dict(**{"class": 1.0}, cycle=5.0, idt=5.0, reg=0.5, idt_reg=0.5, KL=0.0, batch_KL=10.0, corr_enc=100.0, hist=0.0)
    crit = [torch.nn.MSELoss(), torch.nn.MSELoss()]
    return trainer.SRGAN_training([G, D, E], [None, None, None], crit, lbd, k, "cpu", np.eye(4), batch_size=4, encoded_feature="mu",
                                  ndim=8)


@pytest.mark.parametrize("every", [1, 2])
def test_draw_order_per_step(every):
    """two tables per PENALISED update (real rows, then fake rows), none for phase 1, never joined with gate uniforms, and the other
    stages' draws are what they are without the feature"""
    from srgan_amd.augment import DiffAugment, GeometricAugment
    from srgan_amd.consistency import ConsistencyPairs, schedule
    k = 3
    sg = _cpu_trainer(k).enable_diffaugment(seed=11).enable_geometric_augment(seed=12)
    sg.enable_ada()
    sg.enable_bcr(every=every, seed=13)
    assert schedule(k, every) == [i % every == 0 for i in range(k)]
    assert sg._stage_draws(sg.bcr.stage) == 2 * sum(schedule(k, every)) == (6 if every == 1 else 4)
    assert sg._stage_draws(sg.augment) == sg._stage_draws(sg.geometry) == 2 * k + 1
    assert sg._drawing_stages() == [sg.augment, sg.geometry, sg.bcr.stage] and sg._stages() == [sg.augment, sg.geometry]
    assert sg._gated(sg.augment) and sg._gated(sg.geometry) and not sg._gated(sg.bcr.stage)
    before = torch.get_rng_state()
    ref = ConsistencyPairs(seed=13)
    for _ in range(sg._stage_draws(sg.bcr.stage)):
        r = sg._stage_row_draw(sg.bcr.stage, 4, 16, 12)
        assert tuple(r.shape) == (4, 8) and torch.equal(r, ref.draw(4, 16, 12))           # plain tables under enable_ada too
    assert torch.equal(torch.get_rng_state(), before)
    assert torch.equal(sg.bcr.stage.generator.get_state(), ref.generator.get_state())
    assert torch.equal(sg.augment.generator.get_state(), DiffAugment(seed=11).generator.get_state())
    assert torch.equal(sg.geometry.generator.get_state(), GeometricAugment(seed=12).generator.get_state())
    # an empty policy still makes the partner rows (copies): tables are consumed, nothing is drawn
    sg.enable_bcr(every=every, policy="", seed=13)
    state = sg.bcr.stage.generator.get_state()
    assert sg._stage_draws(sg.bcr.stage) == 2 * sum(schedule(k, every)) and not sg._stage_row_draw(sg.bcr.stage, 4, 16, 12).any()
    assert torch.equal(sg.bcr.stage.generator.get_state(), state)
    sg.disable_bcr()
    assert sg._drawing_stages() == sg._stages()


# ---- the object, the trainer's interface ----------------------------------------------------------------------------------------------
def test_validation_fingerprint_and_state_dict_without_a_record():
    from srgan_amd.consistency import BalancedCR
    for bad, what in ((dict(lambda_real=-1.0), "lambda_real"), (dict(lambda_fake=float("nan")), "lambda_fake"),
                      (dict(lambda_real=float("inf")), "lambda_real"), (dict(every=0), "every"), (dict(every=1.5), "every"),
                      (dict(every=True), "every")):
        with pytest.raises(ValueError, match=what):
            BalancedCR(**bad)
    a = BalancedCR(2.0, 3.0, every=2, policy="flip", translation=0.25, seed=4)
    fp = a.fingerprint()
    a.set_weights(5.0, 0.0)
    assert a.fingerprint() == fp and (a.lambda_real, a.lambda_fake) == (5.0, 0.0)        # the weights are device state
    assert BalancedCR(2.0, 3.0, every=2, policy="flip", translation=0.25, seed=4).fingerprint() != fp     # another object
    a.stage.draw_fn = lambda n, h, w: torch.zeros(n, 8)
    assert a.fingerprint() != fp                                                          # the draw source is baked in
    assert a.graph_keepalive() == [] and a.state is None
    assert a.stats() == dict(lambda_real=5.0, lambda_fake=0.0, every=2, cr_real=0.0, cr_fake=0.0, updates=0)
    sd = a.state_dict()
    assert {k: v for k, v in sd.items() if k != "generator"} == dict(lambda_real=5.0, lambda_fake=0.0, every=2, policy="flip",
                                                                     translation=0.25, updates=0)
    b = BalancedCR(every=2, seed=99)
    b.load_state_dict(sd)
    assert b.stage.policy == "flip" and b.stage.translation == 0.25 and (b.lambda_real, b.lambda_fake) == (5.0, 0.0)
    assert torch.equal(b.stage.generator.get_state(), a.stage.generator.get_state()) and b.state is None
    with pytest.raises(ValueError, match="every"):
        BalancedCR(every=1).load_state_dict(sd)
    with pytest.raises(ValueError, match="without a device"):
        b.set_updates(3)
    with pytest.raises(ValueError, match=">= 0"):
        b.set_updates(-1)


def test_trainer_api_without_a_gpu(monkeypatch):
    from srgan_amd import consistency, dp, trainer
    sg = _cpu_trainer()
    assert sg.bcr is None and sg.bcr_stats() is None and "bcr" not in sg._ckpt_sections()
    with pytest.raises(RuntimeError, match="enable_bcr"):
        sg.set_bcr_weights(1.0, 1.0)
    sg.enable_diffaugment(seed=1)
    sg.enable_r1()
    n_ext = len(sg._extensions())
    assert sg.enable_bcr(lambda_real=2.0, lambda_fake=3.0, every=2, policy="flip", translation=0.2, seed=1) is sg
    assert isinstance(sg.bcr, consistency.BalancedCR) and sg._extensions()[-1] is sg.bcr and len(sg._extensions()) == n_ext + 1
    assert sg.bcr_stats() == dict(lambda_real=2.0, lambda_fake=3.0, every=2, cr_real=0.0, cr_fake=0.0, updates=0)
    sg.set_bcr_weights(0.5, 0.0)
    assert (sg.bcr.lambda_real, sg.bcr.lambda_fake) == (0.5, 0.0)
    assert "bcr" in sg._ckpt_sections()
    for bad in (dict(lambda_real=-1.0), dict(every=0), dict(policy="cutout"), dict(translation=-1.0)):
        with pytest.raises(ValueError):
            sg.enable_bcr(**bad)
    sg.disable_bcr()
    assert sg.bcr is None and len(sg._extensions()) == n_ext
    # more than one rank, the generic discriminator path: each names its way out
    monkeypatch.setattr(dp, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match=r"2 ranks.*disable_bcr"):
        sg.enable_bcr()
    monkeypatch.undo()
    assert sg.bcr is None
    sg._fused_paths = lambda: False
    with pytest.raises(NotImplementedError, match=r"fused discriminator pass.*disable_bcr"):
        sg.enable_bcr()
    assert sg.bcr is None
    with pytest.raises(NotImplementedError, match="SRGAN_training.enable_bcr"):
        trainer.SingleGAN_training.enable_bcr(object())


def test_checkpoint_section_round_trips_through_weights_only():
    sg = _cpu_trainer()
    sg.opt_sche_initialization()
    sg.enable_bcr(lambda_real=2.0, lambda_fake=3.0, every=2, policy="translation", translation=0.2, seed=6)
    sg.bcr.stage.draw(4, 16, 16)                                 # the generator has moved
    sd = sg.state_dict()
    assert {k: v for k, v in sd["bcr"].items() if k != "generator"} == dict(lambda_real=2.0, lambda_fake=3.0, every=2,
                                                                            policy="translation", translation=0.2, updates=0)
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    back = torch.load(buf, map_location="cpu", weights_only=True)
    assert torch.equal(back["bcr"]["generator"], sg.bcr.stage.generator.get_state())
    other = _cpu_trainer()
    other.opt_sche_initialization()
    with pytest.raises(ValueError, match="unexpected|missing"):
        other.enable_bcr().load_state_dict({k: v for k, v in back.items() if k != "bcr"})
    other.disable_bcr()
    rep = other.load_state_dict(back)                            # the section enables the feature with its saved settings
    assert rep.missing == [] and rep.unexpected == []
    assert other.bcr is not None and other.bcr.every == 2 and other.bcr.stage.policy == "translation" and other.bcr.stage.translation == 0.2
    assert (other.bcr.lambda_real, other.bcr.lambda_fake) == (2.0, 3.0)
    assert torch.equal(other.bcr.stage.draw(4, 16, 16), sg.bcr.stage.draw(4, 16, 16))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_back_before_any_launch(lib):
    buf = (ctypes.c_char * 4096)()
    b = ctypes.byref(buf)
    nan, inf = float("nan"), float("inf")
    assert lib.srgan_cr_state_bytes() == 32
    for lr, lf, every in ((-1.0, 1.0, 1), (1.0, -1.0, 1), (nan, 1.0, 1), (1.0, nan, 1), (inf, 1.0, 1), (1.0, inf, 1), (1.0, 1.0, 0),
                          (1.0, 1.0, -2)):
        assert lib.srgan_cr_state_init(b, lr, lf, every, None) == -1 and "cr_state_init" in _err(lib), (lr, lf, every)
        assert lib.srgan_cr_state_set(b, lr, lf, every, None) == -1 and "cr_state_set" in _err(lib), (lr, lf, every)
    assert lib.srgan_cr_state_init(None, 1.0, 1.0, 1, None) == -1 and "cr_state_init" in _err(lib)
    assert lib.srgan_cr_state_set(None, 1.0, 1.0, 1, None) == -1 and "cr_state_set" in _err(lib)
    assert lib.srgan_cr_state_set_updates(None, 0, None) == -1 and "cr_state_set_updates" in _err(lib)
    assert lib.srgan_cr_state_set_updates(b, -1, None) == -1 and "updates >= 0" in _err(lib)
    # the pair builder
    p = [ctypes.c_void_p(0x10000000 + (i << 24)) for i in range(4)]          # x0, x1, table, y: far apart
    pairs = lib.srgan_cr_pairs_fwd

    def call(x0=p[0], n0=2, x1=p[1], n1=2, table=p[2], y=p[3], c=3, h=8, w=8, flags=3):
        return pairs(x0, n0, x1, n1, table, y, c, h, w, flags, None)

    assert call(c=4) == -1 and "C = 4" in _err(lib)
    for name in ("x0", "table", "y"):
        assert call(**{name: None}) == -1 and "null pointer" in _err(lib), name
    assert call(x1=None) == -1 and "null pointer" in _err(lib)               # rows without a source
    assert call(n1=0) == -1 and "null pointer" in _err(lib)                  # a source without rows
    for bad in (dict(n0=0), dict(n0=-1), dict(n1=-1, x1=None), dict(h=0), dict(w=-3), dict(h=1 << 15, w=1 << 15)):
        assert call(**bad) == -1 and "n0 = " in _err(lib), bad
    for flags in (4, 8, -1):
        assert call(flags=flags) == -1 and f"flags = {flags}" in _err(lib)
    assert call(x0=ctypes.c_void_p(0x10000002)) == -1 and "aligned" in _err(lib)
    assert call(y=p[0]) == -1 and "alias" in _err(lib)
    assert call(y=p[1]) == -1 and "alias" in _err(lib)
    assert call(y=ctypes.c_void_p(p[0].value + 16)) == -1 and "alias" in _err(lib)           # overlapping, not equal
    assert call(y=ctypes.c_void_p(p[1].value - 16)) == -1 and "alias" in _err(lib)
    # the fused loss
    maps = (ctypes.c_void_p * 5)(*[0x20000000 + (i << 20) for i in range(5)])
    per = (ctypes.c_longlong * 5)(16, 4, 4, 4, 4)
    lab = ctypes.c_void_p(0x30000000)
    vals = ctypes.c_void_p(0x31000000)
    fn = lib.srgan_d_losses_cr

    def loss(o=maps, per_row=per, z=None, S=2, rows=8, rows_first=2, nc=4, label=lab, gk=0, ck=0, v=vals, d_o=maps, dz=None, pairs=4,
             pairs_first=2, state=b):
        return fn(o, per_row, z, S, rows, rows_first, nc, label, 1.0, 0.0, 1.0, gk, ck, v, d_o, dz, pairs, pairs_first, state, None)

    for name in ("o", "per_row", "v", "d_o", "state"):
        assert loss(**{name: None}) == -1 and "null pointer" in _err(lib), name
    assert loss(S=0) == -1 and "0 scales" in _err(lib)
    assert loss(S=5) == -1 and "5 scales" in _err(lib)
    assert loss(gk=2) == -1 and "gan_kind" in _err(lib)
    assert loss(ck=-1) == -1 and "class_kind" in _err(lib)
    assert loss(pairs=0, rows=0) == -1 and "pairs = 0" in _err(lib)
    assert loss(pairs=cc.MAX_PAIRS + 1, rows=2 * cc.MAX_PAIRS + 2) == -1 and f"pairs = {cc.MAX_PAIRS + 1} (1..{cc.MAX_PAIRS}" in _err(lib)
    assert loss(rows=7) == -1 and "rows = 7" in _err(lib)
    assert loss(rows=4) == -1 and "rows = 4" in _err(lib)                    # rows is the whole map, 2 * pairs
    assert loss(pairs_first=5) == -1 and "pairs_first = 5" in _err(lib)
    assert loss(pairs_first=-1) == -1 and "pairs_first = -1" in _err(lib)
    assert loss(rows_first=5) == -1 and "rows_first = 5" in _err(lib)
    assert loss(rows_first=-1) == -1 and "rows_first = -1" in _err(lib)
    per0 = (ctypes.c_longlong * 2)(16, 0)
    assert loss(per_row=per0) == -1 and "null scale" in _err(lib)
    perbig = (ctypes.c_longlong * 2)(16, 1 << 29)
    assert loss(per_row=perbig) == -1 and "2^31" in _err(lib)
    maps0 = (ctypes.c_void_p * 2)(0x20000000, 0)
    assert loss(o=maps0) == -1 and "null scale" in _err(lib)
    assert loss(z=maps, dz=None) == -1 and "class head" in _err(lib)
    assert loss(z=maps, dz=maps, label=None) == -1 and "class head" in _err(lib)
    assert loss(z=maps, dz=maps, nc=17) == -1 and "class head" in _err(lib)
    assert loss(z=maps, dz=maps, rows_first=0) == -1 and "class head" in _err(lib)


# ---- the term acts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 2])
def test_at_the_gpu_tests_weight_the_oracles_discriminator_leaves_the_plain_one(every):
    """tests/test_cr_train_gpu.py asks that the HIP step's D differs from the plain HIP step's by more than close_params; that can
    only hold if the oracle's own two steps do.  Tier T, batch 4, k 2, 128 x 128, the weight and the seeds of that test."""
    from oracle import trainer as otrainer
    from tests import r1_common as rc
    from tests.common import close_params, oracle_params
    B, K, SIZE = 4, 2, 128
    x, label = otrainer.synthetic_batch(B, SIZE, 4, seed=42)
    PG, PD, PE = oracle_params("T")
    torch.manual_seed(5)
    plain = otrainer.SRGANOracle(PG, PD, PE, otrainer.DEFAULT_LBD, K, np.eye(4), B, "mu", 8)
    ref = plain.train(x, label)
    torch.manual_seed(5)
    orc = cc.CROracle(PG, PD, PE, otrainer.DEFAULT_LBD, K, np.eye(4), B, "mu", 8, lambda_real=cc.LAMBDA_ACTS,
                      lambda_fake=cc.LAMBDA_ACTS, every=every, seed=cc.CR_SEED)
    out = orc.train(x, label)
    assert float(out[1]) == float(ref[1])                     # errD of the first update: before any penalised gradient is used
    assert len(orc.trace["errD_cr"]) == len([i for i in range(K) if i % every == 0])
    assert all(a > 0 and b > 0 for a, b in orc.trace["errD_cr"])
    moved = []
    for key in rc.all_weight_keys(PD):
        try:
            close_params(orc.D[key], plain.D[key], 1e-4, K, what=key)
        except AssertionError:
            moved.append(key)
    assert moved, "the oracle's regularised step left D within close_params of its plain step: choose a larger weight"
