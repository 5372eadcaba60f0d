"""CPU: the parts of mode-seeking regularisation (srgan_amd.diversity, csrc/diversity.hip, SRGAN_training.enable_mode_seeking) that
need no GPU -- the yardsticks of tests/ms_common.py against torch autograd, the case list against the constants of diversity.hip,
the float32 emulation of the kernel's summation order against the derived bounds, validation, the trainer's interface and refusals,
the checkpoint section, the C ABI's argument checks, and the oracle-side conditions of the GPU train test (weight 0 is the plain
oracle, the pinned weight acts, the oracle's own float32 deviation of the term)."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

from tests import ms_common as mc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from srgan_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.srgan_last_error().decode()


SMALL = [c for c in mc.CASES if c[0] * c[1] <= 1 << 16]


def _tau_for(form, inp):
    return mc.dsgan_tau(*inp) if form == "dsgan" else None


# ---- the yardsticks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("case", SMALL, ids=str)
def test_yardsticks_equal_torch_autograd_at_float64(case, form):
    """value and both gradients of ref64 / grads64 against autograd of the textbook forms (msgan: 1 / (dI / dz + eps))"""
    B, E, d = case
    inp = mc.random_inputs(B, E, d, seed=1)
    tau = _tau_for(form, inp)
    ref = mc.ref64(*inp, form, weight=1.0, eps=1e-5, tau=tau)
    i1, i2, z1, z2 = (torch.tensor(a, dtype=torch.float64) for a in inp)
    i1.requires_grad_(True)
    i2.requires_grad_(True)
    z1.requires_grad_(True)
    val = mc.torch_ms(i1, i2, z1, z2, form, float(np.float32(1e-5)), tau)
    assert abs(float(val) - ref["ms"]) <= 1e-12 * abs(ref["ms"])
    g1, g2 = torch.autograd.grad(val, [i1, i2])
    d1, d2 = mc.grads64(inp[0], inp[1], ref["coef"])
    scale = max(float(np.abs(d1).max()), 1e-300)
    assert float(np.abs(g1.numpy() - d1).max()) <= 1e-11 * scale and float(np.abs(g2.numpy() - d2).max()) <= 1e-11 * scale
    if form == "dsgan" and B > 1:
        assert 0 < int((ref["coef"] != 0).sum()) < B            # the clamp takes some rows and leaves some
        assert mc.mask_is_stable(ref, tau)


def test_yardstick_edge_rules():
    i1, i2, z1, z2 = mc.quantised_inputs(3, 16, 4, seed=2)
    # msgan: z1 == z2 -> 0 with zero gradients; I1 == I2 -> 1 / eps, finite, zero gradient through sign(0)
    r = mc.ref64(i1, i2, z1, z1, "msgan")
    assert r["ms"] == 0.0 and not r["coef"].any()
    r = mc.ref64(i1, i1, z1, z2, "msgan", eps=0.5)
    assert r["ms"] == 2.0 and np.isfinite(r["coef"]).all() and not np.any(mc.grads64(i1, i1, r["coef"])[0])
    # dsgan: a row with t_i = 0 contributes -tau / B with a zero coefficient; r_i == tau is kept (<=, torch.clamp's mask)
    z2b = z2.copy()
    z2b[1] = z1[1]
    r = mc.ref64(i1, i2, z1, z2b, "dsgan", tau=1e9)
    assert r["coef"][1] == 0.0 and r["terms"][1] == float(np.float32(1e9)) and r["coef"][0] != 0
    a = np.zeros((3, 8), np.float32)
    b = a.copy()
    b[0, :2], b[1, :4], b[2, :6] = 1.0, 1.0, 1.0                         # s = 2, 4, 6 -> s / E = 0.25, 0.5, 0.75
    p, q = np.zeros((3, 2), np.float32), np.ones((3, 2), np.float32)     # t / d = 1
    r = mc.ref64(a, b, p, q, "dsgan", tau=0.5)
    assert r["r"].tolist() == [0.25, 0.5, 0.75] and (r["coef"] != 0).tolist() == [True, True, False]
    ta = torch.tensor(a, dtype=torch.float64, requires_grad=True)
    mc.torch_ms(ta, torch.tensor(b, dtype=torch.float64), torch.tensor(p), torch.tensor(q), "dsgan", tau=0.5).backward()
    assert (ta.grad.abs().sum(1) != 0).tolist() == [True, True, False]   # torch.clamp keeps the row AT tau


# ---- the case list against the kernel's constants ----------------------------------------------------------------------------------------
def test_case_list_is_chosen_against_the_constants_of_diversity_hip():
    src = open(os.path.join(HERE, "..", "style-restricted_gan_amd", "csrc", "diversity.hip")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr int (kMs\w+) = (\d+);", src)}
    assert const == dict(kMsBlock=mc.BLOCK, kMsChunk=mc.CHUNK, kMsRowsPerItem=mc.ROWS_PER_ITEM, kMsGridCap=mc.GRID_CAP)
    assert "#pragma clang fp contract(off)" in src
    assert mc.CHUNK == 16 * mc.BLOCK and mc.DEPTH == 16 + 6 + 2        # 16 slots per thread, 64 lanes, 4 waves
    E = sorted({c[1] for c in mc.CASES})
    assert {1, 63, 64, 65, 105, 3 * 33 * 31, mc.CHUNK, mc.CHUNK + 1, 3 * 128 * 128} <= set(E)
    assert {1, 2, 5, 33} <= {c[0] for c in mc.CASES} and any(c[0] > mc.BLOCK for c in mc.CASES)
    assert {1, 8, 67} <= {c[2] for c in mc.CASES}
    assert mc.n_items(1, mc.CHUNK) == 1 and mc.n_items(1, mc.CHUNK + 1) == 2
    B, Eg, _ = mc.GRID_STRIDE_CASE
    assert mc.GRID_CAP < mc.n_items(B, Eg) <= 2 * mc.GRID_CAP            # the grid-stride loop runs more than once
    assert all(mc.n_items(b, e) <= mc.GRID_CAP for b, e, _ in mc.CASES[:-1])
    for b, e, _ in mc.MISALIGNED:
        assert e % 2 == 1 and (b * e) % 4 != 0                           # rows [B, 2B) of a 3B tensor: 4-byte aligned only


# ---- the emulation meets the derived bounds ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "cloud", "one_pixel"])
@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("case", mc.CASES[:-1], ids=str)
def test_float32_emulation_of_the_kernels_order_meets_the_bounds(case, form, kind):
    B, E, d = case
    inp = mc.random_inputs(B, E, d, kind, seed=3)
    tau = _tau_for(form, inp)
    ref = mc.ref64(*inp, form, weight=2.5, eps=1e-5, tau=tau)
    if form == "dsgan" and not mc.mask_is_stable(ref, tau):
        pytest.fail("the case's tau sits within the error of a ratio: dsgan_tau must choose another")
    emu = mc.emulate(*inp, form, weight=2.5, eps=1e-5, tau=tau)
    bnd = mc.bounds(ref, form)
    worst = 0.0
    for name in ("s", "d_image", "d_latent", "ms", "weighted", "coef"):
        err, lim = np.abs(np.asarray(emu[name]) - np.asarray(ref[name])), np.asarray(bnd[name])
        assert np.all(err <= lim), (name, float(np.max(err - lim)))
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(lim > 0, err / lim, 0.0))))
    print(f"{case} {form} {kind}: worst error / bound = {worst:.3f}")


def test_emulation_is_exact_on_quantised_inputs():
    for B, E, d in SMALL:
        inp = mc.quantised_inputs(B, E, d, seed=4)
        for form in mc.FORMS:
            ref, emu = mc.ref64(*inp, form, weight=0.5, tau=1.0), mc.emulate(*inp, form, weight=0.5, tau=1.0)
            assert np.array_equal(emu["s"], ref["s"]) and np.array_equal(emu["t"], ref["t"])
            for name in ("ms", "d_image", "d_latent", "weighted", "coef"):
                assert np.array_equal(np.asarray(ref[name], np.float32), np.asarray(emu[name], np.float32)), (B, E, d, form, name)


# ---- the object ------------------------------------------------------------------------------------------------------------------------
def test_validation_fingerprint_and_state_dict_without_a_record():
    from srgan_amd.diversity import ModeSeeking
    for bad, what in ((dict(weight=-1.0), "weight"), (dict(weight=float("nan")), "weight"), (dict(weight=float("inf")), "weight"),
                      (dict(weight="much"), "weight"), (dict(eps=0.0), "eps"), (dict(eps=-1e-5), "eps"), (dict(form="hinge"), "form"),
                      (dict(form="dsgan"), "tau"), (dict(form="dsgan", tau=-1.0), "tau"), (dict(tau=float("nan")), "tau"),
                      (dict(weight=True), "weight")):
        with pytest.raises(ValueError, match=what):
            ModeSeeking(**bad)
    a = ModeSeeking(2.0, "dsgan", 1e-4, tau=3.0, seed=4)
    fp = a.fingerprint()
    a.set_weight(5.0)
    assert a.fingerprint() == fp and a.weight == 5.0                    # the weight is device state
    assert ModeSeeking(5.0, "dsgan", 1e-4, tau=3.0, seed=4).fingerprint() != fp           # another object
    assert a.graph_keepalive() == [] and a.state is None
    assert a.stats() == dict(weight=5.0, form="dsgan", eps=1e-4, tau=3.0, ms=0.0, d_image=0.0, d_latent=0.0, updates=0)
    z = a.draw(4, 8)
    assert z.shape == (4, 8) and z.dtype == torch.float32
    assert torch.equal(z, torch.randn(4, 8, generator=torch.Generator().manual_seed(4)))
    sd = a.state_dict()
    assert {k: v for k, v in sd.items() if k != "generator"} == dict(weight=5.0, form="dsgan", eps=1e-4, tau=3.0, updates=0, ms=0.0,
                                                                     d_image=0.0, d_latent=0.0)
    b = ModeSeeking(form="dsgan", tau=1.0, seed=99)
    b.load_state_dict(sd)
    assert (b.weight, b.eps, b.tau) == (5.0, 1e-4, 3.0) and b.state is None
    assert torch.equal(b.draw(4, 8), a.draw(4, 8))
    with pytest.raises(ValueError, match="form"):
        ModeSeeking().load_state_dict(sd)
    with pytest.raises(ValueError, match="without a device"):
        b.load_state_dict(dict(sd, updates=3))
    a.draw_fn = lambda n, ndim: torch.zeros(n, ndim)
    assert a.fingerprint() != fp                                        # the draw source is baked in


def _cpu_trainer(k=2, norm="instance"):
    from srgan_amd import model, trainer
    D = model.SingleDiscriminator_solo_multi(3, 4, 2, 4, "instance", 4)
    G = model.SingleGenerator(3, 4, 2, 2, 1, norm, num_con=12)
    E = model.Encoder(3, 8, 4, 4, "instance", 4, "cpu")
    lbd = dict(**{"class": 1.0}, cycle=5.0, idt=5.0, reg=0.5, idt_reg=0.5, KL=0.0, batch_KL=10.0, corr_enc=100.0, hist=0.0)
    crit = [torch.nn.MSELoss(), torch.nn.MSELoss()]
    return trainer.SRGAN_training([G, D, E], [None, None, None], crit, lbd, k, "cpu", np.eye(4), batch_size=4, encoded_feature="mu",
                                  ndim=8)


def test_trainer_api_without_a_gpu(monkeypatch):
    from srgan_amd import diversity, dp, trainer
    sg = _cpu_trainer()
    assert sg.mode_seeking_stats() is None and "mode_seeking" not in sg._ckpt_sections()
    assert sg._drawing_stages() == [] and "mode_seeking" not in sg.state_dict(rng=False)
    with pytest.raises(RuntimeError, match="enable_mode_seeking"):
        sg.set_mode_seeking_weight(1.0)
    sg.enable_r1()
    sg.enable_bcr(seed=1)
    n_ext = len(sg._extensions())
    assert sg.enable_mode_seeking(weight=2.0, form="dsgan", eps=1e-4, tau=7.0, seed=1) is sg
    ext = sg._extensions()
    assert isinstance(ext[-1], diversity.ModeSeeking) and ext[-2] is sg.bcr and len(ext) == n_ext + 1      # a fixed position, after bcr
    assert sg.mode_seeking_stats() == dict(weight=2.0, form="dsgan", eps=1e-4, tau=7.0, ms=0.0, d_image=0.0, d_latent=0.0, updates=0)
    sg.set_mode_seeking_weight(0.5)
    assert sg.mode_seeking_stats()["weight"] == 0.5
    assert "mode_seeking" in sg._ckpt_sections() and sg._ckpt_sections().index("mode_seeking") == sg._ckpt_sections().index("bcr") + 1
    # one draw per step, [B, ndim], staged beside the stages' tables under its own name; the default generator is not touched
    ms = ext[-1]
    assert sg._drawing_stages()[-1] is ms and sg._stage_draws(ms) == 1 and ms.section == "mode_seeking"
    before = torch.get_rng_state()
    row = sg._stage_row_draw(ms, 4, 16, 16)
    assert row.shape == (4, 8) and torch.equal(torch.get_rng_state(), before)
    assert torch.equal(row, torch.randn(4, 8, generator=torch.Generator().manual_seed(1)))
    for bad in (dict(weight=-1.0), dict(form="dsgan"), dict(eps=0.0), dict(form="other")):
        with pytest.raises(ValueError):
            sg.enable_mode_seeking(**bad)
    assert sg._extensions()[-1] is ms                                   # a refused call leaves what was there
    sg.disable_mode_seeking()
    assert sg.mode_seeking_stats() is None and len(sg._extensions()) == n_ext and "errG_ms" not in sg.loss_terms
    # refusals: each names its way out
    monkeypatch.setattr(dp, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match=r"2 ranks.*disable_mode_seeking"):
        sg.enable_mode_seeking()
    monkeypatch.undo()
    assert sg.mode_seeking_stats() is None
    bn = _cpu_trainer(norm="batch")
    with pytest.raises(NotImplementedError, match=r"batch statistics.*disable_mode_seeking"):
        bn.enable_mode_seeking()
    assert bn.mode_seeking_stats() is None
    with pytest.raises(NotImplementedError, match="SRGAN_training.enable_mode_seeking"):
        trainer.SingleGAN_training.enable_mode_seeking(object())


def test_checkpoint_section_round_trips_through_weights_only():
    sg = _cpu_trainer()
    sg.opt_sche_initialization()
    sg.enable_mode_seeking(weight=2.0, form="dsgan", eps=1e-4, tau=7.0, seed=6)
    sg._ms.draw(4, 8)                                                   # the generator has moved
    sd = sg.state_dict()
    assert list(sd).index("mode_seeking") > list(sd).index("optE")
    assert {k: v for k, v in sd["mode_seeking"].items() if k != "generator"} == dict(weight=2.0, form="dsgan", eps=1e-4, tau=7.0,
                                                                                    updates=0, ms=0.0, d_image=0.0, d_latent=0.0)
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    back = torch.load(buf, map_location="cpu", weights_only=True)
    assert torch.equal(back["mode_seeking"]["generator"], sg._ms.generator.get_state())
    other = _cpu_trainer()
    other.opt_sche_initialization()
    other.enable_mode_seeking()
    rep = other.load_state_dict({k: v for k, v in back.items() if k != "mode_seeking"}, strict=False)
    assert rep.missing == ["mode_seeking"]                              # a checkpoint without the section: the feature stays on, fresh
    with pytest.raises(ValueError, match="missing"):
        other.load_state_dict({k: v for k, v in back.items() if k != "mode_seeking"})
    other.disable_mode_seeking()
    rep = other.load_state_dict(back)                                   # the section enables the feature with its saved settings
    assert rep.missing == [] and rep.unexpected == []
    st = other.mode_seeking_stats()
    assert (st["weight"], st["form"], st["eps"], st["tau"]) == (2.0, "dsgan", 1e-4, 7.0)
    assert torch.equal(other._ms.draw(4, 8), sg._ms.draw(4, 8))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_back_before_any_launch(lib):
    buf = (ctypes.c_char * 4096)()
    b = ctypes.byref(buf)
    nan, inf = float("nan"), float("inf")
    assert lib.srgan_ms_state_bytes() == 32
    for w, eps, tau in ((-1.0, 1e-5, 0.0), (nan, 1e-5, 0.0), (inf, 1e-5, 0.0), (1.0, 0.0, 0.0), (1.0, nan, 0.0), (1.0, 1e-5, -1.0),
                        (1.0, 1e-5, nan), (1.0, 1e-5, inf)):
        assert lib.srgan_ms_state_init(b, w, eps, tau, None) == -1 and "ms_state_init" in _err(lib), (w, eps, tau)
        assert lib.srgan_ms_state_set(b, w, eps, tau, None) == -1 and "ms_state_set" in _err(lib), (w, eps, tau)
    assert lib.srgan_ms_state_init(None, 1.0, 1e-5, 0.0, None) == -1 and lib.srgan_ms_state_set(None, 1.0, 1e-5, 0.0, None) == -1
    assert lib.srgan_ms_state_restore(None, 0, 0.0, 0.0, 0.0, None) == -1 and "ms_state_restore" in _err(lib)
    assert lib.srgan_ms_state_restore(b, -1, 0.0, 0.0, 0.0, None) == -1 and "updates >= 0" in _err(lib)
    assert lib.srgan_ms_workspace(0, 8) == 0 and lib.srgan_ms_workspace(2, 0) == 0 and lib.srgan_ms_workspace(2, 1 << 31) == 0
    assert lib.srgan_ms_workspace(3, mc.CHUNK + 1) == 3 * 2 * 4 + 2 * 3 * 8
    assert lib.srgan_ms_workspace(3, 5) == 16 + 2 * 3 * 8               # the partials rounded up to 8 bytes
    p = [ctypes.c_void_p(0x10000000 + (i << 24)) for i in range(8)]
    odd = ctypes.c_void_p(0x10000002)
    rows, fin, grad = lib.srgan_ms_rows, lib.srgan_ms_finish, lib.srgan_ms_grad
    assert rows(None, p[1], 2, 8, p[2], 64, None) == -1 and "null pointer" in _err(lib)
    assert rows(p[0], p[1], 2, 8, None, 64, None) == -1 and "null pointer" in _err(lib)
    assert rows(p[0], p[1], 0, 8, p[2], 64, None) == -1 and "geometry" in _err(lib)
    assert rows(p[0], p[1], 2, 8, p[2], 4, None) == -1 and "workspace" in _err(lib)
    assert rows(odd, p[1], 2, 8, p[2], 64, None) == -1 and "aligned" in _err(lib)
    assert rows(p[0], p[1], 2, 8, ctypes.c_void_p(0x12000004), 64, None) == -1 and "aligned" in _err(lib)

    def finish(ws=p[2], nb=1 << 16, z1=p[3], z2=p[4], bb=2, e=8, d=4, form=0, state=b, vals=p[5], coef=p[6]):
        return fin(ws, nb, z1, z2, bb, e, d, form, state, vals, coef, None)

    for name in ("ws", "z1", "z2", "state", "vals", "coef"):
        assert finish(**{name: None}) == -1 and "null pointer" in _err(lib), name
    assert finish(d=0) == -1 and "geometry" in _err(lib)
    assert finish(form=2) == -1 and "form = 2" in _err(lib)
    assert finish(nb=16) == -1 and "workspace" in _err(lib)
    assert finish(z1=odd) == -1 and "aligned" in _err(lib)

    def g(i1=p[0], i2=p[1], coef=p[6], gin=p[5], d1=p[3], d2=p[4], bb=2, e=8):
        return grad(i1, i2, coef, gin, d1, d2, bb, e, None)

    for name in ("i1", "i2", "coef", "gin"):
        assert g(**{name: None}) == -1 and "null pointer" in _err(lib), name
    assert g(d1=None, d2=None) == -1 and "null pointer" in _err(lib)
    assert g(d1=p[0]) == -1 and "alias" in _err(lib)
    assert g(d2=p[1]) == -1 and "alias" in _err(lib)
    assert g(d2=p[3]) == -1 and "alias" in _err(lib)
    assert g(d1=odd) == -1 and "aligned" in _err(lib)
    assert g(e=0) == -1 and "geometry" in _err(lib)


# ---- the oracle side of the GPU train test ---------------------------------------------------------------------------------------------
def _oracle(cls, **kw):
    from oracle import trainer as otrainer
    from tests.common import oracle_params
    B, K, SIZE = 4, 2, 128
    x, label = otrainer.synthetic_batch(B, SIZE, 4, seed=mc.TRAIN_BATCH_SEED)
    PG, PD, PE = oracle_params("T")
    torch.manual_seed(mc.TRAIN_SEED)
    orc = cls(PG, PD, PE, otrainer.DEFAULT_LBD, K, np.eye(4), B, "mu", 8, **kw)
    return orc, orc.train(x, label), K


@pytest.fixture(scope="module")
def plain_oracle():
    from oracle import trainer as otrainer
    orc, out, _ = _oracle(otrainer.SRGANOracle)
    return orc, out, torch.get_rng_state()


def test_weight_zero_is_the_plain_oracle_bit_for_bit(plain_oracle):
    plain, ref, rng_after = plain_oracle
    orc, out, _ = _oracle(mc.MSOracle, weight=0.0, seed=mc.MS_SEED)
    assert torch.equal(torch.get_rng_state(), rng_after)                # the term draws from its own generator
    assert [float(v) for v in out] == [float(v) for v in ref]
    for mine, theirs in ((orc.G, plain.G), (orc.D, plain.D), (orc.E, plain.E)):
        for k in theirs:
            assert torch.equal(mine[k], theirs[k]), k
    assert orc.trace["ms"] > 0 and orc.trace["d_image"] > 0 and orc.trace["d_latent"] > 0


@pytest.mark.parametrize("form", mc.FORMS)
def test_at_the_pinned_weight_the_term_acts_and_the_oracles_own_deviation_of_ms(plain_oracle, form):
    """tests/test_ms_train_gpu.py asks that the HIP step's G leaves the plain HIP step's by more than close_params; that can only hold
    if the oracle's own two steps do.  And the oracle's float32 value of the term against a float64 re-run of the two translations:
    the tolerance of errG_ms in the train test follows from it (below 1e-4 relative: the project's 1e-3)."""
    from tests.common import close_params
    plain, ref, _ = plain_oracle
    tau = mc.DSGAN_TAU if form == "dsgan" else None
    orc, out, K = _oracle(mc.MSOracle, weight=mc.LAMBDA_ACTS[form], form=form, tau=tau, seed=mc.MS_SEED)
    assert [float(v) for v in out][1:] == [float(v) for v in ref][1:]   # errD and errE: before any gradient of the term is used
    assert float(out[1]) == float(ref[1])
    for k in plain.D:
        assert torch.equal(orc.D[k], plain.D[k]), k                     # the term never reaches D
    moved = []
    for key in orc.G:
        try:
            close_params(orc.G[key], plain.G[key], 1e-4, 2, what=key)
        except AssertionError:
            moved.append(key)
    assert moved, "the oracle's regularised step left G within close_params of its plain step: choose a larger weight"
    dev = abs(orc.trace["ms"] - orc.trace["ms64"]) / abs(orc.trace["ms64"])
    print(f"{form}: ms {orc.trace['ms']:.9g} float64 {orc.trace['ms64']:.9g} relative deviation {dev:.3e}; "
          f"d_image {orc.trace['d_image']:.6g} d_latent {orc.trace['d_latent']:.6g}")
    assert dev < 1e-4 and mc.ERRG_MS_RTOL == 1e-3
    if form == "dsgan":
        assert -orc.trace["ms"] < mc.DSGAN_TAU / 10                     # no row is clamped at the train test's tau
