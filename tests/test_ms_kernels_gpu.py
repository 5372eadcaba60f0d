"""GPU: the three kernels of csrc/diversity.hip through ctypes on guarded memory (tests/eval_common.Arena: pattern bytes in front of and
behind every buffer), held to the float64 yardsticks of tests/ms_common.py within the bounds derived there from the kernel's summation
order -- exactly where the inputs make every sum exact -- plus ``ops.mode_seeking`` / ``ops.rowwise_l1`` on top of them.  Worst error /
bound is printed per case."""
import ctypes
import struct

import numpy as np
import pytest
import torch

from tests import ms_common as mc
from tests.eval_common import Arena

pytestmark = pytest.mark.gpu
FORM_ID = {"msgan": 0, "dsgan": 1}


@pytest.fixture(scope="module")
def lib():
    from srgan_amd import _lib
    return _lib.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _record(state):
    w, eps, tau, ms, wd, di, dz, updates = struct.unpack("fffffffi", state.cpu().numpy().tobytes())
    return dict(weight=w, eps=eps, tau=tau, ms=ms, weighted=wd, d_image=di, d_latent=dz, updates=updates)


class Run:
    """One scenario on guarded memory: the record, the workspace, the inputs (``sliced``: rows [B, 2B) of a 3B tensor), every output."""

    def __init__(self, lib, inp, form, weight=1.0, eps=1e-5, tau=None, g=1.0, need=(True, True), sliced=False, skew_out=0):
        from srgan_amd import _lib
        self.lib, self.check, self.form = lib, _lib.check, form
        i1, i2, z1, z2 = (np.ascontiguousarray(a, np.float32) for a in inp)
        self.B, self.E = i1.shape[0], int(np.prod(i1.shape[1:]))
        B, E = self.B, self.E
        ar = self.arena = Arena()
        if sliced:
            pad = lambda a: np.concatenate([np.full_like(a, 7.0), a, np.full_like(a, -7.0)], 0)
            self.i1, self.i2 = ar.put(pad(i1), "i1 (3B)")[B:2 * B], ar.put(pad(i2), "i2 (3B)")[B:2 * B]
            assert self.i1.data_ptr() % 16 != 0 or E % 4 != 0
        else:
            self.i1, self.i2 = ar.put(i1, "i1"), ar.put(i2, "i2")
        self.z1, self.z2 = ar.put(z1, "z1"), ar.put(z2, "z2")
        self.state = ar.raw(lib.srgan_ms_state_bytes(), "record")
        self.nb = lib.srgan_ms_workspace(B, E)
        assert self.nb > 0
        self.ws = ar.raw(self.nb, "workspace")
        self.vals, self.coef = ar.out((2,), "vals"), ar.out((B,), "coef")
        self.g = ar.put(np.array([g], np.float32), "incoming gradient")
        # an operand without a gradient gets no buffer; where it would have been stays a guarded, untouched region
        self.d = [None, None]
        self.hole = []
        for j in range(2):
            if need[j]:
                raw = ar.raw(B * E * 4, f"d{j + 1}", skew=skew_out)
                self.d[j] = raw.view(torch.float32).view(B, E)
            else:
                self.hole.append(ar.raw(B * E * 4, f"where d{j + 1} would be"))
        self.check(lib.srgan_ms_state_init(_p(self.state), weight, eps, 0.0 if tau is None else tau, None), "ms_state_init")

    def forward(self):
        lib, B, E = self.lib, self.B, self.E
        self.check(lib.srgan_ms_rows(_p(self.i1), _p(self.i2), B, E, _p(self.ws), self.nb, None), "ms_rows")
        self.check(lib.srgan_ms_finish(_p(self.ws), self.nb, _p(self.z1), _p(self.z2), B, E, self.z1.shape[1], FORM_ID[self.form],
                                       _p(self.state), _p(self.vals), _p(self.coef), None), "ms_finish")
        return self

    def backward(self):
        self.check(self.lib.srgan_ms_grad(_p(self.i1), _p(self.i2), _p(self.coef), _p(self.g), _p(self.d[0]), _p(self.d[1]), self.B,
                                          self.E, None), "ms_grad")
        return self

    def result(self):
        torch.cuda.synchronize()
        self.arena.intact(f"{self.form} B={self.B} E={self.E}")
        for h in self.hole:
            assert bool((h == 0xA5).all()), "bytes written where an absent gradient's buffer would be"
        nchunk = -(-self.E // mc.CHUNK)
        part = self.ws[:self.B * nchunk * 4].view(torch.float32).view(self.B, nchunk).cpu().numpy()
        rec = _record(self.state)
        vals = self.vals.cpu().numpy()
        return dict(part=part, s=part.astype(np.float64).sum(1), ms=float(vals[1]), weighted=float(vals[0]), d_image=rec["d_image"],
                    d_latent=rec["d_latent"], coef=self.coef.cpu().numpy(), record=rec,
                    d1=None if self.d[0] is None else self.d[0].cpu().numpy(), d2=None if self.d[1] is None else self.d[1].cpu().numpy())


def _tau_for(form, inp):
    return mc.dsgan_tau(*inp) if form == "dsgan" else None


def _within(got, ref, bnd, g, what):
    worst = 0.0
    for name in ("s", "d_image", "d_latent", "ms", "weighted", "coef"):
        err, lim = np.abs(np.asarray(got[name], np.float64) - np.asarray(ref[name])), np.asarray(bnd[name])
        assert np.all(err <= lim), (what, name, float(np.max(err - lim)))
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(lim > 0, err / lim, 0.0))))
    return worst


def _grads_within(got, inp, ref, bnd, g, what):
    d1, d2 = mc.grads64(inp[0], inp[1], ref["coef"], g)
    lim = bnd["grad"][:, None]
    worst = 0.0
    for name, want in (("d1", d1), ("d2", d2)):
        if got[name] is None:
            continue
        err = np.abs(got[name].astype(np.float64) - want)
        assert np.all(err <= lim), (what, name, float(np.max(err - lim)))
        assert np.array_equal(got[name] == 0, want == 0), (what, name, "sign(0) = 0")
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(lim > 0, err / lim, 0.0))))
    if got["d1"] is not None and got["d2"] is not None:
        assert np.array_equal(got["d2"], -got["d1"]), (what, "dI2 = -dI1 bit for bit")
    return worst


# ---- general inputs within the derived bounds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("case", mc.CASES, ids=str)
def test_random_inputs_within_the_derived_bounds(lib, case, form):
    B, E, d = case
    kinds = ("plain",) if case == mc.GRID_STRIDE_CASE else ("plain", "cloud", "one_pixel")
    for kind in kinds:
        inp = mc.random_inputs(B, E, d, kind, seed=3)
        tau = _tau_for(form, inp)
        ref = mc.ref64(*inp, form, weight=2.5, eps=1e-5, tau=tau)
        assert form == "msgan" or mc.mask_is_stable(ref, tau)
        got = Run(lib, inp, form, 2.5, 1e-5, tau, g=0.75).forward().backward().result()
        bnd = mc.bounds(ref, form, g=0.75)
        w1 = _within(got, ref, bnd, 0.75, (case, form, kind))
        w2 = _grads_within(got, inp, ref, bnd, 0.75, (case, form, kind))
        assert got["record"]["updates"] == 1 and got["record"]["ms"] == got["ms"] and got["record"]["weighted"] == got["weighted"]
        # the fixed order: the partial sums are those of the float32 emulation, bit for bit
        same = case == mc.GRID_STRIDE_CASE or np.array_equal(got["part"], mc.emulate_partials(inp[0], inp[1]))
        assert same, (case, form, kind, "the partial sums are not those of the stated order")
        print(f"{case} {form} {kind}: worst error / bound: values {w1:.3f}, gradients {w2:.3f}; partials equal the emulation: {same}")


# ---- exactness on quantised inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("case", mc.CASES[:-1], ids=str)
def test_quantised_inputs_are_exact(lib, case, form):
    """multiples of 1/8: every sum is exact, so ms, dI, dz and coef equal float64 rounded to fp32 and the gradients are bit-exact"""
    B, E, d = case
    inp = mc.quantised_inputs(B, E, d, seed=4)
    assert B * E < 64 or np.any(inp[0] == inp[1])       # zero differences occur
    ref = mc.ref64(*inp, form, weight=0.5, eps=2.0 ** -10, tau=1.0)
    got = Run(lib, inp, form, 0.5, 2.0 ** -10, 1.0, g=2.0).forward().backward().result()
    assert np.array_equal(got["s"], ref["s"])
    for name in ("ms", "weighted", "d_image", "d_latent", "coef"):
        assert np.array_equal(np.asarray(got[name], np.float32), np.asarray(ref[name], np.float32)), (name, got[name], ref[name])
    c32 = np.asarray(ref["coef"], np.float32)
    want = (np.float32(2.0) * c32)[:, None] * np.sign(inp[0].astype(np.float64) - inp[1]).astype(np.float32)
    assert np.array_equal(got["d1"], want) and np.array_equal(got["d2"], -want)
    assert not np.any(got["d1"][inp[0] == inp[1]])


# ---- misaligned operands -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("case", mc.MISALIGNED, ids=str)
def test_row_slices_of_a_larger_batch_with_odd_rows(lib, case, form):
    """operands are rows [B, 2B) of a 3B tensor, E odd: row bases 4-byte aligned only, a different misalignment per row; outputs
    skewed by 4 bytes; the same bits as the aligned call"""
    B, E, d = case
    inp = mc.quantised_inputs(B, E, d, seed=5)
    rnd = mc.random_inputs(B, E, d, seed=5)
    for data, tau in ((inp, 1.0), (rnd, _tau_for(form, rnd))):
        a = Run(lib, data, form, 1.5, 1e-5, tau).forward().backward().result()
        b = Run(lib, data, form, 1.5, 1e-5, tau, sliced=True, skew_out=4).forward().backward().result()
        for name in ("part", "coef", "d1", "d2"):
            assert np.array_equal(a[name], b[name]), name
        assert (a["ms"], a["weighted"], a["d_image"], a["d_latent"]) == (b["ms"], b["weighted"], b["d_image"], b["d_latent"])
    ref = mc.ref64(*inp, form, weight=1.5, tau=1.0)
    exact = Run(lib, inp, form, 1.5, 1e-5, 1.0, sliced=True, skew_out=4).forward().backward().result()
    assert np.array_equal(exact["s"], ref["s"]) and np.array_equal(exact["coef"], np.asarray(ref["coef"], np.float32))


# ---- the dsgan mask ------------------------------------------------------------------------------------------------------------------
def test_dsgan_mask_is_less_or_equal(lib):
    """rows with r_i == tau exactly and rows on either side: a `<` in place of `<=` gives the middle rows a zero coefficient"""
    B, E, d = 6, 64, 4
    a = np.zeros((B, E), np.float32)
    b = a.copy()
    for i, n in enumerate((8, 16, 24, 16, 15, 17)):
        b[i, :n] = 2.0                                   # s_i = 2 n, s_i / E = n / 32
    z1, z2 = np.zeros((B, d), np.float32), np.full((B, d), 0.5, np.float32)              # t_i / d = 0.5 -> r_i = n / 16
    tau = 1.0
    ref = mc.ref64(a, b, z1, z2, "dsgan", weight=1.0, tau=tau)
    assert ref["r"].tolist() == [0.5, 1.0, 1.5, 1.0, 0.9375, 1.0625]
    got = Run(lib, (a, b, z1, z2), "dsgan", 1.0, 1e-5, tau).forward().backward().result()
    assert (got["coef"] != 0).tolist() == [True, True, False, True, True, False]
    assert np.array_equal(got["coef"], np.asarray(ref["coef"], np.float32)) and got["ms"] == np.float32(ref["ms"])
    assert not got["d1"][2].any() and not got["d1"][5].any() and got["d1"][1, :16].all() and not got["d1"][1, 16:].any()


# ---- degenerate rows and inputs --------------------------------------------------------------------------------------------------------
def test_degenerate_rows_and_inputs(lib):
    B, E, d = 5, 105, 8
    i1, i2, z1, z2 = mc.quantised_inputs(B, E, d, seed=6)
    # dsgan rows with t_i == 0: clamped, -tau / B each, a zero gradient
    z2b = z2.copy()
    z2b[[1, 3]] = z1[[1, 3]]
    ref = mc.ref64(i1, i2, z1, z2b, "dsgan", weight=1.0, tau=4.0)
    got = Run(lib, (i1, i2, z1, z2b), "dsgan", 1.0, 1e-5, 4.0).forward().backward().result()
    assert got["ms"] == np.float32(ref["ms"]) and np.array_equal(got["coef"], np.asarray(ref["coef"], np.float32))
    assert not got["coef"][[1, 3]].any() and not got["d1"][[1, 3]].any() and np.isfinite(got["d1"]).all()
    for form in mc.FORMS:
        # I1 == I2 everywhere: msgan gives 1 / eps, finite; dsgan 0; zero gradients either way
        got = Run(lib, (i1, i1, z1, z2), form, 1.0, 2.0 ** -10, 4.0).forward().backward().result()
        assert got["ms"] == (1024.0 if form == "msgan" else 0.0) and got["d_image"] == 0.0
        assert not got["d1"].any() and not got["d2"].any() and np.isfinite(got["coef"]).all()
    # z1 == z2 everywhere in msgan: 0 with zero gradients and no NaN (also with I1 == I2: 0 / 0)
    for b in (i2, i1):
        got = Run(lib, (i1, b, z1, z1), "msgan", 3.0, 1e-5).forward().backward().result()
        assert got["ms"] == 0.0 and got["weighted"] == 0.0 and got["d_latent"] == 0.0
        assert not got["coef"].any() and not got["d1"].any() and not got["d2"].any()
        assert not np.isnan(got["d1"]).any() and not np.isnan(got["coef"]).any()


# ---- gradient plumbing -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", mc.FORMS)
def test_incoming_gradient_scales_both_gradients(lib, form):
    inp = mc.quantised_inputs(5, 4097, 8, seed=7)
    one = Run(lib, inp, form, 1.0, 1e-5, 1.0, g=1.0).forward().backward().result()
    for g in (-4.0, 0.5):
        got = Run(lib, inp, form, 1.0, 1e-5, 1.0, g=g).forward().backward().result()
        assert np.array_equal(got["d1"], np.float32(g) * one["d1"]) and np.array_equal(got["d2"], np.float32(g) * one["d2"])
        assert got["ms"] == one["ms"]


@pytest.mark.parametrize("need", [(True, False), (False, True)], ids=["only_i1", "only_i2"])
@pytest.mark.parametrize("form", mc.FORMS)
def test_one_operand_without_a_gradient_writes_nothing_for_it(lib, form, need):
    inp = mc.quantised_inputs(5, 4097, 8, seed=8)
    both = Run(lib, inp, form, 1.0, 1e-5, 1.0).forward().backward().result()
    got = Run(lib, inp, form, 1.0, 1e-5, 1.0, need=need).forward().backward().result()      # result() checks the hole and the guards
    for j, name in enumerate(("d1", "d2")):
        if need[j]:
            assert np.array_equal(got[name], both[name])
        else:
            assert got[name] is None


@pytest.mark.parametrize("form", mc.FORMS)
def test_two_calls_give_the_same_bits_and_count_two_updates(lib, form):
    inp = mc.random_inputs(33, 4097, 8, seed=9)
    tau = _tau_for(form, inp)
    run = Run(lib, inp, form, 1.0, 1e-5, tau)
    a = run.forward().backward().result()
    b = run.forward().backward().result()
    assert a["record"]["updates"] == 1 and b["record"]["updates"] == 2
    for name in ("part", "coef", "d1", "d2"):
        assert np.array_equal(a[name], b[name]), name
    assert (a["ms"], a["weighted"], a["d_image"], a["d_latent"]) == (b["ms"], b["weighted"], b["d_image"], b["d_latent"])
    # the settings are read from the record: a new weight changes the next call, the counter goes on
    from srgan_amd import _lib
    _lib.check(lib.srgan_ms_state_set(_p(run.state), 2.0, 1e-5, 0.0 if tau is None else tau, None), "ms_state_set")
    c = run.forward().backward().result()
    assert c["record"]["updates"] == 3 and c["ms"] == a["ms"] and c["weighted"] == np.float32(2.0) * np.float32(a["ms"])
    assert np.array_equal(c["d1"], np.float32(2.0) * a["d1"])


# ---- the ops on top ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in mc.CASES[:-1] if c[1] >= 63], ids=str)
def test_rowwise_l1_equals_numpy_on_the_quantised_cases(case):
    from srgan_amd import ops
    B, E, d = case
    i1, i2, _, _ = mc.quantised_inputs(B, E, d, seed=10)
    got = ops.rowwise_l1(torch.tensor(i1).cuda(), torch.tensor(i2).cuda())
    want = np.abs(i1.astype(np.float64) - i2).sum(1) / E
    assert got.dtype == torch.float64 and tuple(got.shape) == (B,) and not got.requires_grad
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("form", mc.FORMS)
def test_ops_mode_seeking_autograd(form):
    """the autograd Function on NHWC images: both gradients, one operand detached, a scaled incoming gradient, the record counts; the
    operands are row slices of a larger batch, as the train step hands them over"""
    from srgan_amd import ops
    B, C, H, W, d = 3, 3, 5, 7, 8
    i1, i2, z1, z2 = mc.quantised_inputs(B, C * H * W, d, seed=11)
    tau = 1.0
    ref = mc.ref64(i1, i2, z1, z2, form, weight=0.5, eps=2.0 ** -10, tau=tau)

    def nhwc(a):
        t = torch.tensor(np.concatenate([a, a, a], 0).reshape(3 * B, H, W, C)).cuda().permute(0, 3, 1, 2)
        return t[B:2 * B]

    state = ops.ms_state_new(torch.device("cuda"), 0.5, 2.0 ** -10, tau)
    zz1, zz2 = torch.tensor(z1).cuda(), torch.tensor(z2).cuda()
    a, b = nhwc(i1).requires_grad_(True), nhwc(i2).requires_grad_(True)
    weighted, value = ops.mode_seeking(a, b, zz1, zz2, state, form)
    assert weighted.requires_grad and not value.requires_grad
    assert float(value) == np.float32(ref["ms"]) and float(weighted) == np.float32(ref["weighted"])
    (weighted * 2.0).backward()
    c32 = np.asarray(ref["coef"], np.float32)
    want = (np.float32(2.0) * c32)[:, None] * np.sign(i1.astype(np.float64) - i2).astype(np.float32)
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(B, -1).cpu().numpy()
    assert np.array_equal(flat(a.grad), want) and np.array_equal(flat(b.grad), -want)
    a2 = nhwc(i1).requires_grad_(True)
    w2, _ = ops.mode_seeking(a2, nhwc(i2), zz1, zz2, state, form)
    w2.backward()
    assert np.array_equal(flat(a2.grad), want / np.float32(2.0))
    assert ops.ms_state_read(state)["updates"] == 2
    with pytest.raises(Exception, match="form"):
        ops.mode_seeking(a, b, zz1, zz2, state, "hinge")
