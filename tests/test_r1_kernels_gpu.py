"""GPU: the R1 gradient penalty below the trainer -- the two kernels of csrc/r1.hip alone on random input gradients, and the
whole pass (srgan_amd.r1.r1_accumulate) on the tier-T discriminator against the float64 closed form of tests/r1_common.py
evaluated with the DEVICE's own activation masks (a pre-activation within rounding of the kink may take the other slope, and one
flip moves a gradient by a whole term).

Bounds: the kernels alone max(8 * e32, (L + 16) * 2^-23) (tests/small_common.check; L from the add depths: u0 8 -- two divisions, three
adds of pool^T, the add of h1, c and its product; a partial 24 more); the pass max(8 * e32, floor) with the floors of
tests/conv_common.py (2e-5 for g, u0 and P, 5e-5 for each dW, relative to max |ref| of the tensor).  Measured figures: DESIGN.md
section 7."""
import os

import numpy as np
import pytest
import torch

from tests import r1_common as rc
from tests import small_common as sc

pytestmark = pytest.mark.gpu

SEED_SHAPES = [(1, 1, 1), (2, 3, 5), (3, 32, 32), (2, 33, 47), (1, 37, 111), (2, 40, 24), (2, 128, 128)]
L_U0, L_PART = 8, 32
GAMMA, EVERY = 7.0, 2
FLOOR_X, FLOOR_W = 2e-5, 5e-5          # tests/conv_common.py BOUND: y / dx and dw / db


def _inputs(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    h2, w2 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return (torch.randn(n, 3, h, w, generator=g, dtype=torch.float64), torch.randn(n, 3, h2, w2, generator=g, dtype=torch.float64))


def _nhwc(t, offset=0):
    """NHWC-dense float32 device tensor with the values of ``t``; ``offset`` floats into a larger buffer (a base off 16 bytes)"""
    n, c, h, w = t.shape
    buf = torch.empty(n * h * w * c + offset + 4, dtype=torch.float32, device="cuda")
    v = buf[offset:offset + n * h * w * c].view(n, h, w, c)
    v.copy_(t.permute(0, 2, 3, 1).float())
    return v.permute(0, 3, 1, 2)


def _seed_ref(h1, h2, c, dtype):
    n, _, h, w = h1.shape
    g = h1.to(dtype) + rc.pool_t(h2.to(dtype), h, w)
    u0 = torch.tensor(c, dtype=dtype) * g
    flat = g.permute(0, 2, 3, 1).reshape(n, -1)
    nchunk = -(-flat.shape[1] // 4096)
    pad = torch.zeros(n, nchunk * 4096, dtype=dtype)
    pad[:, :flat.shape[1]] = flat
    part = (pad * pad).view(n, nchunk, 4096).sum(-1)
    return u0, part


def _run_seed(h1, h2, offset=0):
    from srgan_amd import ops
    n, _, h, w = h1.shape
    st = ops.r1_state_new(torch.device("cuda"), GAMMA, EVERY, n)
    a, b = _nhwc(h1, offset), _nhwc(h2)
    u0 = _nhwc(torch.zeros_like(h1), offset)
    ws = torch.full((ops.r1_workspace_bytes(n, h, w) // 4,), float("nan"), dtype=torch.float32, device="cuda")
    ops.r1_seed_(a, b, st, u0, ws)
    ops.r1_finalize_(ws, n, h, w, st)
    return u0.cpu().contiguous(), ws.cpu().view(n, -1), ops.r1_state_read(st)


@pytest.mark.parametrize("shape", SEED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_seed_and_finalize_against_float64(shape):
    n, h, w = shape
    h1, h2 = _inputs(n, h, w, 100 + h)
    c = GAMMA * EVERY / n
    u32, p32 = _seed_ref(h1.float(), h2.float(), c, torch.float32)
    u64, p64 = _seed_ref(h1.float().double(), h2.float().double(), c, torch.float64)     # the device reads the float32 roundings
    u0, part, rec = _run_seed(h1, h2)
    sc.check("r1_seed_kernel", f"u0 {shape}", u0, u64, u32, L_U0)
    sc.check("r1_seed_kernel", f"partials {shape}", part.double(), p64, p32, L_PART)
    S = float(p64.sum())
    assert rec["updates"] == 1 and rec["n"] == n and rec["every"] == EVERY
    assert abs(rec["mean_sq_norm"] - S / n) <= sc.gamma(L_PART + 2) * S / n
    assert abs(rec["penalty"] - GAMMA * EVERY / 2 * S / n) <= sc.gamma(L_PART + 4) * GAMMA * EVERY / 2 * S / n
    # the finalize kernel on the device's own partials: the double sum rounded to float once
    want = float(part.double().sum()) / n
    assert abs(rec["mean_sq_norm"] - want) <= 2.0 ** -23 * want


@pytest.mark.parametrize("shape", SEED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scalar_and_16_byte_paths_agree_bit_for_bit(shape):
    n, h, w = shape
    h1, h2 = _inputs(n, h, w, 200 + w)
    u_a, p_a, r_a = _run_seed(h1, h2, 0)
    u_b, p_b, r_b = _run_seed(h1, h2, 1)            # a view one float into its buffer: the scalar path
    assert torch.equal(u_a, u_b) and torch.equal(p_a, p_b)
    assert r_a["penalty"] == r_b["penalty"] and r_a["mean_sq_norm"] == r_b["mean_sq_norm"]


@pytest.mark.parametrize("shape", [(3, 32, 32), (2, 33, 47)], ids=lambda s: "x".join(map(str, s)))
def test_a_sample_does_not_depend_on_batch_size_or_position(shape):
    """the partials of |g|^2 bit for bit (u0 carries c = gamma * every / N, which depends on N by definition: it is compared between
    two positions of one batch)"""
    n, h, w = shape
    h1, h2 = _inputs(n, h, w, 300)
    _, part, _ = _run_seed(h1, h2)
    big1 = torch.cat([h1.flip(0), h1, h1[:1]], 0)
    big2 = torch.cat([h2.flip(0), h2, h2[:1]], 0)
    ub, pb, _ = _run_seed(big1, big2)
    assert torch.equal(pb[n:2 * n], part) and torch.equal(pb[:n], part.flip(0)) and torch.equal(pb[2 * n], part[0])
    assert torch.equal(ub[:n], ub[n:2 * n].flip(0)) and torch.equal(ub[2 * n], ub[n])
    _, p1, _ = _run_seed(h1[-1:], h2[-1:])
    assert torch.equal(p1[0], part[-1])


def _pass(case, pack, sn=False):
    from srgan_amd import ops, r1, spectral
    n, h, w, layers, seed = case
    P = rc.pass_params(layers)
    x = rc.real_batch(n, h, w, seed)
    D = rc.hip_discriminator(P)
    if sn:
        torch.manual_seed(5)
        spectral.spectral_norm(D)
    st = r1.R1Penalty(rc.PASS_GAMMA, rc.PASS_EVERY)
    xd = ops.to_nhwc(x.float().cuda())
    if pack:
        with ops.pack_cache():
            kept = r1.r1_accumulate(D, xd, st, keep=True)
    else:
        kept = r1.r1_accumulate(D, xd, st, keep=True)
    return P, x, D, st, kept


@pytest.mark.parametrize("pack", [False, True], ids=["unpacked", "pack_cache"])
@pytest.mark.parametrize("case", rc.PASS_CASES, ids=lambda c: "x".join(map(str, c[:3])))
def test_whole_pass_against_the_closed_form_on_the_device_masks(case, pack):
    P, x, D, st, kept = _pass(case, pack)
    n = x.shape[0]
    masks = rc.device_masks(kept)
    rc.assert_masks_within(P, x.float().double(), masks, "device")
    ge = rc.PASS_GAMMA * rc.PASS_EVERY
    x64 = x.float().double()
    dW64, g64, P64, u64 = rc.closed_form(rc.cast(P, torch.float64), x64, ge, masks, detail=True)
    dW32, g32, P32, u32 = rc.closed_form(P, x.float(), ge, masks, detail=True)
    log = os.environ.get("SRGAN_TEST_LOG")

    def hold(what, got, ref64, ref32, floor):
        e32, err = rc.rel_err(ref32, ref64), rc.rel_err(got, ref64)
        bound = max(8 * e32, floor)
        if log:
            print(f"r1 pass {case[:3]} pack {int(pack)} | {what} | e32 {e32:.3e} err {err:.3e} bound {bound:.3e} err/bound {err / bound:.3f}")
        assert err <= bound, f"{what}: error {err:.3e} > bound {bound:.3e} (e32 = {e32:.3e})"

    rec = st.stats()
    u0 = kept["u0"].cpu()
    hold("u0", u0, u64, u32, FLOOR_X)
    hold("g", u0.double() / (ge / n), g64, g32, FLOOR_X)
    hold("P", torch.tensor(rec["penalty"]), P64, P32, FLOOR_X)
    got = rc.device_dW(P, kept)
    for k in dW64:
        hold("dW " + k, got[k], dW64[k], dW32[k], FLOOR_W)
    # head biases and class heads: untouched
    for name, p in D.named_parameters():
        if name not in dW64:
            assert p.grad is None, name


def test_gradients_are_added_to_what_the_backward_left():
    case = rc.PASS_CASES[0]
    from srgan_amd import ops, r1
    P, x, D, st, kept = _pass(case, True)
    pure = {k: v.clone() for k, v in rc.device_dW(P, kept).items()}
    base = {}
    for name, p in D.named_parameters():
        if name in pure:
            base[name] = torch.randn(p.shape, generator=torch.Generator().manual_seed(len(name)))
            p.grad = base[name].cuda()
    with ops.pack_cache():
        r1.r1_accumulate(D, ops.to_nhwc(x.float().cuda()), st)
    assert st.stats()["updates"] == 2
    for name, p in D.named_parameters():
        if name in pure:
            want = base[name].double() + pure[name].double()
            assert float((p.grad.cpu().double() - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max()), name


def test_spectrally_normalised_and_plain_discriminator_agree_bit_for_bit():
    """the pass reads the normalised leaf (m.weight) and writes its .grad: a plain D carrying the same effective weights gives the
    same bits"""
    from srgan_amd import ops, r1
    case = rc.PASS_CASES[2]
    P, x, Dsn, st, kept = _pass(case, True, sn=True)
    eff = dict(P)
    for s in (1, 2):
        keys, head = rc.trunk_keys(P, s)
        for k in keys + [head]:
            mod = Dsn.get_submodule(k.rpartition(".")[0])
            assert "weight" not in dict(mod.named_parameters()) and mod.weight.grad is not None      # the leaf took the gradient
            assert mod.weight_orig.grad is None
            eff[k] = mod.weight.detach().cpu().clone()
    Dp = rc.hip_discriminator(eff)
    st2 = r1.R1Penalty(rc.PASS_GAMMA, rc.PASS_EVERY)
    with ops.pack_cache():
        kept2 = r1.r1_accumulate(Dp, ops.to_nhwc(x.float().cuda()), st2, keep=True)
    a, b = rc.device_dW(P, kept), rc.device_dW(P, kept2)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert st.stats()["penalty"] == st2.stats()["penalty"]
