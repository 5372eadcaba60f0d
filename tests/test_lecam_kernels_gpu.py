"""GPU: ``srgan_lecam`` (csrc/lecam.hip) through ctypes on guarded memory against the restatement of tests/lecam_common.py -- the
anchors, the term, the three values and every element of the gradient's increment against float64 at the bounds derived there, the
2S raw sums bit for bit against the numpy emulation of the summation order, both access paths bit for bit against each other, the
select rules on hostile inputs, the record's entries, and the launch behind ``ops.d_losses`` / ``ops.d_losses_cr``."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import lecam_common as lc

pytestmark = pytest.mark.gpu
GUARD = 256                        # floats on either side of every buffer the kernel writes
SENTINEL = 0x7FDEAD77
WEIGHT, DECAY = 0.5, 0.75
WORST = {}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _prefill(n):
    """the known pattern d_o holds before a call: exact small values of either sign, the size of the term's gradient"""
    i = torch.arange(n, dtype=torch.float32)
    return ((i * 7) % 13 - 6) * 2.0 ** -10


class Device:
    """maps, gradient buffers, the three values, the incoming total and the record, each between two guard regions; ``offset``
    floats into their buffers the maps and gradient buffers start (0: 16-byte aligned, 1: the scalar path at any per_s)"""

    def __init__(self, S, rows, pers, offset, weight=WEIGHT, decay=DECAY, start=0):
        from srgan_amd import _lib
        self.lib, self.S, self.rows, self.pers, self.offset = _lib.load(), S, rows, pers, offset
        self.o = [torch.zeros(rows * p + 8, dtype=torch.float32, device="cuda") for p in pers]
        self.g = [self._guarded(rows * p + 8) for p in pers]
        self.v = self._guarded(4)                   # [total_in, vals[0..2]]
        self.rec = torch.full((64 + 56 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        rc = self.lib.srgan_lc_state_init(self._state(), weight, decay, start, self._stream())
        assert rc == 0, self.lib.srgan_last_error()

    @staticmethod
    def _guarded(n):
        return torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)

    @staticmethod
    def _stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _state(self):
        return ctypes.c_void_p(self.rec.data_ptr() + 64)

    def state_view(self):
        return self.rec[64:64 + 56]

    def read(self):
        from srgan_amd import ops
        return ops.lc_state_read(self.state_view())

    def call(self, maps, P, B1, clamp, total_in, prefill=True):
        """-> (vals [3], [d_o after per scale], [d_o before per scale]) on the CPU; checks every guard"""
        off = self.offset
        before = []
        for s, m in enumerate(maps):
            n = m.numel()
            self.o[s][off:off + n].view(torch.int32).copy_(_bits(m).flatten().cuda())             # bits: NaN payloads survive
            if prefill:
                self.g[s][GUARD + off:GUARD + off + n].copy_(_prefill(n).cuda())
            before.append(self.g[s][GUARD + off:GUARD + off + n].cpu().clone())
        self.v[GUARD:GUARD + 1].view(torch.int32).copy_(_bits(torch.tensor([total_in], dtype=torch.float32)).cuda())
        arr = ctypes.c_void_p * self.S
        rc = self.lib.srgan_lecam(arr(*[t.data_ptr() + 4 * off for t in self.o]), (ctypes.c_longlong * self.S)(*self.pers), self.S,
                                  self.rows, P, B1, int(clamp), ctypes.c_void_p(self.v.data_ptr() + 4 * GUARD),
                                  ctypes.c_void_p(self.v.data_ptr() + 4 * (GUARD + 1)),
                                  arr(*[t.data_ptr() + 4 * (GUARD + off) for t in self.g]), self._state(), self._stream())
        assert rc == 0, self.lib.srgan_last_error()
        torch.cuda.synchronize()
        after = []
        for s, m in enumerate(maps):
            n = m.numel()
            buf = self.g[s].cpu()
            after.append(buf[GUARD + off:GUARD + off + n].clone())
            assert bool((buf[:GUARD + off].view(torch.int32) == SENTINEL).all()), "the guard in front of d_o was written"
            assert bool((buf[GUARD + off + n:].view(torch.int32) == SENTINEL).all()), "the guard behind d_o was written"
        v = self.v.cpu()
        assert bool((v[:GUARD].view(torch.int32) == SENTINEL).all()) and bool((v[GUARD + 4:].view(torch.int32) == SENTINEL).all())
        assert _bits(v[GUARD:GUARD + 1]).item() == _bits(torch.tensor([total_in], dtype=torch.float32)).item()
        rec = self.rec.cpu()
        assert bool((rec[:64] == 0xA5).all()) and bool((rec[120:] == 0xA5).all()), "a guard around the record was written"
        return v[GUARD + 1:GUARD + 4].clone(), after, before


def _note(what, err, bound):
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    WORST[what] = max(WORST.get(what, 0.0), ratio)
    if os.environ.get("SRGAN_TEST_LOG"):
        print(f"lecam | {what} | err {err:.3e} bound {bound:.3e} err/bound {ratio:.3f} | worst {WORST[what]:.3f}")
    return ratio


def _hold(what, got, ref64, ref32, derived):
    """|got - ref64| <= max(8 |ref32 - ref64|, the derived bound), elementwise maxima"""
    got, ref64, ref32 = (torch.as_tensor(t, dtype=torch.float64).reshape(-1) for t in (got, ref64, ref32))
    assert bool(torch.isfinite(got).all()), what
    err, e32 = float((got - ref64).abs().max()), float((ref32 - ref64).abs().max())
    bound = max(8 * e32, derived)
    _note(what.split(" ")[0], err, bound)
    assert err <= bound, f"{what}: error {err:.3e} > max(8 * e32 = {8 * e32:.3e}, derived = {derived:.3e})"


def _check_call(tag, c, maps, P, B1, clamp, total_in, dev_out, dev_rec, rec64, rec32):
    """hold one call's outputs to float64 at the bounds of tests/lecam_common.py -> (the float64 record, the float32 record) after"""
    vals, after, before = dev_out
    S = len(maps)
    v64, i64, new64, _ = lc.call(maps, rec64, P, B1, clamp, total_in, torch.float64)
    v32, i32, new32, _ = lc.call(maps, rec32, P, B1, clamp, total_in, torch.float32)
    w = rec64["weight"]
    E_all, L_all = 0.0, 0
    for s, m in enumerate(maps):
        front = m.reshape(m.shape[0], -1)[:P].double()
        per = front.shape[1]
        L, M = lc.chain_depth(P * per), float(front.abs().max())
        ab = lc.anchor_bound(L, c, M)
        _hold(f"anchor {tag} call {c} a_real[{s}]", dev_rec["a_real"][s], new64["a_real"][s], new32["a_real"][s], ab)
        _hold(f"anchor {tag} call {c} a_fake[{s}]", dev_rec["a_fake"][s], new64["a_fake"][s], new32["a_fake"][s], ab)
        phi_r = lc.phi(front[:B1] - new64["a_fake"][s], clamp)
        phi_f = lc.phi(new64["a_real"][s] - front[B1:], clamp)
        max_phi = max([float(t.abs().max()) for t in (phi_r, phi_f) if t.numel()] + [0.0])
        E = ab + lc.EPS32 * max_phi
        E_all, L_all = max(E_all, E), max(L_all, L)
        incr = (after[s].double() - before[s].double()).reshape(m.shape[0], -1)
        n1, n2 = B1 * per, (P - B1) * per
        k = max(2 * w / (S * n) for n in (n1, n2) if n > 0) if new64["applied"] else 0.0
        gb = lc.grad_bound(k, E, max_phi, float(after[s].abs().max()))
        _hold(f"d_o {tag} call {c} scale {s}", incr[:P], i64[s][:P], i32[s][:P], gb)
        assert torch.equal(_bits(after[s].reshape(m.shape[0], -1)[P:]), _bits(before[s].reshape(m.shape[0], -1)[P:])), "back rows of d_o"
    R = float(v64[0])
    rb = lc.term_bound(L_all, E_all, R)
    _hold(f"R {tag} call {c}", vals[0], v64[0], v32[0], rb)
    wb = w * rb + lc.EPS32 * w * R
    _hold(f"weighted {tag} call {c}", vals[1], v64[1], v32[1], wb)
    _hold(f"total {tag} call {c}", vals[2], v64[2], v32[2], wb + lc.EPS32 * abs(float(v64[2])))
    assert dev_rec["penalty"] == float(vals[0]) and dev_rec["applied"] == new64["applied"] and dev_rec["updates"] == new64["updates"]
    return new64, new32


def _three_calls(shape, clamp, offset, shift=0.3, spread=0.7, tag=None):
    """three consecutive calls on one record with fresh maps -> [(vals, d_o after, record)] per call, every call held to float64"""
    S, P, B1, per, rows = shape
    pers = lc.per_rows(S, per)
    dev = Device(S, rows, pers, offset)
    rec64 = rec32 = lc.new_record(WEIGHT, DECAY, 0, S)
    out = []
    for c in range(1, 4):
        maps = lc.make_maps(S, P, per, rows, seed=100 * c + P + per, shift=shift, spread=spread)
        if rows > P:
            for m in maps:
                m[P:] = float("nan")                                                     # the back rows are nobody's business
        total_in = 0.625 + c
        res = dev.call(maps, P, B1, clamp, total_in)
        rec = dev.read()
        if c == 1:
            # the 2S raw sums, bit for bit: the first update's anchor is 0 * 0 + 1 * (sum / n) = fl(sum / n)
            for s, m in enumerate(maps):
                front = m.reshape(rows, -1)[:P].numpy().ravel()
                sr, sf = lc.emulate_sums(front, B1 * pers[s])
                if B1 > 0:
                    want = np.float32(sr) / np.float32(B1 * pers[s])
                    assert np.float32(rec["a_real"][s]).view(np.int32) == want.view(np.int32), (shape, s, rec["a_real"][s], want)
                if P - B1 > 0:
                    want = np.float32(sf) / np.float32((P - B1) * pers[s])
                    assert np.float32(rec["a_fake"][s]).view(np.int32) == want.view(np.int32), (shape, s, rec["a_fake"][s], want)
        rec64, rec32 = _check_call(tag or str(shape), c, maps, P, B1, clamp, total_in, res, rec, rec64, rec32)
        assert rec["updates"] == c and rec["applied"] == 1
        if B1 == 0:
            assert rec["a_real"] == [0.0] * 4                                            # an empty group's anchor stays
        if B1 == P:
            assert rec["a_fake"] == [0.0] * 4
        assert rec["a_real"][S:] == [0.0] * (4 - S) and rec["a_fake"][S:] == [0.0] * (4 - S)
        out.append((res[0], res[1], rec))
    return out


@pytest.mark.parametrize("clamp", [False, True], ids=["identity", "relu"])
@pytest.mark.parametrize("shape", lc.SHAPES, ids=str)
def test_three_calls_against_float64_on_both_access_paths(shape, clamp):
    """anchors, R, the three values and every d_o element (as the increment over the pre-filled pattern) at the derived bounds, after
    each of three calls on one record; the raw sums bit-equal to the emulated order; the run whose buffers start one float past a
    16-byte boundary (the scalar path whatever per_s is) gives the same bits as the aligned run (16-byte accesses where per_s % 4 ==
    0)"""
    aligned = _three_calls(shape, clamp, 0)
    shifted = _three_calls(shape, clamp, 1)
    for (va, ga, ra), (vb, gb, rb) in zip(aligned, shifted):
        assert torch.equal(_bits(va), _bits(vb)) and ra == rb
        for a, b in zip(ga, gb):
            assert torch.equal(_bits(a), _bits(b))


def test_maps_at_plus_1000_with_unit_spread():
    """The bound scales with max |o|: an anchor is a mean of values near 1000 and is good to (L + 16 + 3 c) 2^-23 * 1000 in absolute
    terms, which is what the differences o - a inherit although they are of size 1 (tests/lecam_common.py).  Held at that bound, not
    at one relative to the spread."""
    for clamp in (False, True):
        _three_calls((2, 7, 3, 64, 7), clamp, 0, shift=1000.0, spread=1.0, tag="plus1000")


def _nan_maps(shape, seed, where="front"):
    S, P, B1, per, rows = shape
    maps = lc.make_maps(S, P, per, rows, seed)
    if where == "front":
        maps[0].view(-1)[1] = float("nan")                  # a real element
        maps[-1].view(-1)[P * lc.per_rows(S, per)[-1] - 1] = float("nan")       # the last generated element of the last scale
    return maps


def test_an_inactive_term_keeps_every_bit_and_still_moves_the_anchors():
    """weight = 0, and updates < start: d_o and the total keep their bits although the maps hold NaN (a select, not a product with
    zero); a NaN batch moves no anchor and does not count; a finite batch moves the anchors while the term is inactive"""
    shape = (2, 7, 3, 64, 7)
    S, P, B1, per, rows = shape
    pers = lc.per_rows(S, per)
    for weight, start in ((0.0, 0), (1.5, 2)):
        dev = Device(S, rows, pers, 0, weight=weight, start=start)
        total_in = -0.0
        vals, after, before = dev.call(_nan_maps(shape, 1), P, B1, False, total_in)
        rec = dev.read()
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(after, before))
        assert _bits(vals[2:3]).item() == _bits(torch.tensor([total_in])).item() and float(vals[1]) == 0.0 and np.isnan(float(vals[0]))
        assert rec["updates"] == 0 and rec["applied"] == 0 and rec["a_real"] == [0.0] * 4 and rec["a_fake"] == [0.0] * 4
        n_finite = 2 if start else 1
        for i in range(n_finite):
            maps = lc.make_maps(S, P, per, rows, seed=20 + i)
            vals, after, before = dev.call(maps, P, B1, False, 1.75)
            rec = dev.read()
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(after, before))
            assert float(vals[2]) == 1.75 and float(vals[1]) == 0.0 and float(vals[0]) > 0
            assert rec["updates"] == i + 1 and rec["applied"] == 0 and all(rec["a_real"][:S]) and all(rec["a_fake"][:S])
            assert rec["penalty"] == float(vals[0])
        if start:
            vals, after, before = dev.call(lc.make_maps(S, P, per, rows, seed=30), P, B1, False, 1.75)       # updates == start
            assert dev.read()["applied"] == 1 and float(vals[1]) > 0 and float(vals[2]) > 1.75
            assert all(not torch.equal(_bits(a), _bits(b)) for a, b in zip(after, before))


def test_a_nan_batch_of_an_active_term_moves_nothing_in_the_record():
    shape = (2, 5, 2, 9, 5)
    S, P, B1, per, rows = shape
    dev = Device(S, rows, lc.per_rows(S, per), 1)
    dev.call(lc.make_maps(S, P, per, rows, seed=1), P, B1, True, 0.5)
    rec = dev.read()
    # (relu keeps a NaN, as torch.relu does; it maps a_R - inf to 0, so the one-sided term of an Inf batch can be finite)
    for clamp, poison in ((False, float("nan")), (False, float("inf")), (True, float("nan"))):
        maps = lc.make_maps(S, P, per, rows, seed=2)
        maps[1][P - 1, 0] = poison
        vals, _, _ = dev.call(maps, P, B1, clamp, 0.5)
        after = dev.read()
        assert after["updates"] == 1 == rec["updates"] and after["a_real"] == rec["a_real"] and after["a_fake"] == rec["a_fake"]
        assert after["applied"] == 1 and not np.isfinite(after["penalty"]) and not np.isfinite(float(vals[2]))
    dev.call(lc.make_maps(S, P, per, rows, seed=3), P, B1, True, 0.5)
    assert dev.read()["updates"] == 2 and np.isfinite(dev.read()["penalty"])


def test_set_between_calls_changes_the_next_call_only():
    shape = (2, 7, 3, 65, 7)
    S, P, B1, per, rows = shape
    dev = Device(S, rows, lc.per_rows(S, per), 0)
    rec64 = rec32 = lc.new_record(WEIGHT, DECAY, 0, S)
    m1, m2 = lc.make_maps(S, P, per, rows, seed=1), lc.make_maps(S, P, per, rows, seed=2)
    res = dev.call(m1, P, B1, False, 0.25)
    rec64, rec32 = _check_call("set", 1, m1, P, B1, False, 0.25, res, dev.read(), rec64, rec32)
    kept = dev.read()
    rc = dev.lib.srgan_lc_state_set(dev._state(), 2.0, 0.25, 0, dev._stream())
    assert rc == 0
    now = dev.read()
    assert now == dict(kept, weight=2.0, decay=0.25)                     # the counter, the anchors and the last outputs stay
    rec64, rec32 = (dict(r, weight=2.0, decay=0.25) for r in (rec64, rec32))
    res = dev.call(m2, P, B1, False, 0.25)
    _check_call("set", 2, m2, P, B1, False, 0.25, res, dev.read(), rec64, rec32)
    # the old settings would have given another second call
    other = Device(S, rows, lc.per_rows(S, per), 0)
    other.call(m1, P, B1, False, 0.25)
    res_old = other.call(m2, P, B1, False, 0.25)
    assert float(res_old[0][1]) != float(res[0][1]) and other.read()["a_real"] != dev.read()["a_real"]


def test_restore_then_a_call_equals_the_uninterrupted_sequence():
    from srgan_amd import ops
    shape = (4, 5, 2, 9, 5)
    S, P, B1, per, rows = shape
    pers = lc.per_rows(S, per)
    maps = [lc.make_maps(S, P, per, rows, seed=40 + i) for i in range(3)]
    a = Device(S, rows, pers, 0)
    for m in maps[:2]:
        a.call(m, P, B1, True, 0.5)
    mid = a.read()
    b = Device(S, rows, pers, 0)
    ops.lc_state_restore(b.state_view(), mid["updates"], mid["a_real"], mid["a_fake"])
    got = b.read()
    assert got == dict(mid, penalty=0.0, applied=0)                      # a restore leaves the last call's outputs alone
    ra, rb = a.call(maps[2], P, B1, True, 0.5), b.call(maps[2], P, B1, True, 0.5)
    assert torch.equal(_bits(ra[0]), _bits(rb[0])) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(ra[1], rb[1]))
    assert torch.equal(a.state_view().cpu(), b.state_view().cpu()) and a.read()["updates"] == 3


def test_the_record_entries_and_their_refusals():
    from srgan_amd import _lib, ops
    st = ops.lc_state_new("cuda", 0.3, 0.99, 5)
    f32 = lambda v: float(np.float32(v))
    assert ops.lc_state_read(st) == dict(weight=f32(0.3), decay=f32(0.99), start=5, updates=0, a_real=[0.0] * 4, a_fake=[0.0] * 4,
                                         penalty=0.0, applied=0)
    ops.lc_state_restore(st, 7, [1.0, 2.0, 3.0, 4.0], [-1.0, -2.0, -3.0, -4.0])
    ops.lc_state_set(st, 1.0, 0.5, 0)
    assert ops.lc_state_read(st) == dict(weight=1.0, decay=0.5, start=0, updates=7, a_real=[1.0, 2.0, 3.0, 4.0],
                                         a_fake=[-1.0, -2.0, -3.0, -4.0], penalty=0.0, applied=0)
    for bad in ((-1.0, 0.5, 0), (1.0, 1.0, 0), (1.0, 0.5, -1), (float("nan"), 0.5, 0), (1.0, float("nan"), 0)):
        with pytest.raises(_lib.SrganHipError, match="lc_state_set"):
            ops.lc_state_set(st, *bad)
        with pytest.raises(_lib.SrganHipError, match="lc_state_init"):
            ops.lc_state_new("cuda", *bad)
    with pytest.raises(_lib.SrganHipError, match="not finite"):
        ops.lc_state_restore(st, 1, [float("nan")] * 4, [0.0] * 4)
    with pytest.raises(_lib.SrganHipError, match="updates >= 0"):
        ops.lc_state_restore(st, -1, [0.0] * 4, [0.0] * 4)
    with pytest.raises(_lib.SrganHipError, match="anchors"):
        ops.lc_state_restore(st, 1, [0.0] * 2, [0.0] * 4)
    assert ops.lc_state_read(st)["updates"] == 7                          # a refused write wrote nothing
    # the launch's refusals on real memory
    o = [torch.zeros(4, 8, device="cuda")]
    with pytest.raises(_lib.SrganHipError, match="record of lc_state_new"):
        ops.d_losses(o, [], None, 2, 1.0, 0.0, 0.0, lecam=(torch.zeros(4, device="cuda"), False))
    # each refusal of the launch on real memory: -1 before anything runs, the record and d_o as they were
    dev = Device(2, 8, [16, 4], 0)
    lib, arr, ll = dev.lib, ctypes.c_void_p * 2, ctypes.c_longlong * 2
    o, g = arr(*[t.data_ptr() for t in dev.o]), arr(*[t.data_ptr() + 4 * GUARD for t in dev.g])
    tot, v = ctypes.c_void_p(dev.v.data_ptr() + 4 * GUARD), ctypes.c_void_p(dev.v.data_ptr() + 4 * GUARD + 4)
    snap = [dev.rec.clone(), dev.v.clone()] + [t.clone() for t in dev.g]

    def call(o=o, per=ll(16, 4), S=2, rows=8, pairs=4, rows_first=2, clamp=0, tot=tot, v=v, g=g, state=dev._state()):
        rc = lib.srgan_lecam(o, per, S, rows, pairs, rows_first, clamp, tot, v, g, state, dev._stream())
        return rc, lib.srgan_last_error().decode()

    for kw, what in ((dict(o=None), "null pointer"), (dict(per=None), "null pointer"), (dict(tot=None), "null pointer"),
                     (dict(v=None), "null pointer"), (dict(g=None), "null pointer"), (dict(state=None), "null pointer"),
                     (dict(S=0), "0 scales"), (dict(S=5), "5 scales"), (dict(rows=7), "rows = 7"), (dict(rows=12), "rows = 12"),
                     (dict(pairs=0, rows=0), "rows = 0"), (dict(rows_first=5), "rows_first = 5"), (dict(rows_first=-1), "rows_first = -1"),
                     (dict(clamp=2), "clamp = 2"), (dict(per=ll(16, 0)), "null scale"), (dict(per=ll(1 << 28, 4)), "2^31"),
                     (dict(o=arr(dev.o[0].data_ptr(), 0)), "null scale"), (dict(g=arr(dev.g[0].data_ptr() + 2, g[1])), "aligned")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg, (kw, msg)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(snap, [dev.rec, dev.v] + dev.g))
    assert call()[0] == 0                                                 # and the arguments they vary are good ones


# ---- behind the fused loss launches --------------------------------------------------------------------------------------------------
def _loss(fn, maps, rows_first, scale, **kw):
    outs = [m.cuda().requires_grad_(True) for m in maps]
    total, parts = fn(outs, [], None, rows_first, 1.0, 0.0, 0.0, **kw)
    assert not parts.requires_grad
    (total * scale).backward()
    return total.detach().cpu().reshape(()), parts.detach().cpu(), [o.grad.cpu() for o in outs]


@pytest.mark.parametrize("clamp", [False, True], ids=["identity", "relu"])
def test_behind_d_losses_the_gradient_rides_the_loss_buffers(clamp):
    """ops.d_losses(..., lecam=): total = errD + weight R, parts = [.., errD, R, weight R]; the gradient is the plain call's plus the
    term's, at the kernel test's bounds, and the incoming gradient scales both in the one multiply of the backward; weight 0: the
    plain call's bits"""
    from srgan_amd import ops
    S, P, B1, per = 2, 8, 4, 49
    maps = lc.make_maps(S, P, per, P, seed=5)
    t0, p0, g0 = _loss(ops.d_losses, maps, B1, 1.0)
    st = ops.lc_state_new("cuda", 0.0, DECAY, 0)
    t1, p1, g1 = _loss(ops.d_losses, maps, B1, 1.0, lecam=(st, clamp))
    assert tuple(p1.shape) == (6,) and torch.equal(_bits(p1[:3]), _bits(p0)) and _bits(t1).item() == _bits(t0).item() == _bits(p1[3]).item()
    assert float(p1[4]) > 0 and float(p1[5]) == 0.0 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(g0, g1))
    assert ops.lc_state_read(st)["updates"] == 1
    st = ops.lc_state_new("cuda", WEIGHT, DECAY, 0)
    t2, p2, g2 = _loss(ops.d_losses, maps, B1, 1.0, lecam=(st, clamp))
    assert _bits(p2[3]).item() == _bits(t0).item()                        # errD is the value without the term
    rec0 = lc.new_record(WEIGHT, DECAY, 0, S)
    _check_call("ops", 1, maps, P, B1, clamp, float(t0), (torch.stack([p2[4], p2[5], t2]), g2, g0), ops.lc_state_read(st), rec0, rec0)
    st = ops.lc_state_new("cuda", WEIGHT, DECAY, 0)
    _, _, g3 = _loss(ops.d_losses, maps, B1, 2.0, lecam=(st, clamp))
    assert all(torch.equal(_bits(a), _bits(2.0 * b)) for a, b in zip(g3, g2))


def test_behind_d_losses_cr_the_back_rows_keep_their_bits():
    from srgan_amd import ops
    S, P, B1, per = 2, 6, 3, 20
    maps = lc.make_maps(S, P, per, 2 * P, seed=6)
    cr = ops.cr_state_new("cuda", 3.0, 0.5, 1)
    t0, p0, g0 = _loss(ops.d_losses_cr, maps, B1, 1.0, state=cr)
    st = ops.lc_state_new("cuda", WEIGHT, DECAY, 0)
    t1, p1, g1 = _loss(ops.d_losses_cr, maps, B1, 1.0, state=cr, lecam=(st, False))
    assert tuple(p1.shape) == (9,) and torch.equal(_bits(p1[:6]), _bits(p0)) and _bits(p1[6]).item() == _bits(t0).item()
    rec0 = lc.new_record(WEIGHT, DECAY, 0, S)
    # (_check_call holds the back rows of the gradient to the bits of the call without the term)
    _check_call("ops_cr", 1, maps, P, B1, False, float(t0), (torch.stack([p1[7], p1[8], t1]), g1, g0), ops.lc_state_read(st), rec0, rec0)
    assert all(not torch.equal(a[:P], b[:P]) for a, b in zip(g1, g0))
