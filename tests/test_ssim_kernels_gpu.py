"""GPU: the structural-similarity kernels (csrc/ssim.hip) through ctypes on guarded memory and through ``ops`` / ``evaluation``
against the float64 restatement of tests/ssim_common.py at the bounds derived there -- the per-sample values, the term, every
element of dx and dy (together and alone), the path without a gradient (no coefficient map is written), rows that start at a
4-byte-only aligned address, the record, a zero weight, equal bits of two calls, a NaN pixel, PSNR and the chunked metrics."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from tests import ssim_common as sc

pytestmark = pytest.mark.gpu
GUARD = 256                        # floats on either side of every buffer a kernel writes
SENTINEL = 0x7FDEAD77
WEIGHT = 0.75
WORST = {}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _guarded(n):
    return torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _guards_intact(buf, n, what):
    b = buf.cpu().view(torch.int32)
    assert bool((b[:GUARD] == SENTINEL).all()), f"the guard in front of {what} was written"
    assert bool((b[GUARD + n:] == SENTINEL).all()), f"the guard behind {what} was written"


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().reshape(-1)


class Device:
    """The images (``offset`` floats into their buffers: 0 = 16-byte aligned, 1 = 4-byte aligned only), dx, dy, the two values, the
    per-sample values, the workspace and the record, each written buffer between two guard regions."""

    def __init__(self, n, c, h, w, window, offset=0, weight=WEIGHT, sigma=1.5, k1=0.01, k2=0.03, data_range=2.0, taps=None):
        from srgan_amd import _lib, ops
        self.lib, self.geom, self.window, self.offset = _lib.load(), (n, c, h, w), window, offset
        self.numel = n * c * h * w
        self.taps = (ctypes.c_float * window)(*(ops.ssim_taps(window, sigma) if taps is None else taps))
        self.c1, self.c2 = sc.constants(k1, k2, data_range)
        self.x = torch.zeros(self.numel + 8, dtype=torch.float32, device="cuda")
        self.y = torch.zeros(self.numel + 8, dtype=torch.float32, device="cuda")
        self.rec = torch.full((64 + 32 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        rc = self.lib.srgan_ssim_state_init(self._state(), weight, self.c1, self.c2, _stream())
        assert rc == 0, self.lib.srgan_last_error()

    def _state(self):
        return ctypes.c_void_p(self.rec.data_ptr() + 64)

    def read(self):
        from srgan_amd import ops
        rec = self.rec.cpu()
        assert bool((rec[:64] == 0xA5).all()) and bool((rec[96:] == 0xA5).all()), "a guard around the record was written"
        return ops.ss_state_read(self.rec[64:96])

    def call(self, x, y, want_dx=True, want_dy=True, g=None, state=True):
        """-> dict(values [N], vals [2], dx, dy [N, C, H, W] or None, ws: the workspace's floats) on the CPU; checks every guard"""
        n, c, h, w = self.geom
        off, lib = self.offset, self.lib
        self.x[off:off + self.numel].view(torch.int32).copy_(_bits(_nhwc(x)).cuda())          # bits: NaN payloads survive
        self.y[off:off + self.numel].view(torch.int32).copy_(_bits(_nhwc(y)).cuda())
        px, py = ctypes.c_void_p(self.x.data_ptr() + 4 * off), ctypes.c_void_p(self.y.data_ptr() + 4 * off)
        nb = lib.srgan_ssim_workspace(n, c, h, w, self.window, int(want_dx), int(want_dy))
        assert nb > 0 and nb % 16 == 0, lib.srgan_last_error()
        ws = _guarded(nb // 4)
        vals, values = _guarded(2), _guarded(n)
        dx = _guarded(self.numel + 8) if want_dx else None
        dy = _guarded(self.numel + 8) if want_dy else None
        at = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + 4 * (GUARD + o)) if t is not None else None
        st = self._state() if state else None
        rc = lib.srgan_ssim_map(px, py, n, c, h, w, self.window, self.taps, st, self.c1, self.c2, int(want_dx), int(want_dy), at(ws),
                                nb, _stream())
        assert rc == 0, lib.srgan_last_error()
        rc = lib.srgan_ssim_finish(at(ws), nb, n, c, h, w, self.window, st, at(vals), at(values), _stream())
        assert rc == 0, lib.srgan_last_error()
        if want_dx or want_dy:
            gdev = None if g is None else torch.tensor([g], dtype=torch.float32, device="cuda")
            rc = lib.srgan_ssim_grad(px, py, n, c, h, w, self.window, self.taps, at(ws), nb, st,
                                     None if gdev is None else ctypes.c_void_p(gdev.data_ptr()), at(dx, off), at(dy, off), _stream())
            assert rc == 0, lib.srgan_last_error()
        torch.cuda.synchronize()
        _guards_intact(ws, nb // 4, "the workspace")
        _guards_intact(vals, 2, "vals")
        _guards_intact(values, n, "values")
        out = dict(vals=vals[GUARD:GUARD + 2].cpu(), values=values[GUARD:GUARD + n].cpu(), ws=ws[GUARD:GUARD + nb // 4].cpu(), dx=None,
                   dy=None)
        for name, buf in (("dx", dx), ("dy", dy)):
            if buf is None:
                continue
            b = buf.cpu().view(torch.int32)
            assert bool((b[:GUARD + off] == SENTINEL).all()), f"the guard in front of {name} was written"
            assert bool((b[GUARD + off + self.numel:] == SENTINEL).all()), f"the guard behind {name} was written"
            flat = buf[GUARD + off:GUARD + off + self.numel].cpu()
            assert not bool((flat.view(torch.int32) == SENTINEL).any()), f"an element of {name} was not written"
            out[name] = flat.reshape(n, h, w, c).permute(0, 3, 1, 2)
        return out


def _note(what, err, bound):
    """worst elementwise err / bound (0 / 0 = 0)"""
    err, bound = torch.as_tensor(err, dtype=torch.float64).reshape(-1), torch.as_tensor(bound, dtype=torch.float64).reshape(-1)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max())
    WORST[what] = max(WORST.get(what, 0.0), worst)
    print(f"ssim | {what} | max err {float(err.max()):.3e} | worst err / bound {worst:.3f} | so far {WORST[what]:.3f}")
    return worst


@functools.lru_cache(maxsize=None)
def _case(name, weight=WEIGHT):
    """the inputs, the float64 reference and the bounds of a case, computed once"""
    _, n, c, h, w, window, kind = next(k for k in sc.CASES if k[0] == name)
    x, y = sc.make_pair(kind, n, c, h, w, seed=len(name))
    ref = sc.reference(x, y, weight=weight, window=window)
    bnd = sc.bounds(x, y, weight=weight, window=window)
    return (n, c, h, w, window), x, y, ref, bnd


def _hold(tag, out, ref, bnd, weight=WEIGHT, g=1.0):
    assert bool(torch.isfinite(out["values"]).all()) and bool(torch.isfinite(out["vals"]).all()), tag
    r = _note("values", (out["values"].double() - ref["values"]).abs(), bnd["values"])
    assert r <= 1.0, f"{tag}: a per-sample value is {r:.3f} of its bound off"
    r = _note("term", abs(float(out["vals"][1]) - ref["term"]), bnd["term"])
    assert r <= 1.0, f"{tag}: the term is {r:.3f} of its bound off"
    wb = weight * bnd["term"] + sc.U * abs(weight * ref["term"]) * 2
    r = _note("weighted", abs(float(out["vals"][0]) - weight * ref["term"]), wb)
    assert r <= 1.0, f"{tag}: the weighted term is {r:.3f} of its bound off"
    for name in ("dx", "dy"):
        if out[name] is None:
            continue
        assert bool(torch.isfinite(out[name]).all()), (tag, name)
        # the incoming gradient multiplies in float64 before the one rounding of k: the bound scales with it
        r = _note(name, (out[name].double() - g * ref[name]).abs(), abs(g) * bnd[name] + 1e-300)
        assert r <= 1.0, f"{tag}: an element of {name} is {r:.3f} of its bound off"


@pytest.mark.parametrize("name", sc.CASE_IDS)
def test_values_term_and_both_gradients_against_float64(name):
    geom, x, y, ref, bnd = _case(name)
    dev = Device(*geom)
    out = dev.call(x, y)
    _hold(name, out, ref, bnd)
    rec = dev.read()
    assert rec["updates"] == 1 and rec["weight"] == WEIGHT
    assert rec["term"] == float(out["vals"][1]) and rec["weighted"] == float(out["vals"][0])
    if name == "equal":
        # SSIM(x, x) = 1 up to the roundings of the quotient; the gradient vanishes with it
        assert float((out["values"] - 1).abs().max()) <= 4 * sc.U
    if name == "constant":
        a, b = x[:, :, 0, 0].double(), y[:, :, 0, 0].double()
        c1 = sc.constants()[0]
        closed = ((2 * a * b + c1) / (a * a + b * b + c1)).mean(1)
        assert float((out["values"].double() - closed).abs().max()) <= float(bnd["values"].max()) + sc.closed_form_slack(a, b)


def test_rows_at_a_4_byte_aligned_address_give_the_same_bits():
    """offset 1: no row of either image starts on the 16-byte grid the vector loads use; W * C = 159 floats per row, so the head and
    the tail of a run change from row to row"""
    geom, x, y, ref, bnd = _case("rect_40x53")
    a = Device(*geom).call(x, y)
    for off in (1, 2, 3):
        b = Device(*geom, offset=off).call(x, y)
        for k in ("vals", "values", "dx", "dy"):
            assert torch.equal(_bits(a[k]), _bits(b[k])), (off, k)
    _hold("offset 3", b, ref, bnd)


def test_dx_alone_and_dy_alone():
    geom, x, y, ref, bnd = _case("rect_40x53")
    both = Device(*geom).call(x, y)
    only_x = Device(*geom).call(x, y, want_dx=True, want_dy=False)
    only_y = Device(*geom).call(x, y, want_dx=False, want_dy=True)
    assert only_x["dy"] is None and only_y["dx"] is None
    assert torch.equal(_bits(only_x["dx"]), _bits(both["dx"])) and torch.equal(_bits(only_y["dy"]), _bits(both["dy"]))
    assert torch.equal(_bits(only_x["vals"]), _bits(both["vals"])) and torch.equal(_bits(only_y["values"]), _bits(both["values"]))
    _hold("dx alone", only_x, ref, bnd)
    _hold("dy alone", only_y, ref, bnd)
    # three maps for one gradient, four for both
    n, c, h, w, window = geom
    lib = Device(*geom).lib
    sizes = [lib.srgan_ssim_workspace(n, c, h, w, window, a, b) for a, b in ((0, 0), (1, 0), (0, 1), (1, 1))]
    maps = -(-(n * c * (h - window + 1) * (w - window + 1) * 4) // 16) * 16
    assert sizes[1] == sizes[2] == sizes[0] + 3 * maps and sizes[3] == sizes[0] + 4 * maps


def test_without_a_gradient_no_coefficient_map_is_written():
    """the workspace of the call holds the tile partials and nothing else: the guard right behind them stays intact (``Device.call``
    checks it), the values are those of the call with a gradient, and the record counts both"""
    geom, x, y, ref, bnd = _case("rect_40x53")
    dev = Device(*geom)
    plain = dev.call(x, y, want_dx=False, want_dy=False)
    n, c, h, w, window = geom
    tiles = -(-(h - window + 1) // sc.TILE[0]) * -(-(w - window + 1) // sc.TILE[1])
    assert plain["ws"].numel() == -(-n * tiles // 4) * 4 and plain["dx"] is None and plain["dy"] is None
    with_grad = dev.call(x, y)
    assert torch.equal(_bits(plain["values"]), _bits(with_grad["values"])) and torch.equal(_bits(plain["vals"]), _bits(with_grad["vals"]))
    assert torch.equal(_bits(plain["ws"][:n * tiles]), _bits(with_grad["ws"][:n * tiles]))
    _hold("no gradient", plain, ref, bnd)
    assert dev.read()["updates"] == 2
    # without a record: weight 1, the constants from the arguments, nothing stored
    free = dev.call(x, y, want_dx=False, want_dy=False, state=False)
    assert torch.equal(_bits(free["values"]), _bits(plain["values"])) and float(free["vals"][0]) == float(free["vals"][1])
    assert dev.read()["updates"] == 2


def test_two_calls_give_equal_bits_and_the_incoming_gradient_scales():
    geom, x, y, ref, bnd = _case("two_channels_w7")
    dev = Device(*geom)
    a, b = dev.call(x, y), dev.call(x, y)
    for k in ("vals", "values", "dx", "dy", "ws"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert dev.read()["updates"] == 2
    scaled = dev.call(x, y, g=-2.5)
    _hold("g = -2.5", scaled, ref, bnd, g=-2.5)
    assert torch.equal(_bits(scaled["values"]), _bits(a["values"]))


def test_the_record_and_a_zero_weight():
    from srgan_amd import ops
    geom, x, y, ref, bnd = _case("valid_T_plus_1")
    dev = Device(*geom, weight=0.0)
    c1, c2 = np.float32(dev.c1), np.float32(dev.c2)
    assert dev.read() == dict(weight=0.0, c1=c1, c2=c2, term=0.0, weighted=0.0, updates=0)
    out = dev.call(x, y)
    assert float(out["vals"][0]) == 0.0 and abs(float(out["vals"][1]) - ref["term"]) <= bnd["term"]
    assert float(out["dx"].abs().max()) == 0.0 and float(out["dy"].abs().max()) == 0.0
    rec = dev.read()
    assert rec["updates"] == 1 and rec["weighted"] == 0.0 and rec["term"] == float(out["vals"][1])
    # set: the three settings and nothing else; restore: the counter and the last values and nothing else
    lib = dev.lib
    assert lib.srgan_ssim_state_set(dev._state(), 2.0, dev.c1, dev.c2, _stream()) == 0
    now = dev.read()
    assert now == dict(rec, weight=2.0)
    assert lib.srgan_ssim_state_restore(dev._state(), 41, 0.25, 0.5, _stream()) == 0
    assert dev.read() == dict(weight=2.0, c1=c1, c2=c2, term=0.25, weighted=0.5, updates=41)
    out2 = dev.call(x, y)
    assert dev.read()["updates"] == 42
    assert torch.equal(_bits(out2["values"]), _bits(out["values"]))
    assert abs(float(out2["vals"][0]) - 2.0 * ref["term"]) <= 2.0 * bnd["term"] + 4 * sc.U * abs(ref["term"])
    r = _note("dx", (out2["dx"].double() - 2.0 / WEIGHT * ref["dx"]).abs(), 2.0 / WEIGHT * bnd["dx"] + 1e-300)
    assert r <= 1.0
    # other constants in the record are what the map kernel reads
    assert lib.srgan_ssim_state_set(dev._state(), 1.0, 4 * dev.c1, 4 * dev.c2, _stream()) == 0
    out3 = dev.call(x, y, want_dx=False, want_dy=False)
    want = sc.reference(x, y, grads=False, window=geom[4], data_range=4.0)
    assert float((out3["values"].double() - want["values"]).abs().max()) <= float(sc.bounds(x, y, window=geom[4], data_range=4.0,
                                                                                            grads=False)["values"].max())
    assert ops.SSIM_TILE == sc.TILE


def test_one_nan_pixel_poisons_its_sample_only():
    geom, x, y, ref, bnd = _case("window_3")
    n, c, h, w, window = geom
    x = x.clone()
    x[2, 1, 7, 9] = float("nan")
    out = Device(*geom).call(x, y)
    assert math.isnan(float(out["values"][2])) and math.isnan(float(out["vals"][0])) and math.isnan(float(out["vals"][1]))
    keep = [0, 1, 3, 4]
    assert _note("values", (out["values"][keep].double() - ref["values"][keep]).abs(), bnd["values"][keep]) <= 1.0
    # the other samples' gradients: inside their bounds (the reference's mean is over all five samples, as the device's k); the
    # poisoned sample's NaN only inside the pixel's window reach and channel
    for name in ("dx", "dy"):
        assert _note(name, (out[name][keep].double() - ref[name][keep]).abs(), bnd[name][keep] + 1e-300) <= 1.0
    bad = torch.isnan(out["dy"][2])
    assert bool(bad[1, 5:10, 7:12].all()) and not bool(bad[0].any()) and not bool(bad[2].any())
    far = torch.ones_like(bad[1])
    far[max(0, 7 - 2 * (window - 1)):7 + 2 * window - 1, max(0, 9 - 2 * (window - 1)):9 + 2 * window - 1] = False
    assert not bool((bad[1] & far).any())


def test_an_asymmetric_tap_table_pins_the_direction_of_both_filters():
    """the C entries take any table of non-negative taps; with an asymmetric one a filter run backwards (forward: tap k on pixel
    o + k; adjoint: tap k on position q - k) gives another number: values, dx and dy against float64 with the same table"""
    asym = [float(v) for v in np.asarray([0.04, 0.09, 0.16, 0.31, 0.40], np.float32)]
    rev = asym[::-1]
    n, c, h, w, window = 2, 3, 17, 41, 5                      # valid 13 x 37: two tiles each way
    x, y = sc.make_pair("gauss", n, c, h, w, seed=21)
    y = (0.5 * x + 0.5 * y).float()
    ref = sc.reference(x, y, weight=WEIGHT, window=window, w=np.asarray(asym))
    bnd = sc.bounds(x, y, weight=WEIGHT, window=window, w=np.asarray(asym))
    out = Device(n, c, h, w, window, taps=asym).call(x, y)
    _hold("asymmetric taps", out, ref, bnd)
    # the check can tell: the reversed table's float64 values and gradients lie far outside the bounds
    wrong = sc.reference(x, y, weight=WEIGHT, window=window, w=np.asarray(rev))
    assert float(((wrong["values"] - ref["values"]).abs() / bnd["values"]).min()) > 100
    assert float(((wrong["dx"] - ref["dx"]).abs() / bnd["dx"]).max()) > 100
    # a wrong direction of the adjoint alone: the right coefficient maps correlated with the reversed table
    X, Y = x.double(), y.double()
    wa = np.asarray(asym, np.float64)
    xs, ys, p, q = sc._shifted(X, Y)
    m = [sc.window_mean(v, wa) for v in (xs, ys, xs * xs, ys * ys, xs * ys)]
    pw = sc.pointwise(m, p, q, float(wa.sum()) ** 2 - 1.0, *sc.constants(), sc._Ops(False))
    k = -WEIGHT / (n * c * pw["value"].shape[-2] * pw["value"].shape[-1])
    for table, same in ((wa, True), (wa[::-1].copy(), False)):
        T = lambda name: sc.full_correlation(pw[name], table)
        dx = k * (T("a_x") + 2 * xs * T("g_s") + ys * T("g_sxy"))
        ratio = float(((dx - ref["dx"]).abs() / bnd["dx"]).max())
        assert (ratio < 1e-3) if same else (ratio > 100), (same, ratio)


def test_ops_ssim_is_a_function_of_its_own():
    from srgan_amd import _lib, ops
    geom, x, y, ref, bnd = _case("rect_40x53")
    state = ops.ss_state_new(torch.device("cuda"), WEIGHT, *sc.constants())
    taps = ops.ssim_taps(11, 1.5)
    assert np.array_equal(np.asarray(taps, np.float64), sc.taps(11, 1.5))
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)          # NCHW-contiguous: ops repacks
    weighted, term, values = ops.ssim(xd, yd, state, taps)
    assert weighted.requires_grad and not term.requires_grad and not values.requires_grad
    (weighted * 3.0).backward()
    out = dict(vals=torch.stack([weighted.detach(), term]).cpu(), values=values.cpu(), dx=xd.grad.cpu(), dy=yd.grad.cpu())
    _hold("ops.ssim", out, ref, bnd, g=3.0)
    # only the second operand wants a gradient (the train step's use), and none: nothing is made for the other
    yd2 = y.cuda().requires_grad_(True)
    w2, _, _ = ops.ssim(x.cuda(), yd2, state, taps)
    w2.backward()
    assert torch.equal(_bits(yd2.grad * 3.0), _bits(yd.grad))
    with torch.no_grad():
        w3, t3, v3 = ops.ssim(x.cuda(), y.cuda(), None, taps)
    assert torch.equal(_bits(v3), _bits(values)) and float(w3) == float(t3) == float(term)
    assert ops.ss_state_read(state)["updates"] == 2
    for bad in (x.cuda().half(), x.cuda().to(torch.bfloat16), x.cuda().double()):
        with pytest.raises(_lib.SrganHipError, match="fp32 images only"):
            ops.ssim(bad, bad, None, taps)
    with pytest.raises(_lib.SrganHipError, match="window"):
        ops.ssim(x.cuda()[:, :, :5], y.cuda()[:, :, :5], None, taps)


def test_psnr_against_float64():
    from srgan_amd import ops
    g = torch.Generator().manual_seed(5)
    for n, shape in ((1, (3, 5, 7)), (5, (3, 40, 53)), (3, (1, 64, 65)), (2, (3, 128, 128))):
        x = torch.rand((n,) + shape, generator=g) * 2 - 1
        y = (x + 0.1 * torch.randn((n,) + shape, generator=g)).clamp(-1, 1)
        y[0] = x[0]                                            # mse == 0 -> +inf
        got = ops.psnr(x.cuda(), y.cuda()).cpu()
        want = sc.psnr(x, y)
        assert got.dtype == torch.float64 and math.isinf(float(got[0])) and float(got[0]) > 0
        if n > 1:
            r = _note("psnr", (got[1:] - want[1:]).abs(), torch.full_like(want[1:], sc.psnr_bound(x, y)))
            assert r <= 1.0
        one = ops.psnr(x.cuda(), y.cuda(), data_range=1.0).cpu()
        if n > 1:
            assert float((one[1:] - sc.psnr(x, y, 1.0)[1:]).abs().max()) <= sc.psnr_bound(x, y)


def test_evaluation_metrics_and_their_chunks():
    from srgan_amd import evaluation
    geom, x, y, ref, bnd = _case("window_3")
    want = sc.reference(x, y, grads=False, window=3, sigma=1.0)
    b = sc.bounds(x, y, window=3, sigma=1.0, grads=False)["values"]
    whole = evaluation.compute_ssim(x.numpy(), y, window=3, sigma=1.0)
    assert isinstance(whole, np.ndarray) and whole.dtype == np.float32 and whole.shape == (5,)
    assert _note("values", (torch.from_numpy(whole).double() - want["values"]).abs(), b) <= 1.0
    chunked = evaluation.compute_ssim(x, y.numpy(), window=3, sigma=1.0, chunk=2)          # slices of 2, 2, 1 samples
    assert np.array_equal(whole, chunked)
    p = evaluation.compute_psnr(x.numpy(), y.numpy())
    p2 = evaluation.compute_psnr(x, y, chunk=2)
    assert p.dtype == np.float64 and np.array_equal(p, p2)
    assert _note("psnr", (torch.from_numpy(p) - sc.psnr(x, y)).abs(), torch.full((5,), sc.psnr_bound(x, y), dtype=torch.float64)) <= 1.0
    with pytest.raises(ValueError, match="one shape"):
        evaluation.compute_ssim(x, y[:, :, :-1])
    with pytest.raises(ValueError, match="chunk"):
        evaluation.compute_psnr(x, y, chunk=0)


def test_the_worst_ratios_of_this_run():
    """last in the file: the worst error / bound of every checked quantity (DESIGN.md section 7 quotes a run)"""
    print("ssim | worst err / bound:", {k: round(v, 3) for k, v in sorted(WORST.items())})
    assert WORST and all(v <= 1.0 for v in WORST.values())
