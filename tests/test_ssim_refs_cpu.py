"""CPU: the references of the structural-similarity tests and the host side of the feature.  The float64 restatement of
tests/ssim_common.py against two independent ones and against closed forms; the derived bound excludes every mutation of the
definition; raw float32 moments break it on low-contrast images near the end of the range while the shifted form meets it on every
case; the shifted gradient formula equals autograd; the settings' refusals; the record's layout, its write masks and
csrc/ssim_math.h through a sanitized stand-alone host program; the C entries' refusals without a GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import ssim_common as sc

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "style-restricted_gan_amd", "csrc")


@pytest.fixture(autouse=True, scope="module")
def the_references_restate_what_the_package_uses():
    """every test of this file stands on it: the window and the constants of ``tests/ssim_common.py`` are the package's, bit for
    bit (``ops.ssim_taps`` is csrc/ssim_math.h's table), and its tile is the kernels'"""
    from srgan_amd import ops, structural
    for window in (3, 5, 7, 9, 11):
        for sigma in (0.8, 1.5, 3.0):
            assert np.array_equal(np.asarray(ops.ssim_taps(window, sigma), np.float64), sc.taps(window, sigma)), (window, sigma)
    s = structural.SSIM(**{k: v for k, v in sc.DEFAULTS.items()})
    assert (s.c1, s.c2) == sc.constants() and (s.c1, s.c2) == (4e-4 * 1.0, (0.03 * 2.0) ** 2) and ops.SSIM_TILE == sc.TILE


def _scipy_map(x, y, window, sigma, k1=0.01, k2=0.03, data_range=2.0):
    """an independent float64 restatement: scipy's 1-d correlation along each axis, cropped to the valid positions"""
    from scipy.ndimage import correlate1d
    w = sc.taps(window, sigma)
    c1, c2 = sc.constants(k1, k2, data_range)
    r = (window - 1) // 2

    def mean(v):
        out = correlate1d(correlate1d(v, w, axis=-1, mode="constant"), w, axis=-2, mode="constant")
        return out[..., r:v.shape[-2] - r, r:v.shape[-1] - r]

    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    mx, my = mean(x), mean(y)
    sx, sy, sxy = mean(x * x) - mx * mx, mean(y * y) - my * my, mean(x * y) - mx * my
    return ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sx + sy + c2))


@pytest.mark.parametrize("name", ["rect_40x53", "tall_narrow", "two_channels_w7", "window_3", "offset_01", "saturated"])
def test_the_restatement_agrees_with_scipy(name):
    _, n, c, h, w, window, kind = next(k for k in sc.CASES if k[0] == name)
    x, y = sc.make_pair(kind, n, c, h, w, seed=len(name))
    mine = sc.ssim_map(x.double(), y.double(), window=window).numpy()
    theirs = _scipy_map(x.numpy(), y.numpy(), window, 1.5)
    assert mine.shape == theirs.shape == (n, c, h - window + 1, w - window + 1)
    assert float(np.abs(mine - theirs).max()) <= 1e-12


def test_the_restatement_agrees_with_a_direct_double_loop():
    x, y = sc.make_pair("gauss", 1, 2, 6, 7, seed=3)
    window, w = 5, sc.taps(5, 1.5)
    c1, c2 = sc.constants()
    mine = sc.ssim_map(x.double(), y.double(), window=window)
    X, Y = x.double().numpy(), y.double().numpy()
    for c in range(2):
        for oy in range(2):
            for ox in range(3):
                e = dict.fromkeys(("x", "y", "xx", "yy", "xy"), 0.0)
                for i in range(window):
                    for j in range(window):
                        a, b, ww = X[0, c, oy + i, ox + j], Y[0, c, oy + i, ox + j], w[i] * w[j]
                        e["x"] += ww * a; e["y"] += ww * b; e["xx"] += ww * a * a; e["yy"] += ww * b * b; e["xy"] += ww * a * b
                sx, sy, sxy = e["xx"] - e["x"] ** 2, e["yy"] - e["y"] ** 2, e["xy"] - e["x"] * e["y"]
                want = (2 * e["x"] * e["y"] + c1) * (2 * sxy + c2) / ((e["x"] ** 2 + e["y"] ** 2 + c1) * (sx + sy + c2))
                assert abs(float(mine[0, c, oy, ox]) - want) <= 1e-13


def test_closed_forms():
    x, y = sc.make_pair("gauss", 2, 3, 20, 23, seed=1)
    same = sc.reference(x, x, grads=False)
    assert float((same["values"] - 1).abs().max()) <= 1e-12 and abs(same["term"]) <= 1e-12
    a, b = sc.reference(x, y, grads=False), sc.reference(y, x, grads=False)
    assert abs(a["term"] - b["term"]) <= 1e-15 and float((a["values"] - b["values"]).abs().max()) <= 1e-15
    cx, cy = sc.make_pair("const", 2, 3, 13, 14)
    got = sc.reference(cx, cy, grads=False)
    A, B = cx[:, :, 0, 0].double(), cy[:, :, 0, 0].double()
    c1 = sc.constants()[0]
    # the fp32 taps sum to 1 - 1.4e-9, so s_x = a^2 (W - W^2) with W = 1 - 2.8e-9 and not 0: the closed form holds to
    # (|a| + |b|)^2 |W - 1| / C2 of the value
    assert float((got["values"] - ((2 * A * B + c1) / (A * A + B * B + c1)).mean(1)).abs().max()) <= sc.closed_form_slack(A, B)
    # the taps: symmetric, fp32 numbers, of sum 1 to the rounding of 11 of them
    for window in (3, 5, 7, 9, 11):
        w = sc.taps(window, 1.5)
        assert np.array_equal(w, w[::-1]) and np.array_equal(w, w.astype(np.float32).astype(np.float64)) and abs(w.sum() - 1) < 1e-7
    # PSNR
    p = sc.psnr(x, torch.stack([x[0], x[1] + 0.5]))
    assert float(p[0]) == float("inf") and abs(float(p[1]) - 10 * np.log10(4 / 0.25)) < 1e-6    # (x + 0.5 rounds in float32)


@pytest.mark.parametrize("mutation", sc.MUTATIONS)
def test_the_bound_excludes_every_mutation(mutation):
    """the derived bound is not vacuous: on the chosen inputs (variances of the size of C2; flat images near the end of the range)
    the float64 value of the wrong formula lies outside it, 20 times over.  (On high-contrast noise the sample covariance moves the
    term by less than the bound: the factor 121 / 120 cancels in the quotient where C2 is small beside the variances.)"""
    for kind in ("midcontrast", "offset01"):
        name, n, c, h, w, window = kind, 2, 3, 40, 53, 11
        x, y = sc.make_pair(kind, n, c, h, w, seed=3)
        true = sc.reference(x, y, grads=False, window=window)["term"]
        bound = sc.bounds(x, y, window=window, grads=False)["term"]
        wrong = sc.mutated_term(mutation, x, y, window=window)
        print(f"{mutation} on {name}: true {true:.9f} wrong {wrong:.9f} bound {bound:.2e}")
        assert abs(wrong - true) > 20 * bound, (mutation, name, true, wrong, bound)


WORST = {}


@pytest.mark.parametrize("name", sc.CASE_IDS)
def test_the_shifted_float32_form_meets_the_bound_on_every_case(name):
    _, n, c, h, w, window, kind = next(k for k in sc.CASES if k[0] == name)
    x, y = sc.make_pair(kind, n, c, h, w, seed=len(name))
    ref = sc.reference(x, y, grads=False, window=window)["map"]
    bound = sc.bounds(x, y, window=window, grads=False)["map"]
    err = (sc.emulate32(x, y, True, window=window) - ref).abs()
    ratio = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())
    WORST[name] = ratio
    print(f"{name}: shifted float32 emulation, max err {float(err.max()):.3e}, worst err / bound {ratio:.3f}")
    assert ratio <= 1.0
    assert abs(ratio - sc.EMULATED[name]) <= 0.02 + 0.1 * sc.EMULATED[name], "the recorded ratio of tests/ssim_common.py is stale"


@pytest.mark.parametrize("name", ["offset_01", "offset_001"])
def test_raw_float32_moments_break_the_bound_on_flat_images_near_the_end_of_the_range(name):
    _, n, c, h, w, window, kind = next(k for k in sc.CASES if k[0] == name)
    x, y = sc.make_pair(kind, n, c, h, w, seed=len(name))
    ref = sc.reference(x, y, grads=False, window=window)["map"]
    bound = sc.bounds(x, y, window=window, grads=False)["map"]
    err = (sc.emulate32(x, y, False, window=window) - ref).abs()
    print(f"{name}: raw float32 moments, max err {float(err.max()):.3e}, worst err / bound {float((err / bound).max()):.1f}")
    assert float(err.max()) > 5e-5 and float((err / bound).max()) > 50


def test_the_shifted_gradient_formula_equals_autograd():
    """d term / dx = k (T[A_x] + 2 (x - p) T[g_s] + (y - q) T[g_sxy]) with the coefficients of ``pointwise`` (csrc/ssim_math.h's
    sequence) and T the full correlation, in float64, against autograd through the raw definition; also on a flat image"""
    for kind, window, shape in (("gauss", 7, (2, 3, 15, 18)), ("offset01", 11, (1, 3, 14, 16)), ("near", 3, (3, 1, 6, 5))):
        x, y = sc.make_pair(kind, *shape, seed=7)
        ref = sc.reference(x, y, weight=1.5, window=window)
        X, Y = x.double(), y.double()
        w = sc.taps(window, 1.5)
        xs, ys, p, q = sc._shifted(X, Y)
        m = [sc.window_mean(v, w) for v in (xs, ys, xs * xs, ys * ys, xs * ys)]
        out = sc.pointwise(m, p, q, float(w.sum()) ** 2 - 1.0, *sc.constants(), sc._Ops(False))
        assert float((out["value"] - ref["map"]).abs().max()) <= 1e-12
        n, c = shape[:2]
        k = -1.5 / (n * c * out["value"].shape[-2] * out["value"].shape[-1])
        T = lambda name: sc.full_correlation(out[name], w)
        dx = k * (T("a_x") + 2 * xs * T("g_s") + ys * T("g_sxy"))
        dy = k * (T("a_y") + 2 * ys * T("g_s") + xs * T("g_sxy"))
        scale = float(ref["dx"].abs().max())
        assert float((dx - ref["dx"]).abs().max()) <= 1e-11 * max(scale, 1.0) and float((dy - ref["dy"]).abs().max()) <= 1e-11 * max(scale, 1.0)
        b = sc.bounds(x, y, weight=1.5, window=window)
        assert bool((b["dx"] > 0).all()) and bool((b["map"] > 0).all()) and float(b["dx"].max()) < 1e-2 * max(scale, 1e-6) + 1e-7


def test_check_settings_and_the_object_without_a_device():
    from srgan_amd import structural
    ok = structural.check_settings(1, 11, 1.5, 0.01, 0.03, 2.0)
    assert ok == (1.0, 11, 1.5, 0.01, 0.03, 2.0) and isinstance(ok[0], float)
    for bad, what in ((dict(weight=-1.0), "weight"), (dict(weight=float("nan")), "weight"), (dict(weight=float("inf")), "weight"),
                      (dict(weight="a"), "weight"), (dict(window=4), "window"), (dict(window=13), "window"), (dict(window=1), "window"),
                      (dict(window=5.0), "window"), (dict(window=True), "window"), (dict(sigma=0.0), "sigma"),
                      (dict(sigma=float("nan")), "sigma"), (dict(k1=-0.01), "k1"), (dict(k2=0.0), "k2"), (dict(k2=float("inf")), "k2"),
                      (dict(data_range=0.0), "data_range"), (dict(data_range=-2.0), "data_range")):
        with pytest.raises(ValueError, match=what):
            structural.SSIM(**bad)
    s = structural.SSIM(weight=0.5, window=7, sigma=1.0, data_range=1.0)
    assert s.state is None and s.c1 == (0.01 * 1.0) ** 2 and s.c2 == (0.03 * 1.0) ** 2
    assert np.array_equal(np.asarray(s.taps, np.float64), sc.taps(7, 1.0))
    assert s.stats() == dict(weight=0.5, window=7, sigma=1.0, k1=0.01, k2=0.03, data_range=1.0, term=0.0, weighted=0.0, updates=0)
    s.set_weight(2)
    assert s.weight == 2.0 and s.state is None
    with pytest.raises(ValueError, match="weight"):
        s.set_weight(-1)
    sd = s.state_dict()
    assert sd == dict(weight=2.0, window=7, sigma=1.0, k1=0.01, k2=0.03, data_range=1.0, updates=0, term=0.0, weighted=0.0)
    t = structural.SSIM(window=7, sigma=1.0, data_range=1.0)
    t.load_state_dict(sd)
    assert t.weight == 2.0 and t.state is None and t.fingerprint() != s.fingerprint()
    with pytest.raises(ValueError, match="window, sigma"):
        structural.SSIM().load_state_dict(sd)
    with pytest.raises(ValueError, match="device"):
        t.load_state_dict(dict(sd, updates=3))
    from srgan_amd.trainer import SingleGAN_training, SRGAN_training
    with pytest.raises(NotImplementedError, match="SRGAN_training.enable_ssim"):
        SingleGAN_training.enable_ssim(object())
    for name in ("enable_ssim", "disable_ssim", "set_ssim_weight", "ssim_stats"):
        assert callable(getattr(SRGAN_training, name))
    from srgan_amd import checkpoint, evaluation
    assert "ssim" in checkpoint._EXTENSIONS and callable(evaluation.compute_ssim) and callable(evaluation.compute_psnr)
    assert callable(evaluation.GAN_evaluation.get_ssim) and callable(evaluation.GAN_evaluation.get_psnr)


def test_the_record_and_the_header_through_a_sanitized_host_program(tmp_path):
    """tests/ssim_host_check.cpp: a stand-alone program, built with the address and undefined-behaviour sanitizers and run here"""
    from srgan_amd import _lib
    lib = _lib.load()
    S = _lib.SsState
    assert ctypes.sizeof(S) == lib.srgan_ssim_state_bytes() == 32
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("weight", 0), ("c1", 4), ("c2", 8), ("term", 12), ("weighted", 16),
                                                                  ("updates", 20), ("_pad", 24)]
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = os.path.join(str(tmp_path), "ssim_host_check")
    built = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I" + CSRC, os.path.join(HERE, "ssim_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ssim host check ok") and not r.stderr.strip(), (r.stdout, r.stderr[-3000:])
    seen = {}
    for line in r.stdout.splitlines():
        if line.startswith("taps "):
            f = line.split()
            seen[int(f[1])] = np.asarray([float.fromhex(v) for v in f[2:]])
    assert sorted(seen) == [3, 5, 7, 9, 11]
    from srgan_amd import ops
    for window, w in seen.items():
        assert np.array_equal(w, sc.taps(window, 1.5)), window                       # the header's table == numpy's, bit for bit
        assert np.array_equal(np.asarray(ops.ssim_taps(window, 1.5)), w)


def test_the_entries_refuse_bad_arguments_without_a_gpu():
    from srgan_amd import _lib, ops
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    big = (ctypes.c_char * (1 << 16))()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ws = ctypes.c_void_p((ctypes.addressof(big) + 15) & ~15)
    taps = (ctypes.c_float * 11)(*ops.ssim_taps(11, 1.5))
    taps3 = (ctypes.c_float * 3)(*ops.ssim_taps(3, 1.5))
    nan, inf = float("nan"), float("inf")

    def refused(rc, what):
        assert rc == -1, what
        msg = lib.srgan_last_error().decode()
        assert what in msg, (what, msg)

    for entry in (lib.srgan_ssim_state_init, lib.srgan_ssim_state_set):
        name = "ssim_state_init" if entry is lib.srgan_ssim_state_init else "ssim_state_set"
        for args in ((None, 1.0, 4e-4, 3.6e-3), (p, -1.0, 4e-4, 3.6e-3), (p, nan, 4e-4, 3.6e-3), (p, inf, 4e-4, 3.6e-3),
                     (p, 1.0, -1e-4, 3.6e-3), (p, 1.0, nan, 3.6e-3), (p, 1.0, 4e-4, 0.0), (p, 1.0, 4e-4, nan), (p, 1.0, 4e-4, inf)):
            refused(entry(*args, None), name)
    for args in ((None, 0, 0.0, 0.0), (p, -1, 0.0, 0.0), (p, 0, nan, 0.0), (p, 0, 0.0, inf)):
        refused(lib.srgan_ssim_state_restore(*args, None), "ssim_state_restore")
    for args in ((4, 1.5, buf), (13, 1.5, buf), (1, 1.5, buf), (11, 0.0, buf), (11, nan, buf), (11, 1.5, None)):
        refused(lib.srgan_ssim_taps(*args), "ssim_taps")
    # geometry: n, c, h, w, window
    bad_geometry = ((0, 3, 16, 16, 11), (1, 0, 16, 16, 11), (1, 4, 16, 16, 11), (1, 3, 16, 16, 10), (1, 3, 16, 16, 13), (1, 3, 16, 16, 1),
                    (1, 3, 10, 16, 11), (1, 3, 16, 10, 11), (2, 3, 32768, 16384, 11), (-1, 3, 16, 16, 11))
    for g in bad_geometry:
        assert lib.srgan_ssim_workspace(*g, 1, 1) == 0 and b"ssim_workspace" in lib.srgan_last_error()
        t = taps3 if g[4] == 3 else taps
        refused(lib.srgan_ssim_map(p, p, *g, t, None, 4e-4, 3.6e-3, 0, 0, ws, 1 << 15, None), "ssim_map: bad geometry")
        refused(lib.srgan_ssim_finish(ws, 1 << 15, *g, None, p, p, None), "ssim_finish: bad geometry")
        refused(lib.srgan_ssim_grad(p, p, *g, t, ws, 1 << 15, None, None, ws, None, None), "ssim_grad: bad geometry")
    g = (1, 3, 16, 16, 11)
    need0, need1, need2 = (lib.srgan_ssim_workspace(*g, a, b) for a, b in ((0, 0), (0, 1), (1, 1)))
    assert need0 == 16 and need1 == 16 + 3 * 432 and need2 == 16 + 4 * 432
    q = ctypes.c_void_p(p.value + 4096)
    # null pointers
    refused(lib.srgan_ssim_map(None, p, *g, taps, None, 4e-4, 3.6e-3, 0, 0, ws, need0, None), "ssim_map: null pointer")
    refused(lib.srgan_ssim_map(p, None, *g, taps, None, 4e-4, 3.6e-3, 0, 0, ws, need0, None), "ssim_map: null pointer")
    refused(lib.srgan_ssim_map(p, p, *g, None, None, 4e-4, 3.6e-3, 0, 0, ws, need0, None), "ssim_map: null pointer")
    refused(lib.srgan_ssim_map(p, p, *g, taps, None, 4e-4, 3.6e-3, 0, 0, None, need0, None), "ssim_map: null pointer")
    refused(lib.srgan_ssim_finish(None, need0, *g, None, p, p, None), "ssim_finish: null pointer")
    refused(lib.srgan_ssim_finish(ws, need0, *g, None, None, p, None), "ssim_finish: null pointer")
    refused(lib.srgan_ssim_finish(ws, need0, *g, None, p, None, None), "ssim_finish: null pointer")
    refused(lib.srgan_ssim_grad(p, p, *g, taps, ws, need2, None, None, None, None, None), "ssim_grad: null pointer")
    refused(lib.srgan_ssim_grad(None, p, *g, taps, ws, need2, None, None, q, None, None), "ssim_grad: null pointer")
    # a short workspace, a misaligned one, misaligned images, a bad tap, bad constants without a record, aliasing
    refused(lib.srgan_ssim_map(p, p, *g, taps, None, 4e-4, 3.6e-3, 0, 0, ws, need0 - 1, None), "ssim_map: workspace")
    refused(lib.srgan_ssim_map(p, p, *g, taps, None, 4e-4, 3.6e-3, 0, 1, ws, need1 - 1, None), "ssim_map: workspace")
    refused(lib.srgan_ssim_map(p, p, *g, taps, None, 4e-4, 3.6e-3, 1, 1, ws, need1, None), "ssim_map: workspace")
    refused(lib.srgan_ssim_finish(ws, need0 - 1, *g, None, p, p, None), "ssim_finish: workspace")
    refused(lib.srgan_ssim_grad(p, p, *g, taps, ws, need2 - 1, None, None, q, ctypes.c_void_p(q.value + 4096), None), "ssim_grad: workspace")
    refused(lib.srgan_ssim_map(p, p, *g, taps, None, 4e-4, 3.6e-3, 0, 0, ctypes.c_void_p(ws.value + 4), need0, None), "16-byte aligned")
    refused(lib.srgan_ssim_map(ctypes.c_void_p(p.value + 2), p, *g, taps, None, 4e-4, 3.6e-3, 0, 0, ws, need0, None), "4-byte aligned")
    refused(lib.srgan_ssim_grad(p, p, *g, taps, ws, need2, None, None, ctypes.c_void_p(q.value + 1), None, None), "4-byte aligned")
    for k, v in ((0, nan), (5, -0.25), (10, inf)):
        bad = (ctypes.c_float * 11)(*ops.ssim_taps(11, 1.5))
        bad[k] = v
        refused(lib.srgan_ssim_map(p, p, *g, bad, None, 4e-4, 3.6e-3, 0, 0, ws, need0, None), "ssim_map: a tap")
        refused(lib.srgan_ssim_grad(p, p, *g, bad, ws, need1, None, None, q, None, None), "ssim_grad: a tap")
    for c1, c2 in ((nan, 3.6e-3), (-1.0, 3.6e-3), (4e-4, 0.0), (4e-4, nan)):
        refused(lib.srgan_ssim_map(p, p, *g, taps, None, c1, c2, 0, 0, ws, need0, None), "ssim_map: without a record")
    refused(lib.srgan_ssim_grad(p, q, *g, taps, ws, need1, None, None, p, None, None), "aliases")
    refused(lib.srgan_ssim_grad(p, q, *g, taps, ws, need2, None, None, ws, ws, None), "aliases")
    # PSNR
    out = ctypes.c_void_p((ctypes.addressof(big) + 32768 + 7) & ~7)
    assert lib.srgan_psnr_workspace(0, 10) == 0 and lib.srgan_psnr_workspace(1, 0) == 0 and lib.srgan_psnr_workspace(2, 1 << 30) == 0
    assert lib.srgan_psnr_workspace(3, 4097) == 24
    refused(lib.srgan_psnr(None, p, 1, 16, 2.0, out, ws, 64, None), "psnr: null pointer")
    refused(lib.srgan_psnr(p, p, 1, 16, 2.0, None, ws, 64, None), "psnr: null pointer")
    refused(lib.srgan_psnr(p, p, 0, 16, 2.0, out, ws, 64, None), "psnr: bad geometry")
    refused(lib.srgan_psnr(p, p, 2, 1 << 30, 2.0, out, ws, 64, None), "psnr: bad geometry")
    for r in (0.0, -1.0, nan, inf):
        refused(lib.srgan_psnr(p, p, 1, 16, r, out, ws, 64, None), "psnr: data_range")
    refused(lib.srgan_psnr(p, p, 3, 4097, 2.0, out, ws, 23, None), "psnr: workspace")
    refused(lib.srgan_psnr(p, p, 1, 16, 2.0, ctypes.c_void_p(out.value + 4), ws, 64, None), "8-byte aligned")
    # ops refuses what needs no device to refuse
    with pytest.raises(_lib.SrganHipError, match="ssim_taps"):
        ops.ssim_taps(4, 1.5)
    with pytest.raises(_lib.SrganHipError, match="window"):
        ops.ssim_taps(11.0, 1.5)
    with pytest.raises(_lib.SrganHipError, match="fp32 images only"):
        ops.ssim(torch.zeros(1, 3, 16, 16, dtype=torch.float16), torch.zeros(1, 3, 16, 16, dtype=torch.float16), None, ops.ssim_taps(11, 1.5))
    with pytest.raises(_lib.SrganHipError, match="no CPU fallback"):
        ops.ssim(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16), None, ops.ssim_taps(11, 1.5))
