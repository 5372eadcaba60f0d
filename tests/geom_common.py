"""Yardstick of the geometric-augmentation tests (csrc/augment_geom.hip, srgan_amd.augment.GeometricAugment): the warp restated in
torch on the CPU from the specification, its adjoint in gather form, the case lists and builders of hand-made tables.  No GPU
code: tests/test_geom_refs_cpu.py pins what is in here (against ``F.grid_sample`` and autograd), tests/test_geom_kernels_gpu.py and
tests/test_geom_train_gpu.py hold the HIP kernels and the train step to it.

One row [fx, k, zoom, cos, sin, 0, 0, mask] per sample; flags flip 1, rot90 2, scale 4, rotate 8; a group that is off (at launch,
or by the row's mask in the gated form) takes its identity value 0, 0, 1, (1, 0).  With cen = ((H - 1) / 2, (W - 1) / 2), offsets
in (row, col) order:

    forward   y[q] = bilinear(x, s(q)),  s(q) = cen + M (q - cen),  M = R(cos, sin) Q(k) F(fx) / zoom;  outside pixels read 0
    adjoint   gx[p] = sum_q hat(s_i(q) - p_i) hat(s_j(q) - p_j) gy[q],  hat(t) = max(0, 1 - |t|), over the 7 x 7 output pixels
              around floor(q* + 0.5), q* = cen + zoom (R Q F)^T (p - cen), row-major

The kernel's window has radius min(ceil(zoom (|cos| + |sin|)), 3) <= 3; a candidate outside the support weighs exactly 0, so the
fixed 7 x 7 window here adds the same terms in the same order plus exact zeros.  Every product and sum is written in the order the
kernels use, so the float32 run of these functions is "the same formulas in float32": ``e32`` of the bound.

Error measure and bound: ``augment_common.check`` -- per sample ``max(8 * e32, gamma(L))``, L = 8 forward (four taps, a product and
an add each), L = 49 backward (the window's serial adds)."""
import math
import os
import shutil
import subprocess

import torch

from tests.augment_common import check, inputs, sample_errs  # noqa: F401  (the suite's bound and inputs, shared)

FLIP, ROT90, SCALE, ROTATE = 1, 2, 4, 8
ALL = 15
ROW = 8
L_FWD, L_BWD = 8, 49
# what csrc/augment_geom.hip cuts its work by: pixels per item, workgroups per launch
ITEM_PIXELS, GRID_CAP = 2048, 2048
MAX_RADIUS = 3


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def effective(table, flags, gated=False):
    """per sample (fx, k, zoom, cos, sin) after the launch flags and (gated) the row's skip mask: int64, int64, float32 x 3"""
    t = table.detach().cpu().to(torch.float32)
    n = t.shape[0]
    eff = torch.full((n,), int(flags), dtype=torch.int64)
    if gated:
        eff = eff & ~(t[:, 7].to(torch.int64) & ALL)
    on = lambda bit: (eff & bit) != 0          # noqa: E731
    fx = torch.where(on(FLIP), t[:, 0].to(torch.int64) & 1, torch.zeros(n, dtype=torch.int64))
    k = torch.where(on(ROT90), t[:, 1].to(torch.int64) & 3, torch.zeros(n, dtype=torch.int64))
    zoom = torch.where(on(SCALE), t[:, 2], torch.ones(n))
    c = torch.where(on(ROTATE), t[:, 3], torch.ones(n))
    s = torch.where(on(ROTATE), t[:, 4], torch.zeros(n))
    return fx, k, zoom, c, s


def maps(table, flags, dtype, gated=False):
    """(M [n, 2, 2], T [n, 2, 2]) in ``dtype``: source offset = M (output offset); window centre offset = T (input offset)"""
    fx, k, zoom, c, s = effective(table, flags, gated)
    ck = torch.tensor([1.0, 0.0, -1.0, 0.0])[k].to(dtype)
    sk = torch.tensor([0.0, 1.0, 0.0, -1.0])[k].to(dtype)
    sgn = (1 - 2 * fx).to(dtype)
    zoom, c, s = zoom.to(dtype), c.to(dtype), s.to(dtype)
    a00 = c * ck - s * sk
    a01 = (c * -sk - s * ck) * sgn
    a10 = s * ck + c * sk
    a11 = (s * -sk + c * ck) * sgn
    M = torch.stack([torch.stack([a00 / zoom, a01 / zoom], -1), torch.stack([a10 / zoom, a11 / zoom], -1)], -2)
    T = torch.stack([torch.stack([zoom * a00, zoom * a10], -1), torch.stack([zoom * a01, zoom * a11], -1)], -2)
    return M, T


def radius(table, flags, gated=False):
    """the kernel's window radius per sample (float32 arithmetic): int64 [n]"""
    _, _, zoom, c, s = effective(table, flags, gated)
    return torch.ceil(zoom * (c.abs() + s.abs())).clamp(max=MAX_RADIUS).to(torch.int64)


def _source(M, h, w, qi, qj, dtype):
    """s(q) for offsets-free pixel coordinates qi [.., h, 1] / qj [.., 1, w] (tensors of ``dtype``): (si, sj) [n, h, w]"""
    n = M.shape[0]
    ci, cj = (h - 1) / 2, (w - 1) / 2
    di, dj = qi - ci, qj - cj
    si = M[:, 0, 0].view(n, 1, 1) * di + M[:, 0, 1].view(n, 1, 1) * dj + ci
    sj = M[:, 1, 0].view(n, 1, 1) * di + M[:, 1, 1].view(n, 1, 1) * dj + cj
    return si, sj


def restate(x, table, flags, dtype=torch.float64, gated=False):
    """y = warp(x) in ``dtype`` on the CPU (differentiable in x when x is a ``dtype`` leaf)"""
    x = x.cpu().to(dtype)
    n, ch, h, w = x.shape
    assert ch == 3 and tuple(table.shape) == (n, ROW)
    M, _ = maps(table, flags, dtype, gated)
    qi = torch.arange(h, dtype=dtype).view(1, h, 1)
    qj = torch.arange(w, dtype=dtype).view(1, 1, w)
    si, sj = _source(M, h, w, qi, qj, dtype)
    i0, j0 = torch.floor(si), torch.floor(sj)
    fi, fj = si - i0, sj - j0
    flat = x.flatten(2)
    y = torch.zeros_like(x)
    for di, wi in ((0, 1 - fi), (1, fi)):
        for dj, wj in ((0, 1 - fj), (1, fj)):
            ii, jj = (i0 + di).long(), (j0 + dj).long()
            ok = (ii >= 0) & (ii < h) & (jj >= 0) & (jj < w)
            idx = (ii.clamp(0, h - 1) * w + jj.clamp(0, w - 1)).view(n, 1, h * w).expand(n, ch, h * w)
            v = flat.gather(2, idx).view(n, ch, h, w)
            y = y + v * ((wi * wj) * ok).unsqueeze(1)
    return y


def restate_with_grad(x, gy, table, flags, dtype, gated=False):
    """(y, gx) of the restatement in ``dtype``: gx by autograd"""
    leaf = x.detach().cpu().to(dtype).requires_grad_(True)
    y = restate(leaf, table, flags, dtype, gated)
    (gx,) = torch.autograd.grad(y, leaf, gy.detach().cpu().to(dtype))
    return y.detach(), gx.detach()


def adjoint_gather(gy, table, flags, dtype=torch.float64, gated=False):
    """the gather-form adjoint in ``dtype``: the 7 x 7 window around floor(q* + 0.5), row-major, the whole batch at once"""
    gy = gy.detach().cpu().to(dtype)
    n, ch, h, w = gy.shape
    M, T = maps(table, flags, dtype, gated)
    ci, cj = (h - 1) / 2, (w - 1) / 2
    pi = torch.arange(h, dtype=dtype).view(1, h, 1)
    pj = torch.arange(w, dtype=dtype).view(1, 1, w)
    di, dj = pi - ci, pj - cj
    ri = torch.floor((T[:, 0, 0].view(n, 1, 1) * di + T[:, 0, 1].view(n, 1, 1) * dj + ci).clamp(-4, h + 3) + 0.5)
    rj = torch.floor((T[:, 1, 0].view(n, 1, 1) * di + T[:, 1, 1].view(n, 1, 1) * dj + cj).clamp(-4, w + 3) + 0.5)
    flat = gy.flatten(2)
    gx = torch.zeros_like(gy)
    for oi in range(-MAX_RADIUS, MAX_RADIUS + 1):
        for oj in range(-MAX_RADIUS, MAX_RADIUS + 1):
            qi, qj = ri + oi, rj + oj
            ok = (qi >= 0) & (qi < h) & (qj >= 0) & (qj < w)
            si, sj = _source(M, h, w, qi, qj, dtype)
            wt = (1 - (si - pi).abs()).clamp_min(0) * (1 - (sj - pj).abs()).clamp_min(0) * ok
            idx = (qi.clamp(0, h - 1) * w + qj.clamp(0, w - 1)).long().view(n, 1, h * w).expand(n, ch, h * w)
            gx = gx + flat.gather(2, idx).view(n, ch, h, w) * wt.unsqueeze(1)
    return gx


def grid_sample_form(x, table, flags):
    """the same warp through ``F.grid_sample(bilinear, zeros, align_corners=False)`` in float64"""
    import torch.nn.functional as F
    x = x.cpu().double()
    n, _, h, w = x.shape
    M, _ = maps(table, flags, torch.float64)
    si, sj = _source(M, h, w, torch.arange(h, dtype=torch.float64).view(1, h, 1), torch.arange(w, dtype=torch.float64).view(1, 1, w),
                     torch.float64)
    grid = torch.stack([(2 * sj + 1) / w - 1, (2 * si + 1) / h - 1], -1)
    return F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def permutation(x, fx, k):
    """what a pure flip / rot90 row must give, bit for bit: y[q] = x[Q(k) F(fx) q] about the centre -- k quarter turns clockwise
    (``torch.rot90`` counts them counter-clockwise), then the columns of the result mirrored"""
    y = torch.rot90(x, -k, (2, 3))
    return y.flip(3) if fx else y


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def build_table(rows):
    """(fx, k, zoom, theta) per sample -> float32 [n, 8] as GeometricAugment.draw lays it out (cos / sin from float64)"""
    t = torch.zeros(len(rows), ROW, dtype=torch.float32)
    for i, (fx, k, zoom, theta) in enumerate(rows):
        th = torch.tensor(theta, dtype=torch.float64)
        t[i, 0], t[i, 1], t[i, 2] = float(fx), float(k), float(zoom)
        t[i, 3], t[i, 4] = torch.cos(th).to(torch.float32), torch.sin(th).to(torch.float32)
    return t


PI = math.pi
# both ends of the zoom range, the quarter and eighth turns, the largest footprints (an output pixel spread over the most inputs at
# zoom 0.5, an input pixel read by the most outputs at zoom 2, both at 45 degrees), the identity
EXTREME_ROWS = [
    (0, 0, 0.5, 0.0), (0, 0, 2.0, 0.0), (0, 0, 1.0, PI / 4), (0, 0, 1.0, -PI / 4), (1, 1, 1.0, PI / 2), (0, 2, 1.0, -PI / 2),
    (1, 3, 1.0, PI), (0, 0, 1.0, -PI), (0, 0, 0.5, PI / 4), (1, 1, 2.0, PI / 4), (0, 0, 1.0, 0.0),
]


def _rotations(n, count):
    """offsets at which a list of ``count`` rows is laid over a batch of n so that every row is met"""
    return range(0, count, n) if n < count else (0,)


def drawn_table(shape, seed_offset=0):
    from srgan_amd.augment import GeometricAugment
    n, h, w = shape
    return GeometricAugment(seed=2000 + seed_offset + n + 7 * h + 13 * w).draw(n, h, w)


def extreme_tables(shape):
    n = shape[0]
    rows = EXTREME_ROWS
    return [(f"extremes +{off}", build_table([rows[(off + i) % len(rows)] for i in range(n)]))
            for off in _rotations(n, len(rows))]


def gated_tables(shape):
    """drawn rows whose slot 7 runs through every mask value 0..15"""
    n = shape[0]
    out = []
    for off in _rotations(n, 16):
        t = drawn_table(shape, 1)
        t[:, 7] = torch.tensor([float((off + i) % 16) for i in range(n)])
        out.append((f"masks +{off}", t))
    return out


def pure_tables(shape):
    """[(fx, k, table)]: every sample the same pure flip / rot90 row (zoom 1, cos 1, sin 0); odd k on square images only"""
    n, h, w = shape
    return [(fx, k, build_table([(fx, k, 1.0, 0.0)] * n)) for fx in (0, 1) for k in range(4) if h == w or k % 2 == 0]


# ---- cases -----------------------------------------------------------------------------------------------------------------------
# (N, H, W), why.  The switch-over points of the implementation, one shape on either side: four consecutive pixels go out as three
# 16-byte stores when H W is a multiple of 4 (scalar stores otherwise), an item covers ITEM_PIXELS pixels (one or two items per
# sample), a launch holds GRID_CAP workgroups and strides beyond.
SHAPES = [
    ((1, 1, 1), "one pixel: every neighbour but one is outside"),
    ((1, 2, 2), "smallest non-trivial image"),
    ((3, 5, 7), "odd, non-square, 35 pixels: scalar path, rows off 16-byte alignment"),
    ((2, 8, 8), "square, even: 16-byte path"),
    ((5, 16, 12), "non-square, aligned rows"),
    ((2, 7, 7), "square, odd: the centre is a pixel; scalar path"),
    ((2, 6, 10), "non-square, H W a multiple of 4: 16-byte path"),
    ((2, 32, 64), "2048 pixels: one item"),
    ((2, 36, 57), "2052 pixels: two items (16-byte path)"),
    ((2, 3, 683), "2049 pixels: two items (scalar path)"),
    ((4, 128, 128), "the workload's rows: 8 items per sample"),
    ((2048, 2, 2), "2048 work items: the grid cap exactly"),
    ((2049, 2, 2), "2049 work items at a tiny image: one workgroup strides"),
]
CASES = [s for s, _ in SHAPES]


def items(shape):
    n, h, w = shape
    return n * -(-(h * w) // ITEM_PIXELS)


# ---- the stand-alone host program ----------------------------------------------------------------------------------------------------
_SAN = ["-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all"]


def build_host_program(tmp_dir, sanitize=True):
    """Build tests/geom_host_sweep.cpp with the host compiler from csrc/geom_math.h alone (its own main).  ``sanitize``: with the host
    sanitizers where the compiler has their runtimes, plainly otherwise.  -> (path, was it built with the sanitizers?)"""
    here = os.path.dirname(os.path.abspath(__file__))
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    inc = os.path.join(os.path.dirname(here), "style-restricted_gan_amd", "csrc")
    exe = os.path.join(str(tmp_dir), "geom_host_sweep" + ("_san" if sanitize else ""))
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I" + inc, os.path.join(here, "geom_host_sweep.cpp"), "-o", exe]
    if sanitize:
        built = subprocess.run(base + _SAN, capture_output=True, text=True)
        if built.returncode == 0:
            return exe, True
        return build_host_program(tmp_dir, sanitize=False)                # (no sanitizer runtime for this compiler)
    built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    return exe, False


def run_host_sweep(tmp_dir, sanitize=True):
    """Build the host program and run its sweep as a child process, in the environment this process has: hostile table rows over
    images from 1 x 1 to 256 x 256.  A sanitized build that the environment does not let start (the sanitizer's runtime has to be
    the first library loaded) gives way to the plain build.  Which build ran is printed and returned: -> (the number of checks the
    sweep made, was it the sanitized build?); raises AssertionError when the sweep fails."""
    exe, sanitized = build_host_program(tmp_dir, sanitize)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    if sanitized and r.returncode != 0 and not r.stdout and "runtime does not come first" in r.stderr:
        exe, sanitized = build_host_program(tmp_dir, sanitize=False)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-2000:])
    checks = int(r.stdout.split()[1])
    print(f"geom host sweep | {'address, undefined, float-cast-overflow sanitizers' if sanitized else 'NO sanitizer (plain build)'} | "
          f"{checks} checks")
    return checks, sanitized


def probe(exe, h, w, flags, row):
    """What csrc/geom_math.h makes of one table row on an h x w image (the host program's ``probe`` mode): {"radius": int,
    "outside" / "inside": the largest weight an output pixel outside / inside an input pixel's window gives that input pixel,
    "src": float32 [h, w, 2] the source position of every output pixel, "i0": int [h, w, 2], "f": float32 [h, w, 2]}"""
    args = [str(h), str(w), str(int(flags))] + [repr(float(v)) for v in row[:5].tolist()]
    r = subprocess.run([exe, "probe"] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    out = {"src": torch.zeros(h, w, 2), "i0": torch.zeros(h, w, 2, dtype=torch.int64), "f": torch.zeros(h, w, 2)}
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] == "radius":
            out["radius"] = int(t[1])
        elif t[0] in ("outside", "inside"):
            out[t[0]] = float(t[1])
        elif t[0] == "src":
            qi, qj = int(t[1]), int(t[2])
            out["src"][qi, qj] = torch.tensor([float(t[3]), float(t[4])])
            out["i0"][qi, qj] = torch.tensor([int(t[5]), int(t[6])])
            out["f"][qi, qj] = torch.tensor([float(t[7]), float(t[8])])
    return out
