"""Yardstick of the DiffAugment tests (csrc/augment.hip, srgan_amd.augment): a step-by-step restatement of the operation in torch,
written from the specification (colour, then translation, then cutout; one row [b, s, a, ty, tx, cy, cx, 0] per sample), the
closed-form gradient, the case list and a builder of hand-made tables.  No GPU code: tests/test_augment_refs_cpu.py pins what is in
here, tests/test_augment_kernels_gpu.py and tests/test_augment_train_gpu.py hold the HIP kernels and the train step to it.

Restatement: brightness x1 = x + b; saturation x2 = (x1 - m) s + m with m the channel mean of the pixel; contrast x3 = (x2 - M) a + M
with M the mean of x2 over the sample, computed from x2 itself; translation by zero padding and an index gather,
x4[i, j] = x3[i + ty, j + tx]; cutout by a mask over rows [cy - ch // 2, cy - ch // 2 + ch) x the columns defined likewise.
Gradients are autograd of that, in float64 for the reference.

Error measure: ``small_common.rel_err`` (max |a - ref| relative to max |ref|), PER SAMPLE -- the gradient magnitudes of the
samples of one batch span six decades and every sum of the operation stays inside one sample.  Bound: ``max(8 * e32, gamma(L))`` of
tests/small_common.py, L the longest sequential float32 sum one thread of the reduction performs: a thread of the partial-sum
kernel adds the up to 16 elements it owns of a 4096-float chunk, a thread of the second level adds ceil(chunks / 256) partials.
"""
import os

import torch
import torch.nn.functional as F

from tests.small_common import ceil_div, gamma, rel_err

COLOR, TRANSLATION, CUTOUT = 1, 2, 4
ALL = COLOR | TRANSLATION | CUTOUT
ROW = 8
# what csrc/augment.hip cuts its work by: floats per partial sum, pixels per item of the gather pass, workgroups per launch
CHUNK, ITEM_PIXELS, GRID_CAP = 4096, 2048, 2048


def window(size, ratio):
    return int(size * ratio + 0.5)


def chunks(h, w):
    return ceil_div(3 * h * w, CHUNK)


def seq_len(h, w):
    """L of the bound for an h x w image"""
    e = 3 * h * w
    return max(min(16, 4 * ceil_div(min(e, CHUNK), 1024)), ceil_div(chunks(h, w), 256))


def workspace_bytes(n, h, w):
    return 4 * n * chunks(h, w)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def _ints(table, col):
    return table[:, col].detach().cpu().to(torch.int64)


def _shift(x, ty, tx):
    """out[n, :, i, j] = x[n, :, i + ty[n], j + tx[n]] where that pixel exists, else 0: zero padding, then an index gather"""
    n, _, h, w = x.shape
    py, px = int(ty.abs().max()), int(tx.abs().max())
    xp = F.pad(x, (px, px, py, py))
    rows = torch.arange(h).view(1, h) + ty.view(n, 1) + py           # in [0, h + 2 py)
    cols = torch.arange(w).view(1, w) + tx.view(n, 1) + px
    out = xp[torch.arange(n).view(n, 1, 1), :, rows.view(n, h, 1), cols.view(n, 1, w)]          # [n, h, w, c]
    return out.permute(0, 3, 1, 2)


def _keep_mask(table, n, h, w, cut, dtype):
    """1 outside the cutout window, 0 inside: [n, 1, h, w]"""
    ch, cw = cut
    r0 = _ints(table, 5) - ch // 2
    c0 = _ints(table, 6) - cw // 2
    ii, jj = torch.arange(h).view(1, h), torch.arange(w).view(1, w)
    rows = (ii >= r0.view(n, 1)) & (ii < (r0 + ch).view(n, 1))
    cols = (jj >= c0.view(n, 1)) & (jj < (c0 + cw).view(n, 1))
    return (~(rows.view(n, 1, h, 1) & cols.view(n, 1, 1, w))).to(dtype)


def restate(x, table, flags, cut, dtype=torch.float64):
    """y = T(x) step by step in ``dtype`` on the CPU (differentiable in x when x is a ``dtype`` leaf)."""
    x = x.cpu().to(dtype)
    table = table.detach().cpu()
    n, c, h, w = x.shape
    assert c == 3 and tuple(table.shape) == (n, ROW)
    if flags & COLOR:
        b, s, a = (table[:, i].to(dtype).view(n, 1, 1, 1) for i in range(3))
        x = x + b
        m = x.mean(dim=1, keepdim=True)
        x = (x - m) * s + m
        M = x.mean(dim=(1, 2, 3), keepdim=True)
        x = (x - M) * a + M
    if flags & TRANSLATION:
        x = _shift(x, _ints(table, 3), _ints(table, 4))
    if flags & CUTOUT:
        x = x * _keep_mask(table, n, h, w, cut, dtype)
    return x


def restate_with_grad(x, gy, table, flags, cut, dtype):
    """(y, gx) of the restatement in ``dtype``: gx by autograd"""
    leaf = x.detach().cpu().to(dtype).requires_grad_(True)
    y = restate(leaf, table, flags, cut, dtype)
    (gx,) = torch.autograd.grad(y, leaf, gy.detach().cpu().to(dtype))
    return y.detach(), gx.detach()


def closed_form_grad(gy, table, flags, cut, dtype=torch.float64):
    """gx[p, c] = a s g'[p, c] + a (1 - s) / 3 * sum_c g'[p, c] + (1 - a) / (3 H W) * sum_all g', g' = gy zeroed inside the cutout
    window and moved back by the translation (a pixel no output reads gets 0)."""
    g = gy.detach().cpu().to(dtype)
    table = table.detach().cpu()
    n, _, h, w = g.shape
    if flags & CUTOUT:
        g = g * _keep_mask(table, n, h, w, cut, dtype)
    if flags & TRANSLATION:
        g = _shift(g, -_ints(table, 3), -_ints(table, 4))
    if flags & COLOR:
        s, a = (table[:, i].to(dtype).view(n, 1, 1, 1) for i in (1, 2))
        g = a * s * g + a * (1 - s) / 3 * g.sum(dim=1, keepdim=True) + (1 - a) / (3 * h * w) * g.sum(dim=(1, 2, 3), keepdim=True)
    return g


def sample_errs(a, ref):
    """``small_common.rel_err`` of every sample at once: float64 [n]"""
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    err = (a - ref).abs().flatten(1).max(dim=1).values / ref.abs().flatten(1).max(dim=1).values.clamp_min(1e-30)
    return torch.where(torch.isfinite(a).flatten(1).all(dim=1), err, torch.full_like(err, float("inf")))


def check(what, got, ref64, ref32, L):
    """Hold every sample of ``got`` to the float64 reference; with SRGAN_TEST_LOG set, print the worst figures first."""
    g = gamma(L)
    e32s, errs = sample_errs(ref32, ref64), sample_errs(got, ref64)
    ratio = errs / torch.maximum(8 * e32s, torch.full_like(e32s, g))
    i = int(ratio.argmax())
    worst = (float(ratio[i]), float(errs[i]), float(e32s[i]), i)
    if os.environ.get("SRGAN_TEST_LOG"):
        print(f"augment | {what} | sample {worst[3]} e32 {worst[2]:.3e} gamma {g:.3e} err {worst[1]:.3e} err/bound {worst[0]:.3f}")
    assert worst[0] <= 1.0, (f"{what} sample {worst[3]}: error {worst[1]:.3e} > max(8 * e32 = {8 * worst[2]:.3e}, "
                             f"gamma({L}) = {g:.3e})")


# ---- cases -----------------------------------------------------------------------------------------------------------------------
# (N, H, W), why.  The switch-over points of the implementation, one shape on either side: a partial sum covers CHUNK floats (one
# or two chunks per sample), an item of the gather pass ITEM_PIXELS pixels (one or two items), the second level adds the partials
# thread-strided beyond 256 of them, a launch holds GRID_CAP workgroups and strides beyond.
SHAPES = [
    ((1, 1, 1), "cutout covers the image, shift range 0"),
    ((1, 2, 2), "smallest non-trivial image"),
    ((3, 5, 7), "odd, non-square, 21 floats per row: ragged tail, rows off 16-byte alignment"),
    ((2, 8, 8), "even cutout, centre range H + 1"),
    ((5, 16, 12), "non-square, aligned rows"),
    ((4, 128, 128), "the workload's rows: 12 chunks, 8 items per sample"),
    ((2, 256, 256), "the 256 x 256 workload: 48 chunks, 32 items per sample"),
    ((66, 32, 32), "more samples than the step ever passes"),
    ((5, 44, 31), "4092 floats: one chunk (16-byte path)"),
    ((5, 36, 38), "4104 floats: two chunks (16-byte path)"),
    ((2, 35, 39), "4095 floats: one chunk (scalar path)"),
    ((2, 2, 683), "4098 floats: two chunks (scalar path)"),
    ((2, 32, 64), "2048 pixels: one item"),
    ((2, 36, 57), "2052 pixels: two items (16-byte path)"),
    ((2, 3, 683), "2049 pixels: two items (scalar path)"),
    ((1, 591, 591), "256 chunks: one partial per thread at the second level"),
    ((1, 592, 592), "257 chunks: thread 0 adds two partials at the second level"),
    ((2048, 4, 4), "2048 work items: the grid cap exactly"),
    ((2049, 4, 4), "2049 work items: one workgroup strides"),
]
CASES = [s for s, _ in SHAPES]


def is_small(shape):
    return shape[1] * shape[2] <= 4096


def extreme_rows(h, w, ratio_t, ratio_c):
    """hand-made (r_b, r_s, r_c, ty, tx, cy, cx): both ends of every range"""
    sy, sx = window(h, ratio_t), window(w, ratio_t)
    ch, cw = window(h, ratio_c), window(w, ratio_c)
    cy_top, cx_top = h + (1 - ch % 2) - 1, w + (1 - cw % 2) - 1
    top = 1.0 - 2.0 ** -24          # the largest float32 below 1
    return [
        (0.0, 0.5, 0.5, sy, sx, 0, 0),
        (top, 0.0, 0.25, -sy, -sx, cy_top, cx_top),             # r_s = 0: grey
        (0.5, 0.75, 0.0, 0, 0, h // 2, w // 2),                 # r_c = 0; no shift, central window
        (0.25, top, top, sy, -sx, cy_top, 0),
        (0.75, 0.3, 0.6, -sy, 0, 0, cx_top),
    ]


def build_table(rows):
    """(r_b, r_s, r_c, ty, tx, cy, cx) per sample -> float32 [n, 8] as DiffAugment.draw lays it out"""
    t = torch.zeros(len(rows), ROW, dtype=torch.float32)
    for i, (rb, rs, rc, ty, tx, cy, cx) in enumerate(rows):
        rb, rs, rc = (torch.tensor(v, dtype=torch.float32) for v in (rb, rs, rc))
        t[i, 0], t[i, 1], t[i, 2] = rb - 0.5, rs * 2.0, rc + 0.5
        t[i, 3], t[i, 4], t[i, 5], t[i, 6] = float(ty), float(tx), float(cy), float(cx)
    return t


def tables(shape):
    """[(name, table [n, 8], (ch, cw))] of a shape: the extremes at the default ratios (rotated so that a batch smaller than the
    list still meets every row, on the small shapes), at ratio 1.0 for both (a shift of a whole image, a window of a whole image),
    and random rows from DiffAugment.draw."""
    from srgan_amd.augment import DiffAugment
    n, h, w = shape
    out = []
    for ratio_t, ratio_c in ((0.125, 0.5), (1.0, 1.0)):
        rows = extreme_rows(h, w, ratio_t, ratio_c)
        offsets = range(0, len(rows), n) if n < len(rows) and is_small(shape) else (0,)
        for off in offsets:
            out.append((f"extremes t{ratio_t} c{ratio_c} +{off}", build_table([rows[(off + i) % len(rows)] for i in range(n)]),
                        (window(h, ratio_c), window(w, ratio_c))))
    aug = DiffAugment(seed=1000 + n + 7 * h + 13 * w)
    out.append(("drawn", aug.draw(n, h, w), aug.cut(h, w)))
    return out


def inputs(shape, seed=0):
    """x ~ U(-1, 1); gy standard normal times a per-sample magnitude from 1e-3 to 1e3"""
    n, h, w = shape
    g = torch.Generator().manual_seed(9000 + seed + n + 3 * h + 5 * w)
    x = torch.rand(n, 3, h, w, generator=g) * 2 - 1
    mag = 10.0 ** torch.linspace(-3, 3, n) if n > 1 else torch.ones(1)
    gy = torch.randn(n, 3, h, w, generator=g) * mag.view(n, 1, 1, 1)
    return x, gy
