"""CPU: what the geometric-augmentation tests measure against (tests/geom_common.py) and the host side of the feature -- the
restatement against ``F.grid_sample``, the gather-form adjoint against autograd, the exact permutations, the draws of
srgan_amd.augment.GeometricAugment, its independence from DiffAugment, the trainer's switches and checkpoint section, the C ABI's
argument checks and launch descriptors (the library loads without a GPU), and a stand-alone host program that sweeps hostile table
rows through the arithmetic the kernels share (csrc/geom_math.h)."""
import ctypes
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import geom_common as gc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_SHAPES = [(3, 8, 8), (2, 5, 7), (4, 16, 16), (2, 16, 12), (2, 32, 32), (1, 1, 1), (1, 2, 2)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from srgan_amd import _lib
    return _lib.load()


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def _tables(shape):
    return [("drawn", gc.drawn_table(shape))] + gc.extreme_tables(shape)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", REF_SHAPES, ids=str)
def test_restatement_equals_grid_sample_in_float64(shape):
    x, _ = gc.inputs(shape)
    for name, table in _tables(shape):
        for flags in range(16):
            assert _rel(gc.restate(x, table, flags), gc.grid_sample_form(x, table, flags)) <= 1e-13, (shape, name, flags)


@pytest.mark.parametrize("shape", REF_SHAPES, ids=str)
def test_gather_adjoint_equals_autograd_and_the_inner_products_agree(shape):
    x, gy = gc.inputs(shape)
    for name, table in _tables(shape) + gc.gated_tables(shape):
        gated = name.startswith("masks")
        for flags in ((15,) if gated else range(16)):
            y, gx = gc.restate_with_grad(x, gy, table, flags, torch.float64, gated)
            ga = gc.adjoint_gather(gy, table, flags, torch.float64, gated)
            assert float(gc.sample_errs(ga, gx).max()) <= 1e-13, (shape, name, flags)
            lhs, rhs = float((y * gy.double()).sum()), float((x.double() * ga).sum())             # <A x, y> = <x, A^T y>
            assert abs(lhs - rhs) <= 1e-12 * float((y.abs() * gy.double().abs()).sum()) + 1e-300, (shape, name, flags)


@pytest.mark.parametrize("shape", REF_SHAPES, ids=str)
def test_float32_restatement_stays_close_to_float64(shape):
    """coordinate rounding: a few float32 ulps of a coordinate of size H, times the image's slope"""
    x, gy = gc.inputs(shape)
    for name, table in _tables(shape):
        y64, g64 = gc.restate_with_grad(x, gy, table, 15, torch.float64)
        y32 = gc.restate(x, table, 15, torch.float32)
        g32 = gc.adjoint_gather(gy, table, 15, torch.float32)
        bound = 64 * max(shape[1], shape[2]) * 2.0 ** -24
        assert float(gc.sample_errs(y32, y64).max()) <= bound and float(gc.sample_errs(g32, g64).max()) <= bound, (shape, name)


def test_masked_rows_are_the_ungated_rows_with_the_groups_removed():
    shape = (16, 8, 8)
    x, gy = gc.inputs(shape)
    (_, table), = gc.gated_tables(shape)
    y = gc.restate(x, table, 15, torch.float32, gated=True)
    g = gc.adjoint_gather(gy, table, 15, torch.float32, gated=True)
    for m in range(16):
        assert torch.equal(y[m], gc.restate(x, table, 15 & ~m, torch.float32)[m])
        assert torch.equal(g[m], gc.adjoint_gather(gy, table, 15 & ~m, torch.float32)[m])
    assert torch.equal(y[15], x[15]) and torch.equal(g[15], gy[15])


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/geom_host_sweep.cpp built plainly from csrc/geom_math.h: its ``probe`` mode prints what the shipped header computes"""
    exe, _ = gc.build_host_program(tmp_path_factory.mktemp("geom_host"), sanitize=False)
    return exe


@pytest.mark.parametrize("shape", [(4, 8, 8), (4, 7, 7), (3, 6, 10)], ids=str)
def test_pure_flip_and_rot90_rows_are_exact_permutations_in_float32(shape, host_program):
    """the float32 restatement, and the header the kernels compile: integer source positions, weights exactly 1 and 0, and the pixel
    read is the one ``flip(rot90(x, -k))`` puts there"""
    x, gy = gc.inputs(shape)
    n, h, w = shape
    index = torch.arange(h * w, dtype=torch.float32).view(1, 1, h, w).expand(1, 3, h, w)
    seen = 0
    for fx, k, table in gc.pure_tables(shape):
        want = gc.permutation(x, fx, k)
        for flags in (gc.FLIP | gc.ROT90, gc.ALL):
            assert torch.equal(gc.restate(x, table, flags, torch.float32), want), (shape, fx, k, flags)
            pr = gc.probe(host_program, h, w, flags, table[0])
            assert pr["radius"] == 1 and pr["outside"] == 0.0 and pr["inside"] == 1.0
            assert float(pr["f"].abs().max()) == 0.0 and torch.equal(pr["src"], pr["i0"].float())      # weights 1, 0, 0, 0
            read = pr["i0"][..., 0] * w + pr["i0"][..., 1]
            assert torch.equal(read, gc.permutation(index, fx, k)[0, 0].long()), (shape, fx, k, flags)
        # the adjoint of a permutation is its inverse
        gx = gc.adjoint_gather(gy, table, gc.ALL, torch.float32)
        assert torch.equal(gc.permutation(gx, fx, k), gy), (shape, fx, k)
        seen += 1
    assert seen == (8 if shape[1] == shape[2] else 4)


def test_radius_covers_the_support(host_program):
    """No output pixel outside an input pixel's window reads it.  From the shipped header (the host program's ``probe``, float32, the
    functions the backward kernel calls): the radius of every extreme and drawn row is the restatement's, the largest weight outside
    the window is exactly 0 and the source positions are the restatement's bit for bit.  And in float64 from the restatement's maps,
    for the same rows."""
    shape = (11, 16, 12)
    n, h, w = shape
    (_, table), = gc.extreme_tables(shape)
    r = gc.radius(table, 15)
    assert int(r.max()) == 3 and int(r.min()) == 1 and r.tolist()[:2] == [1, 2]
    for tab in (table, gc.drawn_table(shape)):
        rad = gc.radius(tab, 15)
        M32, _ = gc.maps(tab, 15, torch.float32)
        qi, qj = torch.arange(h, dtype=torch.float32).view(1, h, 1), torch.arange(w, dtype=torch.float32).view(1, 1, w)
        si, sj = gc._source(M32, h, w, qi, qj, torch.float32)
        for b in range(n):
            pr = gc.probe(host_program, h, w, 15, tab[b])
            assert pr["radius"] == int(rad[b]), (b, pr["radius"], int(rad[b]))
            assert pr["outside"] == 0.0 and pr["inside"] > 0.2, (b, pr["outside"], pr["inside"])
            inside = (si[b] > -2) & (si[b] < h + 1) & (sj[b] > -2) & (sj[b] < w + 1)                  # (the header clamps beyond)
            assert torch.equal(pr["src"][..., 0][inside], si[b][inside]) and torch.equal(pr["src"][..., 1][inside], sj[b][inside]), b
    M, T = gc.maps(table, 15, torch.float64)
    cen = torch.tensor([(h - 1) / 2, (w - 1) / 2], dtype=torch.float64)
    pix = torch.stack(torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij"), -1).reshape(-1, 2).double()      # [P, 2]
    for b in range(n):
        centre = torch.floor((pix - cen) @ T[b].T + cen + 0.5)                        # [P(p), 2]
        src = (pix - cen) @ M[b].T + cen                                             # [P(q), 2]
        hat = (1 - (src[None, :, :] - pix[:, None, :]).abs()).clamp_min(0)           # [p, q, 2]
        weight = hat[..., 0] * hat[..., 1]
        outside = ((pix[None, :, :] - centre[:, None, :]).abs() > int(r[b])).any(-1)  # q outside p's window
        assert float((weight * outside).max()) <= 1e-9, b
        assert float(weight.max()) > 0.2


# ---- draws ---------------------------------------------------------------------------------------------------------------------------
def test_draws():
    from srgan_amd import ops
    from srgan_amd.augment import GeometricAugment
    assert (ops.GEOM_FLIP, ops.GEOM_ROT90, ops.GEOM_SCALE, ops.GEOM_ROTATE, ops.GEOM_ROW) == (1, 2, 4, 8, 8)
    a, b = GeometricAugment(seed=11), GeometricAugment(seed=11)
    state = torch.get_rng_state()
    t = a.draw(20000, 16, 16)
    assert torch.equal(torch.get_rng_state(), state)                 # the default generator is not touched
    assert torch.equal(t, b.draw(20000, 16, 16)) and not torch.equal(t, GeometricAugment(seed=12).draw(20000, 16, 16))
    assert t.dtype == torch.float32 and tuple(t.shape) == (20000, 8) and not t.is_cuda
    assert set(t[:, 0].tolist()) == {0.0, 1.0} and set(t[:, 1].tolist()) == {0.0, 1.0, 2.0, 3.0}
    assert float(t[:, 2].min()) >= 0.5 and float(t[:, 2].max()) <= 2.0 and float(t[:, 2].std()) > 0.05
    assert float((t[:, 3] ** 2 + t[:, 4] ** 2 - 1).abs().max()) <= 4 * 2.0 ** -24
    assert float(t[:, 3].min()) < -0.99 and float(t[:, 4].min()) < -0.99 and float(t[:, 4].max()) > 0.99
    assert float(t[:, 5:].abs().max()) == 0.0
    wide = GeometricAugment(scale_std=5.0, seed=3).draw(2000, 8, 8)[:, 2]                       # the clamp is met at both ends
    assert float(wide.min()) == 0.5 and float(wide.max()) == 2.0
    assert set(GeometricAugment(seed=5).draw(4000, 16, 12)[:, 1].tolist()) == {0.0, 2.0}       # non-square: never an odd k
    small = GeometricAugment(rotate_max=0.25, seed=5).draw(4000, 8, 8)
    assert float(small[:, 3].min()) >= math.cos(math.pi / 4) - 1e-6
    u = a.draw_gate(1000)
    assert tuple(u.shape) == (1000, 4) and u.dtype == torch.float32 and float(u.min()) >= 0 and float(u.max()) < 1
    assert not torch.equal(GeometricAugment().draw(4, 8, 8), GeometricAugment().draw(4, 8, 8))  # unseeded: fresh entropy each
    assert a.draw_fn == a.draw and a.gate_fn == a.draw_gate


def test_groups_that_are_off_yield_identity_rows_and_consume_nothing():
    from srgan_amd.augment import GeometricAugment
    ident = torch.tensor([0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0]).repeat(6, 1)
    none = GeometricAugment("", seed=1)
    before = none.generator.get_state()
    assert torch.equal(none.draw(6, 16, 16), ident) and torch.equal(none.generator.get_state(), before) and none.flags == 0
    t = GeometricAugment("scale", seed=1).draw(6, 16, 16)
    assert torch.equal(t[:, :2], ident[:, :2]) and torch.equal(t[:, 3:], ident[:, 3:]) and not torch.equal(t[:, 2], ident[:, 2])
    # a group that is off consumes nothing: "rotate" alone draws what the rotate group of "scale,rotate" draws after scale's randn
    g = torch.Generator().manual_seed(4)
    want = (2.0 * torch.rand(6, generator=g).double() - 1.0) * math.pi
    t = GeometricAugment("rotate", seed=4).draw(6, 16, 16)
    assert torch.equal(t[:, 3], torch.cos(want).float()) and torch.equal(t[:, 4], torch.sin(want).float())
    assert torch.equal(t[:, :3], ident[:, :3])
    # identity rows are the identity of the restatement, whatever the flags say
    x, _ = gc.inputs((6, 16, 16))
    assert torch.equal(gc.restate(x, ident, gc.ALL, torch.float32), x)


def test_state_dict_round_trip_and_argument_errors():
    from srgan_amd.augment import GeometricAugment
    a = GeometricAugment("flip,rotate", scale_std=0.3, rotate_max=0.5, seed=11)
    a.draw(7, 16, 16)
    sd = a.state_dict()
    nxt = a.draw(5, 32, 32)
    c = GeometricAugment("scale", seed=99)
    c.load_state_dict({k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()})
    assert (c.policy, c.scale_std, c.rotate_max) == ("flip,rotate", 0.3, 0.5) and c.flags == 9
    assert torch.equal(c.draw(5, 32, 32), nxt)
    assert GeometricAugment().flags == 15 and GeometricAugment().policy == "flip,rot90,scale,rotate"
    assert (GeometricAugment().scale_std, GeometricAugment().rotate_max) == (0.2, 1.0)
    assert GeometricAugment("rot90, flip").flags == 3
    for bad in ("flipp", "flip,color", "flip,,scale", None, 3):
        with pytest.raises(ValueError):
            GeometricAugment(bad)
    with pytest.raises(ValueError, match="color"):
        GeometricAugment("flip,color")
    g = GeometricAugment("flip")
    g.policy = "shear"                                             # edited in place: refused where it is read
    with pytest.raises(ValueError, match="shear"):
        g.flags
    for kw in (dict(scale_std=-0.1), dict(rotate_max=-0.1), dict(rotate_max=1.5), dict(scale_std=float("nan")), dict(rotate_max="x")):
        with pytest.raises(ValueError):
            GeometricAugment(**kw)
    f1, f2 = GeometricAugment("flip", seed=1), GeometricAugment("flip", seed=1)
    assert f1.fingerprint() != f2.fingerprint() and f1.fingerprint() == f1.fingerprint() and f1.graph_keepalive() == []
    fp = f1.fingerprint()
    f1.policy = "flip,scale"
    assert f1.fingerprint() != fp


# ---- the trainer's host side ---------------------------------------------------------------------------------------------------------
def _cpu_trainers(k=3, torch_opts=False):
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
    opts = [torch.optim.Adam(net.parameters(), lr=1e-4) for net in (G, D, E)] if torch_opts else [None] * 3
    sg = SRGAN_training([G, D, E], opts, crit, lbd, k, "cpu", np.eye(4), 4, "mu", 8)
    return single, sg


def test_trainers_host_side():
    from srgan_amd.augment import GeometricAugment
    single, sg = _cpu_trainers()
    with pytest.raises(NotImplementedError, match="SingleGAN_training.*SRGAN_training.enable_geometric_augment"):
        single.enable_geometric_augment()
    assert sg.geometry is None and sg._stage_draws(sg.geometry) == 0 and not sg._stage_on(sg.geometry)
    assert sg.enable_geometric_augment(policy="flip,scale", scale_std=0.1, rotate_max=0.5, seed=3) is sg
    assert isinstance(sg.geometry, GeometricAugment) and sg.geometry in sg._extensions()
    assert (sg.geometry.flags, sg.geometry.scale_std, sg.geometry.rotate_max) == (5, 0.1, 0.5) and sg._stage_draws(sg.geometry) == 7      # 2k + 1
    assert sg.augment is None and sg._stage_draws(sg.augment) == 0                      # DiffAugment is a switch of its own
    with pytest.raises(ValueError):
        sg.enable_geometric_augment(policy="turn")
    sg.enable_geometric_augment(policy="")
    assert sg.geometry is not None and sg._stage_draws(sg.geometry) == 0 and not sg._stage_on(sg.geometry)                                          # identity
    img = torch.zeros(4, 3, 8, 8)
    assert sg._aug(img) is img and sg._aug(img, 1, [sg.geometry]) is img                  # no draw, no launch
    sg.disable_geometric_augment()
    assert sg.geometry is None and sg._extensions() == []
    # the draw order of a step: the injected source is asked 2k + 1 times for [B, 8]; the eager path uploads what it returns
    sg.enable_geometric_augment(seed=1)
    calls = []

    def fixed(n, h, w):
        calls.append((n, h, w))
        return torch.full((n, 8), float(len(calls)))

    sg.geometry.draw_fn = fixed
    pair = sg._stage_tables(sg.geometry, 2, 4, 16, 12)
    one = sg._stage_tables(sg.geometry, 1, 4, 16, 12)
    assert calls == [(4, 16, 12)] * 3 and tuple(pair.shape) == (8, 8) and tuple(one.shape) == (4, 8)
    assert torch.equal(pair[:4], torch.full((4, 8), 1.0)) and torch.equal(pair[4:], torch.full((4, 8), 2.0))
    # the switches drop a recording
    dropped = []
    sg._graph = type("G", (), {"_drop": lambda self: dropped.append(1)})()
    sg.enable_geometric_augment(seed=2)
    sg.disable_geometric_augment()
    assert len(dropped) == 2
    sg._graph = None


def test_diffaugment_tables_do_not_depend_on_the_geometric_stage():
    def tables(geometry):
        _, sg = _cpu_trainers(k=2)
        sg.enable_diffaugment(seed=7)
        if geometry:
            sg.enable_geometric_augment(seed=7)
        state = torch.get_rng_state()
        aug, geo = [], []
        for count in [2] * sg.k + [1]:                                    # a step's hand-outs, in its order
            aug.append(sg._stage_tables(sg.augment, count, 4, 16, 16))
            if geometry:
                geo.append(sg._stage_tables(sg.geometry, count, 4, 16, 16))
        assert torch.equal(torch.get_rng_state(), state)                  # the style noise's generator is not touched
        return torch.cat(aug), (torch.cat(geo) if geo else None), sg

    a, none, _ = tables(False)
    b, geo, sg = tables(True)
    assert none is None and torch.equal(a, b) and tuple(a.shape) == (5 * 4, 8) and tuple(geo.shape) == (5 * 4, 8)
    from srgan_amd.augment import GeometricAugment
    ref = GeometricAugment(seed=7)
    assert torch.equal(geo, torch.cat([ref.draw(4, 16, 16) for _ in range(5)]))
    assert sg.geometry.generator is not sg.augment.generator


def test_rows_with_the_adaptive_probability_on():
    """the rows a hand-out stages: the table, then four uniforms per sample from the same generator, in slots 8..11"""
    from srgan_amd.augment import GeometricAugment
    _, sg = _cpu_trainers(k=2)
    sg.enable_geometric_augment(seed=9)
    assert tuple(sg._stage_row_draw(sg.geometry, 4, 8, 8).shape) == (4, 8)
    sg.enable_geometric_augment(seed=9)
    sg._ada = object()                                                    # (on: only its presence is read here)
    rows = sg._stage_row_draw(sg.geometry, 4, 8, 8)
    ref = GeometricAugment(seed=9)
    t, u = ref.draw(4, 8, 8), ref.draw_gate(4)
    assert tuple(rows.shape) == (4, 16) and torch.equal(rows[:, :8], t) and torch.equal(rows[:, 8:12], u)
    assert float(rows[:, 12:].abs().max()) == 0.0 and torch.equal(rows, ref.join_rows(t, u))
    with pytest.raises(ValueError):
        ref.join_rows(t, u[:, :3])


def test_checkpoint_section_is_present_only_when_on():
    _, sg = _cpu_trainers(k=2, torch_opts=True)
    assert "geometry" not in sg._ckpt_sections() and "geometry" not in sg.state_dict()
    sg.enable_geometric_augment(policy="flip,rotate", scale_std=0.3, rotate_max=0.5, seed=5)
    sg.geometry.draw(4, 8, 8)
    sd = sg.state_dict()
    assert "geometry" in sg._ckpt_sections() and sd["version"] == 1
    assert {k: v for k, v in sd["geometry"].items() if k != "generator"} == dict(policy="flip,rotate", scale_std=0.3, rotate_max=0.5)
    nxt = sg.geometry.draw(4, 8, 8)
    _, other = _cpu_trainers(k=2, torch_opts=True)
    report = other.load_state_dict(sd)                                    # an extension the file holds is switched on by the load
    assert report.unexpected == [] and report.missing == [] and other.geometry is not None
    assert (other.geometry.policy, other.geometry.scale_std, other.geometry.rotate_max) == ("flip,rotate", 0.3, 0.5)
    assert torch.equal(other.geometry.draw(4, 8, 8), nxt)
    sg.disable_geometric_augment()
    assert "geometry" not in sg.state_dict()


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_back_before_any_launch(lib):
    p = [ctypes.c_void_p(0x10000000 + (i << 20)) for i in range(4)]
    ok = dict(x=p[0], table=p[1], y=p[2], n=2, c=3, h=4, w=4, flags=15, gated=0)
    for fn, name in ((lib.srgan_geom_augment_fwd, b"geom_augment_fwd"), (lib.srgan_geom_augment_bwd, b"geom_augment_bwd")):
        def call(**kw):
            a = dict(ok, **kw)
            return fn(a["x"], a["table"], a["y"], a["n"], a["c"], a["h"], a["w"], a["flags"], a["gated"], None)

        for kw, word in ((dict(c=4), b"three-channel"), (dict(c=1), b"three-channel"), (dict(x=None), b"null pointer"),
                         (dict(table=None), b"null pointer"), (dict(y=None), b"null pointer"), (dict(n=0), b"N ="), (dict(n=-3), b"N ="),
                         (dict(h=0), b"H ="), (dict(w=-1), b"W ="), (dict(h=1 << 15, w=(1 << 14) + 1), b"2^29"),
                         (dict(flags=16), b"flags"), (dict(flags=-1), b"flags"), (dict(y=p[0]), b"alias")):
            assert call(**kw) == -1, (name, kw)
            err = lib.srgan_last_error()
            assert name in err and word in err, (name, kw, err)
    gate = lib.srgan_ada_gate
    for args, word in (((None, p[3], p[1], 4, 4), b"null pointer"), ((p[0], None, p[1], 4, 4), b"null pointer"),
                       ((p[0], p[3], None, 4, 4), b"null pointer"), ((p[0], p[3], p[1], 0, 4), b"n ="), ((p[0], p[3], p[0], 4, 4), b"alias"),
                       ((ctypes.c_void_p(0x10000004), p[3], p[1], 4, 4), b"aligned")):
        assert gate(*args, None) == -1 and b"ada_gate" in lib.srgan_last_error() and word in lib.srgan_last_error(), args


def test_ops_refuse_what_the_kernels_do_not_take():
    from srgan_amd import _lib, ops
    x = torch.zeros(2, 3, 4, 4)
    assert ops.geom_augment(x, None, 0) is x                              # flags == 0: the input itself, nothing is looked at
    with pytest.raises(_lib.SrganHipError, match="no CPU fallback"):
        ops.geom_augment(x, torch.zeros(2, 8), 15)
    with pytest.raises(_lib.SrganHipError, match="no CPU fallback"):
        ops.ada_gate(torch.zeros(2, 16), torch.zeros(56, dtype=torch.uint8), 4)


# ---- launch descriptors (no GPU: tests/hip_shim/launch_shim.c logs them) -------------------------------------------------------------
def test_launch_descriptors_within_aql_limits_and_launch_counts(lib, tmp_path):
    """one launch of min(N * ceil(H W / 2048), 2048) workgroups each way and one gate launch of ceil(N / 256), 256 threads each,
    inside the AQL limits, no scratch, no LDS"""
    from srgan_amd import _lib
    sys.path.insert(0, HERE)
    import isa_tools
    so = str(tmp_path / "launch_shim.so")
    subprocess.run(["gcc", "-shared", "-fPIC", "-O1", "-o", so, os.path.join(HERE, "hip_shim", "launch_shim.c")], check=True)
    desc = {k["name"]: k for k in isa_tools.kernel_descriptors(_lib.LIB_PATH)}
    log = str(tmp_path / "launches.log")
    env = dict(os.environ, LD_PRELOAD=so, SRGAN_SHIM_LOG=log)
    env.pop("SRGAN_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "hip_shim", "drive_geom.py"), _lib.LIB_PATH], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    seen, cur = {}, None
    for line in open(log):
        if line.startswith("#"):
            cur = line[1:].strip()
            seen[cur] = []
            continue
        kname, gx, gy, gz, bx, by, bz, dyn = line.split()
        gx, gy, gz, bx, by, bz, dyn = map(int, (gx, gy, gz, bx, by, bz, dyn))
        short = next((s for s in ("ada_gate_kernel", "geom_fwd_kernel", "geom_bwd_kernel") if s in kname), None)
        assert short is not None, kname
        k = desc[kname]
        ctx = (cur, kname, (gx, gy, gz), (bx, by, bz))
        assert (gy, gz) == (1, 1) and gx >= 1 and (bx, by, bz) == (256, 1, 1) and 256 <= k["max_wg"], ctx
        assert gx * bx < 2 ** 32, ctx
        assert k["lds"] == 0 and k["scratch"] == 0 and dyn == 0, ctx
        seen[cur].append((short, gx))
    sys.path.insert(0, os.path.join(HERE, "hip_shim"))
    import drive_geom
    assert len(seen) == len(drive_geom.SHAPES) and set(gc.CASES) <= set(drive_geom.SHAPES)
    for n, h, w in drive_geom.SHAPES:
        grid = min(gc.items((n, h, w)), gc.GRID_CAP)
        want = [("geom_fwd_kernel", grid), ("geom_bwd_kernel", grid)] * 2 + [("ada_gate_kernel", -(-n // 256))]
        assert seen[f"{n} {h} {w}"] == want, (n, h, w)
    assert seen["4 128 128"][0][1] == 32 and seen["2049 2 2"][0][1] == 2048 and seen["64 256 256"][0][1] == 2048
    names = [k for k in desc if "geom_fwd_kernel" in k or "geom_bwd_kernel" in k]
    assert len(names) == 4                                                # forward / backward x ungated / gated


# ---- the stand-alone host sweep ------------------------------------------------------------------------------------------------------
def test_hostile_rows_never_leave_the_image_host_sweep(tmp_path):
    """tests/geom_host_sweep.cpp, compiled by the host compiler from csrc/geom_math.h alone and run as a child process: NaN, +-inf,
    +-1e30, zoom 1e-6 / 1e6, |cos|, |sin| up to 1e6, k = -1 / 7.5, over images from 1 x 1 to 256 x 256.  Built with the host
    sanitizers where the compiler has their runtimes (the program has its own main; nothing is preloaded), plainly otherwise."""
    checks, sanitized = gc.run_host_sweep(tmp_path)
    assert checks > 10 ** 6
    if not sanitized:
        warnings.warn("geom host sweep: the host compiler has no sanitizer runtime (or the environment preloads a library in front of "
                      "it); the sweep ran as a plain build -- its range checks hold, the conversions themselves were not instrumented")
