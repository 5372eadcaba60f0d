"""GPU: the instance-norm and CBIN kernels (csrc/norm.hip) against float64 on every dispatch path -- slab kernels of every
register depth, the three two-pass statistics kernels with every finish, both 8192-block caps, the fp32 / bf16 pairings -- and
on inputs that are not well-conditioned Gaussians.  References, cases, the restated dispatch and the error measure live in
tests/norm_common.py (pinned without a GPU by tests/test_norm_refs_cpu.py).  Every comparison is bounded by
max(8 * e32, gamma(L)), plus half a bf16 ulp of max |ref| for a tensor stored as bf16; the skip tensor's gradient is compared
exactly.  Where the float64 pre-activation lies within rounding of an activation's kink the upstream gradient is zero
(norm_common.kink_mask).
SRGAN_TEST_LOG=1 prints e32, gamma, err and err / bound of every comparison."""
import pytest
import torch

from tests import norm_common as nc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from srgan_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


def _ids(cases):
    return [c["name"] for c in cases]


def _norm_hip(ops, act):
    return lambda x, scale, shift, res: ops.instance_norm_act(x, scale, shift, res, act, nc.SLOPE, nc.EPS)


def _hold_fp32(ops, what, shape, x, affine, with_res, act, backward=True):
    """One call of ops.instance_norm_act (and its backward) against the yardstick."""
    scale, shift, res = nc.case_params(shape, affine, with_res)
    inputs = (x, scale, shift, res)
    what = f"{what} affine={int(affine)} res={int(with_res)} act={act}"
    if not backward:
        needs = (False,) * 4
        (r64, r32), gout = nc.yardstick(nc.norm_ref(act), inputs, needs), None
    else:
        needs = (True, affine, affine, with_res)
        (r64, r32), gout = nc.norm_yardstick(x, scale, shift, res, act, nc.path_L(shape), nc.upstream(shape))
    got = nc.run(_norm_hip(ops, act), inputs, needs, gout, torch.float32, "cuda")
    names = ["y"] + [n for n, need in zip(("dx", "dscale", "dshift", "dres"), needs) if need]
    assert len(got) == len(r64) == len(names)
    for name, g, a, b in zip(names, got, r64, r32):
        if name == "dres":                       # passed through
            assert torch.equal(g.cpu(), gout), f"{what} dres"
        else:
            nc.check("instance_norm_act", f"{what} {name}", g, a, b, nc.path_L(shape, backward=name != "y"))


FULL_CASES = [c for c in nc.FP32_CASES if c["grid"] in ("full", "fold")]
CAP_CASES = [c for c in nc.FP32_CASES if c["grid"] == "cap"]
CAPACT_CASES = [c for c in nc.FP32_CASES if c["grid"] == "capact"]


@pytest.mark.parametrize("act", [nc.ACT_NONE, nc.ACT_RELU, nc.ACT_LRELU])
@pytest.mark.parametrize("case", FULL_CASES, ids=_ids(FULL_CASES))
def test_instance_norm_act(ops, case, act):
    x = nc.default_input(case["shape"])
    for affine, with_res in nc.param_grid(case, act):
        _hold_fp32(ops, case["name"], case["shape"], x, affine, with_res, act)


@pytest.mark.parametrize("case", CAP_CASES, ids=_ids(CAP_CASES))
def test_instance_norm_act_beyond_the_block_caps(ops, case):
    """More elements than 8192 workgroups cover in one pass of in_apply / in_bwd_apply: the grid-stride loop takes the rest.
    L of these paths is in the hundreds (S = 256 and 1024 splits summed by one thread), so the backward runs without an
    activation; the forward with LeakyReLU."""
    x = nc.default_input(case["shape"])
    _hold_fp32(ops, case["name"], case["shape"], x, True, True, nc.ACT_LRELU, backward=False)
    _hold_fp32(ops, case["name"], case["shape"], x, True, True, nc.ACT_NONE)


@pytest.mark.parametrize("case", CAPACT_CASES, ids=_ids(CAPACT_CASES))
def test_instance_norm_act_beyond_the_block_caps_with_activation(ops, case):
    """Beyond the caps with few splits (L below 100): LeakyReLU both ways, so the mask recomputation of in_bwd_apply<V4> runs in
    the grid-stride remainder."""
    _hold_fp32(ops, case["name"], case["shape"], nc.default_input(case["shape"]), True, True, nc.ACT_LRELU)


def _nhwc_dev(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).cuda().permute(0, 3, 1, 2)


@pytest.mark.parametrize("io", nc.IO_PAIRINGS, ids=lambda io: f"x16={int(io[0])}_y16={int(io[1])}")
@pytest.mark.parametrize("case", nc.IO_CASES, ids=_ids(nc.IO_CASES))
def test_instance_norm_act_io(ops, case, io):
    """ops.instance_norm_act_io: the reference consumes the bf16-rounded x (and dy, which has y's type); y and dx are rounded
    once when they are stored as bf16."""
    shape, (x16, y16) = case["shape"], io
    x = nc.default_input(shape)
    x = nc.bf16_round(x) if x16 else x
    L_fwd, L_bwd = nc.path_L(shape, x16, y16), nc.path_L(shape, x16, y16, backward=True)
    for affine, act in nc.IO_COMBOS:
        scale, shift, _ = nc.case_params(shape, affine, False)
        gout = nc.upstream(shape)
        gout = nc.bf16_round(gout) if y16 else gout
        (r64, r32), gout = nc.norm_yardstick(x, scale, shift, None, act, L_fwd, gout)
        xd = _nhwc_dev(x, torch.bfloat16 if x16 else torch.float32).requires_grad_(True)
        scd, shd = (t.cuda().requires_grad_(True) for t in (scale, shift)) if affine else (None, None)
        y = ops.instance_norm_act_io(xd, scd, shd, act, nc.SLOPE, nc.EPS, y16)
        assert y.dtype == (torch.bfloat16 if y16 else torch.float32)
        grads = torch.autograd.grad(y, [xd, scd, shd] if affine else [xd], _nhwc_dev(gout, y.dtype))
        assert grads[0].dtype == xd.dtype
        what = f"{case['name']} x16={int(x16)} y16={int(y16)} affine={int(affine)} act={act}"
        names = ["y", "dx"] + (["dscale", "dshift"] if affine else [])
        for name, g, a, b in zip(names, [y.detach(), *grads], r64, r32):
            stored16 = (name == "y" and y16) or (name == "dx" and x16)
            nc.check("instance_norm_act_io", f"{what} {name}", g.float(), a, b, L_fwd if name == "y" else L_bwd,
                     nc.bf16_store(a) if stored16 else 0.0)


# The two-pass statistics shift every value by pixel 0 of its column and finish with var = b/HW - (a/HW)^2: a pixel 0 100 sigma
# from the column's mean cancels.  Measured on the MI355X (error of y, forward with ReLU, and its multiple of the bound); no
# shift that repairs it was found inside the run-to-run spread of the benchmark (profiles/LOG.md).
PIXEL0_SHIFT_ERROR = {(2, 8, 64, 64): "6.5e-4 (48 x bound)", (2, 6, 40, 40): "1.7e-4 (27 x bound)", (2, 8, 128, 128): "3.5e-3 (95 x bound)"}


def _hostile_params():
    out = []
    for shape, kind in nc.HOSTILE_CASES:
        marks = ()
        if kind == nc.OUTLIER_FIRST and nc.features(shape)["kind"] == "two-pass":
            marks = pytest.mark.xfail(strict=True, reason="two-pass shift is pixel 0: error " + PIXEL0_SHIFT_ERROR[shape])
        out.append(pytest.param(shape, kind, marks=marks))
    return out


@pytest.mark.parametrize("shape,kind", _hostile_params(), ids=nc.hostile_id)
def test_instance_norm_act_on_hostile_inputs(ops, shape, kind):
    """Offset means, a constant channel, a 100-sigma outlier at the first or the last pixel, an offset first row: finite and
    within the same bound as everything else.  Forward with every activation, backward without one."""
    x = nc.HOSTILE_INPUTS[kind](shape)
    what = "x".join(map(str, shape)) + " " + kind
    for act in (nc.ACT_RELU, nc.ACT_LRELU):
        _hold_fp32(ops, what, shape, x, True, True, act, backward=False)
    _hold_fp32(ops, what, shape, x, True, True, nc.ACT_NONE)


# ---- one launch path behind the six entries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(32, 128, 7, 9), (2, 16, 9, 9)], ids=nc.hostile_id)      # slab R = 1; two-pass, pow2 finish, last block partial
def test_fp32_and_io_entries_agree_bit_for_bit_on_fp32_tensors(ops, shape):
    """ops.instance_norm_act (srgan_instnorm_fwd / _bwd) and ops.instance_norm_act_io with fp32 tensors on both sides
    (srgan_instnorm_fwd_io / _bwd_io) launch the same instantiations with the same grids and arguments
    (norm_common.launch_plan), and the kernels reduce in a fixed order: equal bits, not close values."""
    assert nc.launch_plan(shape, False) == nc.launch_plan(shape, False, (False, False))
    assert nc.launch_plan(shape, True) == nc.launch_plan(shape, True, (False, False))
    x, gout = nc.default_input(shape), nc.upstream(shape)
    for affine, act in nc.IO_COMBOS:
        scale, shift, _ = nc.case_params(shape, affine, False)
        got = []
        for io in (False, True):
            xd = _nhwc_dev(x, torch.float32).requires_grad_(True)
            scd, shd = (t.cuda().requires_grad_(True) for t in (scale, shift)) if affine else (None, None)
            y = (ops.instance_norm_act_io(xd, scd, shd, act, nc.SLOPE, nc.EPS, False) if io else
                 ops.instance_norm_act(xd, scd, shd, None, act, nc.SLOPE, nc.EPS))
            assert y.dtype == torch.float32
            got.append([y.detach(), *torch.autograd.grad(y, [xd, scd, shd] if affine else [xd], _nhwc_dev(gout, torch.float32))])
        for name, a, b in zip(("y", "dx", "dscale", "dshift"), *got):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b), f"{shape} affine={int(affine)} act={act} {name}"


def test_slab_entries_are_the_slab_branch_of_the_io_entries(ops):
    """srgan_instnorm_slab_fwd_io / _slab_bwd_io called directly, bf16 x, y, dy and dx: the bits of srgan_instnorm_fwd_io /
    _bwd_io on the same tensors."""
    from srgan_amd import _lib
    lib = _lib.load()
    shape = (32, 128, 8, 16)
    N, C, H, W = shape
    assert nc.features(shape)["kind"] == "slab"
    p, st = ops._ptr, ops._stream()
    x = _nhwc_dev(nc.default_input(shape), torch.bfloat16)
    dy = _nhwc_dev(nc.upstream(shape), torch.bfloat16)
    scale, shift = (t.cuda() for t in nc.case_params(shape, True, False)[:2])
    nb = lib.srgan_instnorm_workspace(N, H * W, C)
    ws = ops.workspace(x.device, nb)

    def blank(like=None):              # NaN everywhere: an element that no kernel wrote fails the comparison
        return torch.full_like(like, float("nan")) if like is not None else torch.full((N * C,), float("nan"), device="cuda")

    out = []
    for slab in (True, False):
        y, mean, rstd = blank(x), blank(), blank()
        head = (p(x), 1, p(scale), p(shift), None, p(y), 1, p(mean), p(rstd), N, H * W, C, nc.EPS, nc.ACT_LRELU, nc.SLOPE)
        _lib.check(lib.srgan_instnorm_slab_fwd_io(*head, st) if slab else lib.srgan_instnorm_fwd_io(*head, p(ws), nb, st), "forward")
        dx, dscale, dshift = blank(x), blank(), blank()
        head = (p(x), 1, p(dy), 1, p(scale), p(shift), p(mean), p(rstd), p(dx), 1, p(dscale), p(dshift), N, H * W, C, nc.ACT_LRELU, nc.SLOPE)
        _lib.check(lib.srgan_instnorm_slab_bwd_io(*head, st) if slab else lib.srgan_instnorm_bwd_io(*head, p(ws), nb, st), "backward")
        out.append((y, mean, rstd, dx, dscale, dshift))
    for name, a, b in zip(("y", "mean", "rstd", "dx", "dscale", "dshift"), *out):
        assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b), name


@pytest.mark.parametrize("alias", ["y_is_x", "res_is_y"])
def test_instance_norm_forward_in_place(ops, alias):
    """srgan_instnorm_fwd with y == x, and with the skip tensor overwritten by the result: the fused finish of the pow2 apply
    pass would re-read pixel 0 of x while another workgroup stores y there, so these calls take the separate finalize launch
    and in_apply_pow2 without partial sums.  Same yardstick as the out-of-place call; the references use the inputs as they
    were before the call."""
    from srgan_amd import _lib
    lib = _lib.load()
    shape, act = (2, 16, 9, 9), nc.ACT_LRELU
    N, C, H, W = shape
    f = nc.features(shape)
    assert f["kind"] == "two-pass" and f["finish"] == "pow2"
    x = nc.default_input(shape)
    scale, shift, res = nc.case_params(shape, True, alias == "res_is_y")
    r64, r32 = nc.yardstick(nc.norm_ref(act), (x, scale, shift, res), (False,) * 4)
    xd = _nhwc_dev(x, torch.float32)
    y = xd if alias == "y_is_x" else _nhwc_dev(res, torch.float32)
    resd = None if alias == "y_is_x" else y
    scd, shd = scale.cuda(), shift.cuda()
    mean = torch.empty(N * C, device="cuda")
    rstd = torch.empty_like(mean)
    nb = lib.srgan_instnorm_workspace(N, H * W, C)
    ws = ops.workspace(xd.device, nb)
    p = ops._ptr
    _lib.check(lib.srgan_instnorm_fwd(p(xd), p(scd), p(shd), p(resd), p(y), p(mean), p(rstd), N, H * W, C, nc.EPS, act, nc.SLOPE,
                                      p(ws), nb, ops._stream()), "instnorm_fwd")
    nc.check("instnorm_fwd", f"in place ({alias}) y", y, r64[0], r32[0], nc.path_L(shape))


# ---- CBIN affine -------------------------------------------------------------------------------------------------------------------------
CBIN_NAMES = ("scale", "shift", "dc", "dW", "db", "dgamma", "dbeta")


def _cbin_L(name, N, C, num_con, layers=0, visits=1):
    if name in ("scale", "shift"):
        return num_con                      # the dot product of one style code with one row of W
    return nc.cbin_L_dc(C, layers) if name == "dc" else nc.cbin_L_params(N, visits)


@pytest.mark.parametrize("num_con", nc.CBIN_NUM_CON)
def test_cbin_affine(ops, num_con):
    for N in nc.CBIN_N:
        for C in nc.CBIN_C:
            (c, params, g1, g2), r64, r32 = nc.cbin_yardstick(N, C, num_con)
            for want_dc in (True, False):                   # the style code's own gradient requested and not
                dev = [t.detach().cuda().requires_grad_(want_dc or i > 0) for i, t in enumerate((c, *params))]
                scale, shift = ops.cbin_affine(*dev)
                grads = torch.autograd.grad((scale * g1.cuda()).sum() + (shift * g2.cuda()).sum(), dev[0 if want_dc else 1:])
                assert torch.equal(scale.detach().cpu(), params[2][None, :].expand(N, C))     # a copy of gamma per sample
                names = CBIN_NAMES[1:] if want_dc else CBIN_NAMES[1:2] + CBIN_NAMES[3:]
                refs = list(zip(CBIN_NAMES, r64, r32))
                for name, g in zip(names, [shift.detach(), *grads]):
                    _, a, b = next(r for r in refs if r[0] == name)
                    nc.check("cbin_affine", f"N={N} C={C} num_con={num_con} dc={int(want_dc)} {name}", g, a, b,
                             _cbin_L(name, N, C, num_con))


def test_cbin_affine_refuses_more_than_16_conditions(ops):
    from srgan_amd._lib import SrganHipError
    n = nc.CBIN_NUM_CON_REFUSED
    c, params = nc.rnd(3, n, seed=1).cuda(), [t.cuda() for t in nc.cbin_params(8, n, 10)]
    with pytest.raises(SrganHipError, match="1\\.\\.16"):
        ops.cbin_affine(c, *params)
    with pytest.raises(SrganHipError, match="1\\.\\.16"):
        ops.cbin_affine_multi(c, [tuple(params)])


def _multi_loss(outs, weights, dev=None):
    loss = 0
    for l, ((sc, sh), (g1, g2)) in enumerate(zip(outs, weights)):
        g1, g2 = (g1.to(sc.dtype), g2.to(sc.dtype)) if dev is None else (g1.cuda(), g2.cuda())
        loss = loss + (sh * g2).sum() + ((sc * g1).sum() if l != nc.CBIN_MULTI_NO_SCALE_GRAD else 0)
    return loss


def _multi_ref(cs, params, weights, dtype, want_dc):
    """The table reached once per style code of ``cs``: ([outputs per visit], dc per visit or None, [parameter gradients])."""
    cs = [c.detach().clone().to(dtype).requires_grad_(want_dc) for c in cs]
    ps = [tuple(t.detach().clone().to(dtype).requires_grad_(True) for t in p) for p in params]
    outs = [[nc.cbin_ref(c, *p) for p in ps] for c in cs]
    loss = sum(_multi_loss(o, w) for o, w in zip(outs, weights))
    flat = [t for p in ps for t in p]
    grads = torch.autograd.grad(loss, flat + (cs if want_dc else []))
    return outs, (grads[len(flat):] if want_dc else None), grads[:len(flat)]


def _multi_case(N, num_con, visits):
    widths = nc.CBIN_MULTI_WIDTHS
    cs = [nc.rnd(N, num_con, seed=1 + v) for v in range(visits)]
    params = [nc.cbin_params(C, num_con, 100 + 10 * l) for l, C in enumerate(widths)]
    weights = [[(nc.rnd(N, C, seed=300 + 40 * v + l), nc.rnd(N, C, seed=700 + 40 * v + l)) for l, C in enumerate(widths)]
               for v in range(visits)]
    return cs, params, weights


def _check_multi(what, N, num_con, visits, outs, dcs, pgrads, ref64, ref32):
    widths = nc.CBIN_MULTI_WIDTHS
    for v in range(visits):
        for l, C in enumerate(widths):
            assert torch.equal(outs[v][l][0].detach().cpu(), ref32[0][v][l][0].detach())
            nc.check("cbin_affine_multi", f"{what} visit {v} layer {l} shift", outs[v][l][1].detach(), ref64[0][v][l][1].detach(),
                     ref32[0][v][l][1].detach(), num_con)
        if dcs is not None:
            nc.check("cbin_affine_multi", f"{what} visit {v} dc", dcs[v], ref64[1][v], ref32[1][v],
                     nc.cbin_L_dc(max(widths), len(widths)))
    for i, (g, a, b) in enumerate(zip(pgrads, ref64[2], ref32[2])):
        nc.check("cbin_affine_multi", f"{what} layer {i // 4} {('dW', 'db', 'dgamma', 'dbeta')[i % 4]}", g, a, b,
                 nc.cbin_L_params(N, visits))


@pytest.mark.parametrize("want_dc", [True, False], ids=["dc", "no_dc"])
@pytest.mark.parametrize("N,num_con", [(7, 12), (65, 16), (130, 1)])
def test_cbin_affine_multi_17_layers(ops, N, num_con, want_dc):
    """17 layers of mixed widths (the second pass of the layer loop of the dc kernel), one without a gradient on its scale."""
    cs, params, weights = _multi_case(N, num_con, 1)
    ref64, ref32 = (_multi_ref(cs, params, weights, dt, want_dc) for dt in (torch.float64, torch.float32))
    cd = cs[0].cuda().requires_grad_(want_dc)
    pd = [tuple(t.cuda().requires_grad_(True) for t in p) for p in params]
    outs = ops.cbin_affine_multi(cd, pd)
    flat = [t for p in pd for t in p]
    grads = torch.autograd.grad(_multi_loss(outs, weights[0], "cuda"), flat + ([cd] if want_dc else []))
    _check_multi(f"N={N} num_con={num_con}", N, num_con, 1, [outs], grads[len(flat):] if want_dc else None, grads[:len(flat)],
                 ref64, ref32)


def test_cbin_affine_multi_accumulates_a_second_visit(ops):
    """The same table reached twice in one backward pass inside ops.fused_param_grads (the trainer's phase that reuses the
    generator): the second visit's records carry ``accumulate`` and the kernels add to the first visit's sums."""
    N, num_con = 65, 12
    cs, params, weights = _multi_case(N, num_con, 2)
    ref64, ref32 = (_multi_ref(cs, params, weights, dt, True) for dt in (torch.float64, torch.float32))
    cds = [c.cuda().requires_grad_(True) for c in cs]
    pd = [tuple(t.cuda().requires_grad_(True) for t in p) for p in params]
    outs = [ops.cbin_affine_multi(cd, pd) for cd in cds]
    loss = sum(_multi_loss(o, w, "cuda") for o, w in zip(outs, weights))
    with ops.fused_param_grads():
        loss.backward()
    _check_multi("two visits", N, num_con, 2, outs, [cd.grad for cd in cds], [t.grad for p in pd for t in p], ref64, ref32)
