"""CPU: the parts of spectral normalisation (srgan_amd.spectral, srgan_spectral_* of the C ABI) that need no GPU -- the float64
restatement of tests/sn_common.py pinned to torch.nn.utils.spectral_norm, the gradient formula against autograd, argument errors
before any launch, the table layout, the host-side refusals and the launch descriptors."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import sn_common as sn


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from srgan_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.srgan_last_error().decode()


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------
def test_restatement_follows_torch_spectral_norm_with_one_forward_per_step():
    """two convs in float64, 4 Adam steps: torch's hook (one training forward per step) against project -> Adam -> iterate on the
    restated state; outputs at every step and the weights after the last one to 1e-12"""
    torch.manual_seed(0)
    ref = nn.Sequential(nn.Conv2d(3, 5, 3, bias=True), nn.LeakyReLU(0.2), nn.Conv2d(5, 2, 4, stride=2, bias=False)).double()
    W0 = {i: ref[i].weight.detach().clone() for i in (0, 2)}
    b0 = ref[0].bias.detach().clone()
    for i in (0, 2):
        torch.nn.utils.spectral_norm(ref[i])
    uv = {i: (ref[i].weight_u.detach().clone(), ref[i].weight_v.detach().clone()) for i in (0, 2)}
    ref.train()
    opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-2, betas=(0.5, 0.999))

    st = sn.Restated(W0, uv=uv)                          # the iteration at application = the one in torch's first forward
    orig = {i: W0[i].clone().requires_grad_(True) for i in (0, 2)}
    bias = b0.clone().requires_grad_(True)
    opt = torch.optim.Adam([bias, orig[0], orig[2]], lr=1e-2, betas=(0.5, 0.999))
    x = torch.randn(4, 4, 3, 12, 12, dtype=torch.float64)
    for s in range(4):
        y_ref = ref(x[s])
        opt_ref.zero_grad()
        (y_ref ** 2).sum().backward()
        opt_ref.step()

        leaf = {i: st.Wsn[i].clone().requires_grad_(True) for i in (0, 2)}
        bias.grad = None
        h = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(x[s], leaf[0], bias), 0.2)
        y = torch.nn.functional.conv2d(h, leaf[2], None, 2)
        (y ** 2).sum().backward()
        assert float((y - y_ref).detach().abs().max()) <= 1e-12 * max(1.0, float(y_ref.detach().abs().max())), s
        for i in (0, 2):
            orig[i].grad = st.project(i, leaf[i].grad)
        opt.step()
        for i in (0, 2):
            st.W[i] = orig[i].detach().clone()
        st.refresh()
    for i in (0, 2):
        assert float((orig[i] - ref[i].weight_orig).detach().abs().max()) <= 1e-12, i
    assert float((bias - ref[0].bias).detach().abs().max()) <= 1e-12
    y_ref = ref(x[0])                                    # one more training forward: torch's (u, v) catch up with the restated ones
    for i in (0, 2):
        assert float((st.u[i] - ref[i].weight_u).abs().max()) <= 1e-12 and float((st.v[i] - ref[i].weight_v).abs().max()) <= 1e-12


@pytest.mark.parametrize("shape", [(1, 16, 4, 4), (2, 3, 4, 4), (4, 8, 8, 8), (5, 7, 3, 3), (64, 3, 4, 4), (33, 9, 2, 2)])
def test_gradient_formula_equals_autograd_through_w_over_sigma(shape):
    g = torch.Generator().manual_seed(sum(shape))
    W = torch.randn(shape, dtype=torch.float64, generator=g).requires_grad_(True)
    u, v = sn.iterate(W.detach().reshape(shape[0], -1), sn.normalize(torch.randn(shape[0], dtype=torch.float64, generator=g)),
                      sn.normalize(torch.randn(W[0].numel(), dtype=torch.float64, generator=g)))
    sigma, Wsn = sn.materialize(W, u, v)                  # u, v constants, as torch detaches them
    G = torch.randn(shape, dtype=torch.float64, generator=g)
    (Wsn * G).sum().backward()
    got = sn.project(G, Wsn.detach(), u, v, sigma.detach())
    assert float((got - W.grad).abs().max()) <= 1e-12 * float(W.grad.abs().max())


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
def _host_table(layers, base=1 << 20):
    rows = []
    for i, (o, k) in enumerate(layers):
        b = base + (i << 16)
        rows += [b, b + 4096, b + 8192, b + 12288, base - 64 + 4 * i, o, k] + [0] * 9
    return (ctypes.c_char * (8 * len(rows))).from_buffer_copy(struct.pack(f"{len(rows)}Q", *rows))


def _plan(lib, layers):
    host = _host_table(layers)
    plan = (ctypes.c_char * lib.srgan_spectral_plan_bytes())()
    assert lib.srgan_spectral_plan(ctypes.byref(host), len(layers), ctypes.byref(plan)) == 0, _err(lib)
    return host, plan


def test_table_layout(lib):
    """sixteen 64-bit words per record; the plan holds the three work lists' lengths and the workspace size"""
    assert lib.srgan_spectral_record_bytes() == 128 and lib.srgan_spectral_plan_bytes() == 40
    layers = [(1, 4096), (2, 48), (4, 16384), (5, 63), (512, 4096), (33, 1025)]
    host, plan = _plan(lib, layers)
    n, _, slab_items, col_items, elem_items, ws_floats = struct.unpack("iiqqqq", bytes(plan))
    recs = np.frombuffer(bytes(host), dtype=np.uint64).reshape(len(layers), 16).astype(np.int64)
    slab = col = elem = ws = 0
    r4 = lambda x: -(-x // 4) * 4                                                    # noqa: E731
    for (o, k), rec in zip(layers, recs):
        nslab, ncc, nch = -(-o // 32), -(-k // 1024), -(-(o * k) // 4096)
        assert tuple(rec[5:10]) == (o, k, slab, col, elem)
        want = []
        for size in (nslab * k, k, ncc, o * ncc, nch):
            want.append(ws)
            ws += r4(size)
        assert tuple(rec[10:15]) == tuple(want) and rec[15] == 0 and all(w % 4 == 0 for w in want)
        slab, col, elem = slab + nslab * ncc, col + ncc, elem + nch
    assert (n, slab_items, col_items, elem_items, ws_floats) == (len(layers), slab, col, elem, ws)
    assert lib.srgan_spectral_workspace(ctypes.byref(plan)) == 4 * ws


def test_bad_arguments_return_minus_one_without_a_gpu(lib):
    buf = (ctypes.c_char * 4096)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    host, plan = _plan(lib, [(4, 100), (1, 4096)])
    ws = lib.srgan_spectral_workspace(ctypes.byref(plan))
    pl = ctypes.byref(plan)
    big = (ctypes.c_char * (ws + 16))()
    w = ctypes.c_void_p((ctypes.addressof(big) + 15) & ~15)
    refresh, project = lib.srgan_spectral_refresh, lib.srgan_spectral_project
    zero = (ctypes.c_char * 40)()                                                   # a plan of zero records
    for it in (0, 1):
        assert refresh(None, pl, it, 1, 1e-12, w, ws, None) == -1 and "NULL table" in _err(lib)
        assert refresh(b, None, it, 1, 1e-12, w, ws, None) == -1 and "spectral_refresh" in _err(lib)
        assert refresh(b, ctypes.byref(zero), it, 1, 1e-12, w, ws, None) == -1 and "0 records" in _err(lib)
        assert refresh(b, pl, it, 1, 1e-12, None, ws, None) == -1 and "workspace" in _err(lib)
        assert refresh(b, pl, it, 1, 1e-12, w, ws - 4, None) == -1 and "workspace" in _err(lib)
        assert refresh(b, pl, it, 1, 1e-12, ctypes.c_void_p(w.value + 4), ws, None) == -1 and "aligned" in _err(lib)
        for eps in (0.0, -1e-12, float("nan")):
            assert refresh(b, pl, it, 1, eps, w, ws, None) == -1 and "eps" in _err(lib), eps
        for n in (0, -2):
            assert refresh(b, pl, it, n, 1e-12, w, ws, None) == -1 and "n_power_iterations" in _err(lib), n
    assert project(None, pl, b, w, ws, None) == -1 and "NULL table" in _err(lib)
    assert project(b, ctypes.byref(zero), b, w, ws, None) == -1 and "0 records" in _err(lib)
    assert project(b, pl, None, w, ws, None) == -1 and "gradient table" in _err(lib)
    assert project(b, pl, b, w, ws - 4, None) == -1 and "workspace" in _err(lib)
    assert lib.srgan_spectral_workspace(None) == 0 and "spectral_workspace" in _err(lib)
    assert lib.srgan_spectral_workspace(ctypes.byref(zero)) == 0
    # the plan refuses records it cannot serve, and writes nothing then
    out = (ctypes.c_char * 40)()
    assert lib.srgan_spectral_plan(None, 1, ctypes.byref(out)) == -1 and lib.srgan_spectral_plan(ctypes.byref(host), 0, ctypes.byref(out)) == -1
    for o, k in ((0, 16), (4, 0), (1 << 16, 1 << 15)):
        bad = _host_table([(2, 48), (o, k)])
        before = bytes(bad)
        assert lib.srgan_spectral_plan(ctypes.byref(bad), 2, ctypes.byref(out)) == -1 and "record 1" in _err(lib), (o, k)
        assert bytes(bad) == before
    nul = _host_table([(2, 48)])
    nul[0:8] = b"\x00" * 8                                                          # W = NULL
    assert lib.srgan_spectral_plan(ctypes.byref(nul), 1, ctypes.byref(out)) == -1 and "pointer" in _err(lib)
    assert all(c == b"\x00" for c in buf) and all(c == b"\x00" for c in big) and all(c == b"\x00" for c in out)   # nothing was touched


# ---- host side ---------------------------------------------------------------------------------------------------------------------
def _cpu_nets():
    from srgan_amd import model
    from tests.common import TIER_T
    g, d, e = TIER_T["G"], TIER_T["D"], TIER_T["E"]
    G = model.SingleGenerator(g["nch_in"], g["nch"], g["reduce"], g["num_cls"], g["res_num"], "instance", num_con=g["num_con"])
    D = model.SingleDiscriminator_solo_multi(d["nch_in"], d["nch"], d["reduce"], d["num_cls"], "instance", d["n_class"])
    E = model.Encoder(e["nch_in"], e["nch_out"], e["nch"], e["num_cls"], "instance", e["num_con"], "cpu")
    return G, D, E


def test_layer_order_of_the_restatement_is_the_module_order():
    from oracle import params
    from srgan_amd import model
    from tests.common import TIER_T
    _, D, _ = _cpu_nets()
    convs = [n + ".weight" for n, m in D.named_modules() if isinstance(m, model._Conv2d)]
    assert convs == sn.sn_keys(params.fill(params.discriminator_spec(**TIER_T["D"]), 1)) and len(convs) == 12


def test_host_side_refusals():
    from srgan_amd import model, spectral
    from srgan_amd.trainer import SingleGAN_training, SRGAN_training
    G, D, E = _cpu_nets()
    with pytest.raises(RuntimeError, match="move the network to the GPU"):          # .to() would not move the plain attribute
        spectral.spectral_norm(D)
    assert "weight" in dict(D.discriminator1.down_convs[0].named_parameters())       # refused before anything was changed
    with pytest.raises(NotImplementedError, match="transposed convolution / linear"):
        spectral.spectral_norm(G)
    with pytest.raises(NotImplementedError, match="transposed convolution / linear"):
        spectral.spectral_norm(E)
    with pytest.raises(NotImplementedError, match="transposed convolution / linear"):
        spectral.spectral_norm(nn.Sequential(model._Conv2d(3, 4, 3), model._Linear(4, 2)))
    for bad in (0, -1):
        with pytest.raises(ValueError, match="n_power_iterations"):
            spectral.spectral_norm(D, n_power_iterations=bad)
    for bad in (0.0, float("nan")):
        with pytest.raises(ValueError, match="eps"):
            spectral.spectral_norm(D, eps=bad)
    for call in (spectral.remove_spectral_norm, spectral.sigmas, spectral.refresh, spectral.project, spectral.zero_grad):
        with pytest.raises(RuntimeError, match="not marked"):
            call(D)
    assert spectral.controller(D) is None and spectral.find(D) == []

    # a mark, as far as the refusals look at it (applying one needs the GPU)
    class Mark:
        leaves = []
    lbd = dict(**{"class": 1.0}, cycle=5.0, idt=5.0, reg=0.5, idt_reg=0.5, KL=0.0, batch_KL=10.0, corr_enc=0.0, hist=0.0)
    crit = [nn.MSELoss(), nn.MSELoss()]

    def marked(net, where=None):
        (where if where is not None else net).__dict__[spectral._ATTR] = Mark()
        spectral._marks_epoch += 1
        return net

    def unmark(net, where=None):
        del (where if where is not None else net).__dict__[spectral._ATTR]
        spectral._marks_epoch += 1

    marked(D)
    with pytest.raises(RuntimeError, match="marked already"):                        # a second application
        spectral.spectral_norm(D)
    unmark(D)
    for name, net in (("G", G), ("E", E)):
        marked(net)
        with pytest.raises(NotImplementedError, match=f"{name} is marked.*remove_spectral_norm"):
            SRGAN_training([G, D, E], [None] * 3, crit, lbd, 1, "cpu", np.eye(4), 4, "mu", 8)
        unmark(net)
    marked(D, D.discriminator1)
    with pytest.raises(NotImplementedError, match="whole discriminator"):
        SRGAN_training([G, D, E], [None] * 3, crit, lbd, 1, "cpu", np.eye(4), 4, "mu", 8)
    unmark(D, D.discriminator1)
    from srgan_amd import dp
    sg = SRGAN_training([G, D, E], [None] * 3, crit, lbd, 1, "cpu", np.eye(4), 4, "mu", 8)   # unmarked: nothing to refuse
    assert sg._sn() is None
    marked(D)
    orig = dp.world_size
    dp.world_size = lambda: 2
    try:
        with pytest.raises(NotImplementedError, match="2 ranks.*remove_spectral_norm"):
            sg._sn()                                                                 # what train() asks first
    finally:
        dp.world_size = orig
    with pytest.raises(NotImplementedError, match="SingleGAN_training.*SRGAN_training"):
        SingleGAN_training([G, D, E], [None] * 3, crit, lbd, 1, "cpu", np.eye(4), 8, [0, 1, 2, 3], singleD=True)
    unmark(D)
    SingleGAN_training([G, D, E], [None] * 3, crit, lbd, 1, "cpu", np.eye(4), 8, [0, 1, 2, 3], singleD=True)


# ---- launch descriptors (no GPU: tests/hip_shim/launch_shim.c logs them) ----------------------------------------------------------
KERNELS = ("sn_wtu_partials_kernel", "sn_vnorm_partials_kernel", "sn_wv_partials_kernel", "sn_unorm_sigma_kernel", "sn_scale_kernel",
           "sn_dot_partials_kernel", "sn_project_kernel")


def test_launch_descriptors_within_aql_limits_and_launch_counts(lib, tmp_path):
    """tier F's discriminator (12 layers) and a single 1 x 4096 layer: the same number of launches, within the caps (6 per
    refresh, 3 per projection with the upload of the gradient pointers), every descriptor inside the AQL limits"""
    from srgan_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    import isa_tools
    so = str(tmp_path / "launch_shim.so")
    subprocess.run(["gcc", "-shared", "-fPIC", "-O1", "-o", so, os.path.join(here, "hip_shim", "launch_shim.c")], check=True)
    desc = {k["name"]: k for k in isa_tools.kernel_descriptors(_lib.LIB_PATH)}
    log = str(tmp_path / "launches.log")
    env = dict(os.environ, LD_PRELOAD=so, SRGAN_SHIM_LOG=log)
    env.pop("SRGAN_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(here, "hip_shim", "drive_spectral.py"), _lib.LIB_PATH], env=env, capture_output=True,
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
        short = next((s for s in KERNELS if s in kname), None)
        assert short is not None, kname
        k = desc[kname]
        ctx = (cur, kname, (gx, gy, gz), (bx, by, bz))
        assert min(gx, gy, gz, bx, by, bz) >= 1 and (bx, by, bz) == (256, 1, 1) and 256 <= k["max_wg"], ctx
        assert gx * bx < 2 ** 32 and gy < 2 ** 16 and gz < 2 ** 16, ctx
        assert k["lds"] + dyn <= 160 * 1024 and k["scratch"] == 0 and dyn == 0, ctx
        seen[cur].append((short, gx))
    sys.path.insert(0, os.path.join(here, "hip_shim"))
    import drive_spectral
    for name, layers in drive_spectral.CASES:
        slab = sum(-(-o // 32) * -(-k // 1024) for o, k in layers)
        col = sum(-(-k // 1024) for o, k in layers)
        elem = sum(-(-(o * k) // 4096) for o, k in layers)
        g = lambda n: min(n, 2048)                                                   # noqa: E731
        assert seen[f"{name}: refresh"] == [(KERNELS[0], g(slab)), (KERNELS[1], g(col)), (KERNELS[2], g(slab)),
                                            (KERNELS[3], len(layers)), (KERNELS[4], g(elem))], name
        assert seen[f"{name}: materialise"] == [(KERNELS[2], g(slab)), (KERNELS[3], len(layers)), (KERNELS[4], g(elem))], name
        assert seen[f"{name}: project"] == [(KERNELS[5], g(elem)), (KERNELS[6], g(elem))], name
        assert len(seen[f"{name}: refresh"]) <= 6 and len(seen[f"{name}: project"]) + 1 <= 3
    assert [len(seen[f"discriminator: {w}"]) for w in ("refresh", "materialise", "project")] == \
        [len(seen[f"one layer: {w}"]) for w in ("refresh", "materialise", "project")]
