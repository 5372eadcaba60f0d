"""CPU: batch-statistics norms under data parallelism (dp.sync_batch_stats) without a GPU -- the mark and its predicate, the
trainer's constructor gate under two gloo ranks, argument errors of the synced entry points of the C ABI, their launch
descriptors, and the slab plan that makes a rank's partial rows the rows of the one-process array."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import isa_tools                                                               # noqa: E402
from syncbn_common import bn_plan, exchange_floats, free_port                  # noqa: E402


def _tier_t(norm="batch"):
    from srgan_amd import model
    return [model.SingleGenerator(3, 4, 2, 2, 1, norm, num_con=12), model.SingleDiscriminator_solo_multi(3, 4, 2, 4, norm, 4),
            model.Encoder(3, 8, 4, 4, norm, 4, "cpu")]


def test_mark_and_predicate():
    from srgan_amd import dp, model
    G, D, E = _tier_t()
    keys = [list(net.state_dict()) for net in (G, D, E)]
    assert not model.batch_stats_synced(G) and not model.batch_stats_synced(E)
    assert model.batch_stats_synced(D)                                  # no batch-statistics norm: nothing to mark
    assert dp.sync_batch_stats(G) is G and model.batch_stats_synced(G)
    norms = [m for m in G.modules() if model._is_batch_stat(m)]
    assert norms and all(isinstance(m, (model.BatchNorm2d, model.CBBNorm2d)) and m.sync_stats is True for m in norms)
    w = dp.DataParallel(E, device_ids=[0])
    assert dp.sync_batch_stats(w) is w and model.batch_stats_synced(w) and model.batch_stats_synced(E)
    assert [list(net.state_dict()) for net in (G, D, E)] == keys        # the mark is no parameter and no buffer
    assert list(w.state_dict()) == ["module." + k for k in keys[2]]
    dp.sync_batch_stats(G, enable=False)
    assert not model.batch_stats_synced(G) and model.batch_stats_synced(E)
    for net in _tier_t("instance"):                                     # instance mode: a no-op, and true
        assert model.batch_stats_synced(net) and dp.sync_batch_stats(net) is net and model.batch_stats_synced(net)
        assert not any(hasattr(m, "sync_stats") for m in net.modules())
    # a batch norm of another class has no synced path: it stays unmarked and keeps the network refused
    other = torch.nn.Sequential(torch.nn.BatchNorm2d(4))
    assert not model.batch_stats_synced(dp.sync_batch_stats(other))
    # without a process group a marked norm takes the one-process path (here: the CPU refusal of that path, no collective)
    from srgan_amd import _lib
    with pytest.raises(_lib.SrganHipError, match="no CPU fallback"):
        dp.sync_batch_stats(model.BatchNorm2d(8))(torch.zeros(2, 8, 4, 4))


def _gate_worker(rank, world, port, out):
    import numpy as np
    import torch.nn as nn
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from srgan_amd import dp
    from srgan_amd.trainer import SRGAN_training
    dp.init_from_env("gloo")
    try:
        lbd = {"class": 1.0, "cycle": 5.0, "idt": 5.0, "reg": 0.5, "idt_reg": 0.5, "KL": 0.0, "batch_KL": 0.0, "corr_enc": 0.0,
               "hist": 0.0}
        got = {}
        for case, (mark_g, mark_e, wrap) in dict(unmarked=(0, 0, 0), both=(1, 1, 0), both_wrapped=(1, 1, 1), only_g=(1, 0, 0),
                                                 only_e=(0, 1, 0)).items():
            G, D, E = _tier_t()
            if wrap:
                G, E = dp.DataParallel(G), dp.DataParallel(E)
            if mark_g:
                dp.sync_batch_stats(G)
            if mark_e:
                dp.sync_batch_stats(E)
            try:
                SRGAN_training([G, D, E], [None] * 3, [nn.MSELoss(), nn.MSELoss()], lbd, 2, "cpu", np.eye(4), 4, "mu", 8)
                got[case] = "constructed"
            except NotImplementedError as e:
                got[case] = str(e)
        out[rank] = got
    finally:
        torch.distributed.destroy_process_group()


def test_two_rank_trainer_gate():
    import torch.multiprocessing as mp
    out = mp.Manager().dict()
    mp.spawn(_gate_worker, args=(2, free_port(), out), nprocs=2, join=True)
    for r in (0, 1):
        got = out[r]
        assert got["both"] == "constructed" and got["both_wrapped"] == "constructed", got
        for case in ("unmarked", "only_g", "only_e"):
            assert "batch-statistics norms" in got[case] and "per-replica statistics" in got[case], got[case]
            assert "dp.sync_batch_stats" in got[case], got[case]
        assert got["unmarked"] == got["only_g"] == got["only_e"]


def test_fingerprint_and_fallback_follow_the_mark():
    """The recording's fingerprint takes the mark; a synced network under a process group without the single-graph transport
    names the segmented form as the reason to run eagerly (no process group here: the reason is absent)."""
    from srgan_amd import dp, model, trainer
    fp = trainer._StepGraph._fingerprint
    assert "synced batch norms in the segmented form" in trainer._StepGraph.SEGMENTED_SYNC

    class Opt:
        param_groups, state = (), {}

    class SG:
        k, n_batch, ndim, encoded_feature, lbd, criterion, criterion_class, ref_label = 2, 4, 8, "mu", {}, None, None, [[1.0]]
        optG = optD = optE = Opt()

        def _opts(self):
            return (self.optG, self.optD, self.optE)

        def _extensions(self):
            return []
    sg = SG()
    sg.G, sg.D, sg.E = _tier_t()
    g = trainer._StepGraph.__new__(trainer._StepGraph)
    g.sg = sg
    g._all_params = lambda: []
    a = fp(g)
    dp.sync_batch_stats(sg.G)
    b = fp(g)
    dp.sync_batch_stats(sg.G, enable=False)
    assert a != b and fp(g) == a
    dp.sync_batch_stats(sg.E)
    assert g._synced_norms()
    sg.E.eval()
    assert not g._synced_norms()                                        # eval-mode norms issue no collective


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from srgan_amd import _lib
    return _lib


def test_abi_argument_errors_without_a_gpu(lib):
    L = lib.load()
    buf = (ctypes.c_char * (1 << 16))()
    b = ctypes.cast(buf, ctypes.c_void_p)
    err = L.srgan_last_error
    NG, NL, HW, C = 4, 2, 16, 8
    nb = L.srgan_batchnorm_sync_exchange_bytes(NG, NL, HW, C, 0)
    nbs = L.srgan_batchnorm_sync_exchange_bytes(NG, NL, HW, C, 1)
    wb = L.srgan_batchnorm_sync_workspace(NL, C)
    assert nb == 4 * exchange_floats(NG, NL, HW, C, False) and nbs == 4 * exchange_floats(NG, NL, HW, C, True) == nb + 4 * NG * C
    assert wb == 4 * (2 * NL * C + C) and L.srgan_batchnorm_sync_workspace(0, C) == 0
    assert L.srgan_batchnorm_sync_exchange_bytes(2, 4, HW, C, 0) == 0 and L.srgan_batchnorm_sync_exchange_bytes(4, 3, HW, C, 0) == 0
    geo = lambda ng=NG, n0=0, nl=NL, hw=HW, c=C: (ng, n0, nl, hw, c)           # noqa: E731
    fwd_p = lambda xb=nb, **k: L.srgan_batchnorm_sync_fwd_partial(b, b, xb, *geo(**k), None)      # noqa: E731
    fwd_bn = lambda xb=nb, x=b, **k: L.srgan_batchnorm_sync_fwd_apply(x, None, None, b, b, b, b, b, b, None, None, None, b, xb, *geo(**k), 0.1, 0, 1e-5, 1, 0.0, None)      # noqa: E731
    fwd_cbb = lambda xb=nb, sc=b, **k: L.srgan_cbbnorm_sync_fwd_apply(b, sc, b, None, b, b, b, b, b, b, None, None, None, b, xb, *geo(**k), 0.1, 0, 1e-5, 1, 0.0, None)      # noqa: E731
    bwd_p = lambda xb=nbs, sc=b, **k: L.srgan_batchnorm_sync_bwd_partial(b, b, sc, b, b, b, b, b, xb, *geo(**k), 1, 0.0, None)      # noqa: E731
    bwd_bn = lambda xb=nb, ws=wb, **k: L.srgan_batchnorm_sync_bwd_apply(b, b, b, b, b, b, b, b, b, xb, b, b, b, *geo(**k), 1, 0.0, b, ws, None)      # noqa: E731
    bwd_cbb = lambda xb=nbs, ws=wb, **k: L.srgan_cbbnorm_sync_bwd_apply(b, b, b, b, b, b, b, b, xb, b, b, b, *geo(**k), 1, 0.0, b, ws, None)      # noqa: E731
    every = dict(fwd_partial=fwd_p, fwd_bn=fwd_bn, fwd_cbb=fwd_cbb, bwd_partial=bwd_p, bwd_bn=bwd_bn, bwd_cbb=bwd_cbb)
    for name, f in every.items():
        assert f(nl=8) == -1 and b"N_local > N_global" in err(), name
        assert f(nl=3, n0=0) == -1 and b"not a multiple of N_local" in err(), name
        for n0 in (4, -2, 1):
            assert f(n0=n0) == -1 and b"rank offset outside the global batch" in err(), (name, n0)
        assert f(c=6) == -1 and b"C % 4" in err(), name
        assert f(ng=1, nl=1, hw=1) == -1 and b"Expected more than 1 value per channel when training" in err(), name
        assert f(hw=0) == -1 and b"bad shape" in err(), name
        assert f(xb=nb - 1) == -1 and b"exchange buffer too small" in err(), name
        # sized for the LOCAL batch (what srgan_batchnorm_workspace(N_local, ...) holds for partials): the trunk's 256 x 32 x 32
        big = dict(ng=8, nl=4, hw=32 * 32, c=256)
        local_bytes = 4 * 8 * bn_plan(4, 32 * 32, 256)[0] * 256
        assert local_bytes == L.srgan_batchnorm_sync_exchange_bytes(4, 4, 32 * 32, 256, 0) < L.srgan_batchnorm_sync_exchange_bytes(8, 4, 32 * 32, 256, 0)
        assert f(xb=local_bytes, **big) == -1 and b"exchange buffer too small" in err(), name
    # the "more than 1 value per channel" check applies to the GLOBAL count: one image of one pixel per rank passes it (and
    # fails on the next check, the null pointer)
    assert L.srgan_batchnorm_sync_fwd_partial(None, b, nb, 2, 1, 1, 1, 8, None) == -1 and b"null pointer" in err()
    assert L.srgan_batchnorm_sync_fwd_partial(None, b, nb, *geo(), None) == -1 and b"null pointer" in err()
    assert fwd_bn(x=None) == -1 and b"batchnorm_sync_fwd_apply: null pointer" in err()
    assert fwd_cbb(sc=None) == -1 and b"scale / shift" in err()
    assert L.srgan_batchnorm_sync_fwd_apply(b, None, None, b, b, b, b, b, b, b, b, None, b, nb, *geo(), 0.0, 1, 1e-5, 1, 0.0, None) == -1
    assert b"num_batches_tracked" in err()
    assert L.srgan_batchnorm_sync_fwd_apply(b, b, None, b, b, b, b, b, b, None, None, None, b, nb, *geo(), 0.1, 0, 1e-5, 1, 0.0, None) == -1
    assert b"weight and bias go together" in err()
    assert bwd_bn(ws=wb - 1) == -1 and b"workspace too small" in err()
    assert bwd_cbb(ws=wb - 1) == -1 and b"workspace too small" in err()
    assert bwd_cbb(xb=nb) == -1 and b"exchange buffer too small" in err()      # the CBB backward's chunks carry the scale rows
    assert bwd_p(xb=nb) == -1 and b"exchange buffer too small" in err()


def test_ops_keyword_defaults_off_and_cpu_tensors_are_refused(lib):
    import inspect
    from srgan_amd import ops
    for fn in (ops.batch_norm_act, ops.cbb_norm_act):
        assert inspect.signature(fn).parameters["sync"].default is False
    with pytest.raises(lib.SrganHipError, match="no CPU fallback"):
        ops.batch_norm_act(torch.zeros(2, 8, 4, 4), None, None, None, None, None, True, sync=True)


# ---- the slab plan ------------------------------------------------------------------------------------------------------------
def _norm_shapes(H):
    sys.path.insert(0, os.path.join(HERE, "hip_shim"))
    from drive_batchnorm import norm_shapes
    return [(hw, c, cbb) for _, _, hw, c, cbb in norm_shapes(H, 1)]


def test_local_and_global_slab_plans_differ():
    """The statement of the issue, checked: with C = 64, HW = 128 * 128 the plans of 4 and of 8 images have different S."""
    assert bn_plan(4, 128 * 128, 64)[0] != bn_plan(8, 128 * 128, 64)[0]
    assert bn_plan(4, 128 * 128, 64) == (128, 128) and bn_plan(8, 128 * 128, 64) == (64, 256)
    assert any(bn_plan(NG // W, hw, c)[0] != bn_plan(NG, hw, c)[0] for NG in (32, 64) for W in (2, 4, 8) for H in (128, 256)
               for hw, c, _ in _norm_shapes(H))


@pytest.mark.parametrize("NG", [32, 64])
@pytest.mark.parametrize("W", [2, 4, 8])
def test_rank_rows_are_the_rows_of_the_global_layout(lib, NG, W):
    """The exchange buffer the library sizes is the one-process partial array [N_global][S][C] of the GLOBAL plan (forward and BN
    backward), cut into W equal chunks: the float2 rows [r * N_local, (r + 1) * N_local) are exactly rank r's chunk -- and it is
    NOT what the local plan would give wherever the two plans differ."""
    L = lib.load()
    NL = NG // W
    for H in (64, 128, 256):
        for hw, c, cbb in _norm_shapes(H) + [(128 * 128, 64, 1)]:
            S, rps = bn_plan(NG, hw, c)
            assert S * rps >= hw and (S == 1 or hw // S >= 64)
            nb = L.srgan_batchnorm_sync_exchange_bytes(NG, NL, hw, c, 0)
            assert nb == NG * S * c * 8 == L.srgan_batchnorm_workspace(NG, hw, c) - 4 * (2 * NG * c + c)
            chunk = nb // W
            for r in range(W):
                first_row, last_row = r * NL * S * c * 8, (r + 1) * NL * S * c * 8
                assert (first_row, last_row) == (r * chunk, (r + 1) * chunk)
            Sl, _ = bn_plan(NL, hw, c)
            if Sl != S:
                assert NG * Sl * c * 8 != nb
            # CBB backward: every chunk additionally ends in its images' scale rows
            assert L.srgan_batchnorm_sync_exchange_bytes(NG, NL, hw, c, 1) == nb + NG * c * 4


# ---- launch descriptors (no GPU: tests/hip_shim/launch_shim.c logs them) --------------------------------------------------------
@pytest.mark.parametrize("H,NG", [(64, 32), (128, 32), (128, 64), (256, 32)])
@pytest.mark.parametrize("W", [2, 4, 8])
def test_launch_descriptors_within_aql_limits(lib, H, NG, W, tmp_path):
    so = str(tmp_path / "launch_shim.so")
    subprocess.run(["gcc", "-shared", "-fPIC", "-O1", "-o", so, os.path.join(HERE, "hip_shim", "launch_shim.c")], check=True)
    desc = {k["name"]: k for k in isa_tools.kernel_descriptors(lib.LIB_PATH)}
    log = str(tmp_path / "launches.log")
    env = dict(os.environ, LD_PRELOAD=so, SRGAN_SHIM_LOG=log)
    env.pop("SRGAN_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "hip_shim", "drive_syncbn.py"), lib.LIB_PATH, str(H), str(NG), str(W)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    n, kernels, NL = 0, set(), NG // W
    for line in open(log):
        if line.startswith("#"):
            continue
        kname, gx, gy, gz, bx, by, bz, dyn = line.split()
        gx, gy, gz, bx, by, bz, dyn = map(int, (gx, gy, gz, bx, by, bz, dyn))
        k = desc[kname]
        threads = bx * by * bz
        ctx = (kname, (gx, gy, gz), (bx, by, bz))
        assert min(gx, gy, gz, bx, by, bz) >= 1, ctx
        assert threads % 64 == 0 and threads <= k["max_wg"], ctx
        assert gx * bx < 2 ** 32 and gy < 2 ** 16 and gz < 2 ** 16, ctx
        assert k["lds"] + dyn <= 160 * 1024 and k["scratch"] == 0, ctx
        if "bn_stats_partial" in kname or "bn_bwd_partial" in kname:     # the slab passes cover the LOCAL images only
            assert gz == NL, ctx
        n += 1
        kernels.add(kname)
    assert any("bn_sync_finalize" in k for k in kernels) and any("bn_sync_bwd_combine" in k for k in kernels), sorted(kernels)
    assert any("bn_sync_pack_scale" in k for k in kernels)
    assert not any(k.endswith("bn_finalize") or "11bn_finalizeE" in k or "14bn_bwd_combineE" in k for k in kernels), sorted(kernels)
    assert n >= 100 and len(kernels) >= 8, (n, sorted(kernels))
