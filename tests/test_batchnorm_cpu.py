"""CPU: norm_type="batch" without a GPU -- module state (state-dict layout, seed-7 initialisation, load_state_dict, the
pretrained-E freeze_melt pattern) against tests/golden/batchnorm_host.json (made by running the reference), the data-parallel
pass-through and refusal, argument errors of the C ABI, and the launch descriptors of the new kernels."""
import collections
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import isa_tools                                                               # noqa: E402


@pytest.fixture(scope="module")
def host():
    with open(os.path.join(HERE, "golden", "batchnorm_host.json")) as f:
        return json.load(f)


def _nets(nch=4):
    from srgan_amd import model
    return dict(G=lambda: model.SingleGenerator(3, nch, 2, 2, 1 if nch == 4 else 2, "batch", num_con=12),
                E=lambda: model.Encoder(3, 8, nch, 4, "batch", 4, "cpu"),
                E_original=lambda: model.Encoder_original(3, 8, nch, 4, "batch", 4, "cpu"),
                E_classifier=lambda: model.Encoder_classifier(3, 8, nch, 4, "batch", 4))


def test_state_dict_layout_matches_the_reference(host):
    for name, make in _nets().items():
        got = [[k, list(v.shape), str(v.dtype)] for k, v in make().state_dict().items()]
        assert got == host["layout"][name], name


def test_seed7_initialisation_matches_the_reference(host):
    torch.manual_seed(7)
    nets = _nets(8)
    built = {n: nets[n]() for n in ("G", "E", "E_original")}          # the reference's construction order
    for name, net in built.items():
        want = host["init_seed7"][name]
        got = [[k, float(v.double().sum()), float(v.double().abs().sum())] for k, v in net.state_dict().items()]
        assert [g[0] for g in got] == [w[0] for w in want], name
        for (k, s, a), (_, ws, wa) in zip(got, want):
            assert abs(s - ws) <= 1e-5 * max(1.0, abs(wa)) and abs(a - wa) <= 1e-5 * max(1.0, abs(wa)), (name, k, s, ws)


def test_load_state_dict_round_trip_and_missing_counter():
    from srgan_amd import model
    nets = _nets()
    for name, make in nets.items():
        a, b = make(), make()
        with torch.no_grad():
            for i, (k, v) in enumerate(a.state_dict().items()):
                v.copy_(torch.full_like(v, i + 1) if v.dtype == torch.long else torch.randn_like(v))
        b.load_state_dict(a.state_dict())
        for (k, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):
            assert torch.equal(va, vb), (name, k)
    # CBBNorm2d: loads (the reference's raises NameError, model.py:163); a missing num_batches_tracked loads as 0
    n = model.CBBNorm2d(8, 4)
    sd = collections.OrderedDict((k, v.clone()) for k, v in n.state_dict().items() if not k.endswith("num_batches_tracked"))
    n.num_batches_tracked.fill_(5)
    n.load_state_dict(sd)
    assert int(n.num_batches_tracked) == 0 and n.num_batches_tracked.dtype == torch.long
    bn = model.BatchNorm2d(8)                     # nn.BatchNorm2d's own version handling: an old checkpoint loads
    assert isinstance(bn, torch.nn.BatchNorm2d) and bn._version == torch.nn.BatchNorm2d._version
    bn.load_state_dict(collections.OrderedDict((k, v) for k, v in bn.state_dict().items() if not k.endswith("num_batches_tracked")))
    # the variants of the reference constructor
    assert model.CBBNorm2d(8, 4, affine=False).weight is None
    nt = model.CBBNorm2d(8, 4, track_running_stats=False)
    assert nt.running_mean is None and list(nt.state_dict()) == ["weight", "bias", "ConBias.0.weight", "ConBias.0.bias"]
    assert model.get_norm_layer("batch", 4)[1](8).num_con == 4


def test_freeze_melt_pattern_matches_the_reference(host):
    from srgan_amd import model
    E = model.Encoder(3, 8, 4, 4, "batch", 4, "cpu")
    keys = list(model.Encoder_classifier(3, 8, 4, 4, "batch", 4).state_dict().keys())
    E.freeze_melt(keys, "freeze")
    assert [[k, bool(p.requires_grad)] for k, p in E.named_parameters()] == host["freeze_requires_grad"]


def test_per_sample_predicate_and_dp_pass_through():
    from srgan_amd import dp, model
    G = model.SingleGenerator(3, 4, 2, 2, 1, "batch", num_con=12)
    Gi = model.SingleGenerator(3, 4, 2, 2, 1, "instance", num_con=12)
    assert not model.per_sample(G) and model.per_sample(Gi)
    assert not model.per_sample(model.Encoder(3, 8, 4, 4, "batch", 4, "cpu"))
    assert not model.per_sample(model.Encoder_original(3, 8, 4, 4, "batch", 4, "cpu"))
    w = dp.DataParallel(G, device_ids=[0])
    assert dp.unwrap(w) is G and list(w.state_dict()) == ["module." + k for k in G.state_dict()]
    seen = []
    G.forward = lambda *a: seen.append(a) or "out"
    assert w("x", "c") == "out" and seen == [("x", "c")]


def _dp_worker(rank, world, port, out):
    import numpy as np
    import torch.nn as nn
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from srgan_amd import dp, model
    from srgan_amd.trainer import SRGAN_training
    dp.init_from_env("gloo")
    try:
        lbd = {"class": 1.0, "cycle": 5.0, "idt": 5.0, "reg": 0.5, "idt_reg": 0.5, "KL": 0.0, "batch_KL": 0.0, "corr_enc": 0.0,
               "hist": 0.0}
        nets = [model.SingleGenerator(3, 4, 2, 2, 1, "batch", num_con=12), model.SingleDiscriminator_solo_multi(3, 4, 2, 4, "batch", 4),
                model.Encoder(3, 8, 4, 4, "batch", 4, "cpu")]
        try:
            SRGAN_training(nets, [None] * 3, [nn.MSELoss(), nn.MSELoss()], lbd, 2, "cpu", np.eye(4), 4, "mu", 8)
            out[rank] = "constructed"
        except NotImplementedError as e:
            out[rank] = str(e)
    finally:
        torch.distributed.destroy_process_group()


def test_two_rank_trainer_refuses_batch_norms():
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = mp.Manager().dict()
    mp.spawn(_dp_worker, args=(2, port, out), nprocs=2, join=True)
    for r in (0, 1):
        assert "batch-statistics norms" in out[r] and "per-replica statistics" in out[r], out[r]


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
    nb = L.srgan_batchnorm_workspace(2, 16, 8)
    assert nb > 0 and L.srgan_batchnorm_workspace(0, 16, 8) == 0
    args = lambda n, hw, c, tr, ws=b, wsb=nb: (n, hw, c, tr, 0.1, 0, 1e-5, 1, 0.0, ws, wsb, None)      # noqa: E731
    assert L.srgan_batchnorm_fwd(None, None, None, b, b, b, b, b, b, None, None, None, *args(2, 16, 8, 1)) == -1
    assert b"batchnorm_fwd: null pointer" in L.srgan_last_error()
    assert L.srgan_batchnorm_fwd(b, None, None, b, b, b, b, b, b, None, None, None, *args(2, 16, 6, 1)) == -1
    assert b"C % 4" in L.srgan_last_error()
    assert L.srgan_cbbnorm_fwd(b, b, b, None, b, b, b, b, b, b, None, None, None, *args(1, 1, 8, 1)) == -1
    assert b"Expected more than 1 value per channel when training" in L.srgan_last_error()
    assert L.srgan_cbbnorm_fwd(b, None, b, None, b, b, b, b, b, b, None, None, None, *args(2, 16, 8, 1)) == -1
    assert b"scale / shift" in L.srgan_last_error()
    assert L.srgan_batchnorm_fwd(b, None, None, b, b, b, b, b, b, None, None, None, *args(2, 16, 8, 0)) == -1
    assert b"eval mode without running statistics" in L.srgan_last_error()
    assert L.srgan_batchnorm_fwd(b, None, None, b, b, b, b, b, b, b, b, None, 2, 16, 8, 1, 0.0, 1, 1e-5, 1, 0.0, b, nb, None) == -1
    assert b"num_batches_tracked" in L.srgan_last_error()
    assert L.srgan_batchnorm_fwd(b, None, None, b, b, b, b, b, b, None, None, None, *args(2, 16, 8, 1, wsb=nb - 1)) == -1
    assert b"workspace too small" in L.srgan_last_error()
    assert L.srgan_batchnorm_bwd(b, b, b, b, b, b, b, b, b, b, b, 2, 16, 10, 1, 1, 0.0, b, nb, None) == -1
    assert b"C % 4" in L.srgan_last_error()
    assert L.srgan_cbbnorm_bwd(b, b, None, b, b, b, b, b, b, b, b, 2, 16, 8, 1, 1, 0.0, b, nb, None) == -1
    assert b"cbbnorm_bwd: null pointer" in L.srgan_last_error()
    assert L.srgan_batchnorm_bwd(b, b, b, b, b, b, b, b, b, b, b, 1, 1, 8, 1, 1, 0.0, b, nb, None) == -1
    assert b"Expected more than 1 value" in L.srgan_last_error()


def test_ops_refuse_bad_channel_counts_and_cpu_tensors(lib):
    from srgan_amd import ops
    with pytest.raises(lib.SrganHipError, match="no CPU fallback"):
        ops.batch_norm_act(torch.zeros(2, 8, 4, 4), None, None, None, None, None, True)


# ---- launch descriptors of the new entry points (no GPU: tests/hip_shim/launch_shim.c logs them) --------------------------------
GEOMETRIES = [(64, 8), (128, 32), (128, 64), (256, 16)]


@pytest.mark.parametrize("H,B", GEOMETRIES)
def test_launch_descriptors_within_aql_limits(lib, H, B, tmp_path):
    so = str(tmp_path / "launch_shim.so")
    subprocess.run(["gcc", "-shared", "-fPIC", "-O1", "-o", so, os.path.join(HERE, "hip_shim", "launch_shim.c")], check=True)
    desc = {k["name"]: k for k in isa_tools.kernel_descriptors(lib.LIB_PATH)}
    log = str(tmp_path / "launches.log")
    env = dict(os.environ, LD_PRELOAD=so, SRGAN_SHIM_LOG=log)
    env.pop("SRGAN_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "hip_shim", "drive_batchnorm.py"), lib.LIB_PATH, str(H), str(B)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    n, kernels = 0, set()
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
        n += 1
        kernels.add(kname)
    assert n >= 50 and len(kernels) >= 7, (n, sorted(kernels))
