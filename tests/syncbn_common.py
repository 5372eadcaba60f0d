"""Shared pieces of the synced batch-norm tests (dp.sync_batch_stats): a host restatement of the kernels' slab plan, the
deterministic op-level cases, and the rank workers (spawned processes: importable top-level functions)."""
import os
import socket
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BN_CH = 32


def bn_plan(N, HW, C):
    """csrc/norm_batch.hip bn_plan: (S slabs per image, pixel rows per slab)."""
    blocks = N * ((C + BN_CH - 1) // BN_CH)
    S = 1
    while blocks * S < 1024 and HW // (S * 2) >= 64:
        S *= 2
    return S, (HW + S - 1) // S


def exchange_floats(N_global, N_local, HW, C, with_scale):
    """Floats of the exchange buffer: N_global / N_local rank chunks of [N_local][S][C] float2 (+ [N_local][C] scale rows)."""
    S, _ = bn_plan(N_global, HW, C)
    return N_global * (2 * S * C + (C if with_scale else 0))


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def child_paths():
    for p in (ROOT, os.path.join(ROOT, "style-restricted_gan_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)


def spawn(target, world, make_args, timeout=300):
    """tests/test_dp_gpu.py::_spawn for any worker: one result per rank, every process reaped whatever happens (a rank that
    dies must not leave its peers parked in a collective on the GPU)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=target, args=make_args(r, port, q)) for r in range(world)]
    try:
        for p in procs:
            p.start()
        res = sorted([q.get(timeout=timeout) for _ in procs], key=lambda t: t[0])
        for p in procs:
            p.join(timeout=120)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
                if p.is_alive():
                    p.kill()
                    p.join(timeout=10)
    assert [p.exitcode for p in procs] == [0] * world, [p.exitcode for p in procs]
    return res


def init_rank(rank, world, port, backend="gloo", force=False, transport=None):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), SRGAN_DP_DEVICE="0", SRGAN_DP_BACKEND=backend)
    if force:
        os.environ["SRGAN_DP_FORCE"] = "1"
    if transport:
        os.environ["SRGAN_DP_COMM"] = transport
    child_paths()
    from srgan_amd import dp
    dp.init_from_env()
    assert dp.world_size() == world and dp.is_distributed()
    return dp


# ---- op-level cases ---------------------------------------------------------------------------------------------------------
# global shapes: one small, one whose slab count differs between the local and the global plan (test_syncbn_cpu checks that it
# does), the generator trunk's 256 x 32 x 32
OP_SHAPES = [(4, 8, 16, 16), (8, 64, 128, 128), (8, 256, 32, 32)]
# (cbb, act, with_res, momentum)
OP_VARIANTS = [(False, 0, False, 0.1), (False, 2, False, None), (True, 1, False, 0.1), (True, 0, True, None)]
CALLS = 3
SLOPE = 0.2


def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _fp32(t):
    return t.float().double()


def case_inputs(shape, seed, call):
    """float64 CPU tensors holding fp32-exact values, as tests/test_batchnorm_gpu.py::run_case draws them; x and dy change with
    the call, the parameters and the initial running buffers do not."""
    n, c, h, w = shape
    return dict(x=_fp32(_rnd(*shape, seed=seed + 100 * call) * 1.5 + 0.3), gy=_fp32(_rnd(*shape, seed=seed + 100 * call + 6)),
                gam=_fp32(1 + 0.25 * _rnd(c, seed=seed + 1)), bet=_fp32(0.1 * _rnd(c, seed=seed + 2)),
                sc=_fp32(1 + 0.25 * _rnd(n, c, seed=seed + 3)), sh=_fp32(0.3 * _rnd(n, c, seed=seed + 4)),
                res=_fp32(_rnd(*shape, seed=seed + 100 * call + 5)), rm=_fp32(0.2 * _rnd(c, seed=seed + 7)),
                rv=_fp32(1 + 0.5 * _rnd(c, seed=seed + 8).abs()))


def case_seed(si, vi):
    return 1000 * si + 10 * vi + 1


def run_op(ops, inp, rows, variant, buffers, sync, training=True):
    """One forward + backward of the op on the images `rows` of the case.  Returns y, the kept statistics and the gradients."""
    cbb, act, with_res, momentum = variant
    dev = dict(device="cuda", dtype=torch.float32)
    x = inp["x"][rows].to(**dev).requires_grad_(True)
    rm, rv, nbt = buffers
    if cbb:
        p0, p1 = inp["sc"][rows].to(**dev).requires_grad_(True), inp["sh"][rows].to(**dev).requires_grad_(True)
        y = ops.cbb_norm_act(x, p0, p1, rm, rv, nbt if training else None, training, momentum, 1e-5, act, SLOPE,
                             inp["res"][rows].to(**dev) if with_res else None, sync=sync)
    else:
        p0, p1 = inp["gam"].to(**dev).requires_grad_(True), inp["bet"].to(**dev).requires_grad_(True)
        y = ops.batch_norm_act(x, p0, p1, rm, rv, nbt if training else None, training, momentum, 1e-5, act, SLOPE, sync=sync)
    saved = y.grad_fn.saved_tensors
    mean, rstd = (saved[2], saved[3]) if cbb else (saved[1], saved[2])
    y.backward(inp["gy"][rows].to(**dev))
    return dict(y=y.detach(), mean=mean.clone(), rstd=rstd.clone(), dx=x.grad, d0=p0.grad, d1=p1.grad)


def new_buffers(inp):
    dev = dict(device="cuda", dtype=torch.float32)
    return [inp["rm"].to(**dev), inp["rv"].to(**dev), torch.tensor(3, dtype=torch.long, device="cuda")]


def op_worker(rank, world, port, q):
    """Every op case on this rank: the synced op on its rows against the plain op on the whole batch, run here on the same
    device (torch.equal on the device; only flags, parameter gradients and running buffers travel back)."""
    dp = init_rank(rank, world, port)
    import torch.distributed as dist
    from srgan_amd import model, ops
    out = {}
    try:
        for si, shape in enumerate(OP_SHAPES):
            per = shape[0] // world
            rows = slice(rank * per, (rank + 1) * per)
            for vi, variant in enumerate(OP_VARIANTS):
                cbb = variant[0]
                ref_buf = syn_buf = None
                for call in range(CALLS):
                    inp = case_inputs(shape, case_seed(si, vi), call)
                    if ref_buf is None:
                        ref_buf, syn_buf = new_buffers(inp), new_buffers(inp)
                    ref = run_op(ops, inp, slice(0, shape[0]), variant, ref_buf, False)
                    dp.exchange_trace = []
                    got = run_op(ops, inp, rows, variant, syn_buf, True)
                    trace, dp.exchange_trace = dp.exchange_trace, None
                    flags = {k: bool(torch.equal(got[k], ref[k][rows])) for k in ("y", "dx")}
                    flags.update({k: bool(torch.equal(got[k], ref[k])) for k in ("mean", "rstd")})
                    flags.update(running_mean=bool(torch.equal(syn_buf[0], ref_buf[0])), running_var=bool(torch.equal(syn_buf[1], ref_buf[1])),
                                 num_batches_tracked=int(syn_buf[2]) == int(ref_buf[2]) == 4 + call)
                    if cbb:      # per-image parameter gradients: this rank's rows of the one-process ones
                        flags.update(dscale=bool(torch.equal(got["d0"], ref["d0"][rows])), dshift=bool(torch.equal(got["d1"], ref["d1"][rows])))
                    S, _ = bn_plan(shape[0], shape[2] * shape[3], shape[1])
                    want = [(("cbb_norm" if cbb else "batch_norm") + ".forward", exchange_floats(shape[0], per, shape[2] * shape[3], shape[1], False)),
                            (("cbb_norm" if cbb else "batch_norm") + ".backward", exchange_floats(shape[0], per, shape[2] * shape[3], shape[1], cbb))]
                    flags["exchanges"] = trace == want
                    out[(si, vi, call)] = dict(flags=flags, d0=got["d0"].cpu().numpy(), d1=got["d1"].cpu().numpy(),
                                               rm=syn_buf[0].cpu().numpy(), rv=syn_buf[1].cpu().numpy(),
                                               ref_d0=ref["d0"].cpu().numpy() if rank == 0 and not cbb else None,
                                               ref_d1=ref["d1"].cpu().numpy() if rank == 0 and not cbb else None)
        # eval mode and unmarked norms under the group: the one-process modules on the local rows, and no collective
        torch.manual_seed(5)
        quiet = {}
        x = torch.randn(8 // world, 16, 32, 32, device="cuda")
        c = torch.randn(8 // world, 4, device="cuda")
        for name, make, args in (("bn", lambda: model.BatchNorm2d(16), ()), ("cbb", lambda: model.CBBNorm2d(16, 4), (c,))):
            for mode in ("eval_marked", "train_unmarked"):
                torch.manual_seed(9)
                a = make().cuda()
                b = make().cuda()
                b.load_state_dict(a.state_dict())
                if mode == "eval_marked":
                    dp.sync_batch_stats(a)
                    a.eval(), b.eval()
                dp.exchange_trace = []
                ya = a(x, *args)
                ya.sum().backward()
                n_calls, dp.exchange_trace = len(dp.exchange_trace), None
                # `b` through the plain ops with no process group in sight: what the module does today
                saved = dp.is_distributed
                dp.is_distributed = lambda: False
                try:
                    yb = b(x, *args)
                    yb.sum().backward()
                finally:
                    dp.is_distributed = saved
                same = torch.equal(ya, yb) and all(torch.equal(va, vb) for va, vb in zip(a.state_dict().values(), b.state_dict().values()))
                same = same and all(torch.equal(pa.grad, pb.grad) for pa, pb in zip(a.parameters(), b.parameters()))
                quiet[(name, mode)] = (bool(same), n_calls)
        q.put((rank, out, quiet))
        dist.barrier()
    finally:
        dist.destroy_process_group()


# ---- one rank over RCCL -----------------------------------------------------------------------------------------------------
def onerank_worker(rank, world, port, q, transport, graph):
    """SRGAN_DP_FORCE=1, one-rank nccl group: the synced op (both all-gathers through RCCL) against the plain op; graph: the
    synced forward + backward captured in a torch.cuda.graph (abi transport: the collectives are captured) and replayed."""
    dp = init_rank(0, 1, port, backend="nccl", force=True, transport=transport)
    import torch.distributed as dist
    from srgan_amd import ops
    res = {}
    try:
        assert dp.transport() == transport
        shape = (4, 64, 64, 64)
        for vi, variant in enumerate(OP_VARIANTS):
            inp = case_inputs(shape, case_seed(7, vi), 0)
            rows = slice(0, shape[0])
            ref_buf, syn_buf = new_buffers(inp), new_buffers(inp)
            ref = run_op(ops, inp, rows, variant, ref_buf, False)
            dp.exchange_trace = []
            got = run_op(ops, inp, rows, variant, syn_buf, True)
            n_calls, dp.exchange_trace = len(dp.exchange_trace), None
            ok = all(torch.equal(got[k], ref[k]) for k in got) and all(torch.equal(a, b) for a, b in zip(ref_buf, syn_buf))
            res[("eager", vi)] = (bool(ok), n_calls)
            if graph:
                cbb, act, with_res, momentum = variant
                dev = dict(device="cuda", dtype=torch.float32)
                xs = inp["x"].to(**dev).requires_grad_(True)
                p0 = (inp["sc"] if cbb else inp["gam"]).to(**dev).requires_grad_(True)
                p1 = (inp["sh"] if cbb else inp["bet"]).to(**dev).requires_grad_(True)
                r, gy = inp["res"].to(**dev), inp["gy"].to(**dev)
                gbuf = new_buffers(inp)

                def body():
                    if cbb:
                        y = ops.cbb_norm_act(xs, p0, p1, gbuf[0], gbuf[1], gbuf[2], True, momentum, 1e-5, act, SLOPE, r if with_res else None, sync=True)
                    else:
                        y = ops.batch_norm_act(xs, p0, p1, gbuf[0], gbuf[1], gbuf[2], True, momentum, 1e-5, act, SLOPE, sync=True)
                    return (y,) + torch.autograd.grad(y, (xs, p0, p1), gy)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    body()                                   # warm-up outside the capture (advances the buffers once)
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    outs = body()
                # eager twin: the same four calls (warm-up + three) from the same start
                ebuf = new_buffers(inp)
                same = True
                run_op(ops, inp, rows, variant, ebuf, True)
                for _ in range(3):
                    g.replay()
                    e = run_op(ops, inp, rows, variant, ebuf, True)
                    torch.cuda.synchronize()
                    same = same and all(torch.equal(a, b) for a, b in zip(outs, (e["y"], e["dx"], e["d0"], e["d1"])))
                    same = same and all(torch.equal(a, b) for a, b in zip(gbuf, ebuf))
                res[("graph", vi)] = (bool(same), int(gbuf[2]))
        q.put((0, res))
        dist.barrier()
    finally:
        dist.destroy_process_group()


# ---- the trainer ------------------------------------------------------------------------------------------------------------
K, B, STEPS = 2, 4, 4


def noise_source(rank, world):
    gen = torch.Generator().manual_seed(77)

    def fn(batch, ndim):          # every rank draws the GLOBAL noise and keeps its rows
        full = torch.randn(batch * world, ndim, generator=gen)
        return full[rank * batch:(rank + 1) * batch].clone()
    return fn


def batch_trainer(norm="batch", sync=False):
    """tests/test_batchnorm_gpu.py::_trainer with the optimisers of tests/test_dp_gpu.py::_run (Adam with a large eps is nearly
    linear in the gradient, so rounding-level differences are not amplified to O(lr))."""
    import torch.nn as nn
    from oracle import params, trainer as otrainer
    from srgan_amd import dp, model, optim as hoptim
    from srgan_amd.trainer import SRGAN_training
    from tests.batch_common import batch_fill
    G = batch_fill(model.SingleGenerator(3, 4, 2, 2, 1, norm, num_con=12), 0)
    E = batch_fill(model.Encoder(3, 8, 4, 4, norm, 4, "cuda"), 2)
    D = model.SingleDiscriminator_solo_multi(3, 4, 2, 4, norm, 4)
    D.load_state_dict(params.fill(params.discriminator_spec(nch_in=3, nch=4, reduce=2, num_cls=4, n_class=4), 1))
    if sync:
        dp.sync_batch_stats(G)
        dp.sync_batch_stats(E)
    torch.manual_seed(0)
    np.random.seed(0)
    nets = [G.cuda(), D.cuda(), E.cuda()]
    opts = [hoptim.Adam(list(net.parameters()), lr=1e-4, betas=(0.5, 0.999), eps=1e-2) for net in nets]
    sg = SRGAN_training(nets, opts, [nn.MSELoss(), nn.MSELoss()], dict(otrainer.DEFAULT_LBD), K, "cuda", np.eye(4), B, "mu", 8)
    sg.opt_sche_initialization()
    return sg


def run_trainer(rank, world, norm="batch", graph=False, steps=STEPS, keep_states=False):
    from oracle import trainer as otrainer
    from srgan_amd import dp
    sg = batch_trainer(norm, sync=dp.is_distributed())
    if graph:
        sg.enable_graph()
    sg.noise_fn = noise_source(rank, world)
    per = B // world
    losses, states, active = [], [], []
    for s in range(steps):
        x, label = otrainer.synthetic_batch(B, 128, 4, seed=100 + s)
        sl = slice(rank * per, (rank + 1) * per)
        lab = {"source": label["source"][sl].cuda(), "target": label["target"][sl]}
        losses.append([float(v) for v in sg.train(x[sl].cuda(), lab)])
        active.append(bool(sg.graph_active))
        if keep_states:
            states.append({f"{n}.{k}": v.detach().cpu().numpy().copy() for n, net in (("G", sg.G), ("D", sg.D), ("E", sg.E))
                           for k, v in net.state_dict().items()})
    state = {f"{n}.{k}": v.detach().cpu().numpy().copy() for n, net in (("G", sg.G), ("D", sg.D), ("E", sg.E))
             for k, v in net.state_dict().items()}
    return dict(losses=losses, state=state, states=states, active=active)


def trainer_worker(rank, world, port, q, norm, graph, backend="gloo", force=False, transport=None, keep_states=False):
    dp = init_rank(rank, world, port, backend=backend, force=force, transport=transport)
    import torch.distributed as dist
    try:
        q.put((rank, run_trainer(rank, world, norm, graph, keep_states=keep_states)))
        dist.barrier()
    finally:
        dist.destroy_process_group()
