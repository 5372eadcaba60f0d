"""GPU: batch-statistics norms under data parallelism (dp.sync_batch_stats).  Ranks are processes sharing the one device over
gloo.  The yardstick is always the one-process result of the plain batch path on the concatenated batch (itself pinned to
reference-generated fixtures by tests/test_batchnorm_gpu.py), never the synced path run a second time."""
import os

import numpy as np
import pytest
import torch

from tests import syncbn_common as sc
from tests.common import close, close_grad

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def float64_param_grads():
    """dgamma / dbeta of the float64 restatement (tests/test_batchnorm_gpu.py::ref_batch_norm) for every BN case and call."""
    from tests.test_batchnorm_gpu import ref_batch_norm
    out = {}
    for si, shape in enumerate(sc.OP_SHAPES):
        for vi, (cbb, act, with_res, momentum) in enumerate(sc.OP_VARIANTS):
            if cbb:
                continue
            rm = rv = None
            nbt = [3]
            for call in range(sc.CALLS):
                inp = sc.case_inputs(shape, sc.case_seed(si, vi), call)
                if rm is None:
                    rm, rv = inp["rm"].clone(), inp["rv"].clone()
                x, gam, bet = inp["x"].clone().requires_grad_(True), inp["gam"].clone().requires_grad_(True), inp["bet"].clone().requires_grad_(True)
                ref_batch_norm(x, gam, bet, rm, rv, nbt, True, momentum, act, sc.SLOPE).backward(inp["gy"])
                out[(si, vi, call)] = (gam.grad, bet.grad)
    return out


@pytest.mark.parametrize("world", [2, 4])
def test_synced_ops_equal_the_one_process_op_bit_for_bit(world, float64_param_grads):
    """Every rank's y, mean, rstd, running buffers, counter and dx are torch.equal to the one-process op's on the concatenated
    batch, three consecutive calls; CBB's per-image dscale / dshift too; the running buffers are equal between the ranks; each
    call issues exactly two exchanges of the expected size.  BN's dweight / dbias are LOCAL sums: their rank sum equals the
    one-process value up to summation order, held to the float64 restatement with the bound of
    tests/test_batchnorm_gpu.py::test_ops_match_float64_restatement.  Eval-mode and unmarked modules under the group: identical to
    the modules outside a group, and no exchange."""
    res = sc.spawn(sc.op_worker, world, lambda r, port, q: (r, world, port, q), timeout=500)
    cases = sorted(res[0][1])
    assert len(cases) == len(sc.OP_SHAPES) * len(sc.OP_VARIANTS) * sc.CALLS
    for key in cases:
        si, vi, call = key
        shape, (cbb, act, _, _) = sc.OP_SHAPES[si], sc.OP_VARIANTS[vi]
        for rank, out, _ in res:
            bad = [k for k, ok in out[key]["flags"].items() if not ok]
            assert not bad, (key, shape, "rank", rank, bad)
            assert np.array_equal(out[key]["rm"], res[0][1][key]["rm"]) and np.array_equal(out[key]["rv"], res[0][1][key]["rv"]), key
        if not cbb:
            n, c, h, w = shape
            cmp = close_grad if n * h * w * c >= 1 << 18 and act else close
            for name, j in (("dweight", 0), ("dbias", 1)):
                total = sum(torch.from_numpy(out[key]["d%d" % j]).double() for _, out, _ in res)
                one = torch.from_numpy(res[0][1][key]["ref_d%d" % j]).double()
                print(f"{key} {name}: rank sum vs one process max |diff| {float((total - one).abs().max()):.3e} of {float(one.abs().max()):.3e}")
                cmp(total, float64_param_grads[key][j], 1e-4, what=f"{key} {name} (rank sum)")
                cmp(one, float64_param_grads[key][j], 1e-4, what=f"{key} {name} (one process)")
                # summation order only: the per-image sums are bit-identical in both runs, what differs is the order in which at
                # most 8 of them are added (a few ulp of the largest partial sum; measured 1e-7 relative); a 1/W or W mistake is
                # of the order of the value itself
                assert float((total - one).abs().max()) <= 1e-4 * float(one.abs().max()), (key, name)
    for rank, _, quiet in res:
        assert len(quiet) == 4
        for case, (same, n_calls) in quiet.items():
            assert same and n_calls == 0, (rank, case, same, n_calls)


@pytest.mark.parametrize("transport", ["torch", "abi"])
def test_one_rank_group_over_rccl(transport):
    """The only place the RCCL calls of the synced norms themselves run: a one-rank nccl group with SRGAN_DP_FORCE=1 (two ranks
    cannot share a device under RCCL), through torch.distributed and through the library's C-ABI communicator
    (srgan_allgather_rows, in place).  The synced op is bit-identical to the plain op; with "abi" the forward + backward are also
    captured in a torch.cuda.graph -- the all-gathers inside the capture, the backward's issued from autograd's thread -- and
    three replays are bit-identical to the eager calls, running buffers and counter included."""
    graph = transport == "abi"
    (rank, res), = sc.spawn(sc.onerank_worker, 1, lambda r, port, q: (0, 1, port, q, transport, graph), timeout=300)
    for vi in range(len(sc.OP_VARIANTS)):
        assert res[("eager", vi)] == (True, 2), (vi, res[("eager", vi)])
        if graph:
            assert res[("graph", vi)] == (True, 7), (vi, res[("graph", vi)])


def _compare_runs(res, ref, bound=1e-5):
    dp_losses = sum(np.array(r["losses"]) for _, r in res) / len(res)
    np.testing.assert_allclose(dp_losses[:, :2], np.array(ref["losses"])[:, :2], rtol=1e-3)
    worst = {}
    for key, v in res[0][1]["state"].items():
        if key.endswith("num_batches_tracked"):
            assert int(v) == int(ref["state"][key]), key
            continue
        kind = "running" if "running" in key else "param"
        worst[kind] = max(worst.get(kind, 0.0), float(np.abs(v - ref["state"][key]).max()))
    print("max |2 ranks - 1 process| after the steps:", worst)
    assert worst["param"] <= bound and worst.get("running", 0.0) <= bound, worst
    for _, r in res[1:]:                      # replicas stay replicas: buffers included
        for key, v in r["state"].items():
            assert np.array_equal(v, res[0][1]["state"][key]), key
    return worst


@pytest.mark.parametrize("graph", [False, True])
def test_two_ranks_equal_one_process_batch_mode(graph, golden_dir):
    """Tier T, batch-mode G / D / E with G and E synced: 2 ranks x B/2 against one process x B, 4 steps, with the bounds of
    tests/test_dp_gpu.py::test_two_ranks_equal_one_process (rank-averaged errG / errD at rtol 1e-3, parameters and running buffers
    at 1e-5 absolute); num_batches_tracked equal as integers and equal to what tests/golden/train_T_b4_k2_batch.npz pins.
    graph=True: enable_graph() on the ranks.  The HIP runtime refuses to end, in autograd's thread, a capture begun in the main
    thread (hipErrorStreamCaptureWrongThread), so a synced step is not recorded in the segmented form: every rank runs it eagerly
    (trainer._StepGraph.SEGMENTED_SYNC), with the same results.  The recorded form of a synced step is the single graph of the
    C-ABI transport: test_graph_replay_of_the_synced_step_is_bit_identical_to_eager.
    Measured on an MI355X: parameters within 5.2e-7 and running buffers within 2.4e-7 of the one-process run after the 4 steps."""
    ref = sc.run_trainer(0, 1)
    gold = np.load(os.path.join(golden_dir, "train_T_b4_k2_batch.npz"))
    counts = [int(v) for k, v in ref["state"].items() if k.endswith("num_batches_tracked") and k[0] in "GE"]
    assert counts == [int(c) for c in gold["num_batches_tracked"][sc.STEPS - 1]]
    res = sc.spawn(sc.trainer_worker, 2, lambda r, port, q: (r, 2, port, q, "batch", graph), timeout=400)
    for _, r in res:
        assert r["active"] == [False] * sc.STEPS
        assert [int(v) for k, v in r["state"].items() if k.endswith("num_batches_tracked") and k[0] in "GE"] == counts
    _compare_runs(res, ref)


def test_graph_replay_of_the_synced_step_is_bit_identical_to_eager():
    """The recorded synced step: one rank over RCCL with the C-ABI transport (the collectives are captured, no cut; two ranks
    cannot share a device under RCCL).  Step 0 eager, step 1 records, steps 2 and 3 replay: losses and the state of every network
    after every step are bit-identical to the eager synced steps from the same start, and both equal the plain one-process run."""
    runs = {}
    for graph in (False, True):
        (rank, r), = sc.spawn(sc.trainer_worker, 1, lambda rk, port, q: (0, 1, port, q, "batch", graph, "nccl", True, "abi", True), timeout=400)
        runs[graph] = r
    assert runs[True]["active"] == [False, True, True, True] and runs[False]["active"] == [False] * sc.STEPS
    assert runs[True]["losses"] == runs[False]["losses"]
    for s, (a, b) in enumerate(zip(runs[False]["states"], runs[True]["states"])):
        for k in a:
            assert np.array_equal(a[k], b[k]), (s, k)
    ref = sc.run_trainer(0, 1)
    np.testing.assert_allclose(np.array(runs[True]["losses"]), np.array(ref["losses"]), rtol=1e-4)
    for key, v in runs[True]["state"].items():      # the bound of the two-rank test above: data parallel against one process, 4 steps
        assert float(np.abs(v.astype(np.float64) - ref["state"][key]).max()) <= 1e-5, key
