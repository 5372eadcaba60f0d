#!/usr/bin/env python3
"""Cost of the R1 gradient penalty (SRGAN_training.enable_r1) on the benchmark's workload, and of its two kernels alone.

  python scratch/bench_r1.py [--steps 20] [--out FILE] [--kernels-only]

Part 1: bench.py's trainer (tier F, 128 x 128, bs 32, k 5, fp32) -- step time with the feature off, with every = 1 and with
every = 4, eager launches and hipGraph replay, a fresh trainer per configuration after its own warm-up, the configurations
alternating (off, every 1, every 4, off, every 1, every 4) in one process.  Part 2: r1_seed_kernel + r1_finalize_kernel at
(32, 128, 128) and (32, 256, 256), timed as a captured graph of REPS calls replayed ROUNDS times (device time per call, launch
gaps included, no host time), with the bytes the seed pass must move (h1 read, h2 read, u0 written) over that time.
``--kernels-only`` runs part 2 alone (a kernel trace of it shows the two kernels by name).  Prints one JSON document."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "style-restricted_gan_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import bench  # noqa: E402

REPS, ROUNDS = 20, 10


def step_times(every, graph, steps, warm=4):
    """ms per step (mean over `steps`, and the median of the per-step device times); every = None: feature off"""
    device = torch.device("cuda", 0)
    sg = bench.build_trainer(128, 32, 5, device)
    if every is not None:
        sg.enable_r1(gamma=10.0, every=every)
    if graph:
        sg.enable_graph()
    torch.manual_seed(1000)
    batches = []
    for s in range(steps + warm):
        x, src, tgt = bench.synthetic_batch(32, 128, 4, seed=10_000 + s)
        batches.append((x.to(device), {"source": src.to(device), "target": tgt}))
    for s in range(warm):
        sg.train(*batches[s])
    torch.cuda.synchronize()
    assert not graph or sg.graph_active
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(steps):
        last = sg.train(*batches[warm + i])
        marks[i + 1].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps
    per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    assert all(torch.isfinite(v) for v in last)
    out = {"ms_per_step": round(1e3 * wall, 3), "ms_per_step_median": round(per[len(per) // 2], 3)}
    if every is not None:
        st = sg.r1_stats()
        out["penalised_updates"] = st["updates"]
        out["penalty_last"] = st["penalty"]
    return out


def graph_time_us(fn):
    """device microseconds per call of fn(), from a captured graph of REPS calls"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            fn()
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ROUNDS):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / (REPS * ROUNDS)


def kernel_times(n, h, w):
    from srgan_amd import ops
    dev = torch.device("cuda", 0)
    st = ops.r1_state_new(dev, 10.0, 1, n)
    h1 = ops.to_nhwc(torch.randn(n, 3, h, w, device=dev))
    h2 = ops.to_nhwc(torch.randn(n, 3, (h - 1) // 2 + 1, (w - 1) // 2 + 1, device=dev))
    u0 = torch.empty_like(h1)
    ws = torch.empty(ops.r1_workspace_bytes(n, h, w), dtype=torch.uint8, device=dev)
    moved = 4 * (2 * h1.numel() + h2.numel())
    both = graph_time_us(lambda: (ops.r1_seed_(h1, h2, st, u0, ws), ops.r1_finalize_(ws, n, h, w, st)))
    seed = graph_time_us(lambda: ops.r1_seed_(h1, h2, st, u0, ws))
    return {"shape": [n, h, w], "bytes_moved_mb": round(moved / 1e6, 2), "seed_plus_finalize_us": round(both, 2),
            "seed_us": round(seed, 2), "seed_tb_per_s": round(moved / (seed * 1e-6) / 1e12, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    doc = {"workload": "bench.py trainer: 128x128, bs 32, k 5, fp32", "steps": args.steps, "step": {}, "kernels": []}
    if not args.kernels_only:
        for graph in (False, True):
            for every in (None, 1, 4, None, 1, 4):           # alternated
                key = f"{'replay' if graph else 'eager'}_{'off' if every is None else 'every' + str(every)}"
                doc["step"].setdefault(key, []).append(step_times(every, graph, args.steps))
                torch.cuda.empty_cache()
    for shape in ((32, 128, 128), (32, 256, 256)):
        doc["kernels"].append(kernel_times(*shape))
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
