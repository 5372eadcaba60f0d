#!/usr/bin/env python3
"""Cost of the geometric augmentation (SRGAN_training.enable_geometric_augment) on the benchmark's workload, and of its kernels alone.

  python scratch/bench_geom.py [--steps 20] [--out FILE] [--kernels-only]

Part 1: bench.py's trainer (128 x 128, bs 32, k 5, fp32) -- step time with the feature off and with the full policy on, eager
launches and hipGraph replay, a fresh trainer per configuration after its own warm-up, the configurations alternating (off, on,
off, on) in one process.  Part 2: the forward kernel on the 2B = 64 rows of a discriminator update, the forward and the backward on
the B = 32 rows of phase 1, and the gate on 64 rows, each timed as a captured graph of REPS calls replayed ROUNDS times (device time
per call, launch gaps included, no host time), with the bytes the pass must move (one read and one write of the batch; the gathers
re-read through the caches) over that time.  Prints one JSON document."""
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


def step_times(geometry, graph, steps, warm=4):
    """ms per step (mean over `steps`, and the median of the per-step device times)"""
    device = torch.device("cuda", 0)
    sg = bench.build_trainer(128, 32, 5, device)
    if geometry:
        sg.enable_geometric_augment(seed=1)
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
    return {"ms_per_step": round(1e3 * wall, 3), "ms_per_step_median": round(per[len(per) // 2], 3),
            "losses": [float(v) for v in last]}


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


def kernel_times():
    from srgan_amd import _lib, ops
    from srgan_amd.augment import GeometricAugment
    dev = torch.device("cuda", 0)
    out = {}
    geo = GeometricAugment(seed=3)
    state = ops.ada_state_new(dev, 0.5, 0.6, 0.01, 0.8, 4)
    for n in (64, 32):
        x = ops.to_nhwc(torch.rand(n, 3, 128, 128, device=dev))
        table = geo.draw(n, 128, 128).to(dev)
        rows = geo.join_rows(geo.draw(n, 128, 128), geo.draw_gate(n)).to(dev)
        gated = ops.ada_gate(rows, state, 4)
        moved = 2 * x.numel() * 4
        lib_fwd = lambda t=table, g=False: ops.geom_augment(x, t, 15, g)          # noqa: E731
        gy, gx = torch.randn_like(x), torch.empty_like(x)

        def lib_bwd():
            _lib.check(_lib.load().srgan_geom_augment_bwd(ops._ptr(gy), ops._ptr(table), ops._ptr(gx), n, 3, 128, 128, 15, 0, ops._stream()),
                       "geom_augment_bwd")

        entry = {}
        for name, fn in (("fwd", lib_fwd), ("fwd_gated", lambda: lib_fwd(gated, True)),
                         ("bwd", lib_bwd),
                         ("gate", lambda: ops.ada_gate(rows, state, 4))):
            us = graph_time_us(fn)
            entry[name] = {"us": round(us, 2)}
            if name != "gate":
                entry[name]["GB_per_s"] = round(moved / us * 1e-3, 1)
        out[f"{n}x3x128x128"] = entry
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    doc = {"workload": "bench.py trainer: 128x128, bs 32, k 5, fp32", "steps": args.steps, "step": {}}
    if not args.kernels_only:
        for graph in (False, True):
            for geometry in (False, True, False, True):                            # alternated: off, on, off, on
                key = f"{'replay' if graph else 'eager'}_{'geometry' if geometry else 'off'}"
                doc["step"].setdefault(key, []).append(step_times(geometry, graph, args.steps))
                torch.cuda.empty_cache()
    doc["kernels"] = kernel_times()
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
