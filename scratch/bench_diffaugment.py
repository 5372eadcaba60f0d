#!/usr/bin/env python3
"""Cost of DiffAugment (SRGAN_training.enable_diffaugment) on the benchmark's workload, and of its kernels alone.

  python scratch/bench_diffaugment.py [--steps 20] [--out FILE]

Part 1: bench.py's trainer (128 x 128, bs 32, k 5, fp32) -- step time with the feature off and with the full policy, eager
launches and hipGraph replay, each after its own warm-up.  Part 2: the kernels at (64, 128, 128) and (32, 256, 256): forward and
backward with colour on (two launches each) and off (one launch), and the two-source forward; each timed as a captured graph of
REPS calls replayed ROUNDS times (device time per call, launch gaps included, no host time), with the bytes each must move
(colour on: the tensor read twice and written once; off: read once, written once) over that time.  Prints one JSON document."""
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


def step_times(policy, graph, steps, warm=4):
    """ms per step (mean over `steps`, and the median of the per-step device times)"""
    device = torch.device("cuda", 0)
    sg = bench.build_trainer(128, 32, 5, device)
    if policy is not None:
        sg.enable_diffaugment(policy=policy, seed=1)
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
    return {"ms_per_step": round(1e3 * wall, 3), "ms_per_step_median": round(per[len(per) // 2], 3)}


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
    from srgan_amd import _lib, ops
    from srgan_amd.augment import DiffAugment
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    aug = DiffAugment(seed=2)
    table = aug.draw(n, h, w).to(dev)
    cut = aug.cut(h, w)
    x = ops.to_nhwc(torch.rand(n, 3, h, w, device=dev) * 2 - 1)
    gy = ops.to_nhwc(torch.randn(n, 3, h, w, device=dev))
    y = torch.empty_like(x)
    nb = lib.srgan_diffaugment_workspace(n, h, w)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    tensor_bytes = 4 * x.numel()
    half = n // 2
    a, b = x[:half], x[half:]

    def fwd(flags):
        return lambda: _lib.check(lib.srgan_diffaugment_fwd(ops._ptr(x), n, None, 0, ops._ptr(table), ops._ptr(y), 3, h, w, flags,
                                                            cut[0], cut[1], ops._ptr(ws), nb, ops._stream()), "fwd")

    def bwd(flags):
        return lambda: _lib.check(lib.srgan_diffaugment_bwd(ops._ptr(gy), ops._ptr(table), ops._ptr(y), n, 3, h, w, flags, cut[0],
                                                            cut[1], ops._ptr(ws), nb, ops._stream()), "bwd")

    def cat():
        _lib.check(lib.srgan_diffaugment_fwd(ops._ptr(a), half, ops._ptr(b), n - half, ops._ptr(table), ops._ptr(y), 3, h, w, 7,
                                             cut[0], cut[1], ops._ptr(ws), nb, ops._stream()), "cat")

    out = {"shape": [n, h, w], "tensor_mb": round(tensor_bytes / 1e6, 2)}
    for name, fn, passes in (("fwd_full_2_launches", fwd(7), 3), ("fwd_no_colour_1_launch", fwd(6), 2),
                             ("bwd_full_2_launches", bwd(7), 3), ("bwd_no_colour_1_launch", bwd(6), 2),
                             ("fwd_two_sources_2_launches", cat, 3), ("copy_flags0_1_launch", fwd(0), 2)):
        us = graph_time_us(fn)
        out[name] = {"us": round(us, 2), "bytes_moved_mb": round(passes * tensor_bytes / 1e6, 2),
                     "tb_per_s": round(passes * tensor_bytes / (us * 1e-6) / 1e12, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    doc = {"workload": "bench.py trainer: 128x128, bs 32, k 5, fp32", "steps": args.steps, "step": {}, "kernels": []}
    for graph in (False, True):
        for policy in (None, "color,translation,cutout", None, "color,translation,cutout"):       # alternated: off, on, off, on
            key = f"{'replay' if graph else 'eager'}_{'on' if policy else 'off'}"
            doc["step"].setdefault(key, []).append(step_times(policy, graph, args.steps))
            torch.cuda.empty_cache()
    for shape in ((64, 128, 128), (32, 256, 256)):
        doc["kernels"].append(kernel_times(*shape))
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
