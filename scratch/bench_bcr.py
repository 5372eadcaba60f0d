#!/usr/bin/env python3
"""Cost of balanced consistency regularisation (SRGAN_training.enable_bcr) on the benchmark's workload, and of its two kernels.

  python scratch/bench_bcr.py [--steps 20] [--out FILE]

Part 1: bench.py's trainer (tier F, 128 x 128, bs 32, k 5, fp32) in graph mode -- ms per step with the feature off (the plain
step), with every = 1 and with every = 4; a fresh trainer per configuration after its own warm-up, the configurations alternating
(off, every 1, every 4, off, every 1, every 4) in one process.  Part 2: one EAGER step of the every = 1 trainer under the library's
own launch timer (srgan_prof_*): launches and mean time per launch of cr_pairs_kernel and d_losses_cr_kernel, with the bytes the
pair builder moves (2B images read, 4B written) over its time.  Prints one JSON document."""
import argparse
import ctypes
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

BATCH, SIZE, K = 32, 128, 5


def make(every, graph):
    device = torch.device("cuda", 0)
    sg = bench.build_trainer(SIZE, BATCH, K, device)
    if every is not None:
        sg.enable_bcr(lambda_real=10.0, lambda_fake=10.0, every=every, seed=1)
    if graph:
        sg.enable_graph()
    return sg, device


def batches_for(device, n):
    out = []
    for s in range(n):
        x, src, tgt = bench.synthetic_batch(BATCH, SIZE, 4, seed=10_000 + s)
        out.append((x.to(device), {"source": src.to(device), "target": tgt}))
    return out


def step_times(every, steps, warm=4):
    """ms per step in graph mode (host clock around `steps` replays ending in a synchronise, and the median of the per-step device
    times); every = None: feature off"""
    sg, device = make(every, True)
    torch.manual_seed(1000)
    batches = batches_for(device, steps + warm)
    for s in range(warm):
        sg.train(*batches[s])
    torch.cuda.synchronize()
    assert sg.graph_active
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
        st = sg.bcr_stats()
        out.update(penalised_updates=st["updates"], cr_real_last=st["cr_real"], cr_fake_last=st["cr_fake"])
    return out


def kernel_times():
    from srgan_amd import _lib
    lib = _lib.load()
    sg, device = make(1, False)
    torch.manual_seed(1000)
    batches = batches_for(device, 3)
    for b in batches[:2]:
        sg.train(*b)
    torch.cuda.synchronize()
    lib.srgan_prof_enable(1)
    sg.train(*batches[2])
    torch.cuda.synchronize()
    lib.srgan_prof_enable(0)
    out = {}
    for kid in range(lib.srgan_prof_num_kernels()):
        name = lib.srgan_prof_kernel_name(kid).decode()
        if name not in ("cr_pairs_kernel", "d_losses_cr_kernel"):
            continue
        ms, n, fl = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double()
        _lib.check(lib.srgan_prof_collect(kid, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)), "prof_collect")
        out[name] = {"launches": int(n.value), "us_per_launch": round(1e3 * ms.value / max(n.value, 1), 2)}
    moved = 4 * 3 * SIZE * SIZE * (2 * BATCH + 4 * BATCH)
    pairs = out["cr_pairs_kernel"]
    pairs["bytes_moved_mb"] = round(moved / 1e6, 2)
    pairs["tb_per_s"] = round(moved / (pairs["us_per_launch"] * 1e-6) / 1e12, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    doc = {"workload": "bench.py trainer: 128x128, bs 32, k 5, fp32, graph mode", "steps": args.steps, "step": {}}
    for every in (None, 1, 4, None, 1, 4):           # alternated
        key = "off" if every is None else f"every{every}"
        doc["step"].setdefault(key, []).append(step_times(every, args.steps))
        torch.cuda.empty_cache()
    doc["kernels"] = kernel_times()
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
