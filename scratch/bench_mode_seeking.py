#!/usr/bin/env python3
"""Cost of mode-seeking regularisation (SRGAN_training.enable_mode_seeking) on the benchmark's workload, and of its three kernels.

  python scratch/bench_mode_seeking.py [--steps 20] [--out FILE]

Part 1: bench.py's trainer (tier F, 128 x 128, bs 32, k 5, fp32) eagerly and in graph mode -- ms per step with the feature off (the
plain step) and on (form msgan); a fresh trainer per configuration after its own warm-up, the configurations alternating (off, on,
off, on) per mode in one process.  Part 2: one EAGER step of the trainer with the feature on under the library's own launch timer
(srgan_prof_*): launches and mean time per launch of the three kernels, with the bytes each streaming pass must move over its time.
Part 3: the reduction pass alone, 50 launches between two device events, at the step's shape (32 x 3 x 128 x 128) and at
64 x 3 x 256 x 256 (where the launch itself no longer dominates): achieved bytes per second.  Prints one JSON document."""
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
KERNELS = ("ms_rows_kernel", "ms_finish_kernel", "ms_grad_kernel")


def make(on, graph):
    device = torch.device("cuda", 0)
    sg = bench.build_trainer(SIZE, BATCH, K, device)
    if on:
        sg.enable_mode_seeking(weight=1.0, form="msgan", seed=1)
    if graph:
        sg.enable_graph()
    return sg, device


def batches_for(device, n):
    out = []
    for s in range(n):
        x, src, tgt = bench.synthetic_batch(BATCH, SIZE, 4, seed=10_000 + s)
        out.append((x.to(device), {"source": src.to(device), "target": tgt}))
    return out


def step_times(on, graph, steps, warm=4):
    """ms per step (host clock around `steps` steps ending in a synchronise, and the median of the per-step device times)"""
    sg, device = make(on, graph)
    torch.manual_seed(1000)
    batches = batches_for(device, steps + warm)
    for s in range(warm):
        sg.train(*batches[s])
    torch.cuda.synchronize()
    assert sg.graph_active == graph
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
    out = {"ms_per_step": round(1e3 * wall, 3), "ms_per_step_median": round(per[len(per) // 2], 3),
           "losses_last": [round(float(v), 5) for v in last]}
    if on:
        st = sg.mode_seeking_stats()
        out.update(updates=st["updates"], ms_last=st["ms"], d_image_last=st["d_image"], d_latent_last=st["d_latent"])
    return out


def kernel_times():
    from srgan_amd import _lib
    lib = _lib.load()
    sg, device = make(True, False)
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
        if name not in KERNELS:
            continue
        ms, n, fl = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double()
        _lib.check(lib.srgan_prof_collect(kid, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)), "prof_collect")
        out[name] = {"launches": int(n.value), "us_per_launch": round(1e3 * ms.value / max(n.value, 1), 2)}
    image = 4 * 3 * SIZE * SIZE * BATCH
    for name, moved in (("ms_rows_kernel", 2 * image), ("ms_grad_kernel", 4 * image)):      # 2 reads; 2 reads + 2 writes
        k = out[name]
        k["bytes_moved_mb"] = round(moved / 1e6, 2)
        k["tb_per_s"] = round(moved / (k["us_per_launch"] * 1e-6) / 1e12, 3)
    return out


def reduction_rate(b, c, h, w, launches=50):
    from srgan_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    x, y = torch.rand(b, h, w, c, device=dev), torch.rand(b, h, w, c, device=dev)
    e = c * h * w
    nb = lib.srgan_ms_workspace(b, e)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    st = ops._stream()

    def launch():
        _lib.check(lib.srgan_ms_rows(ops._ptr(x), ops._ptr(y), b, e, ops._ptr(ws), nb, st), "ms_rows")

    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        launch()
    z.record()
    torch.cuda.synchronize()
    us = 1e3 * a.elapsed_time(z) / launches
    moved = 2 * 4 * b * e
    return {"shape": [b, c, h, w], "launches": launches, "us_per_launch": round(us, 2), "bytes_read_mb": round(moved / 1e6, 2),
            "tb_per_s": round(moved / (us * 1e-6) / 1e12, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    doc = {"workload": "bench.py trainer: 128x128, bs 32, k 5, fp32", "steps": args.steps, "step": {}}
    for graph in (True, False):
        for on in (False, True, False, True):            # alternated
            key = ("graph" if graph else "eager") + (".on" if on else ".off")
            doc["step"].setdefault(key, []).append(step_times(on, graph, args.steps))
            torch.cuda.empty_cache()
    doc["kernels"] = kernel_times()
    doc["reduction"] = [reduction_rate(BATCH, 3, SIZE, SIZE), reduction_rate(64, 3, 256, 256)]
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
