#!/usr/bin/env python3
"""Cost of the structural-similarity term (SRGAN_training.enable_ssim) on the benchmark's workload, and of its three kernels.

  python scratch/bench_ssim.py [--steps 20] [--out FILE] [--kernel-only]

Part 1: bench.py's trainer (tier F, 128 x 128, bs 32, k 5, fp32) in graph mode -- ms per step with the feature off (the plain step),
on the cycle reconstruction, and on both reconstructions; a fresh trainer per configuration after its own warm-up, the
configurations alternating in one process.  Part 2: two images of the step's shape [32, 3, 128, 128], then the map launch (with the
three coefficient maps of a one-sided gradient and without), the finish and the gradient launch, each timed the same way: HIP events
around LAUNCHES back-to-back launches on one stream, five rounds, the median per launch, and the bytes each has to move (computed
from the shapes) over that time.  None of the kernels has a launch-timer slot.  Prints one JSON document."""
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
LAUNCHES = 200


def make(on, graph):
    device = torch.device("cuda", 0)
    sg = bench.build_trainer(SIZE, BATCH, K, device)
    if on:
        sg.enable_ssim(weight=1.0, on=on)
    if graph:
        sg.enable_graph()
    return sg, device


def batches_for(device, n):
    out = []
    for s in range(n):
        x, src, tgt = bench.synthetic_batch(BATCH, SIZE, 4, seed=10_000 + s)
        out.append((x.to(device), {"source": src.to(device), "target": tgt}))
    return out


def step_times(on, steps, warm=4):
    """ms per step in graph mode: host clock around `steps` replays ending in a synchronise, and the median of the per-step device
    times"""
    sg, device = make(on, True)
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
    if on:
        st = sg.ssim_stats()
        out.update(updates=st["updates"], term_last=st["term"])
    return out


def _per_launch_us(launch):
    """the median over five rounds of (HIP events around LAUNCHES launches) / LAUNCHES"""
    for _ in range(10):
        launch()
    torch.cuda.synchronize()
    rounds = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(LAUNCHES):
            launch()
        b.record()
        torch.cuda.synchronize()
        rounds.append(1e3 * a.elapsed_time(b) / LAUNCHES)
    return round(sorted(rounds)[2], 2)


def kernel_times(window=11):
    from srgan_amd import _lib, ops
    lib = _lib.load()
    device = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    x = ops.to_nhwc((torch.rand(BATCH, 3, SIZE, SIZE, generator=g) * 2 - 1).to(device))
    y = ops.to_nhwc((x + 0.1 * torch.randn(BATCH, 3, SIZE, SIZE, generator=g).to(device)).clamp(-1, 1))
    dy = torch.empty_like(y)
    n, c, h, w = x.shape
    taps = (ctypes.c_float * window)(*ops.ssim_taps(window, 1.5))
    state = ops.ss_state_new(device, 1.0, 4e-4, 3.6e-3)
    nb = lib.srgan_ssim_workspace(n, c, h, w, window, 0, 1)
    ws = torch.empty(nb, dtype=torch.uint8, device=device)
    vals = torch.empty(2, dtype=torch.float32, device=device)
    values = torch.empty(n, dtype=torch.float32, device=device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def map_(want):
        _lib.check(lib.srgan_ssim_map(P(x), P(y), n, c, h, w, window, taps, P(state), 0.0, 0.0, 0, want, P(ws), nb, stream), "ssim_map")

    def finish():
        _lib.check(lib.srgan_ssim_finish(P(ws), nb, n, c, h, w, window, P(state), P(vals), P(values), stream), "ssim_finish")

    def grad():
        _lib.check(lib.srgan_ssim_grad(P(x), P(y), n, c, h, w, window, taps, P(ws), nb, P(state), None, None, P(dy), stream), "ssim_grad")

    image = 4.0 * n * c * h * w
    maps = 4.0 * n * c * (h - window + 1) * (w - window + 1)
    out = {"shape": [n, c, h, w], "window": window, "image_bytes": image, "map_bytes": maps, "launches_per_round": LAUNCHES}
    for name, fn, nbytes in (("map_no_gradient", lambda: map_(0), 2 * image), ("map_with_3_maps", lambda: map_(1), 2 * image + 3 * maps),
                             ("finish", finish, 0.0), ("gradient_dy", grad, 3 * maps + 3 * image)):
        us = _per_launch_us(fn)
        out[name] = {"us": us, "bytes": nbytes, "TB_per_s": round(nbytes / us / 1e6, 3)}
    # the same bytes through torch's copy kernel, as this box's yardstick
    src, dst = torch.empty(int(image) // 4 * 4, device=device), torch.empty(int(image) // 4 * 4, device=device)
    us = _per_launch_us(lambda: dst.copy_(src))
    out["copy_of_4_images"] = {"us": us, "bytes": 8 * image, "TB_per_s": round(8 * image / us / 1e6, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true", help="part 2 alone")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    doc = {"workload": "bench.py trainer: 128x128, bs 32, k 5, fp32, graph mode", "steps": args.steps, "step": {}}
    order = () if args.kernel_only else ((), ("cycle",), ("cycle", "idt"), (), ("cycle",), ("cycle", "idt"), (), ("cycle",))
    for on in order:                                           # alternated
        doc["step"].setdefault("+".join(on) if on else "off", []).append(step_times(on, args.steps))
        torch.cuda.empty_cache()
    doc["kernel"] = kernel_times()
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
