#!/usr/bin/env python3
"""Cost of LeCam regularisation (SRGAN_training.enable_lecam) on the benchmark's workload, and of its one kernel.

  python scratch/bench_lecam.py [--steps 20] [--out FILE] [--kernel-only]

Part 1: bench.py's trainer (tier F, 128 x 128, bs 32, k 5, fp32) in graph mode -- ms per step with the feature off (the plain step)
and on; a fresh trainer per configuration after its own warm-up, the two configurations alternating (off, on, off, on, off, on) in one
process.  Part 2: the maps of one discriminator update of that trainer, then `srgan_lecam` and -- the yardstick -- `srgan_d_losses_crit`
on them, each timed the same way: HIP events around LAUNCHES back-to-back launches on one stream, five rounds, the median per launch.
Neither kernel has a launch-timer slot.  Prints one JSON document."""
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
        sg.enable_lecam()
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
        st = sg.lecam_stats()
        out.update(updates=st["updates"], penalty_last=st["penalty"], applied=st["applied"])
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


def kernel_times():
    from srgan_amd import _lib, ops
    lib = _lib.load()
    sg, device = make(False, False)
    torch.manual_seed(1000)
    batch = batches_for(device, 1)[0]
    sg.train(*batch)
    with torch.no_grad():
        d_in = ops.cat_batch([sg.source_image, sg.target_image.detach()])
        outs, _ = sg.D.forward_logits(d_in)
    o = [t.detach().contiguous() if not ops.is_nhwc_dense(t) else t.detach() for t in outs]
    rows, S = o[0].shape[0], len(o)
    d_o = [torch.zeros_like(t) for t in o]
    vals = torch.zeros(8, dtype=torch.float32, device=device)
    state = ops.lc_state_new(device, 0.3, 0.99, 0)
    arr = ctypes.c_void_p * S
    po, pg = arr(*[t.data_ptr() for t in o]), arr(*[t.data_ptr() for t in d_o])
    per = (ctypes.c_longlong * S)(*[t.numel() // rows for t in o])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def d_losses():
        _lib.check(lib.srgan_d_losses_crit(po, per, None, S, rows, rows // 2, 0, None, 1.0, 0.0, 1.0, 0, 0, ctypes.c_void_p(vals.data_ptr()),
                                           pg, None, stream), "d_losses")

    def lecam():
        _lib.check(lib.srgan_lecam(po, per, S, rows, rows, rows // 2, 0, ctypes.c_void_p(vals.data_ptr() + 12),
                                   ctypes.c_void_p(vals.data_ptr() + 16), pg, ctypes.c_void_p(state.data_ptr()), stream), "lecam")

    out = {"maps": [list(t.shape) for t in o], "floats": int(sum(t.numel() for t in o)), "launches_per_round": LAUNCHES}
    out["d_losses_kernel_us"] = _per_launch_us(d_losses)
    out["lecam_kernel_us"] = _per_launch_us(lecam)
    out["d_losses_kernel_us_again"] = _per_launch_us(d_losses)
    out["ratio"] = round(out["lecam_kernel_us"] / out["d_losses_kernel_us"], 2)
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
    for on in (() if args.kernel_only else (False, True, False, True, False, True)):           # alternated
        doc["step"].setdefault("on" if on else "off", []).append(step_times(on, args.steps))
        torch.cuda.empty_cache()
    doc["kernel"] = kernel_times()
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
