#!/usr/bin/env python3
"""Cost of the adaptive augmentation probability (SRGAN_training.enable_ada) on the benchmark's workload.

  python scratch/bench_ada.py [--steps 20] [--only-aug] [--out FILE]

bench.py's trainer (128 x 128, bs 32, k 5, fp32) with DiffAugment's full policy, and with enable_ada(p=0.5) on top of it: step time
with eager launches and as a hipGraph replay, each after its own warm-up, fresh trainers alternating in one process (aug, ada, aug,
ada).  ``--only-aug`` times the DiffAugment step alone: the form to run from a checkout of the parent commit in the same call, for
the same-box A/B.  Prints one JSON document."""
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


def step_times(ada, graph, steps, warm=4):
    """ms per step (mean over `steps`, and the median of the per-step device times)"""
    device = torch.device("cuda", 0)
    sg = bench.build_trainer(128, 32, 5, device)
    sg.enable_diffaugment(seed=1)
    if ada:
        sg.enable_ada(p=0.5)
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
    if ada:
        st = sg.ada_stats()
        out.update(p=st["p"], adjustments=st["adjustments"], last_r=st["last_r"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only-aug", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    doc = {"workload": "bench.py trainer: 128x128, bs 32, k 5, fp32, DiffAugment full policy", "steps": args.steps, "step": {}}
    order = (False, False) if args.only_aug else (False, True, False, True)        # alternated: aug, ada, aug, ada
    for graph in (False, True):
        for ada in order:
            key = f"{'replay' if graph else 'eager'}_{'ada' if ada else 'aug'}"
            doc["step"].setdefault(key, []).append(step_times(ada, graph, args.steps))
            torch.cuda.empty_cache()
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
