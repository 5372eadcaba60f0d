"""Cost of the device-side gradient guard on the headline step (tier F, 128x128, batch 32, k = 5, fp32, graph replay): three
trainers in ONE process -- guard off, on with max_norm=None, on with a max_norm nothing reaches -- replayed in alternating blocks of
STEPS steps, ROUNDS times; per configuration the median, minimum and maximum block time per step.  The three start from the same
weights and see the same batches, and an idle guard changes no bit, so they do the same work.  DT=fp32|bf16, B, STEPS, ROUNDS."""
import os, statistics, sys, time
_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, _R); sys.path.insert(0, os.path.join(_R, "style-restricted_gan_amd"))
import torch
import bench
from srgan_amd import ops
dev = torch.device("cuda", 0)
dt = os.environ.get("DT", "fp32")
ops.set_compute_dtype(dt)
B, STEPS, ROUNDS = int(os.environ.get("B", "32")), int(os.environ.get("STEPS", "10")), int(os.environ.get("ROUNDS", "6"))
batches = []
for s in range(4):
    x, src, tgt = bench.synthetic_batch(B, 128, 4, seed=s)
    batches.append((x.to(dev), {"source": src.to(dev), "target": tgt}))
configs = {}
for name, guard in (("off", None), ("on, max_norm=None", (None,)), ("on, max_norm=1e30", (1e30,))):
    torch.manual_seed(0)
    sg = bench.build_trainer(128, B, 5, dev)
    if guard is not None:
        sg.enable_grad_guard(*guard)
    sg.enable_graph()
    torch.manual_seed(1)
    for i in range(4):                      # eager, capture, two replays
        sg.train(*batches[i % 4])
    torch.cuda.synchronize()
    assert sg.graph_active
    configs[name] = sg
times = {name: [] for name in configs}
for r in range(ROUNDS):
    for name, sg in configs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(STEPS):
            sg.train(*batches[i % 4])
        torch.cuda.synchronize()
        times[name].append(1e3 * (time.perf_counter() - t0) / STEPS)
base = statistics.median(times["off"])
for name, ts in times.items():
    med = statistics.median(ts)
    print(f"{dt} batch {B}, guard {name}: median {med:.3f} ms per step (min {min(ts):.3f}, max {max(ts):.3f}, {ROUNDS} blocks of {STEPS}),"
          f" {100 * (med - base) / base:+.2f} % against off")
for name, sg in configs.items():
    if name != "off":
        print(name, {n: (st["steps"], st["skipped"], st["clipped"], round(st["norm"], 4)) for n, st in sg.grad_guard_stats().items()})
