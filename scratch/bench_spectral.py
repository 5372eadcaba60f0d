"""Cost of spectral normalisation of D on the headline step (tier F, 128x128, batch 32, k = 5, fp32, graph replay): two trainers
in ONE process -- D plain, D marked with spectral.spectral_norm -- replayed in alternating blocks of STEPS steps, ROUNDS times; per
configuration the median, minimum and maximum block time per step.  Both see the same batches; the marked one trains other
weights (W / sigma), the work per launch is the same.  PROFILE=1: only the marked trainer, STEPS replays after the warm-up (for a
separate `rocprofv3 --kernel-trace --stats -- python scratch/bench_spectral.py` run).  DT=fp32|bf16, B, STEPS, ROUNDS."""
import os, statistics, sys, time
_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, _R); sys.path.insert(0, os.path.join(_R, "style-restricted_gan_amd"))
import torch
import bench
from srgan_amd import ops, spectral
dev = torch.device("cuda", 0)
dt = os.environ.get("DT", "fp32")
ops.set_compute_dtype(dt)
B, STEPS, ROUNDS = int(os.environ.get("B", "32")), int(os.environ.get("STEPS", "10")), int(os.environ.get("ROUNDS", "6"))
profile = os.environ.get("PROFILE") == "1"
batches = []
for s in range(4):
    x, src, tgt = bench.synthetic_batch(B, 128, 4, seed=s)
    batches.append((x.to(dev), {"source": src.to(dev), "target": tgt}))
configs = {}
for name in (("on",) if profile else ("off", "on")):
    torch.manual_seed(0)
    sg = bench.build_trainer(128, B, 5, dev)
    if name == "on":
        spectral.spectral_norm(sg.D)
    sg.enable_graph()
    torch.manual_seed(1)
    for i in range(4):                      # eager, capture, two replays
        sg.train(*batches[i % 4])
    torch.cuda.synchronize()
    assert sg.graph_active
    configs[name] = sg
times = {name: [] for name in configs}
for r in range(1 if profile else ROUNDS):
    for name, sg in configs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(STEPS):
            sg.train(*batches[i % 4])
        torch.cuda.synchronize()
        times[name].append(1e3 * (time.perf_counter() - t0) / STEPS)
base = statistics.median(times["off"]) if "off" in times else None
for name, ts in times.items():
    med = statistics.median(ts)
    rel = f", {100 * (med - base) / base:+.2f} % against off" if base else ""
    print(f"{dt} batch {B}, spectral norm {name}: median {med:.3f} ms per step (min {min(ts):.3f}, max {max(ts):.3f}, "
          f"{len(ts)} blocks of {STEPS}){rel}")
sig = spectral.sigmas(configs["on"].D)
print("sigma after the run:", {k: round(v, 4) for k, v in sig.items()})
