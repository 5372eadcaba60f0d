"""Wall-clock of one save_checkpoint / load_checkpoint of the tier-F trainer (128 x 128, batch 32, k 5, EMA on, graph mode),
next to the replayed step time of the same run."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "style-restricted_gan_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from tests.ema_common import make_trainer  # noqa: E402
from tests.guard_common import batch_of  # noqa: E402

B, K = 32, 5
sg = make_trainer("F", B, K, 2)
sg.enable_ema()
sg.enable_graph()
batches = []
for s in range(4):
    x, label = batch_of(900 + s, B, 128)
    batches.append((x.cuda(), {"source": label["source"].cuda(), "target": label["target"]}))


def steps(n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        sg.train(*batches[i % 4])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


steps(4)
assert sg.graph_active
step_ms = steps(20)
d = tempfile.mkdtemp()
path = os.path.join(d, "ckpt.pt")
out = {"replayed_step_ms": step_ms, "save_ms": [], "state_dict_ms": [], "load_ms": [], "torch_load_ms": []}
for _ in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sd = sg.state_dict()
    t1 = time.perf_counter()
    out["state_dict_ms"].append((t1 - t0) * 1e3)
    del sd
    t0 = time.perf_counter()
    sg.save_checkpoint(path)
    out["save_ms"].append((time.perf_counter() - t0) * 1e3)
out["file_bytes"] = os.path.getsize(path)
for _ in range(3):
    t0 = time.perf_counter()
    sd = torch.load(path, map_location="cpu", weights_only=True)
    out["torch_load_ms"].append((time.perf_counter() - t0) * 1e3)
    del sd
    t0 = time.perf_counter()
    sg.load_checkpoint(path)
    torch.cuda.synchronize()
    out["load_ms"].append((time.perf_counter() - t0) * 1e3)
    first = steps(1)            # eager
    second = steps(1)           # records
    assert sg.graph_active
    out.setdefault("eager_after_load_ms", []).append(first)
    out.setdefault("record_after_load_ms", []).append(second)
out["replayed_step_after_ms"] = steps(20)
os.remove(path)
os.rmdir(d)
print("CKPT_TIMING " + json.dumps(out))
