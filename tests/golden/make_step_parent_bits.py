"""Record what ``SRGAN_training.train`` computes, bit for bit, in the five configurations of tests/step_bits_common.py, run
EAGERLY: tests/golden/train_step_parent_bits.npz, which tests/test_train_gpu.py::test_train_step_keeps_the_parent_bits holds
later commits to (eagerly, and for two of the cases replayed from a hipGraph).  Per case the file holds the float32 matrix of the
returned losses and the sorted ``loss_terms`` of every step, and one JSON document with a sha256 digest per tensor (the state
dicts of G / D / E, the Adam moments, and where they are on the EMA twins and the spectral u / v / sigma), ``r1_stats()``,
``grad_guard_stats()`` and -- cases ``plain`` and ``all_on`` -- the launch count per kernel of the last step, taken with the
library's launch timer.  Digests, not tensors: about 50 kB.

Run on the MI355X from the repository root, against a built tree of the commit to record:

    python tests/golden/make_step_parent_bits.py <hash of that commit> [out.npz]

The committed file was recorded from the parent of the commit that moved graph mode into ``srgan_amd/step_graph.py``, with
``git diff HEAD -- style-restricted_gan_amd`` empty, before the first edit to ``trainer.py``: the stored ``parent_commit`` is that
parent, and the refactored step reproduces the file unchanged.  When a later change moves bits ON PURPOSE (another summation
order, a kernel fused into the step, a launch added), check that commit out before the change -- again with no difference
under ``style-restricted_gan_amd`` -- build it, run this script with its hash and commit the new file together with the change;
the launch counts in it say what the change did to the step's launch sequence."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "style-restricted_gan_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(commit, out):
    from tests.step_bits_common import CASES, run_case
    rec = {"parent_commit": np.array(commit)}
    for case in CASES:
        losses, meta = run_case(case)
        rec[case + "/losses"] = losses
        rec[case + "/meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
        print(case, losses.shape, losses[-1, :3], len(meta["digests"]), "digests",
              sum(meta["launches"].values()) if meta["launches"] else "-", "launches", flush=True)
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    if len(sys.argv) < 2 or len(sys.argv[1]) != 40:
        sys.exit("usage: make_step_parent_bits.py <40-digit hash of the recorded commit> [out.npz]")
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "train_step_parent_bits.npz"))
