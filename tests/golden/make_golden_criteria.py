#!/usr/bin/env python3
"""Reference trajectories with criteria other than nn.MSELoss (tests/test_criteria_gpu.py).

Run from the repo root:  python tests/golden/make_golden_criteria.py
Like make_golden.py (which it imports for the networks, the torch-1.4 Adam, the synthetic batches and the loss weights) it
RUNS the imported reference on the CPU and writes only numbers.  ``run_train`` / ``run_singlegan`` are make_golden's, restated
with a criterion argument; the MSE / MSE run must reproduce train_T_b4_k2.npz exactly before anything is written.

  train_T_b4_k2_bce.npz       nn.BCEWithLogitsLoss + nn.BCELoss: losses, hist_target, final parameters
  train_T_b4_k2_mixed.npz     the two mixed pairs: losses only
  singlegan_T_b8_k1_bce.npz   config 1 with the BCE criteria: losses and final parameters.  The parameters are stored as their
                              distance from the deterministic fill in float32 bit patterns (int32, lossless: a few lr is a few
                              thousand units in the last place), which compresses below the size of train_T_b4_k2.npz where the
                              raw values do not; tests/criteria_common.py::load_singlegan_params adds the same fill back.
"""
import os
import sys
import zipfile

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402

from tests.criteria_common import SG_BASE, SG_FILL  # noqa: E402  (make_golden put the repo root on sys.path)


def run_train(criterion, tier="T", batch=4, k=2, steps=3, seed=0, size=128, params=True):
    G, D, E = mg.build_nets(tier)
    torch.manual_seed(seed)
    np.random.seed(seed)
    sg = mg.ref_nb.SRGAN_training([G, D, E], [mg.LegacyAdam(G.parameters()), mg.LegacyAdam(D.parameters()), mg.LegacyAdam(E.parameters())],
                                  criterion, dict(mg.LBD), k, "cpu", np.eye(4), batch, "mu", 8)
    sg.opt_sche_initialization()
    losses = []
    for s in range(steps):
        x, label = mg.synthetic_batch(batch, size, 4, seed=100 + s)
        errG, errD, errE = sg.train(x, label)
        losses.append([float(errG), float(errD), float(errE)])
    out = {"losses": np.array(losses, dtype=np.float64), "hist_target": sg.hi.target.detach().numpy()}
    if params:
        for name, net in (("G", sg.G), ("D", sg.D), ("E", sg.E)):
            for k_, v in net.state_dict().items():
                out[f"{name}.{k_}"] = v.detach().float().numpy()
    return out


def run_singlegan(criterion, k=1, steps=3, seed=0, lbd=SG_BASE, batch=8):
    G = mg.load_fill(mg.ref_model.SingleGenerator(3, 4, 2, 2, 1, "instance", num_con=2 + 8), SG_FILL["G"])
    D = [mg.load_fill(mg.ref_model.SingleDiscriminator_original_multi(3, 4, 2, 4, "instance"), SG_FILL["D%d" % i]) for i in range(2)]
    E = mg.load_fill(mg.ref_model.Encoder_original(3, 8, 4, 4, "instance", 2, "cpu"), SG_FILL["E"])
    torch.manual_seed(seed)
    np.random.seed(seed)
    sg = mg.ref_nb.SingleGAN_training([G, D, E], [mg.LegacyAdam(G.parameters()), None, mg.LegacyAdam(E.parameters())],
                                      criterion, dict(lbd), k, "cpu", np.eye(2), 8, (0, 1), batch, "latent", False)
    sg.opt_sche_initialization()
    losses = []
    for s in range(steps):
        x, label = mg.synthetic_batch(batch, 64, 2, seed=200 + s)
        errG, errD, errE = sg.train(x, label)
        losses.append([float(errG), float(errD), float(errE)])
    out = {"losses": np.array(losses, dtype=np.float64)}
    for name, net in (("G", sg.G), ("D0", sg.D[0]), ("D1", sg.D[1]), ("E", sg.E)):
        for k_, v in net.state_dict().items():
            final = v.detach().float().numpy()
            fill = mg.oparams.fill_array(k_, tuple(v.shape), SG_FILL[name]).astype(np.float32)
            steps_ = final.view(np.int32) - fill.view(np.int32)            # (wraps for the few elements that changed sign)
            assert np.array_equal((fill.view(np.int32) + steps_).view(np.float32), final), (name, k_)
            out[f"{name}_ulps.{k_}"] = steps_
    return out


def main():
    torch.set_num_threads(8)
    limit = os.path.getsize(os.path.join(HERE, "train_T_b4_k2.npz"))
    base = np.load(os.path.join(HERE, "train_T_b4_k2.npz"))
    check = run_train([nn.MSELoss(), nn.MSELoss()], params=False)
    assert np.array_equal(check["losses"], base["losses"]), (check["losses"], base["losses"])
    written = []

    def save(name, **arrays):
        # an .npz as np.savez_compressed writes it, at zlib's highest level (the default level leaves the BCE / BCE fixture a
        # few bytes above train_T_b4_k2.npz)
        path = os.path.join(HERE, name)
        with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
            for key, value in arrays.items():
                with zf.open(key + ".npy", "w") as fh:
                    np.lib.format.write_array(fh, np.asanyarray(value), allow_pickle=False)
        assert os.path.getsize(path) <= limit, (name, os.path.getsize(path), limit)
        written.append((name, os.path.getsize(path)))

    bce = run_train([nn.BCEWithLogitsLoss(), nn.BCELoss()])
    save("train_T_b4_k2_bce.npz", **bce)
    mixed = {"bcelogits_mse": run_train([nn.BCEWithLogitsLoss(), nn.MSELoss()], params=False)["losses"],
             "mse_bce": run_train([nn.MSELoss(), nn.BCELoss()], params=False)["losses"]}
    save("train_T_b4_k2_mixed.npz", **mixed)
    save("singlegan_T_b8_k1_bce.npz", **run_singlegan([nn.BCEWithLogitsLoss(), nn.BCELoss()]))
    print("first-step errD: bce/bce %.8f  bcelogits/mse %.8f  mse/bce %.8f" % (bce["losses"][0, 1], mixed["bcelogits_mse"][0, 1],
                                                                              mixed["mse_bce"][0, 1]))
    print("written:", written, "limit", limit)


if __name__ == "__main__":
    main()
