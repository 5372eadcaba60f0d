#!/usr/bin/env python3
"""Golden fixtures of norm_type="batch" (nn.BatchNorm2d / CBBNorm2d), made by RUNNING the reference in the build container.

Run from the repo root:  python tests/golden/make_golden_batch.py
Same rules as make_golden.py: needs the reference checkout, never runs on the GPU box, writes numbers only.  The reference's
CBBNorm2d cannot load_state_dict (model.py:163), so parameters are filled by COPYING (tests/batch_common.batch_fill, gamma
around 1); buffers start at their defaults, and the eval-mode cases take what the train-mode passes before them left.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as mg                     # noqa: E402  (imports the reference, LegacyAdam, synthetic batches)
from tests.batch_common import batch_buffers, batch_fill, module_inputs, objective_E, objective_G  # noqa: E402

ref_model, ref_util, ref_nb = mg.ref_model, mg.ref_util, mg.ref_nb


def nets_T():
    G = ref_model.SingleGenerator(3, 4, 2, 2, 1, "batch", num_con=12)
    D = ref_model.SingleDiscriminator_solo_multi(3, 4, 2, 4, "batch", 4)
    E = ref_model.Encoder(3, 8, 4, 4, "batch", 4, "cpu")
    return batch_fill(G, 0), mg.load_fill(D, 1), batch_fill(E, 2)


def layout(net):
    return [[k, list(v.shape), str(v.dtype)] for k, v in net.state_dict().items()]


def golden_host():
    out = {"layout": {"G": layout(ref_model.SingleGenerator(3, 4, 2, 2, 1, "batch", num_con=12)),
                      "E": layout(ref_model.Encoder(3, 8, 4, 4, "batch", 4, "cpu")),
                      "E_original": layout(ref_model.Encoder_original(3, 8, 4, 4, "batch", 4, "cpu")),
                      "E_classifier": layout(ref_model.Encoder_classifier(3, 8, 4, 4, "batch", 4))}}
    torch.manual_seed(7)
    nets = dict(G=ref_model.SingleGenerator(3, 8, 2, 2, 2, "batch", num_con=12),
                E=ref_model.Encoder(3, 8, 8, 4, "batch", 4, "cpu"),
                E_original=ref_model.Encoder_original(3, 8, 8, 4, "batch", 4, "cpu"))
    out["init_seed7"] = {n: [[k, float(v.double().sum()), float(v.double().abs().sum())] for k, v in net.state_dict().items()]
                         for n, net in nets.items()}
    # the pretrained-E recipe (05-train cell 22): freeze the Encoder_classifier keys; with the buffers in the state dict the
    # reference's zip of parameters() with state_dict().keys() is misaligned (model.py:465-472)
    E = ref_model.Encoder(3, 8, 4, 4, "batch", 4, "cpu")
    keys = list(ref_model.Encoder_classifier(3, 8, 4, 4, "batch", 4).state_dict().keys())
    E.freeze_melt(keys, "freeze")
    out["freeze_requires_grad"] = [[k, bool(p.requires_grad)] for k, p in E.named_parameters()]
    with open(os.path.join(HERE, "batchnorm_host.json"), "w") as f:
        json.dump(out, f)


def golden_modules():
    """G, E, Encoder_original: two train-mode forward / backward passes (outputs, input and parameter gradients), the buffers
    after them, then one eval-mode forward."""
    out = {}
    xs, c_g, c_e = module_inputs()
    G, _, E = nets_T()
    Eo = batch_fill(ref_model.Encoder_original(3, 8, 4, 4, "batch", 4, "cpu"), 3)
    for name, net in (("G", G), ("E", E), ("Eo", Eo)):
        net.train()
        for i, x in enumerate(xs):
            net.zero_grad()
            xi = x.clone().requires_grad_(True)
            if name == "G":
                y = net(xi, c_g)
                s = objective_G(y)
                out[f"{name}{i}_y_pool8"] = mg.pool8(y)
            else:
                torch.manual_seed(3)
                res = net(xi) if name == "E" else net(xi, c_e)
                s = objective_E(res)
                out[f"{name}{i}_mu"] = res[1].detach().numpy()
                out[f"{name}{i}_logvar"] = res[2].detach().numpy()
            s.backward()
            out[f"{name}{i}_dx_pool8"] = mg.pool8(xi.grad)
            for k, p in net.named_parameters():
                out[f"{name}{i}_grad.{k}"] = p.grad.numpy().copy()
        for k, v in net.state_dict().items():
            if "running" in k or "num_batches" in k:
                out[f"{name}_buf.{k}"] = v.numpy().copy()
        net.eval()
        with torch.no_grad():
            if name == "G":
                out[f"{name}_eval_y_pool8"] = mg.pool8(net(xs[0], c_g))
            else:
                torch.manual_seed(3)
                res = net(xs[0]) if name == "E" else net(xs[0], c_e)
                out[f"{name}_eval_mu"] = res[1].numpy()
                out[f"{name}_eval_logvar"] = res[2].numpy()
    np.savez_compressed(os.path.join(HERE, "modules_batch_T.npz"), **out)


def golden_train(steps=4, batch=4, k=2):
    """SRGAN_training with batch-mode G and E (LBD of make_golden.py: idt_reg > 0, k = 2): losses and num_batches_tracked after
    every step, every parameter and running buffer at the end."""
    G, D, E = nets_T()
    torch.manual_seed(0)
    np.random.seed(0)
    sg = ref_nb.SRGAN_training([G, D, E], [mg.LegacyAdam(G.parameters()), mg.LegacyAdam(D.parameters()),
                                           mg.LegacyAdam(E.parameters())],
                               [nn.MSELoss(), nn.MSELoss()], dict(mg.LBD), k, "cpu", np.eye(4), batch, "mu", 8)
    sg.opt_sche_initialization()
    losses, counts = [], []
    for s in range(steps):
        x, label = mg.synthetic_batch(batch, 128, 4, seed=100 + s)
        errG, errD, errE = sg.train(x, label)
        losses.append([float(errG), float(errD), float(errE)])
        counts.append([int(v) for net in (sg.G, sg.E) for kk, v in net.state_dict().items() if kk.endswith("num_batches_tracked")])
    out = {"losses": np.array(losses, dtype=np.float64), "num_batches_tracked": np.array(counts, dtype=np.int64)}
    for name, net in (("G", sg.G), ("D", sg.D), ("E", sg.E)):
        for kk, v in net.state_dict().items():
            out[f"{name}.{kk}"] = v.numpy().copy()
    np.savez_compressed(os.path.join(HERE, "train_T_b4_k2_batch.npz"), **out)


def golden_inference():
    """get_samples (util_notebook.py:858-949; it puts both networks in eval mode) on batch-mode tier-T networks whose running
    statistics are set (batch_common.batch_buffers): the running statistics stand in for the batch ones."""
    G, _, E = nets_T()
    batch_buffers(G, 4)
    batch_buffers(E, 5)
    torch.manual_seed(3)
    dataset = [(torch.rand(3, 128, 128) * 2 - 1, int(i % 4)) for i in range(3)]
    latent = np.random.RandomState(7).randn(5, 8).astype(np.float32)
    data, label = ref_nb.get_samples(G, E, dataset, 1, latent=latent, classes=(0, 1, 2, 3), ref_label=np.eye(4), ndim=8,
                                     image_type="tensor", batch=2, device="cpu")
    # (the images are regenerated by the test from the same seed; targets as 4x4 means: the file stays small)
    out = {"latent": latent, "source_label": np.asarray(label["source"]), "labels": np.array([d[1] for d in dataset])}
    for c in range(4):
        out[f"target.{c}.pool4"] = torch.nn.functional.avg_pool2d(data["target"][c], 4).numpy()
        out[f"target.{c}.sum"] = np.float64(data["target"][c].double().sum())
        out[f"mu.{c}"] = np.concatenate(label["latent"][c], axis=0)
    np.savez_compressed(os.path.join(HERE, "inference_batch_T.npz"), **out)


if __name__ == "__main__":
    golden_host()
    golden_modules()
    golden_train()
    golden_inference()
    print("batch-mode goldens written")
