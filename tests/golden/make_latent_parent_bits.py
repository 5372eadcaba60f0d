"""Record what ``latent_losses_kernel`` returns, bit for bit, at the golden (32, 8) inputs with the train step's weights
(10, 100, 100): tests/golden/latent_losses_parent_bits.npz, which test_small_kernels_gpu.py holds later builds to.

Run on the MI355X against the build to record, from the repository root:

    SRGAN_HIP_LIB=<libsrgan_hip.so of that build> python tests/golden/make_latent_parent_bits.py [out.npz]

The committed file was recorded from the build of the commit before the zero-weight selects went into the kernel."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "style-restricted_gan_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(out):
    from srgan_amd import ops
    gold = np.load(os.path.join(HERE, "losses.npz"))
    tgt = torch.from_numpy(gold["hist_target_seed0"]).cuda()
    rec = {}
    for name in ("randn1234", "sin"):
        mu = torch.from_numpy(gold[f"{name}_mu"]).cuda().requires_grad_(True)
        total, parts, corr = ops.latent_losses(mu, 32, tgt, 10.0, 100.0, 100.0)
        (dmu,) = torch.autograd.grad(total, mu)
        rec[f"{name}_vals"] = torch.cat([parts, total.detach().reshape(1)]).cpu().numpy()
        rec[f"{name}_dmu"] = dmu.cpu().numpy()
        rec[f"{name}_corr"] = corr.cpu().numpy()
    np.savez(out, **rec)
    print("wrote", out, {k: v.shape for k, v in rec.items()})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "latent_losses_parent_bits.npz"))
