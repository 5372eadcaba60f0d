"""Shared pieces of the norm_type="batch" fixtures (tests/golden/make_golden_batch.py) and their tests: the parameter fill by
copying (the reference's CBBNorm2d cannot load_state_dict), the module inputs and the scalar objectives."""
import re

import numpy as np
import torch

from oracle import params

# nn.BatchNorm2d weights of the generator's up path and the encoder blocks: gamma around 1, as fill_array does for the
# central-biasing layers ("cn1.weight", "cnorms.i.weight", ...)
_BN_WEIGHT = re.compile(r"(^|\.)(norm[12]|up_norms\.\d+)\.weight$")


def batch_fill_array(key, shape, seed):
    a = params.fill_array(key, tuple(shape), seed)
    if _BN_WEIGHT.search(key):
        a = (1.0 + 2.5 * a.astype(np.float64)).astype(np.float32)
    return a


def batch_fill(net, seed):
    """Copy the deterministic fill into every PARAMETER (buffers keep their defaults)."""
    with torch.no_grad():
        for k, p in net.named_parameters():
            p.copy_(torch.from_numpy(batch_fill_array(k, p.shape, seed)))
    return net


def batch_buffers(net, seed):
    """Deterministic running statistics (eval-mode cases that start from a trained state): running_mean small, running_var
    around 1; num_batches_tracked stays."""
    with torch.no_grad():
        for k, v in net.named_buffers():
            if k.endswith("running_mean"):
                v.copy_(torch.from_numpy(0.2 * params.fill_array(k, tuple(v.shape), seed)))
            elif k.endswith("running_var"):
                v.copy_(torch.from_numpy(1.0 + 2.0 * abs(params.fill_array(k, tuple(v.shape), seed))))
    return net


def module_inputs():
    """Two input batches (two train-mode passes), the generator's condition and Encoder_original's code."""
    gens = [torch.Generator().manual_seed(s) for s in (11, 12)]
    xs = [torch.rand(3, 3, 128, 128, generator=g) * 2 - 1 for g in gens]
    g = torch.Generator().manual_seed(5)
    z = torch.randn(3, 8, generator=g)
    onehot = torch.eye(4)[torch.tensor([1, 3, 0])]
    c_g = torch.cat([onehot, z], 1)
    c_e = torch.randn(3, 4, generator=g)
    return xs, c_g, c_e


def objective_G(y):
    wy = torch.linspace(-1, 1, y.numel(), device=y.device).view(y.shape)
    return (y * wy).sum()


def objective_E(res):
    mu, logvar = res[1], res[2]
    s = (mu * torch.linspace(0.5, 1.5, mu.numel(), device=mu.device).view(mu.shape)).sum() + (logvar ** 2).sum() + res[0].sum()
    return s + res[3].sum() if len(res) > 3 else s
