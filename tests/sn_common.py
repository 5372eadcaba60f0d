"""Shared by the spectral-normalisation tests: the float64 restatement of srgan_amd.spectral and the train-step oracle on top of it.

Restatement, for a conv weight W[O][I][kh][kw] viewed as Wm = W.reshape(O, K):
    one iteration:  v <- Wm^T u / max(|Wm^T u|, eps);  u <- Wm v / max(|Wm v|, eps)
    sigma = u^T Wm v;  W_sn = W / sigma
    gradient of W from G = dL/dW_sn with u, v, sigma held constant:  (G - <G, W_sn> u v^T) / sigma
The contract is "torch.nn.utils.spectral_norm with one training forward per optimiser step" (tests/test_spectral_cpu.py pins the
restatement to it in float64).  Op-level bound: 1e-5 * max|ref| per quantity, the bound this project uses for kernels held to a
float64 restatement (tests/test_criteria_gpu.py); everything else is bit-equality or the bounds of the existing trainer tests."""
import numpy as np
import torch

from oracle import trainer as otrainer

EPS = 1e-12
OP_BOUND = 1e-5

# (O, I, kh, kw) for the (O, K) of the op-level table: O = 1 (patch heads), tier T's smallest layer, O = n_class with a large K,
# odd K (tails, misaligned rows), and shapes with several row slabs and column chunks
OP_SHAPES = [(1, 256, 4, 4), (2, 3, 4, 4), (4, 256, 8, 8), (5, 7, 3, 3), (64, 3, 4, 4), (130, 257, 2, 2), (512, 256, 4, 4)]
OP_OK = [(1, 4096), (2, 48), (4, 16384), (5, 63), (64, 48), (130, 1028), (512, 4096)]


def normalize(x, eps=EPS):
    return x / max(float(x.norm()), eps)


def iterate(Wm, u, v, n=1, eps=EPS):
    """n power iterations in the dtype of the arguments -> (u, v)"""
    for _ in range(n):
        v = normalize(Wm.t() @ u, eps)
        u = normalize(Wm @ v, eps)
    return u, v


def materialize(W, u, v):
    """-> (sigma, W_sn) from the stored (u, v)"""
    Wm = W.reshape(W.shape[0], -1)
    sigma = u @ (Wm @ v)
    return sigma, W / sigma


def refresh(W, u, v, n=1, eps=EPS, do_iterate=True):
    """float64 restatement of one refresh: -> (u, v, sigma, W_sn)"""
    W, u, v = W.double(), u.double(), v.double()
    if do_iterate:
        u, v = iterate(W.reshape(W.shape[0], -1), u, v, n, eps)
    sigma, Wsn = materialize(W, u, v)
    return u, v, sigma, Wsn


def project(G, Wsn, u, v, sigma):
    """gradient of W from the gradient G of W_sn, (u, v, sigma) constant"""
    c = (G * Wsn).sum()
    return (G - c * torch.outer(u, v).reshape(G.shape)) / sigma


def draw_uv(o, k, eps=EPS):
    """u0, v0 as srgan_amd.spectral draws them: float32 normal_(0, 1) from the CPU default generator (u first), normalised"""
    u = torch.nn.functional.normalize(torch.empty(o).normal_(0, 1), dim=0, eps=eps)
    v = torch.nn.functional.normalize(torch.empty(k).normal_(0, 1), dim=0, eps=eps)
    return u, v


def sn_keys(P):
    """the conv weights of a discriminator parameter dict, in the module order of the HIP network"""
    return [k for k, v in P.items() if v.dim() == 4]


class Restated:
    """(weight_orig, u, v, sigma, W_sn) of a set of layers, float64, driven like srgan_amd.spectral drives its table"""

    def __init__(self, weights, n_power_iterations=1, eps=EPS, uv=None):
        """``weights``: {name: float tensor}; draws (u0, v0) per layer in order unless ``uv`` {name: (u, v)} hands them in; one
        iteration follows, as at application"""
        self.n, self.eps = n_power_iterations, eps
        self.W = {k: w.detach().double().clone() for k, w in weights.items()}
        self.u, self.v, self.sigma, self.Wsn = {}, {}, {}, {}
        for k, w in self.W.items():
            u, v = uv[k] if uv is not None else draw_uv(w.shape[0], w[0].numel(), eps)
            self.u[k], self.v[k] = u.double(), v.double()
        self.refresh(n=1)

    def refresh(self, do_iterate=True, n=None):
        for k, w in self.W.items():
            self.u[k], self.v[k], self.sigma[k], self.Wsn[k] = refresh(w, self.u[k], self.v[k], self.n if n is None else n, self.eps,
                                                                       do_iterate)

    def project(self, k, G):
        return project(G.double(), self.Wsn[k], self.u[k], self.v[k], self.sigma[k])


class _SNOptD:
    """optD of the oracle: project -> Adam14 on the originals (and the biases) -> iterate -> rewrite the leaves"""

    def __init__(self, orc, lr):
        self.orc = orc
        self.adam = otrainer.Adam14(list(orc.sn_orig.values()) + [p for k, p in orc.D.items() if k not in orc.sn_orig], lr)

    @property
    def lr(self):
        return self.adam.lr

    @lr.setter
    def lr(self, value):
        self.adam.lr = value

    def step(self):
        orc = self.orc
        for k, orig in orc.sn_orig.items():
            g = orc.D[k].grad
            orig.grad = None if g is None else orc.sn.project(k, g).to(orig.dtype)
        self.adam.step()
        for k, orig in orc.sn_orig.items():
            orc.sn.W[k] = orig.detach().double().clone()
        orc.sn.refresh()
        for k in orc.sn_orig:
            orc.D[k].data.copy_(orc.sn.Wsn[k].to(orc.D[k].dtype))


class SNOracle(otrainer.SRGANOracle):
    """SRGANOracle whose D holds the normalised weights as leaves; ``sn_seed`` seeds the CPU generator right before the (u0, v0)
    draws, as the tests do right before ``spectral.spectral_norm(sg.D)``."""

    def __init__(self, PG, PD, PE, *args, sn_seed=77, n_power_iterations=1, lr=(1e-4, 1e-4, 1e-4), **kw):
        super().__init__(PG, PD, PE, *args, lr=lr, **kw)
        keys = sn_keys(PD)
        self.sn_orig = {k: PD[k].detach().clone().requires_grad_(True) for k in keys}
        torch.manual_seed(sn_seed)
        self.sn = Restated({k: PD[k] for k in keys}, n_power_iterations)
        for k in keys:
            self.D[k].data.copy_(self.sn.Wsn[k].to(self.D[k].dtype))
        self.optD = _SNOptD(self, lr[1])


def np64(t):
    return t.detach().cpu().double()


def ratio(got, ref, bound=OP_BOUND):
    """max|got - ref| / (bound * max|ref|): <= 1 passes"""
    ref = np64(ref) if torch.is_tensor(ref) else torch.as_tensor(ref, dtype=torch.float64)
    got = np64(got) if torch.is_tensor(got) else torch.as_tensor(got, dtype=torch.float64)
    return float((got.reshape(ref.shape) - ref).abs().max()) / (bound * max(float(ref.abs().max()), 1e-300))


# ---- GPU helpers -------------------------------------------------------------------------------------------------------------
def sn_state(D):
    """sigma and the normalised weights of a marked HIP network, cloned (weight_orig / u / v are in its state_dict())"""
    from srgan_amd import spectral
    ctl = spectral.controller(D)
    torch.cuda.synchronize()
    out = {"sigma": ctl.sigma.detach().clone()}
    out.update({f"W_sn.{n}": w.detach().clone() for n, w in zip(ctl.names, ctl.leaves)})
    return out
