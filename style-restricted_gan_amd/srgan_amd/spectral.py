"""Spectral normalisation of the discriminator's convolution weights (Miyato et al., 2018) on the HIP path.  Extension: the
reference's discriminators take no normalisation.

``spectral_norm(net)`` is ``torch.nn.utils.spectral_norm`` on every conv of ``net`` with ONE power iteration per optimiser
step instead of one per training forward (SN-GAN, Algorithm 1): the trainer sends real and fake images through D as one batch
and re-uses D between updates, so a per-forward count would depend on batching.  For ``Wm = weight_orig.reshape(O, K)``:

    v <- Wm^T u / max(|Wm^T u|, eps);   u <- Wm v / max(|Wm v|, eps);   sigma = u^T Wm v;   weight = weight_orig / sigma

The stored (u, v, sigma, weight) always come from iterating on the current ``weight_orig``: once when the mark is applied, once
after every optimiser step; a loaded state dict re-materialises sigma and ``weight`` from its (weight_orig, u, v) without
iterating, as torch does in eval mode.  ``train()`` / ``eval()`` change nothing.

``weight`` is a persistent fp32 leaf tensor (not a parameter) that the kernels write through its raw pointer, so the packed
operand cache, the gradient sink and every conv path see an ordinary constant weight.  Its gradient G is mapped to the
parameter before the optimiser step, with u, v, sigma held constant as in torch:

    d L / d weight_orig = (G - <G, weight> u v^T) / sigma

One device table covers the whole network (``ops.spectral_refresh_`` / ``ops.spectral_project_``): 5 launches per refresh and
3 per projection whatever the number of layers, capturable into a hipGraph.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .model import _Conv2d, _ConvTranspose2d, _Linear, host_to_device

__all__ = ["spectral_norm", "remove_spectral_norm", "sigmas", "refresh", "project", "zero_grad", "controller", "find"]

_ATTR = "_srgan_spectral"
_marks_epoch = 0          # moves whenever a mark is applied or removed anywhere (callers cache what they found under it)


def marks_epoch():
    return _marks_epoch


def controller(net):
    """The controller ``spectral_norm`` left on ``net`` (a module or a ``dp.DataParallel`` wrapper's module), or None."""
    return net.__dict__.get(_ATTR) if isinstance(net, nn.Module) else None


def find(net):
    """[(module name, controller)] of every marked module at or under ``net``."""
    return [(name, m.__dict__[_ATTR]) for name, m in net.named_modules() if _ATTR in m.__dict__]


class SpectralNorm:
    """Table, workspace and buffers of one marked network."""

    def __init__(self, net, convs, n_power_iterations, eps):
        self.net = net
        self.names = [n for n, _ in convs]
        self.mods = [m for _, m in convs]
        self.n_power_iterations, self.eps = int(n_power_iterations), float(eps)
        self.device = self.mods[0].weight.device
        self.origs, self.leaves = [], []
        self.sigma = torch.zeros(len(convs), dtype=torch.float32, device=self.device)
        for m in self.mods:
            p = m.weight
            o, k = p.shape[0], p[0].numel()
            # u0, v0 as torch draws them (normal_(0, 1), then normalise), from the CPU default generator like every draw here
            u = F.normalize(torch.empty(o).normal_(0, 1), dim=0, eps=self.eps)
            v = F.normalize(torch.empty(k).normal_(0, 1), dim=0, eps=self.eps)
            leaf = torch.empty(p.shape, dtype=torch.float32, device=self.device).requires_grad_(True)
            del m._parameters["weight"]
            m.register_parameter("weight_orig", p)          # the same Parameter object: an optimiser built earlier keeps working
            m.register_buffer("weight_u", host_to_device(u, self.device))
            m.register_buffer("weight_v", host_to_device(v, self.device))
            m.weight = leaf                                 # a plain attribute: not in parameters(), buffers() or state_dict()
            self.origs.append(p)
            self.leaves.append(leaf)
        self.orig_ids = {id(p) for p in self.origs}
        self.gtab = torch.zeros(8 * len(convs), dtype=torch.uint8, device=self.device)
        self._dirty = False
        self._hooks = [m.register_load_state_dict_post_hook(self._loaded) for m in self.mods]
        self._hooks.append(net.register_load_state_dict_post_hook(self._flush_hook))
        self._build()
        self.refresh(iterate=True, n_power_iterations=1)

    def __deepcopy__(self, memo):
        raise NotImplementedError("spectral_norm: a marked network cannot be deep-copied (the device table points at its tensors); "
                                  "copy the plain network and apply spectral_norm to the copy")

    # -- table ------------------------------------------------------------------------------------------------------------------
    def _pointers(self):
        return tuple(t.data_ptr() for m, p, w in zip(self.mods, self.origs, self.leaves) for t in (p, w, m.weight_u, m.weight_v))

    def _build(self):
        rows = []
        for i, (m, p, w) in enumerate(zip(self.mods, self.origs, self.leaves)):
            if m.weight is not w or m._parameters.get("weight_orig") is not p:
                raise RuntimeError("spectral_norm: weight / weight_orig of a marked layer were replaced; remove_spectral_norm first")
            for t in (p, m.weight_u, m.weight_v):
                if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                    raise RuntimeError(f"spectral_norm: weight_orig / weight_u / weight_v must stay contiguous float32 on {self.device}")
            rows.append((p.data_ptr(), w.data_ptr(), m.weight_u.data_ptr(), m.weight_v.data_ptr(), self.sigma.data_ptr() + 4 * i,
                         p.shape[0], p[0].numel()))
        self.table, self.plan, self.ws = ops.spectral_table(rows, self.device)
        self._ptrs = self._pointers()

    def _ensure(self):
        """A ``.to()`` / ``.data =`` that moved a tensor the table points at: rebuild it (never inside a capture)."""
        if self._ptrs != self._pointers():
            ops.refuse_in_capture("spectral_norm: a tensor of a marked layer moved inside a hipGraph capture")
            ops.bump_structure_epoch()
            self._build()
            self._dirty = True
        if self._dirty:
            self.flush()

    # -- the two operations ---------------------------------------------------------------------------------------------------
    def refresh(self, iterate=True, n_power_iterations=None):
        """(u, v,) sigma and ``weight`` from the current ``weight_orig``, on the current stream (capturable)."""
        if not iterate:
            self._dirty = False
        self._ensure()
        n = self.n_power_iterations if n_power_iterations is None else n_power_iterations
        ops.spectral_refresh_(self.table, self.plan, self.ws, iterate, n, self.eps)
        ops.mark_stale(self.leaves)                          # written through raw pointers

    def flush(self):
        """After a state dict was loaded: sigma and ``weight`` from the loaded (weight_orig, u, v) without iterating, and the
        cached packed operands of ``weight`` re-packed (a recorded step replays without looking at the cache)."""
        ops.refuse_in_capture("spectral_norm: a state dict was loaded inside a hipGraph capture")
        self.refresh(iterate=False)
        ops.refresh_packed(self.leaves, force=True)

    def project(self):
        """Before the optimiser step: the gradients of ``weight`` become those of ``weight_orig`` (in place, shared tensors)."""
        self._ensure()
        ptrs = []
        for p, w in zip(self.origs, self.leaves):
            g = w.grad
            if g is not None and not (g.is_contiguous() and g.dtype == torch.float32):
                g = w.grad = g.contiguous().float()
            p.grad = g
            ptrs.append(g.data_ptr() if g is not None else 0)
        if not any(ptrs):
            return
        import struct
        # the gradient pointers change from step to step (the capture-time ones inside a graph): rewritten through kernel arguments
        ops.upload_small(struct.pack(f"{len(ptrs)}Q", *ptrs), self.device, out=self.gtab)
        ops.spectral_project_(self.table, self.plan, self.gtab, self.ws)

    def zero_grad(self):
        """``net.zero_grad()`` does not reach the hidden leaves."""
        for p, w in zip(self.origs, self.leaves):
            w.grad = None
            p.grad = None

    def sigmas(self):
        self._ensure()
        torch.cuda.current_stream(self.device).synchronize()
        return dict(zip(self.names, (float(s) for s in self.sigma.cpu())))

    # -- hooks -----------------------------------------------------------------------------------------------------------------
    def _loaded(self, module, incompatible_keys):
        self._dirty = True

    def _flush_hook(self, module, incompatible_keys):
        if self._dirty:
            self.flush()

    # -- hipGraph support ------------------------------------------------------------------------------------------------------
    def graph_keepalive(self):
        return [self.table, self.ws, self.gtab, self.sigma] + self.leaves

    def fingerprint(self):
        return (id(self), self.table.data_ptr(), self.ws.data_ptr(), self.gtab.data_ptr(), self.sigma.data_ptr(), self.n_power_iterations,
                self.eps, self._pointers(), tuple(w.requires_grad for w in self.leaves))

    def step_params(self, params):
        """The tensors whose packed operands go stale with an optimiser step over ``params``: ``weight`` in place of ``weight_orig``."""
        return [p for p in params if id(p) not in self.orig_ids] + self.leaves

    def remove(self):
        ops.refuse_in_capture("remove_spectral_norm inside a hipGraph capture")
        self._ensure()
        for h in self._hooks:
            h.remove()
        with torch.no_grad():
            for m, p, w in zip(self.mods, self.origs, self.leaves):
                p.copy_(w)                                   # bake W_sn into the same Parameter object, like torch's removal
                p.grad = None
                del m.__dict__["weight"]
                del m._parameters["weight_orig"]
                del m._buffers["weight_u"], m._buffers["weight_v"]
                m._non_persistent_buffers_set.discard("weight_u")
                m._non_persistent_buffers_set.discard("weight_v")
                rest = [(k, m._parameters.pop(k)) for k in list(m._parameters)]
                m.register_parameter("weight", p)            # first again, as nn.Conv2d registers it: the state_dict() order
                for k, q in rest:
                    m._parameters[k] = q
        del self.net.__dict__[_ATTR]
        global _marks_epoch
        _marks_epoch += 1
        ops.invalidate_packed(self.leaves)


def spectral_norm(net, n_power_iterations=1, eps=1e-12):
    """Mark every ``_Conv2d`` under ``net`` (see the module docstring); returns ``net``.  ``state_dict()`` keys, shapes and dtypes
    are those of ``torch.nn.utils.spectral_norm`` on the same convs: ``weight_orig``, ``weight_u``, ``weight_v`` and no ``weight``."""
    if not isinstance(net, nn.Module):
        raise TypeError("spectral_norm: expected a module (unwrap a dp.DataParallel wrapper with dp.unwrap)")
    if int(n_power_iterations) < 1:
        raise ValueError("spectral_norm: n_power_iterations must be >= 1")
    if not float(eps) > 0.0:
        raise ValueError("spectral_norm: eps must be > 0")
    ops.refuse_in_capture("spectral_norm: applied inside a hipGraph capture -- apply it between steps")
    if find(net) or any(hasattr(m, "weight_orig") for m in net.modules()):
        raise RuntimeError("spectral_norm: this network (or a part of it) is marked already; remove_spectral_norm first")
    bad = [n for n, m in net.named_modules() if isinstance(m, (_ConvTranspose2d, _Linear, nn.ConvTranspose2d, nn.Linear))]
    if bad:
        raise NotImplementedError(f"spectral_norm: {bad[0]} is a transposed convolution / linear layer; only _Conv2d weights are "
                                  "normalised here (apply it to a network of convolutions, such as the discriminators)")
    convs = [(n, m) for n, m in net.named_modules() if isinstance(m, _Conv2d)]
    if not convs:
        raise RuntimeError("spectral_norm: no _Conv2d under this network")
    for n, m in convs:
        w = m.weight
        if not w.is_cuda:
            raise RuntimeError(f"spectral_norm: {n}.weight is on {w.device}; move the network to the GPU first -- the normalised "
                               "weight is a plain tensor attribute that .to() would not move, and the update is a HIP kernel (no CPU "
                               "fallback)")
        if w.dtype != torch.float32 or not w.is_contiguous():
            raise RuntimeError(f"spectral_norm: {n}.weight must be contiguous float32")
    global _marks_epoch
    _marks_epoch += 1
    net.__dict__[_ATTR] = SpectralNorm(net, convs, n_power_iterations, eps)
    return net


def _need(net, what):
    ctl = controller(net)
    if ctl is None:
        raise RuntimeError(f"{what}: this network is not marked (spectral_norm)")
    return ctl


def remove_spectral_norm(net):
    """Bake ``weight_orig / sigma`` back into a ``weight`` parameter (the same Parameter object) and drop the mark; the network's
    forward is bit-identical to the one before.  Returns ``net``."""
    _need(net, "remove_spectral_norm").remove()
    return net


def sigmas(net):
    """{layer name: sigma}; synchronises."""
    return _need(net, "sigmas").sigmas()


def refresh(net, iterate=True):
    """For users who write ``weight_orig`` by hand: one power iteration (``iterate``) or none, then sigma and ``weight``."""
    _need(net, "refresh").refresh(iterate=iterate)


def project(net):
    """For users who write their own loop: map the gradients of the normalised weights to ``weight_orig.grad`` (call it after
    ``backward()`` and before the optimiser step, then ``refresh(net)`` after the step)."""
    _need(net, "project").project()


def zero_grad(net):
    """Clear the gradients of the normalised weights and of ``weight_orig`` (``net.zero_grad()`` misses the former)."""
    _need(net, "zero_grad").zero_grad()
