"""Fused Adam on the HIP path with the formula of the reference's pinned torch==1.4.0
(``optim.Adam(lr, betas=(0.5, 0.999))`` built at util_notebook.py:498-507; formula SURVEY.md F.6).

One difference in the arithmetic: the betas enter as the float32 numbers of the device record, and the kernels derive ``1.f - b``
and the bias corrections ``1 - b^t`` from ``b = float32(beta)``; torch 1.4 takes ``float32(1 - beta)`` and ``1 - beta^t`` from the
Python doubles.  On the update this is a relative difference of at most ``c = |float32(beta) - beta| / (1 - beta)`` per beta --
1.29e-5 for ``beta2 = 0.999``, 0 for ``beta1 = 0.5`` -- and ``tests/test_adam_kernels_gpu.py::test_distance_to_torch14_stays_inside_c``
holds it there (derivation in ``tests/adam_common.py``).

Parameters are updated through raw device pointers: the autograd version counters are NOT bumped,
which is what lets phase 2 of ``update_GandE`` back-propagate a graph recorded before the step
(SURVEY.md Appendix C-1).  It is a ``torch.optim.Optimizer`` so ``ExponentialLR`` can drive ``lr``.

The step counter and the hyper-parameters of a parameter cohort live in a small DEVICE record
(``ops.adam_state_new``): ``step()`` launches "t += 1; derive the bias corrections; update" without
baking t or lr into the launch, so a train step captured into a hipGraph advances the optimiser on every
replay.  The host keeps ``state[p]["step"]`` in step for ``state_dict()`` / resume (``advance_host`` after a
replay) and pushes ``lr`` changes made by a scheduler to the device record (``sync_device``).

Gradient guard (``enable_grad_guard``; off by default, extension): every ``step()`` first reduces ``S = sum g^2`` over every
parameter that has a gradient in that call (all groups and cohorts) on the device.  ``S`` not finite -- a NaN, an Inf, squares that
overflow -- skips the step: no parameter or moment is written (GradScaler's "found inf").  With ``max_norm`` set the update runs
on ``g * min(1, max_norm / (sqrt(S) + 1e-6))`` (``clip_grad_norm_``, norm type 2; the gradient tensors are not modified).  The
decision, the scale and three cumulative counters live in a 32-byte device record, so a replayed hipGraph decides, skips, clips
and counts without the host.  A skipped step still counts as a step -- ``t`` and ``state[p]["step"]`` advance -- which keeps the
host mirrors exact without a device read; the price is a bias correction one step ahead after each skip.  A guard that does not
trigger changes no bit of the result (``g * 1.0f == g``).  The guard is not part of ``state_dict()``.
"""
import struct

import torch

from . import ops


class _Cohort:
    """Parameters of one group that share a step count: one pointer table, one device-side state record."""
    __slots__ = ("state", "table", "steps", "lr", "n", "max_numel")

    def __init__(self):
        self.state = self.table = None
        self.steps = -1            # completed steps the device record stands at
        self.lr = None
        self.n = self.max_numel = 0


class _Guard:
    """Device record, reduce table and partials workspace of one optimiser's gradient guard."""
    __slots__ = ("state", "max_norm", "table", "rows", "ws", "chunks")

    def __init__(self, device, max_norm):
        self.state = ops.grad_guard_state_new(device, max_norm)
        self.max_norm = max_norm
        self.table = self.ws = None         # sized by the first guarded step (and re-sized if a later one needs more)
        self.rows = self.chunks = 0


def _check_max_norm(max_norm):
    if max_norm is not None and not float(max_norm) > 0.0:        # (NaN compares false)
        raise ValueError(f"grad guard: max_norm must be None (no clipping) or a number > 0, got {max_norm!r}")
    return None if max_norm is None else float(max_norm)


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        if lr < 0.0 or eps < 0.0 or not (0.0 <= betas[0] < 1.0) or not (0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self._cohorts = {}
        self._guard = None

    def _cohort(self, gi, params, group, steps_done):
        key = (gi,) + tuple(id(p) for p in params)
        co = self._cohorts.get(key)
        capturing = ops.capturing()
        if co is None or co.steps != steps_done:
            # first use, or the host-side count moved (load_state_dict / resume): (re)seed the device record
            if capturing:
                raise RuntimeError("srgan_amd.optim.Adam: an optimiser cohort first appears (or was re-seeded) inside a hipGraph "
                                   "capture -- run one eager train step with the same parameter set first")
            if co is not None:
                ops.bump_structure_epoch()       # a captured step points at the record being replaced
            if co is None:
                co = self._cohorts[key] = _Cohort()
                co.table = torch.empty(40 * len(params), dtype=torch.uint8, device=params[0].device)
            b1, b2 = group["betas"]
            co.state = ops.adam_state_new(params[0].device, group["lr"], b1, b2, group["eps"], steps_done)
            co.lr, co.steps = group["lr"], steps_done
            co.n, co.max_numel = len(params), max(p.numel() for p in params)
        if co.lr != group["lr"]:
            if capturing:
                raise RuntimeError("srgan_amd.optim.Adam: lr changed inside a hipGraph capture")
            ops.adam_state_set_lr(co.state, group["lr"])
            co.lr = group["lr"]
        return co

    def _collect(self, group):
        """completed step count -> [(p, g, m, v)] of one group: one multi-tensor launch per count; advances state[p]["step"]"""
        batches = {}
        for p in group["params"]:
            if p.grad is None:       # torch 1.4 skips parameters that received no gradient
                continue
            st = self.state[p]
            if len(st) == 0:
                st["step"] = 0
                st["exp_avg"] = torch.zeros_like(p.data, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p.data, memory_format=torch.contiguous_format)
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            if not p.data.is_contiguous():
                raise RuntimeError("srgan_amd.optim.Adam needs contiguous parameters")
            batches.setdefault(int(st["step"]), []).append((p, g, st["exp_avg"], st["exp_avg_sq"]))
            st["step"] += 1
        return batches

    def _update(self, gi, group, batches, guard):
        kept = []
        for steps_done, items in batches.items():
            params = [it[0] for it in items]
            co = self._cohort(gi, params, group, steps_done)
            rows = []
            for p, g, m, v in items:
                rows.extend((p.data.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()))
            # the gradient pointers change from step to step (and are the capture-time ones inside a graph): the table is
            # rewritten by every step, in stream order, through kernel arguments
            ops.upload_small(struct.pack(f"{len(rows)}q", *rows), params[0].device, out=co.table)
            if guard is None:
                ops.adam_multi_dev_(co.table, co.n, co.max_numel, co.state)
            else:
                ops.adam_multi_dev_guard_(co.table, co.n, co.max_numel, co.state, guard.state)
            co.steps = steps_done + 1
            kept = items
        ops.mark_stale(group["params"])                  # parameters were written through raw pointers
        return kept

    def _reduce(self, guard, grads):
        """The guard's two launches over every gradient of this call; (re)sizes its table and workspace outside a capture."""
        device = grads[0].device
        rows = sum(1 for g in grads if g.numel())
        chunks = sum(-(-g.numel() // ops.GRAD_GUARD_CHUNK) for g in grads)
        if guard.table is None or rows > guard.rows or chunks > guard.chunks:
            ops.refuse_in_capture("srgan_amd.optim.Adam: the gradient guard's table / workspace first appear (or grow) inside a "
                                  "hipGraph capture -- run one eager train step with the guard enabled first")
            if guard.table is not None:
                ops.bump_structure_epoch()       # a captured step points at the buffers being replaced
            guard.rows, guard.chunks = max(rows, guard.rows), max(chunks, guard.chunks)
            guard.table = torch.empty(24 * guard.rows, dtype=torch.uint8, device=device)
            guard.ws = torch.empty(ops.grad_guard_workspace_bytes(guard.chunks), dtype=torch.uint8, device=device)
        table, n_records, total_chunks = ops.grad_guard_table(grads, device, out=guard.table)
        ops.grad_guard_reduce_(table, n_records, total_chunks, guard.ws, guard.state)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        guard = self._guard
        if guard is None:
            for gi, group in enumerate(self.param_groups):
                kept = self._update(gi, group, self._collect(group), None)
                if kept:
                    self._keep_alive = kept                  # until the next step: the launch reads them asynchronously
            return loss
        # guarded: ONE reduction over the gradients of all groups and cohorts of this call decides for all of them, so the
        # gradients are collected first; then per cohort the tick and the guarded update, as above
        collected = [self._collect(group) for group in self.param_groups]
        items = [it for batches in collected for its in batches.values() for it in its]
        if items:
            self._reduce(guard, [it[1] for it in items])
            self._keep_alive = items
        for gi, (group, batches) in enumerate(zip(self.param_groups, collected)):
            self._update(gi, group, batches, guard)
        return loss

    # -- resume -----------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        """``torch.optim.Optimizer.load_state_dict`` plus what the raw-pointer step needs of the result: ``state[p]["step"]`` is
        an ``int`` again (a file may hand back a 0-dim tensor), the moments are contiguous float32 on their parameter's device
        (torch casts them to the parameter's dtype and keeps the strides it was given), ``betas`` a tuple.  The cohorts are
        forgotten, so the next ``step()`` seeds fresh device records at the loaded counts with the loaded hyper-parameters (a
        recording that points at the old ones is dropped by its owner: ``ops.bump_structure_epoch``).  Between steps only.  A
        parameter without saved state stays without state; the gradient guard is not part of the dict and stays as it is."""
        ops.refuse_in_capture("srgan_amd.optim.Adam: load_state_dict inside a hipGraph capture")
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            group["betas"] = tuple(float(b) for b in group["betas"])
            for p in group["params"]:
                st = self.state.get(p)
                if not st:
                    continue
                st["step"] = int(st["step"])
                for key in ("exp_avg", "exp_avg_sq"):
                    m = st[key]
                    if m.shape != p.shape:
                        raise ValueError(f"srgan_amd.optim.Adam.load_state_dict: {key} of shape {tuple(m.shape)} for a parameter of "
                                         f"shape {tuple(p.shape)}")
                    if m.device != p.device or m.dtype != torch.float32 or not m.is_contiguous():
                        st[key] = m.to(device=p.device, dtype=torch.float32).contiguous()
        if self._cohorts:
            ops.bump_structure_epoch()           # a captured step points at the records being dropped
            self._cohorts = {}
        self._keep_alive = None

    # -- gradient guard -------------------------------------------------------------------------------------------------
    def enable_grad_guard(self, max_norm=None):
        """Skip steps whose gradients are not finite and, with ``max_norm``, clip by the global 2-norm -- on the device, see the
        module docstring.  Between steps only; a hipGraph recording of the step made before is dropped by its owner
        (``grad_guard_fingerprint``).  Enabling again re-creates the record (counters at zero)."""
        max_norm = _check_max_norm(max_norm)
        ops.refuse_in_capture("srgan_amd.optim.Adam: gradient guard enabled inside a hipGraph capture -- enable it between steps")
        params = [p for g in self.param_groups for p in g["params"]]
        if not params or params[0].device.type != "cuda":
            raise RuntimeError("srgan_amd.optim.Adam: the gradient guard is a HIP kernel; the parameters are not on the GPU "
                               "(no CPU fallback)")
        if self._guard is not None:
            ops.bump_structure_epoch()
        self._guard = _Guard(params[0].device, max_norm)
        return self

    def disable_grad_guard(self):
        if self._guard is not None and ops.capturing():
            raise RuntimeError("srgan_amd.optim.Adam: gradient guard disabled inside a hipGraph capture")
        self._guard = None

    def _need_guard(self, what):
        if self._guard is None:
            raise RuntimeError(f"{what}: the gradient guard is off (enable_grad_guard)")
        return self._guard

    def set_max_norm(self, max_norm):
        """Write a new clipping threshold (``None``: no clipping) into the device record, between steps; a recorded step reads it
        from there and stays valid."""
        guard = self._need_guard("set_max_norm")
        max_norm = _check_max_norm(max_norm)
        ops.refuse_in_capture("srgan_amd.optim.Adam: max_norm changed inside a hipGraph capture")
        ops.grad_guard_state_set_max_norm(guard.state, max_norm)
        guard.max_norm = max_norm

    def set_grad_guard_counters(self, steps, skipped, clipped):
        """Resume: write a checkpoint's cumulative counters into the device record, between steps; the threshold and the last
        step's decision stay."""
        guard = self._need_guard("set_grad_guard_counters")
        ops.refuse_in_capture("srgan_amd.optim.Adam: guard counters written inside a hipGraph capture")
        ops.grad_guard_state_set_counters(guard.state, steps, skipped, clipped)

    def grad_guard_stats(self):
        """{"max_norm", "norm", "scale", "skip", "steps", "skipped", "clipped"} read from the device record: norm / scale / skip
        of the last ``step()``, cumulative counters since ``enable_grad_guard``.  SYNCHRONISES the current stream -- the only
        point at which the host looks at the guard."""
        return ops.grad_guard_state_read(self._need_guard("grad_guard_stats").state)

    def grad_guard_fingerprint(self):
        """What a recording of ``step()`` bakes in of the guard: whether it is on, and which record (the threshold is device
        state and stays out)."""
        g = self._guard
        return None if g is None else (id(g), g.state.data_ptr())

    # -- hipGraph support --------------------------------------------------------------------------------------------
    def sync_device(self):
        """Push a scheduler's lr change to the device records (call between steps, outside any capture)."""
        for key, co in self._cohorts.items():
            lr = self.param_groups[key[0]]["lr"]
            if co.lr != lr:
                ops.adam_state_set_lr(co.state, lr)
                co.lr = lr

    def graph_keepalive(self):
        keep = [t for co in self._cohorts.values() for t in (co.state, co.table)]
        if self._guard is not None:
            keep += [t for t in (self._guard.state, self._guard.table, self._guard.ws) if t is not None]
        return keep

    def host_counters(self):
        """Snapshot of the host-side step counters (per-parameter ``state[p]["step"]`` and the cohorts')."""
        return ({id(p): self.state[p]["step"] for g in self.param_groups for p in g["params"] if p in self.state and len(self.state[p])},
                {key: co.steps for key, co in self._cohorts.items()})

    def restore_host_counters(self, snap):
        per_param, per_cohort = snap
        for g in self.param_groups:
            for p in g["params"]:
                if id(p) in per_param:
                    self.state[p]["step"] = per_param[id(p)]
        for key, co in self._cohorts.items():
            if key in per_cohort:
                co.steps = per_cohort[key]

    def counters_since(self, snap):
        """What moved between ``snap`` (``host_counters()``) and now -- i.e. what ONE run of the step recorded in between does to
        the host-side counters: per parameter and per cohort (a cohort or parameter that did not take part stays out)."""
        per_param, per_cohort = snap
        now_p, now_c = self.host_counters()
        return ({pid: n - per_param.get(pid, 0) for pid, n in now_p.items() if n != per_param.get(pid, 0)},
                {key: n - per_cohort[key] for key, n in now_c.items() if key in per_cohort and n != per_cohort[key]})

    def advance_host(self, delta):
        """A replayed graph ran its optimiser steps on the device: move the host-side counters by what the recording moved
        (``counters_since``) -- exactly the parameters and cohorts that stepped while it was recorded."""
        per_param, per_cohort = delta
        for group in self.param_groups:
            for p in group["params"]:
                d = per_param.get(id(p))
                if d:
                    self.state[p]["step"] += d
        for key, d in per_cohort.items():
            self._cohorts[key].steps += d
