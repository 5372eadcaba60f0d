"""Adaptive discriminator augmentation (Karras et al., 2020, "Training Generative Adversarial Networks with Limited Data",
sections 2.2 and 3) on top of the augmentation stages of ``srgan_amd.augment`` -- an extension, the reference augments nothing.

Each group of a stage is applied to a sample with probability p instead of always; augmentations applied with p < 1 do not leak
into the generated images, and the right p follows the overfitting heuristic ``r = E[sign(D(real) - thr)]``: every ``interval``
discriminator updates p moves by ``step`` towards keeping ``r`` at ``target``.  A recorded step is replayed without the host, so
everything lives in a device record (``csrc/ada.hip``): p, the settings, the heuristic's counters.  Per discriminator read, for
every stage that is on (DiffAugment, then the geometric stage)

    host      table [n, 8] from the stage's ``draw_fn``, then uniforms [n, n_groups] from its ``gate_fn`` (the stage's own
              generator), joined into rows of 16 floats (the stage's ``join_rows``)
    device    ``ops.ada_gate``      rows + the record's p -> table [n, 8] whose slot 7 is the per-sample skip mask
              the stage's ``apply(..., gated=True)``

and then, in discriminator updates only

              ``ops.ada_observe_``  counts over the real rows of D's maps; every ``interval``-th call moves p

``step = B * interval / (kimg * 1000)``: p can travel from 0 to 1 in ``kimg`` thousand real images.
``SRGAN_training.enable_ada`` wires it into the train step."""
import math

import numpy as np

from . import _lib, ops
from .augment import DiffAugment

__all__ = ["AdaptiveP", "join_rows", "threshold"]


def _number(v, name, what):
    if isinstance(v, bool):
        raise ValueError(f"{what}: {name} must be a number, got {v!r}")
    try:
        return float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} must be a number, got {v!r}") from None


def check_target(target, what="AdaptiveP"):
    t = _number(target, "target", what)
    if not math.isfinite(t):
        raise ValueError(f"{what}: target must be finite, got {target!r}")
    return t


def check_interval(interval, what="AdaptiveP"):
    if isinstance(interval, bool) or not isinstance(interval, int) and not hasattr(interval, "__index__"):
        raise ValueError(f"{what}: interval must be an integer >= 1, got {interval!r}")
    i = int(interval)
    if i < 1:
        raise ValueError(f"{what}: interval must be an integer >= 1, got {interval!r}")
    return i


def check_p(p, p_max, what="AdaptiveP"):
    p, p_max = _number(p, "p", what), _number(p_max, "p_max", what)
    if not 0.0 <= p <= p_max <= 1.0:
        raise ValueError(f"{what}: 0 <= p <= p_max <= 1 expected, got p = {p!r}, p_max = {p_max!r}")
    return p, p_max


def threshold(gan_kind):
    """Where ``sign`` changes on D's raw maps: 0.5 for nn.MSELoss against the targets 1 / 0, 0 for nn.BCEWithLogitsLoss."""
    return 0.5 if gan_kind == ops.CRIT_MSE else 0.0


join_rows = DiffAugment.join_rows     # DiffAugment's rows; every stage has its own ``join_rows(table, uniforms)``


class AdaptiveP(ops.RecordOwner):
    """The settings and the device record of the controller.  ``target``: the value of ``r`` to hold (0.6 in the paper);
    ``interval``: observed discriminator updates per adjustment; ``kimg``: thousands of real images in which p can travel from 0 to
    1; ``p``: where it starts; ``p_max``: its ceiling -- 0.8 is the bound below which translation- and cutout-like transforms stay
    non-leaking in the paper.  The record is made at the first eager use, never inside a hipGraph capture."""

    layout = _lib.AdaState

    def __init__(self, target=0.6, interval=4, kimg=500.0, p=0.0, p_max=0.8):
        self.target = check_target(target)
        self.interval = check_interval(interval)
        k = _number(kimg, "kimg", "AdaptiveP")
        if not (k > 0.0 and math.isfinite(k)):
            raise ValueError(f"AdaptiveP: kimg must be finite and > 0, got {kimg!r}")
        self.kimg = k
        self.p, self.p_max = check_p(p, p_max)     # p: where a fresh record starts (the live value is device state: stats())
        self.state = None
        self._n = None                             # the batch size the record's step was derived for
        self._interval = None                      # the interval the record holds

    def step_size(self, n):
        """what p moves by per adjustment at batch size ``n``, as the float32 the record holds"""
        return float(np.float32(n * self.interval / (self.kimg * 1000.0)))

    # -- device side -----------------------------------------------------------------------------------------------------------
    def _ensure(self, device, n):
        n = int(n)
        if self.state is None:
            self._make_record(ops.ada_state_new, device, self.p, self.target, self.step_size(n), self.p_max, self.interval)
            self._n, self._interval = n, self.interval
        elif self._n != n or self._interval != self.interval:
            ops.refuse_in_capture("AdaptiveP: the batch size changed inside a hipGraph capture; run one eager step first")
            ops.ada_state_set(self.state, self.target, self.step_size(n), self.p_max, self.interval)
            self._n, self._interval = n, self.interval

    def _write(self, p=None):
        if self.state is not None:
            ops.ada_state_set(self.state, self.target, self.step_size(self._n), self.p_max, self.interval, p)
            self._interval = self.interval

    def set_p(self, p):
        """A new p (0 <= p <= p_max), written into the device record between steps: a recorded step reads it from there."""
        ops.refuse_in_capture("set_ada_p inside a hipGraph capture")
        self.p, _ = check_p(p, self.p_max, "set_ada_p")
        self._write(self.p)

    def set_target(self, target):
        """A new target, written into the device record between steps: a recorded step reads it from there."""
        ops.refuse_in_capture("set_ada_target inside a hipGraph capture")
        self.target = check_target(target, "set_ada_target")
        self._write()

    def set_interval(self, interval):
        """A new interval: part of the fingerprint, a recording made before is dropped.  The record follows at the next step."""
        self.interval = check_interval(interval, "AdaptiveP.set_interval")

    def gate(self, rows, n_groups):
        """rows [n, 16] of a stage with ``n_groups`` gated groups, on the device -> the gated table [n, 8] (one launch)"""
        return ops.ada_gate(rows, self.state, n_groups)

    def observe(self, outs, rows_first, thr):
        ops.ada_observe_(outs, rows_first, thr, self.state)

    def p_tensor(self):
        """p as a device scalar (a copy of the record's field; no synchronisation)"""
        return self._record_field("p")

    def stats(self):
        """The record as a dict (``p``, ``target``, ``step``, ``p_max``, ``interval``, ``seen``, ``n_pos``, ``n_neg``, ``n_total``,
        ``adjustments``, ``last_r``); SYNCHRONISES."""
        if self.state is None:
            return dict(p=self.p, target=self.target, step=None, p_max=self.p_max, interval=self.interval, seen=0, n_pos=0, n_neg=0,
                        n_total=0, adjustments=0, last_r=0.0)
        return ops.ada_state_read(self.state)

    # -- checkpoints -----------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """The settings and the whole record (``n``: the batch size its step was derived for, None before the first use);
        SYNCHRONISES."""
        st = self.stats()
        return {"target": float(self.target), "interval": int(self.interval), "kimg": float(self.kimg), "p_max": float(self.p_max),
                "p": float(st["p"]), "seen": int(st["seen"]), "n_pos": int(st["n_pos"]), "n_neg": int(st["n_neg"]),
                "n_total": int(st["n_total"]), "adjustments": int(st["adjustments"]), "last_r": float(st["last_r"]),
                "n": None if self._n is None else int(self._n)}

    def load_state_dict(self, sd, device=None):
        """Restore ``state_dict()``, between steps.  The record is written in place; a controller that has not run yet makes it
        here for the saved batch size on ``device`` (the step re-derives ``step`` should its batch differ).  Without a record and
        without a saved batch size only the settings and the starting p are taken: the counters of such a checkpoint are zero."""
        ops.refuse_in_capture("AdaptiveP: state loaded inside a hipGraph capture")
        target, interval = check_target(sd["target"]), check_interval(sd["interval"])
        kimg = float(sd["kimg"])
        if not (kimg > 0.0 and math.isfinite(kimg)):
            raise ValueError(f"AdaptiveP: kimg must be finite and > 0, got {sd['kimg']!r}")
        p, p_max = check_p(sd["p"], sd["p_max"])
        counters = [int(sd[k]) for k in ("seen", "n_pos", "n_neg", "n_total", "adjustments")]
        n = sd.get("n")
        fresh = self.state is None and (n is None or device is None)
        if fresh and any(counters):
            raise ValueError("AdaptiveP: counters without the batch size of their record (n)")
        self.target, self.interval, self.kimg, self.p, self.p_max = target, interval, kimg, p, p_max
        if fresh:
            return
        if self.state is None:
            self._ensure(device, int(n))
        elif n is not None:
            self._n = int(n)
        self._write(p)
        ops.ada_state_set_counters(self.state, *counters, float(sd["last_r"]))

    # -- hipGraph support -------------------------------------------------------------------------------------------------------
    def fingerprint(self):
        """What a recording bakes in: the object, the record, ``interval`` and the batch size.  Not p, target or step: they are
        device state."""
        return (id(self), self._record_ptr(), self.interval, self._n)
