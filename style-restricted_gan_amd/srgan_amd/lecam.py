"""LeCam regularisation of the discriminator: Tseng et al. 2021, "Regularizing Generative Adversarial Networks under Limited Data".
An extension, the reference ships no code for it.

D's predictions are pulled towards moving averages of its predictions on the OTHER kind of sample: with ``a_R,s`` / ``a_F,s`` the
anchors (exponential moving averages of the mean of scale s's GAN map over the real / the generated rows of an update),

    R = (1 / S) sum_s [ mean_real phi(o - a_F,s)^2 + mean_fake phi(a_R,s - o)^2 ]

``phi`` the identity (the paper's equation) or ``relu`` (``clamp=True``: the one-sided form of the authors' released code).  The
anchors are constants of the term: no gradient flows through them.  Per discriminator update, in one launch behind the fused loss
(``ops.d_losses(..., lecam=...)`` / ``ops.d_losses_cr(..., lecam=...)``; csrc/lecam.hip): the batch means, the anchors (the first
update sets them to the batch means, later ones ``a <- decay a + (1 - decay) m``; an update with a non-finite mean moves none and
does not count), ``R`` from the updated anchors, and -- once ``updates >= start`` and unless ``weight == 0`` -- the gradient of
``weight * R`` added to the loss gradient.  No extra rows through D and no second backward.

``weight``, ``decay``, ``start``, the count of anchor updates, the anchors, the last ``R`` and whether it was applied live in a
device record: ``set`` between steps keeps a recorded hipGraph valid, and a replayed step crosses the ``start`` boundary by itself.
``clamp`` is structural (a launch argument)."""
from . import ops

__all__ = ["LeCam", "check_settings"]


def check_settings(weight, decay, start, what="LeCam"):
    """-> (float weight, float decay, int start); ValueError for a weight < 0 (or not finite), a decay outside [0, 1), a start < 0
    or not an integer."""
    try:
        w = float(weight)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: weight must be a number >= 0, got {weight!r}") from None
    if not 0.0 <= w < float("inf"):
        raise ValueError(f"{what}: weight must be finite and >= 0, got {weight!r}")
    try:
        d = float(decay)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: decay must be a number in [0, 1), got {decay!r}") from None
    if not 0.0 <= d < 1.0:
        raise ValueError(f"{what}: decay must be in [0, 1), got {decay!r}")
    if isinstance(start, bool) or not isinstance(start, int) and not hasattr(start, "__index__"):
        raise ValueError(f"{what}: start must be an integer >= 0, got {start!r}")
    if int(start) < 0:
        raise ValueError(f"{what}: start must be an integer >= 0, got {start!r}")
    return w, d, int(start)


class LeCam(ops.RecordOwner):
    """The three settings, ``clamp`` and the device record, made at the first use -- never inside a hipGraph capture.
    ``SRGAN_training.enable_lecam`` wires it into the train step; ``loss`` serves a training loop of one's own:

        outs, logits = D.forward_logits(ops.cat_batch([real, fake.detach()]))
        total, parts = lecam.loss(outs, logits, label, B, 1., 0., w_class)
        total.backward()                    # parts = [gan_real, class, gan_fake, errD, R, weight * R or 0]
    """

    layout = ops._lib.LcState

    def __init__(self, weight=0.3, decay=0.99, start=0, clamp=False):
        self.weight, self.decay, self.start = check_settings(weight, decay, start)
        if not isinstance(clamp, (bool, int)) or clamp not in (0, 1):
            raise ValueError(f"LeCam: clamp must be True or False, got {clamp!r}")
        self.clamp = bool(clamp)
        self.state = None

    # -- device side -----------------------------------------------------------------------------------------------------------
    def _ensure(self, device):
        if self.state is None:
            self._make_record(ops.lc_state_new, device, self.weight, self.decay, self.start)
        return self.state

    def arg(self, device):
        """what ``ops.d_losses`` / ``ops.d_losses_cr`` take as ``lecam=``"""
        return self._ensure(device), self.clamp

    def set(self, weight=None, decay=None, start=None):
        """New settings (those given), written into the device record between steps: a recorded step reads them from there."""
        self.weight, self.decay, self.start = check_settings(self.weight if weight is None else weight,
                                                             self.decay if decay is None else decay,
                                                             self.start if start is None else start, "set_lecam")
        if self.state is not None:
            ops.refuse_in_capture("set_lecam inside a hipGraph capture")
            ops.lc_state_set(self.state, self.weight, self.decay, self.start)

    def restore(self, updates, a_real, a_fake, device=None):
        """Resume: write a checkpoint's count of anchor updates and its anchors into the device record, between steps.  A
        regulariser that has not run yet has no record: a count of 0 is what a fresh one starts at, any other makes the record
        here, on ``device``."""
        ops.refuse_in_capture("LeCam: the anchors written inside a hipGraph capture")
        updates = int(updates)
        if updates < 0:
            raise ValueError(f"LeCam: updates must be >= 0, got {updates}")
        if self.state is None:
            if updates == 0:
                return                          # what a fresh record starts at
            if device is None:
                raise ValueError("LeCam: a count of updates without a device for its record")
            self._ensure(device)
        ops.lc_state_restore(self.state, updates, a_real, a_fake)

    def stats(self):
        """The record as a dict (``weight``, ``decay``, ``start``, ``updates``, ``a_real``, ``a_fake``: four per group, ``penalty``,
        ``applied``) plus ``clamp``; SYNCHRONISES."""
        if self.state is None:
            rec = dict(weight=self.weight, decay=self.decay, start=self.start, updates=0, a_real=[0.0] * ops.LC_MAX_SCALES,
                       a_fake=[0.0] * ops.LC_MAX_SCALES, penalty=0.0, applied=0)
        else:
            rec = ops.lc_state_read(self.state)
        rec["clamp"] = self.clamp
        return rec

    def penalty(self):
        """The last unweighted term as a device scalar (a copy; no synchronisation)."""
        return self._record_field("penalty")

    # -- a training loop of one's own ----------------------------------------------------------------------------------------------
    def loss(self, outs, logits, label, rows_first, t_first, t_rest, w_class, gan_kind=ops.CRIT_MSE, class_kind=ops.CRIT_MSE):
        """``ops.d_losses`` with this object's record: -> (errD + weight * R while the term is applied, the six values without a
        gradient).  The first ``rows_first`` rows are the real ones."""
        return ops.d_losses(outs, logits, label, rows_first, t_first, t_rest, w_class, gan_kind, class_kind,
                            lecam=self.arg(outs[0].device))

    # -- hipGraph support, checkpoints -----------------------------------------------------------------------------------------------
    def fingerprint(self):
        """What a recording bakes in: the object, ``clamp`` (a launch argument), the record.  Not the settings: they are device
        state."""
        return (id(self), self.clamp, self._record_ptr())

    def state_dict(self):
        """the settings, clamp, and the record's anchors and count of anchor updates; SYNCHRONISES"""
        st = self.stats()
        return {"weight": self.weight, "decay": self.decay, "start": self.start, "clamp": self.clamp,
                "a_real": [float(v) for v in st["a_real"]], "a_fake": [float(v) for v in st["a_fake"]], "updates": int(st["updates"])}

    def load_state_dict(self, sd, device=None):
        """``clamp`` is part of what a step launches: it must be this object's (``SRGAN_training.load_state_dict`` makes a new
        object otherwise)."""
        if bool(sd["clamp"]) != self.clamp:
            raise ValueError(f"LeCam.load_state_dict: clamp = {sd['clamp']} in the state, {self.clamp} here")
        self.set(sd["weight"], sd["decay"], sd["start"])
        self.restore(sd["updates"], sd["a_real"], sd["a_fake"], device)
