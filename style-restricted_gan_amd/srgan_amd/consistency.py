"""Balanced consistency regularisation (bCR) of the discriminator: Zhang et al. 2020, "Consistency Regularization for GANs", in the
balanced form -- on real AND on generated samples -- of Zhao et al. 2020, "Improved Consistency Regularization for GANs".  An
extension, the reference ships no code for it.

D is trained to give an image and a label-preserving transform ``T`` of it the same score.  ``T`` is an x-flip followed by an integer
translation with zeros shifted in; it is applied in the discriminator update only (D's inputs are detached there), so -- unlike an
always-on augmentation -- it cannot leak into the generator's output.  Per penalised update, with B the batch size and P = 2 B:

    rows D reads      [ real (B) | fake (B) | T(real) (B) | T(fake) (B) ]: the front P rows are what D reads anyway (after every
                      augmentation stage that is on), row n + P is the partner of row n           (``ops.cr_pairs``, one launch)
    score             m_s(r) = the patch mean of scale s's GAN map at row r (the per-sample score R1 uses; no class heads)
    cr_real           (1 / S) sum_s (1 / B) sum_{n < B} (m_s(n) - m_s(n + P))^2;  cr_fake: the same over n in [B, 2 B)
    back-propagated   errD + every * (lambda_real * cr_real + lambda_fake * cr_fake)          (``ops.d_losses_cr``, one launch)

Lazy regularisation as for R1: update i of a step's k is penalised iff ``i % every == 0``, with the weights scaled by ``every``.
The weights, ``every``, the two terms of the last penalised update and the count of penalised updates live in a device record, so
``set_weights`` between steps keeps a recorded hipGraph valid."""
import torch

from . import ops
from .augment import _Stage, _window

__all__ = ["ConsistencyPairs", "BalancedCR", "CR_GROUPS", "schedule"]

CR_GROUPS = {"flip": ops.CR_FLIP, "translation": ops.CR_TRANSLATION}


def schedule(k, every):
    """Which of a step's k discriminator updates are penalised: update i iff i % every == 0 (static per step)."""
    return [i % every == 0 for i in range(k)]


class ConsistencyPairs(_Stage):
    """The transform ``T`` of the consistency pairs, applied by ``ops.cr_pairs`` (csrc/consistency.hip).  One float32 row per image:

        [fx, ty, tx, 0, 0, 0, 0, 0]      fx in {0, 1}, Bernoulli(1/2): mirror the columns                             (flip)
                                         ty in [-Sy, Sy], tx in [-Sx, Sx], S = int(size * translation + 0.5)          (translation)

    ``T(x)[i, j] = xf[i - ty, j - tx]`` inside the image, else 0, with ``xf[i, j] = x[i, W - 1 - j]`` if fx else ``x[i, j]``.  A
    group that is off draws nothing and is the identity.  Unlike the stages of ``SRGAN_training._stages()`` this one is not applied
    to everything D reads -- it makes the partner rows of a penalised update -- and the adaptive probability never gates it."""

    groups, n_groups, section, settings = CR_GROUPS, 2, "bcr", ("translation",)

    def __init__(self, policy="flip,translation", translation=0.125, seed=None):
        super().__init__(policy, seed, translation=translation)

    @staticmethod
    def _check_settings(translation):
        try:
            t = float(translation)
        except (TypeError, ValueError):
            t = float("nan")
        if not 0.0 <= t < float("inf"):
            raise ValueError(f"ConsistencyPairs: translation = {translation!r} (a ratio >= 0, finite)")
        return (t,)

    def draw(self, n, h, w):
        """One CPU float32 table [n, 8] for n images of h x w; groups that are off get identity values and draw nothing."""
        g, flags = self.generator, self.flags
        t = torch.zeros(n, ops.CR_ROW, dtype=torch.float32)
        if flags & ops.CR_FLIP:
            t[:, 0] = (torch.rand(n, generator=g, dtype=torch.float32) < 0.5).to(torch.float32)
        if flags & ops.CR_TRANSLATION:
            sy, sx = _window(h, self.translation), _window(w, self.translation)
            t[:, 1] = torch.randint(-sy, sy + 1, (n,), generator=g).to(torch.float32)
            t[:, 2] = torch.randint(-sx, sx + 1, (n,), generator=g).to(torch.float32)
        return t

    def apply(self, x, table, gated=False):
        """``table``: device float32 [n, 8] -> the 2n rows ``[x | T(x)]``; forward only.  Never gated."""
        if gated:
            raise ValueError("ConsistencyPairs: the consistency transform is not gated by the adaptive probability")
        return ops.cr_pairs([x], table, self.flags)

    def __call__(self, x):
        """Draw, copy to the device, apply (also with an empty policy: the partner rows are then copies)."""
        n, _, h, w = x.shape
        table = self.draw_fn(n, h, w).to(dtype=torch.float32).pin_memory().to(x.device, non_blocking=True)
        return self.apply(x, table)


def check_weights(lambda_real, lambda_fake, every, what="BalancedCR"):
    """-> (float lambda_real, float lambda_fake, int every); ValueError for a weight < 0 (or not finite), every < 1 or not an integer."""
    out = []
    for name, v in (("lambda_real", lambda_real), ("lambda_fake", lambda_fake)):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: {name} must be a number >= 0, got {v!r}") from None
        if not 0.0 <= f < float("inf"):
            raise ValueError(f"{what}: {name} must be finite and >= 0, got {v!r}")
        out.append(f)
    if isinstance(every, bool) or not isinstance(every, int) and not hasattr(every, "__index__"):
        raise ValueError(f"{what}: every must be an integer >= 1, got {every!r}")
    if int(every) < 1:
        raise ValueError(f"{what}: every must be an integer >= 1, got {every!r}")
    return out[0], out[1], int(every)


class BalancedCR(ops.RecordOwner):
    """The two weights, ``every``, the stage that draws ``T`` (``self.stage``) and the device record, made at the first use -- never
    inside a hipGraph capture.  ``SRGAN_training.enable_bcr`` wires it into the train step; ``pairs`` / ``loss`` serve a training loop
    of one's own:

        rows = bcr.pairs(ops.cat_batch([real, fake.detach()]))        # [4 B, 3, H, W]
        outs, logits = D.forward_logits(rows)
        total, parts = bcr.loss(outs, logits, label, B, 1., 0., w_class)
        total.backward()                                              # parts = [gan_real, class, gan_fake, errD, cr_real, cr_fake]
    """

    def __init__(self, lambda_real=10.0, lambda_fake=10.0, every=1, policy="flip,translation", translation=0.125, seed=None):
        self.lambda_real, self.lambda_fake, self.every = check_weights(lambda_real, lambda_fake, every)
        self.stage = ConsistencyPairs(policy, translation, seed)
        self.state = None

    # -- device side -----------------------------------------------------------------------------------------------------------
    def _ensure(self, device):
        if self.state is None:
            self._make_record(ops.cr_state_new, device, self.lambda_real, self.lambda_fake, self.every)
        return self.state

    def set_weights(self, lambda_real, lambda_fake):
        """New weights (>= 0), written into the device record between steps: a recorded step reads them from there."""
        self.lambda_real, self.lambda_fake, _ = check_weights(lambda_real, lambda_fake, self.every, "set_bcr_weights")
        if self.state is not None:
            ops.refuse_in_capture("set_bcr_weights inside a hipGraph capture")
            ops.cr_state_set(self.state, self.lambda_real, self.lambda_fake, self.every)

    def set_updates(self, updates, device=None):
        """Resume: write a checkpoint's count of penalised updates into the device record, between steps.  A regulariser that has
        not run yet has no record: a count of 0 is what a fresh one starts at, any other makes the record here, on ``device``."""
        ops.refuse_in_capture("BalancedCR: updates written inside a hipGraph capture")
        updates = int(updates)
        if updates < 0:
            raise ValueError(f"BalancedCR: updates must be >= 0, got {updates}")
        if self.state is None:
            if updates == 0:
                return                          # what a fresh record starts at
            if device is None:
                raise ValueError("BalancedCR: a count of updates without a device for its record")
            self._ensure(device)
        ops.cr_state_set_updates(self.state, updates)

    def stats(self):
        """The record as a dict (``lambda_real``, ``lambda_fake``, ``every``, ``cr_real``, ``cr_fake``, ``updates``); SYNCHRONISES."""
        if self.state is None:
            return dict(lambda_real=self.lambda_real, lambda_fake=self.lambda_fake, every=self.every, cr_real=0.0, cr_fake=0.0,
                        updates=0)
        return ops.cr_state_read(self.state)

    # -- a training loop of one's own ----------------------------------------------------------------------------------------------
    def pairs(self, x):
        """``x[n, 3, H, W]`` (detached) -> ``[x | T(x)]`` of 2n rows with a fresh draw of the stage's generator"""
        return self.stage(x.detach())

    def loss(self, outs, logits, label, rows_first, t_first, t_rest, w_class, gan_kind=ops.CRIT_MSE, class_kind=ops.CRIT_MSE,
             pairs_first=None):
        """``ops.d_losses_cr`` with this object's record: -> (errD + every * (lambda_real cr_first + lambda_fake cr_rest), the six
        values without a gradient)."""
        return ops.d_losses_cr(outs, logits, label, rows_first, t_first, t_rest, w_class, self._ensure(outs[0].device), gan_kind,
                               class_kind, pairs_first)

    # -- hipGraph support, checkpoints -----------------------------------------------------------------------------------------------
    def fingerprint(self):
        """What a recording bakes in: the object, ``every`` (the schedule and the launches), the policy, the settings and the draw
        source of the stage, the record.  Not the weights: they are device state."""
        return (id(self), self.every, self.stage.fingerprint(), self._record_ptr())

    def state_dict(self):
        """weights, every, the stage's policy / translation / generator and the record's count of penalised updates; SYNCHRONISES"""
        return {"lambda_real": self.lambda_real, "lambda_fake": self.lambda_fake, "every": self.every, **self.stage.state_dict(),
                "updates": int(self.stats()["updates"])}

    def load_state_dict(self, sd, device=None):
        """``every`` is part of what a step launches: it must be this object's (``SRGAN_training.load_state_dict`` makes a new
        object otherwise)."""
        if int(sd["every"]) != self.every:
            raise ValueError(f"BalancedCR.load_state_dict: every = {sd['every']} in the state, {self.every} here")
        self.stage.load_state_dict(sd)
        self.set_weights(sd["lambda_real"], sd["lambda_fake"])
        self.set_updates(sd["updates"], device)
