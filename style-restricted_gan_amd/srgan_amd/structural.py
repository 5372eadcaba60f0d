"""Structural similarity (Wang et al. 2004, "Image quality assessment: from error visibility to structural similarity") as a
reconstruction loss beside L1 (Zhao et al. 2017, "Loss functions for image restoration with neural networks") and as a metric.  An
extension, the reference ships no code for it.

For images ``x``, ``y`` [N, C, H, W] (fp32, C <= 3) and a Gaussian window of ``window`` taps per axis (odd, 3..11; ``sigma``), at the
VALID positions only -- ``(H - window + 1) x (W - window + 1)`` per plane, no padding -- with ``E[.]`` the windowed mean:

    mu_x = E[x], mu_y = E[y], s_x = E[x^2] - mu_x^2, s_y = E[y^2] - mu_y^2, s_xy = E[xy] - mu_x mu_y        (population form, no clamp)
    SSIM = (2 mu_x mu_y + C1)(2 s_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(s_x + s_y + C2)),  C1 = (k1 L)^2, C2 = (k2 L)^2, L = data_range

The value of a sample is the mean over its positions and channels, the term ``1 - mean over the samples``; ``weight * term`` is
minimised.  The window's weights are computed and normalised in double on the host and rounded to fp32.  The kernels
(``csrc/ssim.hip``, ``ops.ssim``) take every windowed moment of values shifted by one pivot per plane, so that the variances are
differences of numbers of the size of the local contrast.  ``weight``, ``C1``, ``C2``, the last term and an
update counter live in a device record, so ``set_weight`` between steps keeps a recorded hipGraph valid; ``window``, ``sigma``,
``k1``, ``k2`` and ``data_range`` are structural: another value is another object."""
import math

from . import ops

__all__ = ["SSIM", "check_settings"]


def _number(name, v, what, low_open=False):
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} must be a number, got {v!r}") from None
    if isinstance(v, bool) or not (0.0 < f if low_open else 0.0 <= f) or not f < float("inf"):
        raise ValueError(f"{what}: {name} must be finite and {'> 0' if low_open else '>= 0'}, got {v!r}")
    return f


def check_settings(weight, window, sigma, k1, k2, data_range, what="SSIM"):
    """-> (float weight, int window, float sigma, float k1, float k2, float data_range); ValueError for a weight < 0, a window that
    is not an odd integer in [3, 11], sigma <= 0, k1 < 0, k2 <= 0, data_range <= 0, or any not finite."""
    if isinstance(window, bool) or not isinstance(window, int) or window % 2 == 0 \
            or not ops.SSIM_MIN_WINDOW <= window <= ops.SSIM_MAX_WINDOW:
        raise ValueError(f"{what}: window must be an odd integer in [{ops.SSIM_MIN_WINDOW}, {ops.SSIM_MAX_WINDOW}], got {window!r}")
    return (_number("weight", weight, what), window, _number("sigma", sigma, what, low_open=True), _number("k1", k1, what),
            _number("k2", k2, what, low_open=True), _number("data_range", data_range, what, low_open=True))


class SSIM(ops.RecordOwner):
    """The settings, the tap table and the device record, made at the first use -- never inside a hipGraph capture.
    ``SRGAN_training.enable_ssim`` wires it into the train step; for a loop of one's own:

        weighted, term = ssim.loss(source, reconstruction)      # add ``weighted`` to the generator's loss
        values = ssim.value(a, b)                               # per-sample SSIM, no gradient, the record untouched
    """

    layout = ops._lib.SsState

    def __init__(self, weight=1.0, window=11, sigma=1.5, k1=0.01, k2=0.03, data_range=2.0):
        self.weight, self.window, self.sigma, self.k1, self.k2, self.data_range = check_settings(weight, window, sigma, k1, k2,
                                                                                                 data_range)
        self.c1, self.c2 = (self.k1 * self.data_range) ** 2, (self.k2 * self.data_range) ** 2
        self.taps = ops.ssim_taps(self.window, self.sigma)
        self.state = None

    def structure(self):
        """what makes another object (and another recording) when it changes"""
        return (self.window, self.sigma, self.k1, self.k2, self.data_range)

    # -- device side -----------------------------------------------------------------------------------------------------------
    def _ensure(self, device):
        if self.state is None:
            self._make_record(ops.ss_state_new, device, self.weight, self.c1, self.c2)
        return self.state

    def set_weight(self, weight):
        """A new weight (>= 0), written into the device record between steps: a recorded step reads it from there."""
        self.weight = _number("weight", weight, "set_ssim_weight")
        if self.state is not None:
            ops.refuse_in_capture("set_ssim_weight inside a hipGraph capture")
            ops.ss_state_set(self.state, self.weight, self.c1, self.c2)

    def loss(self, a, b):
        """``ops.ssim`` with this object's record and window -> (weight * (1 - mean SSIM), 1 - mean SSIM), device scalars; the first
        is differentiable in whichever of ``a``, ``b`` requires a gradient."""
        weighted, term, _ = ops.ssim(a, b, self._ensure(a.device), self.taps)
        return weighted, term

    def value(self, a, b):
        """Per-sample SSIM [N] (fp32, on the device) without a gradient; the record is neither read nor written."""
        import torch
        with torch.no_grad():
            return ops.ssim(a.detach(), b.detach(), None, self.taps, self.c1, self.c2)[2]

    def stats(self):
        """The settings and the record's ``term`` (the last unweighted one), ``weighted``, ``updates``; SYNCHRONISES."""
        out = dict(weight=self.weight, window=self.window, sigma=self.sigma, k1=self.k1, k2=self.k2, data_range=self.data_range,
                   term=0.0, weighted=0.0, updates=0)
        if self.state is not None:
            rec = ops.ss_state_read(self.state)
            out.update(weight=rec["weight"], term=rec["term"], weighted=rec["weighted"], updates=rec["updates"])
        return out

    # -- hipGraph support, checkpoints -----------------------------------------------------------------------------------------------
    def fingerprint(self):
        """What a recording bakes in: the object, its structure (the taps and the record's constants), the record.  Not the weight:
        it is device state."""
        return (id(self), self.structure(), self._record_ptr())

    def state_dict(self):
        """the settings, the record's counter and last values; SYNCHRONISES"""
        st = self.stats()
        return {"weight": self.weight, "window": self.window, "sigma": self.sigma, "k1": self.k1, "k2": self.k2,
                "data_range": self.data_range, "updates": int(st["updates"]), "term": float(st["term"]),
                "weighted": float(st["weighted"])}

    def load_state_dict(self, sd, device=None):
        """The structure is part of what a step launches: it must be this object's (``SRGAN_training.load_state_dict`` makes a new
        object otherwise)."""
        theirs = (int(sd["window"]), float(sd["sigma"]), float(sd["k1"]), float(sd["k2"]), float(sd["data_range"]))
        if theirs != self.structure():
            raise ValueError(f"SSIM.load_state_dict: (window, sigma, k1, k2, data_range) = {theirs} in the state, {self.structure()} here")
        ops.refuse_in_capture("SSIM.load_state_dict inside a hipGraph capture")
        weight = _number("weight", sd["weight"], "SSIM.load_state_dict")
        updates = int(sd["updates"])
        term, weighted = float(sd["term"]), float(sd["weighted"])
        if updates < 0 or not (math.isfinite(term) and math.isfinite(weighted)):
            raise ValueError(f"SSIM: updates must be >= 0 and the last values finite, got {updates}, {term}, {weighted}")
        self.weight = weight
        if self.state is None and updates == 0:
            return                              # what a fresh record starts at
        if self.state is None and device is None:
            raise ValueError("SSIM: a count of updates without a device for its record")
        self._ensure(device)
        ops.ss_state_set(self.state, self.weight, self.c1, self.c2)
        ops.ss_state_restore(self.state, updates, term, weighted)
