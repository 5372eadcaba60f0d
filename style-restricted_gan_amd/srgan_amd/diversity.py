"""Mode-seeking (diversity) regularisation of the generator: the ratio term of MSGAN (Mao et al., CVPR 2019, "Mode Seeking
Generative Adversarial Networks for Diverse Image Synthesis") and its per-sample, clamped form of DSGAN (Yang et al., ICLR 2019,
"Diversity-Sensitive Conditional Generative Adversarial Networks").  An extension, the reference ships no code for it.

The same sources are translated twice, with two latent codes ``z1``, ``z2``; the generator is penalised where a large distance of
the codes gives a small distance of the images -- the failure in which G ignores the style code.  With ``s_i = sum |I1_i - I2_i|``
over the ``CHW`` values of row i and ``t_i = sum |z1_i - z2_i|`` over the ``d`` values of its code:

    msgan     dI = sum_i s_i / (B CHW), dz = sum_i t_i / (B d), ms = dz / (dI + eps dz)       (= MSGAN's 1 / (dI / dz + eps); 0 at dz = 0)
    dsgan     r_i = (s_i / CHW) / (t_i / d), ms = -(1 / B) sum_i min(r_i, tau)                (a row with t_i = 0 counts as clamped)

``weight * ms`` is minimised.  No gradient goes to the codes (they are noise).  ``weight``, ``eps``, ``tau``, the last values and an
update counter live in a device record, so ``set_weight`` between steps keeps a recorded hipGraph valid; the three kernels are in
``csrc/diversity.hip`` (``ops.mode_seeking``)."""
import torch

from . import ops

__all__ = ["ModeSeeking", "FORMS", "check_settings"]

FORMS = tuple(sorted(ops.MS_FORMS))


def _number(name, v, what, low_open=False):
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} must be a number, got {v!r}") from None
    if isinstance(v, bool) or not (0.0 < f if low_open else 0.0 <= f) or not f < float("inf"):
        raise ValueError(f"{what}: {name} must be finite and {'> 0' if low_open else '>= 0'}, got {v!r}")
    return f


def check_settings(weight, form, eps, tau, what="ModeSeeking"):
    """-> (float weight, form, float eps, float tau or None); ValueError for a weight < 0, eps <= 0, tau < 0 (or any not finite), an
    unknown form, and ``form="dsgan"`` without ``tau``: the right clamp depends on the data's scale, so there is no default."""
    if form not in ops.MS_FORMS:
        raise ValueError(f"{what}: form must be one of {list(FORMS)}, got {form!r}")
    weight = _number("weight", weight, what)
    eps = _number("eps", eps, what, low_open=True)
    if tau is None:
        if form == "dsgan":
            raise ValueError(f"{what}: form='dsgan' needs tau, the clamp of the per-sample ratio (it depends on the data's scale: "
                             "no default)")
    else:
        tau = _number("tau", tau, what)
    return weight, form, eps, tau


class ModeSeeking(ops.RecordOwner):
    """The settings, a CPU generator of its own for the second latent code and the device record, made at the first use -- never
    inside a hipGraph capture.  ``SRGAN_training.enable_mode_seeking`` wires it into the train step; for a loop of one's own:

        z2 = ms.draw(B, ndim).to(device)
        i2 = G(src, torch.cat([onehot, z2], 1))
        weighted, value = ms.loss(i1, i2, z1, z2)         # add ``weighted`` to the generator's loss
    """

    section = "mode_seeking"       # its name in a checkpoint and among the staged draws of a recorded step

    def __init__(self, weight=1.0, form="msgan", eps=1e-5, tau=None, seed=None):
        self.weight, self.form, self.eps, self.tau = check_settings(weight, form, eps, tau)
        self.generator = torch.Generator()
        if seed is None:
            self.generator.seed()
        else:
            self.generator.manual_seed(int(seed))
        self.draw_fn = self.draw           # tests may inject callable(n, ndim) -> CPU float32 [n, ndim]
        self.state = None

    def draw(self, n, ndim):
        """One CPU float32 ``[n, ndim]`` of standard normals from the object's own generator (never the default one)."""
        return torch.randn(n, ndim, generator=self.generator, dtype=torch.float32)

    # -- device side -----------------------------------------------------------------------------------------------------------
    def _tau(self):
        return 0.0 if self.tau is None else self.tau

    def _ensure(self, device):
        if self.state is None:
            self._make_record(ops.ms_state_new, device, self.weight, self.eps, self._tau())
        return self.state

    def set_weight(self, weight):
        """A new weight (>= 0), written into the device record between steps: a recorded step reads it from there."""
        self.weight = check_settings(weight, self.form, self.eps, self.tau, "set_mode_seeking_weight")[0]
        if self.state is not None:
            ops.refuse_in_capture("set_mode_seeking_weight inside a hipGraph capture")
            ops.ms_state_set(self.state, self.weight, self.eps, self._tau())

    def loss(self, i1, i2, z1, z2):
        """``ops.mode_seeking`` with this object's record and form -> (weight * ms, ms), device scalars."""
        return ops.mode_seeking(i1, i2, z1, z2, self._ensure(i1.device), self.form)

    def stats(self):
        """``weight``, ``form``, ``eps``, ``tau`` and the record's ``ms``, ``d_image``, ``d_latent``, ``updates``; SYNCHRONISES."""
        out = dict(weight=self.weight, form=self.form, eps=self.eps, tau=self.tau, ms=0.0, d_image=0.0, d_latent=0.0, updates=0)
        if self.state is not None:
            rec = ops.ms_state_read(self.state)
            out.update(weight=rec["weight"], ms=rec["ms"], d_image=rec["d_image"], d_latent=rec["d_latent"], updates=rec["updates"])
        return out

    # -- hipGraph support, checkpoints -----------------------------------------------------------------------------------------------
    def fingerprint(self):
        """What a recording bakes in: the object, the form (a kernel argument), the draw source, the record.  Not the weight (nor
        eps, tau): they are device state."""
        return (id(self), self.form, id(getattr(self.draw_fn, "__func__", self.draw_fn)), self._record_ptr())

    def state_dict(self):
        """the settings, the generator's state, the record's counter and last values; SYNCHRONISES"""
        st = self.stats()
        return {"weight": self.weight, "form": self.form, "eps": self.eps, "tau": self.tau,
                "generator": self.generator.get_state().clone(), "updates": int(st["updates"]), "ms": float(st["ms"]),
                "d_image": float(st["d_image"]), "d_latent": float(st["d_latent"])}

    def load_state_dict(self, sd, device=None):
        """``form`` is part of what a step launches: it must be this object's (``SRGAN_training.load_state_dict`` makes a new object
        otherwise)."""
        if sd["form"] != self.form:
            raise ValueError(f"ModeSeeking.load_state_dict: form = {sd['form']!r} in the state, {self.form!r} here")
        ops.refuse_in_capture("ModeSeeking.load_state_dict inside a hipGraph capture")
        self.weight, _, self.eps, self.tau = check_settings(sd["weight"], sd["form"], sd["eps"], sd["tau"], "ModeSeeking.load_state_dict")
        updates = int(sd["updates"])
        if updates < 0:
            raise ValueError(f"ModeSeeking: updates must be >= 0, got {updates}")
        self.generator.set_state(sd["generator"])
        if self.state is None and updates == 0:
            return                              # what a fresh record starts at
        if self.state is None and device is None:
            raise ValueError("ModeSeeking: a count of updates without a device for its record")
        self._ensure(device)
        ops.ms_state_set(self.state, self.weight, self.eps, self._tau())
        ops.ms_state_restore(self.state, updates, sd["ms"], sd["d_image"], sd["d_latent"])
