"""Augmentation stages for the discriminator's inputs on the HIP path.  Extension, no counterpart in the reference.

Every batch the discriminator sees -- real and fake -- goes through each stage that is on, in order, and the generator's gradient
flows back through it.  Two stages exist: ``DiffAugment`` (Zhao et al., 2020: random colour change, translation and cutout; the
standard remedy when D memorises a small training set) and ``GeometricAugment`` (x-flip, 90-degree turns, isotropic scale,
rotation as one bilinear warp per sample), which runs after it.

What a stage provides (``_Stage`` holds what all of them share; a new stage is a subclass):

    groups          {policy entry: flag bit}; ``n_groups`` of them are gated per sample by adaptive augmentation (``srgan_amd.ada``)
    section         its name in a checkpoint, which is also the ``SRGAN_training`` attribute it lives in
    settings        the names of its numeric settings (saved, and part of a recording's fingerprint), ``_check_settings`` their check
    draw(n, h, w)   one CPU float32 table [n, 8] of per-sample parameters, drawn from a generator the STAGE owns (never the default
                    one: the step's style and reparametrisation noise is the same with the stage on or off); a group that is off
                    draws nothing and gets its identity values
    apply(x, table, gated)   the HIP kernels on a device table; ``gated``: slot 7 of a row is the skip mask ``ops.ada_gate`` wrote

``SRGAN_training._stages()`` is the list the train step, graph staging and checkpoints iterate; ``enable_diffaugment`` and
``enable_geometric_augment`` put a stage there."""
import math

import torch

from . import ops

__all__ = ["DiffAugment", "GROUPS", "GeometricAugment", "GEOM_GROUPS"]

GROUPS = {"color": ops.AUG_COLOR, "translation": ops.AUG_TRANSLATION, "cutout": ops.AUG_CUTOUT}
GEOM_GROUPS = {"flip": ops.GEOM_FLIP, "rot90": ops.GEOM_ROT90, "scale": ops.GEOM_SCALE, "rotate": ops.GEOM_ROTATE}


class _Stage:
    """What the stages share: the policy, the private generator, the injectable draw sources, the rows of the adaptive gate, and the
    extension interface of the train step (``fingerprint``, ``graph_keepalive``, ``state_dict`` / ``load_state_dict``)."""

    groups, n_groups, section, settings = {}, 0, None, ()

    def __init__(self, policy, seed, **settings):
        self.parse_policy(policy)              # an unknown name raises here
        self.policy = policy
        self._take(settings)
        self.generator = torch.Generator()
        if seed is None:
            self.generator.seed()
        else:
            self.generator.manual_seed(int(seed))
        self.draw_fn = self.draw               # tests may inject callable(n, h, w) -> CPU float32 [n, 8]
        self.gate_fn = self.draw_gate          # ... and callable(n) -> CPU float32 [n, n_groups] (adaptive augmentation only)

    @classmethod
    def parse_policy(cls, policy):
        """a comma-separated subset of the stage's groups ('' = identity) -> flag bits"""
        names = sorted(cls.groups)
        if not isinstance(policy, str):
            raise ValueError(f"{cls.__name__}: policy is a comma-separated string of {names}, got {policy!r}")
        flags = 0
        for name in (p.strip() for p in policy.split(",")):
            if name == "" and policy.strip() == "":
                continue
            if name not in cls.groups:
                raise ValueError(f"{cls.__name__}: unknown policy entry {name!r} (a comma-separated subset of {names})")
            flags |= cls.groups[name]
        return flags

    def _take(self, sd):
        for name, v in zip(self.settings, self._check_settings(*(sd[k] for k in self.settings))):
            setattr(self, name, v)

    @property
    def flags(self):
        return self.parse_policy(self.policy)

    def draw_gate(self, n):
        """One CPU float32 [n, n_groups] of uniforms in [0, 1) for n images, one per group in the order of ``groups``.  Adaptive
        augmentation (``srgan_amd.ada``) applies group g to a sample iff ``u_g < p``; drawn after the sample's table, from the same
        generator, and only with that feature on."""
        return torch.rand(n, self.n_groups, generator=self.generator, dtype=torch.float32)

    @classmethod
    def join_rows(cls, table, uniforms):
        """CPU ``[n, 8]`` table and ``[n, n_groups]`` uniforms -> the ``[n, 16]`` rows ``ops.ada_gate`` reads: the table in slots
        0..7, the uniforms from slot 8 on, zeros elsewhere."""
        n, g = table.shape[0], cls.n_groups
        if tuple(table.shape) != (n, ops.AUG_ROW) or tuple(uniforms.shape) != (n, g):
            raise ValueError(f"{cls.__name__}.join_rows: table {tuple(table.shape)} and uniforms {tuple(uniforms.shape)}; [n, 8] and "
                             f"[n, {g}] expected")
        rows = torch.zeros(n, ops.ADA_ROW, dtype=torch.float32)
        rows[:, :ops.AUG_ROW] = table.to(torch.float32)
        rows[:, 8:8 + g] = uniforms.to(torch.float32)
        return rows

    def __call__(self, x):
        """Draw, copy to the device, apply: for a training loop of one's own (differentiable in x)."""
        if self.flags == 0:
            return x
        n, _, h, w = x.shape
        table = self.draw_fn(n, h, w).to(dtype=torch.float32).pin_memory().to(x.device, non_blocking=True)
        return self.apply(x, table)

    def fingerprint(self):
        """what a recorded step bakes in: the groups launched, the settings, the draw sources"""
        return (id(self), self.flags, *(getattr(self, k) for k in self.settings), id(getattr(self.draw_fn, "__func__", self.draw_fn)),
                id(getattr(self.gate_fn, "__func__", self.gate_fn)))

    def graph_keepalive(self):
        """device buffers a recorded step points at: none (the tables are staged by the recording's owner)"""
        return []

    def state_dict(self):
        return {"policy": self.policy, **{k: getattr(self, k) for k in self.settings}, "generator": self.generator.get_state().clone()}

    def load_state_dict(self, sd):
        self.parse_policy(sd["policy"])
        self._take(sd)
        self.policy = sd["policy"]
        self.generator.set_state(sd["generator"])


def _window(size, ratio):
    return int(size * ratio + 0.5)


class DiffAugment(_Stage):
    """DiffAugment (Zhao et al., 2020), applied by ``ops.diffaugment`` (csrc/augment.hip).  One float32 row per sample:

        [b, s, a, ty, tx, cy, cx, 0]      b = r_b - 0.5, s = 2 r_s, a = r_c + 0.5 with r ~ U[0, 1)          (colour)
                                          ty in [-Sy, Sy], tx in [-Sx, Sx], S = int(size * translation + 0.5)  (translation)
                                          cy in [0, H + (1 - ch % 2)), cx likewise, ch = int(H * cutout + 0.5) (cutout)

    A group that is off gets identity values (0, 1, 1 / 0, 0 / 0, 0) and is not launched.  ``SRGAN_training.enable_diffaugment``
    wires it into the train step."""

    groups, n_groups, section, settings = GROUPS, 3, "augment", ("translation", "cutout")

    def __init__(self, policy="color,translation,cutout", translation=0.125, cutout=0.5, seed=None):
        super().__init__(policy, seed, translation=translation, cutout=cutout)
        if not (translation >= 0 and cutout >= 0):
            raise ValueError(f"DiffAugment: translation = {translation}, cutout = {cutout} (ratios >= 0)")

    @staticmethod
    def _check_settings(translation, cutout):
        return float(translation), float(cutout)

    def cut(self, h, w):
        """the cutout window (ch, cw) of an h x w image"""
        return _window(h, self.cutout), _window(w, self.cutout)

    def draw(self, n, h, w):
        """One CPU float32 table [n, 8] for n images of h x w; groups that are off get identity values and draw nothing."""
        g, flags = self.generator, self.flags
        t = torch.zeros(n, ops.AUG_ROW, dtype=torch.float32)
        t[:, 1:3] = 1.0
        if flags & ops.AUG_COLOR:
            r = torch.rand(n, 3, generator=g, dtype=torch.float32)
            t[:, 0] = r[:, 0] - 0.5
            t[:, 1] = r[:, 1] * 2.0
            t[:, 2] = r[:, 2] + 0.5
        if flags & ops.AUG_TRANSLATION:
            sy, sx = _window(h, self.translation), _window(w, self.translation)
            t[:, 3] = torch.randint(-sy, sy + 1, (n,), generator=g).to(torch.float32)
            t[:, 4] = torch.randint(-sx, sx + 1, (n,), generator=g).to(torch.float32)
        if flags & ops.AUG_CUTOUT:
            ch, cw = self.cut(h, w)
            t[:, 5] = torch.randint(0, h + (1 - ch % 2), (n,), generator=g).to(torch.float32)
            t[:, 6] = torch.randint(0, w + (1 - cw % 2), (n,), generator=g).to(torch.float32)
        return t

    def apply(self, x, table, gated=False):
        """``table``: device float32 [n, 8]; ``gated``: its slot 7 holds the per-sample skip mask (``ops.ada_gate``)"""
        flags = self.flags
        if flags == 0:
            return x
        return ops.diffaugment(x, table, flags, self.cut(x.shape[2], x.shape[3]), gated)


def _geom_settings(scale_std, rotate_max):
    try:
        s, r = float(scale_std), float(rotate_max)
    except (TypeError, ValueError):
        s = r = math.nan
    if not (0.0 <= s < math.inf and 0.0 <= r <= 1.0):
        raise ValueError(f"GeometricAugment: scale_std = {scale_std!r}, rotate_max = {rotate_max!r} (scale_std >= 0 and finite, "
                         "0 <= rotate_max <= 1)")
    return s, r


class GeometricAugment(_Stage):
    """The pixel-blitting and geometric groups of Karras et al. (2020) -- x-flip, 90-degree turns, isotropic scale, arbitrary rotation --
    as ONE bilinear affine warp per sample (``ops.geom_augment``, csrc/augment_geom.hip); a second stage, applied after
    ``DiffAugment``'s pass, with its own generator, table and kernels.  One float32 row per sample:

        [fx, k, zoom, cos, sin, 0, 0, 0]      fx in {0, 1}: mirror the columns                                      (flip)
                                              k in {0, 1, 2, 3} quarter turns; {0, 2} on non-square images          (rot90)
                                              zoom = 2 ** (N(0, 1) * scale_std), clamped to [0.5, 2]                (scale)
                                              theta ~ U(-pi, pi) * rotate_max, stored as cos and sin, computed in
                                              float64 and rounded to float32                                        (rotate)

    Output pixel q reads the source at ``cen + R(theta) Q(k) F(fx) (q - cen) / zoom``; pixels outside the image read 0 and the image
    size is kept.  A group that is off draws nothing and gets its identity value (0, 0, 1, (1, 0)).  ``rot90`` and ``rotate`` applied
    always are LEAKING augmentations in the sense of that paper (the generator learns to produce turned images): they are meant to
    run under the adaptive probability (``SRGAN_training.enable_ada``); ``flip`` is safe on flip-symmetric data.
    ``SRGAN_training.enable_geometric_augment`` wires it into the train step."""

    groups, n_groups, section, settings = GEOM_GROUPS, 4, "geometry", ("scale_std", "rotate_max")
    _check_settings = staticmethod(_geom_settings)

    def __init__(self, policy="flip,rot90,scale,rotate", scale_std=0.2, rotate_max=1.0, seed=None):
        super().__init__(policy, seed, scale_std=scale_std, rotate_max=rotate_max)

    def draw(self, n, h, w):
        """One CPU float32 table [n, 8] for n images of h x w; groups that are off get identity values and draw nothing."""
        g, flags = self.generator, self.flags
        t = torch.zeros(n, ops.GEOM_ROW, dtype=torch.float32)
        t[:, 2:4] = 1.0
        if flags & ops.GEOM_FLIP:
            t[:, 0] = (torch.rand(n, generator=g, dtype=torch.float32) < 0.5).to(torch.float32)
        if flags & ops.GEOM_ROT90:
            k = torch.randint(0, 4, (n,), generator=g) if h == w else 2 * torch.randint(0, 2, (n,), generator=g)
            t[:, 1] = k.to(torch.float32)
        if flags & ops.GEOM_SCALE:
            z = torch.randn(n, generator=g, dtype=torch.float32).to(torch.float64) * self.scale_std
            t[:, 2] = torch.exp2(z).clamp(0.5, 2.0).to(torch.float32)
        if flags & ops.GEOM_ROTATE:
            theta = (2.0 * torch.rand(n, generator=g, dtype=torch.float32).to(torch.float64) - 1.0) * (math.pi * self.rotate_max)
            t[:, 3] = torch.cos(theta).to(torch.float32)
            t[:, 4] = torch.sin(theta).to(torch.float32)
        return t

    def apply(self, x, table, gated=False):
        """``table``: device float32 [n, 8]; ``gated``: its slot 7 holds the per-sample skip mask (``ops.ada_gate``)"""
        return ops.geom_augment(x, table, self.flags, gated)
