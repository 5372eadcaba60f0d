"""Differentiable augmentation of the discriminator's inputs (DiffAugment: Zhao et al., 2020) on the HIP path.

Extension, no counterpart in the reference.  Every batch the discriminator sees -- real and fake -- goes through the same random
colour change, translation and cutout, and the generator's gradient flows back through it; the standard remedy when D memorises a
small training set.  The random parameters are drawn on the host from a generator THIS object owns (never the default one: the
step's style and reparametrisation noise is the same with the feature on or off), one float32 row per sample:

    [b, s, a, ty, tx, cy, cx, 0]      b = r_b - 0.5, s = 2 r_s, a = r_c + 0.5 with r ~ U[0, 1)          (colour)
                                      ty in [-Sy, Sy], tx in [-Sx, Sx], S = int(size * translation + 0.5)  (translation)
                                      cy in [0, H + (1 - ch % 2)), cx likewise, ch = int(H * cutout + 0.5) (cutout)

and applied by ``ops.diffaugment`` (csrc/augment.hip).  A group that is off gets identity values (0, 1, 1 / 0, 0 / 0, 0) and is
not launched.  ``SRGAN_training.enable_diffaugment`` wires it into the train step.

``GeometricAugment`` (below) is a second, independent stage -- x-flip, 90-degree turns, isotropic scale, rotation as one bilinear
warp per sample -- with its own generator, table and kernels; ``SRGAN_training.enable_geometric_augment`` runs it after this one."""
import math

import torch

from . import ops

__all__ = ["DiffAugment", "GROUPS", "GeometricAugment", "GEOM_GROUPS"]

GROUPS = {"color": ops.AUG_COLOR, "translation": ops.AUG_TRANSLATION, "cutout": ops.AUG_CUTOUT}


def parse_policy(policy):
    """'color,translation,cutout' (any comma-separated subset; '' = identity) -> flag bits"""
    if not isinstance(policy, str):
        raise ValueError(f"DiffAugment: policy is a comma-separated string of {sorted(GROUPS)}, got {policy!r}")
    flags = 0
    for name in (p.strip() for p in policy.split(",")):
        if name == "" and policy.strip() == "":
            continue
        if name not in GROUPS:
            raise ValueError(f"DiffAugment: unknown policy entry {name!r} (a comma-separated subset of {sorted(GROUPS)})")
        flags |= GROUPS[name]
    return flags


def _window(size, ratio):
    return int(size * ratio + 0.5)


class DiffAugment:
    def __init__(self, policy="color,translation,cutout", translation=0.125, cutout=0.5, seed=None):
        parse_policy(policy)                   # an unknown name raises here
        self.policy = policy
        if not (translation >= 0 and cutout >= 0):
            raise ValueError(f"DiffAugment: translation = {translation}, cutout = {cutout} (ratios >= 0)")
        self.translation = float(translation)
        self.cutout = float(cutout)
        self.generator = torch.Generator()
        if seed is None:
            self.generator.seed()
        else:
            self.generator.manual_seed(int(seed))
        self.draw_fn = self.draw               # tests may inject callable(n, h, w) -> CPU float32 [n, 8]
        self.gate_fn = self.draw_gate          # ... and callable(n) -> CPU float32 [n, 3] (adaptive augmentation only)

    @property
    def flags(self):
        return parse_policy(self.policy)

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

    def draw_gate(self, n):
        """One CPU float32 [n, 3] of uniforms in [0, 1) for n images: colour, translation, cutout.  Adaptive augmentation
        (``srgan_amd.ada``) applies group g to a sample iff ``u_g < p``; drawn after the sample's table, from the same generator,
        and only with that feature on."""
        return torch.rand(n, 3, generator=self.generator, dtype=torch.float32)

    def apply(self, x, table, gated=False):
        """``table``: device float32 [n, 8]; ``gated``: its slot 7 holds the per-sample skip mask (``ops.ada_gate``)"""
        flags = self.flags
        if flags == 0:
            return x
        return ops.diffaugment(x, table, flags, self.cut(x.shape[2], x.shape[3]), gated)

    def __call__(self, x):
        """Draw, copy to the device, apply: for a training loop of one's own (differentiable in x)."""
        if self.flags == 0:
            return x
        n, _, h, w = x.shape
        table = self.draw_fn(n, h, w).to(dtype=torch.float32).pin_memory().to(x.device, non_blocking=True)
        return self.apply(x, table)

    def fingerprint(self):
        """what a recorded step bakes in: the groups launched, the window ratios, the draw source"""
        return (id(self), self.flags, self.translation, self.cutout, id(getattr(self.draw_fn, "__func__", self.draw_fn)),
                id(getattr(self.gate_fn, "__func__", self.gate_fn)))

    def graph_keepalive(self):
        """device buffers a recorded step points at: none (the tables are staged by the recording's owner)"""
        return []

    def state_dict(self):
        return {"policy": self.policy, "translation": self.translation, "cutout": self.cutout,
                "generator": self.generator.get_state().clone()}

    def load_state_dict(self, sd):
        parse_policy(sd["policy"])
        self.policy = sd["policy"]
        self.translation, self.cutout = float(sd["translation"]), float(sd["cutout"])
        self.generator.set_state(sd["generator"])


# ---- the geometric stage --------------------------------------------------------------------------------------------------------------
GEOM_GROUPS = {"flip": ops.GEOM_FLIP, "rot90": ops.GEOM_ROT90, "scale": ops.GEOM_SCALE, "rotate": ops.GEOM_ROTATE}


def parse_geom_policy(policy):
    """'flip,rot90,scale,rotate' (any comma-separated subset; '' = identity) -> flag bits"""
    if not isinstance(policy, str):
        raise ValueError(f"GeometricAugment: policy is a comma-separated string of {sorted(GEOM_GROUPS)}, got {policy!r}")
    flags = 0
    for name in (p.strip() for p in policy.split(",")):
        if name == "" and policy.strip() == "":
            continue
        if name not in GEOM_GROUPS:
            raise ValueError(f"GeometricAugment: unknown policy entry {name!r} (a comma-separated subset of {sorted(GEOM_GROUPS)})")
        flags |= GEOM_GROUPS[name]
    return flags


def _geom_settings(scale_std, rotate_max):
    try:
        s, r = float(scale_std), float(rotate_max)
    except (TypeError, ValueError):
        s = r = math.nan
    if not (0.0 <= s < math.inf and 0.0 <= r <= 1.0):
        raise ValueError(f"GeometricAugment: scale_std = {scale_std!r}, rotate_max = {rotate_max!r} (scale_std >= 0 and finite, "
                         "0 <= rotate_max <= 1)")
    return s, r


class GeometricAugment:
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
    run under the adaptive probability (``SRGAN_training.enable_ada``); ``flip`` is safe on flip-symmetric data."""

    def __init__(self, policy="flip,rot90,scale,rotate", scale_std=0.2, rotate_max=1.0, seed=None):
        parse_geom_policy(policy)              # an unknown name raises here
        self.policy = policy
        self.scale_std, self.rotate_max = _geom_settings(scale_std, rotate_max)
        self.generator = torch.Generator()
        if seed is None:
            self.generator.seed()
        else:
            self.generator.manual_seed(int(seed))
        self.draw_fn = self.draw               # tests may inject callable(n, h, w) -> CPU float32 [n, 8]
        self.gate_fn = self.draw_gate          # ... and callable(n) -> CPU float32 [n, 4] (adaptive augmentation only)

    @property
    def flags(self):
        return parse_geom_policy(self.policy)

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

    def draw_gate(self, n):
        """One CPU float32 [n, 4] of uniforms in [0, 1) for n images: flip, rot90, scale, rotate.  Adaptive augmentation applies group
        g to a sample iff ``u_g < p``; drawn after the sample's table, from the same generator, and only with that feature on."""
        return torch.rand(n, 4, generator=self.generator, dtype=torch.float32)

    def apply(self, x, table, gated=False):
        """``table``: device float32 [n, 8]; ``gated``: its slot 7 holds the per-sample skip mask (``ops.ada_gate_geom``)"""
        return ops.geom_augment(x, table, self.flags, gated)

    def __call__(self, x):
        """Draw, copy to the device, apply: for a training loop of one's own (differentiable in x)."""
        if self.flags == 0:
            return x
        n, _, h, w = x.shape
        table = self.draw_fn(n, h, w).to(dtype=torch.float32).pin_memory().to(x.device, non_blocking=True)
        return self.apply(x, table)

    def fingerprint(self):
        """what a recorded step bakes in: the groups launched and the draw sources (the settings only shape the host draws)"""
        return (id(self), self.flags, self.scale_std, self.rotate_max, id(getattr(self.draw_fn, "__func__", self.draw_fn)),
                id(getattr(self.gate_fn, "__func__", self.gate_fn)))

    def graph_keepalive(self):
        """device buffers a recorded step points at: none (the tables are staged by the recording's owner)"""
        return []

    def state_dict(self):
        return {"policy": self.policy, "scale_std": self.scale_std, "rotate_max": self.rotate_max,
                "generator": self.generator.get_state().clone()}

    def load_state_dict(self, sd):
        parse_geom_policy(sd["policy"])
        self.scale_std, self.rotate_max = _geom_settings(sd["scale_std"], sd["rotate_max"])
        self.policy = sd["policy"]
        self.generator.set_state(sd["generator"])


def join_geom_rows(table, uniforms):
    """CPU ``[n, 8]`` geometry table and ``[n, 4]`` uniforms -> the ``[n, 16]`` rows ``ops.ada_gate_geom`` reads (slots 8..11 the
    uniforms)."""
    n = table.shape[0]
    if tuple(table.shape) != (n, ops.GEOM_ROW) or tuple(uniforms.shape) != (n, 4):
        raise ValueError(f"join_geom_rows: table {tuple(table.shape)} and uniforms {tuple(uniforms.shape)}; [n, 8] and [n, 4] expected")
    rows = torch.zeros(n, ops.ADA_ROW, dtype=torch.float32)
    rows[:, :ops.GEOM_ROW] = table.to(torch.float32)
    rows[:, 8:12] = uniforms.to(torch.float32)
    return rows
