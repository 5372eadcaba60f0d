"""Whole-trainer checkpoints: ``state_dict`` / ``load_state_dict`` / ``save_checkpoint`` / ``load_checkpoint`` of
``SRGAN_training`` and ``SingleGAN_training`` (extension: the reference's notebooks save ``G/D/E.state_dict()`` and cannot resume).

The dict holds everything the next ``train()`` depends on, as CPU tensors and plain ``int / float / bool / str / None / list /
dict`` -- a file written from it loads with ``torch.load(path, weights_only=True)``:

    version                  format version (``VERSION``); a newer one is refused
    config                   what changes the computation: trainer class, k, lbd, ndim, encoded_feature, n_batch, the two criteria,
                             the compute dtype (compared on load)
    G, D, E                  ``state_dict()`` of the unwrapped networks, the reference's keys (D: a list for per-domain discriminators)
    optG/D/E, scheG/D/E      ``state_dict()`` of the optimisers and schedulers (lists where the trainer keeps lists)
    hist_target              the histogram-imitation target the constructor drew (``lbd["hist"] > 0``)
    ema, augment, geometry,  the step's extensions that are on: the averaged copies and their update count, DiffAugment's settings
    ada, r1, bcr, lecam,     and generator, the geometric stage's settings and generator, the adaptive probability's settings and
    mode_seeking, ssim,      whole record (p, seen, the three counts, adjustments, last_r, the record's batch size n), R1's
                             gamma / every / updates (and the record's batch size n), consistency regularisation's weights / every /
                             policy / translation / generator / updates, LeCam's weight / decay / start / clamp / anchors / updates, mode seeking's weight / form / eps / tau / generator /
    grad_guard               updates and last ms / d_image / d_latent, the SSIM term's weight / on / window / sigma / k1 / k2 /
                             data_range / updates and last term / weighted, per guarded net max_norm and the cumulative steps /
                             skipped / clipped
    rng                      the CPU default generator (style and reparametrisation noise) and numpy's global one (``get_target``)

Not saved: the last step's images, ``loss_terms``, the label cache, workspaces, packed operands, the guard's decision and R1's
penalty of the last step -- the next step recomputes all of them.  A recording of the step is not saved either: a load drops it.

Data parallel: ``state_dict()`` is per process and issues no collective.  The replicas are identical by construction, the
generators are not (every rank draws its own DiffAugment tables, and its own noise): rank-exact resume needs one file per rank;
a rank-0 file loaded everywhere restores everything but the other ranks' random streams.
"""
import collections
import os
import tempfile

import numpy as np
import torch

from . import dp, ops
from .optim import Adam

__all__ = ["VERSION", "LoadReport", "Checkpointing"]

VERSION = 1

LoadReport = collections.namedtuple("LoadReport", ["missing", "unexpected"])
LoadReport.__doc__ = """Sections the trainer has but the checkpoint lacks (they keep their fresh state) / sections the trainer has no
use for (skipped)."""

_NETS = ("G", "D", "E")
_EXTENSIONS = ("ema", "augment", "geometry", "ada", "r1", "bcr", "lecam", "mode_seeking", "ssim", "grad_guard")
# the augmentation stages (srgan_amd.augment): (section, the trainer attribute the stage lives in, the switch that makes one, the keys
# of a saved section the switch takes, in its order), in the order of application
_STAGES = (("augment", "augment", "enable_diffaugment", ("policy", "translation", "cutout")),
           ("geometry", "geometry", "enable_geometric_augment", ("policy", "scale_std", "rotate_max")))


def _plain(obj, where="state_dict"):
    """A deep copy made of CPU tensor clones and plain Python values only; tuples become lists, numpy scalars Python ones."""
    if torch.is_tensor(obj):
        return obj.detach().to("cpu", copy=True).contiguous()
    if obj is None or isinstance(obj, (bool, int, float, str)):
        return obj
    if isinstance(obj, (np.bool_, np.integer, np.floating)):
        return obj.item()
    if isinstance(obj, dict):
        out = {}
        for k, v in obj.items():
            if not isinstance(k, (int, str)):
                raise TypeError(f"{where}: key {k!r} of type {type(k).__name__} (int or str expected)")
            out[k] = _plain(v, f"{where}[{k!r}]")
        return out
    if isinstance(obj, (list, tuple)):
        return [_plain(v, f"{where}[{i}]") for i, v in enumerate(obj)]
    raise TypeError(f"{where}: a {type(obj).__module__}.{type(obj).__qualname__} cannot go into a checkpoint (tensors and plain "
                    "Python values only)")


def _each(x):
    """the trainer keeps one object or a list of them (SingleGAN_training's per-domain discriminators)"""
    return list(x) if isinstance(x, (list, tuple)) else [x]


def _save_each(x, fn):
    return [fn(v) for v in x] if isinstance(x, (list, tuple)) else fn(x)


def _load_each(x, sd, what, fn):
    if isinstance(x, (list, tuple)) != isinstance(sd, (list, tuple)) or (isinstance(x, (list, tuple)) and len(x) != len(sd)):
        raise ValueError(f"load_state_dict: section '{what}' does not match the trainer's (one object against a list, or lists of "
                         "different lengths)")
    if isinstance(x, (list, tuple)):
        for v, s in zip(x, sd):
            fn(v, s)
    else:
        fn(x, sd)


def _criterion_name(c):
    name = type(c).__name__
    red = getattr(c, "reduction", "mean")
    return name if red == "mean" else f"{name}(reduction={red})"


def _numpy_rng_state():
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    return {"kind": str(kind), "keys": [int(v) for v in keys], "pos": int(pos), "has_gauss": int(has_gauss),
            "cached_gaussian": float(cached)}


def _set_numpy_rng_state(sd):
    np.random.set_state((sd["kind"], np.asarray(sd["keys"], dtype=np.uint32), int(sd["pos"]), int(sd["has_gauss"]),
                         float(sd["cached_gaussian"])))


class Checkpointing:
    """Mixin of the two trainer classes.  It reads the trainer through the attributes both keep (``G/D/E``, ``optG/D/E``,
    ``scheG/D/E``, ``hi``, ``lbd`` ...) and the extensions through the switches of ``SRGAN_training`` where they exist."""

    # ---- what this trainer has ---------------------------------------------------------------------------------------------------
    def _ckpt_config(self):
        cfg = {"trainer": type(self).__name__, "k": int(self.k), "lbd": {str(k): float(v) for k, v in self.lbd.items()},
               "ndim": int(self.ndim), "encoded_feature": str(self.encoded_feature), "n_batch": int(self.n_batch),
               "criterion": _criterion_name(self.criterion), "criterion_class": _criterion_name(self.criterion_class),
               "compute_dtype": ops.get_compute_dtype()}
        if hasattr(self, "singleD"):
            cfg.update(singleD=bool(self.singleD), classes=[int(c) for c in self.classes])
        return cfg

    def _ckpt_guards(self):
        """{net: its optimiser} for the nets with a gradient guard on"""
        if not hasattr(self, "enable_grad_guard"):
            return {}
        return {n: opt for n, opt in zip(_NETS, (self.optG, self.optD, self.optE)) if isinstance(opt, Adam) and opt._guard is not None}

    def _ckpt_sections(self):
        """Names of the sections ``state_dict(rng=False)`` writes besides version and config, without reading the device."""
        out = list(_NETS)
        out += [n for n in ("optG", "optD", "optE", "scheG", "scheD", "scheE") if getattr(self, n, None) is not None]
        if getattr(self, "hi", None) is not None:
            out.append("hist_target")
        for name, attr in (("ema", "_ema"), *(s[:2] for s in _STAGES), ("ada", "_ada"), ("r1", "_r1"), ("bcr", "bcr"),
                           ("lecam", "_lecam"), ("mode_seeking", "_ms"), ("ssim", "_ssim")):
            if getattr(self, attr, None) is not None:
                out.append(name)
        out += [f"grad_guard.{n}" for n in self._ckpt_guards()]
        return out

    def _ckpt_usable(self, name):
        """Can this trainer take section ``name`` of a checkpoint?"""
        if name in _NETS or name == "rng":
            return True
        if name in ("optG", "optD", "optE", "scheG", "scheD", "scheE"):
            return getattr(self, name, None) is not None
        if name == "hist_target":
            return getattr(self, "hi", None) is not None
        if name in _EXTENSIONS:
            return hasattr(self, "_extensions")          # SRGAN_training's interface; SingleGAN_training refuses these features
        return False

    def _ckpt_between_steps(self, what):
        if getattr(self, "_ema_scope", False):
            raise RuntimeError(f"{type(self).__name__}.{what} inside ema_weights(): self.G / self.E are the averaged copies there")
        ops.refuse_in_capture(f"{type(self).__name__}.{what} inside a hipGraph capture; checkpoints are taken between steps")

    # ---- save ---------------------------------------------------------------------------------------------------------------------
    def state_dict(self, rng=True):
        """A snapshot of everything the next ``train()`` depends on (module docstring): CPU clones and plain values.  Between steps
        only; reads the adaptive-probability, R1, consistency, LeCam, mode-seeking, SSIM and gradient-guard records, so it SYNCHRONISES the stream.  ``rng=False`` leaves the two host
        generators out.  Per process: no collective."""
        self._ckpt_between_steps("state_dict")
        sd = {"version": VERSION, "config": self._ckpt_config()}
        for n in _NETS:
            sd[n] = _save_each(getattr(self, n), lambda net: _plain(dp.unwrap(net).state_dict(), n))
        for n in ("optG", "optD", "optE", "scheG", "scheD", "scheE"):
            obj = getattr(self, n, None)
            if obj is not None:
                sd[n] = _save_each(obj, lambda o: _plain(o.state_dict(), n))
        if getattr(self, "hi", None) is not None:
            sd["hist_target"] = _plain(self.hi.target)
        if getattr(self, "_ema", None) is not None:
            sd["ema"] = _plain(self._ema.state_dict(), "ema")
        for name, attr, _, _ in _STAGES:
            if getattr(self, attr, None) is not None:
                sd[name] = _plain(getattr(self, attr).state_dict(), name)
        if getattr(self, "_ada", None) is not None:
            sd["ada"] = _plain(self._ada.state_dict(), "ada")
        r1 = getattr(self, "_r1", None)
        if r1 is not None:
            st = r1.stats()
            sd["r1"] = {"gamma": float(r1.gamma), "every": int(r1.every), "updates": int(st["updates"]),
                        "n": None if st["n"] is None else int(st["n"])}
        if getattr(self, "bcr", None) is not None:
            sd["bcr"] = _plain(self.bcr.state_dict(), "bcr")
        if getattr(self, "_lecam", None) is not None:
            sd["lecam"] = _plain(self._lecam.state_dict(), "lecam")
        if getattr(self, "_ms", None) is not None:
            sd["mode_seeking"] = _plain(self._ms.state_dict(), "mode_seeking")
        if getattr(self, "_ssim", None) is not None:
            sd["ssim"] = _plain(dict(self._ssim.state_dict(), on=list(self._ssim_on)), "ssim")
        guards = self._ckpt_guards()
        if guards:
            sd["grad_guard"] = {}
            for n, opt in guards.items():
                st = opt.grad_guard_stats()
                sd["grad_guard"][n] = {"max_norm": None if opt._guard.max_norm is None else float(opt._guard.max_norm),
                                       "steps": int(st["steps"]), "skipped": int(st["skipped"]), "clipped": int(st["clipped"])}
        if rng:
            sd["rng"] = {"torch": torch.get_rng_state().clone(), "numpy": _numpy_rng_state()}
        return sd

    def save_checkpoint(self, path, rng=True):
        """``torch.save(self.state_dict(rng), path)``, atomically: written to a temporary file in ``path``'s directory, then
        ``os.replace``.  A save that fails leaves the previous file as it was and no temporary file behind."""
        sd = self.state_dict(rng)
        path = os.fspath(path)
        fd, tmp = tempfile.mkstemp(dir=os.path.dirname(os.path.abspath(path)), prefix=os.path.basename(path) + ".", suffix=".tmp")
        try:
            with os.fdopen(fd, "wb") as f:
                torch.save(sd, f)
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp, path)
        except BaseException:
            try:
                os.unlink(tmp)
            except FileNotFoundError:
                pass
            raise

    # ---- load ---------------------------------------------------------------------------------------------------------------------
    def load_checkpoint(self, path, strict=True):
        """``load_state_dict`` of a file written by ``save_checkpoint`` (read to the CPU with ``weights_only=True``)."""
        return self.load_state_dict(torch.load(os.fspath(path), map_location="cpu", weights_only=True), strict)

    def _ckpt_compare_config(self, saved):
        mine, diff = self._ckpt_config(), []
        for key in sorted(set(mine) | set(saved)):
            a, b = mine.get(key), saved.get(key)
            if key == "lbd" and isinstance(a, dict) and isinstance(b, dict):
                diff += [f"lbd.{k}" for k in sorted(set(a) | set(b)) if k not in a or k not in b or float(a[k]) != float(b[k])]
            elif a != b:
                diff.append(key)
        return diff

    def load_state_dict(self, sd, strict=True):
        """Restore ``state_dict()`` into this trainer (built as for the run that saved: networks of the same layout,
        ``opt_sche_initialization()`` called).  Between steps only: ``RuntimeError`` inside a hipGraph capture and inside
        ``ema_weights()``.  -> ``LoadReport(missing, unexpected)``.

        Extensions the checkpoint holds are enabled with their saved settings if they are off; extensions that are on but not in
        the checkpoint stay on with fresh state (``missing``); sections this trainer has no use for are skipped (``unexpected``).
        ``strict=True``: either list, or a ``config`` that differs from the trainer's, raises ``ValueError`` naming the sections /
        fields BEFORE anything is written.  A recording of the step and the warm-up of its input shape are forgotten (torch's
        optimiser load replaces the moment tensors a recording points at): the next step runs eagerly, the one after records
        again; graph mode stays enabled.  Cached packed operands of every network and of the averaged copies are marked stale.
        ``ema_updates``, ``grad_guard_stats()``, ``r1_stats()``, ``bcr_stats()``, ``lecam_stats()``, ``mode_seeking_stats()`` and ``ssim_stats()`` continue from the saved
        counts."""
        self._ckpt_between_steps("load_state_dict")
        who = type(self).__name__
        if not isinstance(sd, dict) or "version" not in sd:
            raise ValueError(f"{who}.load_state_dict: not a trainer checkpoint (no 'version')")
        if int(sd["version"]) > VERSION:
            raise ValueError(f"{who}.load_state_dict: the checkpoint has format version {int(sd['version'])}, this package reads up "
                             f"to {VERSION}")
        diff = self._ckpt_compare_config(sd.get("config") or {}) if "config" in sd else []
        if diff and strict:
            raise ValueError(f"{who}.load_state_dict: the checkpoint's config differs from the trainer's in {', '.join(diff)} "
                             "(strict=False loads anyway)")
        in_file = [k for k in sd if k not in ("version", "config", "grad_guard")]
        in_file += [f"grad_guard.{n}" for n in (sd.get("grad_guard") or {})]
        unexpected = [k for k in in_file if not self._ckpt_usable(k.split(".")[0])]
        missing = [k for k in self._ckpt_sections() if k not in in_file]
        if strict and (missing or unexpected):
            raise ValueError(f"{who}.load_state_dict: " + "; ".join(
                t for t in ("missing in the checkpoint: " + ", ".join(missing) if missing else "",
                            "unexpected in the checkpoint: " + ", ".join(unexpected) if unexpected else "") if t)
                + " (strict=False loads what fits)")

        def use(name):
            return name in sd and name not in unexpected

        if use("ssim"):
            # what enable_ssim would refuse further down, refused here: nothing has been written yet
            from .structural import check_settings as _ssim_settings
            m = sd["ssim"]
            _ssim_settings(m["weight"], int(m["window"]), m["sigma"], m["k1"], m["k2"], m["data_range"], f"{who}.load_state_dict: ssim")
            if "idt" in m["on"] and not self.lbd["idt"] > 0:
                raise ValueError(f"{who}.load_state_dict: the checkpoint's SSIM term is taken on the identity reconstruction and this "
                                 "trainer's lbd['idt'] is 0, so its step makes no identity image (build the trainer with lbd['idt'] > "
                                 "0, or load with the section removed)")

        # a recording points at the moment tensors and device records replaced below, and the graphs the last step kept pin them
        graph = getattr(self, "_graph", None)
        if graph is not None:
            graph._drop()
        if hasattr(self, "_forget_step"):
            self._forget_step()
        else:
            self.target_image = self.recon_image = self.c_rand = self.enc_info = self.target_cenc = None
            self.loss_terms = {}

        stale = []
        for n in _NETS:
            if use(n):
                _load_each(getattr(self, n), sd[n], n, lambda net, s: dp.unwrap(net).load_state_dict(s))
            stale += [p for net in _each(getattr(self, n)) for p in net.parameters()]
        for n in ("optG", "optD", "optE"):
            if use(n):
                _load_each(getattr(self, n), sd[n], n, lambda o, s: o.load_state_dict(s))
        for n in ("scheG", "scheD", "scheE"):
            if use(n):
                _load_each(getattr(self, n), sd[n], n, lambda o, s: o.load_state_dict(s))
        for n in ("optG", "optD", "optE"):
            for opt in _each(getattr(self, n, None)):
                if isinstance(opt, Adam):
                    opt.sync_device()            # the learning rate a loaded scheduler stands at reaches the device records
        if use("hist_target"):
            with torch.no_grad():
                self.hi.target.copy_(sd["hist_target"])
        if use("ema"):
            self.load_ema_state_dict(sd["ema"])          # (enables it for the saved nets if it is off; re-seeds the record in place)
        for name, attr, enable, keys in _STAGES:
            if use(name):
                if getattr(self, attr) is None:
                    getattr(self, enable)(*(sd[name][k] for k in keys))
                getattr(self, attr).load_state_dict(sd[name])
        if use("ada"):
            a = sd["ada"]
            if self._ada is None or self._ada.interval != int(a["interval"]):
                self.enable_ada(a["target"], int(a["interval"]), a["kimg"], a["p"], a["p_max"])
            self._ada.load_state_dict(a, next(dp.unwrap(self.D).parameters()).device)
        if use("r1"):
            r = sd["r1"]
            if self._r1 is None or self._r1.every != int(r["every"]):
                self.enable_r1(r["gamma"], int(r["every"]))
            else:
                self.set_r1_gamma(r["gamma"])
            self._r1.set_updates(r["updates"], next(dp.unwrap(self.D).parameters()).device, r.get("n"))
        if use("bcr"):
            c = sd["bcr"]
            if self.bcr is None or self.bcr.every != int(c["every"]):
                self.enable_bcr(c["lambda_real"], c["lambda_fake"], int(c["every"]), c["policy"], c["translation"])
            self.bcr.load_state_dict(c, next(dp.unwrap(self.D).parameters()).device)
        if use("lecam"):
            c = sd["lecam"]
            if self._lecam is None or self._lecam.clamp != bool(c["clamp"]):
                self.enable_lecam(c["weight"], c["decay"], int(c["start"]), bool(c["clamp"]))
            self._lecam.load_state_dict(c, next(dp.unwrap(self.D).parameters()).device)
        if use("mode_seeking"):
            m = sd["mode_seeking"]
            if self._ms is None or self._ms.form != m["form"]:
                self.enable_mode_seeking(m["weight"], m["form"], m["eps"], m["tau"])
            self._ms.load_state_dict(m, next(dp.unwrap(self.G).parameters()).device)
        if use("ssim"):
            m = sd["ssim"]
            structure = (int(m["window"]), float(m["sigma"]), float(m["k1"]), float(m["k2"]), float(m["data_range"]))
            if self._ssim is None or self._ssim.structure() != structure or self._ssim_on != tuple(m["on"]):
                self.enable_ssim(m["weight"], tuple(m["on"]), *structure)
            self._ssim.load_state_dict(m, next(dp.unwrap(self.G).parameters()).device)
        for n, g in (sd.get("grad_guard") or {}).items():
            if f"grad_guard.{n}" in unexpected:
                continue
            opt = self._guard_opts((n,), "load_state_dict")[n]
            if opt._guard is None:
                opt.enable_grad_guard(g["max_norm"])
            else:
                opt.set_max_norm(g["max_norm"])
            opt.set_grad_guard_counters(g["steps"], g["skipped"], g["clipped"])
        if use("rng"):
            torch.set_rng_state(sd["rng"]["torch"])
            _set_numpy_rng_state(sd["rng"]["numpy"])

        # every cached packed operand describes the weights before the load (the bf16 mode runs on them alone)
        sn = self._sn() if hasattr(self, "_sn") else None
        if sn is not None:
            stale += sn.leaves
        if getattr(self, "_ema", None) is not None:
            stale += self._ema._params
        ops.mark_stale(stale)
        if graph is not None:
            graph._drop()                # (an extension enabled above must not leave a half-made state behind either)
        return LoadReport(missing, unexpected)
