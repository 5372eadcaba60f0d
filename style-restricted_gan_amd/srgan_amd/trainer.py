"""``SRGAN_training``: the Style-Restricted GAN train step on the MI355X HIP path.

Same constructor / method signatures and return values as the reference class
(pyfiles/util_notebook.py:419-734); ``sg.train(source_image, label)`` drops into the loop of
``05-train_Style-Restricted_GAN.ipynb``.  What differs is HOW the step is executed:

* every network op and loss is a hand-written gfx950 kernel (``srgan_amd.ops``);
* result-preserving work savings of SURVEY.md Appendix B.2: the G forwards of the first k-1
  D-updates record no graph; D's weight gradients are not computed in phase 1 and E's not in
  phase 2 (they are discarded by the reference's ``zero_grad`` calls); the encoder trunk runs once
  for the two phase-1 ``E(source)`` calls; errG and errE are back-propagated in one pass;
* under ``torch.distributed`` (one process per GPU) gradients are averaged with bucketed RCCL
  all-reduce (``srgan_amd.dp``) and the batch-statistics losses see the all-gathered mu.

This module chooses the launches (the step body, ``_step``, the ``enable_*`` switches, ``SingleGAN_training``); how a fixed launch
sequence is recorded into a hipGraph and replayed (``_StepGraph``, ``_Recording``) lives in ``srgan_amd.step_graph``; saving and
resuming the whole trainer (``state_dict``, ``load_state_dict``, ``save_checkpoint``, ``load_checkpoint``) in
``srgan_amd.checkpoint``.

Semantics kept on purpose: stale ``target_image`` graph re-used after
``optG.step()`` with weights read at backward time; the no-op "unrolled" restore of D; corr/hist
nested under batch_KL; the n/(n-1) double correction with the constructor's batch size; errE returned
is the reporting sum; CPU-generator RNG order (k x randn, then normal_ x2, then normal_ x3).
"""
import contextlib
import gc

import numpy as np
import torch
import torch.nn as nn
import torch.optim as optim

from . import dp, ema, ops, spectral
from . import ada as _adamod
from .augment import DiffAugment, GeometricAugment
from . import consistency as _crmod
from . import diversity as _msmod
from . import lecam as _lcmod
from . import structural as _ssmod
from .checkpoint import Checkpointing
from . import r1 as _r1mod
from .losses import class_encode, criterion_kind, get_domainloss_D, get_loss_D, has_fused_kind, histogram_imitation
from .model import SingleGenerator, batch_stats_synced, host_to_device, per_sample
from .optim import Adam
from .step_graph import _Recording, _StepGraph, lib_prof_off  # noqa: F401  (graph mode: how the step below is recorded / replayed)

__all__ = ["SRGAN_training", "SingleGAN_training"]


@contextlib.contextmanager
def _frozen(params):
    """Temporarily mark parameters as not requiring grad (skips their weight-gradient kernels)."""
    flags = [(p, p.requires_grad) for p in params]
    for p, _ in flags:
        p.requires_grad_(False)
    try:
        yield
    finally:
        for p, f in flags:
            p.requires_grad_(f)


class SRGAN_training(Checkpointing):
    """
    net            : [G, D, E] nn.Modules          opt : [optG, optD, optE] (None -> fused HIP Adam)
    criterion      : [criterion, criterion_class]   (nn.MSELoss in every reference notebook; nn.BCEWithLogitsLoss / nn.BCELoss
                     are the other kinds with fused kernels: losses.criterion_kind)
    lbd            : dict of loss weights: class, cycle, idt, reg, idt_reg, KL, batch_KL, corr_enc, hist
    unrolled_k     : number of D updates per G/E update
    device         : "cuda" / torch.device           ref_label : np.array (class_num, dim), usually one-hot
    batch_size     : GLOBAL batch size (n of the batch-KL correction)
    encoded_feature: "latent" or "mu"                ndim : style-code dimension
    """

    def __init__(self, net, opt, criterion, lbd, unrolled_k, device, ref_label,
                 batch_size=64, encoded_feature="latent", ndim=8):
        self.G, self.D, self.E = net[0].to(device), net[1].to(device), net[2].to(device)
        self.optG, self.optD, self.optE = opt[0], opt[1], opt[2]
        self.scheG, self.scheD, self.scheE = None, None, None
        self.criterion, self.criterion_class = criterion
        self.lbd = lbd
        self.k = unrolled_k
        self.device = device
        self.ref_label = ref_label
        self.n_batch = batch_size
        self.encoded_feature = encoded_feature
        self.ndim = ndim
        self.source_image = None
        self.target_image = None
        self.recon_image = None
        self.label = None
        self.c_rand = None
        self.enc_info = None
        self.target_cenc = None
        if lbd["hist"] > 0:
            self.hi = histogram_imitation(device)
        self.loss_terms = {}           # last step's individual loss values (device scalars)
        self._reducers = {}
        self.noise_fn = torch.randn    # style noise source (CPU default generator, as the reference); tests may inject
        self._graph = None             # hipGraph mode (enable_graph)
        self._g_active = False         # True while the step body reads its inputs from the static device buffers
        self._ema = None               # averaged copies of G / E (enable_ema)
        self.G_ema = self.E_ema = None
        self._ema_scope = False        # inside ema_weights(): self.G / self.E are the copies
        self.augment = None            # DiffAugment of the discriminator's inputs (enable_diffaugment)
        self.geometry = None           # geometric augmentation of the discriminator's inputs, after DiffAugment (enable_geometric_augment)
        self._ada = None               # adaptive augmentation probability on the device (enable_ada)
        self._r1 = None                # R1 gradient penalty on the real rows (enable_r1)
        self.bcr = None                # balanced consistency regularisation of D (enable_bcr)
        self._lecam = None             # LeCam regularisation of D (enable_lecam)
        self._ms = None                # mode-seeking regularisation of G (enable_mode_seeking)
        self._ssim = None              # structural-similarity term of the reconstructions (enable_ssim)
        self._ssim_on = ()             # which of ("cycle", "idt") it is taken on
        self._label_cache = {}         # (kind, which) -> (label tensor, its device form): _cached
        self._d_pending = None         # an update_D left its all-reduce / optimiser step to _finish_D: the reducer, or True
        self._sn_cache = (None, None)  # (key, spectral controller or None): _sn
        ref = np.asarray(ref_label)
        self._ref_is_onehot = ref.ndim == 2 and ref.shape[0] == ref.shape[1] and np.array_equal(ref, np.eye(ref.shape[0]))
        # norm_type="batch": G / E normalise with batch statistics, so batching several of the reference's calls into one is a
        # different computation (and a different number of running-buffer updates); those sites run call by call
        self._g_per_sample = per_sample(dp.unwrap(self.G))
        self._e_per_sample = per_sample(dp.unwrap(self.E))
        if dp.world_size() > 1 and not (batch_stats_synced(dp.unwrap(self.G)) and batch_stats_synced(dp.unwrap(self.E))):
            raise NotImplementedError(
                "SRGAN_training: G / E hold batch-statistics norms (norm_type='batch') and a process group has "
                f"{dp.world_size()} ranks; nn.DataParallel gives per-replica statistics and rank-0 running buffers, which this "
                "package does not build (one process, or norm_type='instance'). Statistics of the global batch are an opt-in: "
                "mark both networks with dp.sync_batch_stats(net).")
        self._sn()

    # ------------------------------------------------------------------------------------------
    def opt_sche_initialization(self, lr=[0.0001, 0.0001, 0.0001]):
        """Create the missing optimisers (Adam lr, betas=(0.5,0.999)) and ExponentialLR(gamma=0.95)
        schedulers for G, D, E   (util_notebook.py:484-508)."""
        lr_G, lr_D, lr_E = lr
        if self.optG is None:
            self.optG = Adam(self.G.parameters(), lr=lr_G, betas=(0.5, 0.999))
        self.scheG = optim.lr_scheduler.ExponentialLR(self.optG, gamma=0.95)
        if self.optD is None:
            self.optD = Adam(self.D.parameters(), lr=lr_D, betas=(0.5, 0.999))
        self.scheD = optim.lr_scheduler.ExponentialLR(self.optD, gamma=0.95)
        if self.optE is None:
            self.optE = Adam(self.E.parameters(), lr=lr_E, betas=(0.5, 0.999))
        self.scheE = optim.lr_scheduler.ExponentialLR(self.optE, gamma=0.95)
        return

    # ------------------------------------------------------------------------------------------
    # helpers
    def _cached(self, kind, which, make):
        """Per-label-tensor cache (labels are fixed during a step; class_encode forces a host sync)."""
        lab = self.label[which]
        hit = self._label_cache.get((kind, which))
        if hit is None or hit[0] is not lab:
            hit = self._label_cache[(kind, which)] = (lab, make(lab))
        return hit[1]

    def _onehot(self, which):
        if self._g_active:
            return self._graph.onehot(which)
        return self._cached("onehot", which, lambda lab: class_encode(lab, self.device, self.ref_label))

    def _label_dev(self, which):
        if self._g_active:
            return self._graph.lab[which]
        return self._cached("index", which,
                            lambda lab: host_to_device(torch.as_tensor(lab).to(dtype=torch.int64), self.device))

    def _noise(self, kind, nb):
        """Next style / reparametrisation noise [nb, ndim] of the step, on the device.  All of it comes from the CPU default
        generator in the reference's order: k x ``randn`` (util_notebook.py:554), then ``normal_`` per
        encoder call (model.py:461).  Graph mode: the draws were made up front (same order) and staged; this hands out the
        next slice of the static buffer."""
        if self._g_active:
            return self._graph.staged_noise.next(1)
        cpu = self.noise_fn(nb, self.ndim) if kind == "randn" else torch.FloatTensor(nb, self.ndim).normal_()
        return host_to_device(cpu, self.device)

    def _stages(self):
        """The augmentation stages (``srgan_amd.augment``) the trainer holds, in the order they are applied to what D reads.  The
        step, graph staging (``step_graph``) and checkpoints go by this list; a stage lives in the attribute its ``section`` names."""
        return [s for s in (self.augment, self.geometry) if s is not None]

    @staticmethod
    def _stage_on(stage):
        """Does the step run this stage?  (None, or an empty policy, is the plain step: no draw, no launch)"""
        return stage is not None and stage.flags != 0

    def _drawing_stages(self):
        """Every stage whose host-drawn tables a step consumes: those of ``_stages()``, then the consistency pairs' (which is not
        applied to everything D reads: its tables go to the penalised discriminator updates alone), then mode seeking's object,
        whose one "table" per step is the second latent code [B, ndim] of phase 1 (staged under its ``section``)."""
        return (self._stages() + ([self.bcr.stage] if self.bcr is not None else [])
                + ([self._ms] if self._ms is not None else []))            # (mode seeking: the second latent code, one draw per step)

    def _gated(self, stage):
        """Does the adaptive probability gate this stage's groups?  Those applied to everything D reads; never the consistency
        transform."""
        return self._ada is not None and any(stage is s for s in self._stages())

    def _stage_draws(self, stage):
        """tables of a stage a step consumes: 2 per discriminator update, 1 for phase 1; the consistency pairs: 2 per PENALISED
        discriminator update (real rows, then fake rows), none for phase 1, also with an empty policy; mode seeking: 1"""
        if self.bcr is not None and stage is self.bcr.stage:
            return 2 * sum(_crmod.schedule(self.k, self.bcr.every))
        if stage is self._ms and stage is not None:
            return 1                            # mode seeking: the second latent code of phase 1
        return 2 * self.k + 1 if self._stage_on(stage) else 0

    def _stage_row_draw(self, stage, nb, h, w):
        """One host draw of the step: the CPU table [nb, 8] of the stage's ``draw_fn``; with adaptive augmentation on, followed by
        one uniform per group and sample of its ``gate_fn`` and joined into the [nb, 16] rows ``ops.ada_gate`` reads."""
        if stage is self._ms:
            return stage.draw_fn(nb, self.ndim).to(torch.float32)      # mode seeking: [nb, ndim] standard normals, its own generator
        table = stage.draw_fn(nb, h, w).to(torch.float32)
        if not self._gated(stage):
            return table
        return stage.join_rows(table, stage.gate_fn(nb))

    def _stage_tables(self, stage, count, nb, h, w):
        """The next ``count`` parameter tables of a stage as ONE device tensor [count * nb, 8].  Draw order of a step
        (``_stage_draws``): per discriminator update the real rows' table, then the fake rows'; after the k updates phase 1's.  They
        come from the stage's own generator, never the default one.  Graph mode: drawn up front in the same order and staged; this
        hands out the next slice of the stage's static buffer.  Adaptive augmentation: the rows are [count * nb, 16] and go through
        ONE ``ada_gate`` launch, which reads p and writes the tables with their skip masks (every stage's gate of an update reads
        the same p: the record is moved by the update's observation, after all of them)."""
        if self._g_active:
            rows = self._graph.staged[stage.section].next(count)
        else:
            tabs = [self._stage_row_draw(stage, nb, h, w) for _ in range(count)]
            rows = host_to_device(tabs[0] if count == 1 else torch.cat(tabs, 0), self.device)
        if not self._gated(stage):
            return rows
        self._ada._ensure(rows.device, nb)
        return self._ada.gate(rows, stage.n_groups)

    def _aug(self, image, count=1, stages=None):
        """The stages that are on (all, or ``stages``), in order, on a batch of ``count`` tables' worth of rows D is about to read
        (differentiable): ONE launch per stage; the image itself with all of them off."""
        n, _, h, w = image.shape
        for stage in self._stages() if stages is None else stages:
            if self._stage_on(stage):
                image = stage.apply(image, self._stage_tables(stage, count, n // count, h, w), gated=self._ada is not None)
        return image

    def _noise_kinds(self):
        """The step's noise draws in order (fused execution paths)."""
        L = self.lbd
        return (["randn"] * self.k + ["normal"] * (2 if L["idt"] > 0 else 1)
                + ["normal"] * (3 if L["idt_reg"] * L["idt"] > 0 else 1))

    @staticmethod
    def _opt_params(opt):
        return [p for g in opt.param_groups for p in g["params"]]

    # What the step is made of, for graph mode (srgan_amd.step_graph).  An optional feature joins a recording's fingerprint and
    # keep-alive list by being in _extensions(), in a fixed order: it needs fingerprint() and graph_keepalive().
    def _opts(self):
        return (self.optG, self.optD, self.optE)

    def _extensions(self):
        return [x for x in (self._ema, self._sn(), *self._stages(), self._ada, self._r1, self.bcr, self._lecam, self._ms, self._ssim) if x is not None]

    def _mirrors(self):
        """who mirrors, on the host, a device-side count that the step advances: Adam's step counts, the EMA's update count"""
        return list(self._opts()) + ([self._ema] if self._ema is not None else [])

    def _forget_step(self):
        """Drop what the last step left behind.  It keeps its last autograd graph on purpose (``target_image`` is back-propagated
        twice); a parameter's AccumulateGrad node lives as long as any graph that points at it and remembers the stream it was
        made on, which an eager step and a recorded one must not share (step_graph).  Every retained reference pins such a
        graph, so all go: the images, the loss terms, the label cache, the optimisers' keep-alives.  All are rebuilt on demand."""
        self.target_image = self.recon_image = self.c_rand = self.enc_info = self.target_cenc = None
        self.loss_terms = {}
        self._label_cache.clear()
        for opt in self._opts():
            opt._keep_alive = None
        gc.collect()

    def _step(self, opt):
        """optimiser step + one launch that re-packs the cached conv operands of the weights it just changed"""
        sn = self._sn() if opt is self.optD else None
        if sn is None:
            opt.step()
            ops.refresh_packed(self._opt_params(opt))
            return
        # spectrally normalised D: the gradients of the normalised weights are mapped to the parameters first (the gradient guard
        # then sees the projected ones); the power iteration follows the step -- also a skipped one, on the unchanged weights, so
        # that a recorded launch sequence stays static -- and the operands re-packed are those of the normalised weights
        sn.project()
        opt.step()
        sn.refresh(iterate=True)
        ops.refresh_packed(sn.step_params(self._opt_params(opt)))

    def _sn(self):
        """The spectral-norm controller of a marked ``self.D`` (``spectral.spectral_norm(sg.D)``), or None; refuses the marks this
        trainer does not serve."""
        key = (spectral.marks_epoch(), id(self.G), id(self.D), id(self.E), dp.world_size())
        if self._sn_cache[0] != key:
            self._sn_cache = (key, self._sn_lookup())
        return self._sn_cache[1]

    def _sn_lookup(self):
        for name in ("G", "E"):
            if spectral.find(dp.unwrap(getattr(self, name))):
                raise NotImplementedError(f"SRGAN_training: {name} is marked with spectral_norm; only the discriminator's step maps "
                                          "the gradients and runs the power iteration (spectral.remove_spectral_norm(sg." + name + "))")
        D = dp.unwrap(self.D)
        marks = spectral.find(D)
        if not marks:
            return None
        sn = spectral.controller(D)
        if sn is None or len(marks) != 1:
            raise NotImplementedError("SRGAN_training: a part of D is marked with spectral_norm; one table serves the step -- remove "
                                      "the marks and apply spectral.spectral_norm(sg.D) to the whole discriminator")
        if dp.world_size() > 1:
            raise NotImplementedError(f"SRGAN_training: D is marked with spectral_norm and the process group has {dp.world_size()} "
                                      "ranks; the normalised weights are not in the gradient reducer's buckets yet (run one "
                                      "process, or spectral.remove_spectral_norm(sg.D))")
        return sn

    def _d_frozen(self):
        """What phase 1's pass through D must not compute gradients for: D's parameters and, for a marked D, the normalised
        weights the convolutions read."""
        sn = self._sn()
        return list(self.D.parameters()) + (sn.leaves if sn is not None else [])

    def _reducer(self, name, opt):
        red = self._reducers.get(name)
        if red is None:
            red = self._reducers[name] = dp.GradReducer(self._opt_params(opt))
            ops._sink_alloc = dp.grad_slot      # the weight-gradient kernels of a recorded step write into the bucket slices
        return red

    def _reduce_arm(self, name, opt):
        """before the backward whose gradients `opt` will consume: buckets are all-reduced as they complete"""
        if dp.is_distributed():
            self._reducer(name, opt).arm()

    def _reduce_start(self, name, opt):
        if not dp.is_distributed():
            return None
        red = self._reducer(name, opt)
        red.start()
        return red

    def _encode(self, image, feat=None, noise=None):
        """E(image) -> 5-list; with a precomputed trunk feature only the heads run.  The reparametrisation noise is
        drawn here (CPU default generator, as model.py:461) unless the caller pre-drew it to fix the RNG order."""
        E = dp.unwrap(self.E)
        if feat is None and noise is not None and hasattr(E, "features"):
            feat = E.features(image)
        if feat is not None and hasattr(E, "features"):
            mu, logvar = E.fcmean(feat), E.fcvar(feat)
            eps = noise if noise is not None else self._noise("normal", mu.shape[0])
            return [E.reparam_with(mu, logvar, eps), mu, logvar, E.fcclass(feat), None]
        return list(self.E(image))

    def _mu_pair(self, a, make_b, noise_a, noise_b):
        """mu of E(a) and of E(b), b = make_b(), with pre-drawn reparametrisation noise (fused paths).  Per-sample encoder: b is
        made first and both go through the trunk as ONE batch.  Batch statistics: each forward normalises its own batch and
        advances the running buffers once, so they run one by one in the reference's order -- E(a), what make_b runs, E(b)."""
        if not self._e_per_sample:
            mu_a = self._encode(a, noise=noise_a)[1]
            return mu_a, self._encode(make_b(), noise=noise_b)[1]
        feats = dp.unwrap(self.E).features(ops.cat_batch([a, make_b()]))
        nb = a.shape[0]
        return self._encode(None, feats[:nb], noise_a)[1], self._encode(None, feats[nb:], noise_b)[1]

    def _fused_paths(self):
        """The batched / fused execution needs this package's own modules (feature / logit entry points) and a fused kernel
        kind for BOTH criteria: a criterion without one takes the generic path, whose loss helpers refuse it."""
        return (hasattr(dp.unwrap(self.D), "forward_logits") and self._ref_is_onehot
                and hasattr(dp.unwrap(self.E), "features") and has_fused_kind(self.criterion, "gan")
                and has_fused_kind(self.criterion_class, "class"))

    def _class_is_mse(self):
        """criterion_class is nn.MSELoss() with mean reduction (05-train cell 13): the softmax + MSE instantiation of the fused
        class-loss kernels."""
        c = self.criterion_class
        return isinstance(c, nn.MSELoss) and getattr(c, "reduction", "mean") == "mean"

    def _kinds(self):
        """(gan_kind, class_kind) of the two criteria for the fused loss kernels (raises for a criterion without one)."""
        return (criterion_kind(self.criterion, "gan", "SRGAN_training"),
                criterion_kind(self.criterion_class, "class", "SRGAN_training"))

    def _d_losses(self, image, gan_target, class_which, want_class):
        """GAN loss (+ class loss) of D(image) through the fused head/loss kernels."""
        D = dp.unwrap(self.D)
        if hasattr(D, "forward_logits") and self._ref_is_onehot and has_fused_kind(self.criterion_class, "class"):
            outs, logits = D.forward_logits(image)
            gan = get_loss_D(outs, gan_target, self.criterion, self.device)
            cls = None
            if want_class:
                lab = self._label_dev(class_which)
                w = 1.0 / len(logits)
                ck = criterion_kind(self.criterion_class, "class", "SRGAN_training")
                cls = 0.0
                for z in logits:
                    cls = cls + (ops.softmax_mse(z, lab, w)[0] if ck == ops.CRIT_MSE else ops.softmax_crit(z, lab, w, ck)[0])
            return gan, cls
        outs, probs = self.D(image)
        gan = get_loss_D(outs, gan_target, self.criterion, self.device)
        cls = get_domainloss_D(probs, self._onehot(class_which), self.criterion_class) if want_class else None
        return gan, cls

    # ------------------------------------------------------------------------------------------
    def G_transformation(self, target_label, source_image, encoder=False, ref_image=None, _enc_info=None):
        """Translate ``source_image`` to ``target_label`` with a style code from E(ref_image) (encoder=True) or
        N(0, I) noise drawn on the CPU default generator   (util_notebook.py:510-561).
        Returns (image, info): info = [latent, mu, logvar, class_output, None] or the random latent."""
        if encoder:
            info = _enc_info if _enc_info is not None else self._encode(ref_image)
            latent, mu = info[0], info[1]
            if self.encoded_feature == "latent":
                latent_vector = latent
            elif self.encoded_feature == "mu":
                latent_vector = mu
        else:
            latent_vector = self._noise("randn", source_image.shape[0])
            info = latent_vector
        if isinstance(target_label, str):
            class_vector = self._onehot(target_label)
        else:
            class_vector = class_encode(target_label, self.device, self.ref_label)
        class_vector = torch.cat([class_vector, latent_vector], 1)
        target_image = self.G(source_image, class_vector)
        return target_image, info

    # ------------------------------------------------------------------------------------------
    def update_D(self, _fake=None, _next_fake=None, _defer=False, _index=0):
        """One discriminator update (util_notebook.py:563-594); returns errD.
        Data parallel: ``_fake`` hands in a pre-computed translation, ``_next_fake`` is work to run UNDER this update's gradient
        all-reduce (the next translation: G does not change during the discriminator loop), ``_defer`` leaves the wait for the
        all-reduce and the optimiser step to ``_finish_D()`` so that the caller can put more independent work in between.
        ``_index``: which of the step's k updates this is (the R1 penalty and the consistency terms run on update i iff
        i % every == 0, each with its own every)."""
        self._finish_D()
        self.D.zero_grad()
        sn = self._sn()
        if sn is not None:
            sn.zero_grad()                                 # the normalised weights are not parameters: D.zero_grad() misses them
        if _fake is None:
            self.target_image, self.c_rand = self.G_transformation("target", self.source_image, False)
        else:
            self.target_image, self.c_rand = _fake

        if self._ada is not None:
            self._ada_check()
        cr = self.bcr if self.bcr is not None and _index % self.bcr.every == 0 else None
        if self.bcr is not None:
            self._bcr_check()
        lc = self._lecam
        if lc is not None:
            self._lecam_check()
        if self._fused_paths():
            # real and fake halves through D as ONE batch (per-sample network: exact; 2x the rows per GEMM launch)
            B = self.source_image.shape[0]
            rest = [s for s in self._stages() if s is not self.augment]
            staged = any(self._stage_on(s) for s in self._stages())
            _, _, h, w = self.source_image.shape
            if cr is not None and not staged:
                # consistency pairs straight from the two halves: [real | fake | T(real) | T(fake)] in the launch that would have
                # concatenated them (tables: real rows, then fake rows, from the pairs' own generator)
                d_in = ops.cr_pairs([self.source_image.detach(), self.target_image.detach()],
                                    self._stage_tables(cr.stage, 2, B, h, w), cr.stage.flags)
            elif self._stage_on(self.augment):
                # both halves augmented and concatenated in ONE pass (no gradient needed: real rows have none, fake rows are detached)
                # adaptive augmentation: the two tables went through one gate launch of 2B rows (_stage_tables)
                d_in = ops.diffaugment_cat([self.source_image.detach(), self.target_image.detach()],
                                           self._stage_tables(self.augment, 2, B, h, w), self.augment.flags, self.augment.cut(h, w),
                                           gated=self._ada is not None)
            else:
                d_in = ops.cat_batch([self.source_image, self.target_image.detach()])
            d_in = self._aug(d_in, 2, rest)                # the remaining stages on the 2B rows: one launch each, tables real then fake
            if cr is not None and staged:
                # the partners are made of what D reads AFTER every stage: one more launch, the front 2B rows a bit copy
                d_in = ops.cr_pairs([d_in], self._stage_tables(cr.stage, 2, B, h, w), cr.stage.flags)
            # what D read as the real rows (the R1 penalty is taken there)
            d_real = d_in[:B] if staged else self.source_image
            outs, logits = dp.unwrap(self.D).forward_logits(d_in)
            if self._ada is not None:
                # the overfitting heuristic on what D says about the real rows; every interval-th call moves p, so the p that
                # gated THIS update's input is the one from before this observation
                self._ada.observe(outs, B, _adamod.threshold(self._kinds()[0]))
                self.loss_terms["ada_p"] = self._ada.p_tensor()
            # criterion(real, 1) + class loss * lbd + criterion(fake, 0) over both scales, values and gradients: one launch
            if cr is None and lc is not None:
                # the same launch, then the LeCam term on the same maps (anchors, settings and the warm-up count from its device
                # record), its gradient added into the buffers the backward scales; errD stays the value without it
                loss_D, parts = ops.d_losses(outs, logits, self._label_dev("source"), B, 1., 0., self.lbd["class"], *self._kinds(),
                                             lecam=lc.arg(outs[0].device))
                errD = parts[3]
                self.loss_terms["errD_lecam"] = parts[4]
            elif cr is None:
                errD, parts = ops.d_losses(outs, logits, self._label_dev("source"), B, 1., 0., self.lbd["class"], *self._kinds())
                loss_D = errD
            else:
                # the same over the front 2B rows, plus the consistency terms between row n and row n + 2B and their gradients
                # (weights from the device record), still one launch; errD stays the value without them
                # (LeCam, if on, follows on the front 2B rows)
                loss_D, parts = ops.d_losses_cr(outs, logits, self._label_dev("source"), B, 1., 0., self.lbd["class"],
                                                cr._ensure(outs[0].device), *self._kinds(),
                                                lecam=lc.arg(outs[0].device) if lc is not None else None)
                errD = parts[3]
                self.loss_terms.update(errD_cr_real=parts[4], errD_cr_fake=parts[5])
                if lc is not None:
                    self.loss_terms["errD_lecam"] = parts[7]
            errD_real, errD_class, errD_fake = parts[0], parts[1], parts[2]
        else:
            d_real = self._aug(self.source_image)
            errD_real, errD_class = self._d_losses(d_real, 1., "source", True)
            errD_fake, _ = self._d_losses(self._aug(self.target_image.detach()), 0., None, False)
            errD = errD_real + errD_class * self.lbd["class"] + errD_fake
            loss_D = errD
        self._reduce_arm("D", self.optD)
        with ops.fused_param_grads(not dp.hooks_need_live_grads(), self.device):
            loss_D.backward()
        if self._r1 is not None and _index % self._r1.every == 0:
            # R1 on the real rows D just read: dP/dW is added to the gradients the backward left, before the optimiser step (and
            # so before the spectral-norm projection and the gradient guard); errD is unchanged
            self._r1_check()
            _r1mod.r1_accumulate(dp.unwrap(self.D), d_real.detach(), self._r1)
            self.loss_terms["errD_r1"] = self._r1.penalty()
        self._d_pending = self._reduce_start("D", self.optD) or True
        dp.launch_pending()                                         # recorded step: the all-reduces start here ...
        nxt = _next_fake() if _next_fake is not None else None      # ... and this runs under them
        if not _defer:
            self._finish_D()
        self.loss_terms.update(errD_real=errD_real.detach(), errD_class=errD_class.detach(), errD_fake=errD_fake.detach())
        return (errD, nxt) if _next_fake is not None else errD

    def _finish_D(self):
        """Wait for the discriminator's gradient all-reduce (if any) and take its optimiser step, if an ``update_D`` left them."""
        red, self._d_pending = self._d_pending, None
        if red is None:
            return
        if red is not True:
            red.finish()
        self._step(self.optD)

    # ------------------------------------------------------------------------------------------
    def update_GandE(self):
        """Generator + encoder update in two phases (util_notebook.py:596-694); returns [errG, errE_output]."""
        L = self.lbd
        self.G.zero_grad()
        self.E.zero_grad()
        E = dp.unwrap(self.E)
        src = self.source_image
        ws = dp.world_size()

        # ---------------- phase 1: G and E ----------------
        optE_ids = {id(p) for p in self._opt_params(self.optE)}
        e_unused = [p for p in self.E.parameters() if p.requires_grad and id(p) not in optE_ids]
        with _frozen(e_unused):
            feat = E.features(src) if hasattr(E, "features") else None
            source_enc_info = self._encode(src, feat)
            pair = feat is not None and L["idt"] > 0 and self._g_per_sample and self._e_per_sample
            # Recorded data-parallel step (round 4): phase 1 reaches the kept target_image graph LAST in its backward (autograd
            # runs the youngest nodes first and that graph was built in the last discriminator update) -- after E's gradients are
            # final.  The pass is cut there: phase 1 reads target_image through a detached alias, the first backward stops at the
            # alias, E's all-reduce is started on the communication stream, and the stale graph is back-propagated from the
            # alias's gradient UNDER it (the same two contributions summed in the same order: the alias's gradient is what the
            # engine's input buffer would hold).
            cut = pair and dp.recording() and self.target_image.requires_grad
            t_img = self.target_image.detach().requires_grad_(True) if cut else self.target_image
            ms = self._ms
            i2 = z2 = None
            if ms is not None:
                # mode seeking: the second translation of the source, by the G that made target_image (no optimiser step has run
                # since), under a second latent code from the feature's own generator
                self._ms_check()
                z2 = self._stage_tables(ms, 1, src.shape[0], src.shape[2], src.shape[3])
                c2 = torch.cat([self._onehot("target"), z2], 1)
            if pair:
                # the reference calls E(source) a second time for the identity path: same weights, same input -> same
                # mu; only the reparametrisation noise is drawn again (keeps the CPU RNG sequence identical).  The
                # reconstruction G(target_image, c) and the identity G(source, c') then run as ONE batch through G.
                idt_info = self._encode(src, feat)
                pick = 0 if self.encoded_feature == "latent" else 1
                oh = self._onehot("source")
                c_pair = torch.cat([torch.cat([oh, source_enc_info[pick]], 1), torch.cat([oh, idt_info[pick]], 1)], 0)
                nb = src.shape[0]
                if ms is not None and self._ms_rides(nb, src):
                    # ... and the second translation as a third group of rows: per-sample network, so exact, and no convolution
                    # launch more than the step without the feature
                    both = self.G(ops.cat_batch([t_img, src, src]), torch.cat([c_pair, c2], 0))
                    i2 = both[2 * nb:]
                else:
                    both = self.G(ops.cat_batch([t_img, src]), c_pair)
                recon_image, identity_image = both[:nb], both[nb:2 * nb]
            else:
                recon_image, _ = self.G_transformation("source", self.target_image, True, src, _enc_info=source_enc_info)
            if ms is not None and i2 is None:
                i2 = self.G(src, c2)                       # a forward of its own: no batched pass, or 3B rows would cross 4 GiB
            self._finish_D()                               # (data parallel: the last D update's all-reduce ran under the passes above)
            fused = self._fused_paths()
            # loss terms as (device scalar, weight) lists: the optimised sums and the two reported sums are each ONE launch
            # (ops.lincomb) instead of one launch per python-level `+` / `*`
            g_terms, e_terms, rep_terms = [], [], []
            with _frozen(self._d_frozen()):                # D's weight grads would be discarded
                d_img = self._aug(t_img)                   # (the step's last table; the generator's gradient flows back through it)
                if fused:
                    outs, logits = dp.unwrap(self.D).forward_logits(d_img)
                    d_total, parts = ops.d_losses(outs, logits, self._label_dev("target"), self.target_image.shape[0], 1., 0., L["class"],
                                                  *self._kinds())
                    errG_dis, errG_class = parts[0], parts[1]
                    g_terms.append((d_total, 1.0))
                else:
                    errG_dis, errG_class = self._d_losses(d_img, 1., "target", True)
                    g_terms += [(errG_dis, 1.0), (errG_class, L["class"])]
            errG_cycle = ops.l1_mean(src, recon_image, 1.0)
            g_terms.append((errG_cycle, L["cycle"]))
            rep_terms.append((errG_cycle, L["cycle"]))
            terms = dict(errG_dis=errG_dis, errG_class=errG_class, errG_cycle=errG_cycle)
            ss_terms = []
            if self._ssim is not None and "cycle" in self._ssim_on:
                # weight * (1 - SSIM(src, recon_image)) from the device record, optimised with weight 1 beside the L1 term; the
                # gradient reaches the reconstruction only (src is data).  errG and errE_output stay the reference's sums.
                ss_weighted, ss_term = self._ssim.loss(src.detach(), recon_image)
                ss_terms.append((ss_weighted, 1.0))
                terms["errG_ssim_cycle"] = ss_term

            _, mu, logvar, _, _ = source_enc_info
            if L["KL"] > 0:
                # a SUM over the rows of the batch (util_notebook.py:630-634): under data parallelism each rank holds the
                # sum over ITS rows and the gradient all-reduce averages, so the optimised term is pre-scaled by the world
                # size (as the batch-statistics losses below); the reported value stays the local sum
                errE_KL = ops.kl_normal(mu, logvar)
                e_terms.append((errE_KL, L["KL"] * ws if ws > 1 else L["KL"]))
                rep_terms.append((errE_KL, L["KL"]))
                terms["errE_KL"] = errE_KL

            if L["idt"] > 0:
                if not pair:
                    # batch statistics: the reference's second E(source) is a train-mode forward of its own (it advances E's
                    # running buffers again), then G(source) runs as its own batch
                    info = self._encode(src, noise=self._noise("normal", src.shape[0])) if feat is not None else None
                    identity_image, _ = self.G_transformation("source", src, True, src, _enc_info=info)
                errG_idt = ops.l1_mean(src, identity_image, 1.0)
                g_terms.append((errG_idt, L["idt"]))
                rep_terms.append((errG_idt, L["idt"]))
                terms["errG_idt"] = errG_idt
                if self._ssim is not None and "idt" in self._ssim_on:
                    ss_weighted, ss_term = self._ssim.loss(src.detach(), identity_image)
                    ss_terms.append((ss_weighted, 1.0))
                    terms["errG_ssim_idt"] = ss_term
            elif self._ssim is not None and "idt" in self._ssim_on:
                raise RuntimeError(self._SSIM_IDT_OFF)

            if L["batch_KL"] > 0:
                w_corr = L["corr_enc"] if L["corr_enc"] > 0 else 0.0
                w_hist = L["hist"] if L["hist"] > 0 else 0.0
                target = self.hi.target if w_hist > 0 else torch.full((50,), 0.02, device=mu.device)
                mu_all = dp.all_gather_rows(mu)
                total, parts, _ = ops.latent_losses(mu_all, self.n_batch, target, L["batch_KL"], w_corr, w_hist)
                # every rank evaluates the global-batch loss; its local rows' gradient must be SUMMED over ranks
                # while the all-reduce averages -> pre-scale by the world size
                e_terms.append((total, float(ws) if ws > 1 else 1.0))
                rep_terms.append((total, 1.0))
                terms.update(errE_bKL=parts[0], errE_corr=parts[1], errE_hist=parts[2])

            ms_terms = []
            if ms is not None:
                # weight * ms from the device record, optimised with weight 1; its gradient reaches G through i2's graph and
                # through the kept target_image graph, never E or D.  errG stays the reference's sum without it.
                ms_weighted, ms_value = ms.loss(t_img, i2, self.c_rand, z2)
                ms_terms.append((ms_weighted, 1.0))
                terms["errG_ms"] = ms_value
            total_p1 = ops.lincomb(g_terms + ms_terms + ss_terms + e_terms)
            with torch.no_grad():
                errG = ops.lincomb(g_terms)
                errE_output = ops.lincomb(rep_terms)
            self._reduce_arm("G", self.optG)
            self._reduce_arm("E", self.optE)
            # the generator's weights are reached twice in this pass (reconstruction / identity graph and the kept target_image
            # graph): their weight-gradient kernels add the second contribution themselves (ops.fused_param_grads)
            with ops.fused_param_grads(not dp.hooks_need_live_grads(), self.device):
                total_p1.backward(retain_graph=True)     # target_image's graph is needed again in phase 2
            redE = None
            if cut:
                # E's gradients are final: flatten its buckets and start their all-reduce (a cut of the recording), then run the
                # stale-graph generator backward under it; the generator's parameters take their second contribution on top of
                # the first (ops.fused_param_grads(seed=True): the weight-gradient kernels add into p.grad)
                redE = self._reduce_start("E", self.optE)
                dp.launch_pending()
                with ops.fused_param_grads(True, self.device, seed=True):
                    self.target_image.backward(t_img.grad, retain_graph=True)
        # Data parallel: E's buckets go out first, G's behind them on the same communication stream; E's optimiser step, its
        # repack and phase 2's E(source) forward (which needs the new E, not the new G) then run UNDER G's all-reduce.  The two
        # Adam steps touch disjoint parameters, so their order does not matter.
        if redE is None:
            redE = self._reduce_start("E", self.optE)
        redG = self._reduce_start("G", self.optG)
        dp.launch_pending(then_wait=redE)
        if redE is not None:
            redE.finish()
        self._step(self.optE)
        do_idt_reg = L["idt_reg"] * L["idt"] > 0
        info = reg_noise = None
        if redG is not None and do_idt_reg and self._fused_paths() and self._e_per_sample:
            reg_noise = [self._noise("normal", src.shape[0]) for _ in range(3)]     # reference order: E(target_image), E(source), E(idt_random_image)
            with _frozen(list(self.E.parameters())), torch.no_grad():
                info = self._encode(src, noise=reg_noise[1])
        if redG is not None:
            redG.finish()
        self._step(self.optG)

        # ---------------- phase 2: G only ----------------
        self.G.zero_grad()
        self.E.zero_grad()
        with _frozen(list(self.E.parameters())):           # only optG steps: E's weight grads are discarded
            if do_idt_reg and self._fused_paths():
                # reference order of the noise draws: E(target_image), E(source), E(idt_random_image); data parallel: drawn above
                n1, n2, n3 = reg_noise or [self._noise("normal", src.shape[0]) for _ in range(3)]

                def translate_source():
                    nonlocal info
                    if info is None:
                        with torch.no_grad():               # its gradient only reaches E's parameters
                            info = self._encode(src, noise=n2)
                    return self.G_transformation("source", src, True, src, _enc_info=info)[0]

                target_cenc, idt_cenc_rand = self._mu_pair(self.target_image, translate_source, n1, n3)
                errG_reg = ops.l1_mean(self.c_rand, target_cenc, 1.0)
                errG_idt_reg = ops.l1_mean(info[1], idt_cenc_rand, 1.0)
                errG_ex = ops.lincomb([(errG_reg, L["reg"]), (errG_idt_reg, L["idt_reg"] * (L["idt"] / L["cycle"]))])
                terms["errG_reg"], terms["errG_idt_reg"] = errG_reg, errG_idt_reg
            else:
                _, target_cenc, _, _, _ = self._encode(self.target_image)
                errG_reg = ops.l1_mean(self.c_rand, target_cenc, 1.0)
                errG_ex = errG_reg * L["reg"]
                terms["errG_reg"] = errG_reg
                if do_idt_reg:
                    with torch.no_grad():                   # its gradient only reaches E's parameters
                        info = self._encode(src)
                    idt_random_image, info = self.G_transformation("source", src, True, src, _enc_info=info)
                    source_c_rand = info[1]
                    _, idt_cenc_rand, _, _, _ = self._encode(idt_random_image)
                    errG_idt_reg = ops.l1_mean(source_c_rand, idt_cenc_rand, 1.0)
                    errG_ex = errG_ex + errG_idt_reg * (L["idt_reg"] * (L["idt"] / L["cycle"]))
                    terms["errG_idt_reg"] = errG_idt_reg
            self._reduce_arm("G", self.optG)
            with ops.fused_param_grads(not dp.hooks_need_live_grads(), self.device):
                errG_ex.backward()
        redG = self._reduce_start("G", self.optG)
        if redG is not None:
            redG.finish()
        self._step(self.optG)

        self.recon_image = recon_image.detach()
        self.loss_terms.update({k: v.detach() for k, v in terms.items()})
        with torch.no_grad():
            errG = ops.lincomb([(errG, 1.0), (errG_ex, 1.0)])
        return [errG, errE_output.detach()]

    # ------------------------------------------------------------------------------------------
    def UnrolledUpdate(self):
        """k discriminator updates then one G/E update (util_notebook.py:696-728).  The reference then
        "restores" D from ``paramD = self.D.state_dict()``, which aliases the live tensors -- a no-op that
        is not replayed here.  Returns [errorG, errorD(first iteration), errorE]."""
        src, k = self.source_image, self.k
        nb = src.shape[0]
        # G does not change during the k discriminator updates, so all k translations are computed up front, with the
        # noise drawn in the reference's order (k x randn(B, ndim) on the CPU generator).  Only the LAST translation's
        # graph is ever back-propagated (phases 1 and 2); the first k-1 run as ONE no-grad batch of (k-1)*B images.
        noises = [self._noise("randn", nb) for _ in range(k)]
        oh = self._onehot("target")
        if dp.is_distributed():
            # Data parallel: every discriminator update ends in a gradient all-reduce, and the only work of the loop that does
            # not depend on it is the NEXT translation (G is fixed during the loop).  So the translations run one at a time, each
            # under the previous update's all-reduce; the last update's all-reduce runs under the encoder / generator forward
            # passes of phase 1 (update_GandE calls _finish_D() right before it needs the updated discriminator).
            def translate(i):
                with torch.set_grad_enabled(i == k - 1):       # the last one's graph is what phases 1 and 2 back-propagate
                    return self.G(src, torch.cat([oh, noises[i]], 1)), noises[i]

            fake = translate(0)
            for i in range(k):
                nxt = (lambda j=i + 1: translate(j)) if i + 1 < k else None
                out = self.update_D(_fake=fake, _next_fake=nxt, _defer=(i == k - 1), _index=i)
                errD, fake = out if nxt is not None else (out, None)
                if i == 0:
                    errorD = errD.detach()
        else:
            fakes = []
            if k > 1 and isinstance(dp.unwrap(self.G), SingleGenerator) and self._g_per_sample:   # per-sample network: batching is exact
                # the kernels address an activation with 32-bit byte offsets (< 4 GiB per tensor): translations are batched in
                # groups whose widest activation (the first conv's nch planes at full resolution) stays under that, e.g.
                # 256x256, B=64, k=5 runs as two groups of 2*B images instead of one of 4*B
                Gm = dp.unwrap(self.G)
                widest = max(int(Gm.down_convs[0].weight.shape[0]), 3) * src.shape[2] * src.shape[3] * 4
                per_group = max(1, min(k - 1, (((1 << 32) - (1 << 26)) // widest) // nb))
                with torch.no_grad():
                    for lo in range(0, k - 1, per_group):
                        zs = noises[lo:min(lo + per_group, k - 1)]
                        c_all = torch.cat([torch.cat([oh, z], 1) for z in zs], 0)
                        imgs = self.G(ops.cat_batch([src] * len(zs)) if len(zs) > 1 else src, c_all)
                        fakes += [(imgs[i * nb:(i + 1) * nb], z) for i, z in enumerate(zs)]
            elif k > 1:
                with torch.no_grad():
                    fakes = [(self.G(src, torch.cat([oh, z], 1)), z) for z in noises[:-1]]
            fakes.append((self.G(src, torch.cat([oh, noises[-1]], 1)), noises[-1]))
            for i in range(k):
                errD = self.update_D(_fake=fakes[i], _index=i)
                fakes[i] = None
                if i == 0:
                    errorD = errD.detach()
        errorG, errorE = self.update_GandE()
        if self._ema is not None:
            # one EMA update per train() (one iteration of the reference's loop), after phase 2's optG.step(): on the step's
            # stream, inside its ops.pack_cache() scope and inside its recording.  Two launches, none with the EMA off.
            self._ema.update()
        return [errorG, errorD, errorE]

    def train(self, source_image, label):
        if self._ema_scope:
            raise RuntimeError("SRGAN_training.train() inside ema_weights(): self.G / self.E are the averaged copies there")
        self.label = label
        self.loss_terms = {}
        g = self._graph
        sn = self._sn()
        if sn is not None:
            sn._ensure()               # a state dict loaded since the last step: sigma and the normalised weights follow it
        if g is not None and g.accepts(source_image, label):
            return g.run(source_image, label)
        if g is not None:
            g.before_eager_step()
        self._g_active = False
        self.source_image = ops.to_nhwc(source_image)
        with ops.pack_cache():        # weights only change at self._step() inside this scope
            error = self.UnrolledUpdate()
        if g is not None:
            g.note_eager_step(source_image, label)
        return error

    # ------------------------------------------------------------------------------------------
    # hipGraph mode (BASELINE configs[4]: "hipGraph step"; the step captured is util_notebook.py:696-734)
    def enable_graph(self):
        """From now on ``train()`` replays the whole step -- k discriminator updates, both generator / encoder phases, the
        optimiser steps and weight repacks, ~1900 launches -- as ONE captured hipGraph.  The first call with a given input
        shape still runs eagerly (it creates the optimiser state, packed operands and workspaces a capture must not
        re-create), the second captures and replays, later ones only stage the step's inputs (image batch, labels, the
        CPU-generator noise drawn in the reference's order) into static device buffers and launch the graph.  Inputs of
        another shape (an epoch's last partial batch) run eagerly.  Results are bit-identical to eager execution.
        Under a process group the recording is cut where a collective starts and where its result is needed, so that the
        all-reduces run UNDER the following segment (``step_graph._Recording``, ``dp.launch_pending``); if any rank fails to
        record, all ranks drop graph mode together and continue eagerly (``SRGAN_DP_GRAPH=0`` refuses graph mode under a process
        group altogether).  Networks marked with ``dp.sync_batch_stats`` are recorded only in the single-graph form of the C-ABI
        transport and run eagerly otherwise (``step_graph._StepGraph.SEGMENTED_SYNC``)."""
        self._graph = _StepGraph(self)
        return self

    def disable_graph(self):
        if self._graph is not None:
            self._graph.before_eager_step()
        self._graph = None
        self._g_active = False

    @property
    def graph_active(self):
        return self._graph is not None and self._graph.graph is not None

    # ------------------------------------------------------------------------------------------
    # exponential moving average of the sampling weights (extension, no counterpart in the reference; srgan_amd.ema)
    def enable_ema(self, decay=0.999, nets=("G", "E"), ramp=True):
        """Keep ``self.G_ema`` / ``self.E_ema`` (``None`` for a network not in ``nets``): copies of the live G / E at their
        current weights -- same class and ``state_dict()`` layout, eval mode, no gradients -- that every ``train()`` from now on
        moves by ``e <- e + (1 - d_n) * (p - e)``, ``d_n = min(decay, (1 + n) / (10 + n))`` with ``ramp`` (n = 1, 2, ... counts
        the updates) or ``decay`` without; batch-norm buffers are carried over.  Two launches per step for everything, captured
        with the step in graph mode (a recording made before is dropped).  Live weights, losses and optimiser states are
        bit-identical to a run without it.  Under a process group every rank keeps its own, identical copies."""
        nets = tuple(nets)
        if not nets or any(n not in ("G", "E") for n in nets) or len(set(nets)) != len(nets):
            raise ValueError("enable_ema: nets is a non-empty selection of 'G' and 'E'")
        if self._ema_scope:
            raise RuntimeError("enable_ema inside ema_weights()")
        self._ema = ema.WeightEMA({n: getattr(self, n) for n in ("G", "E") if n in nets}, decay, ramp)
        self.G_ema, self.E_ema = self._ema.twins.get("G"), self._ema.twins.get("E")
        return self

    def disable_ema(self):
        if self._ema_scope:
            raise RuntimeError("disable_ema inside ema_weights()")
        self._ema = None
        self.G_ema = self.E_ema = None

    @property
    def ema_updates(self):
        """Updates done so far (host mirror of the device record's n)."""
        return self._ema.updates if self._ema is not None else 0

    def _need_ema(self, what):
        if self._ema is None:
            raise RuntimeError(f"{what}: the EMA is off (enable_ema)")
        return self._ema

    def set_ema_decay(self, decay):
        """Write a new decay into the device record, between steps; a recorded step reads it from there and stays valid."""
        self._need_ema("set_ema_decay").set_decay(decay)

    def ema_state_dict(self):
        """{"G": state_dict, "E": state_dict (the selected ones), "updates", "decay", "ramp"} -- a snapshot (cloned tensors)."""
        return self._need_ema("ema_state_dict").state_dict()

    def load_ema_state_dict(self, sd):
        """Restore ``ema_state_dict()``; enables the EMA for the networks ``sd`` holds if it is off.  The copies are written in
        place and the device record is re-seeded in place (outside any capture)."""
        nets = tuple(n for n in ("G", "E") if n in sd)
        if self._ema is None or tuple(self._ema.twins) != nets:
            self.enable_ema(sd["decay"], nets, sd["ramp"])
        self._ema.load_state_dict(sd)

    # ------------------------------------------------------------------------------------------
    # differentiable augmentation of what D reads (extension, no counterpart in the reference; srgan_amd.augment)
    def enable_diffaugment(self, policy="color,translation,cutout", translation=0.125, cutout=0.5, seed=None):
        """From now on every batch the discriminator reads -- the real and the fake rows of each of the k discriminator updates and
        phase 1's D(target_image) -- goes through DiffAugment (random colour, translation, cutout per sample; ``policy``: any
        comma-separated subset, '' = none), and the generator's gradient flows back through it.  ``self.augment`` is the
        ``augment.DiffAugment`` that draws the parameters: 2k + 1 tables of [B, 8] per step (per update real, then fake; then phase
        1) from its OWN generator (``seed``), so the step's style and reparametrisation noise is what it is with the feature off.
        2(k + 1) + 2 launches per step; captured with the step in graph mode, where the tables are staged like the noise (a
        recording made before is dropped).  With the feature off, or an empty policy, the step is bit-identical to the plain one.
        Data parallel: the operation is per sample, every rank draws its own tables."""
        self.augment = DiffAugment(policy, translation, cutout, seed)
        self._guard_changed()
        return self

    def disable_diffaugment(self):
        """Also turns the adaptive probability off (``enable_ada``): there is nothing left to gate."""
        self.augment = None
        self._ada = None
        self._guard_changed()

    # ------------------------------------------------------------------------------------------
    # geometric augmentation of what D reads (extension, no counterpart in the reference; srgan_amd.augment.GeometricAugment)
    def enable_geometric_augment(self, policy="flip,rot90,scale,rotate", scale_std=0.2, rotate_max=1.0, seed=None):
        """From now on every batch the discriminator reads goes, AFTER DiffAugment's pass (or as it is, with DiffAugment off), through
        one bilinear affine warp per sample: x-flip, 90-degree turns, isotropic scale (``zoom = 2 ** (N(0, 1) * scale_std)`` in
        [0.5, 2]) and rotation by ``U(-pi, pi) * rotate_max`` (``policy``: any comma-separated subset, '' = none); pixels outside
        the image read 0, and the generator's gradient flows back through the warp (a gather: no atomics, a fixed order).
        ``self.geometry`` is the ``augment.GeometricAugment`` that draws the parameters: 2k + 1 tables of [B, 8] per step, in
        DiffAugment's order, from its OWN generator (``seed``) -- DiffAugment's tables and the step's noise are what they are
        without it.  k + 1 forward launches and 1 backward per step (the 2B rows of a discriminator update in one launch); captured
        with the step in graph mode, where the tables are staged beside DiffAugment's (a recording made before is dropped); saved
        in a checkpoint (section ``geometry``).  With ``enable_ada`` on the four groups are gated per sample by the same p as
        DiffAugment's (k + 1 more gate launches, four uniforms per sample after each table); ``enable_ada`` itself still asks for a
        non-empty DiffAugment policy.  ``rot90`` and ``rotate`` applied always (without ``enable_ada``) leak into the generated
        images in the ADA paper's sense; ``flip`` is safe on flip-symmetric data.  R1 penalises at what D read.  Off, or an empty
        policy: no draw, no launch, no allocation, the step is bit-identical to the one without.  Data parallel: per sample, every
        rank draws its own tables."""
        self.geometry = GeometricAugment(policy, scale_std, rotate_max, seed)
        self._guard_changed()
        return self

    def disable_geometric_augment(self):
        self.geometry = None
        self._guard_changed()

    # ------------------------------------------------------------------------------------------
    # adaptive augmentation probability (extension, no counterpart in the reference; srgan_amd.ada)
    def _ada_check(self):
        if not self._stage_on(self.augment):
            raise NotImplementedError("SRGAN_training: the adaptive probability gates DiffAugment's groups and "
                                      + ("DiffAugment is off" if self.augment is None else "its policy is empty")
                                      + " (enable_diffaugment(policy=...) first, or disable_ada())")
        if dp.is_distributed():
            raise NotImplementedError("SRGAN_training: the adaptive probability is on under a process group of several ranks; p "
                                      "and the heuristic's counters would have to be agreed across the ranks (run one process, or "
                                      "disable_ada())")
        if not self._fused_paths():
            raise NotImplementedError("SRGAN_training: the adaptive probability is wired into the fused discriminator pass only "
                                      "(this package's own G / D / E modules with forward_logits, a one-hot ref_label, criteria "
                                      "with a fused kernel); use those, or disable_ada()")

    def enable_ada(self, target=0.6, interval=4, kimg=500.0, p=0.0, p_max=0.8):
        """Adaptive discriminator augmentation (Karras et al., 2020) on top of ``enable_diffaugment``: from now on each group of the
        policy is applied to a sample with probability p instead of always, and p follows the overfitting heuristic
        ``r = E[sign(D(real) - thr)]`` over the real rows of both scales (thr: 0.5 for nn.MSELoss, 0 for nn.BCEWithLogitsLoss):
        every ``interval`` discriminator updates p moves by ``step = B * interval / (kimg * 1000)`` up if ``r > target``, down if
        ``r < target``, inside [0, ``p_max``].  p, the counters and the per-sample decisions are device state (``srgan_amd.ada``,
        ``csrc/ada.hip``): captured with the step in graph mode (a recording made before is dropped), saved in a checkpoint.  Each
        table is followed by three uniforms per sample from the augmentation's own generator; k observe + (k + 1) gate launches
        per step (and k copies of p: ``loss_terms["ada_p"]``, a device scalar, is p after the step's last update).  The p that
        gated an update's input is the one from before that update's observation.  R1 on top penalises at what D read.  Off:
        draws, rows and launches are exactly DiffAugment's.  Refused: DiffAugment off or an empty policy, more than one rank,
        the generic (non-fused) discriminator path."""
        state = _adamod.AdaptiveP(target, interval, kimg, p, p_max)
        self._ada = state
        try:
            self._ada_check()
        except NotImplementedError:
            self._ada = None
            raise
        self._guard_changed()
        return self

    def disable_ada(self):
        self._ada = None
        self._guard_changed()

    def _need_ada(self, what):
        if self._ada is None:
            raise RuntimeError(f"{what}: the adaptive probability is off (enable_ada)")
        return self._ada

    def set_ada_p(self, p):
        """Write a new p into the device record, between steps; a recorded step reads it from there and stays valid."""
        self._need_ada("set_ada_p").set_p(p)

    def set_ada_target(self, target):
        """Write a new target into the device record, between steps; a recorded step reads it from there and stays valid."""
        self._need_ada("set_ada_target").set_target(target)

    def ada_stats(self):
        """The controller's device record as a dict (``p``, ``target``, ``step``, ``p_max``, ``interval``, ``seen``, ``n_pos``,
        ``n_neg``, ``n_total``, ``adjustments``, ``last_r``), or None with the feature off.  SYNCHRONISES the stream."""
        return self._ada.stats() if self._ada is not None else None

    # ------------------------------------------------------------------------------------------
    # R1 gradient penalty on the real rows (extension, no counterpart in the reference; srgan_amd.r1)
    def _r1_check(self):
        if dp.world_size() > 1:
            raise NotImplementedError(f"SRGAN_training: the R1 penalty is on and the process group has {dp.world_size()} ranks; the "
                                      "penalty's gradients are not ordered against the gradient reducer's buckets (run one "
                                      "process, or disable_r1())")
        _r1mod._layers(dp.unwrap(self.D))

    def enable_r1(self, gamma=10.0, every=1):
        """From now on discriminator update ``i`` of a step's k adds the gradient of the R1 penalty ``gamma_eff / 2 * mean_n
        |grad_x S_n|^2`` (``S_n``: the patch MEAN of the two GAN heads at real row n, ``gamma_eff = gamma * every``: lazy
        regularisation) to D's gradients iff ``i % every == 0``, between ``errD.backward()`` and the optimiser step; the gradient
        guard and the spectral-norm projection see the penalised gradients.  ``errD`` and the returned losses are unchanged;
        ``loss_terms["errD_r1"]`` is the penalty of the step's last penalised update (a device scalar).  With DiffAugment on the
        penalty is taken at the AUGMENTED real rows D read in that update (same table) -- a departure from the DiffAugment
        paper, which penalises at the raw images.  Closed form on the existing convolution kernels plus ``csrc/r1.hip``
        (``srgan_amd.r1``), no double backward; captured with the step in graph mode (a recording made before is dropped).  Off:
        no launch, no allocation, the step is bit-identical to the plain one.  Refused: more than one rank, the bf16 compute
        mode (when the step runs), a discriminator other than ``SingleDiscriminator_solo_multi``, images whose H or W is not a
        multiple of 16 (when the step runs)."""
        state = _r1mod.R1Penalty(gamma, every)
        self._r1 = state
        try:
            self._r1_check()
        except NotImplementedError:
            self._r1 = None
            raise
        self._guard_changed()
        return self

    def disable_r1(self):
        self._r1 = None
        self._guard_changed()

    def set_r1_gamma(self, gamma):
        """Write a new ``gamma`` into the penalty's device record, between steps; a recorded step reads it from there and stays
        valid."""
        if self._r1 is None:
            raise RuntimeError("set_r1_gamma: the R1 penalty is off (enable_r1)")
        self._r1.set_gamma(gamma)

    def r1_stats(self):
        """The penalty's device record as a dict (``gamma``, ``every``, ``c``, ``penalty``, ``mean_sq_norm``, ``updates``, ``n``), or
        None with the feature off.  The only host look at the record: SYNCHRONISES the stream."""
        return self._r1.stats() if self._r1 is not None else None

    # ------------------------------------------------------------------------------------------
    # balanced consistency regularisation of D (extension, no counterpart in the reference; srgan_amd.consistency)
    def _bcr_check(self):
        if dp.world_size() > 1:
            raise NotImplementedError(f"SRGAN_training: consistency regularisation is on and the process group has {dp.world_size()} "
                                      "ranks; the doubled discriminator batch is not ordered against the gradient reducer's buckets "
                                      "(run one process, or disable_bcr())")
        if not self._fused_paths():
            raise NotImplementedError("SRGAN_training: consistency regularisation is wired into the fused discriminator pass only "
                                      "(this package's own G / D / E modules with forward_logits, a one-hot ref_label, criteria "
                                      "with a fused kernel); use those, or disable_bcr()")

    def enable_bcr(self, lambda_real=10.0, lambda_fake=10.0, every=1, policy="flip,translation", translation=0.125, seed=None):
        """Balanced consistency regularisation (Zhang et al., 2020; Zhao et al., 2020): from now on discriminator update ``i`` of a
        step's k reads ``[real | fake | T(real) | T(fake)]`` -- 4B rows, the front 2B exactly what it reads anyway, after every
        augmentation stage that is on -- iff ``i % every == 0`` and back-propagates ``errD + every * (lambda_real * cr_real +
        lambda_fake * cr_fake)``, ``cr = mean over the scales and the samples of (m_s(x) - m_s(T(x)))^2`` with ``m_s`` the patch
        mean of scale s's GAN map (the score R1 uses).  ``T`` is an x-flip (probability 1/2) and an integer translation by up to
        ``int(size * translation + 0.5)`` pixels with zeros shifted in (``policy``: any comma-separated subset of ``flip``,
        ``translation``), one draw per row from the regulariser's OWN generator (``seed``): two tables per penalised update (real
        rows, then fake rows), none for phase 1; the step's noise and the other stages' tables are what they are without it, and
        the adaptive probability never gates ``T``.  ``T`` exists in the discriminator update only, so it cannot leak into G.
        ``errD`` and the returned losses are unchanged; ``loss_terms["errD_cr_real"]`` / ``["errD_cr_fake"]`` are the unweighted
        terms of the step's last penalised update (device scalars).  A penalised update launches the pair builder instead of the
        concatenation (or after the last stage, with a stage on) and ``d_losses_cr`` instead of ``d_losses``; D's passes run on
        twice the rows; an unpenalised update is the plain one.  Captured with the step in graph mode, where the tables are staged
        beside the other stages' (a recording made before is dropped); the weights are device state (``set_bcr_weights``).  R1 is
        still taken at the front B rows, the adaptive probability still observes them.  Off: no draw, no launch, no allocation, the
        step is bit-identical to the plain one.  Refused: more than one rank, the generic (non-fused) discriminator path."""
        state = _crmod.BalancedCR(lambda_real, lambda_fake, every, policy, translation, seed)
        self.bcr = state
        try:
            self._bcr_check()
        except NotImplementedError:
            self.bcr = None
            raise
        self._guard_changed()
        return self

    def disable_bcr(self):
        self.bcr = None
        self._guard_changed()

    def set_bcr_weights(self, lambda_real, lambda_fake):
        """Write new weights into the regulariser's device record, between steps; a recorded step reads them from there and stays
        valid."""
        if self.bcr is None:
            raise RuntimeError("set_bcr_weights: consistency regularisation is off (enable_bcr)")
        self.bcr.set_weights(lambda_real, lambda_fake)

    def bcr_stats(self):
        """The regulariser's device record as a dict (``lambda_real``, ``lambda_fake``, ``every``, ``cr_real``, ``cr_fake``,
        ``updates``), or None with the feature off.  SYNCHRONISES the stream."""
        return self.bcr.stats() if self.bcr is not None else None

    # ------------------------------------------------------------------------------------------
    # LeCam regularisation of D (extension, no counterpart in the reference; srgan_amd.lecam)
    def _lecam_check(self):
        if dp.world_size() > 1:
            raise NotImplementedError(f"SRGAN_training: LeCam regularisation is on and the process group has {dp.world_size()} ranks; "
                                      "the anchors are averages of the global batch's predictions and would need a cross-rank mean "
                                      "(run one process, or disable_lecam())")
        if not self._fused_paths():
            raise NotImplementedError("SRGAN_training: LeCam regularisation is wired into the fused discriminator pass only (this "
                                      "package's own G / D / E modules with forward_logits, a one-hot ref_label, criteria with a "
                                      "fused kernel); use those, or disable_lecam()")

    def enable_lecam(self, weight=0.3, decay=0.99, start=0, clamp=False):
        """LeCam regularisation (Tseng et al., 2021): from now on EVERY discriminator update back-propagates ``errD + weight * R``,
        ``R = mean over the scales of [ mean_real phi(D(x) - a_F)^2 + mean_fake phi(a_R - D(G(z)))^2 ]`` on the raw GAN maps (scores
        under ``nn.MSELoss``, logits under ``nn.BCEWithLogitsLoss``), ``a_R`` / ``a_F`` exponential moving averages (``decay``) of
        the maps' means over the real / generated rows, per scale, updated BEFORE the term and constants of it; ``phi``: identity
        (the paper's equation), ``clamp=True``: relu (the one-sided form of the authors' released code).  The first update sets
        the anchors to the batch means; an update with a non-finite mean moves none.  The gradient is added from anchor update
        ``start`` on (a warm-up of the averages); ``R`` is computed and reported from the first.  One small launch per update
        behind the fused loss launch (``csrc/lecam.hip``); no extra rows through D, no launch in the backward; with consistency
        regularisation on, the term is taken on the front 2B rows only.  ``errD`` and the returned losses are unchanged;
        ``loss_terms["errD_lecam"]`` is the unweighted ``R`` of the step's last update (a device scalar).  Anchors, the count of
        updates and the three settings are device state (``set_lecam`` keeps a recording; a replayed step crosses ``start`` by
        itself); ``clamp`` is structural.  The defaults are this project's choice for LSGAN targets 0 / 1 and are not taken from
        any release; a criterion on the logit scale wants a much smaller weight.  Enabling drops a recording made before.  Off: no
        launch, no allocation, the step is bit-identical to the plain one.  Refused: more than one rank, the generic (non-fused)
        discriminator path."""
        state = _lcmod.LeCam(weight, decay, start, clamp)
        prev, self._lecam = self._lecam, state
        try:
            self._lecam_check()
        except NotImplementedError:
            self._lecam = prev
            raise
        self._guard_changed()
        return self

    def disable_lecam(self):
        self._lecam = None
        self._guard_changed()

    def set_lecam(self, weight=None, decay=None, start=None):
        """Write new settings (those given) into the regulariser's device record, between steps; a recorded step reads them from
        there and stays valid."""
        if self._lecam is None:
            raise RuntimeError("set_lecam: LeCam regularisation is off (enable_lecam)")
        self._lecam.set(weight, decay, start)

    def lecam_stats(self):
        """``weight``, ``decay``, ``start``, ``clamp`` and the device record's ``updates``, ``a_real``, ``a_fake`` (four per group, one
        per scale in use), ``penalty``, ``applied`` as a dict, or None with the feature off.  SYNCHRONISES the stream."""
        return self._lecam.stats() if self._lecam is not None else None

    # ------------------------------------------------------------------------------------------
    # mode-seeking regularisation of G (extension, no counterpart in the reference; srgan_amd.diversity)
    def _ms_check(self):
        if dp.world_size() > 1:
            raise NotImplementedError(f"SRGAN_training: mode seeking is on and the process group has {dp.world_size()} ranks; the "
                                      "msgan ratio is a statistic of the global batch and no reduced form exists (run one process, "
                                      "or disable_mode_seeking())")
        if not self._g_per_sample:
            raise NotImplementedError("SRGAN_training: mode seeking is on and the generator normalises with batch statistics; the "
                                      "second translation would advance its running buffers once more per step (build G with "
                                      "per-sample norms, or disable_mode_seeking())")

    def _ms_rides(self, nb, src):
        """May the second translation ride phase 1's batched forward as rows [2B, 3B)?  The kernels address an activation with
        32-bit byte offsets: the widest one of 3B images must stay under the limit ``UnrolledUpdate`` keeps for its groups."""
        Gm = dp.unwrap(self.G)
        if not isinstance(Gm, SingleGenerator):
            return False
        widest = max(int(Gm.down_convs[0].weight.shape[0]), 3) * src.shape[2] * src.shape[3] * 4
        return 3 * nb * widest <= (1 << 32) - (1 << 26)

    def enable_mode_seeking(self, weight=1.0, form="msgan", eps=1e-5, tau=None, seed=None):
        """Mode-seeking regularisation of the generator (Mao et al., 2019; per-sample clamped form: Yang et al., 2019): from now on
        phase 1 of ``update_GandE`` translates the source a second time, ``I2 = G(src, [onehot(target) | z2])`` with ``z2 ~ N(0, I)``
        drawn once per step from the feature's OWN generator (``seed``; the default generator and the step's noise order are what
        they are without it), and back-propagates ``weight * ms`` on top of the phase's loss: ``form="msgan"``: ``ms = dz / (dI +
        eps dz)``, ``dI`` / ``dz`` the batch means of ``|target_image - I2|`` and ``|z1 - z2|``; ``form="dsgan"``: ``ms = -mean_i
        min(r_i, tau)`` with the per-sample ratio ``r_i`` (``tau`` has no default).  The gradient reaches G through ``I2`` and
        through the kept ``target_image`` graph, never E or D.  ``I2`` rides phase 1's batched generator forward as a third group of
        rows (no convolution launch more), or takes a forward of its own where that batch is not formed or would cross the 4 GiB
        activation limit; three launches of ``csrc/diversity.hip`` per step.  The returned ``errG`` is unchanged;
        ``loss_terms["errG_ms"]`` is the unweighted term.  Captured with the step in graph mode (``z2`` staged beside the stages'
        tables; a recording made before is dropped); the weight is device state (``set_mode_seeking_weight``).  Off: no draw, no
        launch, no allocation, the step is bit-identical to the plain one.  Refused: more than one rank, a generator with
        batch-statistics norms."""
        state = _msmod.ModeSeeking(weight, form, eps, tau, seed)
        prev, self._ms = self._ms, state
        try:
            self._ms_check()
        except NotImplementedError:
            self._ms = prev
            raise
        self._guard_changed()
        return self

    def disable_mode_seeking(self):
        self._ms = None
        self._guard_changed()

    def set_mode_seeking_weight(self, weight):
        """Write a new weight into the regulariser's device record, between steps; a recorded step reads it from there and stays
        valid."""
        if self._ms is None:
            raise RuntimeError("set_mode_seeking_weight: mode seeking is off (enable_mode_seeking)")
        self._ms.set_weight(weight)

    def mode_seeking_stats(self):
        """``weight``, ``form``, ``eps``, ``tau`` and the device record's ``ms``, ``d_image``, ``d_latent``, ``updates`` as a dict, or
        None with the feature off.  SYNCHRONISES the stream."""
        return self._ms.stats() if self._ms is not None else None

    # ------------------------------------------------------------------------------------------
    # structural-similarity term of the reconstructions (extension, no counterpart in the reference; srgan_amd.structural)
    _SSIM_IDT_OFF = ("SRGAN_training: the SSIM term is asked for on the identity reconstruction and lbd['idt'] is 0, so the step makes "
                     "no identity image (set lbd['idt'] > 0, or enable_ssim(on=('cycle',)))")

    def enable_ssim(self, weight=1.0, on=("cycle",), window=11, sigma=1.5, k1=0.01, k2=0.03, data_range=2.0):
        """A structural-similarity term beside the L1 reconstruction terms (Wang et al., 2004; as a loss: Zhao et al., 2017): from
        now on phase 1 of ``update_GandE`` back-propagates ``weight * (1 - SSIM(source, recon_image))`` on top of the phase's loss
        (``"cycle"`` in ``on``), and the same for ``identity_image`` (``"idt"`` in ``on``; needs ``lbd["idt"] > 0``).  SSIM: Gaussian
        window of ``window`` taps (odd, 3..11) and ``sigma``, valid positions only, ``C1 = (k1 data_range)^2``, ``C2 = (k2
        data_range)^2``, the mean over positions, channels and samples (``srgan_amd.structural``).  The gradient reaches the
        reconstruction only, never the source.  Three launches of ``csrc/ssim.hip`` per term in the forward, none in the backward
        beyond one scaling.  The returned ``errG`` and ``errE_output`` are unchanged; ``loss_terms["errG_ssim_cycle"]`` /
        ``["errG_ssim_idt"]`` are the unweighted terms.  Captured with the step in graph mode; the weight is device state
        (``set_ssim_weight`` keeps a recording), the other settings are structural: enabling, disabling or other settings drop a
        recording made before.  With both reconstructions the record holds the last term taken (the identity's).  Off: no
        launch, no allocation, the step is bit-identical to the plain one.  Data parallel: the term is a mean over the rank's own
        rows like ``errG_cycle``, so the gradient all-reduce averages it as it averages that; untested beyond one process."""
        if isinstance(on, str):
            on = (on,)
        on = tuple(on)
        if not on or any(o not in ("cycle", "idt") for o in on) or len(set(on)) != len(on):
            raise ValueError(f"enable_ssim: on must be a non-empty subset of ('cycle', 'idt'), got {on!r}")
        if "idt" in on and not self.lbd["idt"] > 0:
            raise ValueError(self._SSIM_IDT_OFF)
        self._ssim = _ssmod.SSIM(weight, window, sigma, k1, k2, data_range)
        self._ssim_on = tuple(o for o in ("cycle", "idt") if o in on)
        self._guard_changed()
        return self

    def disable_ssim(self):
        self._ssim = None
        self._ssim_on = ()
        self._guard_changed()

    def set_ssim_weight(self, weight):
        """Write a new weight into the term's device record, between steps; a recorded step reads it from there and stays valid."""
        if self._ssim is None:
            raise RuntimeError("set_ssim_weight: the SSIM term is off (enable_ssim)")
        self._ssim.set_weight(weight)

    def ssim_stats(self):
        """The settings, ``on`` and the device record's ``term``, ``weighted``, ``updates`` as a dict, or None with the feature off.
        SYNCHRONISES the stream."""
        if self._ssim is None:
            return None
        out = self._ssim.stats()
        out["on"] = self._ssim_on
        return out

    # ------------------------------------------------------------------------------------------
    # device-side gradient guard (extension, no counterpart in the reference; srgan_amd.optim.Adam.enable_grad_guard)
    _GUARD_NETS = ("G", "D", "E")

    def _guard_opts(self, nets, what):
        nets = tuple(nets)
        if not nets or any(n not in self._GUARD_NETS for n in nets) or len(set(nets)) != len(nets):
            raise ValueError(f"{what}: nets is a non-empty selection of 'G', 'D' and 'E'")
        out = {}
        for n in nets:
            opt = getattr(self, "opt" + n)
            if opt is None:
                raise RuntimeError(f"{what}: opt{n} does not exist yet (call opt_sche_initialization() first)")
            if not isinstance(opt, Adam):
                raise TypeError(f"{what}: opt{n} is {type(opt).__module__}.{type(opt).__qualname__}, not srgan_amd.optim.Adam -- the "
                                "guard lives inside that optimiser's step (call opt_sche_initialization(), or pass that class)")
            out[n] = opt
        return out

    @staticmethod
    def _guard_value(max_norm, n, what):
        if isinstance(max_norm, dict):
            if n not in max_norm:
                raise ValueError(f"{what}: max_norm has no entry for '{n}'")
            return max_norm[n]
        return max_norm

    def enable_grad_guard(self, max_norm=None, nets=("G", "D", "E")):
        """From now on every optimiser step of the selected networks first checks its gradients ON THE DEVICE: a step whose squared
        gradient norm is not finite (a NaN or Inf anywhere, an overflow in the bf16 mode, a broken image) writes no parameter and
        no Adam moment, and with ``max_norm`` (a number, or a dict per net; ``None``: no clipping) the update runs on gradients
        scaled to that global 2-norm (``clip_grad_norm_``).  Works the same in a replayed hipGraph, which the host never looks
        into; a recording made before is dropped and made again.  A skipped step still advances the step counts (the bias
        correction runs one step ahead after it).  A guard that does not trigger changes no bit of the run.
        Data parallel: the check runs on the all-reduced gradients (the optimiser steps come after the reducer has finished), so
        every rank takes the same decision and no collective is added.  EMA: the update after a skipped step runs as always -- the
        live weights are unchanged and finite.  ``norm_type="batch"``: the running buffers are written by the forward pass, before
        any gradient exists, and are NOT protected (``grad_guard_stats()`` still shows the skip).  The returned losses are not
        filtered: a NaN loss stays NaN."""
        opts = self._guard_opts(nets, "enable_grad_guard")
        values = {n: self._guard_value(max_norm, n, "enable_grad_guard") for n in opts}
        for n, opt in opts.items():
            opt.enable_grad_guard(values[n])
        self._guard_changed()
        return self

    def _guard_changed(self):
        """The step's launches changed: forget a recording AND the warm-up of the input shape, so that the next step runs eagerly
        (it sizes the guards' tables and workspaces, which a capture must not create) and the one after records again."""
        if self._graph is not None:
            self._graph._drop()

    def set_grad_clip(self, max_norm, nets=("G", "D", "E")):
        """Write a new clipping threshold (a number, a dict per net, ``None``: no clipping) into the guards' device records,
        between steps; a recorded step reads it from there and stays valid."""
        opts = self._guard_opts(nets, "set_grad_clip")
        for n, opt in opts.items():
            opt.set_max_norm(self._guard_value(max_norm, n, "set_grad_clip"))

    def disable_grad_guard(self):
        for opt in self._opts():
            if isinstance(opt, Adam):
                opt.disable_grad_guard()
        self._guard_changed()

    def grad_guard_stats(self):
        """{"G": {...}, "D": {...}, "E": {...}} of ``optim.Adam.grad_guard_stats()`` (``None`` for a net without a guard): norm,
        scale and skip of each optimiser's last step and its cumulative steps / skipped / clipped counts.  Reads the device
        records: SYNCHRONISES the stream."""
        return {n: opt.grad_guard_stats() if isinstance(opt, Adam) and opt._guard is not None else None
                for n, opt in zip(self._GUARD_NETS, self._opts())}

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the scope ``self.G`` / ``self.E`` are the averaged copies, so ``G_transformation`` and the helpers of
        ``srgan_amd.inference`` that take the trainer sample from them; ``train()`` raises there."""
        cur = self._need_ema("ema_weights")
        if self._ema_scope:
            raise RuntimeError("ema_weights() scopes do not nest")
        live = (self.G, self.E)
        self.G = cur.twins.get("G", self.G)
        self.E = cur.twins.get("E", self.E)
        self._ema_scope = True
        try:
            yield self
        finally:
            self.G, self.E = live
            self._ema_scope = False


def _select_rows(x, mask):
    """x[mask] along the batch dimension of an NHWC-dense (logical NCHW) tensor, keeping it NHWC-dense."""
    mask = torch.as_tensor(mask).to(x.device)
    return x.permute(0, 2, 3, 1)[mask].permute(0, 3, 1, 2)


class SingleGAN_training(Checkpointing):
    """Conventional SingleGAN trainer on the HIP path -- BASELINE.json configs[0] (notebook 01).

    Same constructor / method signatures as the reference class (pyfiles/util_notebook.py:76-417):
      net = [G, D, E] with D a LIST of per-domain discriminators when ``singleD=False`` (each applied to the
      boolean-masked sub-batch of its domain) or one SingleDiscriminator_solo_multi when ``singleD=True``;
      E is the CBIN-conditioned ``Encoder_original(x, onehot(label))``.
    Kept semantics: ``update_D`` returns the LAST domain's errD; the per-domain D optimisers are always rebuilt by
    ``opt_sche_initialization``; phase 2's identity-regression path draws a RANDOM latent; stale-graph phase 2;
    the no-op "unrolled" restore.  Networks are used where the caller put them (the reference does not move them).
    """

    def __init__(self, net, opt, criterion, lbd, unrolled_k, device, ref_label, ndim,
                 classes, batch_size=64, encoded_feature="latent", singleD=False):
        self.G, self.D, self.E = net[0], net[1], net[2]
        self.optG, self.optD, self.optE = opt[0], opt[1], opt[2]
        self.scheG, self.scheD, self.scheE = None, None, None
        self.criterion, self.criterion_class = criterion
        self.lbd = lbd
        self.k = unrolled_k
        self.device = device
        self.ref_label = ref_label
        self.n_batch = batch_size
        self.encoded_feature = encoded_feature
        self.ndim = ndim
        self.classes = classes
        self.singleD = singleD
        self.source_image = None
        self.target_image = None
        self.recon_image = None
        self.label = None
        self.c_rand = None
        self.enc_info = None
        self.target_cenc = None
        if lbd["hist"] > 0:
            self.hi = histogram_imitation(device)
        self.loss_terms = {}
        self.noise_fn = torch.randn
        self._refuse_spectral()

    def _refuse_spectral(self):
        nets = [self.G, self.E] + (list(self.D) if isinstance(self.D, (list, tuple)) else [self.D])
        if any(spectral.find(dp.unwrap(n)) for n in nets if isinstance(n, nn.Module)):
            raise NotImplementedError("SingleGAN_training: a network is marked with spectral_norm; this trainer's optimiser steps "
                                      "neither map the gradients nor run the power iteration (use SRGAN_training, or "
                                      "spectral.remove_spectral_norm(net))")

    def enable_diffaugment(self, *args, **kwargs):
        raise NotImplementedError("SingleGAN_training: DiffAugment is not wired into this trainer's discriminator passes (per-domain "
                                  "sub-batches); use SRGAN_training.enable_diffaugment, or augment.DiffAugment in a loop of your own")

    def enable_geometric_augment(self, *args, **kwargs):
        raise NotImplementedError("SingleGAN_training: the geometric augmentation is not wired into this trainer's discriminator "
                                  "passes (per-domain sub-batches); use SRGAN_training.enable_geometric_augment, or "
                                  "augment.GeometricAugment in a loop of your own")

    def enable_ada(self, *args, **kwargs):
        raise NotImplementedError("SingleGAN_training: the adaptive augmentation probability is not wired into this trainer's "
                                  "discriminator passes (per-domain sub-batches); use SRGAN_training.enable_ada, or ada.AdaptiveP "
                                  "in a loop of your own")

    def enable_r1(self, *args, **kwargs):
        raise NotImplementedError("SingleGAN_training: the R1 penalty is not wired into this trainer's discriminator passes (per-domain "
                                  "sub-batches); use SRGAN_training.enable_r1, or r1.r1_accumulate in a loop of your own")

    def enable_bcr(self, *args, **kwargs):
        raise NotImplementedError("SingleGAN_training: consistency regularisation is not wired into this trainer's discriminator "
                                  "passes (per-domain sub-batches); use SRGAN_training.enable_bcr, or consistency.BalancedCR in a "
                                  "loop of your own")

    def enable_lecam(self, *args, **kwargs):
        raise NotImplementedError("SingleGAN_training: LeCam regularisation is not wired into this trainer's discriminator passes "
                                  "(per-domain sub-batches); use SRGAN_training.enable_lecam, or lecam.LeCam in a loop of your own")

    def enable_ssim(self, *args, **kwargs):
        raise NotImplementedError("SingleGAN_training: the SSIM term is not wired into this trainer's generator update (per-domain "
                                  "sub-batches); use SRGAN_training.enable_ssim, or structural.SSIM in a loop of your own")

    def enable_mode_seeking(self, *args, **kwargs):
        raise NotImplementedError("SingleGAN_training: mode seeking is not wired into this trainer's generator update (per-domain "
                                  "sub-batches); use SRGAN_training.enable_mode_seeking, or diversity.ModeSeeking in a loop of your own")

    def opt_sche_initialization(self, lr=[0.0001, 0.0001, 0.0001]):
        lr_G, lr_D, lr_E = lr
        if self.optG is None:
            self.optG = Adam(self.G.parameters(), lr=lr_G, betas=(0.5, 0.999))
        self.scheG = optim.lr_scheduler.ExponentialLR(self.optG, gamma=0.95)
        if self.singleD:
            if self.optD is None:
                self.optD = Adam(self.D.parameters(), lr=lr_D, betas=(0.5, 0.999))
            self.scheD = optim.lr_scheduler.ExponentialLR(self.optD, gamma=0.95)
        else:
            self.optD = []
            self.scheD = []
            for i in self.classes:
                self.optD.append(Adam(self.D[i].parameters(), lr=lr_D, betas=(0.5, 0.999)))
                self.scheD.append(optim.lr_scheduler.ExponentialLR(self.optD[i], gamma=0.95))
        if self.optE is None:
            self.optE = Adam(self.E.parameters(), lr=lr_E, betas=(0.5, 0.999))
        self.scheE = optim.lr_scheduler.ExponentialLR(self.optE, gamma=0.95)
        return

    def _onehot(self, label):
        return class_encode(label, self.device, self.ref_label)

    def G_transformation(self, target_label, source_image, encoder=False, ref_image=None):
        class_vector = self._onehot(target_label)
        if encoder:
            latent, mu, logvar = self.E(ref_image, class_vector)
            info = [latent, mu, logvar]
            latent_vector = latent if self.encoded_feature == "latent" else mu
        else:
            latent_vector = host_to_device(self.noise_fn(source_image.shape[0], self.ndim), self.device)
            info = latent_vector
        target_image = self.G(source_image, torch.cat([class_vector, latent_vector], 1))
        return target_image, info

    def _mask(self, which, i):
        return (torch.as_tensor(self.label[which]) == i)

    def update_D(self):
        self.target_image, self.c_rand = self.G_transformation(self.label["target"], self.source_image, False)
        if self.singleD:
            self.D.zero_grad()
            output, output_class = self.D(self.source_image)
            errD_real = get_loss_D(output, 1., self.criterion, self.device)
            errD_class = get_domainloss_D(output_class, self._onehot(self.label["source"]), self.criterion_class)
            errD = errD_real + errD_class * self.lbd["class"]
            output, _ = self.D(self.target_image.detach())
            errD = errD + get_loss_D(output, 0., self.criterion, self.device)
            errD.backward()
            self.optD.step()
            return errD
        errD = None
        for i in self.classes:
            errD = 0
            self.D[i].zero_grad()
            m_real, m_fake = self._mask("source", i), self._mask("target", i)
            if int(m_real.sum()) != 0:
                errD = errD + get_loss_D(self.D[i](_select_rows(self.source_image, m_real)), 1., self.criterion, self.device)
            if int(m_fake.sum()) != 0:
                fake = _select_rows(self.target_image.detach(), m_fake)
                errD = errD + get_loss_D(self.D[i](fake), 0., self.criterion, self.device)
            errD.backward()
            self.optD[i].step()
        return errD

    def update_GandE(self):
        L = self.lbd
        self.G.zero_grad()
        self.E.zero_grad()
        src = self.source_image
        recon_image, source_enc_info = self.G_transformation(self.label["source"], self.target_image, True, src)
        d_params = list(self.D.parameters()) if self.singleD else [p for d in self.D for p in d.parameters()]
        errG = 0
        with _frozen(d_params):                      # D's weight gradients are discarded by the next zero_grad
            if self.singleD:
                output, output_class = self.D(self.target_image)
                errG_dis = get_loss_D(output, 1., self.criterion, self.device)
                errG_class = get_domainloss_D(output_class, self._onehot(self.label["target"]), self.criterion_class)
                errG = errG + errG_dis + errG_class * L["class"]
            else:
                for i in self.classes:
                    m = self._mask("target", i)
                    if int(m.sum()) != 0:
                        out = self.D[i](_select_rows(self.target_image, m))
                        errG = errG + get_loss_D(out, 1., self.criterion, self.device) / len(self.classes)
        errG_cycle = ops.l1_mean(src, recon_image, 1.0)
        errG = errG + errG_cycle * L["cycle"]
        errE = 0
        errE_output = errG_cycle * L["cycle"]
        terms = dict(errG_cycle=errG_cycle)
        _, mu, logvar = source_enc_info
        if L["KL"] > 0:
            errE_KL = ops.kl_normal(mu, logvar)
            errE = errE + errE_KL * L["KL"]
            errE_output = errE_output + errE_KL * L["KL"]
            terms["errE_KL"] = errE_KL
        if L["idt"] > 0:
            identity_image, _ = self.G_transformation(self.label["source"], src, True, src)
            errG_idt = ops.l1_mean(src, identity_image, 1.0)
            errG = errG + errG_idt * L["idt"]
            errE_output = errE_output + errG_idt * L["idt"]
            terms["errG_idt"] = errG_idt
        if L["batch_KL"] > 0:
            w_corr = L["corr_enc"] if L["corr_enc"] > 0 else 0.0
            w_hist = L["hist"] if L["hist"] > 0 else 0.0
            target = self.hi.target if w_hist > 0 else torch.full((50,), 0.02, device=mu.device)
            total, parts, _ = ops.latent_losses(mu, self.n_batch, target, L["batch_KL"], w_corr, w_hist)
            errE = errE + total
            errE_output = errE_output + total
            terms.update(errE_bKL=parts[0], errE_corr=parts[1], errE_hist=parts[2])
        (errG + errE).backward(retain_graph=True)
        self.optG.step()
        self.optE.step()

        self.G.zero_grad()
        self.E.zero_grad()
        with _frozen(list(self.E.parameters())):
            _, target_cenc, _ = self.E(self.target_image, self._onehot(self.label["target"]))
            errG_reg = ops.l1_mean(self.c_rand, target_cenc, 1.0)
            errG_ex = errG_reg * L["reg"]
            terms["errG_reg"] = errG_reg
            if L["idt_reg"] * L["idt"] > 0:
                idt_random_image, source_c_rand = self.G_transformation(self.label["source"], src, False)
                _, idt_cenc_rand, _ = self.E(idt_random_image, self._onehot(self.label["source"]))
                errG_idt_reg = ops.l1_mean(source_c_rand, idt_cenc_rand, 1.0)
                errG_ex = errG_ex + errG_idt_reg * (L["idt_reg"] * (L["idt"] / L["cycle"]))
                terms["errG_idt_reg"] = errG_idt_reg
            errG_ex.backward()
        self.optG.step()
        self.recon_image = recon_image.detach()
        self.loss_terms.update({k: v.detach() for k, v in terms.items()})
        return [errG.detach() + errG_ex.detach(), errE_output.detach()]

    def UnrolledUpdate(self):
        errorD = None
        for i in range(self.k):
            errD = self.update_D()
            if i == 0:
                errorD = errD.detach()
        errorG, errorE = self.update_GandE()
        return [errorG, errorD, errorE]

    def train(self, source_image, label):
        self._refuse_spectral()
        self.source_image = ops.to_nhwc(source_image)
        self.label = label
        self.loss_terms = {}
        return self.UnrolledUpdate()
