"""hipGraph mode of ``SRGAN_training`` (``enable_graph``): HOW a fixed launch sequence is recorded and replayed.

``trainer.py`` chooses the launches; this module stages the step's inputs (``_StepGraph._stage``), records ``sg.UnrolledUpdate()``
(``_capture``, ``_Recording``), replays it, and drops the recording when something it baked in has changed.  It names no optional
feature: a feature joins ``_fingerprint()`` and the keep-alive list by being in ``sg._extensions()``, the host-side counters a
recording advances are those of ``sg._mirrors()``, and the augmentation stages whose host-drawn tables are staged beside the noise
(one ``_Staged`` per stage, keyed by its ``section``) are those of ``sg._drawing_stages()``: the stages applied to everything D reads
and any other object whose host draws the step consumes (the consistency pairs' tables, mode seeking's second latent code).
"""
import gc
import os

import numpy as np
import torch

from . import _lib, dp, ops
from .losses import has_fused_kind
from .model import _is_batch_stat, _is_synced
from .optim import Adam


class _Staged:
    """``what`` ("noise draws", "augment tables") the step draws on the host: staged into one static device buffer
    [n, B, row] and handed out slice by slice while the captured body runs."""

    def __init__(self, what):
        self.what, self.buf, self.i = what, None, 0

    def reset(self):
        self.i = 0

    def stage(self, draws, device):
        """copy this step's host draws (stream-ordered, from pinned memory) into the buffer, made at the first use"""
        host = torch.stack([d.to(torch.float32) for d in draws]).pin_memory()
        if self.buf is None:
            self.buf = torch.empty(host.shape, dtype=torch.float32, device=device)
        self.buf.copy_(host, non_blocking=True)

    def staged(self):
        return self.buf.shape[0] if self.buf is not None else 0

    def next(self, count):
        """the next ``count`` entries as one [count * B, row] view of the static buffer"""
        t = self.buf[self.i:self.i + count]
        if t.shape[0] != count:
            raise RuntimeError(f"the step asks for more {self.what} than the {self.staged()} staged")
        self.i += count
        return t.reshape(-1, t.shape[-1])

    def check_consumed(self):
        if self.i != self.staged():
            raise RuntimeError(f"captured step consumed {self.i} {self.what}, staged {self.staged()}")


class _StepGraph:
    """Static inputs, capture and replay of one ``SRGAN_training`` step (see ``SRGAN_training.enable_graph``)."""

    def __init__(self, sg):
        self.sg = sg
        self.key = None          # input signature the eager warm-up ran with
        self.graph = None
        self.x = self.out = None
        self.staged_noise = _Staged("noise draws")            # [len(sg._noise_kinds()), B, ndim]
        self.staged = {}         # a stage's section -> _Staged of [its draws per step, B, row width], for the stages that draw
        self.lab = {}
        self._onehot = {}
        self._versions = None
        self.table = None
        self._epoch = -1
        self._keep = None
        self._baked = None       # fingerprint of everything the recording holds by value or by pointer (see _fingerprint)
        self._steps = None       # host-side optimiser step counts the device records stand at after the last replay
        self._graph_ran = False  # the previous step ran on the capture stream (recorded or replayed)
        self._force_segmented = False   # a single-graph recording failed on some rank: record segments from here on
        self._last_single = False       # the recording being made / made last captured its collectives (one graph)
        self._deltas = None             # [(mirror, what one run of the recording moves its host-side counters by)]
        reason = self.unsupported_reason()
        if reason and reason is not self.SEGMENTED_SYNC:      # (that one is not a refusal: such steps run eagerly, _local_mode)
            raise NotImplementedError("SRGAN_training.enable_graph: " + reason)

    def tables(self, section):
        """the staged tables of the stage ``section`` names (None with the stage off)"""
        return self.staged[section].buf if section in self.staged else None

    aug = property(lambda self: self.tables("augment"))         # shorthands of the two stages that exist today
    geom = property(lambda self: self.tables("geometry"))

    fault_hook = None            # tests: callable(stage) with stage in {"before", "inside"}; raising makes the recording fail

    # A synced norm's backward exchanges partials from autograd's thread; cutting the recording there would end, in that thread, a
    # capture begun in this one, which the HIP runtime refuses (hipErrorStreamCaptureWrongThread).  Such a step runs eagerly on
    # every rank, or as ONE graph with the captured C-ABI collectives (SRGAN_DP_COMM=abi: no cut).
    SEGMENTED_SYNC = ("synced batch norms in the segmented form: their backward exchange cannot cut a recording from autograd's "
                      "thread; the step runs eagerly (or as one graph with SRGAN_DP_COMM=abi)")

    def unsupported_reason(self):
        sg = self.sg
        if not sg._fused_paths():
            return ("needs this package's own G / D / E modules, a one-hot ref_label and criteria with a fused kernel (nn.MSELoss, "
                    "nn.BCEWithLogitsLoss / nn.BCELoss)")
        for name, opt in zip(("optG", "optD", "optE"), sg._opts()):
            if not isinstance(opt, Adam):
                return f"{name} is not srgan_amd.optim.Adam (call opt_sche_initialization(), or pass that class)"
        if dp.is_distributed() and os.environ.get("SRGAN_DP_GRAPH") == "0":
            return "SRGAN_DP_GRAPH=0: data-parallel steps run eagerly (hook-driven all-reduce under the backward)"
        if dp.is_distributed() and self._synced_norms() and not self._single_graph():
            return self.SEGMENTED_SYNC
        return None

    def _synced_norms(self):
        sg = self.sg
        return any(_is_synced(m) and m.training for net in (sg.G, sg.E) for m in net.modules() if _is_batch_stat(m))

    def _single_graph(self):
        """Would a recording made now capture its collectives (one graph, no cut)?  The condition of _Recording.single."""
        return not self._force_segmented and dp.transport() == "abi" and os.environ.get("SRGAN_DP_SINGLE_GRAPH") != "0"

    @staticmethod
    def _key(source_image, label):
        def dev(t):
            return t.device.type if torch.is_tensor(t) else "host"
        return (tuple(source_image.shape), dev(label["source"]), dev(label["target"]))

    def _fingerprint(self):
        """Everything a recording bakes in besides the input shape and the buffers ``ops.structure_epoch()`` watches: the
        optimiser objects, their hyper-parameters and moment tensors (``load_state_dict`` replaces them), which parameters
        take gradients (``freeze_melt`` / ``requires_grad_``), k, the loss weights, the criteria, the style-code source, the
        label table, the gradient guards, the optional features that are on.  A replay with any of these changed would silently
        keep training the OLD configuration."""
        sg = self.sg
        fp = [sg.k, sg.n_batch, sg.ndim, sg.encoded_feature, tuple(sorted((k, float(v)) for k, v in sg.lbd.items())),
              type(sg.criterion), type(sg.criterion_class), np.asarray(sg.ref_label, dtype=np.float64).tobytes()]
        # the kernel kinds follow from the types, but a criterion edited in place (reduction, weight) can lose its kind
        fp.append((has_fused_kind(sg.criterion, "gan"), has_fused_kind(sg.criterion_class, "class")))
        for opt in sg._opts():
            fp.append(id(opt))
            for g in getattr(opt, "param_groups", ()):
                fp.append((tuple(g["betas"]), float(g["eps"])))
                for p in g["params"]:
                    st = opt.state.get(p) or {}
                    m, v = st.get("exp_avg"), st.get("exp_avg_sq")
                    fp.append((id(p), m.data_ptr() if m is not None else 0, v.data_ptr() if v is not None else 0))
        fp.append(tuple((id(p), p.data_ptr(), p.requires_grad) for p in self._all_params()))
        # batch norms: train / eval mode, momentum and eps are baked into the recorded launches (the running buffers themselves are
        # device state the step updates in place)
        # so is the mark of dp.sync_batch_stats (another autograd function, with exchanges)
        fp.append(tuple((id(m), m.training, m.momentum, m.eps, m.track_running_stats, _is_synced(m)) for net in (sg.G, sg.E)
                        for m in net.modules() if _is_batch_stat(m)))
        # the gradient guards: their reduce launches, the guarded update and the records (enable / disable between steps); the
        # clipping threshold is device state
        fp.append(tuple(opt.grad_guard_fingerprint() if isinstance(opt, Adam) else None for opt in sg._opts()))
        # the optional features that are on: their launches, records, tables and workspaces (what is device state stays out)
        fp.append(tuple((type(x).__name__, x.fingerprint()) for x in sg._extensions()))
        return tuple(fp)

    def _opt_steps(self):
        return [[int(opt.state[p]["step"]) if len(opt.state.get(p) or {}) else -1 for g in opt.param_groups for p in g["params"]]
                for opt in self.sg._opts()]

    def _drop(self):
        self.graph = self.key = self._keep = self._baked = self._steps = self._deltas = None
        self.x = self.out = self.staged_noise.buf = None
        self.staged = {}

    def _local_mode(self, source_image, label):
        """2: replay the recording, 1: record (the eager warm-up of this input shape has run), 0: eager."""
        if dp.is_distributed() and self.unsupported_reason() is self.SEGMENTED_SYNC:
            # the same answer on every rank (the marks, the transport and a failed single-graph recording are agreed state)
            if self.graph is not None:
                self._drop()
            return 0
        if self.graph is not None:
            stale = self._epoch != ops.structure_epoch()
            # a buffer the recording points at was replaced (compute-mode switch, invalidate_packed, optimiser re-seeded), or
            # something it baked in changed (optimiser state loaded, requires_grad toggled, lbd / k edited), or the host-side
            # step counts are not where the last replay left them (load_state_dict): forget the graph; this step runs eagerly
            # with the new state (which also re-seeds the device-side Adam records), the next one records again
            if not stale and (self._baked != self._fingerprint() or self._steps != self._opt_steps()):
                stale = True
                reason = self.unsupported_reason()
                if reason:
                    raise NotImplementedError("SRGAN_training graph mode: " + reason)
            if stale:
                self._drop()
        if self.key is None or self._key(source_image, label) != self.key or not source_image.is_cuda:
            return 0
        return 2 if self.graph is not None else 1

    def accepts(self, source_image, label):
        """Replay / record this step (True) or run it eagerly (False).  Under a process group the decision is COLLECTIVE (one
        MIN all-reduce of the local answer on the host-side control group): a rank replaying index-ordered flat buckets beside
        a rank running the hook-ordered eager step -- or recording, with its extra agreement all-reduce -- would issue different
        collectives.  If any rank has to record, every rank records again; if any rank runs eagerly, all do."""
        failure = None
        try:
            mode = self._local_mode(source_image, label)
        except NotImplementedError as e:
            # A rank that can no longer take graph mode must still join the agreement below -- raising before the collective would
            # leave the other ranks blocked in it.  It votes -1, a value no healthy rank uses (a vote of 0 read as
            # "eager" on the peers, which then entered the eager step and blocked in its first gradient all-reduce until the dead
            # rank's connection timed out); on a negative minimum EVERY rank raises, at the same point of its program.
            failure, mode = e, -1
            if not dp.is_distributed():
                raise
        if dp.is_distributed() and mode == 2 and failure is None and self.graph.single:
            # Single-graph data-parallel step (round 6): the collectives are INSIDE the recording, so a replay is one launch with
            # no host-side exchange at all -- graph-or-eager was decided collectively when the step was recorded, and every
            # condition that drops a recording (_local_mode) is a program-state change an SPMD program makes on every rank at the
            # same step.  A rank that has to re-record alone votes below while its peers replay: it blocks there until the control
            # group's timeout and raises (dp.control_group); the segmented mode keeps the per-step vote.
            return True
        if dp.is_distributed():
            agreed = dp.all_min(mode)
            if failure is not None:
                raise failure
            if agreed < 0:
                raise RuntimeError("SRGAN_training graph mode: another rank cannot take this step (see its own error); no rank "
                                   "runs it")
            if agreed < 2 and self.graph is not None:
                if agreed == 1:
                    key = self.key
                    self._drop()           # another rank re-records: record again with it (same segment structure)
                    self.key = key
            mode = agreed
        return mode >= 1

    def before_eager_step(self):
        """An eager step follows a recorded / replayed one: the graphs the step keeps pin AccumulateGrad nodes made on the CAPTURE
        stream; an eager backward would synchronise across streams on every gradient (PyTorch warns about the mismatch)."""
        if self._graph_ran:
            self._graph_ran = False
            self.sg._forget_step()

    def note_eager_step(self, source_image, label):
        if self.key is None and source_image.is_cuda:
            self.key = self._key(source_image, label)
        # the eager step left every packed operand fresh: writes from here on (load_state_dict, copy_) must be noticed
        self._versions = sum(p._version for p in self._all_params())
        if self.graph is not None:      # an eager step of this trainer (another batch shape) moved the optimisers legitimately
            self._steps = self._opt_steps()

    # -- what the captured body reads -----------------------------------------------------------------------------
    def onehot(self, which):
        hit = self._onehot.get(which)
        if hit is None:              # once per step (inside the graph): rows of the device copy of ref_label
            hit = self._onehot[which] = self.table.index_select(0, self.lab[which])
        return hit

    def _rewind(self):           # the body about to run reads the staged inputs from the start
        for st in (self.staged_noise, *self.staged.values()):
            st.reset()
        self._onehot = {}

    # -- staging (outside the graph, stream-ordered before the replay) ---------------------------------------------
    def _stage(self, source_image, label):
        sg = self.sg
        dev = source_image.device
        nb = source_image.shape[0]
        kinds = sg._noise_kinds()
        draws = [sg.noise_fn(nb, sg.ndim) if kd == "randn" else torch.FloatTensor(nb, sg.ndim).normal_() for kd in kinds]
        x = ops.to_nhwc(source_image)
        if self.x is None:
            self.x = torch.empty_like(x)
            self.lab = {w: torch.empty(nb, dtype=torch.int64, device=dev) for w in ("source", "target")}
            self.table = torch.tensor(np.asarray(sg.ref_label), dtype=torch.float32).to(dev)
        _, _, h, w = x.shape
        for stage in sg._drawing_stages():
            # a stage's rows (2k + 1 where it is applied to everything D reads; the trainer says how many: _stage_draws), drawn up
            # front in the order the eager step draws them (SRGAN_training._stage_tables), stage by stage: each draws from its own
            # generator; what a row holds and how wide it is, is the trainer's business
            n = sg._stage_draws(stage)
            if n:
                st = self.staged.setdefault(stage.section, _Staged(stage.section + " tables"))
                st.stage([sg._stage_row_draw(stage, nb, h, w) for _ in range(n)], dev)
        self.x.copy_(x)
        self.staged_noise.stage(draws, dev)
        for w in ("source", "target"):
            lab = torch.as_tensor(label[w]).detach().to(dtype=torch.int64)
            if not lab.is_cuda:
                lab = lab.pin_memory()
            self.lab[w].copy_(lab.view(-1), non_blocking=True)

    def _all_params(self):
        sg = self.sg
        return [p for net in (sg.G, sg.D, sg.E) for p in net.parameters()]

    def _guard_packed(self):
        """Weights written behind the graph's back (load_state_dict, copy_: they bump the autograd version, the raw-pointer
        Adam does not) would leave the captured step multiplying stale packed operands: re-pack before replaying."""
        v = sum(p._version for p in self._all_params())
        if self._versions is not None and v != self._versions:
            ops.refresh_packed(self._all_params(), force=True)
        self._versions = v

    def _capture(self):
        sg = self.sg
        lib_prof_off()
        # Every autograd graph of the eager warm-up must be gone before recording: its AccumulateGrad nodes -- made on the caller's
        # stream -- would be re-used by the recorded step and pull that stream into the capture as an unjoined fork.
        sg._forget_step()
        hook = type(self).fault_hook
        if hook is not None:
            hook("before")
        ops.mark_singles_stale()          # their pack launches belong to the recording (ops.refresh_packed)
        g = _Recording(self.x.device, single=not self._force_segmented)
        self._last_single = g.single
        epoch0 = ops.structure_epoch()    # a buffer replaced DURING the recording (the weight-gradient arena grown
        sg._g_active = True               # between two segments) would leave earlier segments pointing at freed memory
        self._rewind()
        sg.source_image = self.x
        try:
            with g:
                with ops.pack_cache(refresh_on_entry=False):
                    err = sg.UnrolledUpdate()
                if hook is not None:
                    hook("inside")
                self.out = torch.stack([e.detach().reshape(()) for e in err])
        finally:
            sg._g_active = False
        for st in (self.staged_noise, *self.staged.values()):
            st.check_consumed()
        if ops.structure_epoch() != epoch0:
            raise RuntimeError("a workspace the step points at was replaced while the step was being recorded "
                               "(ops.structure_epoch moved): the recording is dropped")
        self.graph = g
        self.terms = dict(sg.loss_terms)
        self._epoch = ops.structure_epoch()
        self._keep = ops.graph_keepalive() + [t for x in list(sg._opts()) + sg._extensions() for t in x.graph_keepalive()]
        self._baked = self._fingerprint()

    def _undo_recording(self, snap):
        """A recording was given up.  It advanced the host-side counters without running anything: they go back where ``snap`` --
        [(mirror, its host_counters())] -- found them.  Host-side caches may describe device buffers whose filling launch was only
        RECORDED (a packed operand, a repack table): all are forgotten, as are the graphs and caches of the recorded body."""
        for m, c in snap:
            m.restore_host_counters(c)
        ops.invalidate_packed()
        self.sg._forget_step()

    def _abandon(self, err, snap, keep_graph_mode=False):
        """Some rank could not record the step: every rank drops graph mode together.  THIS step still runs -- eagerly, from the
        inputs already staged for the recording (same image batch, labels and pre-drawn noise, so the CPU generator is where an
        eager run would have left it) -- and later steps take the ordinary eager path."""
        import warnings
        sg = self.sg
        warnings.warn("SRGAN_training: the step could not be recorded as " + ("ONE hipGraph with captured collectives" if keep_graph_mode
                                                                              else "hipGraph segments") + " on every rank"
                      + (f" (this rank: {type(err).__name__}: {err})" if err is not None else "")
                      + ("; this step runs eagerly, the next one is recorded as segments" if keep_graph_mode else "; running eagerly from here on"))
        self.graph = self._keep = self._baked = self._steps = None
        self._undo_recording(snap)
        self._rewind()                            # (the staged noise and the stages' tables are used again)
        sg.source_image = self.x
        sg._g_active = True
        try:
            with ops.pack_cache():
                out = sg.UnrolledUpdate()
        finally:
            sg._g_active = False
            if not keep_graph_mode:
                sg._graph = None
        return out

    def run(self, source_image, label):
        sg = self.sg
        self._stage(source_image, label)
        self._guard_packed()
        for opt in sg._opts():
            opt.sync_device()
        if self.graph is None:
            err = None
            snap = [(m, m.host_counters()) for m in sg._mirrors()]
            try:
                self._capture()      # records; the host-side optimiser counters advanced while recording
            except Exception as e:   # noqa: BLE001 -- under a process group the ranks first agree on what happened
                if not dp.is_distributed():
                    # leave nothing half-advanced behind for a caller that catches this, and graph mode stays off
                    self._undo_recording(snap)
                    self._drop()
                    sg._graph = None
                    raise
                err = e
            if dp.is_distributed() and not dp.all_agree(err is None):
                # some rank could not record the step: EVERY rank gives the recording up together (a rank replaying segments
                # beside a rank running eagerly would issue the same collectives in another order) and runs eagerly.  If the
                # attempt was the single-graph form (collectives captured), the segmented form is tried at the next step before
                # graph mode is given up: this step runs eagerly, the next one records segments.
                retry = self._last_single and not self._force_segmented
                self._force_segmented = self._force_segmented or self._last_single
                return self._abandon(err, snap, keep_graph_mode=retry)
            self._deltas = [(m, m.counters_since(c)) for m, c in snap]     # (the recording advanced the mirrors already)
        else:
            for m, d in self._deltas:        # the replay moves the device-side counters; the host mirrors follow
                m.advance_host(d)
        self.graph.replay()
        self._graph_ran = True
        self._steps = self._opt_steps()
        sg.source_image = self.x
        sg.loss_terms = dict(self.terms)
        return list(self.out.clone())       # (the static result vector is overwritten by the next replay)


class _Recording:
    """One train step as a chain of hipGraph segments with host callables between them.

    Single process: one segment -- the whole step is one graph launch.  Data parallel: ``srgan_amd.dp`` ends the segment being
    recorded wherever the step starts a collective (``dp.launch_pending``: the bucket all-reduces after a backward; the mu
    all-gather) and wherever it needs the result (``GradReducer.finish``), and hands over a host callable; ``replay()`` launches
    segment, callable, segment, ... on the caller's stream.  A "start" callable enqueues the in-place all-reduces of the flat
    buckets on the communication stream behind a ``ready`` event and returns; the segments launched next -- the work the trainer
    placed between start and finish: the next translation during the discriminator loop, phase 1's encoder / generator forward
    under the last discriminator all-reduce, E's optimiser step and phase 2's E(source) under G's -- run UNDER the collectives;
    the "wait" callable makes the compute stream wait for the ``done`` events right before the optimiser-step segment.  Nothing
    of RCCL is captured and no stream is forked inside a capture: the collectives stay ordinary eager calls on static buffers in
    a fixed order.  2k + 6 segments per step (k x (start, wait), the all-gather, start(E) inside phase 1's backward, start(G) + wait(E), wait(G),
    start(G) + wait(G): a wait that follows its start directly rides in the same callable).  All segments allocate from one private pool and are replayed in recording order, so a tensor made in one segment
    is valid in the following ones."""

    def __init__(self, device, single=True):
        self.device = device
        # Round 6: with the C-ABI collectives (dp.set_transport("abi") / SRGAN_DP_COMM=abi) a collective is one
        # RCCL enqueue on a stream -- capturable -- so the step is recorded as ONE graph: where the segmented form cuts, the host
        # callable runs INSIDE the capture (the communication stream forks off the capture stream at the bucket's `ready` event
        # and joins it again at `done`), and a replay is a single launch.  SRGAN_DP_SINGLE_GRAPH=0 keeps the segments.
        self.single = bool(single and dp.is_distributed() and dp.transport() == "abi" and os.environ.get("SRGAN_DP_SINGLE_GRAPH") != "0")
        self.inline = []           # single-graph form: kinds of the captured collectives, in enqueue order
        self.segments = []         # [(CUDAGraph, callable or None)]
        self.trace = None          # tests: a list -> the host-side order of the last replay: ("segment", i) / (comm kind, i)
        self.pending = []          # flat gradient buckets laid out since the last cut (dp.GradReducer)
        self._cur = None
        self._pool = None
        self._stream = None
        self._stream_ctx = None
        # other threads of a data-parallel process (the process group's watchdog) may touch HIP while this one records
        self._mode = "thread_local" if dp.is_distributed() else "global"

    def _begin(self):
        self._cur = torch.cuda.CUDAGraph()
        self._cur.capture_begin(pool=self._pool, capture_error_mode=self._mode)

    def cut(self, comm):
        if self.single:
            comm()                 # enqueued into the capture (fork to / join from the communication stream)
            self.inline.append(getattr(comm, "kind", "comm"))
            return
        self._cur.capture_end()
        self.segments.append((self._cur, comm))
        self._begin()

    def __enter__(self):
        torch.cuda.synchronize(self.device)
        gc.collect()
        torch.cuda.empty_cache()
        self._pool = torch.cuda.graph_pool_handle()
        self._stream = torch.cuda.Stream(self.device)
        self._stream.wait_stream(torch.cuda.current_stream(self.device))
        self._stream_ctx = torch.cuda.stream(self._stream)
        self._stream_ctx.__enter__()
        dp.set_recorder(self if dp.is_distributed() else None)
        self._begin()
        return self

    def __exit__(self, *exc):
        dp.set_recorder(None)
        try:
            self._cur.capture_end()
            self.segments.append((self._cur, None))
        finally:
            self._cur = None
            self._stream_ctx.__exit__(*exc)
        if exc[0] is None and self.pending:
            raise RuntimeError("recorded step left gradient buckets without their all-reduce (GradReducer.finish() not called)")
        return False

    def replay(self):
        trace = self.trace
        if trace is not None:
            trace.clear()
        with torch.no_grad():          # the collectives write buffers (views made inside autograd functions) in place
            for i, (graph, comm) in enumerate(self.segments):
                graph.replay()
                if trace is not None:
                    trace.append(("segment", i))
                if comm is not None:
                    comm()
                    if trace is not None:
                        trace.append((getattr(comm, "kind", "comm"), i))


def lib_prof_off():
    _lib.load().srgan_prof_enable(0)     # HIP-event brackets cannot be recorded into a capture
