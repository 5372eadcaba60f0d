"""R1 gradient penalty on real samples (Mescheder et al., 2018), ``gamma / 2 * E_x |grad_x D(x)|^2``, for the two-scale
discriminator ``SingleDiscriminator_solo_multi`` -- an extension, the reference has no gradient penalty.

The convolution Functions of ``ops`` have no double backward, and this discriminator does not need one: bias-free convolutions,
LeakyReLU, one bias conv per head and a 3x3 / stride-2 average pool in front of the second scale make it piecewise linear in
``x``.  Per scale, with trunk layers ``l = 1..L`` (weights ``W_l``), head ``W_o`` and ``phi'_l = 1 where y_l > 0 else slope``:

    forward      y_0 = x (scale 2: pool(x)), y_l = lrelu(conv(W_l, y_{l-1})), o = conv(W_o, y_L) + b_o
    S_n          sum over the scales of the MEAN over the patches of o[n]      (the class heads do not enter)
    chain        q_L = dgrad(W_o, 1 / P_s) * phi'_L, q_{l-1} = dgrad(W_l, q_l) * phi'_{l-1}, h_0 = dgrad(W_1, q_1)
    g            h_0 of scale 1 + pool^T(h_0 of scale 2);  P = gamma_eff / (2 N) * sum_n |g_n|^2,  gamma_eff = gamma * every
    seed         u_0 = gamma_eff / N * g  (= dP/dg); scale 2 starts from pool(u_0)
    tangent      u_l = conv(W_l, u_{l-1}) * phi'_l
    gradients    dP/dW_l = wgrad(x = u_{l-1}, dy = q_l), dP/dW_o = wgrad(x = u_L, dy = 1 / P_s); biases and class heads: none

(``h`` is linear in each ``W_l`` and ``phi'' = 0`` almost everywhere.)  Everything runs on the library's forward, input-gradient
and weight-gradient entry points, ``srgan_act_bwd`` for the masks, the pool kernels and the two kernels of ``csrc/r1.hip``
(``ops.r1_seed_`` / ``ops.r1_finalize_``).  No atomics, one stream, a fixed order: deterministic.  ``gamma`` and ``every`` live in a
device record, so ``set_gamma`` between steps keeps a recorded hipGraph valid."""
import torch

from . import _lib, ops
from .ops import ACT_LRELU, ACT_NONE, PAD_REFLECT, PAD_ZERO

__all__ = ["R1Penalty", "r1_accumulate"]


def check_gamma_every(gamma, every, what="R1Penalty"):
    """-> (float gamma, int every); ValueError for gamma < 0 (or not finite), every < 1 or not an integer."""
    try:
        g = float(gamma)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: gamma must be a number >= 0, got {gamma!r}") from None
    if not (g >= 0.0 and g < float("inf")):
        raise ValueError(f"{what}: gamma must be finite and >= 0, got {gamma!r}")
    if isinstance(every, bool) or not isinstance(every, int) and not (hasattr(every, "__index__")):
        raise ValueError(f"{what}: every must be an integer >= 1, got {every!r}")
    e = int(every)
    if e < 1:
        raise ValueError(f"{what}: every must be an integer >= 1, got {every!r}")
    return g, e


def schedule(k, every):
    """Which of a step's k discriminator updates are penalised: update i iff i % every == 0 (static per step)."""
    return [i % every == 0 for i in range(k)]


class R1Penalty(ops.RecordOwner):
    """``gamma``, ``every`` (lazy regularisation: the caller penalises every ``every``-th update, with ``gamma_eff = gamma *
    every``) and the device side of the penalty: the record, the constant seed tensors (``1 / P_s`` per head) and the partial-sum
    workspace, made at the first use of a batch geometry -- never inside a hipGraph capture."""

    layout = _lib.R1State

    def __init__(self, gamma=10.0, every=1):
        self.gamma, self.every = check_gamma_every(gamma, every)
        self.state = None
        self._n = None
        self._bufs = {}            # (N, H, W) -> (workspace, [constant seed per scale])

    # -- device side -----------------------------------------------------------------------------------------------------------
    def _ensure(self, device, n):
        if self.state is None:
            self._make_record(ops.r1_state_new, device, self.gamma, self.every, n)
            self._n = n
        elif self._n != n:
            ops.refuse_in_capture("R1Penalty: the batch size changed inside a hipGraph capture; run one eager step first")
            ops.r1_state_set(self.state, self.gamma, self.every, n)
            self._n = n

    def _buffers(self, device, n, h, w, head_hw):
        key = (n, h, w)
        hit = self._bufs.get(key)
        if hit is None:
            ops.refuse_in_capture("R1Penalty: workspaces of a new batch geometry would be allocated inside a hipGraph capture; "
                                  "run one eager step first")
            ws = torch.empty(ops.r1_workspace_bytes(n, h, w), dtype=torch.uint8, device=device)
            seeds = []
            for ho, wo in head_hw:
                seeds.append(ops.nhwc_empty(n, 1, ho, wo, device).fill_(1.0 / (ho * wo)))
            hit = self._bufs[key] = (ws, seeds)
        return hit

    def set_gamma(self, gamma):
        """A new ``gamma`` (>= 0), written into the device record between steps: a recorded step reads it from there."""
        self.gamma, _ = check_gamma_every(gamma, self.every, "set_r1_gamma")
        if self.state is not None:
            ops.refuse_in_capture("set_r1_gamma inside a hipGraph capture")
            ops.r1_state_set(self.state, self.gamma, self.every, self._n)

    def set_updates(self, updates, device=None, n=None):
        """Resume: write a checkpoint's count of penalised updates into the device record, between steps.  A penalty that has not
        run yet has no record; it is made here for batch size ``n`` on ``device`` (the step re-derives ``c`` should its batch
        differ).  Without a record and without ``n`` only a count of 0 can be taken: that is what a fresh record starts at."""
        ops.refuse_in_capture("R1Penalty: updates written inside a hipGraph capture")
        updates = int(updates)
        if updates < 0:
            raise ValueError(f"R1Penalty: updates must be >= 0, got {updates}")
        if self.state is None:
            if n is None or device is None:
                if updates:
                    raise ValueError("R1Penalty: a count of updates without the batch size of its record (n)")
                return
            self._ensure(device, int(n))
        ops.r1_state_set_updates(self.state, updates)

    @property
    def gamma_eff(self):
        return self.gamma * self.every

    def penalty(self):
        """The last penalty as a device scalar (a copy of the record's field; no synchronisation)."""
        return self._record_field("penalty")

    def stats(self):
        """The record as a dict (``gamma``, ``every``, ``c``, ``penalty``, ``mean_sq_norm``, ``updates``, ``n``); SYNCHRONISES."""
        if self.state is None:
            return dict(gamma=self.gamma, every=self.every, c=None, penalty=0.0, mean_sq_norm=0.0, updates=0, n=None)
        return ops.r1_state_read(self.state)

    # -- hipGraph support -------------------------------------------------------------------------------------------------------
    def graph_keepalive(self):
        out = super().graph_keepalive()
        for ws, seeds in self._bufs.values():
            out += [ws] + list(seeds)
        return out

    def fingerprint(self):
        """What a recording bakes in: the object, ``every`` (the schedule and the launches), the record and the buffers.  Not
        ``gamma``: it is device state."""
        return (id(self), self.every, self._record_ptr(), self._n,
                tuple((k, ws.data_ptr(), tuple(s.data_ptr() for s in seeds)) for k, (ws, seeds) in sorted(self._bufs.items())))


# ---------------------------------------------------------------------------------------------------------------------------
def _layers(D):
    """[(trunk [(conv, slope)], head conv)] of the two scales; NotImplementedError for another layout."""
    from .model import _Conv2d, _LeakyReLU
    need = ("discriminator1", "discriminator2", "last_layer1", "last_layer2", "down", "forward_logits")
    if not all(hasattr(D, a) for a in need):
        raise NotImplementedError(f"r1_accumulate: {type(D).__name__} has no forward_logits / two-scale layout; the closed form "
                                  "serves SingleDiscriminator_solo_multi only (disable_r1(), or that discriminator)")
    out = []
    for trunk, head in ((D.discriminator1, D.last_layer1), (D.discriminator2, D.last_layer2)):
        mods = list(trunk.down_convs)
        pairs = []
        if len(mods) % 2:
            raise NotImplementedError("r1_accumulate: a trunk of conv + LeakyReLU pairs expected")
        for conv, act in zip(mods[0::2], mods[1::2]):
            if not isinstance(conv, _Conv2d) or not isinstance(act, _LeakyReLU) or conv.bias is not None:
                raise NotImplementedError("r1_accumulate: a trunk of bias-free conv + LeakyReLU pairs expected (no norm layers)")
            pairs.append((conv, float(act.negative_slope)))
        if not isinstance(head, _Conv2d):
            raise NotImplementedError("r1_accumulate: the heads must be convolutions")
        out.append((pairs, head))
    return out


def _desc(m, x):
    n, i, hi, wi = x.shape
    w = m.weight
    o, i2, kh, kw = w.shape
    if i != i2:
        raise _lib.SrganHipError(f"r1_accumulate: input has {i} channels, weight expects {i2}")
    stride, pad = m.stride[0], m.padding[0]
    ho, wo = (hi + 2 * pad - kh) // stride + 1, (wi + 2 * pad - kw) // stride + 1
    mode = PAD_REFLECT if m.padding_mode == "reflect" else PAD_ZERO
    return ops._conv_desc(n, hi, wi, i, ho, wo, o, kh, kw, stride, pad, mode, w), (n, o, ho, wo)


def _pool(x):
    n, c, h, w = x.shape
    y = ops.nhwc_empty(n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1, x.device)
    _lib.check(_lib.load().srgan_avgpool3s2_fwd(ops._ptr(x), ops._ptr(y), n, h, w, c, ops._stream()), "srgan_avgpool3s2_fwd")
    return y


def _mask_(y, t, slope):
    """t *= phi'(y) in place"""
    _lib.check(_lib.load().srgan_act_bwd(ops._ptr(y), ops._ptr(t), ops._ptr(t), t.numel(), ACT_LRELU, float(slope), ops._stream()),
               "act_bwd")


def _wgrad_into(m, desc, x, dy):
    """dW of the conv ``m`` from (x, dy), ADDED to ``m.weight.grad`` in the weight-gradient kernel's own epilogue (a weight without
    a gradient yet gets a fresh buffer).  ``m.weight`` is the tensor the convolutions read: for a spectrally normalised layer the
    normalised leaf.  -> the tensor that now is ``m.weight.grad``."""
    w = m.weight
    g = w.grad
    acc = g is not None
    if acc and not (g.dtype == torch.float32 and g.is_contiguous()):
        g = w.grad = g.contiguous().float()
    if not acc:
        g = torch.empty(w.shape, dtype=torch.float32, device=w.device)
    dd = ops.ConvDesc.from_buffer_copy(desc)
    dd.sO, dd.sI, dd.sH, dd.sW = g.stride()
    ws, nb = ops._conv_ws(dd, g.device)
    with ops._wgrad_accumulate(acc):
        ops._run_conv_wgrad(dd, x, dy, g, None, ws, nb)
    if not acc:
        w.grad = g
    return g


def check_supported(D, x):
    """The refusals of the pass, each with its way out."""
    if ops.get_compute_dtype() == "bf16":
        raise NotImplementedError("r1_accumulate: the bf16 compute mode is not served (the masks and the tangent pass are fp32 "
                                  "kernels); ops.set_compute_dtype('fp32'), or disable_r1()")
    if x.dim() != 4 or x.shape[1] != 3:
        raise NotImplementedError(f"r1_accumulate: images of shape {tuple(x.shape)}; [N, 3, H, W] expected")
    if x.shape[2] % 16 or x.shape[3] % 16:
        raise NotImplementedError(f"r1_accumulate: images of {x.shape[2]} x {x.shape[3]}; H and W must be multiples of 16 (the "
                                  "strided input-gradient kernels are tested on such maps only): resize / crop, or disable_r1()")
    return _layers(D)


def r1_accumulate(D, x_real, state, keep=False):
    """Add ``dP/dW`` of ``P = state.gamma_eff / (2 N) * sum_n |grad_x S_n|^2`` at the real rows ``x_real`` to the ``.grad`` of every
    trunk and head weight of the unwrapped two-scale discriminator ``D`` (head biases and class heads get nothing), and write the
    penalty into ``state``'s device record.  Runs under ``no_grad`` with its own forward of ``x_real``; hipGraph-capturable once
    ``state`` has seen the batch geometry.  ``keep=True`` -> a dict with the per-scale activations ``y`` (lists), ``g``-related
    tensors ``h`` (the two input gradients), ``u0`` and the gradient tensors ``dW`` (the ``.grad`` tensors: pure ``dP/dW`` only if
    they were None before); else None."""
    scales = check_supported(D, x_real)
    lib = _lib.load()
    with torch.no_grad():
        x = ops.to_nhwc(x_real.detach())
        ops._require_gpu(x, "r1_accumulate")
        n, _, h, w = x.shape
        state._ensure(x.device, n)
        inputs = [x, _pool(x)]
        # stage 0: forward of the real rows, every y_l kept
        ys, descs, head_hw = [], [], []
        for (pairs, head), x0 in zip(scales, inputs):
            y, yl, dl = x0, [], []
            for conv, slope in pairs:
                d, shp = _desc(conv, y)
                out = ops.nhwc_empty(*shp, x.device)
                ops._run_conv_fwd(d, y, conv.weight, None, out, ACT_LRELU, slope)
                dl.append(d)
                yl.append(out)
                y = out
            d, shp = _desc(head, y)
            dl.append(d)
            head_hw.append((shp[2], shp[3]))
            ys.append(yl)
            descs.append(dl)
        ws, seeds = state._buffers(x.device, n, h, w, head_hw)
        # stage 1: the input-gradient chain, q_l kept for the weight gradients
        qs, hs = [], []
        for (pairs, head), x0, yl, dl, seed in zip(scales, inputs, ys, descs, seeds):
            L = len(pairs)
            ql = [None] * (L + 1)                  # ql[l] = q_l, l = 1..L
            q = torch.empty_like(yl[L - 1])
            ops._run_conv_dgrad(dl[L], seed, head.weight, q, None, yl[L - 1], pairs[L - 1][1])
            ql[L] = q
            for l in range(L, 1, -1):
                q = torch.empty_like(yl[l - 2])
                ops._run_conv_dgrad(dl[l - 1], ql[l], pairs[l - 1][0].weight, q, None, yl[l - 2], pairs[l - 2][1])
                ql[l - 1] = q
            h0 = torch.empty_like(x0)
            ops._run_conv_dgrad(dl[0], ql[1], pairs[0][0].weight, h0)
            qs.append(ql)
            hs.append(h0)
        # stage 2: g = h1 + pool^T(h2), u0 = c g, partials of |g|^2; then the record
        u0 = torch.empty_like(x)
        ops.r1_seed_(hs[0], hs[1], state.state, u0, ws)
        ops.r1_finalize_(ws, n, h, w, state.state)
        # stage 3: the tangent pass and the weight gradients
        dws = []
        for (pairs, head), u, yl, dl, ql, seed in zip(scales, [u0, _pool(u0)], ys, descs, qs, seeds):
            L = len(pairs)
            dwl = []
            for l in range(1, L + 1):
                conv, slope = pairs[l - 1]
                dwl.append(_wgrad_into(conv, dl[l - 1], u, ql[l]))
                nxt = torch.empty_like(yl[l - 1])
                ops._run_conv_fwd(dl[l - 1], u, conv.weight, None, nxt, ACT_NONE, 0.0)
                _mask_(yl[l - 1], nxt, slope)
                u = nxt
            dwl.append(_wgrad_into(head, dl[L], u, seed))
            dws.append(dwl)
    if keep:
        return dict(y=ys, h=hs, q=[ql[1:] for ql in qs], u0=u0, dW=dws)
    return None
