"""Exponential moving average (EMA) of the weights used for sampling -- the generator, and the style encoder whose ``mu``
feeds it in the reference-guided calls.  Extension: the reference keeps no averaged weights.

The update of number n = 1, 2, ... is ``e <- e + c_n * (p - e)`` with ``c_n = 1 - d_n`` and
``d_n = min(decay, (1 + n) / (10 + n))`` (``ramp``) or ``decay``: two launches for all tensors of all averaged networks
(``ops.ema_multi_dev_``).  n lives in a device record next to the decay, so a train step captured into a hipGraph advances it
on every replay; ``WeightEMA.updates`` mirrors it on the host.  Batch-norm buffers are carried over bit for bit in the same
launch.  The pointer table is static (neither the live tensors nor the copies ever move) and is uploaded once.
"""
import copy
import struct

import numpy as np
import torch

from . import dp, ops

__all__ = ["decay_at", "make_copy", "read_state", "WeightEMA"]

KIND_AVERAGE, KIND_COPY = 0, 1


def decay_at(n, decay, ramp):
    """d_n of update number ``n`` (1-based) as the device evaluates it: in double, rounded to float32 once."""
    d = float(np.float32(decay))
    if ramp:
        d = min(d, (1.0 + n) / (10.0 + n))
    return np.float32(d)


def make_copy(net):
    """The averaged twin of ``net`` (a module or a ``dp.DataParallel`` wrapper) at its current weights: same class, same
    ``state_dict()`` keys / shapes / dtypes, eval mode, no gradients.  Works on CPU modules."""
    twin = copy.deepcopy(dp.unwrap(net))
    twin.eval()
    twin.requires_grad_(False)
    return twin


def read_state(state):
    """(n, ramp, decay, c) of a device record; synchronises."""
    return tuple(ops.ema_state_read(state).values())


def _records(live, twin):
    """[(dst, src, numel, kind)] of one network; the tensors are kept by the caller."""
    recs = []
    lp, tp = dict(live.named_parameters()), dict(twin.named_parameters())
    lb, tb = dict(live.named_buffers()), dict(twin.named_buffers())
    if list(lp) != list(tp) or list(lb) != list(tb):
        raise RuntimeError("ema: the copy's parameters / buffers do not match the live network's")
    for name, p in lp.items():
        e = tp[name]
        if p.dtype != torch.float32 or e.dtype != torch.float32 or not p.is_contiguous() or not e.is_contiguous() or p.shape != e.shape:
            raise RuntimeError(f"ema: parameter {name} must be contiguous float32 on both sides")
        if p.numel():
            recs.append((e.data_ptr(), p.data_ptr(), p.numel(), KIND_AVERAGE))
    for name, b in lb.items():
        e = tb[name]
        nbytes = b.numel() * b.element_size()
        if b.dtype != e.dtype or b.shape != e.shape or not b.is_contiguous() or not e.is_contiguous() or nbytes % 4:
            raise RuntimeError(f"ema: buffer {name} must be contiguous, of one dtype on both sides and a multiple of 4 bytes")
        if nbytes:
            recs.append((e.data_ptr(), b.data_ptr(), nbytes // 4, KIND_COPY))
    return recs


def build_table(records, device):
    """records [(dst, src, numel, kind)] -> (device table, n_records, total_chunks): five 64-bit words per record, the fifth the
    index of the record's first chunk in the flat chunk list the kernel walks."""
    chunk = ops.ema_chunk()
    rows, at = [], 0
    for dst, src, numel, kind in records:
        rows.extend((dst, src, numel, kind, at))
        at += -(-numel // chunk)
    table = ops.upload_small(struct.pack(f"{len(rows)}q", *rows), device)
    return table, len(records), at


class WeightEMA:
    """Averaged twins of ``nets`` ({name: live module}); one table and one device record cover all of them."""

    def __init__(self, nets, decay=0.999, ramp=True, updates=0):
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError("ema: decay must lie in [0, 1)")
        ops.refuse_in_capture("ema: the averaged copies first appear inside a hipGraph capture -- enable the EMA between steps")
        self.live = {k: dp.unwrap(v) for k, v in nets.items()}
        self.twins = {k: make_copy(v) for k, v in self.live.items()}
        self.decay, self.ramp, self.updates = float(decay), bool(ramp), int(updates)
        records = [r for k in self.live for r in _records(self.live[k], self.twins[k])]
        if not records:
            raise RuntimeError("ema: nothing to average")
        self.device = next(p for net in self.live.values() for p in net.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError(f"ema: the networks are on {self.device}; the update is a HIP kernel (no CPU fallback)")
        self.table, self.n_records, self.total_chunks = build_table(records, self.device)
        self.state = ops.ema_state_new(self.device, self.decay, self.ramp, self.updates)
        self._params = [p for t in self.twins.values() for p in t.parameters()]

    def update(self):
        """One update of every copy, on the current stream (capturable).  The copies are written through raw pointers: their
        cached packed operands go stale."""
        ops.ema_multi_dev_(self.table, self.n_records, self.total_chunks, self.state)
        self.updates += 1
        ops.mark_stale(self._params)

    # -- the host mirror of n, under the names of optim.Adam's step counters: a recording moves both without running anything
    def host_counters(self):
        return self.updates

    def restore_host_counters(self, snap):
        self.updates = snap

    def counters_since(self, snap):
        return self.updates - snap

    def advance_host(self, delta):
        """A replayed graph ran ``delta`` updates on the device: move the host mirror and drop the copies' cached operands."""
        self.updates += delta
        ops.mark_stale(self._params)

    def set_decay(self, decay):
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError("ema: decay must lie in [0, 1)")
        ops.refuse_in_capture("ema: decay changed inside a hipGraph capture")
        ops.ema_state_set_decay(self.state, decay)
        self.decay = float(decay)

    def reseed(self, decay, ramp, updates):
        """Re-seed the device record IN PLACE (a recording that points at it stays valid)."""
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError("ema: decay must lie in [0, 1)")
        ops.refuse_in_capture("ema: record re-seeded inside a hipGraph capture")
        ops.ema_state_init(self.state, decay, ramp, updates)
        self.decay, self.ramp, self.updates = float(decay), bool(ramp), int(updates)

    def device_updates(self):
        """n read back from the device record (synchronises)."""
        return read_state(self.state)[0]

    def graph_keepalive(self):
        return [self.state, self.table]

    def fingerprint(self):
        return (id(self), self.state.data_ptr(), self.table.data_ptr(), self.n_records, self.total_chunks)

    def state_dict(self):
        out = {k: {n: v.detach().clone() for n, v in t.state_dict().items()} for k, t in self.twins.items()}
        out.update(updates=self.updates, decay=self.decay, ramp=self.ramp)
        return out

    def load_state_dict(self, sd):
        for k, t in self.twins.items():
            t.load_state_dict(sd[k])          # in place: the table keeps pointing at the same storage
        self.reseed(sd["decay"], sd["ramp"], sd["updates"])
        ops.mark_stale(self._params)          # the copies' cached packed operands describe the weights before the load
