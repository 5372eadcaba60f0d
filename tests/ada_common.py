"""Yardstick of the adaptive-augmentation tests (csrc/ada.hip, the gated kernels of csrc/augment.hip, srgan_amd.ada): numpy
restatements of the controller, the gate rule, the observe counts and the decoding of a table's slot 7, written from the
specification.  No GPU code.  Everything here is exact by construction -- integer counts, comparisons, one float32 add, one float32
division of two correctly rounded integers -- so every comparison the tests make against it is for equality.

Controller, per observed discriminator update (p, target, step, p_max float32; the counts Python ints):
    n_pos += #(v > thr);  n_neg += #(v < thr);  n_total += #elements     over the first B rows of every map (a NaN: n_total only)
    seen += 1
    if seen == interval:
        r = float32(n_pos - n_neg) / float32(n_total);  d = (r > target) - (r < target)
        p = min(max(p + d * step, 0), p_max);  n_pos = n_neg = n_total = seen = 0;  adjustments += 1;  last_r = r
Gate: bit g of a sample's skip mask is set iff not (u_g < p), g = colour, translation, cutout.
Slot 7 of a gated table row: clamped to [-2^29, 2^29] (a NaN reads -2^29), truncated to an integer, masked with 7.
"""
import numpy as np

F32 = np.float32
FIELDS = ("p", "target", "step", "p_max", "interval", "seen", "n_pos", "n_neg", "n_total", "adjustments", "last_r")


def new_state(p, target, step, p_max, interval):
    return dict(p=F32(p), target=F32(target), step=F32(step), p_max=F32(p_max), interval=int(interval), seen=0, n_pos=0, n_neg=0,
                n_total=0, adjustments=0, last_r=F32(0))


def step_size(batch, interval, kimg):
    return F32(batch * interval / (kimg * 1000.0))


def observe_counts(maps, rows_first, thr):
    """(pos, neg, total) over rows [0, rows_first) of every map (arrays whose first axis is the batch)"""
    thr = F32(thr)
    pos = neg = tot = 0
    for m in maps:
        v = np.asarray(m, dtype=F32)[:rows_first].reshape(-1)
        pos += int(np.count_nonzero(v > thr))
        neg += int(np.count_nonzero(v < thr))
        tot += int(v.size)
    return pos, neg, tot


def controller(st, pos, neg, tot):
    """one observed update: the counts of ``observe_counts`` into the state dict, in place; -> st"""
    st["n_pos"] += pos
    st["n_neg"] += neg
    st["n_total"] += tot
    st["seen"] += 1
    if st["seen"] == st["interval"]:
        r = F32(st["n_pos"] - st["n_neg"]) / F32(st["n_total"])
        d = F32(int(r > st["target"]) - int(r < st["target"]))
        p = F32(st["p"] + F32(d * st["step"]))
        st["p"] = F32(min(max(p, F32(0)), st["p_max"]))
        st["last_r"] = F32(r)
        st["n_pos"] = st["n_neg"] = st["n_total"] = st["seen"] = 0
        st["adjustments"] += 1
    return st


def observe(st, maps, rows_first, thr):
    return controller(st, *observe_counts(maps, rows_first, thr))


def same_record(got, st):
    """a record read from the device (dict of Python values) against the restated state: every field, for equality"""
    for k in FIELDS:
        a, b = got[k], st[k]
        if isinstance(b, (F32, float)):
            assert F32(a) == F32(b), (k, a, b, got, st)
        else:
            assert int(a) == int(b), (k, a, b, got, st)


def gate_masks(uniforms, p):
    """uniforms float32 [n, groups], p float32 -> int64 [n]: bit g set iff not (u_g < p)"""
    u = np.asarray(uniforms, dtype=F32)
    skip = ~(u < F32(p))                               # a NaN compares false: skipped
    return sum(skip[:, g].astype(np.int64) << g for g in range(u.shape[1]))


def gate_rows(rows, p, n_groups=3):
    """rows float32 [n, 16] -> the table float32 [n, 8]: slots 0..6 copied (bit for bit), slot 7 the float of the mask over the
    first ``n_groups`` uniforms (slots 8 .. 8 + n_groups - 1)"""
    rows = np.asarray(rows, dtype=F32)
    out = rows[:, :8].copy()
    out[:, 7] = gate_masks(rows[:, 8:8 + n_groups], p).astype(F32)
    return out


def slot7_mask(v):
    """what the gated kernels make of slot 7, whatever the float holds"""
    v = float(v)
    if v != v:
        v = -536870912.0
    return int(min(max(v, -536870912.0), 536870912.0)) & 7
