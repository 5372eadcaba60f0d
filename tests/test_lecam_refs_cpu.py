"""CPU: the parts of LeCam regularisation (srgan_amd.lecam, csrc/lecam.hip, SRGAN_training.enable_lecam) that need no GPU -- the
record's layout against ctypes and its write masks through a host program, the restatement of tests/lecam_common.py against autograd
and its recurrences by hand, the numpy emulation of the summation order, the object, the trainer's interface and refusals, the
checkpoint section and the C ABI's argument checks."""
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import lecam_common as lc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from srgan_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.srgan_last_error().decode()


# ---- the record -----------------------------------------------------------------------------------------------------------------------
def test_layout_matches_the_library_and_the_literal_offsets(lib):
    from srgan_amd import _lib
    offsets = dict(weight=0, decay=4, start=8, updates=12, a_real=16, a_fake=32, penalty=48, applied=52)
    layout = _lib.LcState
    assert issubclass(layout, ctypes.Structure)
    assert ctypes.sizeof(layout) == 56 == lib.srgan_lc_state_bytes() <= 64            # the image a record write carries holds 64
    assert [f for f, _ in layout._fields_] == list(offsets)
    assert {f: getattr(layout, f).offset for f in offsets} == offsets
    assert {f: getattr(layout, f).size for f in offsets} == {f: 16 if f in ("a_real", "a_fake") else 4 for f in offsets}


def test_the_write_masks_by_a_host_program(tmp_path):
    """lecam_host_check.cpp static_asserts the layout and the two masks against literals and replays the kernel's store rule"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = os.path.join(str(tmp_path), "lecam_host_check")
    inc = os.path.join(os.path.dirname(HERE), "style-restricted_gan_amd", "csrc")
    built = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I" + inc, os.path.join(HERE, "lecam_host_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "lecam record ok", (r.stdout, r.stderr[-2000:])


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("shape", lc.SHAPES, ids=str)
def test_the_closed_gradient_equals_autograd_at_float64(shape, clamp):
    """detached anchors; both phi; the empty groups are in the list; back rows get exactly zero"""
    S, P, B1, per, rows = shape
    outs = [o.double().requires_grad_(True) for o in lc.make_maps(S, P, per, rows, seed=P + per)]
    g = torch.Generator().manual_seed(3)
    a_r, a_f = (torch.randn(S, generator=g).double() * 0.5 for _ in range(2))
    R = lc.term(outs, a_r, a_f, P, B1, clamp)
    auto = torch.autograd.grad(R, outs, allow_unused=True)
    closed = lc.grad_closed(outs, a_r, a_f, P, B1, clamp)
    for s in range(S):
        want = auto[s] if auto[s] is not None else torch.zeros_like(outs[s])
        assert float((closed[s] - want).abs().max()) <= 1e-15 * max(1.0, float(want.abs().max())), (shape, clamp, s)
        assert not closed[s][P:].any()
    if clamp:                               # the one-sided form is the two-sided one with the negative differences taken out
        both = lc.term(outs, a_r, a_f, P, B1, False)
        assert float(R.detach()) <= float(both.detach())
    assert float(R.detach()) >= 0


def test_the_term_by_hand():
    o = [torch.tensor([[1.0, 3.0], [0.0, 2.0], [5.0, 7.0]], dtype=torch.float64)]       # P = 2 of 3 rows: row 0 real, row 1 generated
    a_r, a_f = [2.0], [1.5]
    # real: (1 - 1.5)^2, (3 - 1.5)^2 -> mean 1.25; generated: (2 - 0)^2, (2 - 2)^2 -> mean 2
    assert float(lc.term(o, a_r, a_f, 2, 1, False)) == 3.25
    # relu: real -0.5 -> 0, 1.5 -> 2.25 / 2; generated 2 -> 4 / 2
    assert float(lc.term(o, a_r, a_f, 2, 1, True)) == 1.125 + 2.0
    g = lc.grad_closed(o, a_r, a_f, 2, 1, True)[0]
    assert g.tolist() == [[0.0, 1.5], [-2.0, 0.0], [0.0, 0.0]]                          # 2 / (1 * 2) * phi, the back row untouched


def _maps(seed, S=2, P=6, per=11, rows=6):
    return lc.make_maps(S, P, per, rows, seed)


def test_first_update_sets_the_anchors_and_the_recurrence_follows():
    rec = lc.new_record(0.5, 0.75, 0, 2)
    o1, o2 = _maps(1), _maps(2)
    vals, incr, rec1, (m_r, m_f) = lc.call(o1, rec, 6, 2, False, 1.25, torch.float64)
    assert rec1["updates"] == 1 and rec1["applied"] == 1
    assert rec1["a_real"] == [float(m) for m in m_r] and rec1["a_fake"] == [float(m) for m in m_f]      # d = 0 on the first update
    assert float(vals[1]) == 0.5 * float(vals[0]) and float(vals[2]) == 1.25 + float(vals[1]) and rec1["penalty"] == float(vals[0])
    assert rec["updates"] == 0 and rec["a_real"] == [0.0, 0.0]                                           # the input is not modified
    _, _, rec2, (m_r2, _) = lc.call(o2, rec1, 6, 2, False, 0.0, torch.float64)
    assert rec2["updates"] == 2
    for s in range(2):
        assert rec2["a_real"][s] == pytest.approx(0.75 * rec1["a_real"][s] + 0.25 * float(m_r2[s]), rel=1e-15)
    # the term reads the UPDATED anchors
    want = lc.term([o.double() for o in o2], rec2["a_real"], rec2["a_fake"], 6, 2, False)
    assert lc.call(o2, rec1, 6, 2, False, 0.0, torch.float64)[0][0] == want


def test_the_start_boundary_and_a_zero_weight():
    rec = lc.new_record(2.0, 0.5, 2, 2)
    total_in = 0.75
    for i in range(4):
        vals, incr, rec, _ = lc.call(_maps(10 + i), rec, 6, 3, True, total_in, torch.float64)
        active = i >= 2
        assert rec["applied"] == int(active) and rec["updates"] == i + 1
        assert float(vals[0]) > 0                                                        # R is reported during the warm-up too
        assert (float(vals[1]) == 2.0 * float(vals[0])) if active else (float(vals[1]) == 0.0 and float(vals[2]) == total_in)
        assert all(bool(g.any()) == active for g in incr)
    rec0 = lc.new_record(0.0, 0.5, 0, 2)
    vals, incr, rec0, _ = lc.call(_maps(3), rec0, 6, 3, False, total_in, torch.float64)
    assert rec0["applied"] == 0 and rec0["updates"] == 1 and any(rec0["a_real"]) and not any(bool(g.any()) for g in incr)
    assert float(vals[2]) == total_in


def test_a_non_finite_batch_neither_moves_nor_counts():
    rec = lc.new_record(1.0, 0.5, 0, 2)
    _, _, rec, _ = lc.call(_maps(1), rec, 6, 3, False, 0.0, torch.float64)
    for poison in (float("nan"), float("inf")):
        bad = _maps(2)
        bad[1][4, 3] = poison                                                            # ONE generated element of ONE scale
        vals, _, after, _ = lc.call(bad, rec, 6, 3, False, 0.0, torch.float64)
        assert after["updates"] == 1 and after["a_real"] == rec["a_real"] and after["a_fake"] == rec["a_fake"]
        assert after["applied"] == 1 and not np.isfinite(float(vals[0]))                 # the step's gradient guard is what skips it
    back = _maps(2)
    back_rows = [torch.cat([o, torch.full_like(o, float("nan"))], 0) for o in back]     # NaN in the back rows is nobody's business
    a = lc.call(back, rec, 6, 3, False, 0.0, torch.float64)
    b = lc.call(back_rows, rec, 6, 3, False, 0.0, torch.float64)
    assert torch.equal(a[0], b[0]) and a[2] == b[2]


def test_an_empty_group_keeps_its_anchor_and_drops_its_half():
    rec = lc.new_record(1.0, 0.5, 0, 2)
    rec["a_real"], rec["a_fake"], rec["updates"] = [0.25, 0.5], [0.75, 1.0], 3
    o = _maps(5)
    vals, incr, after, _ = lc.call(o, rec, 6, 0, False, 0.0, torch.float64)             # no real row
    assert after["a_real"] == [0.25, 0.5] and after["a_fake"] != rec["a_fake"] and after["updates"] == 4
    want = sum(((a - t.double()) ** 2).mean() for a, t in zip([0.25, 0.5], o)) / 2
    assert float(vals[0]) == pytest.approx(float(want), rel=1e-14)
    vals, incr, after, _ = lc.call(o, rec, 6, 6, False, 0.0, torch.float64)             # no generated row
    assert after["a_fake"] == [0.75, 1.0] and after["a_real"] != rec["a_real"] and np.isfinite(float(vals[0]))


# ---- the emulation of the summation order --------------------------------------------------------------------------------------------
def test_the_emulated_order_sums_what_it_should():
    rng = np.random.default_rng(0)
    for N, n1 in ((1, 1), (5, 2), (1023, 400), (1024, 0), (4100, 4100), (33000, 16000)):
        x = rng.integers(-8, 9, N).astype(np.float32)                                    # integers: every order gives the exact sum
        sr, sf = lc.emulate_sums(x, n1)
        assert sr == x[:n1].sum(dtype=np.float64) and sf == x[n1:].sum(dtype=np.float64), (N, n1)
        assert sr.dtype == np.float32
    x = (rng.standard_normal(33000) * 0.7 + 0.3).astype(np.float32)
    sr, sf = lc.emulate_sums(x, 16000)
    L = lc.chain_depth(33000)
    assert L == 4 * 33                                                                   # 8250 quads over 256 threads
    for got, part in ((sr, x[:16000]), (sf, x[16000:])):
        ref = part.astype(np.float64).sum()
        assert abs(float(got) - ref) <= (L + 16) * lc.EPS32 * np.abs(part).astype(np.float64).sum()
    assert lc.chain_depth(1) == 4 and lc.chain_depth(1024) == 4 and lc.chain_depth(1025) == 8


# ---- the object, the trainer's interface ----------------------------------------------------------------------------------------------
def test_validation_fingerprint_and_state_dict_without_a_record():
    from srgan_amd.lecam import LeCam
    nan, inf = float("nan"), float("inf")
    for bad, what in ((dict(weight=-1.0), "weight"), (dict(weight=nan), "weight"), (dict(weight=inf), "weight"), (dict(weight="x"), "weight"),
                      (dict(decay=1.0), "decay"), (dict(decay=-0.1), "decay"), (dict(decay=nan), "decay"), (dict(start=-1), "start"),
                      (dict(start=1.5), "start"), (dict(start=True), "start"), (dict(clamp=2), "clamp"), (dict(clamp="yes"), "clamp")):
        with pytest.raises(ValueError, match=what):
            LeCam(**bad)
    a = LeCam(2.0, 0.9, 3, clamp=True)
    fp = a.fingerprint()
    a.set(weight=5.0)
    a.set(decay=0.5, start=0)
    assert a.fingerprint() == fp and (a.weight, a.decay, a.start) == (5.0, 0.5, 0)        # the settings are device state
    assert LeCam(5.0, 0.5, 0, clamp=True).fingerprint() != fp                             # another object
    assert a.fingerprint()[1] is True and LeCam().fingerprint()[1] is False
    with pytest.raises(ValueError, match="set_lecam.*decay"):
        a.set(decay=1.5)
    assert (a.weight, a.decay, a.start) == (5.0, 0.5, 0)
    assert a.graph_keepalive() == [] and a.state is None
    assert a.stats() == dict(weight=5.0, decay=0.5, start=0, updates=0, a_real=[0.0] * 4, a_fake=[0.0] * 4, penalty=0.0, applied=0,
                             clamp=True)
    sd = a.state_dict()
    assert sd == dict(weight=5.0, decay=0.5, start=0, clamp=True, a_real=[0.0] * 4, a_fake=[0.0] * 4, updates=0)
    b = LeCam(clamp=True)
    b.load_state_dict(sd)
    assert (b.weight, b.decay, b.start) == (5.0, 0.5, 0) and b.state is None
    with pytest.raises(ValueError, match="clamp"):
        LeCam(clamp=False).load_state_dict(sd)
    with pytest.raises(ValueError, match="without a device"):
        b.restore(3, [0.0] * 4, [0.0] * 4)
    with pytest.raises(ValueError, match=">= 0"):
        b.restore(-1, [0.0] * 4, [0.0] * 4)


def _cpu_trainer(k=2):
    from srgan_amd import model, trainer
    D = model.SingleDiscriminator_solo_multi(3, 4, 2, 4, "instance", 4)
    G = model.SingleGenerator(3, 4, 2, 2, 1, "instance", num_con=12)
    E = model.Encoder(3, 8, 4, 4, "instance", 4, "cpu")
    lbd = dict(**{"class": 1.0}, cycle=5.0, idt=5.0, reg=0.5, idt_reg=0.5, KL=0.0, batch_KL=10.0, corr_enc=100.0, hist=0.0)
    crit = [torch.nn.MSELoss(), torch.nn.MSELoss()]
    return trainer.SRGAN_training([G, D, E], [None, None, None], crit, lbd, k, "cpu", np.eye(4), batch_size=4, encoded_feature="mu",
                                  ndim=8)


def test_trainer_api_without_a_gpu(monkeypatch):
    from srgan_amd import dp, lecam, trainer
    sg = _cpu_trainer()
    assert sg._lecam is None and sg.lecam_stats() is None and "lecam" not in sg._ckpt_sections()
    with pytest.raises(RuntimeError, match="enable_lecam"):
        sg.set_lecam(weight=1.0)
    sg.enable_r1()
    sg.enable_bcr(seed=1)
    sg.enable_mode_seeking(seed=2)
    n_ext = len(sg._extensions())
    assert sg.enable_lecam() is sg
    obj = sg._lecam
    assert isinstance(obj, lecam.LeCam) and (obj.weight, obj.decay, obj.start, obj.clamp) == (0.3, 0.99, 0, False)
    ext = sg._extensions()
    assert len(ext) == n_ext + 1 and ext.index(obj) == ext.index(sg.bcr) + 1 == ext.index(sg._ms) - 1      # after bcr
    assert sg.lecam_stats() == dict(weight=0.3, decay=0.99, start=0, updates=0, a_real=[0.0] * 4, a_fake=[0.0] * 4, penalty=0.0,
                                    applied=0, clamp=False)
    sg.set_lecam(weight=0.5, start=4)
    assert sg._lecam is obj and (obj.weight, obj.decay, obj.start) == (0.5, 0.99, 4)
    assert "lecam" in sg._ckpt_sections()
    sg.enable_lecam(1.0, 0.5, 2, clamp=True)
    assert sg._lecam is not obj and sg._lecam.clamp and len(sg._extensions()) == n_ext + 1
    for bad in (dict(weight=-1.0), dict(decay=1.0), dict(start=-1), dict(clamp=3)):
        with pytest.raises(ValueError):
            sg.enable_lecam(**bad)
    assert sg._lecam.clamp                                                                # a refused call leaves the old one
    sg.disable_lecam()
    assert sg._lecam is None and len(sg._extensions()) == n_ext and sg.lecam_stats() is None
    doc = trainer.SRGAN_training.enable_lecam.__doc__
    assert "not taken from" in doc and "much smaller weight" in doc
    # more than one rank, the generic discriminator path, the other trainer: each names its way out
    monkeypatch.setattr(dp, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match=r"2 ranks.*disable_lecam"):
        sg.enable_lecam()
    monkeypatch.undo()
    assert sg._lecam is None
    sg._fused_paths = lambda: False
    with pytest.raises(NotImplementedError, match=r"fused discriminator pass.*disable_lecam"):
        sg.enable_lecam()
    assert sg._lecam is None
    with pytest.raises(NotImplementedError, match="SRGAN_training.enable_lecam"):
        trainer.SingleGAN_training.enable_lecam(object())


def test_enabling_and_disabling_drop_a_recording_and_set_keeps_it():
    class FakeGraph:
        dropped = 0

        def _drop(self):
            self.dropped += 1

    sg = _cpu_trainer()
    sg._graph = FakeGraph()
    sg.enable_lecam()
    assert sg._graph.dropped == 1
    sg.set_lecam(weight=1.0, decay=0.5, start=3)
    assert sg._graph.dropped == 1
    sg.enable_lecam(clamp=True)
    assert sg._graph.dropped == 2
    sg.disable_lecam()
    assert sg._graph.dropped == 3


def test_checkpoint_section_round_trips_through_weights_only():
    sg = _cpu_trainer()
    sg.opt_sche_initialization()
    assert "lecam" not in sg.state_dict()
    sg.enable_lecam(2.0, 0.5, 3, clamp=True)
    sd = sg.state_dict()
    assert sd["lecam"] == dict(weight=2.0, decay=0.5, start=3, clamp=True, a_real=[0.0] * 4, a_fake=[0.0] * 4, updates=0)
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    back = torch.load(buf, map_location="cpu", weights_only=True)
    assert back["lecam"] == sd["lecam"]
    other = _cpu_trainer()
    other.opt_sche_initialization()
    with pytest.raises(ValueError, match="unexpected|missing"):
        other.enable_lecam().load_state_dict({k: v for k, v in back.items() if k != "lecam"})
    first = other._lecam
    rep = other.load_state_dict(back)                            # another clamp: the section makes a new object
    assert rep.missing == [] and rep.unexpected == []
    assert other._lecam is not first and other._lecam.clamp
    assert (other._lecam.weight, other._lecam.decay, other._lecam.start) == (2.0, 0.5, 3)
    kept = other._lecam
    other.set_lecam(weight=9.0)
    other.load_state_dict(back)                                  # the same clamp: the object stays, the settings are the saved ones
    assert other._lecam is kept and kept.weight == 2.0
    other.disable_lecam()
    other.load_state_dict(back)                                  # off: enabled with the saved settings
    assert other._lecam is not None and other._lecam.clamp and other._lecam.start == 3


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_back_before_any_launch(lib):
    buf = (ctypes.c_char * 4096)()
    b = ctypes.byref(buf)
    nan, inf = float("nan"), float("inf")
    for w, d, start in ((-1.0, 0.5, 0), (nan, 0.5, 0), (inf, 0.5, 0), (1.0, 1.0, 0), (1.0, -0.25, 0), (1.0, nan, 0), (1.0, inf, 0),
                        (1.0, 0.5, -1)):
        assert lib.srgan_lc_state_init(b, w, d, start, None) == -1 and "lc_state_init" in _err(lib), (w, d, start)
        assert lib.srgan_lc_state_set(b, w, d, start, None) == -1 and "lc_state_set" in _err(lib), (w, d, start)
    assert lib.srgan_lc_state_init(None, 1.0, 0.5, 0, None) == -1 and "lc_state_init" in _err(lib)
    assert lib.srgan_lc_state_set(None, 1.0, 0.5, 0, None) == -1 and "lc_state_set" in _err(lib)
    four = ctypes.c_float * 4
    good = four(0.0, 1.0, 2.0, 3.0)
    restore = lib.srgan_lc_state_restore
    assert restore(None, 0, good, good, None) == -1 and "lc_state_restore" in _err(lib)
    assert restore(b, 0, None, good, None) == -1 and "lc_state_restore" in _err(lib)
    assert restore(b, 0, good, None, None) == -1 and "lc_state_restore" in _err(lib)
    assert restore(b, -1, good, good, None) == -1 and "updates >= 0" in _err(lib)
    for poison in (nan, inf, -inf):
        assert restore(b, 1, four(0.0, poison, 0.0, 0.0), good, None) == -1 and "anchor 1 is not finite" in _err(lib)
        assert restore(b, 1, good, four(0.0, 0.0, 0.0, poison), None) == -1 and "anchor 3 is not finite" in _err(lib)
    # the launch
    maps = (ctypes.c_void_p * 5)(*[0x20000000 + (i << 20) for i in range(5)])
    per = (ctypes.c_longlong * 5)(16, 4, 4, 4, 4)
    tot, vals = ctypes.c_void_p(0x31000000), ctypes.c_void_p(0x31000010)
    fn = lib.srgan_lecam

    def call(o=maps, per_row=per, S=2, rows=4, pairs=4, rows_first=2, clamp=0, total_in=tot, v=vals, d_o=maps, state=b):
        return fn(o, per_row, S, rows, pairs, rows_first, clamp, total_in, v, d_o, state, None)

    for name in ("o", "per_row", "total_in", "v", "d_o", "state"):
        assert call(**{name: None}) == -1 and "null pointer" in _err(lib), name
    for S in (0, 5, -1):
        assert call(S=S) == -1 and f"{S} scales (1..4)" in _err(lib)
    for rows, pairs in ((5, 4), (3, 4), (12, 4), (0, 0), (7, 3)):
        assert call(rows=rows, pairs=pairs) == -1 and f"rows = {rows}" in _err(lib), (rows, pairs)
    assert call(rows=8, pairs=4, rows_first=5) == -1 and "rows_first = 5" in _err(lib)
    assert call(rows_first=-1) == -1 and "rows_first = -1" in _err(lib)
    for clamp in (2, -1):
        assert call(clamp=clamp) == -1 and f"clamp = {clamp}" in _err(lib)
    assert call(per_row=(ctypes.c_longlong * 2)(16, 0)) == -1 and "null scale" in _err(lib)
    assert call(per_row=(ctypes.c_longlong * 2)(16, 1 << 29)) == -1 and "2^31" in _err(lib)
    assert call(rows=8, pairs=4, per_row=(ctypes.c_longlong * 2)(1 << 28, 4)) == -1 and "2^31" in _err(lib)   # rows, not pairs, counts
    assert call(o=(ctypes.c_void_p * 2)(0x20000000, 0)) == -1 and "null scale" in _err(lib)
    assert call(d_o=(ctypes.c_void_p * 2)(0, 0x20000000)) == -1 and "null scale" in _err(lib)
    assert call(o=(ctypes.c_void_p * 2)(0x20000002, 0x20100000)) == -1 and "aligned" in _err(lib)
    assert call(v=ctypes.c_void_p(0x31000012)) == -1 and "aligned" in _err(lib)
