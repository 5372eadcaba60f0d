"""GPU: the one write path of the seven device records (csrc/records.h, record_write in csrc/pointwise.hip).  Every writing entry of
the C ABI runs on a record whose bytes all hold a sentinel; the bytes read back must equal a host ``ctypes.Structure`` that started
from the same sentinel and had exactly the fields set that the entry is documented to write -- so a word too many, a word too few
and a wrong bit all fail.  The records are 16 to 56 bytes: no shapes."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
F = np.float32


@pytest.fixture(scope="module")
def lib():
    from srgan_amd import _lib
    return _lib.load()


def _layout(name):
    from srgan_amd import _lib
    return getattr(_lib, name)


def _run(lib, layout, entry, args, stream=None):
    """the entry on a sentinel-filled record -> the record's bytes"""
    from srgan_amd import _lib
    state = torch.full((ctypes.sizeof(layout),), SENTINEL, dtype=torch.uint8, device="cuda")
    _lib.check(getattr(lib, "srgan_" + entry)(ctypes.c_void_p(state.data_ptr()), *args, stream), entry)
    return state.cpu().numpy().tobytes()


def _expect(layout, fields, start=None):
    """a host record: every byte the sentinel (or ``start``), then the named fields set"""
    rec = layout.from_buffer_copy(bytes([SENTINEL]) * ctypes.sizeof(layout) if start is None else start)
    for k, v in fields.items():
        setattr(rec, k, v)
    return bytes(rec)


def _c(gamma, every, n):
    return float(F(F(gamma) * F(every)) / F(n))


# (layout, entry, arguments, the fields the entry writes and what they must hold)
SETS = [
    ("AdamState", "adam_state_set_lr", (3e-4,), dict(lr=3e-4)),
    ("GuardState", "grad_guard_state_set_max_norm", (2.5,), dict(max_norm=2.5)),
    ("GuardState", "grad_guard_state_set_max_norm", (float("inf"),), dict(max_norm=float("inf"))),
    ("GuardState", "grad_guard_state_set_counters", (11, 3, 4), dict(steps=11, skipped=3, clipped=4)),   # not max_norm, norm, scale, skip
    ("EmaState", "ema_state_set_decay", (0.999,), dict(decay=0.999)),
    ("AdaState", "ada_state_set", (0.6, 1e-3, 0.8, 4, 0, 0.0), dict(target=0.6, step=1e-3, p_max=0.8, interval=4)),
    ("AdaState", "ada_state_set", (0.6, 1e-3, 0.8, 4, 1, 0.3), dict(target=0.6, step=1e-3, p_max=0.8, interval=4, p=0.3)),
    ("AdaState", "ada_state_set_counters", (3, 2 ** 32 + 1, 3, 2 ** 33 + 5, 7, -0.25),
     dict(seen=3, n_pos=2 ** 32 + 1, n_neg=3, n_total=2 ** 33 + 5, adjustments=7, last_r=-0.25)),
    ("R1State", "r1_state_set", (7.0, 2, 3), dict(gamma=7.0, every=2, c=_c(7.0, 2, 3), n=3)),
    ("R1State", "r1_state_set_updates", (12,), dict(updates=12)),
    ("CrState", "cr_state_set", (10.0, 0.3, 2), dict(lambda_real=10.0, lambda_fake=0.3, every=2)),
    ("CrState", "cr_state_set_updates", (5,), dict(updates=5)),
    ("MsState", "ms_state_set", (2.0, 1e-5, 0.7), dict(weight=2.0, eps=1e-5, tau=0.7)),
    ("MsState", "ms_state_restore", (9, 1.5, 0.3, 0.1), dict(updates=9, ms=1.5, d_image=0.3, d_latent=0.1)),   # not weighted
]
# (layout, entry, arguments, the non-zero fields of a fresh record)
INITS = [
    ("AdamState", "adam_state_init", (3e-4, 0.5, 0.999, 1e-8, 17), dict(step=17, lr=3e-4, beta1=0.5, beta2=0.999, eps=1e-8)),
    ("GuardState", "grad_guard_state_init", (2.5,), dict(max_norm=2.5, scale=1.0)),
    ("EmaState", "ema_state_init", (0.999, 7, 21), dict(n=21, ramp=1, decay=0.999)),
    ("AdaState", "ada_state_init", (0.3, 0.6, 1e-3, 0.8, 4), dict(p=0.3, target=0.6, step=1e-3, p_max=0.8, interval=4)),
    ("R1State", "r1_state_init", (7.0, 2, 3), dict(gamma=7.0, every=2, c=_c(7.0, 2, 3), n=3)),
    ("CrState", "cr_state_init", (10.0, 0.3, 2), dict(lambda_real=10.0, lambda_fake=0.3, every=2)),
    ("MsState", "ms_state_init", (2.0, 1e-5, 0.7), dict(weight=2.0, eps=1e-5, tau=0.7)),
]


@pytest.mark.parametrize("case", SETS, ids=lambda c: f"{c[1]}{len(c[3])}")
def test_a_set_entry_writes_its_words_and_no_other(lib, case):
    name, entry, args, fields = case
    layout = _layout(name)
    got, want = _run(lib, layout, entry, args), _expect(layout, fields)
    assert got == want, (got.hex(), want.hex())
    words = {getattr(layout, f).offset // 4 + i for f in fields for i in range(getattr(layout, f).size // 4)}
    for w in range(ctypes.sizeof(layout) // 4):                      # the arguments were chosen so that a written word shows
        assert (got[4 * w:4 * w + 4] != bytes([SENTINEL]) * 4) == (w in words), (entry, w)


@pytest.mark.parametrize("case", INITS, ids=lambda c: c[1])
def test_an_init_entry_writes_every_word(lib, case):
    name, entry, args, fields = case
    layout = _layout(name)
    got = _run(lib, layout, entry, args)
    assert SENTINEL not in got, got.hex()
    assert got == _expect(layout, fields, start=bytes(ctypes.sizeof(layout))), got.hex()


def test_the_64_bit_counters_come_back_exactly():
    from srgan_amd import ops
    state = ops.ada_state_new("cuda", 0.0, 0.6, 1e-3, 0.8, 4)
    ops.ada_state_set_counters(state, 0, 2 ** 32 + 1, 3, 2 ** 33 + 5, 0, 0.0)
    rec = ops.ada_state_read(state)
    assert (rec["n_pos"], rec["n_neg"], rec["n_total"]) == (2 ** 32 + 1, 3, 2 ** 33 + 5)


@pytest.mark.parametrize("entry", ["r1_state_init", "r1_state_set"])
@pytest.mark.parametrize("gamma,every,n", [(10.0, 1, 1), (7.0, 2, 3), (0.1, 16, 6), (1e-3, 3, 7), (0.0, 1, 5)])
def test_r1_c_is_the_fp32_product_then_quotient(lib, entry, gamma, every, n):
    layout = _layout("R1State")
    rec = layout.from_buffer_copy(_run(lib, layout, entry, (gamma, every, n)))
    want = F(F(gamma) * F(every)) / F(n)
    assert F(rec.c).tobytes() == want.tobytes(), (rec.c, want)
    assert (F(rec.gamma).tobytes(), rec.every, rec.n) == (F(gamma).tobytes(), every, n)


def test_init_set_read_back_to_back_on_a_side_stream():
    """the writes are ordinary work of the current stream: no synchronisation between them, the read sees the last one"""
    from srgan_amd import ops
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        state = ops.ms_state_new("cuda", 1.0, 1e-5, 0.0)
        ops.ms_state_set(state, 2.0, 1e-4, 0.7)
        ops.ms_state_restore(state, 9, 1.5, 0.3, 0.1)
        rec = ops.ms_state_read(state)
    want = dict(weight=2.0, eps=1e-4, tau=0.7, ms=1.5, weighted=0.0, d_image=0.3, d_latent=0.1, updates=9)
    assert rec == {k: (v if k == "updates" else float(F(v))) for k, v in want.items()}
    torch.cuda.current_stream().wait_stream(side)
