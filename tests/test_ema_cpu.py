"""CPU: the parts of the weight EMA (srgan_amd.ema, srgan_ema_* of the C ABI) that need no GPU -- argument errors, the layout
of the averaged copies, and the host's decay schedule against the restatement of tests/ema_common.py."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests.ema_common import decay_ref


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from srgan_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.srgan_last_error().decode()


def test_bad_arguments_return_minus_one_without_a_gpu(lib):
    buf = (ctypes.c_char * 4096)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.srgan_ema_state_bytes() == 16 and lib.srgan_ema_chunk() == 4096
    assert lib.srgan_ema_multi_dev(None, 1, 1, b, None) == -1 and "ema_multi_dev" in _err(lib)          # NULL table
    assert lib.srgan_ema_multi_dev(b, 1, 1, None, None) == -1 and "ema_multi_dev" in _err(lib)          # NULL state
    assert lib.srgan_ema_multi_dev(b, 0, 1, b, None) == -1 and "ema_multi_dev" in _err(lib)             # zero records
    assert lib.srgan_ema_multi_dev(b, 1, 0, b, None) == -1 and "ema_multi_dev" in _err(lib)             # zero chunks
    for decay in (1.0, 1.5, -0.1, float("nan")):
        assert lib.srgan_ema_state_init(b, decay, 1, 0, None) == -1 and "ema_state_init" in _err(lib), decay
        assert lib.srgan_ema_state_set_decay(b, decay, None) == -1 and "ema_state_set_decay" in _err(lib), decay
    assert lib.srgan_ema_state_init(b, 0.999, 1, -1, None) == -1 and "ema_state_init" in _err(lib)      # negative n_done
    assert lib.srgan_ema_state_init(None, 0.999, 1, 0, None) == -1 and "ema_state_init" in _err(lib)
    assert lib.srgan_ema_state_set_decay(None, 0.5, None) == -1 and "ema_state_set_decay" in _err(lib)
    assert all(c == b"\x00" for c in buf)                                                             # nothing was touched


def _layout(net):
    return [[k, list(v.shape)] for k, v in net.state_dict().items()]


def test_copy_has_the_reference_layout(golden_dir):
    from srgan_amd import ema, model
    ref = json.load(open(os.path.join(golden_dir, "shapes.json")))["T"]
    G = model.SingleGenerator(3, 4, 2, 2, 1, "instance", num_con=12)
    E = model.Encoder(3, 8, 4, 4, "instance", 4, "cpu")
    for live, name in ((G, "G"), (E, "E")):
        live.train()
        twin = ema.make_copy(live)
        assert type(twin) is type(live) and twin is not live
        assert _layout(twin) == ref[name] == _layout(live)
        assert all(v.dtype == live.state_dict()[k].dtype for k, v in twin.state_dict().items())
        assert not twin.training and live.training
        assert not any(p.requires_grad for p in twin.parameters()) and all(p.requires_grad for p in live.parameters())
        for (k, v), w in zip(twin.state_dict().items(), live.state_dict().values()):
            assert torch.equal(v, w) and v.data_ptr() != w.data_ptr(), k
    # the pretrained-encoder recipe leaves parameters frozen on the live side; the copy still holds all of them
    E.freeze_melt([k for k in E.state_dict() if not k.startswith(("fcmean", "fcvar"))], "freeze")
    assert _layout(ema.make_copy(E)) == ref["E"]


def test_copy_of_batch_norm_networks_has_the_buffers():
    from srgan_amd import ema, model
    G = model.SingleGenerator(3, 4, 2, 2, 1, "batch", num_con=12)
    E = model.Encoder(3, 8, 4, 4, "batch", 4, "cpu")
    for live in (G, E):
        twin = ema.make_copy(live)
        assert type(twin) is type(live)
        keys = list(twin.state_dict())
        assert keys == list(live.state_dict())
        assert [(k, v.shape, v.dtype) for k, v in twin.state_dict().items()] == [(k, v.shape, v.dtype) for k, v in live.state_dict().items()]
        for suffix, dtype in (("running_mean", torch.float32), ("running_var", torch.float32), ("num_batches_tracked", torch.int64)):
            hits = [k for k in keys if k.endswith(suffix)]
            assert hits and all(twin.state_dict()[k].dtype == dtype for k in hits), suffix
        assert not any(m.training for m in twin.modules())


@pytest.mark.parametrize("ramp", [True, False])
@pytest.mark.parametrize("decay", [0.999, 0.9999, 0.5, 0.0])
def test_host_decay_schedule_equals_the_restatement(decay, ramp):
    from srgan_amd import ema
    for n in range(1, 2001):
        got, want = ema.decay_at(n, decay, ramp), decay_ref(n, decay, ramp)
        assert got.dtype == np.float32 and got == want, (n, got, want)


def test_table_layout(lib):
    """five 64-bit words per record; the fifth is the prefix sum of ceil(numel / chunk)"""
    import struct
    from srgan_amd import ema, ops
    seen = {}
    orig = ops.upload_small
    ops.upload_small = lambda blob, device, out=None: seen.setdefault("blob", bytes(blob))
    try:
        _, n, total = ema.build_table([(16, 32, 1, 0), (64, 128, 4096, 0), (256, 512, 4097, 1), (1024, 2048, 2, 1)], "cpu")
    finally:
        ops.upload_small = orig
    assert (n, total) == (4, 1 + 1 + 2 + 1)
    assert struct.unpack("20q", seen["blob"]) == (16, 32, 1, 0, 0, 64, 128, 4096, 0, 1, 256, 512, 4097, 1, 2, 1024, 2048, 2, 1, 4)
