"""GPU: the input-pipeline kernels (csrc/preprocess.hip) against Pillow itself (oracle.preprocess.transform_pil), bit for bit,
through the C ABI on guarded memory: the output and the workspace -- which has exactly the bytes srgan_preprocess_workspace
returns -- lie between two regions of pattern bytes that must be intact after every call.  Geometries, images and modes live
in tests/prep_common.py (pinned without a GPU by tests/test_prep_refs_cpu.py): every grid-stride loop runs more than once, a
wave of the min / max reduction is partly idle, MinMax off, mean0 off and the NULL flip pointer are run."""
import ctypes

import numpy as np
import pytest
import torch

from tests import prep_common as pc
from tests.eval_common import Arena

pytestmark = pytest.mark.gpu
pytest.importorskip("PIL.Image")


@pytest.fixture(scope="module")
def ops():
    from srgan_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(scope="module")
def lib():
    from srgan_amd import _lib
    return _lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Pipeline:
    """One geometry's device state: tables, the exact workspace and the output, all guarded; ``run`` may be called repeatedly."""

    def __init__(self, ops, lib, g):
        from srgan_amd import data as hdata
        self.ops, self.lib, self.g, self.ar = ops, lib, g, Arena()
        (ch, cw), (oh, ow), b = g["crop"], g["size"], g["b"]
        self.top, self.left = hdata.center_crop_box(g["h"], g["w"], ch, cw)
        bh, kh, self.ksh = hdata.pil_bilinear_tables(cw, ow)
        bv, kv, self.ksv = hdata.pil_bilinear_tables(ch, oh)
        self.tables = [self.ar.put(a, what) for a, what in ((bh, "h_bounds"), (kh, "h_coeffs"), (bv, "v_bounds"), (kv, "v_coeffs"))]
        self.nbytes = lib.load().srgan_preprocess_workspace(b, ch, oh, ow)
        assert self.nbytes >= b * ch * ow * 3 + b * oh * ow * 3 + b * 8
        self.ws = self.ar.raw(self.nbytes, "workspace")
        self.src = self.ar.raw(b * g["h"] * g["w"] * 3, "src").view(b, g["h"], g["w"], 3)
        self.flip = self.ar.raw(b, "flip")
        self.dst = self.ar.out((b, oh, ow, 3), "dst")

    def run(self, x, flips, minmax, mean0):
        g = self.g
        (ch, cw), (oh, ow) = g["crop"], g["size"]
        self.src.copy_(torch.from_numpy(x))
        if flips is not None:
            self.flip.copy_(torch.from_numpy(flips))
        self.dst.view(torch.uint8).fill_(0xA5)
        hb, hc, vb, vc = self.tables
        code = self.lib.load().srgan_preprocess_u8(_p(self.src), g["b"], g["h"], g["w"], self.top, self.left, ch, cw, oh, ow, _p(hb), _p(hc),
                                                   self.ksh, _p(vb), _p(vc), self.ksv, _p(self.flip) if flips is not None else None,
                                                   int(minmax), int(mean0), _p(self.dst), _p(self.ws), self.nbytes, self.ops._stream())
        self.lib.check(code, "preprocess_u8")
        torch.cuda.synchronize()
        self.ar.intact(f"preprocess_u8 {g['name']}")
        return self.dst.cpu().numpy()


def hold(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ from Pillow, first at {bad[0].tolist()}: "
                             f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


@pytest.mark.parametrize("minmax,mean0", pc.MODES)
@pytest.mark.parametrize("g", pc.GEOMETRIES, ids=lambda g: g["name"])
def test_preprocess_is_pillow_bit_for_bit(ops, lib, g, minmax, mean0):
    """Flips all on, all off, mixed and the NULL pointer, one after the other on the same workspace."""
    pipe = Pipeline(ops, lib, g)
    x = pc.images(g["b"], g["h"], g["w"])
    for kind in pc.FLIPS:
        flips = pc.flip_flags(kind, g["b"])
        hold(pipe.run(x, flips, minmax, mean0), pc.reference(x, flips, g, minmax, mean0), f"{g['name']} flips {kind}")


@pytest.mark.parametrize("g", [pc.GEOMETRIES[0], pc.GEOMETRIES[3]], ids=lambda g: g["name"])
def test_second_call_on_the_same_workspace_sees_its_own_min_max(ops, lib, g):
    """A bright batch, then a dimmer one (bytes 40 .. 82 instead of 0 .. 255) on the same workspace, then the bright one
    again: a min / max left over from the call before would show in either direction."""
    pipe = Pipeline(ops, lib, g)
    x = pc.images(g["b"], g["h"], g["w"])
    dim = (x // 6 + 40).astype(np.uint8)
    flips = pc.flip_flags("mixed", g["b"])
    for batch, what in ((x, "bright"), (dim, "dimmer"), (x, "bright again")):
        hold(pipe.run(batch, flips, True, True), pc.reference(batch, flips, g, True, True), f"{g['name']} {what}")


def test_workspace_too_small_is_an_error(ops, lib):
    pipe = Pipeline(ops, lib, pc.GEOMETRIES[3])
    pipe.nbytes -= 1
    with pytest.raises(lib.SrganHipError, match="workspace too small"):
        pipe.run(pc.images(7, 64, 80), None, True, True)
