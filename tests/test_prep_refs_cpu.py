"""CPU: the yardsticks of tests/prep_common.py.  The resize tables the HIP kernels consume (srgan_amd.data.pil_bilinear_tables),
driven through the numpy restatement of Pillow's two-pass resample, reproduce Pillow byte for byte on every geometry and image
of tests/test_prep_kernels_gpu.py; the geometries reach the launch-plan branches they are there for."""
import os
import re

import numpy as np
import pytest

from oracle import preprocess as opre
from srgan_amd import data as hdata
from tests import prep_common as pc

PIL = pytest.importorskip("PIL.Image")
HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "style-restricted_gan_amd", "csrc", "preprocess.hip")


@pytest.mark.parametrize("g", pc.GEOMETRIES, ids=lambda g: g["name"])
def test_tables_reproduce_pillow_on_every_geometry(g):
    (ch, cw), (oh, ow) = g["crop"], g["size"]
    x = pc.images(min(g["b"], 7), g["h"], g["w"])
    top, left = hdata.center_crop_box(g["h"], g["w"], ch, cw)
    assert (top, left) == opre.center_crop_box(g["h"], g["w"], ch, cw)
    bh, kh, ksh = hdata.pil_bilinear_tables(cw, ow)
    bv, kv, ksv = hdata.pil_bilinear_tables(ch, oh)
    assert kh.shape == (ow, ksh) and kv.shape == (oh, ksv)
    assert (bh[:, 0] >= 0).all() and (bh[:, 0] + bh[:, 1] <= cw).all() and (bh[:, 1] <= ksh).all()      # the windows the kernels read
    assert (bv[:, 0] >= 0).all() and (bv[:, 0] + bv[:, 1] <= ch).all() and (bv[:, 1] <= ksv).all()
    for i in range(len(x)):
        crop = np.ascontiguousarray(x[i, top:top + ch, left:left + cw])
        want = np.asarray(PIL.fromarray(crop, "RGB").resize((ow, oh), PIL.BILINEAR))
        assert np.array_equal(opre.resize_restated(crop, bh, kh, bv, kv), want), (g["name"], i)
        ref = opre.transform_pil(x[i], 0, g["crop"], g["size"], False, False)                       # the crop is Pillow's too
        assert np.array_equal(ref, opre.to_tensor(want))


def test_geometries_reach_their_branches():
    src = open(HIP).read()
    assert re.search(r"ceil_div\(nh, 256\), (\d+)\)", src).group(1) == str(pc.H_CAP)
    assert re.search(r"ceil_div\(out_h \* out_w, 256\), (\d+)\)", src).group(1) == str(pc.V_CAP)
    assert re.search(r"ceil_div\(nt, 256\), (\d+)\)", src).group(1) == str(pc.N_CAP)
    g = {x["name"]: x for x in pc.GEOMETRIES}
    p = {name: pc.plan(x) for name, x in g.items()}
    assert p["178-129x128"]["v_trips"] == 2 and p["178-256"]["v_trips"] == 4
    assert p["178-128-b96"]["h_trips"] == 2 and p["178-128-b96"]["n_trips"] == 3
    assert p["48x64-31x37"]["v_idle"] % 64 != 0 and p["48x64-31x37"]["v_idle"] > 0                   # a wave partly idle in the reduction
    assert all(q["h_trips"] == q["n_trips"] == 1 for n, q in p.items() if n != "178-128-b96")
    assert hdata.pil_bilinear_tables(178, 256)[2] == 3 and hdata.pil_bilinear_tables(178, 16)[2] == 25
    assert hdata.center_crop_box(219, 181, 178, 178) == (20, 2)
    assert g["178-128-b1"]["b"] == 1 and (219 - 178) % 2 == 1 and (181 - 178) % 2 == 1


def test_images_and_flags():
    x = pc.images(15, 64, 80)
    assert x.dtype == np.uint8 and x.shape == (15, 64, 80, 3)
    assert (x[4] == 0).all() and (x[5] == 255).all() and (x[6] == 77).all() and set(np.unique(x[2])) == {0, 255}
    assert np.array_equal(x[9], 255 - x[2])                                   # the second checkerboard is the other phase
    assert (x[3] != 10).any(axis=2).sum() == 1 and (x[10] != 10).any(axis=2).sum() == 1 and not np.array_equal(x[3], x[10])
    assert len(np.unique(x[0])) == 256 and len(np.unique(x[1][:, :, 0])) == 64
    assert pc.flip_flags("null", 5) is None and pc.flip_flags("on", 5).all() and not pc.flip_flags("off", 5).any()
    assert pc.flip_flags("mixed", 5).tolist() == [1, 0, 1, 1, 0] and pc.flip_flags("mixed", 1).tolist() == [1]


def test_reference_is_pillow_with_the_flip_applied():
    g = pc.GEOMETRIES[3]
    x = pc.images(2, g["h"], g["w"])
    plain = pc.reference(x, None, g, True, True)
    assert plain.shape == (2, 31, 37, 3) and plain.dtype == np.float32
    assert np.array_equal(pc.reference(x, np.asarray([1, 0], np.uint8), g, True, True)[0], plain[0, :, ::-1])
    assert np.array_equal(pc.reference(x, np.asarray([0, 0], np.uint8), g, True, True), plain)
    assert plain.min() == -1.0 and abs(plain.max() - 1.0) < 1e-6
    raw = pc.reference(x, None, g, False, True)                                # without MinMax mean0 changes nothing
    assert np.array_equal(raw, pc.reference(x, None, g, False, False)) and raw.min() >= 0 and raw.max() <= 1
