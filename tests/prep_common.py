"""Yardsticks of the input-pipeline tests (csrc/preprocess.hip): geometries, images and modes.  The reference is
oracle.preprocess.transform_pil -- Pillow itself -- and every result has to match it bit for bit.  tests/test_prep_refs_cpu.py
pins the resize tables of every geometry against Pillow without a GPU, tests/test_prep_kernels_gpu.py holds the kernels to it
through the C ABI.

The launch plan of srgan_preprocess_u8, restated (``plan``): the horizontal and the normalise pass run min(ceil(items / 256),
8192) workgroups and stride over the rest; the vertical pass runs min(ceil(out_h * out_w / 256), 64) workgroups per image."""
import numpy as np

from oracle import preprocess as opre

H_CAP, V_CAP, N_CAP, LANES = 8192, 64, 8192, 256


def _g(name, h, w, crop, size, b, why):
    return dict(name=name, h=h, w=w, crop=crop, size=size, b=b, why=why)


GEOMETRIES = [
    _g("178-129x128", 218, 178, (178, 178), (129, 128), 7, "first shape past the vertical pass's 16384 threads"),
    _g("178-256", 218, 178, (178, 178), (256, 256), 7, "the benchmarked resolution; upscale, window size 3"),
    _g("178-16", 218, 178, (178, 178), (16, 16), 7, "window size 25"),
    _g("48x64-31x37", 64, 80, (48, 64), (31, 37), 7, "out_h * out_w no multiple of 256 or 64"),
    _g("178-128-b96", 218, 178, (178, 178), (128, 128), 96, "past both 8192-workgroup caps"),
    _g("178-128-b1", 218, 178, (178, 178), (128, 128), 1, "smallest batch"),
    _g("odd-offsets", 219, 181, (178, 178), (128, 128), 7, "crop offsets 20.5 and 1.5: rounded half to even"),
]
MODES = [(True, True), (True, False), (False, True), (False, False)]          # (minmax, mean0)
FLIPS = ("on", "off", "mixed", "null")


def plan(g):
    """(horizontal trips, vertical trips, idle vertical lanes, normalise trips) of the grid-stride loops."""
    b, (ch, cw), (oh, ow) = g["b"], g["crop"], g["size"]
    cdiv = lambda a, q: -(-a // q)                                          # noqa: E731
    nh, per, nt = b * ch * ow, oh * ow, b * oh * ow * 3
    vg = min(cdiv(per, LANES), V_CAP)
    return dict(h_trips=cdiv(nh, min(cdiv(nh, LANES), H_CAP) * LANES), v_trips=cdiv(per, vg * LANES),
                v_idle=vg * LANES * cdiv(per, vg * LANES) - per, n_trips=cdiv(nt, min(cdiv(nt, LANES), N_CAP) * LANES))


def images(b, h, w, seed=0):
    """uint8 [b, h, w, 3]; image i is of kind i % 7: random, smooth, 0/255 checkerboard, one differing pixel, all 0, all 255,
    constant 77 (max == min: the 1e-8 guard of MinMax)."""
    rng = np.random.default_rng([seed, b, h, w])
    x = rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([(yy * 255 // max(h - 1, 1)), (xx * 255 // max(w - 1, 1)), ((yy + xx) % 256)], -1).astype(np.uint8)
    checker = np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    for i in range(b):
        kind = i % 7
        if kind == 1:
            x[i] = smooth
        elif kind == 2:
            x[i] = checker if (i // 7) % 2 == 0 else 255 - checker
        elif kind == 3:
            x[i] = 10
            x[i, h // 2 - (i // 7) % 5, w // 2 + (i // 7) % 3, :] = (255, 200, 11)
        elif kind == 4:
            x[i] = 0
        elif kind == 5:
            x[i] = 255
        elif kind == 6:
            x[i] = 77
    return x


def flip_flags(kind, b):
    """uint8 [b], or None for the NULL pointer of the C ABI (no image flipped)."""
    if kind == "null":
        return None
    if kind == "mixed":
        return (np.arange(b) % 3 != 1).astype(np.uint8)
    return np.full(b, 1 if kind == "on" else 0, np.uint8)


def reference(x, flips, g, minmax, mean0):
    """float32 [b, out_h, out_w, 3] (the kernels' NHWC) through Pillow, image by image."""
    out = [opre.transform_pil(x[i], 0 if flips is None else int(flips[i]), g["crop"], g["size"], minmax, mean0) for i in range(len(x))]
    return np.ascontiguousarray(np.stack(out).transpose(0, 2, 3, 1))
