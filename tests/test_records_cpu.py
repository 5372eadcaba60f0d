"""CPU: the layouts of the seven device records.  csrc/records.h declares each struct once and srgan_amd/_lib.py mirrors it as a
ctypes.Structure; here the two meet: the sizes against the library's ``srgan_*_state_bytes()``, every field offset against a literal
(the one place that fails loudly when a layout moves), and the word masks of the write entries through a stand-alone host program
over the header (tests/records_host_check.cpp)."""
import ctypes
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# name -> (the library's size entry, bytes, {field: byte offset})
LAYOUTS = {
    "AdamState": ("srgan_adam_state_bytes", 32,
                  dict(step=0, lr=4, beta1=8, beta2=12, eps=16, step_size=20, inv_sqrt_bc2=24, _pad=28)),
    "GuardState": ("srgan_grad_guard_state_bytes", 32,
                   dict(max_norm=0, norm=4, scale=8, skip=12, steps=16, skipped=20, clipped=24, _pad=28)),
    "EmaState": ("srgan_ema_state_bytes", 16, dict(n=0, ramp=4, decay=8, c=12)),
    "AdaState": ("srgan_ada_state_bytes", 56,
                 dict(p=0, target=4, step=8, p_max=12, interval=16, seen=20, n_pos=24, n_neg=32, n_total=40, adjustments=48, last_r=52)),
    "R1State": ("srgan_r1_state_bytes", 32, dict(gamma=0, every=4, c=8, penalty=12, mean_sq_norm=16, updates=20, n=24, _pad=28)),
    "CrState": ("srgan_cr_state_bytes", 32, dict(lambda_real=0, lambda_fake=4, every=8, cr_real=12, cr_fake=16, updates=20, _pad=24)),
    "MsState": ("srgan_ms_state_bytes", 32, dict(weight=0, eps=4, tau=8, ms=12, weighted=16, d_image=20, d_latent=24, updates=28)),
}


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_structure_matches_the_library_and_the_literal_offsets(name):
    from srgan_amd import _lib
    entry, size, offsets = LAYOUTS[name]
    layout = getattr(_lib, name)
    assert issubclass(layout, ctypes.Structure)
    assert ctypes.sizeof(layout) == size == getattr(_lib.load(), entry)()
    assert [f for f, _ in layout._fields_] == list(offsets)                      # the order too: the read dicts keep it
    assert {f: getattr(layout, f).offset for f in offsets} == offsets
    widths = {f: getattr(layout, f).size for f in offsets}
    wide = {"n_pos", "n_neg", "n_total"} if name == "AdaState" else {"_pad"} if name == "CrState" else set()
    assert widths == {f: 8 if f in wide else 4 for f in offsets}


def test_the_write_masks_of_the_header_by_a_host_program(tmp_path):
    """records_host_check.cpp static_asserts every entry's mask against a literal and replays the kernel's store rule"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = os.path.join(str(tmp_path), "records_host_check")
    inc = os.path.join(os.path.dirname(HERE), "style-restricted_gan_amd", "csrc")
    built = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I" + inc, os.path.join(HERE, "records_host_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "records ok", (r.stdout, r.stderr[-2000:])
