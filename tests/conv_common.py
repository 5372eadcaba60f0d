"""Yardsticks of the convolution tests (csrc/conv_*.hip): the case tables of tests/test_ops_gpu.py and
tests/test_conv_kernels_gpu.py, what every hand-picked case is there to launch (CLAIMS / KERNEL_CASES), which entry points of
the C ABI each GPU test drives (COVERAGE), the instantiations nothing can launch (DEAD), the float64 reference and the error
measure.  No GPU code: tests/test_conv_refs_cpu.py pins what is in here against the launches the library really makes (logged by
tests/hip_shim/launch_shim.c through tests/hip_shim/drive_conv.py); the GPU tests hold the HIP kernels to the reference.

A kernel is written as the shim logs it: its name and the values of its template arguments, `igemm_kernel<256,128,4,2,true,false>`
= igemm_kernel<BM, BN, WM, WN, VEC, BF16>; wgrad_kernel<BMc, BNn, WM, WN, VEC, ROWS, BF16, IO16>.  Compute mode m0 = fp32, m1 =
bf16; dispatch `default`, or `forced` = SRGAN_WINOGRAD_THRESHOLD_SCALE=0 (the size thresholds of the Winograd / patch kernels
switched off).  The kernel a case CLAIMS for a direction is the last launch of that entry that is not one of HELPERS.

Error measure (`close` of test_ops_gpu.py): max |got - ref64| <= 1e-6 + bound * max |ref64|, with
  bound = max(2e-5, 8 * e32) for y and dx, max(5e-5, 8 * e32) for dw and db (the project's own fp32 tolerances),
  e32   = the error, by the same measure, of float32 CPU F.conv2d against float64 on the same operands (the margin 8 is the one
          of small_common.check; it matters only for long weight-gradient sums),
  + half a bf16 ulp of max |ref| where the result is stored as bf16 (bf16_store, as norm_common.bf16_store: 2^-9 .. 2^-8)."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))

# The hand-picked cases of test_conv2d_fwd_bwd.  The comment of a case says what it was written for; CLAIMS (below) holds, per
# (compute mode, dispatch, direction), the kernel it launches, and tests/test_conv_refs_cpu.py checks that.
CONV_CASES = [
    # N, I, H, W, O, k, s, p, reflect, bias
    (2, 3, 20, 20, 8, 7, 1, 3, False, False),     # G first layer shape class (Cin=3)
    (2, 64, 16, 16, 128, 4, 2, 1, False, False),  # k4 s2 down conv (vector path)
    (2, 32, 12, 12, 64, 3, 1, 1, False, False),   # 3x3 residual conv class
    (1, 256, 8, 8, 256, 3, 1, 1, False, False),   # exact G res conv channels
    (2, 64, 14, 14, 3, 7, 1, 3, False, False),    # G last layer (Cout=3)
    (2, 3, 32, 32, 64, 4, 2, 1, False, False),    # D first layer
    (3, 128, 8, 8, 1, 4, 1, 1, False, True),      # D last_layer (Cout=1, bias)
    (3, 64, 8, 8, 4, 8, 1, 0, False, True),       # D classification head (valid 8x8)
    (2, 3, 33, 33, 16, 7, 2, 1, False, True),     # E first layer (k7 s2 p1, odd sizes)
    (2, 32, 9, 9, 64, 3, 1, 1, True, False),      # E reflect conv (vector path)
    (2, 4, 7, 7, 8, 3, 1, 1, True, False),        # reflect, generic-channel path
    (2, 8, 3, 3, 16, 3, 1, 1, True, False),       # reflect on a 3x3 map (both mirrors hit row 1)
    (2, 32, 6, 6, 64, 1, 1, 0, False, True),      # 1x1 shortcut with bias
    (1, 16, 10, 10, 32, 4, 2, 1, False, False),   # generic channels, stride 2
    (2, 160, 6, 6, 96, 3, 1, 1, False, False),    # non power-of-two channels (vector path, N mask)
    (2, 64, 64, 64, 3, 7, 1, 3, False, False),    # G RGB head, exact tiles: rgbout_conv_kernel (took the layer over from the narrow-output direct kernels), rgb_wgrad_kernel<1>
    (2, 32, 67, 45, 1, 4, 1, 1, False, True),     # narrow-output, ragged tiles, Cout=1 + bias
    (3, 16, 40, 72, 4, 3, 1, 1, False, True),     # narrow-output, Cout=4, one channel chunk
    (4, 128, 48, 48, 256, 3, 1, 1, False, False), # F(4x4,3x3) forward (wino43_kernel) by default dispatch, input gradient on 64x64 GEMM tiles, wino_wgrad_kernel<0>
    (8, 64, 64, 64, 64, 4, 2, 1, False, False),   # 128x64 tiles, many M tiles
    (4, 64, 32, 32, 128, 3, 1, 1, False, False),  # row-aligned weight-gradient path (Wo % 32 == 0), zero pad: wgrad_kernel<128,64,...,ROWS> in the bf16 mode (fp32: wino_wgrad_kernel<0>)
    (2, 32, 32, 64, 64, 3, 1, 1, True, False),    # Wo % 32 == 0 with reflect padding; I = 32 gives 32-column tiles, which have no row-aligned instantiation: wgrad_kernel<64,32,2,1,true,false>
    (2, 128, 64, 64, 128, 4, 2, 1, False, False), # row-aligned path, stride 2, 128x128 tiles, several splits
    (32, 256, 16, 16, 256, 3, 1, 1, False, False),# F(4x4,3x3) both directions by default dispatch (bf16 mode: igemm16_kernel<128>); the 8-wave 256-row GEMM tiles are KERNEL_CASES'
    (3, 48, 7, 11, 40, 3, 1, 1, False, True),     # generic 128x64 GEMM (Cin % 32 != 0) by default; forced: F(2x2,3x3) forward only (wino_kernel<0>): odd sizes, ragged tile / channel blocks, bias
    (2, 48, 5, 4, 72, 3, 1, 1, True, True),       # forced: F(2x2,3x3) forward only (wino_kernel<0>): reflect padding, bias, 2 output-channel blocks
    (5, 64, 32, 32, 64, 3, 1, 1, False, False),   # forced: F(4x4,3x3) (wino43_kernel): tiles not a multiple of 64 per image boundary
    (8, 64, 18, 14, 128, 3, 1, 1, False, True),   # Winograd weight gradient: 63 tile positions (ragged last group), bias
    (4, 128, 17, 9, 128, 3, 1, 1, True, False),   # Winograd weight gradient: odd sizes (half tiles), reflect padding
    (16, 256, 16, 16, 128, 3, 1, 1, False, False),# Winograd weight gradient: several groups per split
    (8, 128, 40, 44, 128, 4, 2, 1, False, True),  # forced: F(3x3,2x2) Winograd of a 4x4 stride-2 layer (wino_kernel<1> / <2>): fwd and input gradient, ragged 3x3 tiles
    (48, 128, 58, 62, 128, 4, 2, 1, False, True), # same + its Winograd weight gradient (needs >= 192 workgroups, >= 48 chunks), ragged tiles
    (32, 64, 32, 32, 64, 4, 2, 1, False, False),  # forced: F(4x4,2x2) both directions (wino42_kernel<1> / <2>) and wino_wgrad_kernel<1>: one cout tile, many images per tile-position group
    (64, 64, 64, 64, 128, 4, 2, 1, False, False), # D trunk at batch 64: Winograd weight gradient split over groups AND images (16 x 2)
    (50, 128, 32, 32, 256, 4, 2, 1, False, False),# same: 5 groups x 8 batch ranges, ragged last range (50 = 7 x 7 + 1)
    (2, 3, 24, 70, 64, 7, 1, 3, False, False),    # RGB 7x7 layer: input gradient as a narrow-output convolution of dy (flipped filter) on the 7x1 row convolution (128x32 GEMM tiles) + shift-add
    (2, 3, 12, 13, 32, 5, 1, 2, False, True),     # same route, generic narrow kernel (5x5), bias
    (2, 64, 20, 72, 3, 7, 1, 3, False, True),     # RGB head through the 7x1 row convolution + shift-add, bias, ragged rows
    (32, 64, 32, 32, 128, 3, 1, 1, False, True),  # F(4x4,3x3) Winograd by default dispatch (128 workgroups), bias
    (3, 64, 8, 12, 96, 3, 1, 1, False, True),     # F(4x4,3x3) when forced: 18 tiles (ragged block), 8 chunks, 3 channel blocks
    (2, 3, 40, 33, 128, 7, 1, 3, False, True),    # RGB-input 7x7 layer on the MFMA (LDS halo): ragged tiles, 2 channel blocks, bias
    (9, 3, 128, 128, 64, 7, 1, 3, False, False),  # RGB-input layer: MFMA weight gradient, 288 pixel tiles on 256 persistent workgroups
    (3, 64, 32, 64, 3, 7, 1, 3, False, False),    # RGB-output layer: MFMA weight gradient (swapped roles, flipped taps), 12 tiles
    (2, 3, 32, 40, 64, 7, 2, 1, False, True),     # E first layer at even sizes: input gradient as four stride-1 phase convs (3 / 4 taps)
    (3, 3, 33, 31, 32, 7, 2, 1, False, False),    # same, odd sizes (phase images of different heights / widths)
    (2, 4, 18, 22, 48, 6, 2, 2, False, False),    # same route: 4 input channels, 6x6 taps, pad 2
    (2, 3, 16, 16, 16, 5, 2, 0, False, False),    # same route: odd kernel, no padding
    (2, 256, 32, 32, 256, 3, 1, 1, False, False), # residual-trunk layer at full width (bf16 mode: LDS-resident patch kernel, C = 256)
    (1, 128, 8, 64, 128, 3, 1, 1, False, True),   # same kernel family: C = 128, two patches per row, bias
    (1, 256, 64, 64, 256, 3, 1, 1, False, False), # the 256x256 configuration's trunk map (64 x 64): 32 patches of one image
    (2, 64, 16, 64, 128, 4, 2, 1, False, False),  # 64 -> 128 down conv on an 8 x 32 output map (bf16 mode: input gradient on the transposed patch kernel)
    (1, 128, 8, 64, 256, 4, 2, 1, False, False),  # 128 -> 256 down conv, one output patch (same kernel, C = 256 reduce channels)
    (3, 64, 64, 128, 128, 4, 2, 1, False, True),  # same layer class on a wider map: 8 x 2 patches per image, bias
    (2, 64, 40, 70, 3, 7, 1, 3, False, True),     # round 3: RGB head on the 4x4x1 MFMA (direct, LDS halo): ragged 32 x 64 tiles, bias
    (3, 3, 128, 128, 64, 7, 1, 3, False, False),  # RGB input layer at full size: its input gradient on the same kernel (flipped, transposed filter)
    (2, 32, 64, 96, 3, 7, 1, 3, False, False),    # same kernel, 32 reduce channels (8 channel quads), 2 column tiles
    (4, 64, 62, 62, 128, 3, 1, 1, True, False),   # the encoder's own shapes (round 3): E.layers.0.cmp, 62 x 62, reflect padding
    (4, 128, 31, 31, 128, 3, 1, 1, True, True),   # E.layers.1 on 31 x 31, reflect, bias
    (8, 64, 30, 22, 64, 3, 1, 1, False, True),    # even but not multiple-of-4 map, zero padding, bias
    (6, 32, 15, 15, 64, 3, 1, 1, True, False),    # E.layers.2 map size, reflect
    (2, 96, 13, 18, 32, 3, 1, 1, True, True),     # odd sizes in both directions, 3 channel groups, one cout block, bias
    (16, 64, 66, 66, 64, 3, 1, 1, True, False),   # bf16 mode: 545 pixel tiles of igemm16_kernel on <= 512 persistent workgroups (reflect, 64 couts)
    (9, 256, 64, 16, 64, 4, 2, 1, False, False),  # round 5: 256 input channels keep the strided 4x4 / stride-2 form OFF F(4x4,2x2) (1024 reduce terms: 2.07e-5 there); its input gradient (64 reduce channels) takes it
    (4, 128, 32, 48, 192, 4, 2, 1, False, True),  # round 5: F(4x4,2x2) both directions, 3 channel blocks forward, 24 tiles per image (ragged 32-tile blocks), bias
    (3, 3, 128, 128, 64, 4, 2, 1, False, False),  # round 6: D's first layer at full size on the LDS-halo MFMA kernel, stride 2 (rgbin_conv_kernel<4, 4, 3, 2>)
    (2, 3, 70, 90, 128, 4, 2, 1, False, True),    # same kernel: ragged 16 x 32 output tiles (35 x 45 map), two channel blocks, bias
    (3, 3, 128, 128, 64, 7, 2, 1, False, True),   # round 6: E's first layer at full size (7x7 / stride 2 / pad 1 -> 62 x 62), bias (rgbin_conv_kernel<7, 7, 3, 2>)
    (2, 3, 71, 77, 64, 7, 2, 1, False, False),    # same kernel, odd sizes (33 x 36 map)
    (40, 64, 16, 16, 64, 4, 2, 1, False, False),  # round 5: F(4x4,2x2) transposed form on 160 tiles x 4 phases = 20 items over persistent workgroups
]


# ---- what every hand-picked case launches: {case: {"<mode>/<dispatch>": (forward, input gradient, weight gradient)}} -- the main
# kernel (main_kernel) of srgan_conv2d_fwd / _dgrad / _wgrad in every (compute mode, dispatch) a GPU test runs the case in: fp32
# under both dispatch settings (test_conv2d_fwd_bwd), bf16 by default dispatch for BF16_MODE_CASES (test_conv2d_bf16_compute_mode).
# tests/test_conv_refs_cpu.py compares it with the launches the library makes: a threshold that moves a case fails there.
CLAIMS = {
    (2, 3, 20, 20, 8, 7, 1, 3, False, False): {
        "fp32/default": ("igemm_kernel<128,32,4,1,false,false>", "igemm_kernel<128,32,4,1,false,false>",
                         "wgrad_kernel<32,64,1,2,false,false,false,false>"),
        "fp32/forced": ("igemm_kernel<128,32,4,1,false,false>", "igemm_kernel<128,32,4,1,false,false>",
                         "wgrad_kernel<32,64,1,2,false,false,false,false>"),
    },
    (2, 64, 16, 16, 128, 4, 2, 1, False, False): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "igemm_kernel<128,64,2,2,true,false>",
                         "wgrad_kernel<128,64,2,2,true,false,false,false>"),
        "fp32/forced": ("wino42_kernel<1,false>", "wino42_kernel<2,false>", "wgrad_kernel<128,64,2,2,true,false,false,false>"),
        "bf16/default": ("igemm16_kernel<128,false,false,false>", "igemm16_kernel<64,false,false,false>",
                         "halo16s2_wgrad_kernel<8,false,false>"),
    },
    (2, 32, 12, 12, 64, 3, 1, 1, False, False): {
        "fp32/default": ("igemm_kernel<128,64,2,2,true,false>", "igemm_kernel<128,32,4,1,true,false>",
                         "wgrad_kernel<64,32,2,1,true,false,false,false>"),
        "fp32/forced": ("wino43_kernel<false>", "wino43_kernel<false>", "wgrad_kernel<64,32,2,1,true,false,false,false>"),
        "bf16/default": ("igemm_kernel<128,64,2,2,true,true>", "igemm_kernel<128,32,4,1,true,true>",
                         "wgrad_kernel<64,32,2,1,true,false,true,false>"),
    },
    (1, 256, 8, 8, 256, 3, 1, 1, False, False): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "igemm_kernel<64,64,2,2,true,false>",
                         "wgrad_kernel<128,128,2,2,true,false,false,false>"),
        "fp32/forced": ("wino43_kernel<false>", "wino43_kernel<false>", "wino_wgrad_kernel<0>"),
        "bf16/default": ("igemm16_kernel<128,false,false,false>", "igemm16_kernel<128,false,false,false>",
                         "wgrad_kernel<128,128,2,2,true,false,true,false>"),
    },
    (2, 64, 14, 14, 3, 7, 1, 3, False, False): {
        "fp32/default": ("narrow_conv_fwd_kernel<3>", "igemm_kernel<128,64,2,2,false,false>", "narrow_conv_wgrad_kernel<3,4>"),
        "fp32/forced": ("narrow_conv_fwd_kernel<3>", "igemm_kernel<128,64,2,2,false,false>", "narrow_conv_wgrad_kernel<3,4>"),
    },
    (2, 3, 32, 32, 64, 4, 2, 1, False, False): {
        "fp32/default": ("igemm_kernel<128,64,2,2,false,false>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<64,64,2,2,false,false,false,false>"),
        "fp32/forced": ("igemm_kernel<128,64,2,2,false,false>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<64,64,2,2,false,false,false,false>"),
    },
    (3, 128, 8, 8, 1, 4, 1, 1, False, True): {
        "fp32/default": ("narrow_wave_fwd_kernel<1>", "igemm_kernel<64,64,2,2,false,false>", "narrow_conv_wgrad_kernel<1,1>"),
        "fp32/forced": ("narrow_wave_fwd_kernel<1>", "igemm_kernel<64,64,2,2,false,false>", "narrow_conv_wgrad_kernel<1,1>"),
    },
    (3, 64, 8, 8, 4, 8, 1, 0, False, True): {
        "fp32/default": ("dense_head_kernel", "igemm_kernel<128,64,2,2,false,false>",
                         "wgrad_kernel<32,64,1,2,true,false,false,false>"),
        "fp32/forced": ("dense_head_kernel", "igemm_kernel<128,64,2,2,false,false>",
                         "wgrad_kernel<32,64,1,2,true,false,false,false>"),
    },
    (2, 3, 33, 33, 16, 7, 2, 1, False, True): {
        "fp32/default": ("igemm_kernel<128,32,4,1,false,false>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<32,64,1,2,false,false,false,false>"),
        "fp32/forced": ("igemm_kernel<128,32,4,1,false,false>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<32,64,1,2,false,false,false,false>"),
    },
    (2, 32, 9, 9, 64, 3, 1, 1, True, False): {
        "fp32/default": ("igemm_kernel<128,64,2,2,true,false>", "igemm_kernel<128,32,4,1,true,false>",
                         "wgrad_kernel<64,32,2,1,true,false,false,false>"),
        "fp32/forced": ("wino_kernel<0,false>", "wino_kernel<0,false>", "wgrad_kernel<64,32,2,1,true,false,false,false>"),
        "bf16/default": ("igemm_kernel<128,64,2,2,true,true>", "igemm_kernel<128,32,4,1,true,true>",
                         "wgrad_kernel<64,32,2,1,true,false,true,false>"),
    },
    (2, 4, 7, 7, 8, 3, 1, 1, True, False): {
        "fp32/default": ("igemm_kernel<128,32,4,1,false,false>", "igemm_kernel<128,32,4,1,false,false>",
                         "wgrad_kernel<32,64,1,2,false,false,false,false>"),
        "fp32/forced": ("igemm_kernel<128,32,4,1,false,false>", "igemm_kernel<128,32,4,1,false,false>",
                         "wgrad_kernel<32,64,1,2,false,false,false,false>"),
    },
    (2, 8, 3, 3, 16, 3, 1, 1, True, False): {
        "fp32/default": ("igemm_kernel<128,32,4,1,false,false>", "igemm_kernel<128,32,4,1,false,false>",
                         "wgrad_kernel<32,64,1,2,false,false,false,false>"),
        "fp32/forced": ("igemm_kernel<128,32,4,1,false,false>", "igemm_kernel<128,32,4,1,false,false>",
                         "wgrad_kernel<32,64,1,2,false,false,false,false>"),
    },
    (2, 32, 6, 6, 64, 1, 1, 0, False, True): {
        "fp32/default": ("igemm_kernel<128,64,2,2,true,false>", "igemm_kernel<128,32,4,1,true,false>",
                         "wgrad_kernel<64,32,2,1,true,false,false,false>"),
        "fp32/forced": ("igemm_kernel<128,64,2,2,true,false>", "igemm_kernel<128,32,4,1,true,false>",
                         "wgrad_kernel<64,32,2,1,true,false,false,false>"),
        "bf16/default": ("igemm_kernel<128,64,2,2,true,true>", "igemm_kernel<128,32,4,1,true,true>",
                         "wgrad_kernel<64,32,2,1,true,false,true,false>"),
    },
    (1, 16, 10, 10, 32, 4, 2, 1, False, False): {
        "fp32/default": ("igemm_kernel<128,32,4,1,false,false>", "igemm_kernel<128,32,4,1,true,false>",
                         "wgrad_kernel<32,64,1,2,false,false,false,false>"),
        "fp32/forced": ("igemm_kernel<128,32,4,1,false,false>", "igemm_kernel<128,32,4,1,true,false>",
                         "wgrad_kernel<32,64,1,2,false,false,false,false>"),
    },
    (2, 160, 6, 6, 96, 3, 1, 1, False, False): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "igemm_kernel<64,64,2,2,true,false>",
                         "wgrad_kernel<128,32,4,1,true,false,false,false>"),
        "fp32/forced": ("wino_kernel<0,false>", "wino_kernel<0,false>", "wgrad_kernel<128,32,4,1,true,false,false,false>"),
        "bf16/default": ("igemm_kernel<64,64,2,2,true,true>", "igemm_kernel<64,64,2,2,true,true>",
                         "wgrad_kernel<128,32,4,1,true,false,true,false>"),
    },
    (2, 64, 64, 64, 3, 7, 1, 3, False, False): {
        "fp32/default": ("rgbout_conv_kernel", "rgbin_conv_kernel<7,7,3,1>", "rgb_wgrad_kernel<1>"),
        "fp32/forced": ("rgbout_conv_kernel", "rgbin_conv_kernel<7,7,3,1>", "rgb_wgrad_kernel<1>"),
    },
    (2, 32, 67, 45, 1, 4, 1, 1, False, True): {
        "fp32/default": ("narrow_conv_fwd_kernel<1>", "igemm_kernel<128,32,4,1,false,false>", "narrow_conv_wgrad_kernel<1,1>"),
        "fp32/forced": ("narrow_conv_fwd_kernel<1>", "igemm_kernel<128,32,4,1,false,false>", "narrow_conv_wgrad_kernel<1,1>"),
    },
    (3, 16, 40, 72, 4, 3, 1, 1, False, True): {
        "fp32/default": ("narrow_conv_fwd_kernel<4>", "igemm_kernel<128,32,4,1,false,false>", "narrow_conv_wgrad_kernel<4,1>"),
        "fp32/forced": ("narrow_conv_fwd_kernel<4>", "igemm_kernel<128,32,4,1,false,false>", "narrow_conv_wgrad_kernel<4,1>"),
    },
    (4, 128, 48, 48, 256, 3, 1, 1, False, False): {
        "fp32/default": ("wino43_kernel<false>", "igemm_kernel<64,64,2,2,true,false>", "wino_wgrad_kernel<0>"),
        "fp32/forced": ("wino43_kernel<false>", "wino43_kernel<false>", "wino_wgrad_kernel<0>"),
        "bf16/default": ("igemm16_kernel<128,false,false,false>", "igemm16_kernel<128,false,false,false>",
                         "wgrad_kernel<128,128,2,2,true,false,true,false>"),
    },
    (8, 64, 64, 64, 64, 4, 2, 1, False, False): {
        "fp32/default": ("igemm_kernel<128,64,2,2,true,false>", "igemm_kernel<128,64,2,2,true,false>",
                         "wgrad_kernel<64,64,2,2,true,true,false,false>"),
        "fp32/forced": ("wino42_kernel<1,false>", "wino42_kernel<2,false>", "wino_wgrad_kernel<1>"),
        "bf16/default": ("igemm16_kernel<64,false,false,false>", "igemm16_kernel<64,false,false,false>",
                         "halo16s2_wgrad_kernel<32,false,false>"),
    },
    (4, 64, 32, 32, 128, 3, 1, 1, False, False): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "igemm_kernel<128,64,2,2,true,false>", "wino_wgrad_kernel<0>"),
        "fp32/forced": ("wino43_kernel<false>", "wino43_kernel<false>", "wino_wgrad_kernel<0>"),
        "bf16/default": ("igemm16_kernel<128,false,false,false>", "igemm16_kernel<64,false,false,false>",
                         "wgrad_kernel<128,64,2,2,true,true,true,false>"),
    },
    (2, 32, 32, 64, 64, 3, 1, 1, True, False): {
        "fp32/default": ("igemm_kernel<128,64,2,2,true,false>", "igemm_kernel<128,32,4,1,true,false>",
                         "wgrad_kernel<64,32,2,1,true,false,false,false>"),
        "fp32/forced": ("wino_kernel<0,false>", "wino_kernel<0,false>", "wgrad_kernel<64,32,2,1,true,false,false,false>"),
        "bf16/default": ("igemm_kernel<128,64,2,2,true,true>", "igemm_kernel<128,32,4,1,true,true>",
                         "wgrad_kernel<64,32,2,1,true,false,true,false>"),
    },
    (2, 128, 64, 64, 128, 4, 2, 1, False, False): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "igemm_kernel<64,64,2,2,true,false>",
                         "wgrad_kernel<128,128,2,2,true,true,false,false>"),
        "fp32/forced": ("wino42_kernel<1,false>", "wino42_kernel<2,false>", "wino_wgrad_kernel<1>"),
        "bf16/default": ("igemm16_kernel<128,false,false,false>", "igemm16_kernel<128,false,false,false>",
                         "halo16s2_wgrad_kernel<32,false,false>"),
    },
    (32, 256, 16, 16, 256, 3, 1, 1, False, False): {
        "fp32/default": ("wino43_kernel<false>", "wino43_kernel<false>", "wino_wgrad_kernel<0>"),
        "fp32/forced": ("wino43_kernel<false>", "wino43_kernel<false>", "wino_wgrad_kernel<0>"),
        "bf16/default": ("igemm16_kernel<128,false,false,false>", "igemm16_kernel<128,false,false,false>",
                         "wgrad_kernel<128,128,2,2,true,false,true,false>"),
    },
    (3, 48, 7, 11, 40, 3, 1, 1, False, True): {
        "fp32/default": ("igemm_kernel<128,64,2,2,false,false>", "igemm_kernel<128,64,2,2,false,false>",
                         "wgrad_kernel<64,64,2,2,false,false,false,false>"),
        "fp32/forced": ("wino_kernel<0,false>", "igemm_kernel<128,64,2,2,false,false>",
                         "wgrad_kernel<64,64,2,2,false,false,false,false>"),
    },
    (2, 48, 5, 4, 72, 3, 1, 1, True, True): {
        "fp32/default": ("igemm_kernel<64,64,2,2,false,false>", "igemm_kernel<128,64,2,2,false,false>",
                         "wgrad_kernel<128,64,2,2,false,false,false,false>"),
        "fp32/forced": ("wino_kernel<0,false>", "igemm_kernel<128,64,2,2,false,false>",
                         "wgrad_kernel<128,64,2,2,false,false,false,false>"),
    },
    (5, 64, 32, 32, 64, 3, 1, 1, False, False): {
        "fp32/default": ("igemm_kernel<128,64,2,2,true,false>", "igemm_kernel<128,64,2,2,true,false>", "wino_wgrad_kernel<0>"),
        "fp32/forced": ("wino43_kernel<false>", "wino43_kernel<false>", "wino_wgrad_kernel<0>"),
        "bf16/default": ("halo16_kernel<64,64,false,false,false>", "halo16_kernel<64,64,false,false,false>",
                         "halo16_wgrad_kernel<false,false>"),
    },
    (8, 64, 18, 14, 128, 3, 1, 1, False, True): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "igemm_kernel<128,64,2,2,true,false>", "wino_wgrad_kernel<0>"),
        "fp32/forced": ("wino_kernel<0,false>", "wino_kernel<0,false>", "wino_wgrad_kernel<0>"),
        "bf16/default": ("igemm16_kernel<128,false,false,false>", "igemm16_kernel<64,false,false,false>",
                         "wgrad_kernel<128,64,2,2,true,false,true,false>"),
    },
    (4, 128, 17, 9, 128, 3, 1, 1, True, False): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "igemm_kernel<64,64,2,2,true,false>", "wino_wgrad_kernel<0>"),
        "fp32/forced": ("wino_kernel<0,false>", "wino_kernel<0,false>", "wino_wgrad_kernel<0>"),
        "bf16/default": ("igemm16_kernel<128,false,false,false>", "igemm16_kernel<128,false,false,false>",
                         "wgrad_kernel<128,128,2,2,true,false,true,false>"),
    },
    (16, 256, 16, 16, 128, 3, 1, 1, False, False): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "igemm_kernel<64,64,2,2,true,false>", "wino_wgrad_kernel<0>"),
        "fp32/forced": ("wino43_kernel<false>", "wino43_kernel<false>", "wino_wgrad_kernel<0>"),
        "bf16/default": ("igemm16_kernel<128,false,false,false>", "igemm16_kernel<128,false,false,false>",
                         "wgrad_kernel<128,128,2,2,true,false,true,false>"),
    },
    (8, 128, 40, 44, 128, 4, 2, 1, False, True): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "igemm_kernel<64,64,2,2,true,false>",
                         "wgrad_kernel<128,128,2,2,true,false,false,false>"),
        "fp32/forced": ("wino_kernel<1,false>", "wino_kernel<2,false>", "wino_wgrad_kernel<1>"),
        "bf16/default": ("igemm16_kernel<128,false,false,false>", "igemm16_kernel<128,false,false,false>",
                         "wgrad_kernel<128,128,2,2,true,false,true,false>"),
    },
    (48, 128, 58, 62, 128, 4, 2, 1, False, True): {
        "fp32/default": ("wino_kernel<1,false>", "wino_kernel<2,false>", "wino_wgrad_kernel<1>"),
        "fp32/forced": ("wino_kernel<1,false>", "wino_kernel<2,false>", "wino_wgrad_kernel<1>"),
    },
    (32, 64, 32, 32, 64, 4, 2, 1, False, False): {
        "fp32/default": ("igemm_kernel<128,64,2,2,true,false>", "igemm_kernel<128,64,2,2,true,false>",
                         "wgrad_kernel<64,64,2,2,true,false,false,false>"),
        "fp32/forced": ("wino42_kernel<1,false>", "wino42_kernel<2,false>", "wino_wgrad_kernel<1>"),
        "bf16/default": ("igemm16_kernel<64,false,false,false>", "igemm16_kernel<64,false,false,false>",
                         "halo16s2_wgrad_kernel<16,false,false>"),
    },
    (64, 64, 64, 64, 128, 4, 2, 1, False, False): {
        "fp32/default": ("wino42_kernel<1,false>", "wino42_kernel<2,false>", "wino_wgrad_kernel<1>"),
        "fp32/forced": ("wino42_kernel<1,false>", "wino42_kernel<2,false>", "wino_wgrad_kernel<1>"),
    },
    (50, 128, 32, 32, 256, 4, 2, 1, False, False): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "wino42_kernel<2,false>", "wino_wgrad_kernel<1>"),
        "fp32/forced": ("wino42_kernel<1,false>", "wino42_kernel<2,false>", "wino_wgrad_kernel<1>"),
        "bf16/default": ("igemm16_kernel<128,false,false,false>", "igemm16_kernel<128,false,false,false>",
                         "halo16s2_wgrad_kernel<16,false,false>"),
    },
    (2, 3, 24, 70, 64, 7, 1, 3, False, False): {
        "fp32/default": ("rgbin_conv_kernel<7,7,3,1>", "igemm_kernel<128,32,4,1,true,false>",
                         "wgrad_kernel<64,64,2,2,false,false,false,false>"),
        "fp32/forced": ("rgbin_conv_kernel<7,7,3,1>", "igemm_kernel<128,32,4,1,true,false>",
                         "wgrad_kernel<64,64,2,2,false,false,false,false>"),
    },
    (2, 3, 12, 13, 32, 5, 1, 2, False, True): {
        "fp32/default": ("igemm_kernel<128,32,4,1,false,false>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<32,64,1,2,false,false,false,false>"),
        "fp32/forced": ("igemm_kernel<128,32,4,1,false,false>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<32,64,1,2,false,false,false,false>"),
    },
    (2, 64, 20, 72, 3, 7, 1, 3, False, True): {
        "fp32/default": ("igemm_kernel<128,32,4,1,true,false>", "rgbin_conv_kernel<7,7,3,1>", "narrow_conv_wgrad_kernel<3,4>"),
        "fp32/forced": ("igemm_kernel<128,32,4,1,true,false>", "rgbin_conv_kernel<7,7,3,1>", "narrow_conv_wgrad_kernel<3,4>"),
    },
    (32, 64, 32, 32, 128, 3, 1, 1, False, True): {
        "fp32/default": ("wino43_kernel<false>", "wino43_kernel<false>", "wino_wgrad_kernel<0>"),
        "fp32/forced": ("wino43_kernel<false>", "wino43_kernel<false>", "wino_wgrad_kernel<0>"),
        "bf16/default": ("halo16e_kernel<64,2,2,false,false>", "igemm16_kernel<64,false,false,false>",
                         "wgrad_kernel<128,64,2,2,true,true,true,false>"),
    },
    (3, 64, 8, 12, 96, 3, 1, 1, False, True): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "igemm_kernel<128,64,2,2,true,false>",
                         "wgrad_kernel<128,64,2,2,true,false,false,false>"),
        "fp32/forced": ("wino43_kernel<false>", "wino43_kernel<false>", "wgrad_kernel<128,64,2,2,true,false,false,false>"),
        "bf16/default": ("igemm16_kernel<128,false,false,false>", "igemm_kernel<128,64,2,2,true,true>",
                         "wgrad_kernel<128,64,2,2,true,false,true,false>"),
    },
    (2, 3, 40, 33, 128, 7, 1, 3, False, True): {
        "fp32/default": ("rgbin_conv_kernel<7,7,3,1>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<128,64,2,2,false,false,false,false>"),
        "fp32/forced": ("rgbin_conv_kernel<7,7,3,1>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<128,64,2,2,false,false,false,false>"),
    },
    (9, 3, 128, 128, 64, 7, 1, 3, False, False): {
        "fp32/default": ("rgbin_conv_kernel<7,7,3,1>", "rgbout_conv_kernel", "rgb_wgrad_kernel<0>"),
        "fp32/forced": ("rgbin_conv_kernel<7,7,3,1>", "rgbout_conv_kernel", "rgb_wgrad_kernel<0>"),
    },
    (3, 64, 32, 64, 3, 7, 1, 3, False, False): {
        "fp32/default": ("rgbout_conv_kernel", "rgbin_conv_kernel<7,7,3,1>", "rgb_wgrad_kernel<1>"),
        "fp32/forced": ("rgbout_conv_kernel", "rgbin_conv_kernel<7,7,3,1>", "rgb_wgrad_kernel<1>"),
    },
    (2, 3, 32, 40, 64, 7, 2, 1, False, True): {
        "fp32/default": ("igemm_kernel<128,64,2,2,false,false>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<64,64,2,2,false,false,false,false>"),
        "fp32/forced": ("igemm_kernel<128,64,2,2,false,false>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<64,64,2,2,false,false,false,false>"),
    },
    (3, 3, 33, 31, 32, 7, 2, 1, False, False): {
        "fp32/default": ("igemm_kernel<128,32,4,1,false,false>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<32,64,1,2,false,false,false,false>"),
        "fp32/forced": ("igemm_kernel<128,32,4,1,false,false>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<32,64,1,2,false,false,false,false>"),
    },
    (2, 4, 18, 22, 48, 6, 2, 2, False, False): {
        "fp32/default": ("igemm_kernel<128,64,2,2,false,false>", "narrow_conv_fwd_kernel<4>",
                         "wgrad_kernel<64,64,2,2,false,false,false,false>"),
        "fp32/forced": ("igemm_kernel<128,64,2,2,false,false>", "narrow_conv_fwd_kernel<4>",
                         "wgrad_kernel<64,64,2,2,false,false,false,false>"),
    },
    (2, 3, 16, 16, 16, 5, 2, 0, False, False): {
        "fp32/default": ("igemm_kernel<128,32,4,1,false,false>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<32,64,1,2,false,false,false,false>"),
        "fp32/forced": ("igemm_kernel<128,32,4,1,false,false>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<32,64,1,2,false,false,false,false>"),
    },
    (2, 256, 32, 32, 256, 3, 1, 1, False, False): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "igemm_kernel<64,64,2,2,true,false>", "wino_wgrad_kernel<0>"),
        "fp32/forced": ("wino43_kernel<false>", "wino43_kernel<false>", "wino_wgrad_kernel<0>"),
        "bf16/default": ("halo16r_kernel<false,false,false>", "halo16r_kernel<false,false,false>",
                         "halo16_wgrad_kernel<false,false>"),
    },
    (1, 128, 8, 64, 128, 3, 1, 1, False, True): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "igemm_kernel<64,64,2,2,true,false>",
                         "wgrad_kernel<128,128,2,2,true,true,false,false>"),
        "fp32/forced": ("wino43_kernel<false>", "wino43_kernel<false>", "wino_wgrad_kernel<0>"),
        "bf16/default": ("halo16_kernel<128,128,false,false,false>", "halo16_kernel<128,128,false,false,false>",
                         "halo16_wgrad_kernel<false,false>"),
    },
    (1, 256, 64, 64, 256, 3, 1, 1, False, False): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "igemm_kernel<64,64,2,2,true,false>", "wino_wgrad_kernel<0>"),
        "fp32/forced": ("wino43_kernel<false>", "wino43_kernel<false>", "wino_wgrad_kernel<0>"),
        "bf16/default": ("halo16r_kernel<false,false,false>", "halo16r_kernel<false,false,false>",
                         "halo16_wgrad_kernel<false,false>"),
    },
    (2, 64, 16, 64, 128, 4, 2, 1, False, False): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "igemm_kernel<128,64,2,2,true,false>",
                         "wgrad_kernel<128,64,2,2,true,true,false,false>"),
        "fp32/forced": ("wino42_kernel<1,false>", "wino42_kernel<2,false>", "wino_wgrad_kernel<1>"),
        "bf16/default": ("halo16s_kernel<64,128,false,false>", "halo16t_kernel<128,64,false,false>",
                         "halo16s2_wgrad_kernel<32,false,false>"),
    },
    (1, 128, 8, 64, 256, 4, 2, 1, False, False): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "igemm_kernel<64,64,2,2,true,false>",
                         "wgrad_kernel<128,128,2,2,true,true,false,false>"),
        "fp32/forced": ("wino42_kernel<1,false>", "wino42_kernel<2,false>", "wgrad_kernel<128,128,2,2,true,true,false,false>"),
        "bf16/default": ("halo16s_kernel<128,256,false,false>", "halo16t_kernel<256,128,false,false>",
                         "halo16s2_wgrad_kernel<32,false,false>"),
    },
    (3, 64, 64, 128, 128, 4, 2, 1, False, True): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "igemm_kernel<128,64,2,2,true,false>",
                         "wgrad_kernel<128,64,2,2,true,true,false,false>"),
        "fp32/forced": ("wino42_kernel<1,false>", "wino42_kernel<2,false>", "wino_wgrad_kernel<1>"),
        "bf16/default": ("halo16s_kernel<64,128,false,false>", "halo16t_kernel<128,64,false,false>",
                         "halo16s2_wgrad_kernel<32,false,false>"),
    },
    (2, 64, 40, 70, 3, 7, 1, 3, False, True): {
        "fp32/default": ("rgbout_conv_kernel", "rgbin_conv_kernel<7,7,3,1>", "narrow_conv_wgrad_kernel<3,4>"),
        "fp32/forced": ("rgbout_conv_kernel", "rgbin_conv_kernel<7,7,3,1>", "narrow_conv_wgrad_kernel<3,4>"),
    },
    (3, 3, 128, 128, 64, 7, 1, 3, False, False): {
        "fp32/default": ("rgbin_conv_kernel<7,7,3,1>", "rgbout_conv_kernel", "rgb_wgrad_kernel<0>"),
        "fp32/forced": ("rgbin_conv_kernel<7,7,3,1>", "rgbout_conv_kernel", "rgb_wgrad_kernel<0>"),
    },
    (2, 32, 64, 96, 3, 7, 1, 3, False, False): {
        "fp32/default": ("rgbout_conv_kernel", "igemm_kernel<128,32,4,1,false,false>", "narrow_conv_wgrad_kernel<3,4>"),
        "fp32/forced": ("rgbout_conv_kernel", "igemm_kernel<128,32,4,1,false,false>", "narrow_conv_wgrad_kernel<3,4>"),
    },
    (4, 64, 62, 62, 128, 3, 1, 1, True, False): {
        "fp32/default": ("wino_kernel<0,false>", "igemm_kernel<128,64,2,2,true,false>", "wino_wgrad_kernel<0>"),
        "fp32/forced": ("wino_kernel<0,false>", "wino_kernel<0,false>", "wino_wgrad_kernel<0>"),
        "bf16/default": ("igemm16_kernel<128,false,false,false>", "igemm16_kernel<64,false,false,false>",
                         "wgrad_kernel<128,64,2,2,true,false,true,false>"),
    },
    (4, 128, 31, 31, 128, 3, 1, 1, True, True): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "igemm_kernel<64,64,2,2,true,false>", "wino_wgrad_kernel<0>"),
        "fp32/forced": ("wino_kernel<0,false>", "wino_kernel<0,false>", "wino_wgrad_kernel<0>"),
        "bf16/default": ("igemm16_kernel<128,false,false,false>", "igemm16_kernel<128,false,false,false>",
                         "wgrad_kernel<128,128,2,2,true,false,true,false>"),
    },
    (8, 64, 30, 22, 64, 3, 1, 1, False, True): {
        "fp32/default": ("igemm_kernel<128,64,2,2,true,false>", "igemm_kernel<128,64,2,2,true,false>", "wino_wgrad_kernel<0>"),
        "fp32/forced": ("wino_kernel<0,false>", "wino_kernel<0,false>", "wino_wgrad_kernel<0>"),
        "bf16/default": ("igemm16_kernel<64,false,false,false>", "igemm16_kernel<64,false,false,false>",
                         "wgrad_kernel<64,64,2,2,true,false,true,false>"),
    },
    (6, 32, 15, 15, 64, 3, 1, 1, True, False): {
        "fp32/default": ("igemm_kernel<128,64,2,2,true,false>", "igemm_kernel<128,32,4,1,true,false>",
                         "wgrad_kernel<64,32,2,1,true,false,false,false>"),
        "fp32/forced": ("wino_kernel<0,false>", "wino_kernel<0,false>", "wgrad_kernel<64,32,2,1,true,false,false,false>"),
        "bf16/default": ("igemm_kernel<128,64,2,2,true,true>", "igemm_kernel<128,32,4,1,true,true>",
                         "wgrad_kernel<64,32,2,1,true,false,true,false>"),
    },
    (2, 96, 13, 18, 32, 3, 1, 1, True, True): {
        "fp32/default": ("igemm_kernel<128,32,4,1,true,false>", "igemm_kernel<64,64,2,2,true,false>",
                         "wgrad_kernel<32,32,1,1,true,false,false,false>"),
        "fp32/forced": ("wino_kernel<0,false>", "wino_kernel<0,false>", "wgrad_kernel<32,32,1,1,true,false,false,false>"),
        "bf16/default": ("igemm_kernel<128,32,4,1,true,true>", "igemm_kernel<64,64,2,2,true,true>",
                         "wgrad_kernel<32,32,1,1,true,false,true,false>"),
    },
    (16, 64, 66, 66, 64, 3, 1, 1, True, False): {
        "fp32/default": ("wino_kernel<0,false>", "wino_kernel<0,false>", "wino_wgrad_kernel<0>"),
        "fp32/forced": ("wino_kernel<0,false>", "wino_kernel<0,false>", "wino_wgrad_kernel<0>"),
        "bf16/default": ("igemm16_kernel<64,false,false,false>", "igemm16_kernel<64,false,false,false>",
                         "wgrad_kernel<64,64,2,2,true,false,true,false>"),
    },
    (9, 256, 64, 16, 64, 4, 2, 1, False, False): {
        "fp32/default": ("igemm_kernel<128,64,2,2,true,false>", "igemm_kernel<64,64,2,2,true,false>",
                         "wgrad_kernel<64,128,2,2,true,false,false,false>"),
        "fp32/forced": ("wino_kernel<1,false>", "wino42_kernel<2,false>", "wino_wgrad_kernel<1>"),
        "bf16/default": ("igemm16_kernel<64,false,false,false>", "igemm16_kernel<128,false,false,false>",
                         "halo16s2_wgrad_kernel<8,false,false>"),
    },
    (4, 128, 32, 48, 192, 4, 2, 1, False, True): {
        "fp32/default": ("igemm_kernel<64,64,2,2,true,false>", "igemm_kernel<64,64,2,2,true,false>",
                         "wgrad_kernel<128,128,2,2,true,false,false,false>"),
        "fp32/forced": ("wino42_kernel<1,false>", "wino42_kernel<2,false>", "wino_wgrad_kernel<1>"),
        "bf16/default": ("igemm16_kernel<128,false,false,false>", "igemm16_kernel<128,false,false,false>",
                         "wgrad_kernel<128,128,2,2,true,false,true,false>"),
    },
    (3, 3, 128, 128, 64, 4, 2, 1, False, False): {
        "fp32/default": ("rgbin_conv_kernel<4,4,3,2>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<64,64,2,2,false,false,false,false>"),
        "fp32/forced": ("rgbin_conv_kernel<4,4,3,2>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<64,64,2,2,false,false,false,false>"),
    },
    (2, 3, 70, 90, 128, 4, 2, 1, False, True): {
        "fp32/default": ("rgbin_conv_kernel<4,4,3,2>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<128,64,2,2,false,false,false,false>"),
        "fp32/forced": ("rgbin_conv_kernel<4,4,3,2>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<128,64,2,2,false,false,false,false>"),
    },
    (3, 3, 128, 128, 64, 7, 2, 1, False, True): {
        "fp32/default": ("rgbin_conv_kernel<7,7,3,2>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<64,64,2,2,false,false,false,false>"),
        "fp32/forced": ("rgbin_conv_kernel<7,7,3,2>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<64,64,2,2,false,false,false,false>"),
    },
    (2, 3, 71, 77, 64, 7, 2, 1, False, False): {
        "fp32/default": ("rgbin_conv_kernel<7,7,3,2>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<64,64,2,2,false,false,false,false>"),
        "fp32/forced": ("rgbin_conv_kernel<7,7,3,2>", "narrow_conv_fwd_kernel<3>",
                         "wgrad_kernel<64,64,2,2,false,false,false,false>"),
    },
    (40, 64, 16, 16, 64, 4, 2, 1, False, False): {
        "fp32/default": ("igemm_kernel<128,64,2,2,true,false>", "igemm_kernel<128,64,2,2,true,false>",
                         "wgrad_kernel<64,64,2,2,true,false,false,false>"),
        "fp32/forced": ("wino42_kernel<1,false>", "wino42_kernel<2,false>", "wgrad_kernel<64,64,2,2,true,false,false,false>"),
        "bf16/default": ("igemm16_kernel<64,false,false,false>", "igemm16_kernel<64,false,false,false>",
                         "halo16s2_wgrad_kernel<8,false,false>"),
    },
}


def _random_conv_cases(n_cases, seed):
    """Seeded random layer geometries across every dispatch family (narrow / RGB / stride-2 phases / split-K / Winograd / GEMM)."""
    rng = np.random.RandomState(seed)
    cases = []
    while len(cases) < n_cases:
        k = int(rng.choice([1, 3, 3, 4, 4, 5, 7]))
        s_ = int(rng.choice([1, 1, 2]))
        i = int(rng.choice([3, 4, 16, 32, 48, 64, 96, 128, 256]))
        o = int(rng.choice([1, 3, 4, 16, 32, 64, 96, 128, 512]))
        h, w = int(rng.randint(max(k, 3), 41)), int(rng.randint(max(k, 3), 41))
        p_ = int(rng.randint(0, k // 2 + 1))
        reflect = bool(s_ == 1 and 0 < p_ < min(h, w) and k == 3 and rng.rand() < 0.4)
        n = int(rng.randint(1, 7))
        if (h + 2 * p_ - k) // s_ + 1 < 1 or (w + 2 * p_ - k) // s_ + 1 < 1 or n * i * h * w > 3_000_000:
            continue
        cases.append((n, i, h, w, o, k, s_, p_, reflect, bool(rng.rand() < 0.5)))
    return cases


def _random_bf16_conv_cases(n_cases, seed):
    """Seeded random geometries of the layers the bf16 kernels serve (Cin a multiple of 32, Cout >= 32): patch kernels, the
    64-deep-K implicit GEMM (Cin % 64 == 0: ragged pixel / channel tiles, stride-2 phases, reflect, 1x1, split-K) and the rest."""
    rng = np.random.RandomState(seed)
    cases = []
    while len(cases) < n_cases:
        k = int(rng.choice([1, 3, 3, 4, 4]))
        s_ = int(rng.choice([1, 1, 2]))
        i = int(rng.choice([32, 64, 64, 96, 128, 128, 192, 256]))
        o = int(rng.choice([32, 64, 96, 128, 160, 256, 512]))
        h, w = int(rng.randint(max(k, 3), 41)), int(rng.randint(max(k, 3), 41))
        p_ = int(rng.randint(0, k // 2 + 1))
        reflect = bool(s_ == 1 and 0 < p_ < min(h, w) and k == 3 and rng.rand() < 0.4)
        n = int(rng.randint(1, 9))
        if (h + 2 * p_ - k) // s_ + 1 < 1 or (w + 2 * p_ - k) // s_ + 1 < 1 or n * i * h * w > 3_000_000:
            continue
        cases.append((n, i, h, w, o, k, s_, p_, reflect, bool(rng.rand() < 0.5)))
    return cases


RANDOM_CASES = _random_conv_cases(48, seed=20260410)                 # test_conv2d_random_geometries
RANDOM_BF16_CASES = _random_bf16_conv_cases(32, seed=20261004)       # test_conv2d_bf16_random_geometries
# layers the bf16 kernels serve: vector-gather implicit GEMM (Cin % 32 == 0, Cout >= 32); RGB / 1-channel heads stay fp32
BF16_MODE_CASES = [c for c in CONV_CASES if c[1] % 32 == 0 and c[4] >= 32 and c[0] * c[2] * c[3] <= 70000]

# ---- shape lists of the other convolution tests of test_ops_gpu.py (each in the form its test takes it) ------------------------
F43_CASES = [(32, 64, 32, 32, 128, True), (3, 64, 8, 12, 96, True), (5, 128, 16, 16, 64, False),      # n, i, h, w, o, bias
             (2, 256, 32, 32, 256, False)]
SKIP_CASES = [(32, 64, 32, 32, 64), (3, 64, 8, 12, 64), (2, 16, 9, 7, 16), (2, 256, 32, 32, 256)]     # n, i, h, w, o
SKIP_BF16_CASES = [(3, 64, 8, 32, 64), (2, 256, 32, 32, 256), (1, 128, 12, 64, 128)]
# n, c, o, affine (32 x 32 maps); (3, 96, 64): c % 64 != 0, so no V image is kept (srgan_conv2d_wgrad_v_bytes == 0) and the backward of
# ops._NormActConvFn recomputes the normalised input for srgan_conv2d_wgrad
NORM_ACT_CONV_CASES = [(32, 256, 256, True), (4, 64, 64, True), (3, 64, 96, False), (3, 96, 64, True)]
# n, i, o of tests/test_trunk_kernels_gpu.py (32 x 32 maps; tests/trunk_common.py names what each is there for)
TRUNK_CASES = [(1, 32, 32), (3, 96, 64), (8, 64, 32), (16, 128, 96), (5, 256, 256), (1, 64, 32), (2, 64, 128), (2, 128, 64), (8, 64, 64),
               (11, 128, 128), (2, 32, 32), (2, 64, 32)]
RESBLOCK_CASES = [(32, 256), (4, 64), (3, 128)]                                                      # n, c (32 x 32 maps)
RESBLOCK_BF16_CASES = [(32, 256, 32), (64, 64, 32), (32, 128, 32), (8, 256, 64)]                     # n, c, hw
STRIDE2_IO_SHAPE = (2, 64, 128, 16, 64)                                                              # n, ci, co, h, w
CONV_ACT_IO_SHAPES = [(2, 64, 128, 64, 64), (3, 128, 256, 32, 32), (4, 256, 512, 16, 16), (2, 64, 128, 16, 16),
                      (2, 512, 512, 16, 16)]
RGB_IO_SHAPES = [(2, 32, 64), (3, 80, 96)]                                                           # n, h, w
GENERIC_IO_SHAPES = [(2, 64, 128, 30, 30, "reflect"), (3, 128, 128, 15, 15, "reflect"), (4, 256, 512, 7, 7, "reflect"),
                     (2, 128, 64, 12, 20, "zeros"),
                     # round 6: the same Functions with the encoder's large-map layers on halo16e_kernel (the
                     # dispatch threshold switched off so that these small batches take it): every (Cin, Cout) it
                     # is instantiated for, ragged patches in both directions, reflect (input gradient = padded
                     # gradient + fold) and zero padding (input gradient straight into the tensor)
                     (2, 64, 64, 30, 30, "reflect", "halo"), (2, 64, 128, 62, 62, "reflect", "halo"),
                     (3, 128, 128, 31, 31, "reflect", "halo"), (2, 128, 256, 31, 31, "reflect", "halo"),
                     (2, 64, 128, 20, 40, "zeros", "halo"), (1, 128, 128, 9, 33, "zeros", "halo"),
                     (2, 128, 256, 8, 64, "zeros", "halo"), (1, 64, 64, 33, 5, "reflect", "halo")]
RGB_BF16_SHAPES = [(2, 32, 64), (5, 64, 416)]                                                        # n, h, w
LRELU_CHAIN_CASES = [(8, 64, 128, 256, 64, True), (2, 8, 16, 24, 16, True), (2, 32, 64, 64, 32, False)]     # n, c0, c1, c2, hw, packed


# ---- tests/test_conv_kernels_gpu.py: one case per instantiation no case above launches -----------------------------------------
# (case, {compute mode: {direction: kernel the case is there for}}).  Default dispatch; 1x1 and 5x5 filters, because a 3x3 /
# stride-1 or 4x4 / stride-2 layer goes to the Winograd / patch kernels.  The sizes are the smallest choose_tile / plan_wgrad /
# the narrow launch switches allow, with a ragged last tile in M = N * Ho * Wo and in the channel dimension (the row-aligned
# weight-gradient path and the patch kernels take whole 32-pixel rows / 4 x 32 patches only: there the channel tile is the ragged one):
#   256x128 tiles  ceil(M / 256) * ceil(Cd / 128) >= 256: Cd = 480 or 500 (4 tiles, the last 96 / 116 wide), M = 3 * 74 * 73 = 16,206 (64 tiles, the last 78 rows)
#   128x128 tiles  ceil(M / 128) * ceil(Cd / 128) >= 256 and fewer than 256 big tiles: M = 2 * 74 * 73 = 10,804 (85 x 4 / 43 x 4)
#   256x64 tiles   33 <= Cd <= 64 and ceil(M / 256) >= 256: Cd = 48, M = 255 * 258 = 65,790 (257 tiles, the last 254 rows)
# A 256-row tile needs the vector gather (Cs % 32 == 0); with any other Cs run_igemm_tiles falls back to 128 rows.  In the bf16
# mode Cs = 32 keeps the layer off igemm16_kernel (Cs % 64 != 0) and on igemm_kernel<..., true, true>.
_IG = "igemm_kernel"
_WG = "wgrad_kernel"
_NW = "narrow_conv_wgrad_kernel"
KERNEL_CASES = [
    # N, I, H, W, O, k, s, p, reflect, bias
    ((3, 32, 74, 73, 480, 5, 1, 2, False, True),       # E.l0.shortcut forward class (c3_128_b64, c4_256_b16), 5x5 taps
     {"fp32": {"fwd": _IG + "<256,128,4,2,true,false>"}, "bf16": {"fwd": _IG + "<256,128,4,2,true,true>"}}),
    ((3, 480, 74, 73, 32, 1, 1, 0, False, False),      # the same tile on the input gradient (Cd = 480 input channels)
     {"fp32": {"dgrad": _IG + "<256,128,4,2,true,false>"}, "bf16": {"dgrad": _IG + "<256,128,4,2,true,true>"}}),
    ((3, 500, 74, 73, 6, 1, 1, 0, False, True),        # D0.last / D0.cls input gradient class: 256 big tiles but a scalar gather
     {"fp32": {"dgrad": _IG + "<128,128,2,2,false,false>"}}),      # (Cs = 6): the 256-row choice falls back to 128x128 generic
    ((2, 6, 74, 73, 500, 1, 1, 0, False, True),        # 128x128 generic chosen directly (172 big tiles), forward
     {"fp32": {"fwd": _IG + "<128,128,2,2,false,false>"}}),
    ((2, 32, 74, 73, 480, 1, 1, 0, False, False),      # 128x128 vector tile in the bf16 mode (fp32: <..., true, false>)
     {"fp32": {"fwd": _IG + "<128,128,2,2,true,false>"}, "bf16": {"fwd": _IG + "<128,128,2,2,true,true>"}}),
    ((1, 32, 255, 258, 48, 1, 1, 0, False, True),      # 256x64 forward
     {"fp32": {"fwd": _IG + "<256,64,4,2,true,false>"}, "bf16": {"fwd": _IG + "<256,64,4,2,true,true>"}}),
    ((1, 48, 255, 258, 32, 1, 1, 0, False, False),     # 256x64 input gradient (E.l0.shortcut's: Cd = 48 input channels)
     {"fp32": {"dgrad": _IG + "<256,64,4,2,true,false>"}, "bf16": {"dgrad": _IG + "<256,64,4,2,true,true>"}}),
    ((1, 6, 255, 258, 48, 1, 1, 0, False, False),      # 257 big tiles, scalar gather: falls back to 128x64 generic (514 tiles, the last 126 rows)
     {"fp32": {"fwd": _IG + "<128,64,2,2,false,false>"}}),
    # weight gradient, row-aligned path (Wo % 32 == 0, M % 32 == 0, O % 4 == 0): tiles from O (<= 32 / <= 64 / more) and I (% 128 / % 64)
    ((2, 128, 8, 32, 132, 1, 1, 0, False, True),       # 128x128 rows, two output-channel tiles (the second 4 wide)
     {"bf16": {"wgrad": _WG + "<128,128,2,2,true,true,true,false>"}}),
    ((2, 128, 8, 32, 48, 5, 1, 2, False, True),        # 64x128 rows, 5x5 taps with zero padding, 48 of 64 output channels
     {"fp32": {"wgrad": _WG + "<64,128,2,2,true,true,false,false>"}, "bf16": {"wgrad": _WG + "<64,128,2,2,true,true,true,false>"}}),
    ((3, 64, 6, 32, 48, 1, 1, 0, False, False),        # 64x64 rows in the bf16 mode
     {"bf16": {"wgrad": _WG + "<64,64,2,2,true,true,true,false>"}}),
    # narrow-output layers (O <= 4, stride 1, zero padding, I % 16 == 0): narrow_conv_wgrad_kernel<O, ceil(k * k / 16)>; maps of
    # 2 x 2 tiles of 8 x 32 pixels, both ragged; their forward is narrow_conv_fwd_kernel<O>
    ((2, 16, 13, 36, 1, 6, 1, 2, False, True), {"fp32": {"wgrad": _NW + "<1,3>"}}),
    ((2, 16, 12, 35, 1, 7, 1, 3, False, False), {"fp32": {"wgrad": _NW + "<1,4>"}}),
    ((2, 32, 10, 35, 2, 3, 1, 1, False, True), {"fp32": {"wgrad": _NW + "<2,1>", "fwd": "narrow_conv_fwd_kernel<2>"}}),
    ((2, 16, 10, 35, 2, 5, 1, 2, False, False), {"fp32": {"wgrad": _NW + "<2,2>"}}),
    ((1, 16, 13, 36, 2, 6, 1, 2, False, True), {"fp32": {"wgrad": _NW + "<2,3>"}}),
    ((2, 16, 12, 35, 2, 7, 1, 3, False, False), {"fp32": {"wgrad": _NW + "<2,4>"}}),
    ((2, 32, 10, 35, 3, 3, 1, 1, False, True), {"fp32": {"wgrad": _NW + "<3,1>"}}),
    ((2, 16, 10, 35, 3, 5, 1, 2, False, False), {"fp32": {"wgrad": _NW + "<3,2>"}}),
    ((1, 16, 13, 36, 3, 6, 1, 2, False, True), {"fp32": {"wgrad": _NW + "<3,3>"}}),
    ((2, 16, 13, 36, 4, 6, 1, 2, False, False), {"fp32": {"wgrad": _NW + "<4,3>"}}),
    # one wave per output pixel (O <= 4, I % 4 == 0, I >= 128, at most 1024 output pixels)
    ((2, 128, 7, 9, 2, 3, 1, 1, False, True), {"fp32": {"fwd": "narrow_wave_fwd_kernel<2>"}}),
    ((2, 132, 7, 9, 3, 4, 1, 1, False, False), {"fp32": {"fwd": "narrow_wave_fwd_kernel<3>"}}),
    # 7x7 RGB head that the row convolution does not take (I % 32 != 0): 8 x 128 tiles, two ragged column tiles, 6 channel passes
    ((2, 48, 9, 140, 3, 7, 1, 3, False, True), {"fp32": {"fwd": "narrow_conv_fwd4_kernel<3,7>"}}),
]
KERNEL_MODES = {"fp32": "m0", "bf16": "m1"}
# srgan_halo16_conv on the residual-trunk layers (3x3 / stride 1 / pad 1, C -> C, maps of whole 4 x 32 patches, bf16 mode) with a bf16
# source, an fp32 result and no skip tensor: the pairing no Function of srgan_amd.ops uses (the residual-block node writes bf16 or
# adds the skip gradient), so tests/test_conv_kernels_gpu.py calls the entry itself, both kinds: (case, kernel)
HALO16_IO_CASES = [
    ((2, 64, 8, 32, 64, 3, 1, 1, False, False), "halo16_kernel<64,64,false,true,false>"),
    ((1, 128, 8, 64, 128, 3, 1, 1, False, False), "halo16_kernel<128,128,false,true,false>"),
    ((1, 256, 4, 32, 256, 3, 1, 1, False, False), "halo16r_kernel<false,true,false>"),
]
# The LeakyReLU backward of the producing layer in the epilogue of the transposed Winograd kernels (srgan_conv2d_dgrad_packed_mask,
# ops.conv2d(..., in_slope=...) inside a pack-cache scope), dispatch thresholds off: (case, kernel)
MASK_CASES = [
    ((2, 32, 14, 16, 64, 4, 2, 1, False, False), "wino_kernel<2,true>"),        # F(3x3,2x2): 7 x 8 output map, ragged 3x3 tiles
    ((2, 128, 16, 24, 192, 4, 2, 1, False, False), "wino42_kernel<2,true>"),    # F(4x4,2x2): 2 x 3 tiles per image and phase
]
# 128 -> 256 down convolution with 16-bit tensors on either side (ops.conv2d_s2_io, bf16 mode): halo16s_kernel<128, 256, IN16, OUT16>
# forward, halo16t_kernel<256, 128, IN16, OUT16> input gradient, halo16s2_wgrad_kernel<32, X16, D16>; two patches of 4 x 32 pixels
S2_IO_CASE = (1, 128, 16, 64, 256, 4, 2, 1, False, False)

# launches that move operands or sum partial results around the kernel a case is about
HELPERS = {"pack_weights_kernel", "pack_multi_kernel", "wino_pack_kernel", "narrow_pack_kernel", "narrow_pack4_kernel",
           "rowconv_pack_kernel", "rowconv_shift_add_kernel", "rgbin_pack_kernel", "rgbout_pack_kernel", "rgbin16_pack_kernel",
           "rgbout16_pack_kernel", "splitk_reduce_kernel<false>", "splitk_reduce_kernel<true>", "wgrad_reduce_kernel",
           "wgrad_reduce_wave_kernel", "wgrad_reduce_multi_kernel", "colsum_partial_kernel", "colsum_final_kernel",
           "colsum_narrow_kernel", "reflect_fold_kernel<false>", "reflect_fold_kernel<true>", "add_inplace_kernel", "act_bwd_kernel"}


def main_kernel(launches):
    """The kernel an entry's launch list is about: its last launch that is not a helper."""
    ks = [k for k in launches if k not in HELPERS]
    return ks[-1] if ks else None


def full(n, i, h, w, o, k, s, p, reflect=False, bias=False):
    return (n, i, h, w, o, k, s, p, bool(reflect), bool(bias))


# ---- which entry points each GPU test drives, with which cases ---------------------------------------------------------------
# (test, cases in the 10-tuple form, compute modes, dispatch settings, entries).  An entry is a mark of drive_conv.py, or a
# prefix of one ending in ":" (every dtype pairing of that entry); "wgrad*" = srgan_conv2d_wgrad_v where the layer keeps its
# transformed input (srgan_conv2d_wgrad_v_bytes != 0), else srgan_conv2d_wgrad -- what ops.conv2d does inside a pack-cache scope.
UNPACKED = ("fwd", "dgrad", "wgrad")
PACKED = ("pack0", "fwd_packed", "pack1", "dgrad_packed", "wgrad*")
_BOTH = ("default", "forced")
_generic_io = [(full(n, ci, h, w, co, 3, 1, 1, pm == "reflect"), "forced" if rest else "default")
               for n, ci, co, h, w, pm, *rest in GENERIC_IO_SHAPES]
COVERAGE = [
    ("test_ops_gpu::test_conv2d_fwd_bwd", CONV_CASES, ("m0",), _BOTH, UNPACKED),
    ("test_ops_gpu::test_conv2d_random_geometries", RANDOM_CASES, ("m0",), _BOTH, PACKED),
    ("test_ops_gpu::test_conv2d_bf16_compute_mode", BF16_MODE_CASES, ("m1",), ("default",), UNPACKED),
    ("test_ops_gpu::test_conv2d_bf16_random_geometries", RANDOM_BF16_CASES, ("m1",), ("default",), PACKED),
    ("test_ops_gpu::test_conv2d_f43_weight_gradient_from_kept_image", [full(n, i, h, w, o, 3, 1, 1, False, b) for n, i, h, w, o, b in F43_CASES],
     ("m0",), _BOTH, PACKED),
    ("test_ops_gpu::test_conv2d_skip_gradient_rides_in_the_dgrad_epilogue", [full(n, i, h, w, o, 3, 1, 1) for n, i, h, w, o in SKIP_CASES],
     ("m0",), _BOTH, ("pack0", "fwd_packed", "pack1", "dgrad_packed_add", "wgrad*") + UNPACKED),
    ("test_ops_gpu::test_conv2d_skip_bf16_mode", [full(n, i, h, w, o, 3, 1, 1) for n, i, h, w, o in SKIP_BF16_CASES],
     ("m1",), ("default",), ("pack0", "fwd_packed", "pack1", "dgrad_packed_add")),
    # the fused nodes: V / Z images written by the norm kernels of conv_wino43.hip, multiply + weight gradient from them
    ("test_ops_gpu::test_instance_norm_act_conv_equals_the_unfused_chain", [full(n, c, 32, 32, o, 3, 1, 1) for n, c, o, _ in NORM_ACT_CONV_CASES],
     ("m0",), ("forced",), ("pack0", "instnorm_fwd_v", "fwd_from_v", "pack1", "dgrad_packed", "wgrad*")),
    ("test_ops_gpu::test_residual_block_fused_node_vs_chain_and_cpu", [full(n, c, 32, 32, c, 3, 1, 1) for n, c in RESBLOCK_CASES],
     ("m0",), ("forced",), ("pack0", "fwd_packed", "instnorm_fwd_v", "fwd_from_v", "pack1", "instnorm_bwd_vz", "dgrad_from_v",
                            "wgrad_vz", "dgrad_packed_add", "wgrad_v")),
    # the same entries called one by one through ctypes, each composition against float64
    ("test_trunk_kernels_gpu", [full(n, i, 32, 32, o, 3, 1, 1) for n, i, o in TRUNK_CASES], ("m0",), ("forced",),
     ("pack0", "fwd_packed", "instnorm_fwd_v", "fwd_from_v", "pack1", "instnorm_bwd_vz", "dgrad_from_v", "wgrad_vz")),
    ("test_ops_gpu::test_residual_block_bf16_storage", [full(n, c, hw, hw, c, 3, 1, 1) for n, c, hw in RESBLOCK_BF16_CASES],
     ("m1",), ("default",), ("pack0", "pack1", "halo16_conv:kind0:in16=0:out16=1", "halo16_conv:kind0:in16=1:out16=1",      # ops._ResBlockBf16Fn's
                             "halo16_conv:kind1:in16=1:out16=1", "halo16_conv_res:in16=1",                                  # own calls, no others
                             "halo16_wgrad:x16=0:d16=1", "halo16_wgrad:x16=1:d16=1")),
    ("test_ops_gpu::test_stride2_io_functions_every_dtype_pair", [full(*STRIDE2_IO_SHAPE[:2], *STRIDE2_IO_SHAPE[3:], STRIDE2_IO_SHAPE[2], 4, 2, 1)],
     ("m1",), ("default",), ("pack0", "pack1", "halo16_conv:", "halo16_wgrad:")),
    ("test_ops_gpu::test_conv_act_io_every_dtype_pair", [full(n, ci, h, w, co, 4, 2, 1) for n, ci, co, h, w in CONV_ACT_IO_SHAPES],
     ("m1",), ("default",), ("io_fwd:act2:", "io_dgrad:act2:", "io_wgrad:")),
    ("test_ops_gpu::test_rgb_layers_with_a_bf16_64_channel_side",
     [full(n, ci, h, w, co, 7, 1, 3) for n, h, w in RGB_IO_SHAPES for ci, co in ((3, 64), (64, 3))],
     ("m1",), ("default",), ("io_fwd:act0:", "io_dgrad:act0:", "io_wgrad:")),
    ("test_ops_gpu::test_generic_conv_io_every_dtype_pair", [c for c, d in _generic_io if d == "default"],
     ("m1",), ("default",), ("pack0", "pack1", "igemm16_conv:", "igemm16_wgrad") + PACKED),
    ("test_ops_gpu::test_generic_conv_io_every_dtype_pair[halo]", [c for c, d in _generic_io if d == "forced"],
     ("m1",), ("forced",), ("pack0", "pack1", "igemm16_conv:", "igemm16_wgrad") + PACKED),
    ("test_ops_gpu::test_rgb_input_form_bf16_compute_mode",
     [full(n, ci, h, w, co, 7, 1, 3) for n, h, w in RGB_BF16_SHAPES for ci, co in ((3, 64), (64, 3))],
     ("m1",), ("default",), UNPACKED + PACKED),
    ("test_ops_gpu::test_leaky_relu_backward_in_the_consumers_input_gradient",
     [full(n, c1, hw // 2, hw // 2, c2, 4, 2, 1) for n, c0, c1, c2, hw, packed in LRELU_CHAIN_CASES if packed],
     ("m0",), ("default",), ("pack1", "dgrad_packed_mask")),
    ("test_conv_kernels_gpu::test_conv_kernel[fp32]", [c for c, w in KERNEL_CASES if "fp32" in w], ("m0",), ("default",), UNPACKED + PACKED),
    ("test_conv_kernels_gpu::test_conv_kernel[bf16]", [c for c, w in KERNEL_CASES if "bf16" in w], ("m1",), ("default",), UNPACKED + PACKED),
    ("test_conv_kernels_gpu::test_masked_input_gradient", [c for c, _ in MASK_CASES], ("m0",), ("forced",), ("pack0", "fwd_packed", "pack1", "dgrad_packed_mask", "wgrad*")),
    ("test_conv_kernels_gpu::test_halo16_bf16_source_fp32_result", [c for c, _ in HALO16_IO_CASES], ("m1",), ("default",),
     ("pack0", "pack1", "halo16_conv:kind0:in16=1:out16=0", "halo16_conv:kind1:in16=1:out16=0")),
    ("test_conv_kernels_gpu::test_stride2_io_kernels", [S2_IO_CASE], ("m1",), ("default",), ("pack0", "pack1", "halo16_conv:", "halo16_wgrad:")),
    # one launch for all stale operands / all queued slab sums: compared with the single launches, whose results the tests above hold
    ("test_ops_gpu::test_multi_pack_launch_equals_single_pack", [], (), (), ("pack_multi",)),
    ("test_ops_gpu::test_fused_param_grads_equal_autograd_accumulation", [], (), (), ("wgrad_deferred",)),
]

# ---- instantiations that exist in the code objects and that no descriptor can launch ------------------------------------------
# (kernel, the dispatch condition as the source states it -- every string is a quote tests/test_conv_refs_cpu.py looks up -- and
# why no descriptor meets it)
_DMA = (('static const bool no_dma = SRGAN_AB_SET("SRGAN_NO_IG16_DMA");', "const bool dma = !no_dma;",
         "if (p.src16 && o16 && dma)", "else if (p.src16 && dma)"),
        "launch_igemm16: SRGAN_AB_SET is false outside an experiment build, so dma is true and the first two branches take every "
        "bf16 source; the <BN, true, *, false> instantiations behind them are never reached")
_BIG = (("if (tc.BM == 256 && tc.BN == 128 && vec) return launch_igemm<256, 128, 4, 2>(p, phases, true, st, flops);",
         "if (tc.BM == 256 && tc.BN == 64 && vec) return launch_igemm<256, 64, 4, 2>(p, phases, true, st, flops);",
         "if (tc.BM == 256) { tc = {128, tc.BN}; p.m_tiles = (int)ceil_div(p.M, 128); }"),
        "run_igemm_tiles: a 256-row tile is launched with vec = true only, a scalar gather falls back to 128 rows; launch_igemm "
        "instantiates all three gathers of every tile")
_NN = (("if (w.vec) w.BNn = (d->I % 128 == 0) ? 128 : ((d->I % 64 == 0) ? 64 : 32);", "else w.BNn = 64;"),
       "plan_wgrad: a scalar gather always has 64 columns; wgrad_variant instantiates it for every tile of wgrad_lookup")
DEAD = [(k, *_DMA) for k in ("igemm16_kernel<128,true,false,false>", "igemm16_kernel<128,true,true,false>",
                             "igemm16_kernel<64,true,false,false>", "igemm16_kernel<64,true,true,false>")] + \
       [(k, *_BIG) for k in ("igemm_kernel<256,128,4,2,false,false>", "igemm_kernel<256,64,4,2,false,false>")] + \
       [(k, *_NN) for k in ("wgrad_kernel<128,128,2,2,false,false,false,false>", "wgrad_kernel<128,32,4,1,false,false,false,false>",
                            "wgrad_kernel<64,128,2,2,false,false,false,false>", "wgrad_kernel<64,32,2,1,false,false,false,false>",
                            "wgrad_kernel<32,128,1,4,false,false,false,false>", "wgrad_kernel<32,32,1,1,false,false,false,false>")]
# (kernel, smallest reaching shape, why that shape exceeds a seconds-long test)
DEFERRED = []


# ---- the launches the library makes (CPU, under tests/hip_shim/launch_shim.c) ---------------------------------------------------
def kernel_name(mangled):
    """`_ZN5srgan12igemm_kernelILi256ELi128ELi4ELi2ELb1ELb0EEEvNS_11IgemmParamsE` -> `igemm_kernel<256,128,4,2,true,false>`."""
    m = re.match(r"_ZN5srgan(?:12_GLOBAL__N_1)?(\d+)", mangled)
    if not m:
        return mangled
    n = int(m.group(1))
    name, rest = mangled[m.end():m.end() + n], mangled[m.end() + n:]
    t = re.match(r"I((?:L[ib]n?\d+E)+)E", rest)
    if not t:
        assert not rest.startswith("I"), mangled          # a template argument this parser does not know
        return name
    args = [("true" if v == "1" else "false") if ty == "b" else ("-" if neg else "") + v
            for ty, neg, v in re.findall(r"L([ib])(n?)(\d+)E", t.group(1))]
    return name + "<" + ",".join(args) + ">"


def tag(case):
    return "x".join(str(int(v)) for v in case)


def drive(lib_path, shim_so, cases, workdir):
    """{(tag, mode, dispatch, entry): [kernel, ...]} of tests/hip_shim/drive_conv.py over `cases` (10-tuples) under the shim."""
    cases = sorted(set(cases))
    path, log = os.path.join(workdir, "conv_cases.json"), os.path.join(workdir, "conv_launches.log")
    with open(path, "w") as f:
        json.dump([[tag(c)] + [int(v) for v in c] for c in cases], f)
    preload = shim_so + (":" + os.environ["LD_PRELOAD"] if os.environ.get("LD_PRELOAD") else "")
    env = dict(os.environ, LD_PRELOAD=preload, SRGAN_SHIM_LOG=log)
    env.pop("SRGAN_HIP_LIB", None)
    env.pop("SRGAN_WINOGRAD_THRESHOLD_SCALE", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "hip_shim", "drive_conv.py"), lib_path, path], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out, where = {}, None
    for line in open(log):
        if line.startswith("#"):
            where = tuple(line[1:].split())
            assert where not in out, where
            out[where] = []
            continue
        out[where].append(kernel_name(line.split()[0]))
    return out


def covered_entries(launches, case, mode, dispatch, entries):
    """The marks of `launches` that a COVERAGE row's entries select for one (case, mode, dispatch)."""
    t = tag(case)
    have = [k[3] for k in launches if k[:3] == (t, mode, dispatch)]
    out = []
    for e in entries:
        if e == "wgrad*":
            out.append("wgrad_v" if "wgrad_v" in have else "wgrad")
        elif e.endswith(":"):
            out += [h for h in have if h.startswith(e)]
        elif e in have:
            out.append(e)
    return [(t, mode, dispatch, e) for e in out]


# ---- reference and error measure -----------------------------------------------------------------------------------------------
def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def inputs(case):
    """x, w, bias (or None), dy of a case: the seeds and scaling of test_conv2d_fwd_bwd."""
    n, i, h, w, o, k, s, p, reflect, has_bias = case
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    return (rnd(n, i, h, w, seed=1), rnd(o, i, k, k, seed=2) / np.sqrt(i * k * k), (rnd(o, seed=3) * 0.1) if has_bias else None,
            rnd(n, o, ho, wo, seed=4))


def conv_ref(x, w, b, stride, pad, reflect):
    """The convolution of oracle/nets.py: F.conv2d, reflect padding as F.pad in front of an unpadded convolution."""
    if reflect:
        return F.conv2d(F.pad(x, (pad, pad, pad, pad), mode="reflect"), w, b, stride, 0)
    return F.conv2d(x, w, b, stride, pad)


def _grads(case, x, w, b, gy, dtype):
    s, p, reflect = case[6], case[7], case[8]
    # (copies: `.to` of a tensor that already has the type returns the tensor itself, and the caller's inputs stay leaves without a graph)
    xv, wv = (t.detach().to(dtype, copy=True).requires_grad_(True) for t in (x, w))
    bv = b.detach().to(dtype, copy=True).requires_grad_(True) if b is not None else None
    y = conv_ref(xv, wv, bv, s, p, reflect)
    g = torch.autograd.grad(y, [xv, wv] + ([bv] if b is not None else []), gy.detach().to(dtype))
    return y.detach(), g[0], g[1], (g[2] if b is not None else None)


def reference(case, x, w, b, gy, dtype=torch.float64, bf16=False):
    """(y, dx, dw, db) in `dtype` by autograd.  bf16: the products of the bf16 compute mode as test_conv2d_bf16_compute_mode
    states them -- y = conv(bf16(x), bf16(w)), dx = dgrad(bf16(dy), bf16(w)), dw = wgrad(bf16(x), bf16(dy)); db sums dy itself."""
    if not bf16:
        return _grads(case, x, w, b, gy, dtype)
    r = bf16_round
    y = _grads(case, r(x), r(w), b, gy, dtype)[0]
    dx = _grads(case, x, r(w), b, r(gy), dtype)[1]
    dw = _grads(case, r(x), w, b, r(gy), dtype)[2]
    db = _grads(case, x, w, b, gy, dtype)[3]
    return y, dx, dw, db


def rel_err(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if not bool(torch.isfinite(a).all()):
        return float("inf")
    return float((a - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


BOUND = {"y": 2e-5, "dx": 2e-5, "dw": 5e-5, "db": 5e-5}
ATOL = 1e-6
FIGURES = []                    # (kernel, what, e32, err, bound) of every check of the process (test_conv_kernels_gpu.py logs them)


def bf16_store(ref64):
    """Half a bf16 ulp of max |ref|, relative to max |ref| (norm_common.bf16_store): 2^(floor(log2 max |ref|) - 8) / max |ref|,
    between 2^-9 and 2^-8 -- what one round-to-nearest store of the tensor may add."""
    m = float(ref64.detach().abs().max())
    return 2.0 ** (math.floor(math.log2(m)) - 8) / m if m > 0 else 0.0


def check(kernel, what, got, ref64, ref32, stored_bf16=False):
    """Hold `got` to the float64 reference; with SRGAN_TEST_LOG set, print kernel, e32, error and bound first."""
    e32, err = rel_err(ref32, ref64), rel_err(got, ref64)
    bound = max(BOUND[what], 8 * e32) + (bf16_store(ref64) if stored_bf16 else 0.0)
    scale = max(float(ref64.abs().max()), 1e-30)
    FIGURES.append((kernel, what, e32, err, bound))
    if os.environ.get("SRGAN_TEST_LOG"):
        print(f"conv {kernel} | {what} | e32 {e32:.3e} err {err:.3e} bound {bound:.3e} err/bound {err / bound:.3f}")
    assert err * scale <= ATOL + bound * scale, f"{kernel} {what}: error {err:.3e} > bound {bound:.3e} (e32 = {e32:.3e})"
