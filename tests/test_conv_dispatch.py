"""CPU: the host queries of the convolution dispatch answer what the launches write.

oct_conv_stat_blocks (BatchNorm partial rows), oct_conv_wgrad_partials (deterministic weight-gradient slabs),
oct_conv_wgrad_fused_apply_ok and oct_conv_wgrad_all_depth_taps_ok are pinned here with literal values, one descriptor
or more per kernel path, with the pipelined kernels on and with OCT_DISABLE_V2=1 (read once per process, so that table
runs in a child process).  A change in these numbers is a change in which kernel a descriptor selects."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32 = 0, 1
PLAIN, S2D = 0, 1        # OctConvDesc.in_mode / OctWgradDesc.dy_mode
D2S = 1                  # OctConvDesc.out_mode

# name -> ConvDesc fields (dtype, n, h, w, c0, c1, cout, taps, xform0, xform1, in_mode, out_mode, split, want_stats,
# kh, kw, depth, out_img_mul, out_img_add)
FWD = {
    "first_f16": (BF, 2, 64, 96, 1, 0, 16, 9, 0, 0, PLAIN, PLAIN, 0, 1, 0, 0, 0, 0, 0),
    "first_f32": (BF, 2, 64, 96, 1, 0, 32, 9, 0, 0, PLAIN, PLAIN, 0, 1, 0, 0, 0, 0, 0),
    "first_f64": (BF, 4, 496, 512, 1, 0, 64, 9, 0, 0, PLAIN, PLAIN, 0, 1, 0, 0, 0, 0, 0),
    "first_f32_ragged": (BF, 2, 60, 100, 1, 0, 32, 9, 0, 0, PLAIN, PLAIN, 0, 1, 0, 0, 0, 0, 0),
    "first_f32_3d": (BF, 8, 64, 64, 1, 0, 32, 9, 0, 0, PLAIN, PLAIN, 0, 1, 0, 0, 4, 0, 0),
    "first_f16_3d": (BF, 8, 64, 64, 1, 0, 16, 9, 0, 0, PLAIN, PLAIN, 0, 1, 0, 0, 4, 0, 0),
    "first_7x3_f32": (BF, 2, 496, 64, 1, 0, 32, 21, 0, 0, PLAIN, PLAIN, 0, 1, 7, 3, 0, 0, 0),
    "first_7x3_f64": (BF, 8, 496, 64, 1, 0, 64, 21, 0, 0, PLAIN, PLAIN, 0, 1, 7, 3, 0, 0, 0),
    "first_7x3_ragged": (BF, 2, 496, 60, 1, 0, 64, 21, 0, 0, PLAIN, PLAIN, 0, 1, 7, 3, 0, 0, 0),
    "roll3d_c32_stats": (BF, 8, 64, 64, 32, 0, 32, 9, 1, 0, PLAIN, PLAIN, 0, 1, 0, 0, 4, 0, 0),
    "roll3d_c64": (BF, 16, 128, 128, 32, 0, 64, 9, 1, 0, PLAIN, PLAIN, 0, 0, 0, 0, 8, 0, 0),
    "roll3d_c64_split": (BF, 8, 64, 64, 32, 0, 64, 9, 1, 0, PLAIN, PLAIN, 32, 1, 0, 0, 4, 0, 0),
    "ig2_3d_c32_nostats": (BF, 8, 64, 64, 32, 0, 32, 9, 1, 0, PLAIN, PLAIN, 0, 0, 0, 0, 4, 0, 0),
    "ig2_3d_c64_in64": (BF, 8, 64, 64, 64, 0, 64, 9, 1, 0, PLAIN, PLAIN, 0, 1, 0, 0, 4, 0, 0),
    "gemm1_d2s": (BF, 2, 64, 128, 256, 0, 512, 1, 1, 0, PLAIN, D2S, 0, 0, 0, 0, 0, 0, 0),
    "gemm1_s2d": (BF, 2, 64, 128, 64, 0, 256, 1, 0, 0, S2D, PLAIN, 0, 0, 0, 0, 0, 0, 0),
    "ig2_1x1_d2s": (BF, 2, 64, 128, 128, 0, 256, 1, 1, 0, PLAIN, D2S, 0, 0, 0, 0, 0, 0, 0),
    "ig2_1x1_s2d": (BF, 2, 64, 128, 32, 0, 64, 1, 0, 0, S2D, PLAIN, 0, 0, 0, 0, 0, 0, 0),
    "ig2_1x1_plain_stats": (BF, 2, 60, 100, 64, 0, 64, 1, 1, 0, PLAIN, PLAIN, 0, 1, 0, 0, 0, 0, 0),
    "ig2_1x1_plain_c32": (BF, 4, 64, 128, 64, 0, 32, 1, 0, 0, PLAIN, PLAIN, 0, 0, 0, 0, 0, 0, 0),
    "ig2_nt32_wres": (BF, 4, 512, 512, 32, 0, 32, 9, 1, 0, PLAIN, PLAIN, 0, 1, 0, 0, 0, 0, 0),
    "ig2_nt32_16row": (BF, 4, 256, 256, 32, 32, 32, 9, 1, 1, PLAIN, PLAIN, 0, 1, 0, 0, 0, 0, 0),
    "ig2_nt32_8row": (BF, 4, 248, 256, 64, 0, 32, 9, 1, 0, PLAIN, PLAIN, 0, 1, 0, 0, 0, 0, 0),
    "ig2_nt64_16row": (BF, 4, 256, 256, 64, 0, 64, 9, 1, 0, PLAIN, PLAIN, 0, 0, 0, 0, 0, 0, 0),
    "ig2_nt64_wres": (BF, 4, 256, 256, 32, 0, 64, 9, 1, 0, PLAIN, PLAIN, 0, 1, 0, 0, 0, 0, 0),
    "ig2_nt64_dma": (BF, 4, 248, 256, 128, 0, 64, 9, 0, 0, PLAIN, PLAIN, 0, 0, 0, 0, 0, 0, 0),
    "ig2_nt128_dma": (BF, 4, 128, 128, 256, 0, 128, 9, 0, 0, PLAIN, PLAIN, 0, 0, 0, 0, 0, 0, 0),
    "ig2_nt128_stats": (BF, 4, 128, 128, 128, 128, 256, 9, 1, 1, PLAIN, PLAIN, 128, 1, 0, 0, 0, 0, 0),
    "ig2_nt64_split32": (BF, 4, 128, 128, 128, 0, 128, 9, 1, 0, PLAIN, PLAIN, 32, 1, 0, 0, 0, 0, 0),
    "ig2_nt32_16row_small": (BF, 1, 64, 64, 32, 32, 32, 9, 1, 1, PLAIN, PLAIN, 0, 1, 0, 0, 0, 0, 0),
    "ig2_nt64_16row_small": (BF, 1, 64, 64, 64, 0, 64, 9, 1, 0, PLAIN, PLAIN, 0, 0, 0, 0, 0, 0, 0),
    "ig2_nt64_split32_small": (BF, 1, 64, 64, 64, 64, 128, 9, 1, 1, PLAIN, PLAIN, 32, 1, 0, 0, 0, 0, 0),
    "ig2_nt128_small": (BF, 1, 64, 64, 128, 0, 256, 9, 1, 0, PLAIN, PLAIN, 0, 1, 0, 0, 0, 0, 0),
    "ig2_ragged": (BF, 3, 60, 100, 64, 0, 64, 9, 1, 0, PLAIN, PLAIN, 0, 1, 0, 0, 0, 0, 0),
    "ig2_7x3_c64": (BF, 8, 496, 64, 64, 0, 64, 21, 1, 0, PLAIN, PLAIN, 0, 1, 7, 3, 0, 0, 0),
    "ig2_7x3_c128": (BF, 8, 496, 64, 64, 64, 128, 21, 1, 1, PLAIN, PLAIN, 0, 1, 7, 3, 0, 0, 0),
    "generic_7x3_rem1": (BF, 8, 497, 64, 64, 0, 64, 21, 1, 0, PLAIN, PLAIN, 0, 1, 7, 3, 0, 0, 0),
    "generic_c16": (BF, 2, 64, 96, 16, 0, 16, 9, 1, 0, PLAIN, PLAIN, 0, 1, 0, 0, 0, 0, 0),
    "generic_f32": (F32, 2, 60, 100, 64, 0, 64, 9, 1, 0, PLAIN, PLAIN, 0, 1, 0, 0, 0, 0, 0),
    "generic_f32_c128": (F32, 2, 64, 96, 64, 0, 128, 1, 1, 0, PLAIN, PLAIN, 0, 1, 0, 0, 0, 0, 0),
}

# name -> WgradDesc fields (dtype, n, h, w, c0, c1, cout, taps, xform0, xform1, dy_mode, kh, kw, depth, in_img_shift,
# dy_img_mul, dy_img_add, partials)
WGRAD = {
    "first_f16": (BF, 2, 64, 96, 1, 0, 16, 9, 0, 0, PLAIN, 0, 0, 0, 0, 0, 0, 1),
    "first_f32": (BF, 2, 64, 96, 1, 0, 32, 9, 0, 0, PLAIN, 0, 0, 0, 0, 0, 0, 1),
    "first_f64": (BF, 4, 496, 512, 1, 0, 64, 9, 0, 0, PLAIN, 0, 0, 0, 0, 0, 0, 1),
    "first_f32_ragged": (BF, 2, 60, 100, 1, 0, 32, 9, 0, 0, PLAIN, 0, 0, 0, 0, 0, 0, 0),
    "first_7x3_f64": (BF, 8, 496, 64, 1, 0, 64, 21, 0, 0, PLAIN, 7, 3, 0, 0, 0, 0, 1),
    "first_3d_all": (BF, 8, 64, 64, 1, 0, 32, 9, 0, 0, PLAIN, 0, 0, 4, 2, 0, 0, 0),
    "first_3d_all_ragged": (BF, 8, 64, 60, 1, 0, 32, 9, 0, 0, PLAIN, 0, 0, 4, 2, 0, 0, 0),
    "first_3d_f16": (BF, 8, 64, 64, 1, 0, 16, 9, 0, 0, PLAIN, 0, 0, 4, 2, 0, 0, 0),
    "first_3d_tap": (BF, 8, 64, 64, 1, 0, 64, 9, 0, 0, PLAIN, 0, 0, 4, -1, 0, 0, 1),
    "w2_3x3_64x64": (BF, 4, 256, 256, 64, 0, 64, 9, 1, 0, PLAIN, 0, 0, 0, 0, 0, 0, 1),
    "w2_3x3_32x32": (BF, 4, 512, 512, 32, 0, 32, 9, 1, 0, PLAIN, 0, 0, 0, 0, 0, 0, 1),
    "w2_3x3_32x64": (BF, 4, 256, 256, 64, 0, 32, 9, 1, 0, PLAIN, 0, 0, 0, 0, 0, 0, 1),
    "w2_3x3_64x32": (BF, 4, 256, 256, 32, 0, 64, 9, 1, 0, PLAIN, 0, 0, 0, 0, 0, 0, 1),
    "w2_3x3_32x64_small": (BF, 1, 64, 64, 64, 0, 32, 9, 1, 0, PLAIN, 0, 0, 0, 0, 0, 0, 1),
    "w2_3x3_32x32_small": (BF, 1, 64, 64, 32, 0, 32, 9, 1, 0, PLAIN, 0, 0, 0, 0, 0, 0, 1),
    "w2_3x3_ragged": (BF, 3, 60, 100, 64, 32, 64, 9, 1, 1, PLAIN, 0, 0, 0, 0, 0, 0, 1),
    "w2_3x3_3d": (BF, 8, 64, 64, 32, 0, 64, 9, 1, 0, PLAIN, 0, 0, 4, 1, 0, 0, 0),
    "w2_1x1_128x128": (BF, 4, 128, 128, 128, 0, 128, 1, 1, 0, PLAIN, 0, 0, 0, 0, 0, 0, 1),
    "w2_1x1_128x64": (BF, 4, 128, 128, 64, 0, 128, 1, 1, 0, PLAIN, 0, 0, 0, 0, 0, 0, 1),
    "w2_1x1_64x64": (BF, 4, 126, 128, 64, 0, 64, 1, 1, 0, PLAIN, 0, 0, 0, 0, 0, 0, 1),
    "w2_1x1_32x32": (BF, 4, 128, 128, 32, 0, 32, 1, 0, 0, PLAIN, 0, 0, 0, 0, 0, 0, 1),
    "w2_1x1_s2d": (BF, 2, 64, 128, 64, 0, 512, 1, 1, 0, S2D, 0, 0, 0, 0, 0, 0, 1),
    "w2_7x3_64": (BF, 8, 496, 64, 64, 0, 64, 21, 1, 0, PLAIN, 7, 3, 0, 0, 0, 0, 0),
    "w2_7x3_64_small": (BF, 1, 64, 64, 64, 0, 64, 21, 1, 0, PLAIN, 7, 3, 0, 0, 0, 0, 0),
    "w2_7x3_128": (BF, 8, 496, 64, 64, 64, 128, 21, 1, 1, PLAIN, 7, 3, 0, 0, 0, 0, 0),
    "generic_7x3_partials": (BF, 8, 496, 64, 64, 0, 64, 21, 1, 0, PLAIN, 7, 3, 0, 0, 0, 0, 1),
    "generic_c16": (BF, 2, 64, 96, 16, 0, 16, 9, 1, 0, PLAIN, 0, 0, 0, 0, 0, 0, 1),
    "generic_f32": (F32, 2, 60, 100, 64, 0, 64, 9, 1, 0, PLAIN, 0, 0, 0, 0, 0, 0, 1),
    "generic_f32_1x1": (F32, 2, 64, 96, 64, 0, 128, 1, 1, 0, PLAIN, 0, 0, 0, 0, 0, 0, 1),
}

# values computed with the library before the dispatch had a single planner
EXPECTED = {
    "fwd/first_f16": 96,
    "fwd/first_f32": 192,
    "fwd/first_f64": 4096,
    "fwd/first_f32_ragged": 188,
    "fwd/first_f32_3d": 512,
    "fwd/first_f16_3d": 256,
    "fwd/first_7x3_f32": 992,
    "fwd/first_7x3_f64": 4096,
    "fwd/first_7x3_ragged": 248,
    "fwd/roll3d_c32_stats": 32,
    "fwd/roll3d_c64": 128,
    "fwd/roll3d_c64_split": 32,
    "fwd/ig2_3d_c32_nostats": 64,
    "fwd/ig2_3d_c64_in64": 64,
    "fwd/gemm1_d2s": 256,
    "fwd/gemm1_s2d": 128,
    "fwd/ig2_1x1_d2s": 128,
    "fwd/ig2_1x1_s2d": 64,
    "fwd/ig2_1x1_plain_stats": 64,
    "fwd/ig2_1x1_plain_c32": 128,
    "fwd/ig2_nt32_wres": 256,
    "fwd/ig2_nt32_16row": 256,
    "fwd/ig2_nt32_8row": 256,
    "fwd/ig2_nt64_16row": 256,
    "fwd/ig2_nt64_wres": 256,
    "fwd/ig2_nt64_dma": 256,
    "fwd/ig2_nt128_dma": 256,
    "fwd/ig2_nt128_stats": 256,
    "fwd/ig2_nt64_split32": 256,
    "fwd/ig2_nt32_16row_small": 8,
    "fwd/ig2_nt64_16row_small": 8,
    "fwd/ig2_nt64_split32_small": 32,
    "fwd/ig2_nt128_small": 32,
    "fwd/ig2_ragged": 96,
    "fwd/ig2_7x3_c64": 256,
    "fwd/ig2_7x3_c128": 256,
    "fwd/generic_7x3_rem1": 1008,
    "fwd/generic_c16": 48,
    "fwd/generic_f32": 64,
    "fwd/generic_f32_c128": 48,
    "wgrad/first_f16": [96, 1, 0],
    "wgrad/first_f32": [192, 1, 0],
    "wgrad/first_f64": [512, 1, 0],
    "wgrad/first_f32_ragged": [188, 1, 0],
    "wgrad/first_7x3_f64": [512, 0, 0],
    "wgrad/first_3d_all": [512, 1, 1],
    "wgrad/first_3d_all_ragged": [480, 1, 0],
    "wgrad/first_3d_f16": [256, 1, 0],
    "wgrad/first_3d_tap": [512, 1, 0],
    "wgrad/w2_3x3_64x64": [256, 0, 0],
    "wgrad/w2_3x3_32x32": [1024, 0, 0],
    "wgrad/w2_3x3_32x64": [512, 0, 0],
    "wgrad/w2_3x3_64x32": [512, 0, 0],
    "wgrad/w2_3x3_32x64_small": [32, 0, 0],
    "wgrad/w2_3x3_32x32_small": [32, 0, 0],
    "wgrad/w2_3x3_ragged": [96, 0, 0],
    "wgrad/w2_3x3_3d": [256, 0, 0],
    "wgrad/w2_1x1_128x128": [256, 0, 0],
    "wgrad/w2_1x1_128x64": [256, 0, 0],
    "wgrad/w2_1x1_64x64": [256, 0, 0],
    "wgrad/w2_1x1_32x32": [1024, 0, 0],
    "wgrad/w2_1x1_s2d": [64, 0, 0],
    "wgrad/w2_7x3_64": [256, 0, 0],
    "wgrad/w2_7x3_64_small": [16, 0, 0],
    "wgrad/w2_7x3_128": [64, 0, 0],
    "wgrad/generic_7x3_partials": [1024, 0, 0],
    "wgrad/generic_c16": [192, 0, 0],
    "wgrad/generic_f32": [256, 0, 0],
    "wgrad/generic_f32_1x1": [192, 0, 0],
}
EXPECTED_NO_V2 = {
    "fwd/first_f16": 48,
    "fwd/first_f32": 48,
    "fwd/first_f64": 3968,
    "fwd/first_f32_ragged": 64,
    "fwd/first_f32_3d": 128,
    "fwd/first_f16_3d": 128,
    "fwd/first_7x3_f32": 248,
    "fwd/first_7x3_f64": 992,
    "fwd/first_7x3_ragged": 248,
    "fwd/roll3d_c32_stats": 128,
    "fwd/roll3d_c64": 1024,
    "fwd/roll3d_c64_split": 128,
    "fwd/ig2_3d_c32_nostats": 128,
    "fwd/ig2_3d_c64_in64": 128,
    "fwd/gemm1_d2s": 64,
    "fwd/gemm1_s2d": 64,
    "fwd/ig2_1x1_d2s": 64,
    "fwd/ig2_1x1_s2d": 64,
    "fwd/ig2_1x1_plain_stats": 64,
    "fwd/ig2_1x1_plain_c32": 128,
    "fwd/ig2_nt32_wres": 4096,
    "fwd/ig2_nt32_16row": 1024,
    "fwd/ig2_nt32_8row": 992,
    "fwd/ig2_nt64_16row": 1024,
    "fwd/ig2_nt64_wres": 1024,
    "fwd/ig2_nt64_dma": 992,
    "fwd/ig2_nt128_dma": 256,
    "fwd/ig2_nt128_stats": 256,
    "fwd/ig2_nt64_split32": 256,
    "fwd/ig2_nt32_16row_small": 16,
    "fwd/ig2_nt64_16row_small": 16,
    "fwd/ig2_nt64_split32_small": 16,
    "fwd/ig2_nt128_small": 16,
    "fwd/ig2_ragged": 96,
    "fwd/ig2_7x3_c64": 992,
    "fwd/ig2_7x3_c128": 992,
    "fwd/generic_7x3_rem1": 1008,
    "fwd/generic_c16": 48,
    "fwd/generic_f32": 64,
    "fwd/generic_f32_c128": 48,
    "wgrad/first_f16": [192, 0, 0],
    "wgrad/first_f32": [192, 0, 0],
    "wgrad/first_f64": [2048, 0, 0],
    "wgrad/first_f32_ragged": [256, 0, 0],
    "wgrad/first_7x3_f64": [2048, 0, 0],
    "wgrad/first_3d_all": [512, 0, 0],
    "wgrad/first_3d_all_ragged": [512, 0, 0],
    "wgrad/first_3d_f16": [512, 0, 0],
    "wgrad/first_3d_tap": [512, 0, 0],
    "wgrad/w2_3x3_64x64": [1024, 0, 0],
    "wgrad/w2_3x3_32x32": [4096, 0, 0],
    "wgrad/w2_3x3_32x64": [2048, 0, 0],
    "wgrad/w2_3x3_64x32": [2048, 0, 0],
    "wgrad/w2_3x3_32x64_small": [64, 0, 0],
    "wgrad/w2_3x3_32x32_small": [64, 0, 0],
    "wgrad/w2_3x3_ragged": [384, 0, 0],
    "wgrad/w2_3x3_3d": [512, 0, 0],
    "wgrad/w2_1x1_128x128": [256, 0, 0],
    "wgrad/w2_1x1_128x64": [512, 0, 0],
    "wgrad/w2_1x1_64x64": [1024, 0, 0],
    "wgrad/w2_1x1_32x32": [1024, 0, 0],
    "wgrad/w2_1x1_s2d": [128, 0, 0],
    "wgrad/w2_7x3_64": [1024, 0, 0],
    "wgrad/w2_7x3_64_small": [64, 0, 0],
    "wgrad/w2_7x3_128": [256, 0, 0],
    "wgrad/generic_7x3_partials": [1024, 0, 0],
    "wgrad/generic_c16": [192, 0, 0],
    "wgrad/generic_f32": [256, 0, 0],
    "wgrad/generic_f32_1x1": [192, 0, 0],
}


def answers():
    """name -> stat rows (forward) / [slabs, fused_apply_ok, all_depth_taps_ok] (weight gradient)"""
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib as L
    lib = L.lib()
    out = {}
    for name, f in FWD.items():
        out["fwd/" + name] = lib.oct_conv_stat_blocks(C.byref(L.ConvDesc(*f)))
    for name, f in WGRAD.items():
        d = L.WgradDesc(*f)
        out["wgrad/" + name] = [lib.oct_conv_wgrad_partials(C.byref(d)), lib.oct_conv_wgrad_fused_apply_ok(C.byref(d)),
                                lib.oct_conv_wgrad_all_depth_taps_ok(C.byref(d))]
    return out


@pytest.fixture(scope="module")
def L():
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    _lib.lib()
    return _lib


def test_queries_pinned(L):
    assert answers() == EXPECTED


def test_queries_pinned_without_v2(L):
    env = dict(os.environ, OCT_DISABLE_V2="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1]) == EXPECTED_NO_V2


def test_partials_slab_mismatch_is_refused(L):
    """A bias gradient moves the first layer's weight gradient to another kernel with another slab count than
    oct_conv_wgrad_partials answered for: the launch is refused before anything runs (the pointers are never read)."""
    d = L.WgradDesc(*WGRAD["first_f64"])   # 512 slabs; the generic kernel would write 2048
    fake = [0x1000 * (i + 1) for i in range(14)]
    a = L.WgradArgs(*fake)
    a.x1 = a.scale0 = a.shift0 = a.scale1 = a.shift1 = None
    a.dy_y = a.dy_coef = a.dy_scale = a.dy_shift = None
    rc = L.lib().oct_conv_wgrad(C.byref(d), C.byref(a), None)
    assert rc == -22
    assert "slab" in L.last_error()


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    print(json.dumps(answers()))
