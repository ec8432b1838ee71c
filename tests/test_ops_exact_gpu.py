"""Exact-integer operator tests: every conv template the library ships, at small ragged shapes, bit for bit, with the kernel that ran asserted.

Operands come from the integer lattice of tests/exact_lattice.py, on which bf16, fp16 and fp32 accumulation are exact (on the operand-split
precisions every operand fits its hi part: the lo and mid parts of inputs and weights are ZERO in every row here, so of a split kernel's K
segments only hi.hi is exercised -- tests/test_split_carry_gpu.py holds the others), so a correct kernel gives the same bits whatever its summation order and the comparison is assert_array_equal
against one float64 computation plus the storage rounding of the path.  No tolerance appears in this file.  That sees what the Gaussian
tests (tests/test_ops_gpu.py, 2.5e-2 * (1 + max|ref|) on bf16) cannot: one tap-channel product lost at a tile corner, a halo pixel of the
neighbouring image, a residual added after the rounding, a truncating store (with cin >= 256 many bf16 outputs are odd integers beyond
256: exact ties).

Each case first asserts engine.op_last_kernel() against its expected label: the variant is chosen for the case's POLICY batch
(option op_policy_batch, as a handle's max_batch), the launch carries the small real batch (2 or 3: leakage across images shows).  Shapes
are what the network's levels produce, ragged against the 32- and 16-wide tiles, the 4*wp-row tiles and the 8x8 / 8x16 Winograd blocks.
Where the 512-channel trunk needs 256 workgroups for its shipped 8-wave tile the policy batch is 64 or 128 rather than 32: the spatial
sizes here are a quarter of the network's.  (Occupancy -- the same rows on grids that fill the chip: tests/test_ops_occupancy_gpu.py.)

test_shipped_kernels_are_all_in_the_table builds the shipped configurations and fails when their layer tables name a kernel (template
arguments included) that no case here reaches.  A layer table is filled by a forward's planning pass, so each handle runs ONE single-image
forward (the variant depends on max_batch, not on the images in the call).

The storage rows (out_f32 / resid_f32) run an op as the distribution heads store: the output tensor in fp32, the shortcut sum of a bf16 op in
fp32 (options op_out_f32 / op_resid_f32, set by engine.op_conv2d / op_deconv4x4s2 on every call).  They reach what no 16-bit-output case can:
the fp32 store of every 16-bit kernel's epilogue, the fp32-shortcut read of the bf16 kernels, and conv_igemm<bf16,2,2>, which only fp32-output
layers take.  An fp32 shortcut sum is drawn from [-4099, 4099], and the fp32 outputs hold values bf16 cannot (tests/test_ops_exact_cpu.py).  The
plans of the configurations with a distribution head or global hints are held against the table on the CPU (same file; STORAGE_LAYERS here).

Wall time of this file on an MI355X, as measured there: 5.3 s for its 100 tests (pytest's own figure); the slowest are the four census handles
at 0.1 - 0.8 s, every exact case is below 0.15 s.  With the fifteen small-net rows (`*_click11_*`, `*_14`, `f32_igemm_14_16x264`) and
`bf16x3_v2s_22_halo2_small` it holds 117 tests, 5.9 s as measured there (every new row below 0.14 s).  The <1,4> rows go through the single-operator entry's
64-cout form: conv1_2 as the network runs it (test_a_64_cout_split_op_is_conv1_2_as_the_network_runs_it_or_refused holds its refusing side).
"""
import re

import numpy as np
import pytest

import exact_lattice as xl
from exact_lattice import case
from interactive_deep_colorization_amd import _native, engine

pytestmark = pytest.mark.gpu

_OPTION_DEFAULTS = {"op_policy_batch": 0, "winograd": 1, "ds_mfma16": 1, "kwave": 1, "click": -1, "v2p": 1, "fp16_fast": 1, "split_ds_fuse": 1,
                    "op_out_f32": 0, "op_resid_f32": 0}

CASES = [
    # ---------------------------------------------------------------- fp32: small tile, click, Winograd
    case("f32_igemm_leaky_resid", "conv", "fp32", 3, 64, 128, 20, 36, "conv_igemm<f32,2,1>", act=2, resid=True, tile="small", splitk="never"),
    case("f32_igemm_stride2_splitk", "conv", "fp32", 2, 64, 128, 40, 72, "conv_igemm<f32,2,1> splitK2", in_stride=2, act=1, bn=2.0, tile="small", splitk="always"),
    case("f32_igemm_1x1_529", "conv", "fp32", 2, 256, 529, 8, 16, "conv_igemm<f32,2,1> splitK8", ksize=1),
    case("f32_igemm_deconv", "deconv", "fp32", 2, 128, 128, 20, 36, "conv_igemm<f32,2,1>", tile="small", splitk="never"),
    case("f32_igemm_22_deconv_resid", "deconv", "fp32", 3, 128, 128, 20, 36, "conv_igemm<f32,2,2>", act=1, resid=True, policy=16),
    case("f32_click_d2", "conv", "fp32", 2, 512, 512, 5, 9, "conv_click<f32,1,2> splitK16", dilation=2, act=1, bn=1.0, policy=1, opts=(("winograd", 0),)),
    case("f32_click_leaky_resid", "conv", "fp32", 2, 256, 256, 10, 18, "conv_click<f32,1,4> splitK8", act=2, resid=True, policy=1),
    case("f32_click_deconv", "deconv", "fp32", 2, 128, 128, 20, 36, "conv_click<f32,1,4> splitK4", act=1, resid=True, policy=1),
    case("f32_wino12", "conv", "fp32", 2, 512, 512, 7, 33, "conv_wino_f32", act=1, bn=0.5, wmul=4, opts=(("winograd", 12),), wino="conv"),
    case("f32_wino21_d2", "conv", "fp32", 3, 512, 512, 5, 9, "conv_wino_f32", dilation=2, wmul=4, opts=(("winograd", 21),), wino="conv"),
    case("f32_wino22_stride2_leaky", "conv", "fp32", 3, 64, 128, 40, 72, "conv_wino_f32", in_stride=2, act=2, wmul=4, opts=(("winograd", 22),), wino="conv"),
    case("f32_wino_auto_2x2", "conv", "fp32", 2, 256, 256, 2, 2, "conv_wino_f32", act=1, wmul=4, policy=1, wino="conv"),
    case("f32_wino_auto_1x1px", "conv", "fp32", 3, 512, 512, 1, 1, "conv_wino_f32", dilation=2, act=1, bn=2.0, wmul=4, policy=1, wino="conv"),
    case("f32_wino_deconv", "deconv", "fp32", 2, 512, 256, 5, 9, "conv_wino_deconv_f32", act=1, resid=True, policy=1, wino="deconv"),
    case("f32_wino_deconv_plain", "deconv", "fp32", 3, 256, 128, 10, 18, "conv_wino_deconv_f32", policy=1, wino="deconv"),
    # ---------------------------------------------------------------- bf16: small tile, click, K over the waves
    case("bf16_igemm_leaky_resid", "conv", "bf16", 3, 64, 128, 20, 36, "conv_igemm<bf16,2,1>", act=2, resid=True, tile="small", splitk="never"),
    case("bf16_igemm_splitk", "conv", "bf16", 2, 128, 128, 20, 36, "conv_igemm<bf16,2,1> splitK2", act=1, bn=2.0, tile="small", splitk="always"),
    case("bf16_igemm_1x1_529", "conv", "bf16", 2, 256, 529, 8, 16, "conv_igemm<bf16,2,1> splitK4", ksize=1),
    case("bf16_click_leaky_resid", "conv", "bf16", 2, 256, 256, 10, 18, "conv_click<bf16,1,4> splitK4", act=2, resid=True, policy=1),
    case("bf16_click_d2_resid", "conv", "bf16", 3, 512, 512, 5, 9, "conv_click<bf16,1,2> splitK8", dilation=2, act=1, bn=0.5, resid=True, policy=1),
    case("bf16_click_deconv_1chunk", "deconv", "bf16", 2, 64, 128, 20, 36, "conv_click<bf16,1,4>", act=1, policy=1),
    case("bf16_kwave_1chunk_stride2", "conv", "bf16", 2, 64, 128, 40, 72, "conv_kwave_bf16", in_stride=2, act=1, bn=4.0, policy=1),
    case("bf16_kwave_2chunks", "conv", "bf16", 3, 128, 128, 20, 36, "conv_kwave_bf16", policy=1),
    case("bf16_kwave_4chunks_leaky", "conv", "bf16", 2, 256, 256, 10, 18, "conv_kwave_bf16", act=2, policy=1),
    case("bf16_kwave_4chunks_2x2", "conv", "bf16", 3, 256, 256, 2, 2, "conv_kwave_bf16", act=1, policy=1),
    case("bf16_kwave_8chunks", "conv", "bf16", 2, 512, 512, 7, 33, "conv_kwave_bf16", act=1, bn=1.0, policy=1),
    case("bf16_kwave_8chunks_d2", "conv", "bf16", 3, 512, 512, 5, 9, "conv_kwave_bf16", dilation=2, act=1, policy=1),
    case("bf16_kwave_8chunks_d2_1x1px", "conv", "bf16", 2, 512, 512, 1, 1, "conv_kwave_bf16", dilation=2, act=1, bn=2.0, policy=1),
    case("bf16_kwave_deconv_2chunks", "deconv", "bf16", 2, 128, 128, 20, 36, "conv_kwave_deconv_bf16", act=1, resid=True, policy=1),
    case("bf16_kwave_deconv_4chunks", "deconv", "bf16", 3, 256, 128, 10, 18, "conv_kwave_deconv_bf16", policy=1),
    case("bf16_kwave_deconv_8chunks", "deconv", "bf16", 2, 512, 256, 5, 9, "conv_kwave_deconv_bf16", act=1, resid=True, policy=1),
    # ---------------------------------------------------------------- bf16: the throughput tiles
    case("bf16_v2m_24_deconv", "deconv", "bf16", 2, 256, 128, 10, 18, "conv_igemm_v2<2,4>+m16", act=1, policy=32),
    case("bf16_v2m_42_deconv", "deconv", "bf16", 3, 512, 256, 5, 9, "conv_igemm_v2<4,2>+m16", policy=32),
    case("bf16_v2m_24_1x1_529", "conv", "bf16", 2, 256, 529, 8, 16, "conv_igemm_v2<2,4>+m16", ksize=1, policy=16, tile="large"),
    case("bf16_v2m_22_1x1_529", "conv", "bf16", 3, 256, 529, 8, 16, "conv_igemm_v2<2,2>+m16", ksize=1, act=1, bn=2.0, policy=32),
    case("bf16_v2p_42_halo1", "conv", "bf16", 3, 512, 512, 7, 33, "conv_igemm_v2<4,2>+m16p", act=1, bn=0.5, policy=64),
    case("bf16_v2p_42_halo2", "conv", "bf16", 2, 512, 512, 5, 9, "conv_igemm_v2<4,2>+m16p", dilation=2, act=1, tile="large"),
    case("bf16_v2p_42_256ch", "conv", "bf16", 2, 256, 256, 10, 18, "conv_igemm_v2<4,2>+m16p", policy=128),
    case("bf16_v2p_42_1x1px", "conv", "bf16", 3, 512, 512, 1, 1, "conv_igemm_v2<4,2>+m16p", dilation=2, act=1, bn=2.0, tile="large"),
    case("bf16_v2p_42_2x2", "conv", "bf16", 2, 256, 256, 2, 2, "conv_igemm_v2<4,2>+m16p", act=1, tile="large"),
    case("bf16_v2p_22_half_tiles", "conv", "bf16", 3, 128, 128, 20, 36, "conv_igemm_v2<2,2>+m16p", act=1, policy=32),
    case("bf16_v2p_22_rule22", "conv", "bf16", 3, 64, 128, 40, 72, "conv_igemm_v2<2,2>+m16p", act=1, bn=2.0, policy=32),
    case("bf16_v2p_22_stride2", "conv", "bf16", 2, 64, 128, 40, 72, "conv_igemm_v2<2,2>+m16p", in_stride=2, policy=32),
    case("bf16_v2m_22_halo2", "conv", "bf16", 2, 512, 512, 7, 33, "conv_igemm_v2<2,2>+m16", dilation=2, act=1, policy=32),
    case("bf16_ds_8wave", "fused", "bf16", 2, 512, 256, 5, 9, "conv_ds_fused_m+shortcut 8-wave", cin2=256, act=1, policy=32),
    case("bf16_ds_8wave_256", "fused", "bf16", 3, 256, 128, 10, 18, "conv_ds_fused_m+shortcut 8-wave", cin2=128, policy=32),
    case("bf16_ds_half", "fused", "bf16", 2, 128, 128, 20, 36, "conv_ds_fused_m+shortcut half", cin2=64, act=1, policy=32),
    case("bf16_ds_8wave_forced", "fused", "bf16", 3, 128, 128, 20, 36, "conv_ds_fused_m+shortcut 8-wave", cin2=64, policy=32, opts=(("ds_mfma16", 2),)),
    case("bf16_v2_42_partner", "conv", "bf16", 3, 512, 512, 7, 33, "conv_igemm_v2<4,2>", act=1, policy=64, opts=(("mfma16", 0),), partner=True),
    # ---------------------------------------------------------------- fp16: the twins of the bf16 throughput kernels
    case("fp16_v2ph_42", "conv", "fp16", 3, 512, 512, 7, 33, "conv_igemm_v2ph<4,2>", act=1, bn=0.5, policy=64),
    case("fp16_v2ph_42_halo2", "conv", "fp16", 2, 512, 512, 5, 9, "conv_igemm_v2ph<4,2>", dilation=2, act=1, policy=128),
    case("fp16_v2ph_22", "conv", "fp16", 2, 128, 128, 20, 36, "conv_igemm_v2ph<2,2>", policy=32),
    case("fp16_v2ph_22_stride2", "conv", "fp16", 3, 64, 128, 40, 72, "conv_igemm_v2ph<2,2>", in_stride=2, act=1, bn=2.0, policy=32),
    case("fp16_v2sh_22_halo2_small", "conv", "fp16", 2, 512, 512, 5, 9, "conv_igemm_v2sh<2,2>x1", dilation=2, act=1),
    case("fp16_v2psh_leaky_resid", "conv", "fp16", 2, 256, 256, 10, 18, "conv_igemm_v2psh<2,2>x1", act=2, resid=True),
    case("fp16_v2sh_24_deconv", "deconv", "fp16", 2, 256, 128, 10, 18, "conv_igemm_v2sh<2,4>x1", act=1, resid=True, policy=32),
    case("fp16_ds_half", "fused", "fp16", 2, 128, 128, 20, 36, "conv_ds_fused_mh+shortcut half", cin2=64, act=1, policy=32),
    case("fp16_ds_8wave", "fused", "fp16", 3, 512, 256, 5, 9, "conv_ds_fused_mh+shortcut 8-wave", cin2=256, policy=32),
    # ---------------------------------------------------------------- operand-split precisions
    case("bf16x3_v2ps_42", "conv", "bf16x3", 3, 512, 512, 7, 33, "conv_igemm_v2ps<4,2>x3", act=1, bn=0.5, policy=64),
    case("bf16x6_v2ps_42_leaky", "conv", "bf16x6", 2, 256, 256, 10, 18, "conv_igemm_v2ps<4,2>x6", act=2, policy=128),
    case("fp16x3_v2psh_42_halo2", "conv", "fp16x3", 2, 512, 512, 5, 9, "conv_igemm_v2psh<4,2>x3", dilation=2, act=1, policy=128),
    case("bf16x3_v2ps_22_split_small", "conv", "bf16x3", 2, 128, 128, 20, 36, "conv_igemm_v2ps<2,2>x3", act=1, resid=True),
    case("bf16x6_v2ps_22_split_small_1x1px", "conv", "bf16x6", 3, 512, 512, 1, 1, "conv_igemm_v2ps<2,2>x6", act=1, bn=2.0),
    case("fp16x3_v2psh_22_rule22", "conv", "fp16x3", 2, 64, 128, 40, 72, "conv_igemm_v2psh<2,2>x3", act=1, bn=2.0, policy=32),
    case("bf16x3_v2ps_22_stride2", "conv", "bf16x3", 3, 64, 128, 40, 72, "conv_igemm_v2ps<2,2>x3", in_stride=2, policy=32),
    case("bf16x6_v2s_22_halo2_small", "conv", "bf16x6", 2, 512, 512, 5, 9, "conv_igemm_v2s<2,2>x6", dilation=2, act=2),
    case("fp16x3_v2sh_22_1x1_529", "conv", "fp16x3", 2, 256, 529, 8, 16, "conv_igemm_v2sh<2,2>x3", ksize=1, policy=64),
    case("bf16x3_v2s_24_deconv", "deconv", "bf16x3", 2, 256, 128, 10, 18, "conv_igemm_v2s<2,4>x3", act=1, resid=True, policy=32),
    case("fp16x3_v2sh_24_deconv", "deconv", "fp16x3", 3, 128, 128, 20, 36, "conv_igemm_v2sh<2,4>x3", policy=32),
    case("bf16x6_v2s_42_deconv", "deconv", "bf16x6", 2, 512, 256, 5, 9, "conv_igemm_v2s<4,2>x6", act=1, policy=32),
    case("bf16x3_ds_ms", "fused", "bf16x3", 2, 128, 128, 20, 36, "conv_ds_fused_ms+shortcut x3", cin2=64, act=1, policy=32),
    case("bf16x6_ds_ms", "fused", "bf16x6", 2, 512, 256, 5, 9, "conv_ds_fused_ms+shortcut x6", cin2=256, policy=32),
    case("fp16x3_ds_msh", "fused", "fp16x3", 3, 256, 128, 10, 18, "conv_ds_fused_msh+shortcut x3", cin2=128, act=1, policy=32),
    # ---------------------------------------------------------------- the distribution heads' storage: fp32 outputs, fp32 shortcut sums
    # (class_logits 256 -> 529, conv3_pred 256 -> 384, conv34..34567_pred 512 -> 384 deconvs chained through fp32 sums, conv345678_pred
    # reading one, pred_313 384 -> 313).  The planner keeps fp32-output layers off the bf16 large tile, so these are the only cases on
    # conv_igemm<bf16,2,2>.  wmul=4 on the 1x1 convs: with K = 256 / 384 and weights in [-2, 2] every output would fit bf16.
    case("bf16_f32out_22_1x1_529", "conv", "bf16", 2, 256, 529, 8, 16, "conv_igemm<bf16,2,2>", ksize=1, wmul=4, policy=128, out_f32=True),
    case("bf16_f32out_splitk_1x1_529", "conv", "bf16", 3, 256, 529, 8, 16, "conv_igemm<bf16,2,1> splitK4", ksize=1, wmul=4, policy=1, out_f32=True),
    case("bf16_f32out_22_384", "conv", "bf16", 2, 256, 384, 10, 18, "conv_igemm<bf16,2,2>", policy=64, out_f32=True),
    case("bf16_f32out_kwave_384", "conv", "bf16", 3, 256, 384, 10, 18, "conv_kwave_bf16", policy=1, out_f32=True),
    case("bf16_f32sum_22_deconv_384", "deconv", "bf16", 2, 512, 384, 5, 9, "conv_igemm<bf16,2,2>", resid=True, policy=64, out_f32=True, resid_f32=True),
    case("bf16_f32sum_21_deconv_384", "deconv", "bf16", 3, 512, 384, 5, 9, "conv_igemm<bf16,2,1>", resid=True, policy=32, out_f32=True, resid_f32=True),
    case("bf16_f32sum_kwave_deconv_384", "deconv", "bf16", 2, 512, 384, 5, 9, "conv_kwave_deconv_bf16", resid=True, policy=1, out_f32=True, resid_f32=True),
    case("bf16_f32resid_22_384", "conv", "bf16", 3, 256, 384, 10, 18, "conv_igemm<bf16,2,2>", act=1, resid=True, policy=64, resid_f32=True),
    case("bf16_f32resid_click_384", "conv", "bf16", 2, 256, 384, 10, 18, "conv_click<bf16,1,4> splitK4", act=1, resid=True, policy=1, resid_f32=True),
    case("bf16_f32out_22_1x1_313", "conv", "bf16", 2, 384, 313, 10, 18, "conv_igemm<bf16,2,2>", ksize=1, wmul=4, policy=64, out_f32=True),
    case("bf16_f32out_21_1x1_313", "conv", "bf16", 3, 384, 313, 10, 18, "conv_igemm<bf16,2,1>", ksize=1, wmul=4, splitk="never", out_f32=True),
    case("bf16_f32out_splitk_1x1_313", "conv", "bf16", 2, 384, 313, 10, 18, "conv_igemm<bf16,2,1> splitK3", ksize=1, wmul=4, policy=3, out_f32=True),
    # ... and on the operand-split precisions and fp16 (out_parts == 0 of conv_igemm_v2s / v2ps and their fp16 twins); their shortcut sum is fp32 always
    case("fp16x3_f32out_v2psh_384", "conv", "fp16x3", 2, 256, 384, 10, 18, "conv_igemm_v2psh<2,2>x3", out_f32=True),
    case("fp16x3_f32sum_v2sh_deconv_384", "deconv", "fp16x3", 3, 512, 384, 5, 9, "conv_igemm_v2sh<2,4>x3", resid=True, out_f32=True, resid_f32=True),
    case("fp16x3_f32out_v2sh_1x1_313", "conv", "fp16x3", 2, 384, 313, 10, 18, "conv_igemm_v2sh<2,2>x3", ksize=1, wmul=4, out_f32=True),
    case("bf16x6_f32sum_v2s_deconv_384", "deconv", "bf16x6", 2, 512, 384, 5, 9, "conv_igemm_v2s<2,4>x6", resid=True, out_f32=True, resid_f32=True),
    case("fp16_f32sum_v2sh_deconv_384", "deconv", "fp16", 3, 512, 384, 5, 9, "conv_igemm_v2sh<2,4>x1", resid=True, out_f32=True, resid_f32=True),
    case("bf16x6_f32out_v2s_1x1_313", "conv", "bf16x6", 3, 384, 313, 10, 18, "conv_igemm_v2s<2,2>x6", ksize=1, wmul=4, out_f32=True),
    # (what the census of the flagged configurations asks for besides: conv3_pred and conv345678_pred of the operand-split handles)
    case("bf16x6_f32out_v2ps_384", "conv", "bf16x6", 3, 256, 384, 10, 18, "conv_igemm_v2ps<2,2>x6", out_f32=True),
    case("bf16x6_f32resid_v2ps_384", "conv", "bf16x6", 2, 256, 384, 10, 18, "conv_igemm_v2ps<2,2>x6", act=1, resid=True, resid_f32=True),
    case("fp16x3_f32resid_v2psh_384", "conv", "fp16x3", 3, 256, 384, 10, 18, "conv_igemm_v2psh<2,2>x3", act=1, resid=True, resid_f32=True),
    # ---------------------------------------------------------------- what only small nets reach (the census of tests/test_small_nets_cpu.py)
    # conv_click<T,1,1>, the one-wave form: set_geometry halves wp while 4 * wp > 2 * Hs, so a click launch on at most three site rows takes it
    # (the trunk and conv8_1 of an 8 x 8 or 24 x 24 net without Winograd / kwave; conv345678_pred of a dist313 handle on any net 8 pixels tall).
    # Both HALO instantiations, the deconv form, a width that crosses the 16-wide tile, a halo larger than the image.
    case("f32_click11_d2_1x1px", "conv", "fp32", 3, 512, 512, 1, 1, "conv_click<f32,1,1> splitK16", dilation=2, act=1, bn=2.0, policy=1, opts=(("winograd", 0),)),
    case("f32_click11_3x17", "conv", "fp32", 2, 512, 512, 3, 17, "conv_click<f32,1,1> splitK16", act=1, bn=0.5, policy=1, opts=(("winograd", 0),)),
    case("f32_click11_d2_3x3", "conv", "fp32", 3, 512, 512, 3, 3, "conv_click<f32,1,1> splitK16", dilation=2, act=1, policy=1, opts=(("winograd", 0),)),
    case("f32_click11_deconv_resid", "deconv", "fp32", 2, 128, 128, 2, 17, "conv_click<f32,1,1> splitK4", act=1, resid=True, policy=1),
    case("f32_click11_384_resid", "conv", "fp32", 3, 256, 384, 2, 4, "conv_click<f32,1,1> splitK8", act=1, resid=True, policy=1),
    case("bf16_click11_d2_1x1px", "conv", "bf16", 2, 512, 512, 1, 1, "conv_click<bf16,1,1> splitK8", dilation=2, act=1, bn=2.0, policy=1, opts=(("kwave", 0),)),
    case("bf16_click11_3x17", "conv", "bf16", 3, 512, 512, 3, 17, "conv_click<bf16,1,1> splitK8", act=1, bn=0.5, policy=1, opts=(("kwave", 0),)),
    case("bf16_click11_d2_3x3", "conv", "bf16", 2, 512, 512, 3, 3, "conv_click<bf16,1,1> splitK8", dilation=2, act=1, policy=1, opts=(("kwave", 0),)),
    case("bf16_click11_deconv_resid", "deconv", "bf16", 3, 128, 128, 2, 17, "conv_click<bf16,1,1> splitK2", act=1, resid=True, policy=1, opts=(("kwave", 0),)),
    # (default options: conv345678_pred of a dist313 handle -- a ReLU over an fp32 shortcut sum keeps the layer off kwave and off Winograd)
    case("bf16_click11_f32resid_384", "conv", "bf16", 2, 256, 384, 2, 4, "conv_click<bf16,1,1> splitK4", act=1, resid=True, policy=1, resid_f32=True),
    # the 64-cout <1,4> tile of the operand-split precisions and fp16: conv1_2 wherever its grid stays below conv1_2_split_kernel's 256 workgroups
    case("bf16x3_v2ps_14", "conv", "bf16x3", 3, 64, 64, 20, 36, "conv_igemm_v2ps<1,4>x3", act=1, bn=0.5, policy=1),
    case("bf16x6_v2ps_14", "conv", "bf16x6", 3, 64, 64, 20, 36, "conv_igemm_v2ps<1,4>x6", act=1, bn=1.0, policy=1),
    case("fp16x3_v2psh_14", "conv", "fp16x3", 3, 64, 64, 20, 36, "conv_igemm_v2psh<1,4>x3", act=1, bn=2.0, policy=1),
    case("fp16_v2psh_14", "conv", "fp16", 3, 64, 64, 20, 36, "conv_igemm_v2psh<1,4>x1", act=1, bn=1.0, policy=1),
    # conv_igemm_v2s<2,2>x3: the dilated trunk of a small bf16x3 net (the halo-2 form has no v2ps twin; the x6 and fp16 twins are further up)
    case("bf16x3_v2s_22_halo2_small", "conv", "bf16x3", 2, 512, 512, 5, 9, "conv_igemm_v2s<2,2>x3", dilation=2, act=1),
    # conv_igemm<f32,1,4>: conv1_1 and (without Winograd) conv1_2 of an fp32 max_batch-32 handle on 16 x 264, nine 32-wide tile columns
    case("f32_igemm_14_16x264", "conv", "fp32", 2, 64, 64, 16, 264, "conv_igemm<f32,1,4>", act=1, bn=2.0, policy=32, opts=(("winograd", 0),)),
]
assert len(set(c.id for c in CASES)) == len(CASES)


@pytest.fixture(autouse=True)
def _reset_policies():
    yield
    engine.set_tile_policy("auto")
    engine.set_splitk_policy("auto")
    for name, value in _OPTION_DEFAULTS.items():
        engine.set_option(name, value)


def run_case(c, d):
    """One op call as the case describes it -> (output, the label of the kernel that ran)."""
    engine.set_tile_policy(c.tile)
    engine.set_splitk_policy(c.splitk)
    for name, value in c.opts:
        engine.set_option(name, value)
    if c.op == "conv":
        got = engine.op_conv2d(d["x"], d["w"], d["b"], dilation=c.dilation, in_stride=c.in_stride, act=c.act, bn_scale=d.get("bn_s"),
                               bn_shift=d.get("bn_t"), resid=d.get("resid"), precision=c.precision, policy_batch=c.policy,
                               out_f32=c.out_f32, resid_f32=c.resid_f32)
    elif c.op == "deconv":
        got = engine.op_deconv4x4s2(d["x"], d["w"], d["b"], act=c.act, resid=d.get("resid"), precision=c.precision, policy_batch=c.policy,
                                    out_f32=c.out_f32, resid_f32=c.resid_f32)
    else:
        got = engine.op_deconv_shortcut(d["x"], d["w"], d["b"], d["x2"], d["w2"], d["b2"], act=c.act, precision=c.precision, policy_batch=c.policy)
    return got, engine.op_last_kernel()


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_exact(c):
    if c.partner:
        from conftest import has_ab_partners
        if not has_ab_partners():
            pytest.skip("partner kernel: -DIDC_AB_PARTNERS build only")
    d = xl.draw(c)
    exp = xl.expected(c, d)                      # asserts the lattice bounds and the storage fit before anything runs on the GPU
    got, label = run_case(c, d)
    assert label == c.label, "%s ran %r, the table expects %r" % (c.id, label, c.label)
    xl.compare(got, exp, "%s [%s]" % (c.id, label))


def _by_id(case_id):
    return [c for c in CASES if c.id == case_id][0]


def test_storage_options_do_not_outlive_a_call():
    """The wrappers set op_out_f32 / op_resid_f32 on every call: a 16-bit row run right after a storage row stores 16 bits again."""
    for case_id in ("bf16_f32sum_kwave_deconv_384", "bf16_kwave_deconv_8chunks", "bf16_f32resid_click_384", "bf16_click_leaky_resid"):
        c = _by_id(case_id)
        d = xl.draw(c)
        got, label = run_case(c, d)
        assert label == c.label
        xl.compare(got, xl.expected(c, d), "%s after the row before it" % case_id)


def test_fused_op_refuses_an_fp32_output():
    """The deconv + shortcut launch stores 16-bit outputs only: with op_out_f32 set (past the wrapper, which always clears it) the entry point
    answers IDC_ERR_UNSUPPORTED before it plans anything; cleared, the same call runs."""
    import ctypes
    c = _by_id("bf16_ds_half")
    d = {k: np.ascontiguousarray(v, np.float32) for k, v in xl.draw(c).items()}
    y = np.empty((c.n, c.cout) + xl.out_hw(c), np.float32)
    ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    lib = _native.load()
    engine.set_option("op_policy_batch", c.policy)

    def call():
        return lib.idc_op_deconv_shortcut(0, 1, c.n, c.cin, c.h, c.w, ptr(d["x"]), c.cout, ptr(d["w"]), ptr(d["b"]), c.cin2, ptr(d["x2"]), ptr(d["w2"]),
                                          ptr(d["b2"]), c.act, ptr(y))
    engine.set_option("op_out_f32", 1)
    assert _native.STATUS_NAMES[call()] == "IDC_ERR_UNSUPPORTED" and engine.op_last_kernel() == ""
    engine.set_option("op_out_f32", 0)
    assert call() == 0 and engine.op_last_kernel() == c.label
    xl.compare(y, xl.expected(c), "bf16_ds_half through the C entry point")


def test_a_64_cout_split_op_is_conv1_2_as_the_network_runs_it_or_refused():
    """The single-operator entry runs an operand-split conv of at most 64 couts only in conv1_2's own form (3x3, 64 channels in, dilation 1,
    stride 1, no shortcut sum) and only on the <1,4> tile: anything else of 64 couts is refused before a plan is made, and a policy batch whose
    grid hands conv1_2 to conv1_2_split_kernel (2 x 2 tiles x 64 images = 256 workgroups at 20 x 36) is refused after it, before any launch."""
    c = _by_id("bf16x3_v2ps_14")
    d = xl.draw(c)

    def refused(what, x=d["x"], w=d["w"], policy=c.policy, **kw):
        with pytest.raises(_native.IdcError) as ei:
            engine.op_conv2d(x, w, d["b"], act=c.act, bn_scale=d["bn_s"], bn_shift=d["bn_t"], precision=c.precision, policy_batch=policy, **kw)
        assert _native.STATUS_NAMES[ei.value.status] == "IDC_ERR_UNSUPPORTED" and engine.op_last_kernel() == "", (what, str(ei.value))
        return str(ei.value)

    for precision_row in ("bf16x3_v2ps_14", "fp16_v2psh_14"):
        assert _by_id(precision_row).cin == 64 and _by_id(precision_row).cout == 64
    assert "large tile only" in refused("dilated", dilation=2)
    assert "large tile only" in refused("strided", in_stride=2)
    assert "large tile only" in refused("1x1", w=np.ascontiguousarray(d["w"][:, :, :1, :1]))
    assert "large tile only" in refused("shortcut sum", resid=np.zeros((c.n, c.cout) + xl.out_hw(c), np.float32))
    assert "large tile only" in refused("128 channels in", x=np.concatenate([d["x"], d["x"]], axis=1), w=np.concatenate([d["w"], d["w"]], axis=1))
    assert "conv1_2_split_kernel" in refused("policy batch 64", policy=64)
    got, label = run_case(c, d)                                   # ... and the row itself runs as before
    assert label == c.label
    xl.compare(got, xl.expected(c, d), "%s after the refusals" % c.id)


# ---- census: what the shipped configurations launch is what the table reaches -----------------------------------------------------------
SHIPPED = [(32, "bf16"), (32, "fp16x3"), (1, "bf16"), (1, "fp32")]          # 256 x 256: (max_batch, precision)
# kernels no exact case HERE can reach, each with the test that covers it: model1's kernels start from conv1's input pack (exact through a
# forward: tests/test_model1_exact_gpu.py), the fused head ends in the tanh (tests/test_fused_head_gpu.py), and the persistent trunk chain is a
# launch of several layers
CENSUS_EXCEPTIONS = {
    "conv1_block_fused": "tests/test_model1_exact_gpu.py::test_model1_exact (bit for bit, through a forward; rows *_block_32x12, *_block_32x8)",
    "conv1_1_bf16_kernel": "tests/test_model1_exact_gpu.py::test_model1_exact[bf16_conv1_1_partner]",
    "conv1_1_split_kernel": "tests/test_model1_exact_gpu.py::test_model1_exact (rows *_split_pair)",
    "conv1_2_split_kernel": "tests/test_model1_exact_gpu.py::test_model1_exact (rows *_split_pair)",
    "conv_kwave_chain_bf16": "tests/test_round5_gpu.py::test_kwave_chain_equals_the_eleven_launches (each of its layers is conv_kwave_bf16, 8 chunks: in the table)",
}
CENSUS_EXCEPTION_LAYERS = {
    # conv1_1 outside model1's fused kernels: conv_igemm / conv_click reading the fused input pack (K = 36 im2col), which no op entry stages
    "conv1_1": "tests/test_model1_exact_gpu.py::test_model1_exact (rows fp32_batch1 / 3 / 24, bf16_batch1 / 3, bf16_unfused)",
}


def normalise(label):
    """A label without the suffixes that count slices or name a launch form: ' splitK<n>', ' half', ' 8-wave'."""
    return re.sub(r" (splitK\d+|half|8-wave)$", "", label)


def census_misses(rows, table_labels):
    out = []
    for r in rows:
        k = r["kernel"]
        if r["launches"] <= 0 or not k.startswith("conv") or r["name"] in CENSUS_EXCEPTION_LAYERS:
            continue
        if "+head" in k or k.split("<")[0].split(" ")[0] in CENSUS_EXCEPTIONS:
            continue
        if normalise(k) not in table_labels:
            out.append((r["name"], k))
    return out


# ---- census of the configurations with a distribution head or global hints (run on the CPU from tools/plan_dump: tests/test_ops_exact_cpu.py) ----
# Their fp32-kept layers are matched on storage too: (label, output stored in fp32, shortcut sum read from an fp32 tensor).  The table mirrors the
# out_f32 and resid columns of idc_net.h; every tensor a resid column names there is itself out_f32.
STORAGE_LAYERS = {            # name: (out_f32, has a shortcut sum)
    "class_logits": (True, False), "conv3_pred": (True, False), "conv34_pred": (True, True), "conv345_pred": (True, True),
    "conv3456_pred": (True, True), "conv34567_pred": (True, True), "conv345678_pred": (False, True), "pred_313": (True, False),
}
FLAGGED = [(mb, p, 256, f) for mb, p in SHIPPED for f in ("dist", "dist313", "global_hints")] + [(8, "bf16x6", 256, "dist313"), (8, "bf16", 512, "global_hints")]


def case_storage_key(c):
    """(label, fp32 output tensor, fp32 shortcut-sum tensor) of a case: the fp32 path stores everything so, and only the bf16 path has a
    16-bit shortcut sum."""
    return (normalise(c.label), bool(c.out_f32 or c.precision == "fp32"), bool(c.resid and (c.resid_f32 or c.precision != "bf16")))


def row_storage_key(name, kernel, precision):
    out_f32, resid = STORAGE_LAYERS[name]
    return (normalise(kernel), bool(out_f32 or precision == "fp32"), resid)


def storage_census_misses(rows, precision, cases):
    """census_misses, with the rows of STORAGE_LAYERS held to their storage key as well."""
    cases = [c for c in cases if not c.partner]
    out = census_misses([r for r in rows if r["name"] not in STORAGE_LAYERS], set(normalise(c.label) for c in cases))
    keys = set(case_storage_key(c) for c in cases)
    for r in rows:
        if r["name"] in STORAGE_LAYERS and r["launches"] > 0 and row_storage_key(r["name"], r["kernel"], precision) not in keys:
            out.append((r["name"], r["kernel"]) + row_storage_key(r["name"], r["kernel"], precision)[1:])
    return out


@pytest.mark.parametrize("max_batch,precision", SHIPPED)
def test_shipped_kernels_are_all_in_the_table(make_sd, max_batch, precision):
    from interactive_deep_colorization_amd import workloads
    table_labels = set(normalise(c.label) for c in CASES if not c.partner)
    e = engine.HipColorizer(256, 256, max_batch=max_batch, precision=precision)
    try:
        e.load_state_dict(make_sd(0, "he"))
        L, ab, m = workloads.random_batch(1, 256, seed=3)
        e.forward(L, ab, m, 0.0)                                 # fills the layer table: the planning pass runs with a forward
        rows = e.layer_table()
    finally:
        e.close()
    missing = census_misses(rows, table_labels)
    assert not missing, "shipped kernels no exact case reaches (max_batch %d, %s): %s" % (max_batch, precision, missing)
