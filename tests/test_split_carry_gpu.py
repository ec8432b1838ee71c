"""Exact operator tests of the operand-split precisions whose lo and mid parts are not zero: every split kernel the exact table of
tests/test_ops_exact_gpu.py reaches, bit for bit, on the carry lattice of tests/carry_lattice.py.

In every row of that table the operands fit one bf16 / fp16 part, so every K segment but hi.hi multiplies zeros there: a split kernel that read
weight part 0 for every segment, stepped to the wrong plane of a [part][Cpad] pixel, zero-filled the lo halo differently from the hi halo or
swapped the nibbles of a segment would pass it.  Here one operand carries more bits than a part holds (or both do, where few terms meet in an
output), the expected value is the float64 sum over the KEPT segments of conv(part_i(x), part_j(w)) with the parts built on the CPU by the
library's stated rule, and the comparison is exact_lattice.compare: no tolerance appears in this file.  tests/test_split_carry_cpu.py shows, on
the same rows, that a kernel with a segment dropped or reading part 0 cannot pass, that every split label of CASES has its kinds here, and why
the Gaussian tests of tests/test_round6_gpu.py do not replace this.

CARRY_CASES: for every label CASES reaches in bf16x3, bf16x6 or fp16x3 (computed: SPLIT_LABELS) a row of each kind its precision admits, on
the geometry, policy batch and options of a CASES row with that label.  The comment column holds what carry_lattice.derive gives for the row --
X / Wc / m are typed here and held against it, never tuned against a kernel.  LADDER: the span ladder of the helper's docstring.

Wall time of this file on an MI355X, as measured there: 6.6 s for its 71 tests (pytest's own figure; 5.2 s for the 100 tests of
tests/test_ops_exact_gpu.py in the same run).  The first row takes 0.21 s, every other at most 0.16 s -- about half of it the float64 reference of
the 512-channel rows on the host -- against "below 0.15 s" for that file's exact cases.
With the rows of the <1,4> tile and of conv_igemm_v2s<2,2>x3 it holds 84 tests: 7.0 s as measured there, the slowest row still 0.22 s.
"""
import numpy as np  # noqa: F401
import pytest

import carry_lattice as cl
from test_ops_exact_gpu import CASES, _OPTION_DEFAULTS, run_case
from interactive_deep_colorization_amd import engine

pytestmark = pytest.mark.gpu

SPLIT = ("bf16x3", "bf16x6", "fp16x3")
SPLIT_LABELS = sorted(set((c.label, c.precision) for c in CASES if c.precision in SPLIT))
_BASE = {c.id: c for c in CASES}


def row(base, kind, mag=None, m=0, limit=cl.CARRY_LIMIT, twin=False):
    name = "%s%s.%s" % (base, "_fp16twin" if twin else "", kind) + ("_lim2p%d" % (limit.bit_length() - 1) if kind.startswith("ladder") else "")
    return cl.carry(name, _BASE[base], kind, mag=mag, m=m, limit=limit, twin=twin)


CARRY_CASES = [
    # ---------------------------------------------------------------- bf16x3 (dense rows store fp32)          terms per output; the other operand; budget
    row("bf16x3_v2ps_42", "x_carry", 3639),                          # 512 -> 512 at 7 x 33, BN 0.5: K 4608, w in {-1, 0, 1}, 16777191
    row("bf16x3_v2ps_42", "w_carry", 3639),                          # K 4608, x in [-1, 1]
    row("bf16x3_v2ps_42", "both"),                                   # 9 terms of at most 1023 * 1023
    row("bf16x3_v2ps_22_split_small", "x_carry", 14559),             # 128 -> 128 at 20 x 36 with a residual: K 1152
    row("bf16x3_v2ps_22_split_small", "w_carry", 14559),
    row("bf16x3_v2ps_22_split_small", "both"),
    row("bf16x3_v2ps_22_stride2", "x_carry", 29119),                 # stride 2 at 40 x 72: K 576
    row("bf16x3_v2s_24_deconv", "x_carry", 16351),                   # 2,4 deconv with a residual: K 1024
    row("bf16x3_v2s_24_deconv", "w_carry", 16351),
    row("bf16x3_v2s_24_deconv", "both"),                             # 4 terms
    row("bf16x3_ds_ms", "x_carry", 16351, m=4),                      # fused, 16-bit storage: 4 weights of +-1 per cout, |value| < 2^16
    row("bf16x3_ds_ms", "w_carry", 16351, m=4),                      # (no `both` row: a 10-bit by 10-bit product does not fit 16 stored bits)
    # ---------------------------------------------------------------- fp16x3 (dense rows store fp32; carried operands from 2049)
    row("fp16x3_v2psh_42_halo2", "x_carry", 3638),                   # 512 -> 512 d2 at 5 x 9: K 4608
    row("fp16x3_v2psh_42_halo2", "w_carry", 3638),
    row("fp16x3_v2psh_22_rule22", "x_carry", 14555),                 # 64 -> 128 at 40 x 72, BN 2: K 576, budget 8388595
    row("fp16x3_v2psh_22_rule22", "w_carry", 14555),
    row("fp16x3_v2sh_22_1x1_529", "x_carry", 32767),                 # 256 -> 529 1x1: K 256, X at fp16's cap, 32767 (w in {-1, 0, 1}: [-2, 2] would leave the budget)
    row("fp16x3_v2sh_22_1x1_529", "w_carry", 32767),                 # Wc at the cap, x in [-1, 1]
    row("fp16x3_v2sh_24_deconv", "x_carry", 32759),                  # 2,4 deconv: K 512
    row("fp16x3_v2sh_24_deconv", "w_carry", 32759),
    row("fp16x3_ds_msh", "x_carry", 16363, m=4),                     # fused, 16-bit storage: |value| < 65504
    row("fp16x3_ds_msh", "w_carry", 16363, m=4),
    # ---------------------------------------------------------------- bf16x6 (rows store their three parts: 24 bits)
    row("bf16x6_v2ps_42_leaky", "x_carry", 7279),                    # 256 -> 256 at 10 x 18, LeakyReLU: K 2304
    row("bf16x6_v2ps_42_leaky", "w_carry", 7279),
    row("bf16x6_v2ps_42_leaky", "x_lo", m=15),                       # 15 terms of at most (2^20 - 1) * 1, parts' maxima added
    row("bf16x6_v2ps_42_leaky", "w_lo"),                             # 9 terms
    row("bf16x6_v2ps_42_leaky", "both"),
    row("bf16x6_v2ps_22_split_small_1x1px", "x_carry", 1819),        # 1 x 1 pixel, BN 2: K 4608, budget 8388595 (w_lo / both: 9 * 2^20 is beyond it)
    row("bf16x6_v2ps_22_split_small_1x1px", "w_carry", 1819),
    row("bf16x6_v2ps_22_split_small_1x1px", "x_lo", m=7),
    row("bf16x6_f32out_v2ps_384", "x_carry", 7279),                  # 256 -> 384 at 10 x 18, fp32 output: K 2304
    row("bf16x6_f32out_v2ps_384", "w_carry", 7279),
    row("bf16x6_f32out_v2ps_384", "x_lo", m=15),
    row("bf16x6_f32out_v2ps_384", "w_lo"),
    row("bf16x6_f32out_v2ps_384", "both"),
    row("bf16x6_v2s_22_halo2_small", "x_carry", 3639),               # 512 -> 512 d2 at 5 x 9, LeakyReLU: K 4608
    row("bf16x6_v2s_22_halo2_small", "w_carry", 3639),
    row("bf16x6_v2s_22_halo2_small", "x_lo", m=15),
    row("bf16x6_v2s_22_halo2_small", "w_lo"),
    row("bf16x6_v2s_22_halo2_small", "both"),
    row("bf16x6_v2s_42_deconv", "x_carry", 8175),                    # 4,2 deconv 512 -> 256: K 2048
    row("bf16x6_v2s_42_deconv", "w_carry", 8175),
    row("bf16x6_v2s_42_deconv", "x_lo", m=15),
    row("bf16x6_v2s_42_deconv", "w_lo"),                             # 4 terms
    row("bf16x6_v2s_42_deconv", "both"),
    row("bf16x6_ds_ms", "x_carry", 3848),                            # fused 512 + 256: dense (24 stored bits), K 2048 + 2304
    row("bf16x6_ds_ms", "w_carry", 3848),
    row("bf16x6_ds_ms", "x_lo", m=15),                               # 15 weights per cout over the two tensors together
    row("bf16x6_ds_ms", "w_lo"),                                     # 4 + 9 terms
    row("bf16x6_ds_ms", "both"),
    row("bf16x6_f32sum_v2s_deconv_384", "x_carry", 8175),            # 2,4 deconv 512 -> 384, fp32 output and fp32 shortcut sum in [-4099, 4099]: K 2048
    row("bf16x6_f32sum_v2s_deconv_384", "w_carry", 8175),
    row("bf16x6_f32sum_v2s_deconv_384", "x_lo", m=15),
    row("bf16x6_f32sum_v2s_deconv_384", "w_lo"),
    row("bf16x6_f32sum_v2s_deconv_384", "both"),
    # ---------------------------------------------------------------- the 64-cout <1,4> tile: conv1_2 of a split handle below conv1_2_split_kernel's grid
    row("bf16x3_v2ps_14", "x_carry", 29119),                         # 64 -> 64 at 20 x 36, BN 0.5: K 576
    row("bf16x3_v2ps_14", "w_carry", 29119),
    row("bf16x3_v2ps_14", "both"),
    row("fp16x3_v2psh_14", "x_carry", 14555),                        # BN 2: budget 8388595
    row("fp16x3_v2psh_14", "w_carry", 14555),
    row("bf16x6_v2ps_14", "x_carry", 29119),                         # BN 1
    row("bf16x6_v2ps_14", "w_carry", 29119),
    row("bf16x6_v2ps_14", "x_lo", m=15),
    row("bf16x6_v2ps_14", "w_lo"),
    row("bf16x6_v2ps_14", "both"),
    # ---------------------------------------------------------------- conv_igemm_v2s<2,2>x3: the dilated trunk of a small bf16x3 net
    row("bf16x3_v2s_22_halo2_small", "x_carry", 3639),               # 512 -> 512 d2 at 5 x 9: K 4608
    row("bf16x3_v2s_22_halo2_small", "w_carry", 3639),
    row("bf16x3_v2s_22_halo2_small", "both"),
]
# The span ladder (carry_lattice's docstring): conv_igemm_v2ps<4,2>x3 and its fp16 twin on ONE geometry, sums of one sign reaching the rung
LADDER = [
    row("bf16x3_v2ps_42", "ladder", 56, limit=2 ** 18), row("bf16x3_v2ps_42", "ladder", 227, limit=2 ** 20),
    row("bf16x3_v2ps_42", "ladder", 909, limit=2 ** 22), row("bf16x3_v2ps_42", "ladder", 3639, limit=2 ** 24),
    row("bf16x3_v2ps_42", "ladder_m", 4095, m=63, limit=2 ** 18), row("bf16x3_v2ps_42", "ladder_m", 4095, m=254, limit=2 ** 20),
    row("bf16x3_v2ps_42", "ladder_m", 4095, m=1020, limit=2 ** 22), row("bf16x3_v2ps_42", "ladder_m", 4095, m=4080, limit=2 ** 24),
    row("bf16x3_v2ps_42", "ladder", 56, limit=2 ** 18, twin=True), row("bf16x3_v2ps_42", "ladder", 227, limit=2 ** 20, twin=True),
    row("bf16x3_v2ps_42", "ladder", 910, limit=2 ** 22, twin=True), row("bf16x3_v2ps_42", "ladder", 3638, limit=2 ** 24, twin=True),
    row("bf16x3_v2ps_42", "ladder_m", 4095, m=63, limit=2 ** 18, twin=True), row("bf16x3_v2ps_42", "ladder_m", 4095, m=255, limit=2 ** 20, twin=True),
    row("bf16x3_v2ps_42", "ladder_m", 4095, m=1023, limit=2 ** 22, twin=True), row("bf16x3_v2ps_42", "ladder_m", 4095, m=4093, limit=2 ** 24, twin=True),
]
ALL_ROWS = CARRY_CASES + LADDER
assert len(set(c.id for c in ALL_ROWS)) == len(ALL_ROWS)


@pytest.fixture(autouse=True)
def _reset_policies():
    yield
    engine.set_tile_policy("auto")
    engine.set_splitk_policy("auto")
    for name, value in _OPTION_DEFAULTS.items():
        engine.set_option(name, value)


@pytest.mark.parametrize("c", ALL_ROWS, ids=[c.id for c in ALL_ROWS])
def test_exact(c):
    d = cl.draw(c)
    exp = cl.expected(c, d)                      # asserts the bounds, the zero residue and the storage fit before anything runs on the GPU
    got, label = run_case(c, d)
    assert label == c.label, "%s ran %r, the table expects %r" % (c.id, label, c.label)
    cl.compare(got, exp, "%s [%s]" % (c.id, label))
