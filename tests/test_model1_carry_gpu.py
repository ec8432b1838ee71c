"""model1's operand-split pair -- conv1_1_split_kernel + conv1_2_split_kernel x3 / x6 -- bit for bit with conv1_1 values and conv1_2 weights
that need their lo and mid parts.

conv1_2_split_kernel has no single-operator entry (a 64-cout split op is the <1,4> tile or refused); it is reached as tests/test_model1_exact_gpu.py reaches it: a
40 x 72, max_batch 32 forward, reading conv1_1 and conv1_2.  On that file's lattice every conv1_1 value is at most 256 and every weight at
most 2: one part each, so conv1_2's lo / mid segments multiply zeros there.  Here (tests/model1_ref.py, keyword `carry`):
  conv1_1   the exact-fp32 island, integer weights in [-W1, W1]: its post-ReLU values reach 36 * 2 * W1 + 4 and need more than 8 bits (bf16
            parts) or 11 bits (fp16 parts) -- what conv1_1_split_kernel stores as hi + lo (+ lo of three) and conv1_2 reads back
  conv1_2   exactly m weights of +-1 per cout, m the largest for which every conv1_2 value after BN fits the row's split storage (16 significant
            bits; below 65504; 24 bits) for every BN scale the row draws
  *_wcarry  (bf16x6, whose 24 stored bits allow it) conv1_1 as in the exact file (at most 148: one part), conv1_2 m = 8 weights of
            +-[Wc / 2, Wc] per cout: hi.mid.  Weight-side carry on bf16x3 / fp16x3 is LEFT OUT: a 9-bit by 9-bit (12 by 12) product does not fit
            their 16-bit split storage, and conv1_2 has no fp32-output form.
W1, m and Wc follow from the bound (tests/test_model1_carry_cpu.py derives them; none is tuned against a kernel).  One operand of conv1_2 always
fits one part, so the kept segments drop no non-zero product and the expected tensors are model1_ref's exact float64 computation plus the
storage fit.  Labels must still be conv1_1_split_kernel / conv1_2_split_kernel xN.  No tolerance appears in this file.

Wall time of this file on an MI355X, as measured there: 2.8 s for its 4 rows (0.83 s the first handle, 0.45 - 0.53 s the others), beside 7.7 s
for the 20 cases of tests/test_model1_exact_gpu.py and 5.2 s for tests/test_ops_exact_gpu.py in the same run.
"""
import pytest

import exact_lattice as xl
import model1_ref as m1
from interactive_deep_colorization_amd import engine
from test_model1_exact_gpu import _OPTION_DEFAULTS, _labels

pytestmark = pytest.mark.gpu

_PAIR = dict(read=("conv1_1", "conv1_2"), conv1_1="conv1_1_split_kernel")
CARRY_ROWS = [
    # (row, carry keywords)                                                     c1_limit: the largest conv1_1 value the bound allows
    (m1.row("bf16x3_split_pair_carry", "bf16x3", 32, conv1_2="conv1_2_split_kernel x3", w_max=1, **_PAIR),
     dict(w1_max=227, w2_m=2, w2_mag=1, bn_scales=(0.5, 1.0, 2.0), c1_limit=16377)),       # 2 * (2 * c1 + 8) + 8 < 2^16
    (m1.row("fp16x3_split_pair_carry", "fp16x3", 32, conv1_2="conv1_2_split_kernel x3", w_max=1, **_PAIR),
     dict(w1_max=909, w2_m=1, w2_mag=1, bn_scales=(0.5, 1.0), c1_limit=65479)),            # (c1 + 8 + 8 / 0.5) < 65504: no BN scale 2 here
    (m1.row("bf16x6_split_pair_carry", "bf16x6", 32, conv1_2="conv1_2_split_kernel x6", w_max=1, **_PAIR),
     dict(w1_max=77596, w2_m=3, w2_mag=1, bn_scales=(0.5, 1.0), c1_limit=5586916)),          # 3 * c1 + 8 + 8 / 0.5 < 2^24: conv1_1 needs all three parts
    (m1.row("bf16x6_split_pair_wcarry", "bf16x6", 32, conv1_2="conv1_2_split_kernel x6", w_max=2, **_PAIR),
     dict(w1_max=2, w2_m=8, w2_mag=7056, bn_scales=(0.5, 1.0, 2.0), c1_limit=148)),
]
BY_ID = {r.id: (r, kw) for r, kw in CARRY_ROWS}


@pytest.fixture(autouse=True)
def _reset_policies():
    yield
    engine.set_tile_policy("auto")
    engine.set_splitk_policy("auto")
    for name, value in _OPTION_DEFAULTS.items():
        engine.set_option(name, value)


@pytest.mark.parametrize("row", [r.id for r, _ in CARRY_ROWS])
def test_model1_carry(make_sd, row):
    r, kw = BY_ID[row]
    exp = m1.expected(r, carry=kw)               # asserts the lattice, the zero residue, the bounds and the storage fit before anything runs on the GPU
    L, ab, mask, maskcent = m1.planes(r)
    e = engine.HipColorizer(m1.H, m1.W, max_batch=r.max_batch, precision=r.precision)
    try:
        e.load_state_dict(m1.state_dict(r, make_sd(0, "he"), **{k: v for k, v in kw.items() if k != "c1_limit"}))
        e.forward(L, ab, mask, maskcent)
        labels = _labels(e)
        got = {name: e.activation(name, m1.N) for name in r.read}
        e.forward(L[1:2], ab[1:2], mask[1:2], maskcent)
        alone = {name: e.activation(name, 1) for name in r.read}
    finally:
        e.close()
    assert labels == {"conv1_1": (r.conv1_1, 1), "conv1_2": (r.conv1_2, 1)}, "%s ran %r" % (row, labels)
    for name in r.read:
        xl.compare(got[name], exp[name], "%s %s [%s]" % (row, name, labels[name][0]))
    for name in r.read:
        xl.compare(alone[name], got[name][1:2], "%s %s: image 1 alone against image 1 of three" % (row, name))
