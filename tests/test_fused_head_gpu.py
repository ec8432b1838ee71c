"""The head fused into conv10_2's epilogue ('+head' labels) against a float64 restatement (tests/fused_head_ref.py) applied to the device's
OWN stored conv10_1 of the same forward: conv10_2 (3x3, 128 -> 128, LeakyReLU 0.2) is never stored under the fused head, its input is.
Every operand-split forward and the large-tile bf16 / fp16 forwards take this path; until this file only whole-network parity bounds watched it.

model10.1.weight is bf16_rne of the seeded weights with entries below 2^-12 set to 0 (fused_head_ref.quantise_weights): exact in bf16, in
fp16 and in every part of a split precision, and the stored conv10_1 is exact in its own storage, so each MFMA product is exact and the
kernel's only error is the fp32 accumulation order, the fp32 LeakyReLU, the fp32 128 -> 2 dot product and tanhf.  No bar here depends on
the precision the network ran at.  (bf16x6: the activation getter sums the three stored parts in fp32, hi first, which can round the value
the kernel saw by 2^-24 relative -- 3e-7 on inputs of 5, a few 1e-6 on the +-110 scale after 1152 products: inside the measured figure.)

Shapes (fused_head_ref.SHAPES = heads_ref's, at full resolution here): A = 40 x 72, n = 3 (32+32+8 columns, five 8-row tiles);
B = 16 x 24, n = 2 (smaller than one 32-wide tile).  Rows: fused_head_ref.ROWS -- bf16 and fp16 at max_batch 32 with v2p = 1 and 0 (B in
bf16 needs the "large" tile policy: one tile per image otherwise keeps the batch-1 kernels), the three split precisions with v2p = 1 and 0.
Every row asserts conv10_2's label, that activation("conv10_2") is refused, and on the reference side that at least 90 % of the pre-tanh
sums lie inside +-2 (the tanh cannot hide a wrong sum) and that the images and the two planes differ.

Bar: fused_head_ref.FUSED_HEAD_BAR, absolute on the +-110 scale: 4 x the largest error measured on an MI355X over all rows (heads_ref's
convention: two binades for other ROCm versions' tanhf and summation orders), capped at 1e-3, the stand-alone head's cap.  Every row
prints its figure before it asserts.  Measured maximum -> bar:
  bf16    A m16p 3.775e-5, A m16 3.775e-5, B <2,4> m16 2.804e-5          fp16    A v2ph 4.555e-5, A v2sh 4.845e-5, B v2ph 3.373e-5, B v2sh 3.030e-5
  bf16x3  A 3.427e-5, B 2.504e-5      bf16x6  A 3.858e-5, B 2.173e-5      fp16x3  A 4.690e-5, B 3.423e-5      (v2ps and v2s forms: the same figure)
  largest 4.845e-5 (A_fp16_v2sh)  ->  FUSED_HEAD_BAR = 1.938e-4  (cap 1e-3)
About twice the stand-alone head's 2.03e-5 (tests/test_heads_gpu.py): the 1152-term fp32 sums of conv10_2 and its fp32 LeakyReLU come on top of
the 128-term dot product and tanhf.  In every row all pre-tanh sums lie inside +-2 (largest 1.72).
tests/test_fused_head_cpu.py holds six faults against the cap; the weakest (one product of median size dropped at an image corner) moves
the output by 4.5e-3, the bf16 rounding of conv10_2 before the head by 0.27.

Wall time of this file on an MI355X: 6.0 s for its 23 cases (ten handles at 40 x 72 and 16 x 24, the four 256 x 256 census handles); the
slowest case takes 0.8 s, a row on a handle that exists 0.05 - 0.5 s (most of it the float64 reference).
"""
import re

import numpy as np
import pytest

import fused_head_ref as fh
import heads_ref as hr
from interactive_deep_colorization_amd import _native, engine, workloads

pytestmark = pytest.mark.gpu

_OPTION_DEFAULTS = {"op_policy_batch": 0, "winograd": 1, "ds_mfma16": 1, "kwave": 1, "click": -1, "v2p": 1, "fp16_fast": 1, "split_ds_fuse": 1}
SHIPPED = [(32, "bf16"), (32, "fp16x3"), (1, "bf16"), (1, "fp32")]          # 256 x 256: (max_batch, precision)
_STATE = {}


@pytest.fixture(autouse=True)
def _reset_policies():
    yield
    engine.set_tile_policy("auto")
    engine.set_splitk_policy("auto")
    for name, value in _OPTION_DEFAULTS.items():
        engine.set_option(name, value)


def state_dict():
    if "sd" not in _STATE:
        from conftest import state_dict_for
        _STATE["sd"] = fh.state_dict(state_dict_for(fh.WEIGHT_SEED, fh.WEIGHT_STYLE))
    return _STATE["sd"]


def _engine(shape, precision, max_batch):
    key = (shape, precision, max_batch)
    if key not in _STATE:
        H, W, _ = fh.SHAPES[shape]
        e = engine.HipColorizer(H, W, max_batch=max_batch, precision=precision)
        e.load_state_dict(state_dict())
        _STATE[key] = e
    return _STATE[key]


def _row(e, name):
    return [r for r in e.layer_table() if r["name"] == name][0]


@pytest.mark.parametrize("row", [r.id for r in fh.ROWS])
def test_fused_head(row):
    r = fh.BY_ID[row]
    sd = state_dict()
    e = _engine(r.shape, r.precision, r.max_batch)
    engine.set_tile_policy(r.tile)
    for name, value in r.opts:
        engine.set_option(name, value)
    L, ab, m = hr.images(r.shape)
    n = L.shape[0]
    out = e.forward(L, ab, m, 0.0)
    c10 = _row(e, "conv10_2")
    x = e.activation("conv10_1", n)
    with pytest.raises(_native.IdcError):                    # fused away: never stored
        e.activation("conv10_2", n)
    out_1 = e.forward(L[:1], ab[:1], m[:1], 0.0)
    assert c10["launches"] == 1 and "+head" in c10["kernel"] and c10["kernel"] == r.label, "%s: conv10_2 ran %r, the row expects %r" % (row, c10["kernel"], r.label)
    ref, pre = fh.fused_head(x, sd["model10.1.weight"], sd["model10.1.bias"], sd["model_out.0.weight"], sd["model_out.0.bias"])
    live = float((np.abs(pre) < fh.LIVE_RANGE).mean())
    err = float(np.abs(out - ref).max())
    print("fused head %s [%s]: abs err %.3e (bar %.3e), %.1f %% of the pre-tanh sums inside +-%g, conv10_1 up to %.2f" %
          (row, c10["kernel"], err, fh.FUSED_HEAD_BAR, 100 * live, fh.LIVE_RANGE, np.abs(x).max()))
    assert out.shape == ref.shape == (n, 2) + L.shape[2:]
    assert live >= fh.LIVE_SHARE                              # a saturated tanh hides a wrong sum
    assert np.abs(ref[0] - ref[1]).max() > 1.0 and np.abs(ref[:, 0] - ref[:, 1]).max() > 1.0
    assert err <= fh.FUSED_HEAD_BAR
    np.testing.assert_array_equal(out_1[0], out[0])


@pytest.mark.parametrize("max_batch,precision", SHIPPED)
def test_shipped_head_labels_are_in_the_rows(max_batch, precision):
    """Every '+head' label of the shipped 256 x 256 configurations is one a row above asserted."""
    asserted = set(r.label for r in fh.ROWS)
    e = engine.HipColorizer(256, 256, max_batch=max_batch, precision=precision)
    try:
        e.load_state_dict(state_dict())
        L, ab, m = workloads.random_batch(1, 256, seed=3)
        e.forward(L, ab, m, 0.0)
        heads = [r["kernel"] for r in e.layer_table() if "+head" in r["kernel"] and r["launches"] > 0]
    finally:
        e.close()
    if precision != "fp32":                                   # (the fp32 forward keeps the stand-alone head: tests/test_heads_gpu.py)
        assert heads, "no fused head in the (%d, %s) forward" % (max_batch, precision)
    missing = [k for k in heads if re.sub(r" splitK\d+$", "", k) not in asserted]
    assert not missing, "shipped '+head' kernels no row reaches (max_batch %d, %s): %s" % (max_batch, precision, missing)
