"""The kernels around the conv stack, each against a float64 restatement (tests/heads_ref.py) applied to the device's OWN stored input of
the same forward: dist313_kernel, softmax_nchw_kernel, head_kernel (float and bf16 forms), and glob_branch_kernel with the per-image
Global-Hints shift of conv4_3's epilogue in every kernel family that carries one.  class_logits and pred_313 are fp32 tensors in every
precision, conv10_2 is stored whenever the head is not fused, conv4_3 can be read with and without hints: no bar here depends on the
precision the network ran at, each is the arithmetic error of one small kernel.

Shapes (seeded weights, different images and hint rows per image, every handle max_batch = 3 unless a row says 1):
  A = 40 x 72, n = 3: quarter grid 10 x 18 (not square, 180 pixels: no multiple of a wave), trunk 5 x 9
  B = 16 x 24, n = 2: quarter grid 4 x 6 (most 4 x 4 blocks of the 313 head touch the zero border), trunk 2 x 3
A handle carries every head its precision's cases need (dist, dist313 and global_hints together): a head reads a stored tensor, whatever
else the handle computes.

The shift identity.  The shift is added after the ReLU and the BN affine, so for every image, channel and pixel
    conv4_3 with hints - conv4_3 after clear_global_hints() == g(hints[n])[c] - g(0)[c]
with g the four-stage restatement.  On fp32 storage up to SHIFT_REL_BAR (1 + max|g|); on 16-bit storage up to that plus one storage ulp
of each of the two stored values (split tensors: of their lowest part) -- heads_ref.shift_bar.  Every row first asserts the family of the
kernel conv4_3 launched.  The trunk is 5 x 9 here, so a max_batch = 3 handle plans the same batch-1 families (click, Winograd, kwave) as a
max_batch = 1 handle: the rows the table gives for max_batch 1 run on both, with three images and with one.

Bars (heads_ref.*_BAR, shared with the mutants of test_heads_cpu.py): 4 x the largest error measured on an MI355X over all cases
of the comparison -- two binades for expf / tanhf implementations and summation orders of other ROCm versions.  Every test prints its
figure before it asserts.  Measured maximum -> bar (the issue's cap):
  313 probabilities, relative |p - ref| / (ref + 1e-12)   3.711e-6 (A fp32 S=1; S=0.2: 1.09e-6)  -> P313_REL_BAR  = 1.484e-5 (1e-4)
  pred_ab, absolute on the +-110 scale                     2.490e-4 (A fp32; B: 8.2e-5)            -> PRED_AB_BAR   = 9.96e-4
  529 probabilities, relative                              5.598e-7 (A fp16x3; B: 4.4e-7)          -> P529_REL_BAR  = 2.239e-6 (1e-4)
  head output, absolute at out_mul = 110                   2.030e-5 (A fp32; bf16 form 1.90e-5)    -> HEAD_BAR      = 8.12e-5  (1e-3)
  fp32 shift difference, absolute / (1 + max|g|)           1.334e-6 (A Winograd; the other fp32    -> SHIFT_REL_BAR = 5.336e-6 (1e-4)
                                                           rows 1.333e-6, B split-K 1.07e-6)
On the 16-bit rows the error beyond the two storage ulps stays within the fp32 figure (bf16x6 1.25e-6, fp16x3 1.08e-6, bf16x3 5.6e-7
of 1 + max|g|; bf16 and fp16: none), and the bf16 / fp16 rows measure 0.43 - 0.49 of the two ulps alone: the two round-to-nearest
halves.  max|g| is 400 at shape A (80 at B, which has the first two hint rows), so the fp32 term is 2.1e-3 absolute against storage ulps
of up to 2.0 (bf16), 0.25 (fp16), 7.9e-3 (bf16x3), 1.2e-4 (fp16x3) and 3.1e-5 (bf16x6).
Exact: want_dist=False gives the same pred_ab bits, image 0 of a batch equals the same image alone, probabilities sum to 1 within 529 * 2^-24
(measured 3.4e-7 at most).

Not covered here: the head fused into conv10_2's epilogue ('+head' labels: conv10_2 is never stored; every operand-split forward and the
large-tile bf16 one take it) -- tests/test_fused_head_gpu.py holds it against float64 from the stored conv10_1, one layer earlier; and, on
purpose, the partner tile's shift (conv_igemm_v2 without +m16: -DIDC_AB_PARTNERS builds only).  Every other row of the table is reached by a
shipped configuration.

Wall time of this file on an MI355X: 9.1 s for its 42 cases (16 handles at 40 x 72 and 16 x 24 and the four 256 x 256 census handles);
the slowest case takes 1.8 s (the first one: it draws the weights), every case after the first of a handle a few hundredths of a second.
"""
import re

import numpy as np
import pytest

import heads_ref as hr
from interactive_deep_colorization_amd import engine, workloads
from oracle import weights

pytestmark = pytest.mark.gpu

SUM_BAR = 529 * 2.0 ** -24
SHAPES, MAX_BATCH = hr.SHAPES, hr.MAX_BATCH
HEAD_FLAGS = {                                            # what a handle of each precision carries
    "fp32": dict(dist=True, dist313=True, global_hints=True),
    "bf16": dict(dist=True, global_hints=True),
    "bf16x3": dict(dist313=True, global_hints=True),
    "fp16x3": dict(dist=True, global_hints=True),
    "bf16x6": dict(global_hints=True),
    "fp16": dict(global_hints=True),
}
_OPTION_DEFAULTS = {"op_policy_batch": 0, "winograd": 1, "ds_mfma16": 1, "kwave": 1, "click": -1, "v2p": 1, "fp16_fast": 1, "split_ds_fuse": 1}
_STATE = {}


@pytest.fixture(autouse=True)
def _reset_policies():
    yield
    engine.set_tile_policy("auto")
    engine.set_splitk_policy("auto")
    for name, value in _OPTION_DEFAULTS.items():
        engine.set_option(name, value)


def state_dict():
    """One seeded state dict with every branch: he-style trunk (model_out's gain keeps most pre-tanh sums inside +-2), the Global-Hints
    branch and the 313 head."""
    if "sd" not in _STATE:
        from conftest import state_dict_for
        sd = dict(state_dict_for(hr.WEIGHT_SEED, hr.WEIGHT_STYLE))
        weights.add_global_branch(sd, hr.GLOB_SEED)
        weights.add_pred313_head(sd, hr.PRED_SEED)
        _STATE["sd"] = sd
    return _STATE["sd"]


def _engine(shape, precision, max_batch=MAX_BATCH):
    key = (shape, precision, max_batch)
    if key not in _STATE:
        H, W, _ = SHAPES[shape]
        e = engine.HipColorizer(H, W, max_batch=max_batch, precision=precision, **HEAD_FLAGS[precision])
        e.load_state_dict(state_dict())
        _STATE[key] = e
    e = _STATE[key]
    e.clear_global_hints()
    return e


def _rel(p, ref):
    return float((np.abs(p - ref) / (ref + 1e-12)).max())


def _label(e, name):
    return [r for r in e.layer_table() if r["name"] == name][0]


# ---- 1. dist313_kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [hr.S_DEFAULT, 1.0])
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("shape", ["A", "B"])
def test_dist313(shape, precision, S):
    sd = state_dict()
    e = _engine(shape, precision)
    L, ab, m = hr.images(shape)
    n = L.shape[0]
    centres = sd["pred.pred_ab.weight"][:, :, 0, 0].T
    try:
        e.set_dist_temperature(S)
        _, pred, dist = e.forward_dist313(L, ab, m, 0.0)
        l = e.activation("pred_313", n)
        _, pred_nd, none = e.forward_dist313(L, ab, m, 0.0, want_dist=False)
        _, pred_1, dist_1 = e.forward_dist313(L[:1], ab[:1], m[:1], 0.0)
    finally:
        e.set_dist_temperature(hr.S_DEFAULT)
    ref_d, ref_p = hr.dist313(l, S, centres, sd["pred.pred_ab.bias"])
    assert dist.shape == ref_d.shape and pred.shape == ref_p.shape
    rel, err = _rel(dist, ref_d), float(np.abs(pred - ref_p).max())
    ssum = float(np.abs(dist.sum(axis=1, dtype=np.float64) - 1.0).max())
    print("dist313 %s %s S=%g: p rel %.3e, pred_ab abs %.3e, |sum - 1| %.3e (logits +-%.1f, p from %.1e)" %
          (shape, precision, S, rel, err, ssum, np.abs(l).max(), ref_d.min()))
    assert np.abs(l[0] - l[1]).max() > 1.0                 # the images differ: a wrong image base shows
    assert rel <= hr.P313_REL_BAR
    assert err <= hr.PRED_AB_BAR
    assert ssum <= SUM_BAR
    assert none is None
    np.testing.assert_array_equal(pred_nd, pred)
    np.testing.assert_array_equal(pred_1[0], pred[0])
    np.testing.assert_array_equal(dist_1[0], dist[0])


# ---- 2. softmax_nchw_kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16x3"])
@pytest.mark.parametrize("shape", ["A", "B"])
def test_softmax529(shape, precision):
    e = _engine(shape, precision)
    L, ab, m = hr.images(shape)
    n = L.shape[0]
    _, dq = e.forward_dist(L, ab, m, 0.0)
    l = e.activation("class_logits", n)
    _, dq_1 = e.forward_dist(L[:1], ab[:1], m[:1], 0.0)
    ref = hr.softmax529(l)
    assert dq.shape == ref.shape == (n, 529, L.shape[2] // 4, L.shape[3] // 4)
    rel = _rel(dq, ref)
    ssum = float(np.abs(dq.sum(axis=1, dtype=np.float64) - 1.0).max())
    print("softmax529 %s %s: p rel %.3e, |sum - 1| %.3e (logits +-%.1f, p from %.1e)" % (shape, precision, rel, ssum, np.abs(l).max(), ref.min()))
    assert np.abs(l[0] - l[1]).max() > 1.0
    assert rel <= hr.P529_REL_BAR
    assert ssum <= SUM_BAR
    np.testing.assert_array_equal(dq_1[0], dq[0])


# ---- 3. head_kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,precision,out_mul", [("A", "fp32", 110.0), ("B", "fp32", 110.0), ("A", "bf16", 110.0), ("B", "bf16", 110.0),
                                                     ("A", "fp32", 100.0), ("B", "bf16", 100.0)])
def test_head(shape, precision, out_mul):
    sd = state_dict()
    e = _engine(shape, precision)
    if precision == "bf16":
        engine.set_tile_policy("small")
    L, ab, m = hr.images(shape)
    n = L.shape[0]
    try:
        e.set_io_scales(out_mul=out_mul)
        out = e.forward(L, ab, m, 0.0)
        rows = e.layer_table()
        x = e.activation("conv10_2", n)
        out_1 = e.forward(L[:1], ab[:1], m[:1], 0.0)
    finally:
        e.set_io_scales()
    head_row = [r for r in rows if r["name"] == "head"][0]
    c10 = [r for r in rows if r["name"] == "conv10_2"][0]
    assert head_row["kernel"] == "head_kernel" and head_row["launches"] == 1
    assert "+head" not in c10["kernel"] and c10["launches"] == 1, c10
    ref = hr.head(x, sd["model_out.0.weight"], sd["model_out.0.bias"], out_mul)
    live = float((np.abs(ref) < 0.9 * out_mul).mean())
    err = float(np.abs(out - ref).max())
    print("head %s %s x%g [%s]: abs err %.3e, %.0f %% of the pixels below 0.9 out_mul" % (shape, precision, out_mul, c10["kernel"], err, 100 * live))
    assert live >= 0.5                                    # a saturated tanh hides a wrong sum
    assert np.abs(ref[0] - ref[1]).max() > 1.0 and np.abs(ref[:, 0] - ref[:, 1]).max() > 1.0
    assert err <= hr.HEAD_BAR * out_mul / 110.0
    np.testing.assert_array_equal(out_1[0], out[0])


# ---- 4. glob_branch_kernel and the img_shift epilogues ----------------------------------------------------------------------------------
# id: (shape, precision, max_batch, tile policy, split-K policy, options, family of conv4_3's label)
SHIFT_ROWS = {
    "f32_igemm": ("A", "fp32", 3, "small", "never", (), r"conv_igemm<f32,\d,\d>"),
    "f32_igemm_splitk": ("A", "fp32", 3, "small", "always", (), r"conv_igemm<f32,\d,\d> splitK\d+"),
    "f32_click": ("A", "fp32", 3, "auto", "auto", (("winograd", 0),), r"conv_click<f32,\d,\d>( splitK\d+)?"),
    "f32_click_mb1": ("A", "fp32", 1, "auto", "auto", (("winograd", 0),), r"conv_click<f32,\d,\d>( splitK\d+)?"),
    "f32_wino": ("A", "fp32", 3, "auto", "auto", (), r"conv_wino_f32"),
    "f32_wino_mb1": ("A", "fp32", 1, "auto", "auto", (), r"conv_wino_f32"),
    "bf16_kwave": ("A", "bf16", 3, "auto", "auto", (), r"conv_kwave_bf16"),
    "bf16_kwave_mb1": ("A", "bf16", 1, "auto", "auto", (), r"conv_kwave_bf16"),
    "bf16_igemm": ("A", "bf16", 3, "small", "auto", (), r"conv_igemm<bf16,\d,\d>( splitK\d+)?"),
    "bf16_v2p": ("A", "bf16", 3, "large", "auto", (("v2p", 1),), r"conv_igemm_v2<\d,\d>\+m16p"),
    "bf16_v2m": ("A", "bf16", 3, "large", "auto", (("v2p", 0),), r"conv_igemm_v2<\d,\d>\+m16"),
    "fp16_v2ph": ("A", "fp16", 3, "large", "auto", (), r"conv_igemm_v2ph<\d,\d>"),
    "bf16x3_v2ps": ("A", "bf16x3", 3, "auto", "auto", (), r"conv_igemm_v2ps<\d,\d>x3"),
    "bf16x6_v2ps": ("A", "bf16x6", 3, "auto", "auto", (), r"conv_igemm_v2ps<\d,\d>x6"),
    "fp16x3_v2psh": ("A", "fp16x3", 3, "auto", "auto", (), r"conv_igemm_v2psh<\d,\d>x3"),
    "B_f32_igemm_splitk": ("B", "fp32", 3, "small", "always", (), r"conv_igemm<f32,\d,\d> splitK\d+"),
    "B_bf16_kwave": ("B", "bf16", 3, "auto", "auto", (), r"conv_kwave_bf16"),
    "B_bf16x3_v2ps": ("B", "bf16x3", 3, "auto", "auto", (), r"conv_igemm_v2ps<\d,\d>x3"),
}
SHIFT_FAMILIES = sorted(set(r[6] for r in SHIFT_ROWS.values()))


@pytest.mark.parametrize("row", sorted(SHIFT_ROWS))
def test_shift(row):
    shape, precision, max_batch, tile, splitk, opts, family = SHIFT_ROWS[row]
    sd = state_dict()
    e = _engine(shape, precision, max_batch)
    engine.set_tile_policy(tile)
    engine.set_splitk_policy(splitk)
    for name, value in opts:
        engine.set_option(name, value)
    L, ab, m = hr.images(shape)
    glob, sat = hr.hint_rows()
    # a max_batch = 1 handle takes the LAST image with the last hint row; the others the first n of both
    sel = slice(2, 3) if max_batch == 1 else slice(0, L.shape[0])
    L, ab, m, glob, sat = L[sel], ab[sel], m[sel], glob[sel], sat[sel]
    n = L.shape[0]
    e.set_global_hints(glob, sat)
    e.forward(L, ab, m, 0.0)
    label = _label(e, "conv4_3")
    with_hints = e.activation("conv4_3", n).astype(np.float64)
    e.clear_global_hints()
    e.forward(L, ab, m, 0.0)
    label0 = _label(e, "conv4_3")
    cleared = e.activation("conv4_3", n).astype(np.float64)
    for lb in (label, label0):
        assert lb["launches"] == 1 and re.fullmatch(family, lb["kernel"]), "%s: conv4_3 ran %r, the row expects %s" % (row, lb["kernel"], family)
    assert _label(e, "glob_branch")["kernel"] == "glob_branch_kernel"
    g = hr.glob_branch(sd, glob, sat)
    ref = hr.shift_difference(sd, glob, sat)[:, :, None, None]
    err = np.abs((with_hints - cleared) - ref)
    scale = 1.0 + np.abs(g).max()
    bar = hr.shift_bar(with_hints, cleared, precision, hr.SHIFT_REL_BAR * scale)
    ulps = bar - hr.SHIFT_REL_BAR * scale
    print("shift %s [%s]: max err %.3e; beyond the storage ulps %.3e = %.3e (1 + max|g| = %.1f); worst err / bar %.3f (storage ulps up to %.3e)" %
          (row, label["kernel"], err.max(), (err - ulps).max(), (err - ulps).max() / scale, scale, (err / bar).max(), ulps.max()))
    assert with_hints.shape == (n, 512, SHAPES[shape][0] // 8, SHAPES[shape][1] // 8)
    assert (err <= bar).all(), "worst err / bar %.3f at %s" % ((err / bar).max(), np.unravel_index(np.argmax(err / bar), err.shape))


@pytest.mark.parametrize("max_batch,precision", [(32, "bf16"), (32, "fp16x3"), (1, "bf16"), (1, "fp32")])
def test_shipped_conv4_3_families_are_in_the_table(max_batch, precision):
    """What the shipped 256 x 256 configurations launch for conv4_3 on a Global-Hints handle is a family a row above checks."""
    e = engine.HipColorizer(256, 256, max_batch=max_batch, precision=precision, global_hints=True)
    try:
        e.load_state_dict(state_dict())
        L, ab, m = workloads.random_batch(1, 256, seed=3)
        e.forward(L, ab, m, 0.0)
        label = _label(e, "conv4_3")
    finally:
        e.close()
    assert label["launches"] == 1 and any(re.fullmatch(f, label["kernel"]) for f in SHIFT_FAMILIES), label
