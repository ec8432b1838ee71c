"""CPU side of the carry-lattice tests (tests/test_split_carry_gpu.py): every row stays inside its bound and its storage, its carried operand
really has non-zero lo / mid parts, a kernel with a segment dropped or reading part 0 cannot pass it, every operand-split label of the exact
table has its kinds, and the Gaussian tests of tests/test_round6_gpu.py let through what these rows catch.  None of that touches the library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import carry_lattice as cl
import exact_lattice as xl
from test_ops_exact_gpu import CASES
from test_split_carry_gpu import ALL_ROWS, CARRY_CASES, LADDER, SPLIT, SPLIT_LABELS

BASE = {c.id: c for c in CASES}
IDS = lambda c: c.id      # noqa: E731
# kinds a label cannot have, with the reason (carry_lattice's docstring)
NO_ROW = {("conv_ds_fused_ms+shortcut x3", "both"): "16-bit storage, no fp32 output: a 10-bit by 10-bit product does not fit"}


@pytest.fixture(scope="module")
def drawn():
    cache = {}

    def get(c):
        if c.id not in cache:
            cache.clear()                         # (one row's operands at a time)
            cache[c.id] = cl.draw(c)
        return cache[c.id]
    return get


def test_segments_are_the_layout_header_s():
    """kept_segments against the nibbles of split_seg_x / split_seg_w as csrc/idc_layout.h prints them (segment 0 in the low nibble)."""
    for precision, sx, sw in (("bf16x3", 0x001, 0x010), ("fp16x3", 0x001, 0x010), ("bf16x6", 0x001120, 0x010102)):
        names = cl.PART_NAMES[cl.N_PARTS[precision]]
        # the header numbers the parts of x6 hi, mid, lo = 0, 1, 2 and of x3 hi, lo = 0, 1
        got = ["%s.%s" % (names[(sx >> (4 * k)) & 15], names[(sw >> (4 * k)) & 15]) for k in range(len(cl.kept_segments(precision)))]
        assert got == cl.kept_segments(precision) and got[-1] == "hi.hi"


def test_parts_rule():
    v = np.array([257.0, 3599.0, -65535.0, 1048575.0, 1.0, 0.0], np.float32)
    hi, lo = cl.parts(v, "bf16x3")
    np.testing.assert_array_equal(hi, [256.0, 3600.0, -65536.0, 1048576.0, 1.0, 0.0])
    np.testing.assert_array_equal(lo, [1.0, -1.0, 1.0, -1.0, 0.0, 0.0])
    assert all(np.array_equal(sum(p.astype(np.float64) for p in cl.parts(v, p3)), v) for p3 in ("bf16x6",))
    hi, lo = cl.parts(np.array([2049.0, 2048.0, 32767.0, 70000.0], np.float32), "fp16x3")
    np.testing.assert_array_equal(hi, [2048.0, 2048.0, 32768.0, 65504.0])        # (fp16 inputs saturate: X is capped at 32767)
    np.testing.assert_array_equal(lo, [1.0, 0.0, -1.0, 4496.0])
    assert cl.f16_weight_exponent(np.array([1.0])) == 13 and cl.f16_weight_exponent(np.array([3638.0]), np.array([1.0])) == 2
    assert cl.part_maxima(3639, "bf16x3") == [3632.0, 8.0] and cl.part_maxima(1, "fp16x3") == [1.0, 0.0]


@pytest.mark.parametrize("c", ALL_ROWS, ids=IDS)
def test_bounds_hold(c, drawn):
    d = drawn(c)                                  # (asserts that the typed X / Wc / m are what derive() gives)
    acc = cl.assert_bounds(c, d)
    assert acc + cl.extras(c) < c.limit <= cl.CARRY_LIMIT
    b = BASE[c.base]
    assert c.n in (2, 3) and (c.n, c.cin, c.cout, c.h, c.w, c.cin2) == (b.n, b.cin, b.cout, b.h, b.w, b.cin2)      # nothing larger than the row it mirrors
    assert (c.op, c.ksize, c.dilation, c.in_stride, c.act, c.bn, c.resid, c.policy, c.tile, c.splitk, c.opts) == (
        b.op, b.ksize, b.dilation, b.in_stride, b.act, b.bn, b.resid, b.policy, b.tile, b.splitk, b.opts)
    assert c.act != 2 or c.out_f32 or c.precision == "bf16x6"
    exp = cl.expected(c, d)
    assert np.isfinite(exp).all()
    if not c.out_f32:
        assert cl.significant_bits(exp) <= xl.SPLIT_BITS[c.precision]
    if cl.drops_something(c):                     # bf16x3 `both`: the model's value is NOT the exact convolution (lo.lo is dropped)
        assert (exp != xl.store(c, xl.pre_store(c, d))).mean() >= 0.01
    else:                                         # ... everywhere else it is, computed by exact_lattice's own reference
        np.testing.assert_array_equal(exp, xl.store(c, xl.pre_store(c, d)))


@pytest.mark.parametrize("c", [c for c in ALL_ROWS if c.kind != "ladder"], ids=IDS)
def test_the_lowest_carried_part_is_not_zero(c, drawn):
    share = cl.lowest_part_share(c, drawn(c))
    assert share >= 0.25, "%s: only %.0f %% of the carried operand has a non-zero lowest part" % (c.id, 100 * share)


def test_the_dense_ladder_carries_where_its_magnitude_allows():
    """X = limit / K: 56 and 227 fit one bf16 part, 56 .. 910 one fp16 part (the ladder_m rows carry on every rung instead).  Of the integers in
    [X / 2, X] a quarter and more have a non-zero lo part once X >= 1.5 * 2^bits.  The sums of every ladder row reach an eighth of the rung and
    more, BN 0.5 included."""
    for c in LADDER:
        d = cl.draw(c)
        if c.kind == "ladder":
            assert (cl.lowest_part_share(c, d) >= 0.25) == (c.mag >= 1.5 * 2 ** cl.PART_BITS[c.precision]), c.id
        assert np.abs(cl.expected(c, d)).max() * 8 >= c.limit, c.id


def _faults(c):
    out = []
    for name in cl.pinned(c):
        a, b = name.split(".")
        out.append(("drop", name))
        if b != "hi":
            out.append(("wpart0", name))          # (reading weight part 0 for a segment whose weight part IS hi changes nothing)
        if a != "hi":
            out.append(("xpart0", name))
    return out


@pytest.mark.parametrize("c", CARRY_CASES, ids=IDS)
def test_a_wrong_kernel_cannot_pass(c, drawn):
    """A segment left out, or reading part 0 of the weights (of the input), changes at least 1 % of the row's outputs -- among them, in every
    image, outputs on the image border and on both sides of a 32-wide and of a 16-wide tile edge (where the output is that wide)."""
    d = drawn(c)
    exp = cl.expected(c, d)
    wo = exp.shape[3]
    for fault in _faults(c):
        bad = cl.expected(c, d, fault=fault) != exp
        assert bad.mean() >= 0.01, "%s %s: %.2f %% of the outputs differ" % (c.id, fault, 100 * bad.mean())
        px = bad.any(axis=1)                      # (n, H, W)
        for n in range(c.n):
            assert px[n, 0].any() and px[n, -1].any() and px[n, :, 0].any() and px[n, :, -1].any(), "%s %s: image %d, border" % (c.id, fault, n)
            for edge in (16, 32):
                if wo > edge:
                    assert px[n, :, edge - 1].any() and px[n, :, edge].any(), "%s %s: image %d, %d-wide tile edge" % (c.id, fault, n, edge)


def test_every_split_label_has_its_kinds():
    """Census: every label CASES reaches in an operand-split precision has a row of each kind its precision admits, and per label the pinned
    segments are all the kept ones.  Fails when a split row joins CASES without carry rows."""
    assert len(SPLIT_LABELS) == len(set(l for l, _ in SPLIT_LABELS)) == 19, SPLIT_LABELS      # (15 + the <1,4> tile of the three precisions + conv_igemm_v2s<2,2>x3)
    missing = []
    for label, precision in SPLIT_LABELS:
        rows = [c for c in CARRY_CASES if c.label == label and c.precision == precision]
        for kind in cl.KINDS[precision]:
            if not any(c.kind == kind for c in rows) and (label, kind) not in NO_ROW:
                missing.append((label, kind))
        pins = set(s for c in rows for s in cl.pinned(c))
        if pins != set(cl.kept_segments(precision)) or not all("hi.hi" in cl.pinned(c) for c in rows):
            missing.append((label, sorted(set(cl.kept_segments(precision)) - pins)))
    assert not missing, "operand-split labels of CASES without carry rows: %s" % missing
    assert all(c.precision in SPLIT and c.base in BASE and BASE[c.base].label.replace("_v2ps<", "_v2psh<" if c.precision == "fp16x3" else "_v2ps<") == c.label
               for c in ALL_ROWS)
    assert any(c.resid for c in CARRY_CASES) and any(c.bn == 0.5 for c in CARRY_CASES) and any(c.act == 2 for c in CARRY_CASES)
    assert {(c.precision, c.limit) for c in LADDER} == {(p, r) for p in ("bf16x3", "fp16x3") for r in cl.LADDER_RUNGS}
    assert {c.label for c in LADDER} == {"conv_igemm_v2ps<4,2>x3", "conv_igemm_v2psh<4,2>x3"}


# ---- why the Gaussian tests do not replace this ------------------------------------------------------------------------------------------
def _round6_trunk_case():
    """The 512 -> 512 16 x 16 shape and draw of tests/test_round6_gpu.py::test_split_conv, float64 reference included."""
    from test_round6_gpu import CONV_CASES, OP_TOL, _ref_conv
    case = [k for k in CONV_CASES if k[1:5] == (512, 512, 16, 16)][0]
    n, cin, cout, h, w, k, dil, stride, act, bn, has_res = case
    rng = np.random.default_rng(abs(hash(case)) % (2 ** 31))
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32) * 0.1
    bn_s = (0.5 + rng.random(cout)).astype(np.float32)
    bn_t = rng.standard_normal(cout).astype(np.float32) * 0.1
    assert (dil, stride, act, bn, has_res) == (1, 1, 1, True, False)
    return x, wt, b, bn_s, bn_t, _ref_conv(x, wt, b, 1, 1, 1, bn_s, bn_t, None), OP_TOL


def _segment_model(precision, x, wt, b, bn_s, bn_t, drop=None, lose=None):
    """The kept segments in float64 (no accumulation rounding: the kindest case for a faulty kernel), ReLU, BN.  drop: a segment left out;
    lose: (pixel y, x, tap ky, kx, cin) -- ONE lo.hi product missing at one output pixel, for every cout."""
    px, pw = cl.parts(x, precision), cl.parts(wt, precision)
    y = 0.0
    for name in cl.kept_segments(precision):
        if name != drop:
            i, j = cl._seg_index(precision, name)
            y = y + F.conv2d(torch.from_numpy(px[i]).double(), torch.from_numpy(pw[j]).double(), padding=1).numpy()
    if lose is not None:
        oy, ox, ky, kx, ci = lose
        i, j = cl._seg_index(precision, "lo.hi")
        y[0, :, oy, ox] -= pw[j][:, ci, ky, kx].astype(np.float64) * float(px[i][0, ci, oy + ky - 1, ox + kx - 1])
    y = np.maximum(y + b.astype(np.float64)[None, :, None, None], 0.0)
    return y * bn_s.astype(np.float64)[None, :, None, None] + bn_t.astype(np.float64)[None, :, None, None]


def test_the_gaussian_bound_lets_a_dropped_segment_through():
    """bf16x6 without its hi.lo segment, and bf16x3 with one lo product lost at a corner pixel, stay inside OP_TOL * (1 + max|ref|) on the trunk
    shape of test_round6_gpu.py -- while the same faults change the carry rows' bits (test_a_wrong_kernel_cannot_pass)."""
    x, wt, b, bn_s, bn_t, ref, tol = _round6_trunk_case()
    good = np.abs(_segment_model("bf16x6", x, wt, b, bn_s, bn_t) - ref).max()
    bad = np.abs(_segment_model("bf16x6", x, wt, b, bn_s, bn_t, drop="hi.lo") - ref).max()
    bound = tol["bf16x6"] * (1 + np.abs(ref).max())
    assert good < bad <= bound, "bf16x6: %.3e (all six segments), %.3e (hi.lo dropped), bound %.3e" % (good, bad, bound)
    lost = _segment_model("bf16x3", x, wt, b, bn_s, bn_t, lose=(0, 0, 1, 1, 7))
    whole = _segment_model("bf16x3", x, wt, b, bn_s, bn_t)
    assert (lost != whole)[0, :, 0, 0].any() and np.array_equal(lost[0, :, 1:, 1:], whole[0, :, 1:, 1:])
    bad3, bound3 = np.abs(lost - ref).max(), tol["bf16x3"] * (1 + np.abs(ref).max())
    assert bad3 <= bound3 and np.abs(lost - whole).max() < 0.1 * bound3, "bf16x3: %.3e with the product lost, bound %.3e" % (bad3, bound3)
