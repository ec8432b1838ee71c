"""CPU twin of tests/test_model1_carry_gpu.py: the carry rows of model1's split pair stay inside their bounds and storage, W1 / m / Wc are what
the bound gives, conv1_1 (or conv1_2's weights) really need their lo / mid parts, a conv1_2 with a segment dropped or reading part 0 cannot
pass, and model1_ref's new keywords leave every draw of the exact rows bit-identical.  None of that touches the library."""
import hashlib

import numpy as np
import pytest

import carry_lattice as cl
import exact_lattice as xl
import model1_ref as m1
from test_model1_carry_gpu import BY_ID, CARRY_ROWS

STORAGE_LIMIT = {"bf16x3": 2 ** 16, "fp16x3": 65504, "bf16x6": 2 ** 24}      # integers (and halves, counted in halves) below it fit the split storage
IDS = [r.id for r, _ in CARRY_ROWS]


def test_the_exact_rows_draw_what_they_drew():
    """sha256 over model1_tensors of every row of model1_ref.ROWS, taken before the keywords were added."""
    h = hashlib.sha256()
    for r in m1.ROWS:
        t = m1.model1_tensors(r)
        for k in sorted(t):
            h.update(k.encode() + np.ascontiguousarray(t[k]).tobytes())
    assert h.hexdigest() == "8505a445cecea983ab25b1def6524cc4ac9b98214caa83109ade23d1ded5f5d3"


def _fits(precision, scales, m, c1max, wmag):
    """Every conv1_2 value a row can reach, after every BN scale it draws, below the storage's limit (counted in the unit min(scale, 1))."""
    v = m * cl.segment_sum(precision, c1max, wmag) + m1.B2_MAX
    return all((v * s + xl.BN_SHIFT_MAX) / min(s, 1.0) < STORAGE_LIMIT[precision] for s in scales)


@pytest.mark.parametrize("row", IDS)
def test_the_table_is_what_the_bound_gives(row):
    r, kw = BY_ID[row]
    c1 = lambda w1: 36 * m1.K_MAX * w1 + m1.B1_MAX      # noqa: E731
    if kw["w2_mag"] == 1:                         # conv1_1 carries: the largest W1 for the row's m; one more weight per cout would not fit even W1's half
        assert _fits(r.precision, kw["bn_scales"], kw["w2_m"], c1(kw["w1_max"]), 1) and not _fits(r.precision, kw["bn_scales"], kw["w2_m"], c1(kw["w1_max"] + 1), 1) \
            or c1(kw["w1_max"] + 1) > kw["c1_limit"]
        assert c1(kw["w1_max"]) <= kw["c1_limit"]
        # m: the largest that leaves conv1_1 the bits it is here for (bf16x3: 14 bits; fp16x3: beyond 2049 mostly; bf16x6: 20 bits, three parts)
        assert not _fits(r.precision, kw["bn_scales"], kw["w2_m"] + 1, c1(kw["w1_max"]), 1)
    else:                                         # conv1_2's weights carry: the largest Wc for m = 8 and conv1_1 <= 148
        assert kw["w2_m"] == 8 and c1(kw["w1_max"]) == kw["c1_limit"] == 148
        assert _fits(r.precision, kw["bn_scales"], 8, 148, kw["w2_mag"]) and not _fits(r.precision, kw["bn_scales"], 8, 148, kw["w2_mag"] + 1)


@pytest.mark.parametrize("row", IDS)
def test_bounds_storage_and_condition(row):
    r, kw = BY_ID[row]
    exp = m1.expected(r, carry=kw)                # asserts lattice, zero residue, bounds, storage fit
    st = m1._stages(r, kw)
    assert all(np.isfinite(v).all() for v in exp.values())
    assert xl.significant_bits(exp["conv1_1"]) <= xl.SPLIT_BITS[r.precision] and xl.significant_bits(exp["conv1_2"]) <= xl.SPLIT_BITS[r.precision]
    assert (np.abs(st["w2"]) > 0).reshape(64, -1).sum(axis=1).tolist() == [kw["w2_m"]] * 64
    carried = st["c1"].astype(np.float32) if kw["w2_mag"] == 1 else st["w2"].astype(np.float32)
    lowest = cl.parts(carried, r.precision)[2 if (r.precision == "bf16x6" and kw["w2_mag"] == 1) else 1]
    share = float((lowest[carried != 0] != 0).mean())
    assert share >= 0.25, "%s: %.0f %% of the carried operand's non-zero elements have a non-zero lowest part" % (row, 100 * share)
    assert (exp["conv1_2"] > xl.BN_SHIFT_MAX).mean() > 0.05          # conv1_2's ReLU is live on both sides
    assert (st["acc"] < 0).mean() > 0.05


def _conv1_2(r, st, pairs):
    """conv1_2 through the segment model: sum over (input part, weight part) pairs, bias, ReLU, BN -- float32 as model1_ref.expected."""
    p1, p2 = cl.parts(st["c1"].astype(np.float32), r.precision), cl.parts(st["w2"].astype(np.float32), r.precision)
    acc = st["b2"][None, :, None, None] + 0.0
    for i, j in pairs:
        if p1[i].any() and p2[j].any():
            acc = acc + m1._conv3x3(m1._pad(p1[i].astype(np.float64)), p2[j].astype(np.float64))
    v = acc.astype(np.float32)
    return (np.maximum(v, np.float32(0)) * st["scale"][None, :, None, None]).astype(np.float32) + st["shift"][None, :, None, None]


@pytest.mark.parametrize("row", IDS)
def test_a_wrong_conv1_2_cannot_pass(row):
    r, kw = BY_ID[row]
    st = m1._stages(r, kw)
    exp = m1.expected(r, carry=kw)["conv1_2"]
    kept = [cl._seg_index(r.precision, s) for s in cl.kept_segments(r.precision)]
    np.testing.assert_array_equal(_conv1_2(r, st, kept), exp)          # the kept segments ARE the exact computation on these rows
    three = r.precision == "bf16x6"
    pins = (("lo.hi", "mid.hi") if three else ("lo.hi",)) if kw["w2_mag"] == 1 else ("hi.mid",)
    for name in pins + ("hi.hi",):
        i, j = cl._seg_index(r.precision, name)
        variants = [[p for p in kept if p != (i, j)]]
        if (i, j) != (0, 0):
            variants.append([p for p in kept if p != (i, j)] + [(0, j) if i else (i, 0)])      # the segment reads part 0 of its carried operand
        for pairs in variants:
            bad = _conv1_2(r, st, pairs) != exp
            assert bad.mean() >= 0.01, "%s %s: %.2f %%" % (row, name, 100 * bad.mean())
            px = bad.any(axis=1)
            for n in range(m1.N):
                assert px[n, 0].any() and px[n, -1].any() and px[n, :, 0].any() and px[n, :, -1].any(), (row, name, n)
                assert all(px[n, :, x].any() for x in m1.TILE_EDGES_X) and all(px[n, y].any() for y in m1.TILE_EDGES_Y), (row, name, n)
