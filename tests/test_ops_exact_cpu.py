"""CPU side of the exact-integer operator tests (tests/test_ops_exact_gpu.py): the lattice keeps every row of the table inside the exact range
of fp32 and inside its split storage, and the exact comparison flags three faults the Gaussian tests' tolerance lets through.  Nothing here
touches the library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_lattice as xl
from test_ops_exact_gpu import CASES, CENSUS_EXCEPTIONS, census_misses, normalise

BF16_TOL = 2.5e-2            # tests/test_ops_gpu.py: |err| <= 2.5e-2 * (1 + max|ref|) on the bf16 path


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_lattice_bounds_hold(c):
    d = xl.draw(c)
    pre = xl.assert_bounds(c, d)
    assert pre < xl.EXACT_LIMIT
    assert c.n in (2, 3) and max(v.size for k, v in d.items() if k in ("x", "x2")) <= 3 * 64 * 40 * 72      # batch 2 or 3, nothing beyond 3 x 64 x 40 x 72
    assert np.abs(d["x"]).max() <= xl.X_MAX and np.abs(d["w"]).max() <= xl.W_MAX * c.wmul and np.abs(d["b"]).max() <= xl.B_MAX


@pytest.mark.parametrize("c", [c for c in CASES if xl.STORAGE[c.precision] in ("split", "fp16")], ids=lambda c: c.id)
def test_split_storage_holds_every_expected_value(c):
    exp = xl.expected(c)                         # asserts the fit (16 / 24 / 22 significant bits) and fp16's range
    assert np.isfinite(exp).all()
    if xl.STORAGE[c.precision] == "split":
        assert xl.significant_bits(exp) <= xl.SPLIT_BITS[c.precision]


def test_significant_bits():
    assert xl.significant_bits(np.array([0.0, 1.0, 3.0, 257.0, -0.5])) == 9
    assert xl.significant_bits(np.array([np.float32(0.2)], np.float32)) == 24
    assert xl.significant_bits(np.array([65535.0])) == 16 and xl.significant_bits(np.array([65537.0])) == 17


def test_bf16_rounding_formulas():
    v = np.array([257.0, 259.0, 258.0, -257.0, -259.0, 1.0, 0.0, 511.0], np.float32)      # odd integers beyond 256 are exact ties
    np.testing.assert_array_equal(xl.bf16_rne(v), np.array([256.0, 260.0, 258.0, -256.0, -260.0, 1.0, 0.0, 512.0], np.float32))
    np.testing.assert_array_equal(xl.bf16_trunc(v), np.array([256.0, 258.0, 258.0, -256.0, -258.0, 1.0, 0.0, 510.0], np.float32))


def test_census_filter():
    labels = {normalise("conv_igemm<bf16,2,1> splitK4"), normalise("conv_ds_fused_m+shortcut half")}
    rows = [dict(name="conv2_1", kernel="conv_igemm<bf16,2,1> splitK2", launches=1), dict(name="conv10_1", kernel="conv_ds_fused_m+shortcut", launches=1),
            dict(name="conv10_2", kernel="conv_igemm_v2<2,2>+m16p+head", launches=1), dict(name="conv1_1", kernel="conv1_block_fused", launches=1),
            dict(name="conv1_2", kernel="fused into conv1_1", launches=0), dict(name="conv3_1", kernel="conv_igemm<bf16,2,2>", launches=1)]
    assert census_misses(rows, labels) == [("conv3_1", "conv_igemm<bf16,2,2>")]
    assert "conv1_block_fused" in CENSUS_EXCEPTIONS


# ---- the checker sees what the tolerance does not -----------------------------------------------------------------------------------------
def _operands(kind):
    """64 -> 128, 20 x 36, three images: lattice data or the Gaussian data of tests/test_ops_gpu.py."""
    rs = np.random.RandomState(5)
    n, cin, cout, h, w = 3, 64, 128, 20, 36
    if kind == "lattice":
        x = rs.randint(-xl.X_MAX, xl.X_MAX + 1, (n, cin, h, w)).astype(np.float32)
        wt = rs.randint(-xl.W_MAX, xl.W_MAX + 1, (cout, cin, 3, 3)).astype(np.float32)
        b = rs.randint(-xl.B_MAX, xl.B_MAX + 1, cout).astype(np.float32)
    else:
        x = rs.standard_normal((n, cin, h, w)).astype(np.float32)
        wt = (rs.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32)
        b = rs.uniform(-0.5, 0.5, cout).astype(np.float32)
    return x, wt, b


def _conv64(x, wt, b):
    return F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), torch.from_numpy(b).double(), padding=1).numpy()


def _perturbed(x, wt, b):
    """The bf16-stored result of a correct kernel and of three wrong ones."""
    y = _conv64(x, wt, b)
    good = xl.bf16_rne(y.astype(np.float32))
    # 1. one tap-channel product dropped at a corner pixel: output (n 1, cout 7, y 0, x 35) loses x[1, 3, 0, 34] * w[7, 3, 1, 0]
    drop = y.copy()
    prod = float(x[1, 3, 0, 34]) * float(wt[7, 3, 1, 0])
    drop[1, 7, 0, 35] -= prod
    # 2. a border pixel whose lower halo row comes from the NEXT image instead of the zero padding: (n 0, cout 9, y 19, x 5) gains
    #    sum over cin, kx of x[1, ci, 0, 4 + kx] * w[9, ci, 2, kx]
    leak = y.copy()
    extra = float((x[1, :, 0, 4:7].astype(np.float64) * wt[9, :, 2, :].astype(np.float64)).sum())
    leak[0, 9, 19, 5] += extra
    return y, good, xl.bf16_rne(drop.astype(np.float32)), xl.bf16_rne(leak.astype(np.float32)), xl.bf16_trunc(y.astype(np.float32)), prod, extra


def _old_check_passes(got, ref):
    return bool(np.abs(got - ref).max() <= BF16_TOL * (1 + np.abs(ref).max()))


def test_exact_comparison_flags_what_the_tolerance_lets_through():
    x, wt, b = _operands("lattice")
    while x[1, 3, 0, 34] == 0 or wt[7, 3, 1, 0] == 0:            # the dropped product must be a non-zero one
        x[1, 3, 0, 34] += 1; wt[7, 3, 1, 0] += 1
    y, good, drop, leak, trunc, prod, extra = _perturbed(x, wt, b)
    assert prod != 0 and extra != 0
    xl.compare(good, xl.bf16_rne(y.astype(np.float32)), "unperturbed")
    for name, bad, where in (("dropped product", drop, "(n=1, cout=7, y=0, x=35)"), ("neighbour's halo", leak, "(n=0, cout=9, y=19, x=5)"), ("truncating store", trunc, None)):
        with pytest.raises(AssertionError) as ei:
            xl.compare(bad, good, name)
        msg = str(ei.value)
        assert "values differ" in msg and "got" in msg and "expected" in msg, msg
        if where:
            assert where in msg and "1 of" in msg and "image border" in msg, msg
    # the same three faults on the Gaussian data, under the bound the operator tests used so far: the dropped product and the truncation pass
    gx, gw, gb = _operands("gaussian")
    gy, ggood, gdrop, gleak, gtrunc, gprod, gextra = _perturbed(gx, gw, gb)
    assert gprod != 0 and not np.array_equal(gdrop, ggood) and not np.array_equal(gtrunc, ggood)
    assert _old_check_passes(ggood, gy)
    assert _old_check_passes(gdrop, gy), "a dropped tap-channel product is inside 2.5e-2 * (1 + max|ref|)"
    assert _old_check_passes(gtrunc, gy), "a truncating bf16 store is inside 2.5e-2 * (1 + max|ref|)"
