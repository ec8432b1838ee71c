"""Integer-lattice operands for exact operator tests (tests/test_ops_exact_gpu.py, tests/test_ops_exact_cpu.py).

Operands are small integers (x in [-4, 4], weights in [-2, 2], bias in [-8, 8], residual in [-16, 16] -- in [-4099, 4099] where the case stores
it in fp32 --, BN scale a power of two, BN shift an integer).  Such values are exact in bf16 and in fp16, every product is an integer, and every
partial sum of a K loop stays below 2^24 -- so fp32 accumulation never rounds and EVERY summation order (tile shape, split-K, K split over
waves, segments of a split precision, Winograd transforms) yields the same bits.  The expected output is therefore one exact float64
computation followed by the storage rounding of the path, compared with assert_array_equal: there is no tolerance to tune.
On the operand-split precisions these operands fit the hi part ALONE: the lo and mid parts of inputs and weights are zero on this lattice, and
every K segment but hi.hi multiplies zeros (only the OUTPUT's parts are exercised: expected values need up to 16 or 24 bits).  The segments
themselves are held by tests/carry_lattice.py (tests/test_split_carry_gpu.py, tests/test_model1_carry_gpu.py), whose operands carry into lo and mid.

A helper, not a conftest: nothing here touches the library or a GPU.
"""
import collections

import numpy as np
import torch
import torch.nn.functional as F

X_MAX, W_MAX, B_MAX, R_MAX, BN_SHIFT_MAX = 4, 2, 8, 16, 8
R32_MAX = 4099                        # an fp32-stored residual: most integers up to it need more than bf16's 8 significant bits
BN_SCALES = (0.5, 1.0, 2.0, 4.0)
EXACT_LIMIT = 2 ** 24                 # integers below it are exact in fp32
# significant bits the stored parts of an operand-split output hold for certain: two bf16 parts, three bf16 parts, two fp16 parts
SPLIT_BITS = {"bf16x3": 16, "bf16x6": 24, "fp16x3": 22}
STORAGE = {"fp32": "fp32", "bf16": "bf16", "fp16": "fp16", "bf16x3": "split", "bf16x6": "split", "fp16x3": "split"}

# One row of the table of tests/test_ops_exact_gpu.py.
#   op: "conv" (3x3 or 1x1, `ksize`), "deconv" (4x4 s2), "fused" (deconv of x + 3x3 conv of x_short [n, cin2, 2h, 2w] in one launch)
#   h, w: size of x;  in_stride 2: the conv reads x[:, :, ::2, ::2];  act: 0 none, 1 ReLU, 2 LeakyReLU(0.2);  bn: BN scale or None
#   wmul: weights are wmul * integers in [-2, 2] (4 for the Winograd 3x3 form: its transformed weights carry factors 1/4)
#   policy: batch the variant is chosen for (0 = n);  tile / splitk: the two policies;  opts: idc_set_option pairs;  partner: needs -DIDC_AB_PARTNERS
#   wino: None | "conv" | "deconv" (the Winograd bound applies);  label: what engine.op_last_kernel() must say
#   out_f32: the output tensor is fp32 in every precision (option op_out_f32: class / 313 logits, hyper-column partial sums);  resid_f32: the
#   residual is an fp32 tensor on the bf16 path too (option op_resid_f32) and is drawn from [-R32_MAX, R32_MAX]
Case = collections.namedtuple("Case", "id op precision n cin cout h w ksize dilation in_stride act bn resid cin2 wmul policy tile splitk opts "
                                      "partner wino out_f32 resid_f32 label")


def case(id, op, precision, n, cin, cout, h, w, label, ksize=3, dilation=1, in_stride=1, act=0, bn=None, resid=False, cin2=0, wmul=1,
         policy=0, tile="auto", splitk="auto", opts=(), partner=False, wino=None, out_f32=False, resid_f32=False):
    assert bn is None or bn in BN_SCALES
    assert not resid_f32 or resid, "%s: resid_f32 without a residual" % id
    assert op != "fused" or not (out_f32 or resid_f32), "%s: the fused launch stores 16-bit outputs and reads no stored shortcut sum" % id
    return Case(id, op, precision, n, cin, cout, h, w, ksize, dilation, in_stride, act, bn, resid, cin2, wmul, policy, tile, splitk,
                tuple(opts), partner, wino, bool(out_f32), bool(resid_f32), label)


def resid_max(c):
    """The bound the case's residual is drawn within."""
    return R32_MAX if c.resid_f32 else R_MAX


def out_hw(c):
    return (2 * c.h, 2 * c.w) if c.op in ("deconv", "fused") else (c.h // c.in_stride, c.w // c.in_stride)


def _ints(rs, lo, hi, shape):
    return rs.randint(lo, hi + 1, size=shape).astype(np.float32)


def draw(c):
    """The operands of a case, as float32 arrays holding lattice values (seeded by the case's name)."""
    rs = np.random.RandomState(sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id)) % (2 ** 31))
    ho, wo = out_hw(c)
    d = {"x": _ints(rs, -X_MAX, X_MAX, (c.n, c.cin, c.h, c.w)), "b": _ints(rs, -B_MAX, B_MAX, (c.cout,))}
    if c.op == "conv":
        d["w"] = c.wmul * _ints(rs, -W_MAX, W_MAX, (c.cout, c.cin, c.ksize, c.ksize))
    else:
        d["w"] = c.wmul * _ints(rs, -W_MAX, W_MAX, (c.cin, c.cout, 4, 4))
    if c.op == "fused":
        d["x2"] = _ints(rs, -X_MAX, X_MAX, (c.n, c.cin2, ho, wo))
        d["w2"] = _ints(rs, -W_MAX, W_MAX, (c.cout, c.cin2, 3, 3))
        d["b2"] = _ints(rs, -B_MAX, B_MAX, (c.cout,))
    if c.resid:
        d["resid"] = _ints(rs, -resid_max(c), resid_max(c), (c.n, c.cout, ho, wo))
    if c.bn is not None:
        d["bn_s"] = np.full(c.cout, c.bn, np.float32)
        d["bn_t"] = _ints(rs, -BN_SHIFT_MAX, BN_SHIFT_MAX, (c.cout,))
    return d


def assert_bounds(c, d):
    """No partial sum of any correct kernel can leave the exact range of fp32: asserted from the case's own K, max|x| and max|w| (reference
    side, before anything runs).  Returns the bound on |pre-store value|."""
    mx, mw = float(np.abs(d["x"]).max()), float(np.abs(d["w"]).max())
    for k in ("x", "w", "b"):
        assert np.array_equal(d[k], np.round(d[k])), "%s: %s is not on the integer lattice" % (c.id, k)
    taps = {"conv": c.ksize * c.ksize, "deconv": 4, "fused": 4}[c.op]      # a ConvTranspose 4x4 s2 output pixel sees 2 x 2 taps
    acc = taps * c.cin * mx * mw
    if c.op == "fused":
        acc += 9 * c.cin2 * float(np.abs(d["x2"]).max()) * float(np.abs(d["w2"]).max())
    if c.wino == "conv":
        # F(2x2,3x3): input transform sums 4 pixels, U = G g G^T is bounded by 9/4 max|w| and must be an integer (weights multiples of 4),
        # the output transform sums 3 x 3 of the products' sums
        assert c.op == "conv" and c.ksize == 3 and np.array_equal(d["w"] / 4, np.round(d["w"] / 4)), "%s: Winograd weights must be multiples of 4" % c.id
        acc = max(acc, c.cin * (4 * mx) * (9 * mw / 4) * 9)
    if c.wino == "deconv":
        # F(2x2,2x2) per phase: integer G, |U| <= 4 max|w|, input transform sums 4 pixels, output transform 3 x 3
        acc = max(acc, c.cin * (4 * mx) * (4 * mw) * 9)
    if c.resid:
        assert np.array_equal(d["resid"], np.round(d["resid"])) and np.abs(d["resid"]).max() <= resid_max(c), "%s: residual off its lattice" % c.id
    pre = acc + float(np.abs(d["b"]).max()) + (float(np.abs(d["b2"]).max()) if c.op == "fused" else 0.0) + (resid_max(c) if c.resid else 0.0)
    if c.bn is not None:
        pre = pre * c.bn + BN_SHIFT_MAX
    assert acc < EXACT_LIMIT and pre < EXACT_LIMIT, "%s: worst-case sum %.0f / output %.0f leaves the exact fp32 range" % (c.id, acc, pre)
    return pre


def pre_store(c, d):
    """The value a correct kernel holds before it stores, as float32: conv / conv-transpose (+ shortcut conv), residual, activation, BN.
    Exact in float64; LeakyReLU is ONE float32 multiply by float32(0.2), BN one multiply by a power of two and one add."""
    x, w, b = (torch.from_numpy(d[k]).double() for k in ("x", "w", "b"))
    if c.op == "conv":
        y = F.conv2d(x[:, :, ::c.in_stride, ::c.in_stride], w, b, padding=c.dilation * (c.ksize // 2), dilation=c.dilation)
    else:
        y = F.conv_transpose2d(x, w, b, stride=2, padding=1)
    if c.op == "fused":
        y = y + F.conv2d(torch.from_numpy(d["x2"]).double(), torch.from_numpy(d["w2"]).double(), torch.from_numpy(d["b2"]).double(), padding=1)
    if c.resid:
        y = y + torch.from_numpy(d["resid"]).double()
    y64 = y.numpy()
    assert np.array_equal(y64, np.round(y64)) and np.abs(y64).max() < EXACT_LIMIT, c.id
    v = y64.astype(np.float32)                                     # exact: integers below 2^24
    if c.act == 1:
        v = np.maximum(v, np.float32(0))
    elif c.act == 2:
        v = np.where(v < 0, v * np.float32(0.2), v).astype(np.float32)
    if c.bn is not None:
        v = (v * d["bn_s"][None, :, None, None]).astype(np.float32) + d["bn_t"][None, :, None, None]
    return np.ascontiguousarray(v, np.float32)


def bf16_rne(v):
    """fp32 -> bf16 -> fp32, round to nearest even (the bit formula of tests/test_abi_cpu.py::_bf16_bits = f32_to_bf16_rne in idc_layout.h)."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    r = (((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff).astype(np.uint32) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(v))


def bf16_unrepresentable(v):
    """Fraction of the values of v that bf16 cannot hold (what a kernel that rounds before an fp32 store would change)."""
    v = np.ascontiguousarray(v, np.float32)
    return float((bf16_rne(v) != v).mean())


def bf16_trunc(v):
    """fp32 -> bf16 by dropping the low 16 bits (what a store that forgets to round does)."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32) & np.uint32(0xffff0000)
    return u.view(np.float32).reshape(np.shape(v))


def significant_bits(v):
    """Largest number of significant bits any value of v needs (0 for zeros)."""
    m, _ = np.frexp(np.asarray(v, np.float64))
    m = np.abs(m)
    bits = np.zeros(m.shape, np.int64)
    left = m != 0
    for k in range(1, 54):
        m = m * 2
        m = m - np.floor(m)
        bits[left] = k
        left = left & (m != 0)
        if not left.any():
            break
    return int(bits.max()) if bits.size else 0


def assert_split_fit(c, v):
    """Operand-split storage does not round a value that fits its parts: every expected value must."""
    need, have = significant_bits(v), SPLIT_BITS[c.precision]
    assert need <= have, "%s: an expected value needs %d significant bits, %s stores %d" % (c.id, need, c.precision, have)
    if c.precision == "fp16x3":
        assert np.abs(v).max() < 65504, "%s: |value| beyond fp16's range" % c.id


def store(c, v):
    """The storage rounding of the case's path: none where the output tensor is fp32 (any value below 2^24 fits, split-fit or not)."""
    kind = STORAGE[c.precision]
    if kind == "fp32" or getattr(c, "out_f32", False):      # (tests/model1_ref.py passes its own rows: they carry a precision only)
        return v
    if kind == "bf16":
        return bf16_rne(v)
    if kind == "fp16":
        assert np.abs(v).max() < 65504, "%s: |value| beyond fp16's range" % c.id
        return v.astype(np.float16).astype(np.float32)
    assert_split_fit(c, v)
    return v


def expected(c, d=None):
    d = draw(c) if d is None else d
    assert_bounds(c, d)
    return store(c, pre_store(c, d))


def compare(got, exp, what=""):
    """Bit equality (NaN-free data: array_equal on the values; -0.0 == +0.0 is accepted, a ReLU may produce either).  The message names the
    first mismatch (n, cout, y, x), both values, the count, and where the pixel lies."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, "%s: shape %s, expected %s" % (what, got.shape, exp.shape)
    bad = ~(got == exp)
    if not bad.any():
        np.testing.assert_array_equal(got, exp)
        return
    idx = tuple(int(i) for i in np.argwhere(bad)[0])
    n, co, y, x = idx
    H, W = got.shape[2], got.shape[3]
    where = []
    if y in (0, H - 1) or x in (0, W - 1):
        where.append("image border")
    if x % 32 in (0, 31) or x % 16 in (0, 15):
        where.append("%d-wide tile edge" % (32 if x % 32 in (0, 31) else 16))
    if y % 4 in (0, 3):
        where.append("row-of-4 edge")
    raise AssertionError("%s: %d of %d values differ; first at (n=%d, cout=%d, y=%d, x=%d): got %r, expected %r [%s]; mismatching images %s, "
                         "couts %d..%d" % (what, int(bad.sum()), bad.size, n, co, y, x, float(got[idx]), float(exp[idx]),
                                           ", ".join(where) or "interior", sorted(set(np.argwhere(bad)[:, 0].tolist())),
                                           int(np.argwhere(bad)[:, 1].min()), int(np.argwhere(bad)[:, 1].max())))
