"""Carry-lattice operands: exact operator tests of the operand-split precisions whose lo and mid parts are NOT zero
(tests/test_split_carry_gpu.py, tests/test_split_carry_cpu.py).

On the lattice of tests/exact_lattice.py every operand fits one bf16 / fp16 part, so in an exact row of bf16x3, bf16x6 or fp16x3 every K
segment but hi.hi multiplies zeros.  Exactness does not need small operands, though: it needs every product of a KEPT segment to be a
multiple of one unit (here 1: all parts of an integer are integers) and every partial sum to stay below 2^24 units.  So one operand may
carry more significant bits than a part holds while the other stays within one part (dense rows), or both may carry where few terms meet
in an output (sparse rows).

expected = store( epilogue( sum over the kept segments (i, j) of conv(part_i(x), part_j(w)) + bias [+ resid] ) ), in float64, where
  parts     part 0 = rne(v), part 1 = rne(v - part 0), part 2 = rne(v - part 0 - part 1), rne = bf16 / fp16 round-to-nearest-even
            (nchw_to_split_kernel for tensors, put_w for weights; fp16x3 weights are first multiplied by 2^s of f16_weight_exponent, a power of
            two that leaves the bits of the parts unchanged; fp16 inputs are clamped at 65504, so X <= 32767 there)
  segments  (input part, weight part), as the comment of split_seg_x / split_seg_w in csrc/idc_layout.h lists them: x3 and fp16x3 keep lo.hi,
            hi.lo, hi.hi; x6 keeps hi.lo, lo.hi, mid.mid, mid.hi, hi.mid, hi.hi.  Everything else is DROPPED by the model (lo.lo on x3).
  epilogue  as exact_lattice.pre_store: residual, ReLU / LeakyReLU (one fp32 multiply by float32(0.2)), BN (one multiply by a power of two,
            one add); store as exact_lattice.store.
Where no non-zero product is dropped this is the plain exact convolution; expected() asserts which of the two holds (only the `both` rows of
bf16x3 drop something: lo.lo, non-zero in at least 1 % of their outputs).

Kinds of rows (the carried operand's LOWEST non-zero part is what a row is about):
  x_carry   x dense, +-[X/2, X] (fp16 parts: +-[2049, X]); w dense in {-1, 0, 1}, or [-2, 2] where X reaches its cap even so.  Pins lo.hi
            (x6: mid.hi -- X is capped at 16 bits, two bf16 parts).
  w_carry   w dense, +-[Wc/2, Wc]; x dense in [-1, 1], or [-4, 4] where Wc reaches its cap even so.  Pins hi.lo (x6: hi.mid).
  x_lo      (x6) x dense, +-[2^19, 2^20); w exactly m entries of +-1 per cout, scattered over all (tap, cin).  Pins lo.hi and mid.hi.
  w_lo      (x6) x = +-1 in ONE channel per pixel, the channel moving with the pixel through every cin chunk; w dense, +-[2^19, 2^20).
            Pins hi.lo and hi.mid.
  both      (bf16x3, bf16x6) x one channel per pixel, +-[513, 1023]; w dense, +-[513, 1023].  x6: pins mid.mid (and mid.hi, hi.mid).  x3: pins
            lo.hi and hi.lo together, and that lo.lo is NOT added.  Left out for fp16x3: a 12-bit by 12-bit product fills the 24-bit
            accumulator by itself; lo.hi and hi.lo are pinned there by x_carry and w_carry.
X, Wc and m are the LARGEST values for which assert_bounds holds for the row (derive(): from the row's K = taps * cin, its non-zero counts,
the analytic maxima of the parts, bias, residual and BN), capped at 65535 (two bf16 parts hold an integer of 16 bits with zero residue) and
32767 (fp16).  None is tuned against a kernel; test_split_carry_cpu.py holds the typed table against derive().

Storage: dense x3 / fp16x3 rows store fp32 (op_out_f32; split rows take the same tile with it), x6 rows store their three parts (any integer
below 2^24 fits).  The fused deconv + shortcut launch refuses an fp32 output: its x3 / fp16x3 rows have sparse weights, FUSED_M = 4 entries
per cout over the two weight tensors together, and X or Wc such that |value| < 2^16 (x3: 16 significant bits) or < 65504 (fp16x3); their
`both` row cannot exist (a 10-bit by 10-bit product does not fit 16 bits).  The fused x6 rows are dense: their storage holds 24 bits.

The span ladder.  CARRY_LIMIT = 2^24 is fp32's significand; whether gfx950's 16-bit MFMA adds its products exactly into an accumulator that
spans 24 bits is what the ladder rows measure: one geometry on conv_igemm_v2ps<4,2>x3 and on its fp16 twin at limits 2^18, 2^20, 2^22, 2^24,
with all-positive x and half of the couts' weights non-negative so that the sums really reach the limit's magnitude (random signs would leave
them at sqrt(K) of it).  `ladder` rows are x_carry at X = limit / K (the low rungs carry nothing there: 2^18 / 4608 = 56); `ladder_m` rows
keep X = 4095 and thin the weights to m = limit / X entries per cout, so that every rung has non-zero lo parts.
OBSERVED ON THE MI355X (LADDER_OUTCOME): all sixteen ladder rows pass bit for bit, the 2^24 rungs included (sums of 8.7e6 and 1.27e7 before BN), in
bf16 and in fp16 parts.  The 16-bit MFMA adds its products exactly while the accumulator stays below 2^24 units, so CARRY_LIMIT stays 2^24 and X,
Wc and m are derived from it.

A helper, not a conftest: nothing here touches the library or a GPU."""
import collections
import math

import numpy as np
import torch
import torch.nn.functional as F

import exact_lattice as xl
from exact_lattice import Case, bf16_rne, significant_bits, assert_split_fit, store, compare, out_hw  # noqa: F401  (re-exported for the tests)

CARRY_LIMIT = 2 ** 24
LADDER_OUTCOME = "every rung passed, 2^24 included: CARRY_LIMIT = 2^24"
LADDER_RUNGS = (2 ** 18, 2 ** 20, 2 ** 22, 2 ** 24)
PART_BITS = {"bf16x3": 8, "bf16x6": 8, "fp16x3": 11}
N_PARTS = {"bf16x3": 2, "bf16x6": 3, "fp16x3": 2}
PART_NAMES = {2: ("hi", "lo"), 3: ("hi", "mid", "lo")}
CAP = {"bf16x3": 65535, "bf16x6": 65535, "fp16x3": 32767}
OUT_LIMIT = {"bf16x3": 2 ** 16, "fp16x3": 65504}         # 16-bit split storage of the fused x3 / fp16x3 rows: |value| below it fits
FUSED_M = 4
LO3, HI3 = 2 ** 19, 2 ** 20 - 1                          # three-part operands
BOTH_LO, BOTH_HI = 513, 1023
LADDER_X = 4095
KINDS = {"bf16x3": ("x_carry", "w_carry", "both"), "fp16x3": ("x_carry", "w_carry"), "bf16x6": ("x_carry", "w_carry", "x_lo", "w_lo", "both")}
# the segments a row of a kind is about, besides hi.hi (which every row pins)
PINS = {
    ("x_carry", 2): ("lo.hi",), ("w_carry", 2): ("hi.lo",), ("both", 2): ("lo.hi", "hi.lo"),
    ("x_carry", 3): ("mid.hi",), ("w_carry", 3): ("hi.mid",), ("x_lo", 3): ("lo.hi", "mid.hi"), ("w_lo", 3): ("hi.lo", "hi.mid"),
    ("both", 3): ("mid.mid", "mid.hi", "hi.mid"),
}

# A row: the fields of exact_lattice.Case (geometry, policy batch and options of the CASES row `base`), and
#   kind: above, or "ladder" (x_carry at X = limit / K) / "ladder_m" (X = 4095, m weights per cout);  mag: X or Wc (None: fixed ranges)
#   m: non-zero weights per cout (0: dense);  limit: what assert_bounds holds the row to;  lean: sums of one sign (the ladder)
CarryCase = collections.namedtuple("CarryCase", Case._fields + ("kind", "base", "mag", "m", "limit", "lean"))


def carry(id, base, kind, mag=None, m=0, limit=CARRY_LIMIT, twin=False):
    """A row on the geometry, policy and options of the exact row `base`; the storage follows the module docstring.  twin: the bf16x3 row's
    geometry run in fp16x3 (the planner takes the same tile; the kernel is the fp16 twin, "h")."""
    if twin:
        assert base.precision == "bf16x3" and "_v2ps<" in base.label
        base = base._replace(precision="fp16x3", label=base.label.replace("_v2ps<", "_v2psh<"))
    assert base.precision in KINDS and (kind in KINDS[base.precision] or kind in ("ladder", "ladder_m")), "%s: no %s rows on %s" % (id, kind, base.precision)
    out_f32 = False if base.op == "fused" else (True if N_PARTS[base.precision] == 2 else base.out_f32)
    assert base.act != 2 or out_f32 or base.precision == "bf16x6", "%s: LeakyReLU needs 24 stored bits" % id
    return CarryCase(*base._replace(id=id, out_f32=out_f32, wmul=1), kind=kind, base=base.id, mag=mag, m=m, limit=limit, lean=kind.startswith("ladder"))


def rne(v, precision):
    v = np.ascontiguousarray(v, np.float32)
    if precision == "fp16x3":
        return np.clip(v, -65504, 65504).astype(np.float16).astype(np.float32)
    return bf16_rne(v)


def parts(v, precision):
    """The parts the library stores for fp32 values v (float32 arithmetic, as nchw_to_split_kernel and put_w do it)."""
    rest, out = np.ascontiguousarray(v, np.float32), []
    for _ in range(N_PARTS[precision]):
        p = rne(rest, precision)
        out.append(p)
        rest = (rest - p).astype(np.float32)
    return out


def kept_segments(precision):
    """(input part, weight part) names in the order the K loop walks them (idc_layout.h, the comments of split_seg_x / split_seg_w)."""
    if N_PARTS[precision] == 2:
        return ["lo.hi", "hi.lo", "hi.hi"]
    return ["hi.lo", "lo.hi", "mid.mid", "mid.hi", "hi.mid", "hi.hi"]


def _seg_index(precision, name):
    names = PART_NAMES[N_PARTS[precision]]
    a, b = name.split(".")
    return names.index(a), names.index(b)


def pinned(c):
    return ("hi.hi",) + PINS[("x_carry" if c.kind == "ladder" or c.kind == "ladder_m" else c.kind, N_PARTS[c.precision])]


def f16_weight_exponent(*ws):
    """csrc/idc_pack.hip: the s that brings max|w| into [8192, 16384); a fused pair shares the smaller one."""
    out = []
    for w in ws:
        mx = float(np.abs(w).max())
        s = 0 if mx == 0 else 14 - math.frexp(mx)[1]
        out.append(max(-10, min(40, s)))
    return min(out)


def weight_parts(c, d):
    """{"w": parts, "w2": parts}: fp16x3 weights go through 2^s and back (exact unless a part over- or underflows, which the zero-residue assertion
    of expected() would show)."""
    names = ("w", "w2") if c.op == "fused" else ("w",)
    s = f16_weight_exponent(*[d[k] for k in names]) if c.precision == "fp16x3" else 0
    return {k: [np.ldexp(p, -s).astype(np.float32) for p in parts(np.ldexp(d[k], s).astype(np.float32), c.precision)] for k in names}


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------
def taps_of(c):
    return {"conv": c.ksize * c.ksize, "deconv": 4, "fused": 4}[c.op]      # a ConvTranspose 4x4 s2 output pixel sees 2 x 2 taps


def terms(c):
    """The largest number of non-zero products that can meet in one output, per segment."""
    if c.m:
        return c.m
    if c.kind in ("w_lo", "both"):                                        # x has one non-zero channel per pixel
        return taps_of(c) + (9 if c.op == "fused" else 0)
    return taps_of(c) * c.cin + (9 * c.cin2 if c.op == "fused" else 0)


def part_maxima(M, precision):
    """Upper bounds of |part 0|, |part 1|, ... over the integers of magnitude <= M: |v - rne(v)| <= half an ulp of rne(v), and an integer
    remainder below 1 is 0."""
    out, r = [], float(M)
    for _ in range(N_PARTS[precision]):
        p = float(rne(np.array([r], np.float32), precision)[0]) if r >= 1 else 0.0
        out.append(p)
        r = 2.0 ** (math.floor(math.log2(p)) - PART_BITS[precision]) if p >= 1 else 0.0
    return out


def segment_sum(precision, mx, mw):
    """sum over the kept segments of max|part_i(x)| * max|part_j(w)|: what one term can add to a partial sum, all segments together."""
    px, pw = part_maxima(mx, precision), part_maxima(mw, precision)
    return sum(px[i] * pw[j] for i, j in (_seg_index(precision, s) for s in kept_segments(precision)))


def extras(c):
    return xl.B_MAX * (2 if c.op == "fused" else 1) + (xl.resid_max(c) if c.resid else 0)


def budget(c):
    """What the K loops may reach: limit, less bias and residual, less BN (bn >= 1 scales the value, bn < 1 makes the unit smaller), and for
    16-bit split storage the range in which every integer fits."""
    lim = c.limit
    if xl.STORAGE[c.precision] == "split" and not c.out_f32 and c.precision in OUT_LIMIT:
        lim = min(lim, OUT_LIMIT[c.precision])
    top = lim - 1
    if c.bn is not None:
        top = math.floor((top - xl.BN_SHIFT_MAX) / c.bn) if c.bn >= 1 else top - math.ceil(xl.BN_SHIFT_MAX / c.bn)
    return top - extras(c)


def _ranges(c, mag, other):
    """(max|x|, max|w|) of a row of c's kind at magnitude `mag`, the uncarried operand at `other`."""
    if c.kind in ("x_carry", "ladder", "ladder_m"):
        return mag, other
    if c.kind == "w_carry":
        return other, mag
    return {"x_lo": (HI3, 1), "w_lo": (1, HI3), "both": (BOTH_HI, BOTH_HI)}[c.kind]


def derive(c):
    """(mag, m, the uncarried operand's range) of the module docstring's rule, from the row's own geometry, storage and limit."""
    t, room, p = terms(c._replace(m=0)), budget(c), c.precision
    if c.kind == "x_lo":
        m = int(room // segment_sum(p, HI3, 1))
        return None, min(m, t), 1
    if c.kind in ("w_lo", "both"):
        assert t * segment_sum(p, *_ranges(c, None, None)) <= room, "%s: %d terms do not fit" % (c.id, t)
        return None, 0, None
    if c.kind == "ladder_m":
        return LADDER_X, min(int(room // segment_sum(p, LADDER_X, 1)), t), 1
    sparse = c.op == "fused" and N_PARTS[p] == 2
    if sparse:
        t = FUSED_M
    for other in ((1,) if sparse or c.kind == "ladder" else ((2, 1) if c.kind == "x_carry" else (4, 1))):
        mag = min(CAP[p], int(room // (t * other)))
        while mag > 0 and t * segment_sum(p, *_ranges(c, mag, other)) > room:
            mag -= 1
        if mag == CAP[p] or other == 1:
            return mag, (FUSED_M if sparse else 0), other
    raise AssertionError(c.id)


def carried_floor(c):
    """The smallest magnitude the carried operand is drawn at: half the largest; on fp16 parts 2049, the first integer a part cannot hold."""
    if c.kind in ("x_lo", "w_lo"):
        return LO3
    if c.kind == "both":
        return BOTH_LO
    if c.kind == "ladder" or c.precision != "fp16x3":
        return max(1, c.mag // 2)
    return 2049


# ---- draws -----------------------------------------------------------------------------------------------------------------------------
def _signed(rs, lo, hi, shape, positive=False):
    v = rs.randint(lo, hi + 1, size=shape).astype(np.float32)
    return v if positive else v * np.where(rs.randint(0, 2, size=shape) > 0, 1, -1).astype(np.float32)


def _one_channel(rs, lo, hi, n, cin, h, w, salt):
    """+-[lo, hi] in one channel per pixel; the channel moves with the pixel and the image, through every cin chunk where there are pixels enough."""
    x = np.zeros((n, cin, h, w), np.float32)
    nn, yy, xx = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing="ij")
    ch = ((yy * w + xx) * 37 + nn * 171 + salt) % cin
    x[nn, ch, yy, xx] = _signed(rs, lo, hi, (n, h, w))
    return x


def _sparse(rs, m, cout, sizes, lo, hi, positive_from=None):
    """Exactly m entries of +-[lo, hi] per cout over len(sizes) flattened weight tensors together -> one (cout, size) array per tensor."""
    flat = np.zeros((cout, sum(sizes)), np.float32)
    pos = np.argsort(rs.rand(cout, sum(sizes)), axis=1)[:, :m]
    flat[np.arange(cout)[:, None], pos] = _signed(rs, lo, hi, (cout, m))
    if positive_from is not None:
        flat[positive_from:] = np.abs(flat[positive_from:])
    return np.split(flat, np.cumsum(sizes)[:-1], axis=1)


def draw(c):
    """The operands of a row, float32 arrays of integers (seeded by the row's id).  Weights are in torch layout: conv (cout, cin, k, k), deconv
    (cin, cout, 4, 4)."""
    rs = np.random.RandomState(sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id)) % (2 ** 31))
    ho, wo = out_hw(c)
    mag, m, other = derive(c)
    assert (mag, m) == (c.mag, c.m), "%s: the table says X / Wc = %r, m = %r; the bound gives %r, %r" % (c.id, c.mag, c.m, mag, m)
    floor = carried_floor(c)
    xshape, x2shape = (c.n, c.cin, c.h, c.w), (c.n, c.cin2, ho, wo)
    wsizes = [c.cin * (c.ksize * c.ksize if c.op == "conv" else 16)] + ([c.cin2 * 9] if c.op == "fused" else [])
    d = {"b": xl._ints(rs, -xl.B_MAX, xl.B_MAX, (c.cout,))}
    if c.op == "fused":
        d["b2"] = xl._ints(rs, -xl.B_MAX, xl.B_MAX, (c.cout,))
    half = c.cout // 2 if c.lean else None
    if c.kind in ("x_carry", "ladder", "ladder_m"):
        d["x"] = _signed(rs, floor, mag, xshape, positive=c.lean)
        if c.op == "fused":
            d["x2"] = _signed(rs, floor, mag, x2shape)
        ws = _sparse(rs, m, c.cout, wsizes, 1, 1, half) if m else [xl._ints(rs, -other, other, (c.cout, s)) for s in wsizes]
        if c.lean and not m:
            ws[0][half:] = np.abs(ws[0][half:])
    elif c.kind == "w_carry":
        d["x"] = xl._ints(rs, -other, other, xshape)
        if c.op == "fused":
            d["x2"] = xl._ints(rs, -other, other, x2shape)
        ws = _sparse(rs, m, c.cout, wsizes, floor, mag) if m else [_signed(rs, floor, mag, (c.cout, s)) for s in wsizes]
    elif c.kind == "x_lo":
        d["x"] = _signed(rs, LO3, HI3, xshape)
        if c.op == "fused":
            d["x2"] = _signed(rs, LO3, HI3, x2shape)
        ws = _sparse(rs, m, c.cout, wsizes, 1, 1)
    else:                                                                 # w_lo, both: one channel per pixel against dense carrying weights
        lo, hi = (1, 1) if c.kind == "w_lo" else (BOTH_LO, BOTH_HI)
        d["x"] = _one_channel(rs, lo, hi, c.n, c.cin, c.h, c.w, 0)
        if c.op == "fused":
            d["x2"] = _one_channel(rs, lo, hi, c.n, c.cin2, ho, wo, 5)
        ws = [_signed(rs, floor, HI3 if c.kind == "w_lo" else BOTH_HI, (c.cout, s)) for s in wsizes]
    if c.op == "conv":
        d["w"] = np.ascontiguousarray(ws[0].reshape(c.cout, c.cin, c.ksize, c.ksize))
    else:
        d["w"] = np.ascontiguousarray(ws[0].reshape(c.cout, c.cin, 4, 4).transpose(1, 0, 2, 3))
    if c.op == "fused":
        d["w2"] = np.ascontiguousarray(ws[1].reshape(c.cout, c.cin2, 3, 3))
    if c.resid:
        d["resid"] = xl._ints(rs, -xl.resid_max(c), xl.resid_max(c), (c.n, c.cout, ho, wo))
    if c.bn is not None:
        d["bn_s"] = np.full(c.cout, c.bn, np.float32)
        d["bn_t"] = xl._ints(rs, -xl.BN_SHIFT_MAX, xl.BN_SHIFT_MAX, (c.cout,))
    return d


def nonzero_per_output(c, d):
    """The largest count of non-zero weights one output can meet, from the drawn weights: per cout, over cin and the taps one pixel sees."""
    if c.op == "conv":
        n = (d["w"] != 0).sum(axis=(1, 2, 3)).max()
    else:                                                                 # output phase (py, px) sees the taps ky = 1 - py + 2a, kx = 1 - px + 2b
        nz = (d["w"] != 0)
        n = max(nz[:, :, (1 - py)::2, (1 - px)::2].sum(axis=(0, 2, 3)).max() for py in (0, 1) for px in (0, 1))
    return int(n) + (int((d["w2"] != 0).sum(axis=(1, 2, 3)).max()) if c.op == "fused" else 0)


def operand_parts(c, d):
    """{"x": parts, "w": parts, ...}: every operand's parts, once per row."""
    out = weight_parts(c, d)
    for k in ("x", "x2") if c.op == "fused" else ("x",):
        out[k] = parts(d[k], c.precision)
    return out


def assert_bounds(c, d, op=None):
    """No partial sum of a correct kernel -- any subset of the kept segments' products, in any order -- and no pre-store value can reach the
    row's limit: asserted from the row's own count of terms per output and the maxima of the drawn parts, before anything runs on a GPU.
    Returns the bound on |accumulator|."""
    for k in ("x", "w", "b") + (("x2", "w2", "b2") if c.op == "fused" else ()) + (("resid",) if c.resid else ()):
        assert np.array_equal(d[k], np.round(d[k])), "%s: %s is not on the integer lattice" % (c.id, k)
    assert np.abs(d["x"]).max() <= CAP[c.precision] or c.kind == "x_lo", "%s: x beyond what the parts hold" % c.id
    op = operand_parts(c, d) if op is None else op
    acc = 0.0
    for xk, wk in (("x", "w"), ("x2", "w2")) if c.op == "fused" else (("x", "w"),):
        px = [float(np.abs(p).max()) for p in op[xk]]
        pw = [float(np.abs(p).max()) for p in op[wk]]
        acc = max(acc, sum(px[i] * pw[j] for i, j in (_seg_index(c.precision, s) for s in kept_segments(c.precision))))
    if c.kind in ("w_lo", "both"):
        t = terms(c)
        assert ((d["x"] != 0).sum(axis=1) <= 1).all(), "%s: more than one channel per pixel" % c.id
    else:
        t = min(terms(c), nonzero_per_output(c, d))
    acc = t * acc
    assert acc <= budget(c), "%s: worst-case partial sum %.0f leaves the row's budget %.0f (limit %d)" % (c.id, acc, budget(c), c.limit)
    return acc


# ---- expected --------------------------------------------------------------------------------------------------------------------------
def _conv(c, x, w, second=False):
    x, w = torch.from_numpy(np.ascontiguousarray(x)).double(), torch.from_numpy(np.ascontiguousarray(w)).double()
    if second:
        return F.conv2d(x, w, padding=1).numpy()
    if c.op == "conv":
        return F.conv2d(x[:, :, ::c.in_stride, ::c.in_stride], w, padding=c.dilation * (c.ksize // 2), dilation=c.dilation).numpy()
    return F.conv_transpose2d(x, w, stride=2, padding=1).numpy()


def segment_pairs(c, fault=None, all_pairs=False):
    """The (input part, weight part) index pairs a kernel multiplies: the kept ones; with `fault` the deliberately wrong variants of
    tests/test_split_carry_cpu.py: ("drop", k) leaves segment k out, ("wpart0", k) / ("xpart0", k) make it read weight / input part 0."""
    p = N_PARTS[c.precision]
    if all_pairs:
        return [(i, j) for i in range(p) for j in range(p)]
    out = []
    for name in kept_segments(c.precision):
        i, j = _seg_index(c.precision, name)
        if fault is not None and fault[1] == name:
            if fault[0] == "drop":
                continue
            i, j = (i, 0) if fault[0] == "wpart0" else (0, j)
        out.append((i, j))
    assert fault is None or fault[0] in ("drop", "wpart0", "xpart0") and fault[1] in kept_segments(c.precision)
    return out


def k_loops(c, d, pairs, op=None):
    """sum over `pairs` of conv(part_i(x), part_j(w)), float64 (both K loops of a fused row)."""
    wp = operand_parts(c, d) if op is None else op
    y = 0.0
    for xk, wk in (("x", "w"), ("x2", "w2")) if c.op == "fused" else (("x", "w"),):
        px = wp[xk]
        groups = {}                                                       # input parts that meet the same weight parts share one conv (linearity)
        for i in range(len(px)):
            js = tuple(j for ii, j in pairs if ii == i and wp[wk][j].any())
            if js and px[i].any():                                        # (a part that is zero everywhere adds nothing)
                groups[js] = groups.get(js, 0.0) + px[i].astype(np.float64)
        for js, xsum in groups.items():
            y = y + _conv(c, xsum, sum(wp[wk][j].astype(np.float64) for j in js), second=(xk == "x2"))
    return y


_KEPT = {}


def drops_something(c):
    return c.kind == "both" and N_PARTS[c.precision] == 2


def expected(c, d=None, fault=None):
    """What a correct kernel stores, bit for bit.  Without `fault`: asserts the bounds, that the parts hold every operand with zero residue, that
    the model drops a non-zero product exactly where the row says so, and the storage fit."""
    d = draw(c) if d is None else d
    op = operand_parts(c, d)
    if fault is None:
        y = k_loops(c, d, segment_pairs(c), op)
    else:                                         # the one changed segment against the kept sum (shared by a row's faults; the operands are the row's draw)
        if c.id not in _KEPT:
            _KEPT.clear()
            _KEPT[c.id] = k_loops(c, d, segment_pairs(c), op)
        segment_pairs(c, fault)                   # (checks the fault's name)
        i, j = _seg_index(c.precision, fault[1])
        come = {"drop": [], "wpart0": [(i, 0)], "xpart0": [(0, j)]}[fault[0]]
        y = _KEPT[c.id] - k_loops(c, d, [(i, j)], op) + (k_loops(c, d, come, op) if come else 0.0)
    if fault is None:
        assert_bounds(c, d, op)
        for k in ("x", "x2", "w", "w2") if c.op == "fused" else ("x", "w"):
            held = sum(p.astype(np.float64) for p in op[k])
            assert np.array_equal(held, d[k].astype(np.float64)), "%s: the parts do not hold %s" % (c.id, k)
        # (the parts hold the operands, so by linearity kept + dropped segments are the plain exact convolution: tests/test_split_carry_cpu.py)
        kept = segment_pairs(c)
        lost = float((np.zeros_like(y) != k_loops(c, d, [p for p in segment_pairs(c, all_pairs=True) if p not in kept], op)).mean())
        if drops_something(c):
            assert lost >= 0.01, "%s: the dropped lo.lo term is non-zero in %.2f %% of the outputs only" % (c.id, 100 * lost)
        else:
            assert lost == 0.0, "%s: the kept segments drop a non-zero product" % c.id
    y = y + d["b"].astype(np.float64)[None, :, None, None]
    if c.op == "fused":
        y = y + d["b2"].astype(np.float64)[None, :, None, None]
    if c.resid:
        y = y + d["resid"].astype(np.float64)
    if fault is None:
        assert np.array_equal(y, np.round(y)) and np.abs(y).max() < c.limit, "%s: a pre-activation value leaves the lattice (max %.0f)" % (c.id, np.abs(y).max())
    v = y.astype(np.float32)                                              # exact without a fault: integers below 2^24
    if c.act == 1:
        v = np.maximum(v, np.float32(0))
    elif c.act == 2:
        v = np.where(v < 0, v * np.float32(0.2), v).astype(np.float32)
    if c.bn is not None:
        v = (v * d["bn_s"][None, :, None, None]).astype(np.float32) + d["bn_t"][None, :, None, None]
        if fault is None:                                                 # exact: the unit is min(bn, 1), the value below limit units
            assert np.abs(v.astype(np.float64)).max() / min(c.bn, 1.0) < c.limit, c.id
    v = np.ascontiguousarray(v, np.float32)
    if fault is not None:
        return v
    return store(c, v)


def lowest_part_share(c, d):
    """Share of the carried operand's non-zero elements whose lowest carried part is non-zero (lo on two-part precisions and on x_lo / w_lo,
    mid on the dense x6 rows), the smaller of the two operands' on `both` rows."""
    which = {"x_carry": ("x",), "ladder": ("x",), "ladder_m": ("x",), "x_lo": ("x",), "w_carry": ("w",), "w_lo": ("w",), "both": ("x", "w")}[c.kind]
    idx = 2 if c.kind in ("x_lo", "w_lo") else 1
    wp = weight_parts(c, d)
    out = []
    for k in which + tuple(k + "2" for k in which if c.op == "fused"):
        p = (wp[k] if k in wp else parts(d[k], c.precision))[idx]
        out.append(float((p[d[k] != 0] != 0).mean()))
    return min(out)
