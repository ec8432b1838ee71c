"""The antialiased ingestion rule of include/ideepcolor.h (idc_set_ingest_filter) in plain numpy float64, one output index at a time, written
independently of ``colorspace.resize_antialias`` -- and the inputs of tests/test_resample_gpu.py with the condition they have to meet.

``resample(img, H, W)`` -> (the values before rounding, the rounded lattice image).  ``mutant=`` breaks the rule in one of six ways
(tests/test_resample_cpu.py shows that the exact comparison on the GPU inputs catches each).

Bars: the rounded image is compared exactly, every sample: the inputs are drawn, and drawn again where they fail (``case``), until every
value before rounding lies further than EDGE = 1e-6 from a rounding tie -- float64 sums of at most 513 + 513 products of magnitude <= 65535
carry errors below 1e-8, so no order of summation or contraction could flip one.  The exception is the exact 2x case: away from the clipped
windows of the border its weights are 1/8, 3/8, 3/8, 1/8, every product and partial sum is an exact multiple of 1/64, and its ties are
decided by the rule itself.  lab_net / l_net: 1e-9, the project's bar for float64 colour arithmetic."""
import functools
import math

import numpy as np

H = W = 64
EDGE = 1e-6
L_TOL = 1e-9                     # the project's bar for float64 colour arithmetic (tests/gray_ref.py)

# name -> (h, w, channels, dtype); the first group is down-scaled on an axis, the second is not
DOWN = {
    "rgb_65x64": (65, 64, 3, np.uint8),            # s barely above 1 on one axis, the identity on the other
    "rgb_128x128": (128, 128, 3, np.uint8),        # exact 2x
    "rgb_211x83": (211, 83, 3, np.uint8),
    "rgb_100x40": (100, 40, 3, np.uint8),          # down on one axis, up on the other
    "rgb_40x100": (40, 100, 3, np.uint8),
    "rgb_1x1000": (1, 1000, 3, np.uint8),
    "rgb_1000x1": (1000, 1, 3, np.uint8),
    "rgb_700x1000": (700, 1000, 3, np.uint8),      # several column tiles, windows of ~30 taps
    "rgb_4099x67": (4099, 67, 3, np.uint8),        # a prime size, 129-tap windows
    "gray8_65x16384": (65, 16384, 1, np.uint8),    # s = 256: 512-tap windows, 1 MB
    "gray16_211x83": (211, 83, 1, np.uint16),
    "gray16_700x300": (700, 300, 1, np.uint16),
}
SAME = {
    "rgb_64x64": (64, 64, 3, np.uint8),
    "rgb_30x50": (30, 50, 3, np.uint8),
    "rgb_1x1": (1, 1, 3, np.uint8),
}
CASES = dict(DOWN, **SAME)


def full_scale(dtype):
    return 255 if np.dtype(dtype) == np.uint8 else 65535


def taps_down(i, n_in, n_out, mutant=None):
    """s > 1: the taps (source indices, ascending) and weights of output index i."""
    s = float(n_in) / float(n_out)
    c = (i + 0.5) * s
    if mutant == "centre":
        c = c - 0.5
    sup = s / 2 if mutant == "half_support" else s
    lo, hi = int(c - sup + 0.5), int(c + sup + 0.5)
    if mutant != "replicate":
        lo, hi = max(0, lo), min(n_in, hi)
    ks = list(range(lo, hi))
    r = [max(0.0, 1.0 - abs(k + 0.5 - c) / sup) for k in ks]
    tot = 0.0
    for v in r:
        tot = tot + v
    if mutant == "unnormalised":
        tot = sup
    return [min(max(k, 0), n_in - 1) for k in ks], [v / tot for v in r]


def taps_up(i, n_in, n_out):
    """s <= 1: the two clamped taps of the bilinear rule, weights (1 - w) and w."""
    src = (i + 0.5) * (float(n_in) / float(n_out)) - 0.5
    fl = math.floor(src)
    w = src - fl
    i0 = int(fl)
    return [min(max(i0, 0), n_in - 1), min(max(i0 + 1, 0), n_in - 1)], [1.0 - w, w]


def taps(i, n_in, n_out, mutant=None):
    return taps_down(i, n_in, n_out, mutant) if n_in > n_out else taps_up(i, n_in, n_out)


def _bilinear(f, out_h, out_w):
    """A source that is not down-scaled: the ingestion rule as it stands (rows first: top, bottom, then the vertical blend)."""
    out = np.zeros((out_h, out_w, f.shape[2]))
    for y in range(out_h):
        (y0, y1), (_, wy) = taps_up(y, f.shape[0], out_h)
        for x in range(out_w):
            (x0, x1), (_, wx) = taps_up(x, f.shape[1], out_w)
            top = f[y0, x0] * (1.0 - wx) + f[y0, x1] * wx
            bot = f[y1, x0] * (1.0 - wx) + f[y1, x1] * wx
            out[y, x] = top * (1.0 - wy) + bot * wy
    return out


def resample(img, out_h=H, out_w=W, mutant=None):
    """-> (v float64 (out_h,out_w[,c]) before rounding, the rounded image in img's dtype)."""
    img = np.asarray(img)
    full = full_scale(img.dtype)
    f = (img if img.ndim == 3 else img[:, :, None]).astype(np.float64)
    in_h, in_w, ch = f.shape
    if in_h <= out_h and in_w <= out_w:
        v = _bilinear(f, out_h, out_w)
    else:
        acc = np.float32 if mutant == "float32" else np.float64
        t = np.zeros((out_h, in_w, ch), acc)
        for y in range(out_h):                      # t[x] = sum_y wy * f[y][x], ascending y
            ks, ws = taps(y, in_h, out_h, mutant)
            row = np.zeros((in_w, ch), acc)
            for k, w in zip(ks, ws):
                row = row + acc(w) * f[k].astype(acc)
            t[y] = row
        if mutant == "round_first":
            t = np.floor(t + 0.5).clip(0, full)
        v = np.zeros((out_h, out_w, ch), acc)
        for x in range(out_w):                      # v = sum_x wx * t[x], ascending x
            ks, ws = taps(x, in_w, out_w, mutant)
            col = np.zeros((out_h, ch), acc)
            for k, w in zip(ks, ws):
                col = col + acc(w) * t[:, k]
            v[:, x] = col
        v = v.astype(np.float64)
    out = np.floor(v + 0.5).clip(0, full).astype(img.dtype)
    if img.ndim == 2:
        return v[:, :, 0], out[:, :, 0]
    return v, out


def tie_distance(v):
    """How far every value before rounding is from the nearest rounding tie (k + 0.5)."""
    return np.abs(v - np.floor(v) - 0.5)


def exempt_from_edge(name):
    """The samples of a case whose ties the rule itself decides (exact arithmetic): the interior of the exact 2x case."""
    m = np.zeros((H, W), bool)
    if name == "rgb_128x128":
        m[1:-1, 1:-1] = True
    return m


def draw(name, seed):
    h, w, ch, dtype = CASES[name]
    rs = np.random.RandomState(1000 * seed + sum(map(ord, name)))
    a = rs.randint(0, full_scale(dtype) + 1, (h, w, ch)).astype(dtype)
    return a if ch == 3 else a[:, :, 0]


def offenders(name, v):
    """The (y, x, c) of the samples that lie within EDGE of a tie and are not exempt."""
    d = tie_distance(v if v.ndim == 3 else v[:, :, None])
    return np.argwhere((d <= EDGE) & ~exempt_from_edge(name)[:, :, None])


def meets_condition(name, v):
    return len(offenders(name, v)) == 0


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (source, v, rounded), read-only.  The source is a seeded random draw.  A whole image cannot be redrawn until no sample is near a
    tie: at a small rational scale the weights are fractions of a small denominator M (65 -> 64: M = 132) and about one sample in M is an
    exact tie of the rule, dozens per image whatever the seed.  So the draw is repeated where it fails: the source sample under the
    heaviest taps of each offending output sample is drawn again, until every sample meets the condition (``meets_condition``, which the
    tests assert on the result: no sample is left out of it or of any comparison)."""
    src = draw(name, 0)
    rs = np.random.RandomState(77)
    in_h, in_w = src.shape[:2]
    for _ in range(64):
        v, out = resample(src)
        bad = offenders(name, v)
        if len(bad) == 0:
            for a in (src, v, out):
                a.setflags(write=False)
            return src, v, out
        for y, x, c in bad:
            (ky, wy), (kx, wx) = taps(int(y), in_h, H), taps(int(x), in_w, W)
            at = (ky[int(np.argmax(wy))], kx[int(np.argmax(wx))]) + ((int(c),) if src.ndim == 3 else ())
            src[at] = rs.randint(0, full_scale(src.dtype) + 1)
    raise AssertionError("%s: some value stays within %g of a tie" % (name, EDGE))


def stripes(h=520, w=520):
    """One-pixel vertical stripes 0, 255, 0, 255, ...: they average 127.5."""
    g = np.zeros((h, w), np.uint8)
    g[:, 1::2] = 255
    return g
