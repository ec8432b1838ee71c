"""The antialiased ingestion rule of include/ideepcolor.h (idc_set_ingest_filter) in plain numpy float64, one output index at a time, written
independently of ``colorspace.resize_antialias`` -- and the inputs of tests/test_resample_gpu.py with the condition they have to meet.

``resample(img, H, W)`` -> (the values before rounding, the rounded lattice image).  ``mutant=`` breaks the rule in one of six ways, or the
way the kernel walks it in one of four (tests/test_resample_cpu.py shows that the exact comparison on the GPU inputs catches each).

Nets.  CASES run on the 64 x 64 net (H, W below).  NET_CASES carry a net of their own, for what a square 64-wide net cannot reach:
  (16, 8), (24, 16), (8, 24)   RGB sources 16383 / 16384 wide: one-column tiles whose window alone is larger than a chunk of 1365 columns, walked
                               in 2, 3 and 4 chunks with the sum carried across them; last chunks of 342, 171, 682, 683 columns and of ONE
                               column; one- and two-chunk tiles in one launch.  The chunked path is reachable for three channels only, and only
                               for W <= 24 (it needs s > 682; sources end at 16384).  One channel's chunk is 4096 columns, which 16384 -> 8 fills
                               exactly and never passes: the Gray8 / Gray16 3 x 16384 cases sit on that equality and are NOT chunked.
  (64, 64)                     RGB with several column tiles: tw = 20 (last tile 4 columns), tw = 4 (sixteen tiles), tw = 61 (last tile 3):
                               col = i0 + lane / 3, ch = lane % 3 with i0 > 0, which the CASES run for one channel only.
  (40, 72), (72, 40)           not square, so a swap of H and W shows ('transposed_net'); 72 = 64 + 8: two tiles.
  (16, 24)                     a net a forward runs on: one chunked job of 24 tiles beside small ones in ONE pipelined call.
``tiling`` / ``tiles_of`` restate the tile widths, spans and chunks of csrc/idc_resample.h; PATHS holds the path each case is there for.

Bars: the rounded image is compared exactly, every sample: the inputs are drawn, and drawn again where they fail (``case``), until every
value before rounding lies further than EDGE = 1e-6 from a rounding tie -- float64 sums of at most 513 + 513 products of magnitude <= 65535
carry errors below 1e-8, so no order of summation or contraction could flip one.  The windows of NET_CASES hold up to 4097 taps: the weights
sum to 1, so a sum of n = 4097 products of samples <= 65535 carries about n x 2^-53 x 65535 < 3e-8, still far inside EDGE (and the rule fixes
the order: ascending, across chunks too).  The exception is the exact 2x case: away from the clipped
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

# Cases on nets of their own: name -> ((H, W) of the net, h, w, channels, dtype).  What each is for is in PATHS below, which
# tests/test_resample_cpu.py asserts from the tiling restated further down (``tiling``): a case that stops taking its path fails there.
NET_CASES = {
    "n16x8_rgb_3x16384": ((16, 8), 3, 16384, 3, np.uint8),
    "n16x8_rgb_40x6000": ((16, 8), 40, 6000, 3, np.uint8),
    "n24x16_rgb_5x16383": ((24, 16), 5, 16383, 3, np.uint8),
    "n8x24_rgb_3x16384": ((8, 24), 3, 16384, 3, np.uint8),
    "n16x8_gray8_3x16384": ((16, 8), 3, 16384, 1, np.uint8),
    "n16x8_gray16_3x16384": ((16, 8), 3, 16384, 1, np.uint16),
    "n64x64_rgb_5x4099": ((64, 64), 5, 4099, 3, np.uint8),
    "n64x64_rgb_3x16384": ((64, 64), 3, 16384, 3, np.uint8),
    "n64x64_rgb_2x1400": ((64, 64), 2, 1400, 3, np.uint8),
    "n40x72_rgb_211x83": ((40, 72), 211, 83, 3, np.uint8),
    "n40x72_rgb_100x40": ((40, 72), 100, 40, 3, np.uint8),          # down on rows only
    "n40x72_rgb_50x200": ((40, 72), 50, 200, 3, np.uint8),          # down on columns only
    "n40x72_gray16_211x83": ((40, 72), 211, 83, 1, np.uint16),
    "n72x40_rgb_211x83": ((72, 40), 211, 83, 3, np.uint8),          # the transposed net of the same source
    "n16x24_rgb_3x16384": ((16, 24), 3, 16384, 3, np.uint8),        # the pipelined call of tests/test_resample_gpu.py on a net that runs a forward
    "n16x24_rgb_30x50": ((16, 24), 30, 50, 3, np.uint8),
}
# name -> the tiling of its columns: tw, tiles, the set of span widths, of chunk counts and of last-chunk widths (in columns) over its tiles
PATHS = {
    "n16x8_rgb_3x16384": dict(tw=1, tiles=8, spans=[3072, 4096], chunks=[3, 4], last=[1, 342]),
    "n16x8_rgb_40x6000": dict(tw=1, tiles=8, spans=[1125, 1500], chunks=[1, 2], last=[135, 1125]),
    "n24x16_rgb_5x16383": dict(tw=1, tiles=16, spans=[1536, 2047, 2048], chunks=[2], last=[171, 682, 683]),
    "n8x24_rgb_3x16384": dict(tw=1, tiles=24, spans=[1024, 1365, 1366], chunks=[1, 2], last=[1, 1024, 1365]),
    "n16x8_gray8_3x16384": dict(tw=1, tiles=8, spans=[3072, 4096], chunks=[1], last=[3072, 4096]),
    "n16x8_gray16_3x16384": dict(tw=1, tiles=8, spans=[3072, 4096], chunks=[1], last=[3072, 4096]),
    "n64x64_rgb_5x4099": dict(tw=20, tiles=4, last_tile=4),
    "n64x64_rgb_3x16384": dict(tw=4, tiles=16, last_tile=4),
    "n64x64_rgb_2x1400": dict(tw=61, tiles=2, last_tile=3),
    "n40x72_rgb_211x83": dict(tw=64, tiles=2, last_tile=8),
    "n40x72_rgb_100x40": dict(tw=64, tiles=2, last_tile=8),
    "n40x72_rgb_50x200": dict(tw=64, tiles=2, last_tile=8),
    "n40x72_gray16_211x83": dict(tw=64, tiles=2, last_tile=8),
    "n72x40_rgb_211x83": dict(tw=40, tiles=1, last_tile=40),
    "n16x24_rgb_3x16384": dict(tw=1, tiles=24, chunks=[1, 2]),
    "n16x24_rgb_30x50": dict(tw=24, tiles=1, last_tile=24),
}
TILE_MUTANTS = ["chunk_restart", "chunk_drop_last", "first_tile_only"]
LEAN = ("n8x24_rgb_3x16384", "n16x24_rgb_3x16384")              # ``lean_on_the_last_column``


def spec(name):
    """-> ((H, W) of the case's net, h, w, channels, dtype)."""
    return NET_CASES[name] if name in NET_CASES else ((H, W),) + CASES[name]


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


# ---- the tiling of csrc/idc_resample.h, restated from its comments (tools/resample_selftest.cpp prints the header's own figures, and
# tests/test_resample_cpu.py holds these equal to them): one workgroup per tile of tw output columns of one output row; the vertical sums of
# the source columns the tile's windows cover (its span) are staged CHUNK_ELEMS float64 at a time, i.e. CHUNK_ELEMS // channels columns.
CHUNK_ELEMS = 4096
MAX_TW = 64


def chunk_cols(channels):
    return CHUNK_ELEMS // channels


def span(i0, i1, n_in, n_out):
    """The source indices [c0, c1) that the output indices [i0, i1) read (both rules are monotone in i)."""
    return taps(i0, n_in, n_out)[0][0], taps(i1 - 1, n_in, n_out)[0][-1] + 1


def tile_width(n_in, n_out, channels):
    """The largest tw <= min(n_out, MAX_TW) for which the span of EVERY tile fits one chunk; 1 when not even one column's does.  A span of tw
    columns is at most (tw - 1) s + 2 s + 2 wide: the search starts at the largest tw that bound admits."""
    cols = chunk_cols(channels)
    s = float(n_in) / float(n_out) if n_in > n_out else 1.0
    tw = min(n_out, MAX_TW)
    bound = (float(cols) - 2.0 * s - 2.0) / s + 1.0
    if bound < float(tw):
        tw = 1 if bound < 1.0 else int(bound)
    while tw > 1:
        if all(c1 - c0 <= cols for c0, c1 in (span(i0, min(i0 + tw, n_out), n_in, n_out) for i0 in range(0, n_out, tw))):
            break
        tw -= 1
    return tw


def tiles_of(n_in, n_out, channels):
    """-> tw and, per tile, (i0, i1, c0, c1, the chunks [(cc0, cc1), ...] its span is walked in, ascending)."""
    tw, cols = tile_width(n_in, n_out, channels), chunk_cols(channels)
    out = []
    for i0 in range(0, n_out, tw):
        i1 = min(i0 + tw, n_out)
        c0, c1 = span(i0, i1, n_in, n_out)
        out.append((i0, i1, c0, c1, [(cc0, min(cc0 + cols, c1)) for cc0 in range(c0, c1, cols)]))
    return tw, out


def tiling(n_in, n_out, channels):
    """-> (tw, tiles, the largest chunk count of a tile): what ``resample_selftest in out channels`` prints."""
    tw, tiles = tiles_of(n_in, n_out, channels)
    return tw, len(tiles), max(len(t[4]) for t in tiles)


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
    if mutant == "transposed_net":                  # H and W swapped: the rule for a (W, H) net, whose rows of H are then read as rows of W
        v, out = resample(img, out_w, out_h)        # (what a kernel that took W for H and H for W leaves in memory: nothing on a square net)
        return v.reshape((out_h, out_w) + v.shape[2:]), out.reshape((out_h, out_w) + out.shape[2:])
    full = full_scale(img.dtype)
    f = (img if img.ndim == 3 else img[:, :, None]).astype(np.float64)
    in_h, in_w, ch = f.shape
    tw, tiles = tiles_of(in_w, out_w, ch) if mutant in TILE_MUTANTS else (0, None)
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
            if tiles is not None:
                i0, _, c0, c1, chunks = tiles[x // tw]
                if mutant == "first_tile_only":     # the window of the column's index within its tile
                    ks, ws = taps(x - i0, in_w, out_w)
                elif mutant == "chunk_restart":     # the sum starts again at every chunk: what the last chunk holds is left
                    ks, ws = zip(*[(k, w) for k, w in zip(ks, ws) if k >= chunks[-1][0]] or [(0, 0.0)])
                elif len(chunks) > 1:               # chunk_drop_last
                    ks, ws = zip(*[(k, w) for k, w in zip(ks, ws) if k < chunks[-1][0]] or [(0, 0.0)])
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


def exempt_from_edge(name, net=None):
    """The samples of a case whose ties the rule itself decides (exact arithmetic): the interior of the exact 2x case."""
    m = np.zeros(spec(name)[0] if net is None else net, bool)
    if name == "rgb_128x128":
        m[1:-1, 1:-1] = True
    return m


def draw(name, seed):
    """The seeded source of a case.  The cases of NET_CASES lay the noise over a slow wave: the mean of thousands of independent samples is
    127.5 +- 1 whatever is summed, and an image of three levels shows little."""
    _, h, w, ch, dtype = spec(name)
    rs = np.random.RandomState(1000 * seed + sum(map(ord, name)))
    a = rs.randint(0, full_scale(dtype) + 1, (h, w, ch)).astype(dtype)
    if name in NET_CASES:
        y, x, c = np.meshgrid(np.arange(h) / float(h), np.arange(w) / float(w), np.arange(ch), indexing="ij")
        wave = 0.5 + 0.45 * np.sin(2 * np.pi * (2.3 * x + 1.2 * y + 0.31 * c + rs.uniform()))
        a = np.floor(full_scale(dtype) * (0.7 * wave + 0.3 * a / float(full_scale(dtype)))).astype(dtype)
    return a if ch == 3 else a[:, :, 0]


def offenders(name, v):
    """The (y, x, c) of the samples that lie within EDGE of a tie and are not exempt."""
    d = tie_distance(v if v.ndim == 3 else v[:, :, None])
    return np.argwhere((d <= EDGE) & ~exempt_from_edge(name, d.shape[:2])[:, :, None])


def meets_condition(name, v):
    return len(offenders(name, v)) == 0


def lean_on_the_last_column(name, src):
    """A second chunk of ONE column holds the window's last tap, whose weight is about 0.5 / s^2: 1e-6 at s = 682, so that column moves a
    sample by at most 3e-4 of a level and a kernel that dropped it would pass unless a value lay that close below a tie.  This puts one
    there: in the first output row (which reads source row 0 alone when the rows are scaled up) of the first tile with such a chunk, the
    last column is set to full scale and the other taps are stepped, heaviest first, until channel 0 lies below a tie by half of what the
    last column adds.  -> (y, x, c) of that sample.  The re-draw of ``case`` leaves it alone: it is far further than EDGE from the tie."""
    (net_h, net_w), in_h, in_w, ch, dtype = spec(name)
    assert in_h <= net_h and taps(0, in_h, net_h)[0] == [0, 0] and src.ndim == 3
    _, tiles = tiles_of(in_w, net_w, ch)
    i0, _, _, _, chunks = [t for t in tiles if len(t[4]) > 1 and t[4][-1][1] - t[4][-1][0] == 1][0]
    ks, ws = taps(i0, in_w, net_w)
    assert ks[-1] == chunks[-1][0]
    full = full_scale(dtype)
    src[0, ks[-1], 0] = full
    adds = ws[-1] * full
    body = sum(w * float(src[0, k, 0]) for k, w in zip(ks[:-1], ws[:-1]))
    want = np.floor(body) + 0.5 - adds / 2.0            # body + adds crosses the tie, body alone does not
    for j in np.argsort(ws[:-1])[::-1]:
        if ws[j] <= 0.0:
            break
        step = int(np.clip(np.round((want - body) / ws[j]), -int(src[0, ks[j], 0]), full - int(src[0, ks[j], 0])))
        src[0, ks[j], 0] = int(src[0, ks[j], 0]) + step
        body += step * ws[j]
    return 0, i0, 0


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (source, v, rounded), read-only.  The source is a seeded random draw.  A whole image cannot be redrawn until no sample is near a
    tie: at a small rational scale the weights are fractions of a small denominator M (65 -> 64: M = 132) and about one sample in M is an
    exact tie of the rule, dozens per image whatever the seed.  So the draw is repeated where it fails: the source sample under the
    heaviest taps of each offending output sample is drawn again, until every sample meets the condition (``meets_condition``, which the
    tests assert on the result: no sample is left out of it or of any comparison).  A case of NET_CASES is resampled to its own net."""
    net_h, net_w = spec(name)[0]
    src = draw(name, 0)
    if name in LEAN:
        lean_on_the_last_column(name, src)
    rs = np.random.RandomState(77)
    in_h, in_w = src.shape[:2]
    for _ in range(64):
        v, out = resample(src, net_h, net_w)
        bad = offenders(name, v)
        if len(bad) == 0:
            for a in (src, v, out):
                a.setflags(write=False)
            return src, v, out
        for y, x, c in bad:
            (ky, wy), (kx, wx) = taps(int(y), in_h, net_h), taps(int(x), in_w, net_w)
            at = (ky[int(np.argmax(wy))], kx[int(np.argmax(wx))]) + ((int(c),) if src.ndim == 3 else ())
            src[at] = rs.randint(0, full_scale(src.dtype) + 1)
    raise AssertionError("%s: some value stays within %g of a tie" % (name, EDGE))


def stripes(h=520, w=520):
    """One-pixel vertical stripes 0, 255, 0, 255, ...: they average 127.5."""
    g = np.zeros((h, w), np.uint8)
    g[:, 1::2] = 255
    return g
