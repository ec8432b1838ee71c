"""The painted-hint-layer rule of include/ideepcolor.h (idc_set_hints_layer / idc_forward_async_layers) in plain loops and numpy float64,
written from the rule's text, not from the kernel -- with the inputs the GPU file uses, the comparisons it makes, and the mutants of the
rule that tests/test_layer_cpu.py shows those comparisons catch.

Bars (``compare``):
  mask, cells   exact
  ab            within one float32 ulp everywhere (the bar tests/test_eval_gpu.py holds revealed colours to: the device's pow / cbrt and
                numpy's may differ in the last float64 bit, which moves the once-rounded fp32 by at most one step); bit for bit in every cell
                with ONE painted pixel -- there the mean is the colour itself
Nets: ``case`` runs on the 64 x 64 net (H, W), whose 4096 cells fill four thread-form workgroups exactly.  ``net_case`` runs on NET = (40, 72):
2880 cells, so the thread form's third workgroup ends on a fourth pass with ONE live wave (the `p < HW` tail and the fold of the count over
idle waves), a swap of H and W shows, and 640 x 1152 / 641 x 1152 sit on either side of the form threshold (16 x 16 = 256 pixels: thread;
18 x 16: wave).  NET_MUTANTS break the walk over the net rather than the rule of a cell.
Everything here is a function of its arguments and fixed seeds; references are computed once per case and cached (do not write into them)."""
import functools

import numpy as np

H = W = 64
SIZES = [(1, 1), (1, 200), (200, 1), (64, 64), (32, 32), (48, 80), (211, 83), (1000, 700), (65, 16384)]
PARAMS = [(128, 0), (1, 0), (255, 128), (128, 255)]          # (alpha_min, cover)
MASK_VALUE = 1.0
MUTANTS = ["centre_footprints", "alpha_gt", "alpha_weighted", "rgb_mean", "cover_flipped", "cover_strict", "layer_over_rects", "float32_sums"]
THREAD_MAX = 256

_M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
_WHITE = np.array([0.95047, 1.0, 1.08883])


def rgb_to_ab(rgb):
    """(..., 3) sRGB in 0..255 (uint8, or float for the rgb_mean mutant) -> (..., 2) float64 (a, b): skimage's rgb2lab constants."""
    v = np.asarray(rgb, np.float64) / 255.0
    lin = np.where(v > 0.04045, ((v + 0.055) / 1.055) ** 2.4, v / 12.92)
    xyz = np.stack([lin[..., 0] * _M[i, 0] + lin[..., 1] * _M[i, 1] + lin[..., 2] * _M[i, 2] for i in range(3)], -1) / _WHITE
    g = np.where(xyz > 0.008856, np.cbrt(xyz), 7.787 * xyz + 16.0 / 116.0)
    return np.stack([500.0 * (g[..., 0] - g[..., 1]), 200.0 * (g[..., 1] - g[..., 2])], -1)


def footprint(i, l, out):
    """The layer indices [lo, hi) whose extent overlaps net index i's, in integers."""
    return (i * l) // out, ((i + 1) * l + out - 1) // out


def span_bound(l, out):
    if l <= out:
        return 1 if out % l == 0 else 2
    return l // out if l % out == 0 else l // out + 2


def wave_form(lh, lw, H_=H, W_=W):
    return span_bound(lh, H_) * span_bound(lw, W_) > THREAD_MAX


def _ordered_sum(vals, wave, dtype=np.float64):
    """The documented order: row-major upwards from 0.0, or 64 partial sums (pixels j, j + 64, ...) folded by halves."""
    vals = np.asarray(vals, dtype)
    if not wave:
        return np.cumsum(np.concatenate([np.zeros(1, dtype), vals]), dtype=dtype)[-1]
    pad = np.zeros((len(vals) + 63) // 64 * 64, dtype)
    pad[:len(vals)] = vals
    part = np.cumsum(pad.reshape(-1, 64), axis=0, dtype=dtype)[-1]
    for o in (32, 16, 8, 4, 2, 1):
        part = (part[:o] + part[o:2 * o]).astype(dtype)
    return part[0]


def raster_rects(rects, mode, mask_value, H_=H, W_=W):
    """idc_set_hints: inclusive rectangles, corners in either order, clipped, later over earlier -> ab (2,H,W), mask (1,H,W) float32."""
    ab = np.zeros((2, H_, W_), np.float32)
    mask = np.zeros((1, H_, W_), np.float32)
    for r in rects:
        y0, y1 = max(min(r[0], r[2]), 0), min(max(r[0], r[2]), H_ - 1)
        x0, x1 = max(min(r[1], r[3]), 0), min(max(r[1], r[3]), W_ - 1)
        if y0 > y1 or x0 > x1:
            continue
        c = rgb_to_ab(np.array(r[4:7], np.float64).astype(np.uint8)) if mode == "rgb" else np.array(r[4:6], np.float64)
        ab[0, y0:y1 + 1, x0:x1 + 1] = np.float32(c[0])
        ab[1, y0:y1 + 1, x0:x1 + 1] = np.float32(c[1])
        mask[0, y0:y1 + 1, x0:x1 + 1] = np.float32(mask_value)
    return ab, mask


def layer_hints(rgba, alpha_min, cover, rects=(), mode="rgb", mask_value=MASK_VALUE, H_=H, W_=W, mutant=None):
    """The rule.  -> dict(ab (2,H,W) f32, mask (1,H,W) f32, cells int, single (H,W) bool: the layer hinted the cell from ONE painted pixel,
    cnt / tot (H,W) int: the counts of every cell)."""
    assert mutant is None or mutant in MUTANTS + NET_MUTANTS
    rgba = np.asarray(rgba)
    lh, lw = rgba.shape[:2]
    ab, mask = raster_rects(rects, mode, mask_value, H_, W_)
    covered = mask[0] != 0
    if mutant in NET_MUTANTS:
        return _net_mutant(rgba, alpha_min, cover, ab, mask, covered, mask_value, H_, W_, mutant)
    A = rgba[..., 3].astype(np.int64)
    painted = A > alpha_min if mutant == "alpha_gt" else A >= alpha_min
    col = rgb_to_ab(rgba[..., :3])
    wave = wave_form(lh, lw, H_, W_)
    dtype = np.float32 if mutant == "float32_sums" else np.float64
    cells = 0
    single = np.zeros((H_, W_), bool)
    cnts, tots = np.zeros((H_, W_), np.int64), np.zeros((H_, W_), np.int64)
    for y in range(H_):
        r0, r1 = footprint(y, lh, H_)
        if mutant == "centre_footprints":
            rows = [r for r in range(lh) if y * lh <= (2 * r + 1) * H_ // 2 < (y + 1) * lh]
            r0, r1 = (rows[0], rows[-1] + 1) if rows else (0, 0)
        for x in range(W_):
            c0, c1 = footprint(x, lw, W_)
            if mutant == "centre_footprints":
                cols = [c for c in range(lw) if x * lw <= (2 * c + 1) * W_ // 2 < (x + 1) * lw]
                c0, c1 = (cols[0], cols[-1] + 1) if cols else (0, 0)
            p = painted[r0:r1, c0:c1].ravel()
            tot, cnt = p.size, int(p.sum())
            cnts[y, x], tots[y, x] = cnt, tot
            if mutant == "cover_flipped":
                ok = cnt >= 1 and 255 * cnt <= cover * tot
            elif mutant == "cover_strict":
                ok = cnt >= 1 and 255 * cnt > cover * tot
            else:
                ok = cnt >= 1 and 255 * cnt >= cover * tot
            if not ok or (covered[y, x] and mutant != "layer_over_rects"):
                continue
            if mutant == "rgb_mean":
                m = rgb_to_ab(rgba[r0:r1, c0:c1, :3].reshape(-1, 3)[p].astype(np.float64).mean(0))
            else:
                v = col[r0:r1, c0:c1].reshape(-1, 2)
                wgt = np.where(p, A[r0:r1, c0:c1].ravel(), 0).astype(np.float64) if mutant == "alpha_weighted" else p.astype(np.float64)
                den = dtype(wgt.sum()) if mutant == "alpha_weighted" else dtype(cnt)
                m = [_ordered_sum(v[:, k] * wgt, wave, dtype) / den for k in range(2)]
            ab[0, y, x], ab[1, y, x] = np.float32(m[0]), np.float32(m[1])
            mask[0, y, x] = np.float32(mask_value)
            cells += 0 if covered[y, x] else 1
            single[y, x] = cnt == 1
    return dict(ab=ab, mask=mask, cells=cells, single=single, cnt=cnts, tot=tots)


def _net_mutant(rgba, alpha_min, cover, ab, mask, covered, mask_value, H_, W_, mutant):
    """Mistakes in how the kernel walks the net, not in the rule of a cell (the kernel: a workgroup takes PASSES x 256 consecutive cells in the
    thread form, 256 at a time, or PASSES x 4 in the wave form, one per wave; the hits of its four waves are summed into the count):
      'transposed_net'    H and W swapped: the rule for a (W, H) net, whose rows of H cells are then read as rows of W (nothing on a square net)
      'tail_unhinted'     cells from the last, partial pass of the last workgroup on are left alone
      'count_first_wave'  the count takes the hits of each workgroup's first wave only"""
    lh, lw = rgba.shape[:2]
    if mutant == "transposed_net":
        t = layer_hints(rgba, alpha_min, cover, (), "rgb", mask_value, W_, H_)
        t = {k: (v.reshape(v.shape[:-2] + (H_, W_)) if isinstance(v, np.ndarray) else v) for k, v in t.items()}
        wave = wave_form(lh, lw, W_, H_)
    else:
        t = layer_hints(rgba, alpha_min, cover, (), "rgb", mask_value, H_, W_)
        wave = wave_form(lh, lw, H_, W_)
    hinted = (t["mask"][0] != 0) & ~covered
    p = np.arange(H_ * W_).reshape(H_, W_)
    per_pass = 4 if wave else 256
    if mutant == "tail_unhinted":
        hinted &= p < (H_ * W_) // per_pass * per_pass
    ab, mask = ab.copy(), mask.copy()
    ab[:, hinted] = t["ab"][:, hinted]
    mask[0, hinted] = np.float32(mask_value)
    counted = hinted & (p % per_pass < (1 if wave else 64)) if mutant == "count_first_wave" else hinted
    return dict(ab=ab, mask=mask, cells=int(counted.sum()), single=t["single"] & hinted, cnt=t["cnt"], tot=t["tot"])


def _ord32(a):
    b = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def compare(got_ab, got_mask, got_cells, want):
    """The GPU file's comparisons of one image's planes and count with ``want`` (``layer_hints``).  -> the list of what failed (empty: equal)."""
    bad = []
    got_ab, got_mask = np.asarray(got_ab, np.float32).reshape(want["ab"].shape), np.asarray(got_mask, np.float32).reshape(want["mask"].shape)
    if not np.array_equal(got_mask, want["mask"]):
        bad.append("mask differs in %d cells" % int((got_mask != want["mask"]).sum()))
    if int(got_cells) != int(want["cells"]):
        bad.append("cells %d, want %d" % (int(got_cells), int(want["cells"])))
    ulps = np.abs(_ord32(got_ab) - _ord32(want["ab"]))
    if ulps.max() > 1:
        bad.append("ab off by up to %d ulps in %d values" % (int(ulps.max()), int((ulps > 1).sum())))
    one = np.broadcast_to(want["single"], want["ab"].shape)
    if not np.array_equal(got_ab[one].view(np.int32), want["ab"][one].view(np.int32)):
        bad.append("ab of single-pixel cells differs in %d values" % int((got_ab[one].view(np.int32) != want["ab"][one].view(np.int32)).sum()))
    return bad


# ------------------------------------------------------------------------------------------------ the GPU file's inputs
def draw_layer(lh, lw, alpha_min, seed):
    """PIL lines and polygons plus random specks; alpha from {0, alpha_min - 1, alpha_min, 255}.  One and the same array per arguments."""
    from PIL import Image, ImageDraw
    rng = np.random.RandomState(seed)
    alphas = [0, alpha_min - 1, alpha_min, 255]
    im = Image.new("RGBA", (lw, lh), (0, 0, 0, 0))
    d = ImageDraw.Draw(im)

    def colour(a=None):
        return tuple(int(v) for v in rng.randint(0, 256, 3)) + (int(alphas[rng.randint(4)] if a is None else a),)

    def pt():
        return (int(rng.randint(0, lw)), int(rng.randint(0, lh)))

    for k in range(3):
        d.polygon([pt(), pt(), pt(), pt()], fill=colour(255 if k == 0 else None))
    for k in range(6):
        d.line([pt(), pt()], fill=colour(), width=int(rng.randint(1, max(2, min(lh, lw) // 8 + 2))))
    a = np.array(im, np.uint8)
    ns = max(1, lh * lw // 50)
    ys, xs = rng.randint(0, lh, ns), rng.randint(0, lw, ns)
    a[ys, xs, :3] = rng.randint(0, 256, (ns, 3))
    a[ys, xs, 3] = np.array(alphas)[rng.randint(0, 4, ns)]
    if lh * lw <= 4:
        a[..., 3] = 255
    return np.ascontiguousarray(a)


RECTS = [(5, 7, 9, 30, 200, 40, 60), (40, 12, 47, 13, 10, 250, 10), (60, 50, 70, 80, 30, 30, 240), (8, 28, 6, 33, 255, 255, 0)]


@functools.lru_cache(maxsize=None)
def case(k):
    """GPU case k: SIZES[k] with PARAMS[k % 4], over RECTS.  -> (rgba, alpha_min, cover, want)."""
    lh, lw = SIZES[k]
    alpha_min, cover = PARAMS[k % 4]
    rgba = draw_layer(lh, lw, alpha_min, 100 + k)
    rgba.setflags(write=False)
    return rgba, alpha_min, cover, layer_hints(rgba, alpha_min, cover, RECTS)


# ---- a net that is not square: 40 x 72 = 2880 cells.  The thread form gives 3 workgroups, the last of 832 cells: three full passes and a
# fourth with ONE live wave (cells 2816..2879, the last 64 of the bottom row), so `p < HW` and the fold of the count over idle waves run; an
# h / w swap shows.  The wave form takes 180 workgroups of 16 cells and has no partial pass here.
NET = (40, 72)
NET_SIZES = [(1, 1), (40, 72), (72, 40), (211, 83), (1000, 700), (65, 16384), (640, 1152), (641, 1152)]
# bounds: 65 x 16384: 3 x 229, wave; 640 x 1152: 16 x 16 = 256, the largest thread-form footprint; 641 x 1152: 18 x 16, the first wave-form one
NET_WAVE = [False, False, False, False, True, True, False, True]           # (1000 x 700: 25 x 11 = 275, wave on this net)
NET_RECTS = [(5, 7, 9, 30, 200, 40, 60), (30, 12, 35, 13, 10, 250, 10), (38, 60, 45, 80, 30, 30, 240), (8, 28, 6, 33, 255, 255, 0)]
NET_MUTANTS = ["transposed_net", "tail_unhinted", "count_first_wave"]
TAIL = 64                                                               # the cells of the live wave of the last pass


def draw_net_layer(lh, lw, alpha_min, seed, net=NET):
    """``draw_layer`` with a fully painted strip of random colours under the bottom row of the net, from cell 20 to the right edge: hinted cells
    among the last TAIL, some of them under NET_RECTS[2]."""
    a = draw_layer(lh, lw, alpha_min, seed)
    r0, c0 = footprint(net[0] - 1, lh, net[0])[0], footprint(20, lw, net[1])[0]
    rng = np.random.RandomState(seed + 1)
    a[r0:, c0:, :3] = rng.randint(0, 256, a[r0:, c0:, :3].shape)
    a[r0:, c0:, 3] = 255
    return np.ascontiguousarray(a)


@functools.lru_cache(maxsize=None)
def net_case(k, net=NET):
    """GPU case k of the 40 x 72 net: NET_SIZES[k] with PARAMS[k % 4], over NET_RECTS.  -> (rgba, alpha_min, cover, want)."""
    lh, lw = NET_SIZES[k]
    alpha_min, cover = PARAMS[k % 4]
    rgba = draw_net_layer(lh, lw, alpha_min, 300 + k, net)
    rgba.setflags(write=False)
    return rgba, alpha_min, cover, layer_hints(rgba, alpha_min, cover, NET_RECTS, H_=net[0], W_=net[1])


def rects_of_layer(rgba, alpha_min):
    """The 1 x 1 IDC_HINT_RGB rectangle list a net-size layer with cover 0 equals: one per painted pixel."""
    ys, xs = np.nonzero(rgba[..., 3] >= alpha_min)
    return [(int(y), int(x), int(y), int(x)) + tuple(int(v) for v in rgba[y, x, :3]) for y, x in zip(ys, xs)]
