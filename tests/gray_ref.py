"""Greyscale sources (include/ideepcolor.h states the rule; idc_set_image_gray, idc_fullres_rgb / idc_fullres_ab on a kept plane,
idc_fullres_rgb16) restated in numpy float64, the inputs the GPU file runs it on, and the comparisons it holds the device to.

The resize is ``colorspace.resize_bilinear_u8``'s expressions restated for one channel of either width (the rounding lattice is the sample
type's); the colour formulas are the oracle's rgb2lab / lab2rgb written out for arrays; both truncations are ``astype``.  Nothing here reads
the project this one was modelled on.  Nets: SIZES / SEEDS / BATCH are for the 64 x 64 net (H, W); NET = (40, 72) with NET_SIZES / NET_SEEDS /
NET_HINTS is the net that is not square, on which the (H, W) every grey kernel is handed cannot be swapped unseen.  ``variant`` swaps in one of the mistakes tests/test_gray_cpu.py shows the comparisons would catch:
  'drop8'       a 16-bit route that drops to 8 bits before L
  'scale65536'  full scale 65536 instead of 65535
  'round_out'   round-to-nearest where the rule truncates on output
  'resize8'     a resize that rounds to the 8-bit lattice
  'transposed_net'  H and W of the net swapped (``resize``): nothing on the 64 x 64 net, which is why NET = (40, 72) below has cases of its own"""
import numpy as np

import ingest_ref

M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
MI = np.linalg.inv(M)
WHITE = np.array([0.95047, 1.0, 1.08883])

# the GPU file's handle and sources: a 64 x 64 net; 1 x 1, one row, one column, smaller than the net, the net size, and 211 x 83 (several
# ragged joint tiles, non-integer ratios on both axes)
H, W = 64, 64
SIZES = [(1, 1), (1, 5), (7, 1), (2, 3), (23, 31), (64, 64), (211, 83)]     # (2 x 3: with the others, every pixel count mod 4)
# the crop and noise seed of each size: the first for which no resized sample of either width lies on a rounding boundary (the weights are
# multiples of 1/128 on each axis, so an unrounded value is a multiple of 1/16384 and about one image in five has a pixel on k + 1/2;
# tests/test_gray_cpu.py holds the condition)
SEEDS = {(1, 1): 1000, (1, 5): 1000, (7, 1): 1000, (2, 3): 1000, (23, 31): 1008, (64, 64): 1000, (211, 83): 1000}
# the pipelined batches take them in this order: the images start at pixels 0, 1, 6, 12, 19, 732 and 4828 of the flat run, every residue mod 4
BATCH = [(1, 1), (1, 5), (2, 3), (7, 1), (23, 31), (64, 64), (211, 83)]
L_CENT = 50.0
RGB_HINTS = [(2, 3, 20, 30, 200, 40, 90), (16, 25, 50, 60, 10, 250, 128), (40, 2, 62, 20, 0, 0, 255), (0, 50, 10, 63, 255, 255, 0)]
HINTS = [(2, 3, 20, 30, 35.0, -50.0), (16, 25, 50, 60, -30.0, 45.0), (40, 2, 62, 20, 70.0, 20.0), (0, 50, 10, 63, -60.0, -15.0)]
L_TOL = AB_TOL = 1e-9            # the project's bar for float64 colour arithmetic (tests/test_joint_gpu.py, the same quantities)
EDGE = 1e-6                      # a value this close to a rounding boundary may fall on either side of it
MAX_DIFF_SHARE = 1e-3            # ... on at most this share of an image's pixels


def full_scale(dtype, variant=None):
    if np.dtype(dtype) == np.uint8:
        return 255.0
    assert np.dtype(dtype) == np.uint16, dtype
    return 65536.0 if variant == "scale65536" else 65535.0


# A net that is not square: an H / W swap anywhere between the resize, net_sample, zoom_nearest, interp_ab and the joint tile shows.  Planes
# smaller than the net, of the net's size and 211 x 83 (down on rows 5.3x, on columns 1.15x); their seeds are found as SEEDS' are, for the resize
# to 40 x 72 (tests/test_gray_cpu.py holds the condition).  ``gray16(.., net=NET)`` draws them.
NET = (40, 72)
NET_SIZES = [(23, 31), (40, 72), (211, 83)]
NET_SEEDS = {(23, 31): 1016, (40, 72): 1000, (211, 83): 1005}
NET_HINTS = [(2, 3, 12, 30, 35.0, -50.0), (10, 25, 30, 60, -30.0, 45.0), (25, 2, 38, 20, 70.0, 20.0), (0, 50, 6, 71, -60.0, -15.0)]


def gray16(sh, sw, seed=0, net=None):
    """(sh, sw) uint16: the luma of a crop of the golden photograph on the 16-bit lattice (smooth content, real interpolation weights) plus
    seeded noise in the low byte, so that the samples are not multiples of 257.  ``net``: None for the 64 x 64 net's draws, NET for NET's."""
    assert net in (None, NET)
    rgb = ingest_ref.mortar()
    rs = np.random.RandomState((SEEDS.get((sh, sw), 0) if net is None else NET_SEEDS[(sh, sw)]) + seed)
    y, x = rs.randint(0, 256 - sh + 1), rs.randint(0, 256 - sw + 1)
    c = rgb[y:y + sh, x:x + sw].astype(np.int64)
    v = 60 * c[..., 0] + 120 * c[..., 1] + 24 * c[..., 2] + rs.randint(0, 256, (sh, sw))      # at most 204 * 255 + 255: nothing clips
    return v.astype(np.uint16)


def gray8(sh, sw, seed=0, net=None):
    return (gray16(sh, sw, seed, net) >> 8).astype(np.uint8)


def hint_lists(n, rows=None):
    """Per-image hint lists of a batch of n: none for every third image, a tail of ``rows`` (HINTS) for the others."""
    rows = HINTS if rows is None else rows
    return [None if i % 3 == 0 else rows[i % 4:] for i in range(n)]


def starts(sizes):
    """The pixel at which each image of a packed run starts."""
    return [int(x) for x in np.cumsum([0] + [h * w for h, w in sizes])[:-1]]


def ramp16(sh=211, sw=83, first=30000, codes=300):
    """(sh, sw) uint16: ``codes`` consecutive 16-bit codes from ``first`` on, spread over the pixels in raster order."""
    idx = (np.arange(sh * sw, dtype=np.int64) * codes) // (sh * sw)
    return (first + idx).reshape(sh, sw).astype(np.uint16)


def resize_unrounded(g, out_h, out_w):
    """[out_h,out_w] float64: the bilinear value of every net-size pixel before it is rounded (half-pixel centres, clamped taps)."""
    g = np.asarray(g)
    in_h, in_w = g.shape
    ys = (np.arange(out_h) + 0.5) * (in_h / float(out_h)) - 0.5
    xs = (np.arange(out_w) + 0.5) * (in_w / float(out_w)) - 0.5
    y0 = np.floor(ys).astype(np.int64); x0 = np.floor(xs).astype(np.int64)
    wy = (ys - y0)[:, None]; wx = (xs - x0)[None, :]
    y0c = np.clip(y0, 0, in_h - 1); y1c = np.clip(y0 + 1, 0, in_h - 1)
    x0c = np.clip(x0, 0, in_w - 1); x1c = np.clip(x0 + 1, 0, in_w - 1)
    f = g.astype(np.float64)
    top = f[y0c][:, x0c] * (1 - wx) + f[y0c][:, x1c] * wx
    bot = f[y1c][:, x0c] * (1 - wx) + f[y1c][:, x1c] * wx
    return top * (1 - wy) + bot * wy


def resize(g, out_h=H, out_w=W, variant=None):
    """The net-size plane, of g's dtype: round half up on the dtype's own lattice, clamped to it."""
    g = np.asarray(g)
    if variant == "transposed_net":                 # H and W swapped: the plane of a (W, H) net, whose rows of H are then read as rows of W
        return resize(g, out_w, out_h).reshape(out_h, out_w)
    out = resize_unrounded(g, out_h, out_w)
    if variant == "resize8" and g.dtype == np.uint16:
        return (np.floor(out / 257.0 + 0.5).clip(0, 255) * 257).astype(np.uint16)
    return np.floor(out + 0.5).clip(0, full_scale(g.dtype)).astype(g.dtype)


def srgb_to_linear(v):
    return np.where(v > 0.04045, ((v + 0.055) / 1.055) ** 2.4, v / 12.92)


def lightness(g, variant=None):
    """L [.,.] float64 of the samples: rgb2lab's formulas on the value repeated on three channels."""
    g = np.asarray(g)
    if variant == "drop8" and g.dtype == np.uint16:
        g = (g >> 8).astype(np.uint8)
    t = srgb_to_linear(g.astype(np.float64) / full_scale(g.dtype, variant))
    y = (M[1, 0] * t + M[1, 1] * t + M[1, 2] * t) / WHITE[1]
    return 116.0 * np.where(y > 0.008856, np.cbrt(y), 7.787 * y + 16.0 / 116.0) - 16.0


def l_plane(l_net, l_cent=L_CENT):
    """The slot's fp32 L plane from l_net, cast as the kernel casts: (float)(L - (double)l_cent)."""
    return (np.asarray(l_net, np.float64) - np.float64(np.float32(l_cent))).astype(np.float32)


def guide(l_net, l_cent=L_CENT):
    """L_lo of the joint rule: (double)Lplane + (double)l_cent."""
    return l_plane(l_net, l_cent).astype(np.float64) + np.float64(np.float32(l_cent))


def lab_to_srgb(L, ab):
    """[h,w,3] float64 in [0, 1]: lab2rgb's formulas, clipped, not quantised.  L [h,w], ab [2,h,w]."""
    L = np.asarray(L, np.float64)
    fy = (L + 16.0) / 116.0
    f = np.stack([ab[0] / 500.0 + fy, fy, np.maximum(fy - ab[1] / 200.0, 0.0)], axis=-1)
    xyz = np.where(f > 0.2068966, f ** 3, (f - 16.0 / 116.0) / 7.787) * WHITE
    lin = np.stack([xyz[..., 0] * MI[c, 0] + xyz[..., 1] * MI[c, 1] + xyz[..., 2] * MI[c, 2] for c in range(3)], axis=-1)
    s = np.where(lin > 0.0031308, 1.055 * np.power(np.maximum(lin, 0), 1 / 2.4) - 0.055, 12.92 * lin)
    return np.clip(s, 0.0, 1.0)


def quantise(s, depth, variant=None):
    """(uint8)(s * 255.0) or (uint16)(s * 65535.0): truncation."""
    v = s * (255.0 if depth == 8 else 65535.0)
    if variant == "round_out":
        v = np.floor(v + 0.5)
    return v.astype(np.uint8 if depth == 8 else np.uint16)


def image(g, ab, depth, variant=None):
    """[h,w,3] of ``depth`` bits: L of the source samples, the given source-size ab."""
    return quantise(lab_to_srgb(lightness(g, variant), ab), depth, variant)


# ---- the comparisons of the GPU file: (passed, figures)
def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and bool(np.array_equal(got, want)), {}


def close(got, want, tol):
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())
    return err <= tol, {"err": err}


def within_one_level(got, want):
    d = int(np.abs(np.asarray(got).astype(np.int64) - np.asarray(want).astype(np.int64)).max())
    return d <= 1, {"levels": d}


def image16_matches(got, g, ab, variant=None):
    """The 16-bit image against the reference's: equal wherever the reference's s * 65535 is further than EDGE from an integer, at most one
    level off elsewhere, and differing on at most MAX_DIFF_SHARE of the image's pixels."""
    s = lab_to_srgb(lightness(g, variant), ab) * 65535.0
    want = quantise(s / 65535.0, 16, variant) if variant == "round_out" else s.astype(np.uint16)
    d = np.abs(np.asarray(got).astype(np.int64) - want.astype(np.int64))
    far = np.abs(s - np.round(s)) > EDGE
    share = float((d.max(axis=-1) > 0).mean())
    fig = {"levels": int(d.max()), "far_diff": int((d[far] > 0).sum()), "share": share}
    return bool((d[far] == 0).all() and d.max() <= 1 and share <= MAX_DIFF_SHARE), fig
