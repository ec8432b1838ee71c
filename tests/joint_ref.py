"""The joint bilateral ab upsampling (include/ideepcolor.h states the rule; idc_fullres_rgb with IDC_INTERP_JOINT, idc_fullres_ab,
idc_set_batch_upsample) restated in numpy float64, and the inputs the GPU file runs it on.

The restatement walks the taps in plain Python loops, j outer and i inner as the rule says, and carries every output pixel through them
as one element of a float64 array: per pixel that is the rule's own sequence of operations.  A skipped tap adds +0.0 to the three sums,
which changes no bit.  Colours go through tests/ingest_ref.py's formulas (the oracle's rgb2lab / lab2rgb_transpose).  ``variant`` swaps in
one of the mistakes tests/test_joint_cpu.py shows the 1e-9 comparison would catch."""
import numpy as np

import ingest_ref
from oracle import colorspace as ocs

EPS = 1e-6                      # IDC_JOINT_EPS
DEFAULT = (2, 1.0, 8.0)         # R, sigma_s, sigma_r
CORNERS = [(1, 0.25, 0.5), (4, 8.0, 100.0)]
PARAMS = [(1, 1.0, 8.0), DEFAULT, (4, 1.0, 8.0)] + CORNERS

# the GPU file's shapes: the 32 x 48 handle and its source sizes
H, W = 32, 48
SIZES = [(1, 1), (1, 300), (300, 1), (13, 17), (32, 48), (37, 41), (233, 351)]
L_CENT = 50.0
# (y0, x0, y1, x1, a, b) on the 32 x 48 net: what input_ab holds in the GPU file
HINTS = [(2, 3, 12, 20, 35.0, -50.0), (8, 15, 28, 40, -30.0, 45.0), (20, 2, 30, 10, 70.0, 20.0), (0, 40, 6, 47, -60.0, -15.0)]
# the step edge: a 4x grey source, dark | bright, the edge on the net's grid (x = 96 = 4 * 24) or two source pixels off it; the two halves
# of the net carry ab = -40 and ab = +60
STEP_GREYS, STEP_AB = (30, 230), (-40.0, 60.0)
STEP_HINTS = [(0, 0, H - 1, W // 2 - 1, STEP_AB[0], STEP_AB[0]), (0, W // 2, H - 1, W - 1, STEP_AB[1], STEP_AB[1])]
STEP_BOUND, LINEAR_MISS = 0.1, 30.0


def source(sh, sw):
    """The GPU file's source of one size (ingest_ref.source_image: a crop of the golden photograph where it fits)."""
    return ingest_ref.source_image(sh, sw, 2 * (sh + sw))


def step_source(offset):
    """(4H, 4W, 3) uint8 grey step whose edge lies ``offset`` source pixels to the right of the net's grid line."""
    img = np.empty((4 * H, 4 * W, 3), np.uint8)
    edge = 4 * (W // 2) + offset
    img[:, :edge] = STEP_GREYS[0]
    img[:, edge:] = STEP_GREYS[1]
    return img, edge


def raster(hints, h=H, w=W):
    """[2,h,w] float32: idc_set_hints' planes of a hint list in IDC_HINT_AB mode (inclusive rectangles, the later hint wins)."""
    ab = np.zeros((2, h, w), np.float32)
    for y0, x0, y1, x1, a, b in hints:
        ab[0, y0:y1 + 1, x0:x1 + 1] = a
        ab[1, y0:y1 + 1, x0:x1 + 1] = b
    return ab


def guide(src, h=H, w=W, l_cent=L_CENT, with_l_cent=True):
    """L_lo [h,w] float64 = (double)Lplane + (double)l_cent, Lplane = the fp32 plane the ingestion writes: (float)(L - l_cent) of the
    net-size image (ingest_ref's resize and rgb2lab)."""
    plane = np.float32(ingest_ref.net_lab(ingest_ref.net_rgb(src, h, w))[0] - np.float64(np.float32(l_cent)))
    return plane.astype(np.float64) + (np.float64(np.float32(l_cent)) if with_l_cent else 0.0)


def source_l(src):
    """L [h,w] float64 of the source pixels, as IDC_L_IMAGE computes it."""
    return ocs.rgb2lab(src)[..., 0]


def joint_ab(L, a_lo, b_lo, L_lo, R=2, sigma_s=1.0, sigma_r=8.0, variant=None, want_den=False):
    """The rule: L [h,w] float64 of the source pixels, planes a_lo / b_lo / L_lo [H,W] -> ab [2,h,w] float64 (and the smallest den).
    variant: None, 'corner' (scipy's corner-aligned coordinates), 'replicate' (border taps clamped, not skipped), 'no_eps',
    'swap_f32' (i outer, j inner, float32 sums)."""
    L = np.asarray(L, np.float64)
    a_lo, b_lo, L_lo = (np.asarray(p).astype(np.float64) for p in (a_lo, b_lo, L_lo))
    h, w = L.shape
    Hn, Wn = L_lo.shape
    ys, xs = np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64)
    if variant == "corner":
        u = ys * ((Hn - 1) / (h - 1) if h > 1 else 0.0)
        v = xs * ((Wn - 1) / (w - 1) if w > 1 else 0.0)
    else:
        u = (ys + 0.5) * (np.float64(Hn) / h) - 0.5
        v = (xs + 0.5) * (np.float64(Wn) / w) - 0.5
    j0 = np.floor(u + 0.5).astype(np.int64)
    i0 = np.floor(v + 0.5).astype(np.int64)
    acc = np.float32 if variant == "swap_f32" else np.float64
    num_a, num_b, den = (np.zeros((h, w), acc) for _ in range(3))
    eps = 0.0 if variant == "no_eps" else EPS
    taps = [(dj, di) for dj in range(-R, R + 1) for di in range(-R, R + 1)]
    if variant == "swap_f32":
        taps = [(dj, di) for di in range(-R, R + 1) for dj in range(-R, R + 1)]
    for dj, di in taps:
        j, i = j0 + dj, i0 + di
        inside = ((j >= 0) & (j < Hn))[:, None] & ((i >= 0) & (i < Wn))[None, :]
        jc, ic = np.clip(j, 0, Hn - 1), np.clip(i, 0, Wn - 1)
        if variant == "replicate":
            inside = np.ones_like(inside)
        ws = np.exp(-(((j - u) ** 2)[:, None] + ((i - v) ** 2)[None, :]) / (2.0 * sigma_s * sigma_s))
        d = L - L_lo[jc][:, ic]
        wt = ws * (np.exp(-(d * d) / (2.0 * sigma_r * sigma_r)) + eps)
        wt = np.where(inside, wt, 0.0)
        num_a += (wt * a_lo[jc][:, ic]).astype(acc)
        num_b += (wt * b_lo[jc][:, ic]).astype(acc)
        den += wt.astype(acc)
    with np.errstate(invalid="ignore", divide="ignore"):
        ab = np.stack([num_a / den, num_b / den]).astype(np.float64)
    return (ab, float(den.min())) if want_den else ab


def joint_rgb(src, a_lo, b_lo, L_lo, R=2, sigma_s=1.0, sigma_r=8.0):
    """[h,w,3] uint8: Lab -> RGB of the source's L with the rule's ab."""
    L = source_l(src)
    return ocs.lab2rgb_transpose(L[None], joint_ab(L, a_lo, b_lo, L_lo, R, sigma_s, sigma_r))


def srgb_unquantised(L, ab):
    """[h,w,3] float64 = 255 x the clipped sRGB that lab2rgb_transpose truncates to uint8 (the oracle's formulas, not rounded)."""
    lab = np.concatenate([np.asarray(L, np.float64)[None], ab]).transpose((1, 2, 0))
    return np.clip(ocs.lab2rgb(lab), 0, 1) * 255.0


def near_rounding_edge(L, ab, tol=1e-6):
    """Fraction of the bytes whose unquantised value lies within ``tol`` of an integer, where the last bits of pow could move the byte."""
    s = srgb_unquantised(L, ab)
    inner = (s > tol) & (s < 255.0 - tol)             # a clipped channel sits ON 0 or 255 and cannot move
    return float((inner & (np.abs(s - np.round(s)) < tol)).mean())
