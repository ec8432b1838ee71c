"""The reference for the evaluation batches (idc_reveal_hints / idc_forward_async_eval), made of code that is not under test: the net-size
image and its float64 Lab are tests/ingest_ref.py's, a rectangle is clipped as cv2.rectangle clips it, its colour is the float64 mean of
(a, b) over its pixels in row-major order rounded once to float32, the planes are painted in list order (the later hint wins), and the score
is a sum of Python integers.  Also the rectangle lists of the GPU file, in net coordinates, each meaningful on 64 x 64 and on 40 x 72."""
import math

import numpy as np

import ingest_ref

# two 1 x 1 rectangles, a 9 x 9, a 3 x 3 inside it (the later wins), areas 64 and 65 (one wave, one wave plus one)
R1 = [(10, 12, 10, 12), (0, 0, 0, 0), (20, 30, 28, 38), (22, 32, 24, 34), (5, 50, 12, 57), (30, 3, 34, 15)]
# clipped at the origin; clipped at the far corner on 40 x 72 and wholly outside on 64 x 64; outside both; reversed corners
R2 = [(-4, -4, 4, 4), (36, 68, 44, 76), (100, 100, 120, 130), (25, 60, 20, 40)]
# the whole image (4096 / 2880 pixels: many per thread), area 256, area 272
R3 = [(0, 0, 1000, 1000), (1, 1, 16, 16), (2, 20, 17, 36)]
LISTS = [R1, R2, R3, None]


def clip(rect, H, W):
    """(y0, x0, y1, x1) ordered and clipped to the H x W image, or None when it lies wholly outside."""
    y0, y1 = sorted((int(rect[0]), int(rect[2])))
    x0, x1 = sorted((int(rect[1]), int(rect[3])))
    y0, x0, y1, x1 = max(y0, 0), max(x0, 0), min(y1, H - 1), min(x1, W - 1)
    return (y0, x0, y1, x1) if y0 <= y1 and x0 <= x1 else None


def lab_of(src, H, W):
    """[3,H,W] float64 Lab of the net-size image of ``src``."""
    return ingest_ref.net_lab(ingest_ref.net_rgb(src, H, W))


def rect_values(lab, rect):
    """(a values, b values) of a clipped rectangle in row-major order, as Python floats."""
    y0, x0, y1, x1 = rect
    return [[float(v) for v in lab[c, y0:y1 + 1, x0:x1 + 1].ravel()] for c in (1, 2)]


def mean_row_major(values):
    s = 0.0
    for v in values:
        s += v
    return s / len(values)


def reveal(lab, rects):
    """Revealed colours of ``rects`` on the [3,H,W] Lab: (k,2) float64 means (0 for a dropped rectangle) and the list of clipped rectangles."""
    H, W = lab.shape[1:]
    cols = np.zeros((len(rects), 2), np.float64)
    clipped = []
    for k, r in enumerate(rects):
        c = clip(r, H, W)
        clipped.append(c)
        if c is not None:
            cols[k] = [mean_row_major(v) for v in rect_values(lab, c)]
    return cols, clipped


def planes(lab, rects, mask_value):
    """(ab [2,H,W] float64 -- the float32 a kernel may store is np.float32 of it or a float32 neighbour --, mask [1,H,W] float32)."""
    H, W = lab.shape[1:]
    ab, mask = np.zeros((2, H, W), np.float64), np.zeros((1, H, W), np.float32)
    cols, clipped = reveal(lab, rects or [])
    for col, c in zip(cols, clipped):
        if c is None:
            continue
        y0, x0, y1, x1 = c
        ab[:, y0:y1 + 1, x0:x1 + 1] = col[:, None, None]
        mask[0, y0:y1 + 1, x0:x1 + 1] = mask_value
    return ab, mask


def within_one_ulp(got32, want64):
    """got (float32) is np.float32(want) or one of its two float32 neighbours, elementwise."""
    got32 = np.asarray(got32, np.float32)
    w = np.asarray(want64, np.float64).astype(np.float32)
    lo, hi = np.nextafter(w, np.float32(-np.inf)), np.nextafter(w, np.float32(np.inf))
    return (got32 == w) | (got32 == lo) | (got32 == hi)


def sse(result, truth):
    """[3] Python integers: the sum of squared differences per channel of two (h,w,3) uint8 images."""
    d = result.astype(np.int64) - truth.astype(np.int64)
    return [int(sum(int(v) for v in (d[..., c] ** 2).ravel())) for c in range(3)]


def psnr(result, truth):
    """get_result_PSNR's expression (data/colorize_image.py:103-105) on two uint8 images."""
    se = (1. * truth - result) ** 2
    mse = np.mean(se)
    return 20 * np.log10(255. / np.sqrt(mse)) if mse > 0 else math.inf
