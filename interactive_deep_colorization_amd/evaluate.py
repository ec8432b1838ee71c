"""The paper's evaluation on the engine: PSNR against the ground-truth colour image as a function of the number of revealed points
(Zhang et al., "Real-Time User-Guided Image Colorization with Learned Deep Priors", SIGGRAPH 2017: the PSNR-versus-points
figure).  The metric is ``ColorizeImageBase.get_result_PSNR`` (``data/colorize_image.py:98-108``); the simulated user is described in the
paper only ("simulating user interactions": the reference repository ships no code for it).  The device does the work: ``HipColorizer.evaluate_images`` reveals
each point's colour from the image and returns 24 bytes per image."""
import math

import numpy as np


def psnr_from_sse(sse, h, w):
    """``get_result_PSNR``'s expression from the integer sums: ``20 log10(255 / sqrt(mean squared error))`` over the h x w x 3 values, in
    float64; ``sse`` is the (3,) per-channel sums (or their total).  ``inf`` for an exact match."""
    total = int(np.asarray(sse, dtype=np.uint64).astype(object).sum())
    if total == 0:
        return float("inf")
    mse = float(total) / float(3 * int(h) * int(w))
    return 20.0 * math.log10(255.0 / math.sqrt(mse))


def simulate_points(H, W, count, rs):
    """``count`` revealed points of an H x W image as the paper simulates a user: the centre is drawn from a 2-D Gaussian at the
    image centre with sigma = (H/4, W/4), redrawn until it lies inside the image; the patch side P is uniform in 1..9; the colour (not made
    here) is the image's mean ab under the patch.  Returns (count, 4) int32 rows (y0, x0, y1, x1), corners inclusive -- ``put_point``'s
    extent ``[c - p, c + p]`` for an odd P = 2p + 1; an even P has its extra row and column towards the origin.  A patch may reach over the
    border: the engine clips it.  ``rs``: a ``numpy.random.RandomState``; point k consumes the same draws whatever ``count`` is, so the list
    for a smaller count is a prefix of the list for a larger one."""
    rows = np.zeros((int(count), 4), np.int32)
    for k in range(int(count)):
        while True:
            cy = int(np.floor(rs.normal(H / 2.0, H / 4.0)))
            cx = int(np.floor(rs.normal(W / 2.0, W / 4.0)))
            if 0 <= cy < H and 0 <= cx < W:
                break
        P = int(rs.randint(1, 10))
        y0, x0 = cy - P // 2, cx - P // 2
        rows[k] = (y0, x0, y0 + P - 1, x0 + P - 1)
    return rows


def psnr_sweep(engine, images, counts=(0, 1, 2, 5, 10, 20, 50, 100), seed=0, out="net", batch=None):
    """The PSNR-versus-points table of ``images`` (a list of (h,w,3) uint8 ground-truth images) on ``engine`` (a ``HipColorizer`` with
    weights): (len(counts), len(images)) float64.  Image j's points are ``simulate_points(engine.H, engine.W, max(counts),
    RandomState(seed + j))`` and count c uses the first c of them, so a row differs from the next only by the points added."""
    images = list(images)
    most = max(counts) if len(counts) else 0
    points = [simulate_points(engine.H, engine.W, most, np.random.RandomState(seed + j)) for j in range(len(images))]
    table = np.zeros((len(counts), len(images)), np.float64)
    for r, c in enumerate(counts):
        items = ((img, pts[:c]) for img, pts in zip(images, points))
        for j, (psnr, _) in enumerate(engine.evaluate_images(items, batch=batch, out=out, mode="reveal")):
            table[r, j] = psnr
    return table
