"""The paper's evaluation on the engine: PSNR against the ground-truth colour image as a function of the number of revealed points
(Zhang et al., "Real-Time User-Guided Image Colorization with Learned Deep Priors", SIGGRAPH 2017: the PSNR-versus-points
figure).  The metric is ``ColorizeImageBase.get_result_PSNR`` (``data/colorize_image.py:98-108``); the simulated user is described in the
paper only ("simulating user interactions": the reference repository ships no code for it).  The device does the work: ``HipColorizer.evaluate_images`` reveals
each point's colour from the image and returns 24 bytes per image.  ``psnr_sweep(strategy='uncertain')`` draws the same curve for a user who
clicks where the model is least sure (``HipColorizer.forward_async_dist``: the uncertainty peaks come from the device too)."""
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


def guided_rects(peaks, half, H, W):
    """The patches a guided user reveals at uncertainty peaks: rows (y - half, x - half, y + half, x + half) of ``peaks`` (k,2) (y, x),
    clipped to the H x W image, corners inclusive; the (-1, -1) rows an image reports once it ran out of cells are dropped.  (k',4) int32."""
    peaks = np.asarray(peaks, np.int64).reshape(-1, 2)
    peaks = peaks[~((peaks[:, 0] == -1) & (peaks[:, 1] == -1))]
    half = int(half)
    rows = np.stack([np.clip(peaks[:, 0] - half, 0, H - 1), np.clip(peaks[:, 1] - half, 0, W - 1),
                     np.clip(peaks[:, 0] + half, 0, H - 1), np.clip(peaks[:, 1] + half, 0, W - 1)], axis=1)
    return rows.astype(np.int32)


def _sweep_uncertain(engine, images, counts, out, batch, half, radius):
    """``psnr_sweep``'s guided user: one pipelined pass per count over all images on both slots; between passes the host only appends
    the rectangles of the peaks the pass reported."""
    counts = [int(c) for c in counts]
    if any(b < a for a, b in zip(counts, counts[1:])):
        raise ValueError("strategy 'uncertain' needs ascending counts")
    batch = engine.max_batch if batch is None else int(batch)
    if not 1 <= batch <= engine.max_batch:
        raise ValueError("batch %d outside 1..%d" % (batch, engine.max_batch))
    H, W = engine.H, engine.W
    rects = [np.zeros((0, 4), np.int32) for _ in images]
    table = np.zeros((len(counts), len(images)), np.float64)
    steps = ([(None, 0)] if counts and counts[0] > 0 else []) + [(r, c) for r, c in enumerate(counts)]     # (table row | None, points during the pass)
    for si, (row, have) in enumerate(steps):
        more = steps[si + 1][1] - have if si + 1 < len(steps) else 0
        pending = [None, None]

        def finish(slot):
            engine.wait(slot)
            (res, first, sizes), pending[slot] = pending[slot], None
            for i, (h, w) in enumerate(sizes):
                if row is not None:
                    table[row, first + i] = psnr_from_sse(np.array(res.sse[i]), h, w)
                if more:
                    rects[first + i] = np.concatenate([rects[first + i], guided_rects(np.array(res.peaks[i])[:more], half, H, W)])

        try:
            nb = 0
            for first in range(0, len(images), batch):
                slot = nb & 1
                if pending[slot] is not None:
                    finish(slot)
                group = images[first:first + batch]
                res = engine.forward_async_dist(slot, group, [[tuple(int(v) for v in r) for r in rects[first + i]] for i in range(len(group))],
                                                mode="reveal", out=out, want_sse=True, peaks=more, radius=radius, skip_hints=True)
                pending[slot] = (res, first, [g.shape[:2] if out == "source" else (H, W) for g in group])
                nb += 1
            for slot in (nb & 1, (nb + 1) & 1):     # the older batch first
                if pending[slot] is not None:
                    finish(slot)
        finally:
            for slot in (0, 1):
                if pending[slot] is not None:
                    pending[slot] = None
                    engine.wait(slot)
    return table, rects


def psnr_sweep(engine, images, counts=(0, 1, 2, 5, 10, 20, 50, 100), seed=0, out="net", batch=None, strategy="random", half=1, radius=2,
               return_rects=False):
    """The PSNR-versus-points table of ``images`` (a list of (h,w,3) uint8 ground-truth images) on ``engine`` (a ``HipColorizer`` with
    weights): (len(counts), len(images)) float64.  Image j's points are ``simulate_points(engine.H, engine.W, max(counts),
    RandomState(seed + j))`` and count c uses the first c of them, so a row differs from the next only by the points added.
    ``strategy='uncertain'`` (an engine with a distribution head; ascending counts): a user who clicks where the model is least sure.  Going
    from count c_k to c_(k+1), image j reveals ``guided_rects`` (peak +- ``half``) of the first c_(k+1) - c_k uncertainty peaks (``dist_peaks``
    with ``radius``, hinted cells skipped) of the forward that ran with c_k points -- ``forward_async_dist`` on both slots, the host only
    appending rectangles between passes; an image that runs out of cells keeps fewer points than the count.  ``seed`` is not used.
    ``return_rects``: also the list of each image's final (k,4) rectangles."""
    images = list(images)
    if strategy == "uncertain":
        table, rects = _sweep_uncertain(engine, images, counts, out, batch, half, radius)
        return (table, rects) if return_rects else table
    if strategy != "random":
        raise ValueError("strategy %r is not 'random' or 'uncertain'" % (strategy,))
    most = max(counts) if len(counts) else 0
    points = [simulate_points(engine.H, engine.W, most, np.random.RandomState(seed + j)) for j in range(len(images))]
    table = np.zeros((len(counts), len(images)), np.float64)
    for r, c in enumerate(counts):
        items = ((img, pts[:c]) for img, pts in zip(images, points))
        for j, (psnr, _) in enumerate(engine.evaluate_images(items, batch=batch, out=out, mode="reveal")):
            table[r, j] = psnr
    return (table, points) if return_rects else table


def likelihood_sweep(engine, images, centres, counts=(0, 1, 2, 5, 10, 20, 50, 100), seed=0, nn=1, sigma=5.0, ranks=(1, 5), batch=None):
    """How revealed hints sharpen the distribution: the likelihood-versus-points table of ``images`` on ``engine`` (a ``HipColorizer`` with a
    distribution head and weights), from ``HipColorizer.score_images``.  The simulated user is ``psnr_sweep(strategy='random')``'s: image j's
    points are ``simulate_points(engine.H, engine.W, max(counts), RandomState(seed + j))`` and count c reveals the first c of them.
    Returns ``(xent, rates)``: xent (len(counts), len(images)) float64 = the mean cross-entropy of the image's cells against the ground truth
    encoded over its ``nn`` nearest ``centres`` (B,2) with ``sigma``; rates (len(counts), len(images), len(ranks)) float64 = the share of
    cells whose true bin is among the head's ranks[j] most probable.  Row means over the images are the curve."""
    images = list(images)
    most = max(counts) if len(counts) else 0
    points = [simulate_points(engine.H, engine.W, most, np.random.RandomState(seed + j)) for j in range(len(images))]
    hd, wd = engine._dist_grid()
    xent = np.zeros((len(counts), len(images)), np.float64)
    rates = np.zeros((len(counts), len(images), len(ranks)), np.float64)
    for r, c in enumerate(counts):
        items = ((img, pts[:c]) for img, pts in zip(images, points))
        for j, (mean, hits, _) in enumerate(engine.score_images(items, centres, batch=batch, nn=nn, sigma=sigma, ranks=ranks, mode="reveal")):
            xent[r, j] = mean
            rates[r, j] = np.asarray(hits, np.float64) / float(hd * wd)
    return xent, rates
