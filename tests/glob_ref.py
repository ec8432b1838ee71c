"""The reference for the reference-image global hints (idc_global_stats_rgb / idc_set_global_refs / idc_forward_async_rgb_ref), made of code
that is not under test, and the inputs both test files share.

Reference: ``ingest_ref.net_rgb`` (the wrapper's host resize, the rule the kernel's device functions reproduce bit for bit), the oracle's
``rgb2lab``, a float64 mean over every 4x4 block, the nearest of the real ``color_bins.pts_in_hull()`` centres in float64, and the HSV
saturation formula.  A histogram is a count of hard decisions, so the GPU tests compare COUNTS EXACTLY and leave out no block; that is fair
only where the float64 decision is not a rounding matter.  ``stats`` therefore returns the smallest margin -- over all blocks, the gap
between the squared distances to the nearest and the second-nearest centre -- and tests/test_glob_ref_cpu.py asserts ``MARGIN`` for the
very arrays the GPU tests use.

MARGIN = 1e-3: the device rounds the pooled (a, b) to fp32 (|ab| <= 110: half an ulp is 3.8e-6) and the squared distance has slope
2 |delta| <= 24 between neighbouring centres of the 10-spaced grid, about 1e-4 per component; fp32 arithmetic on values <= 150 adds less
than 5e-5; 1e-3 is four times the total.
"""
import functools

import numpy as np

import ingest_ref
from interactive_deep_colorization_amd import color_bins
from oracle import colorspace as ocs

MARGIN = 1e-3
NET = (32, 48)                  # H != W: an h/4 - w/4 swap shows
# the net size itself (the identity), up- and down-scaling both ways, sizes that are no multiple of anything, a strip, one pixel
# (h, w, seed): even seeds are noise, odd ones ramps
SIZES = [(32, 48, 2), (20, 27, 1), (33, 49, 2), (97, 61, 9), (131, 200, 4), (7, 300, 5), (1, 1, 6)]
# what the 64 x 64 handles of the install / pipeline / wrapper tests are given
SIZES64 = [(97, 61, 9), (64, 64, 12), (40, 90, 13), (131, 200, 14)]


def centres():
    return np.ascontiguousarray(color_bins.pts_in_hull(), dtype=np.float32)


def noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def ramp(h, w, seed):
    """Smooth sine colour ramps: real interpolation weights, many bins."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    fy, fx = y / max(h - 1, 1), x / max(w - 1, 1)
    ph = 0.7 * seed
    r = 127.5 + 127.5 * np.sin(2 * np.pi * (1.0 * fx + 0.35 * fy) + ph)
    g = 127.5 + 127.5 * np.sin(2 * np.pi * (0.45 * fx + 1.2 * fy) + 2.1 + ph)
    b = 127.5 + 127.5 * np.sin(2 * np.pi * (0.8 * fx - 0.9 * fy) + 4.2 + 2 * ph)
    return np.clip(np.floor(np.stack([r, g, b], -1) + 0.5), 0, 255).astype(np.uint8)


def make_ref(h, w, seed):
    """(h, w, 3) uint8: noise for even seeds, a ramp for odd ones."""
    return ramp(h, w, seed) if seed % 2 else noise(h, w, seed)


@functools.lru_cache(maxsize=None)
def _refs(key):
    if key == "net":
        out = [make_ref(h, w, s) for h, w, s in SIZES]
    else:
        out = [make_ref(h, w, s) for h, w, s in SIZES64]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def refs_net():
    """The m = 7 references of SIZES for the NET-size handle, mixed noise and ramp (read-only, shared)."""
    return list(_refs("net"))


def refs64():
    """The references of SIZES64 for the 64 x 64 handles (read-only, shared)."""
    return list(_refs("64"))


def stats(src, H, W):
    """-> dict(counts (313,) int64, hist (313,) float32, s_avg float64, margin float64, bins int) of reference ``src`` at net size H x W."""
    net = ingest_ref.net_rgb(np.asarray(src), H, W)
    lab = ocs.rgb2lab(net)
    ab = lab[..., 1:].reshape(H // 4, 4, W // 4, 4, 2).mean(axis=(1, 3))                 # float64 throughout
    c = np.asarray(color_bins.pts_in_hull(), np.float64)
    d = ((ab[:, :, None, :] - c[None, None]) ** 2).sum(-1)
    part = np.partition(d, 1, axis=-1)
    idx = d.argmin(-1)
    counts = np.bincount(idx.ravel(), minlength=313)
    v = net.astype(np.float64) / 255.0
    mx, mn = v.max(-1), v.min(-1)
    sat = np.where(mx > 0, (mx - mn) / np.where(mx > 0, mx, 1), 0.0)
    nblk = (H // 4) * (W // 4)
    return dict(counts=counts, hist=(counts / float(nblk)).astype(np.float32), s_avg=float(sat.mean()),
                margin=float((part[..., 1] - part[..., 0]).min()), bins=int((counts > 0).sum()))


_STATS = {}


def stats_of(key, k, H, W):
    """``stats`` of reference k of ``refs_net()`` (key 'net') or ``refs64()`` (key '64'), computed once per session."""
    kk = (key, k, H, W)
    if kk not in _STATS:
        _STATS[kk] = stats((refs_net() if key == "net" else refs64())[k], H, W)
    return _STATS[kk]


def glob_rows(hists, ref_index, flag=1.0, s_avg=None):
    """(n, 314) glob_ab_313_mask rows (and (n, 2) s_avg_mask rows when ``s_avg`` is given) as the host route builds them: reference
    ref_index[i]'s histogram and the flag, a zero row for -1."""
    n = len(ref_index)
    g = np.zeros((n, 314), np.float32)
    s = np.zeros((n, 2), np.float32)
    for i, r in enumerate(ref_index):
        if r >= 0:
            g[i, :313] = hists[r]
            g[i, 313] = flag
            if s_avg is not None:
                s[i] = (s_avg[r], 1.0)
    return (g, s) if s_avg is not None else g
