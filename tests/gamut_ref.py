"""float64 restatement of the reference's ``data/lab_gamut.py`` (``abGrid.update_gamut`` :66-78, ``snap_ab`` :28-52) for the tests.

Built on ``oracle.colorspace.rgb2lab`` / ``lab2rgb`` and plain numpy loops written from the reference's text; it never imports
the package's ``lab_gamut`` or ``colorspace``.  Besides the results it returns what decides them -- per grid point the Lab
distance ``d`` and the unquantised ``s = 255 * clip(rgb)``, per colour the ``dif`` of every round and the unrounded final
``s`` -- so that a test can tell an input on a knife edge (``d`` at the threshold, ``s`` at a truncation or rounding edge)
from a wrong formula.  Results are cached: the CPU and GPU tests share one computation per input.
"""
import functools

import numpy as np

from oracle import colorspace as ocs

L_VALUES = (27.5, 50.0, 72.5, 100.0)                 # the batch of the GPU test; the CPU test adds 0
GRIDS = ((110, 1), (110, 10), (5, 3), (1, 1))        # (gamut_size, D)
SNAP_COLOURS = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)] + [(128, 128, 128), (255, 128, 0), (1, 2, 3)]
SNAP_LS = (0.0, 5.0, 50.0, 95.0, 100.0)
T_ROUNDS = 20


def grid_axis(gamut_size, D):
    return np.arange(-gamut_size, gamut_size + D, D)


@functools.lru_cache(maxsize=None)
def gamut(L, gamut_size, D):
    """update_gamut(L) on abGrid(gamut_size, D) -> dict: pts_rgb (A,B,3) u8, mask (A,B) bool, masked_rgb (A,B,3) u8, d (A,B) f64,
    s (A,B,3) f64.  Row i is a = axis[i], column j is b = axis[j]."""
    axis = grid_axis(gamut_size, D)
    A = len(axis)
    lab = np.empty((A, A, 3), np.float64)
    for i in range(A):
        for j in range(A):
            lab[i, j] = (L, axis[i], axis[j])
    s = 255 * np.clip(ocs.lab2rgb(lab), 0, 1)
    pts = s.astype('uint8')
    back = ocs.rgb2lab(pts)
    d = np.sqrt(((lab - back) ** 2).sum(axis=2))
    mask = d < 1.0
    masked = pts.copy()
    masked[~mask] = 255
    out = dict(pts_rgb=pts, mask=mask, masked_rgb=masked, d=d, s=s)
    for v in out.values():
        v.setflags(write=False)
    return out


def snap(L, rgb):
    """snap_ab(L, rgb) -> dict: rgb (3,) u8 [return_type 'rgb'], lab (3,) f64 ['lab'], iters, difs (one per round run), s (3,) f64 =
    the final clip(rgb) * 255 before rounding."""
    lab = ocs.rgb2lab(np.array(rgb, np.uint8).reshape(1, 1, 3)).reshape(3)
    difs = []
    for _ in range(T_ROUNDS):
        lab[0] = L                                   # L is overwritten here only: the value that leaves the loop keeps the round trip's L
        old = lab
        tmp = np.clip(ocs.lab2rgb(old.reshape(1, 1, 3)).reshape(3), 0, 1)
        lab = ocs.rgb2lab(tmp.reshape(1, 1, 3)).reshape(3)
        difs.append(float(np.sum(np.abs(lab - old))))
        if difs[-1] < 1:
            break
    s = np.clip(ocs.lab2rgb(lab.reshape(1, 1, 3)).reshape(3), 0, 1) * 255
    out = np.round(s).astype('uint8')
    return dict(rgb=out, lab=ocs.rgb2lab(out.reshape(1, 1, 3)).reshape(3), iters=len(difs), difs=difs, s=s)


def snap_inputs():
    """The colour set of the tests: the corner set at five lightnesses (55 pairs) + 2048 seeded pairs -> ls (2103,) f64, rgbs (2103,3) u8."""
    ls = [l for l in SNAP_LS for _ in SNAP_COLOURS]
    cs = [c for _ in SNAP_LS for c in SNAP_COLOURS]
    rs = np.random.RandomState(0)
    for _ in range(2048):
        ls.append(rs.uniform(0, 100))
        cs.append(tuple(rs.randint(0, 256, 3)))
    return np.array(ls, np.float64), np.array(cs, np.uint8)


@functools.lru_cache(maxsize=None)
def snap_set():
    """snap() of every pair of snap_inputs() -> dict of arrays: rgb (n,3) u8, lab (n,3), iters (n,), s (n,3), and difs (list of lists)."""
    ls, cs = snap_inputs()
    r = [snap(float(l), c) for l, c in zip(ls, cs)]
    out = dict(ls=ls, rgbs=cs, rgb=np.array([x['rgb'] for x in r]), lab=np.array([x['lab'] for x in r]),
               iters=np.array([x['iters'] for x in r], np.int32), s=np.array([x['s'] for x in r]), difs=[x['difs'] for x in r])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
