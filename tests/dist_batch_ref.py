"""The uncertainty-peak rule of idc_dist_peaks restated with plain loops, from the rule's text in include/ideepcolor.h -- not from the kernel:

  candidates of image i: every cell of ent [n,Hd,Wd] that is not NaN; with a mask [n,H,W] (s = H / Hd), minus the cells whose s x s block of
  the mask holds a non-zero value;
  for k = 0..P-1: the candidate with the smallest ent, ties to the lowest cy * Wd + cx; peaks[i][k] = (cy*s + s/2, cx*s + s/2),
  peak_ent[i][k] = its ent; every candidate with max(|dy|, |dx|) < radius leaves; no candidate left: (-1, -1) and +0.0.

Used by tests/test_dist_batch_cpu.py (the rule's properties) and tests/test_dist_batch_gpu.py (the yardstick of the kernel)."""
import numpy as np


def peaks(ent, P, radius, s, mask=None):
    """-> (peaks (n,P,2) int32, peak_ent (n,P) float32)."""
    ent = np.asarray(ent, np.float32)
    n, Hd, Wd = ent.shape
    out = np.full((n, P, 2), -1, np.int32)
    out_ent = np.zeros((n, P), np.float32)
    for i in range(n):
        e = ent[i].tolist()                               # Python floats: the float32 values, exactly
        cand = [[e[cy][cx] == e[cy][cx] for cx in range(Wd)] for cy in range(Hd)]
        if mask is not None:
            for cy in range(Hd):
                for cx in range(Wd):
                    if np.any(mask[i, cy * s:(cy + 1) * s, cx * s:(cx + 1) * s] != 0):
                        cand[cy][cx] = False
        for k in range(P):
            best = None
            for cy in range(Hd):                          # row-major = ascending cy * Wd + cx: a strict < keeps the lowest index of a tie
                for cx in range(Wd):
                    if cand[cy][cx] and (best is None or e[cy][cx] < e[best[0]][best[1]]):
                        best = (cy, cx)
            if best is None:
                break                                     # every later row stays (-1, -1), 0
            out[i, k] = (best[0] * s + s // 2, best[1] * s + s // 2)
            out_ent[i, k] = ent[i, best[0], best[1]]
            for cy in range(max(best[0] - radius + 1, 0), min(best[0] + radius, Hd)):
                for cx in range(max(best[1] - radius + 1, 0), min(best[1] + radius, Wd)):
                    cand[cy][cx] = False
    return out, out_ent


def cells(pk, s):
    """The grid cells (cy, cx) of the valid rows of one image's peaks (P,2)."""
    return [(int(y) // s, int(x) // s) for y, x in pk if not (y == -1 and x == -1)]
