"""The reference for the distribution scores (idc_dist_score / idc_forward_async_dist_score), made of code that is not under test: the
definitions of include/ideepcolor.h restated in numpy float64.  Everything that the definitions order -- the truth's fold, the neighbours, the
sums over j, the per-image sum -- is walked in that order, one step per loop pass (a pass works on all cells at once, which changes no cell's
arithmetic).

  truth       tests/eval_ref.py's Lab of the net-size image; a cell's s x s values t = dy*s + dx folded by halves, / count, one rounding to float32
  neighbours  d^2 = da*da + db*db, d = sqrt(d^2) in float64 from the float32 values; a FULL stable sort of d (ties keep the lower index);
              by="d2": of d^2 itself, the device's documented order (tests/test_dist_edges_gpu.py compares every cell with it)
  weights     exp(-d_j^2 / (2 sigma^2)) / their sum (j ascending); exactly 1 for nn == 1
  xent        0 - sum_j w_j * log(max(p[q_j], FLT_MIN)), j ascending
  rank        #{q : p[q] > p[t] || (p[q] == p[t] && q < t)}
  xent[i]     blocks of 64 consecutive cells (padded with +0.0) folded by halves; 64 running sums over the block sums l, l+64, ... ascending from
              +0.0; those folded by halves
and each cell's margins d_2 - d_1 and d_(nn+1) - d_nn: a cell whose margin is below MARGIN is left out of the per-cell comparisons (the
device's float32 truth can differ from another float32 truth by an ulp, 4e-6 at |ab| <= 128, and orders by d^2; MARGIN is 25 x that ulp)."""
import numpy as np

import eval_ref

MARGIN = 1e-4
EXCLUDED_CAP = 0.002            # at most 0.2 % of the cells of an input may be left out
FLT_MIN = float(np.finfo(np.float32).tiny)


def grid529():
    axis = np.arange(-110, 120, 10)
    return np.ascontiguousarray(np.array(np.meshgrid(axis, axis)).reshape((2, 529)).T.astype(np.float32))


def fold_halves(v):
    """v [..., 2^k] float64 -> [...]: element c is added to element c + half, for half = 2^(k-1), ..., 1."""
    v = np.array(v, np.float64)
    while v.shape[-1] > 1:
        half = v.shape[-1] // 2
        v = v[..., :half] + v[..., half:]
    return v[..., 0]


def truth(src, H, W, s):
    """[2,H/s,W/s] float32: the ground-truth (a, b) of every cell of the net-size image of ``src``."""
    lab = eval_ref.lab_of(src, H, W)
    hd, wd = H // s, W // s
    out = np.zeros((2, hd, wd), np.float32)
    for c in (0, 1):
        cells = lab[1 + c].reshape(hd, s, wd, s).transpose(0, 2, 1, 3).reshape(hd, wd, s * s)      # t = dy*s + dx
        out[c] = ((0.0 + fold_halves(cells)) / float(s * s)).astype(np.float32)
    return out


def neighbours(truth_ab, centres, nn, by="d"):
    """truth_ab [2,...] float32, centres [B,2] float32 -> (q [...,nn] int, d2 [...,nn], margins [...,2] = (d_2 - d_1, d_(nn+1) - d_nn; inf
    where there is no such centre), second [...] = q_2 or -1).  by="d": the stable sort of d = sqrt(d^2), the definition; by="d2": the stable
    sort of d^2 itself, the device's documented rule -- the same order except where two DIFFERENT d^2 round to one square root (then "d" sees a
    tie and takes the lower index, "d2" the smaller d^2)."""
    assert by in ("d", "d2")
    t = np.asarray(truth_ab, np.float32).astype(np.float64)
    c = np.asarray(centres, np.float32).astype(np.float64)
    da, db = t[0][..., None] - c[:, 0], t[1][..., None] - c[:, 1]
    d2 = da * da + db * db
    d = np.sqrt(d2)
    order = np.argsort(d if by == "d" else d2, axis=-1, kind="stable")
    ds = np.take_along_axis(d, order, axis=-1)
    B = c.shape[0]
    inf = np.full(ds.shape[:-1], np.inf)
    m1 = ds[..., 1] - ds[..., 0] if B > 1 else inf
    m2 = ds[..., nn] - ds[..., nn - 1] if B > nn else inf
    q = order[..., :nn]
    return q, np.take_along_axis(d2, q, axis=-1), np.stack([m1, m2], axis=-1), (order[..., 1] if B > 1 else np.full(ds.shape[:-1], -1))


def weights(d2, sigma):
    """d2 [...,nn] -> w [...,nn]: NNEncode.encode_points_mtx_nd's Gaussian weights, normalised; exactly 1 for nn == 1."""
    nn = d2.shape[-1]
    if nn == 1:
        return np.ones_like(d2)
    sig = float(np.float32(sigma))
    e = np.exp(-d2 / (2.0 * (sig * sig)))
    total = np.zeros(d2.shape[:-1])
    for j in range(nn):
        total = total + e[..., j]
    return e / total[..., None]


def rank_of(p, t, tie=True):
    """p [B,...] float32, t [...] -> the number of bins in front of t."""
    pt = np.take_along_axis(p, t[None], axis=0)[0]
    q = np.arange(p.shape[0]).reshape((-1,) + (1,) * (p.ndim - 1))
    before = p > pt
    if tie:
        before = before | ((p == pt) & (q < t))
    return before.sum(axis=0).astype(np.int32)


def score(dist, truth_ab, centres, nn=1, sigma=5.0, tie=True, by="d"):
    """One image: dist [B,Hd,Wd] float32, truth_ab [2,Hd,Wd] float32 -> dict(target, rank int32 [Hd,Wd]; xent float64 [Hd,Wd]; margins
    [Hd,Wd,2]; second [Hd,Wd]; w [Hd,Wd,nn]; q [Hd,Wd,nn]).  ``by``: the neighbours' order, see ``neighbours``."""
    dist = np.asarray(dist, np.float32)
    q, d2, margins, second = neighbours(truth_ab, centres, nn, by)
    w = weights(d2, sigma)
    acc = np.zeros(q.shape[:-1])
    for j in range(nn):
        pj = np.take_along_axis(dist, q[..., j][None], axis=0)[0]
        acc = acc + w[..., j] * np.log(np.maximum(pj, np.float32(FLT_MIN)).astype(np.float64))
    t = q[..., 0]
    return dict(target=t.astype(np.int32), rank=rank_of(dist, t, tie), xent=0.0 - acc, margins=margins, second=second, w=w, q=q)


def image_sum(xent_map):
    """xent[i] from image i's cell values, in the documented order."""
    v = np.asarray(xent_map, np.float64).ravel()
    nblk = (v.size + 63) // 64
    cells = np.zeros(nblk * 64)
    cells[:v.size] = v
    part = fold_halves(cells.reshape(nblk, 64))
    lanes = np.zeros(64)
    for k0 in range(0, nblk, 64):
        chunk = part[k0:k0 + 64]
        lanes[:chunk.size] = lanes[:chunk.size] + chunk
    return float(fold_halves(lanes))


def hits(rank_map, ranks):
    return [int((np.asarray(rank_map) < r).sum()) for r in ranks]


def excluded(ref):
    """The cells left out of the per-cell comparisons: a margin below MARGIN."""
    return ref["margins"].min(axis=-1) < MARGIN


def compare(got, ref, what=""):
    """The per-cell comparisons: got = dict(target, rank, xent) of one image against ``score``'s dict.  Exact target and rank and xent within
    1e-12 relative on the cells that are not excluded; on an excluded cell the target is one of the two candidates.  -> the largest relative
    xent difference seen."""
    out = excluded(ref)
    assert out.mean() <= EXCLUDED_CAP, "%s: %d of %d cells excluded" % (what, out.sum(), out.size)
    keep = ~out
    np.testing.assert_array_equal(np.asarray(got["target"])[keep], ref["target"][keep], err_msg=what + " target")
    assert ((np.asarray(got["target"])[out] == ref["target"][out]) | (np.asarray(got["target"])[out] == ref["second"][out])).all(), what
    np.testing.assert_array_equal(np.asarray(got["rank"])[keep], ref["rank"][keep], err_msg=what + " rank")
    g, r = np.asarray(got["xent"], np.float64)[keep], ref["xent"][keep]
    rel = np.abs(g - r) / np.maximum(np.abs(r), np.finfo(np.float64).tiny)
    rel = np.where(g == r, 0.0, rel)
    worst = float(rel.max()) if rel.size else 0.0
    assert worst <= 1e-12, "%s: xent off by %.3g relative" % (what, worst)
    return worst
