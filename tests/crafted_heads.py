"""Crafted last layers for the two distribution heads: state dicts whose head -- the 1 x 1 conv ``model_class.0`` (529 bins) or
``pred.pred_313`` (313 bins) -- is replaced so that the softmax behind it holds exact zeros, bit-equal ties and one-hot cells, the inputs
for which the resident-distribution kernels document a rule each (include/ideepcolor.h) and which a forward on seeded random weights
never produces.  No device, not a test module; tests/test_dist_edges_cpu.py holds the premises on the oracle, tests/test_dist_edges_gpu.py
on the device's own distribution.

Why the structure is exact in every precision: a zero weight row gives the logit ``sum 0 * x + bias = bias`` (the bias is added in fp32, and
every plateau's bias here is a bfloat16 number as well), so equal biases give bit-equal logits and bit-equal probabilities, and a bias of -1e4
(-9984 as a bfloat16) gives expf(0.2 * (-1e4 - max)) == 0.  On the 313 head the logits pass a bilinear x4 up-sampling first: a convex combination of equal values
in the interior (exact: the weights are multiples of 1/16), a blend with zero padding on the last rows and columns -- there a bias b becomes
a fraction of b, still the same fraction for every bin, so ties hold everywhere and -1e4 stays below -5000.

The kernels split the bins over eight waves in chunks of ceil(B / 8) (67 for 529 bins, 40 for 313): wave w walks [w * chunk, (w + 1) * chunk).
The bin choices below straddle those borders on purpose:

  uniform        weights 0, bias 0: all B bins tie in every cell
  one_hot        weights 0, bias 0 at q0 = 2 * chunk (the first bin of the third wave), -1e4 elsewhere
  plateau        weights 0; top plateau, bias 0: bins chunk - 1, chunk (the last bin of wave 0, the first of wave 1) and B - 1 (the last wave);
                 lower plateau, bias -2: bins 0..9 and 2 * chunk - 15 .. 2 * chunk + 14 (40 bins, across the next border); the rest -1e4
  plateau_lead   the same with the LEADING bins 0..9 zero: the lower plateau's first ten bins are 10..19, and the top plateau has a fourth bin
                 chunk - 8 inside wave 0's walk in front of chunk - 1 (a tie within one wave)
  mixed          the base dict's random rows and biases on every 13th (529) / 8th (313) bin: about 40 bins that vary from cell
                 to cell; a tie plateau of three zero-row bins chunk - 1, chunk, chunk + 1 at the bias MIXED_BIAS[bins]; the rest -1e4.  The bias
                 sits near the median over the cells of the largest random logit, so that the plateau holds the cell's maximum in a good share of
                 the cells and loses it in a good share: both files measure the shares and hold them at a quarter each way at the least."""
import numpy as np

HEADS = {529: "model_class.0", 313: "pred.pred_313"}
NEG = -1.0e4
LOWER = -2.0
RECIPES = ("uniform", "one_hot", "plateau", "plateau_lead", "mixed")
# A bfloat16 number between the medians of the cell's largest random logit at 32 x 48 and at 64 x 64 (the oracle's shares of cells in which
# the plateau is in front: 529 head 0.65 and 0.36, 313 head -- whose up-sampling smooths the random logits -- 0.62 and 0.40).
MIXED_BIAS = {529: 8.25, 313: 8.25}


# A draw that is exactly 0.0: lowbias32(U0_I * 0x9E3779B9 + U0_SEED * 0x85EBCA6B + 0x165667B1) >> 8 == 0 (found by a numpy sweep over 2^22 seeds for
# each small i; tests/test_dist_edges_cpu.py evaluates the hash).  With N > U0_I draws of seed U0_SEED, draw U0_I has u == 0.
U0_SEED, U0_I = 286241, 3


def chunk(bins):
    return (bins + 7) // 8


class Crafted(object):
    """sd: the state dict; bias [B] float32; zero [B] bool: the bins whose probability is exactly 0 in every cell; plateaus: lists of bins with
    one bias each, the highest bias first (bit-equal probabilities within a list); vary: the bins with a random row; q0: one_hot's bin."""

    def __init__(self, sd, bins, recipe, bias, plateaus, vary, q0=None):
        self.sd, self.bins, self.recipe, self.bias = sd, bins, recipe, bias
        self.plateaus = [np.asarray(p, np.int64) for p in plateaus]
        self.vary = np.asarray(vary, np.int64)
        self.q0 = q0
        self.zero = bias == np.float32(NEG)
        self.top = self.plateaus[0]

    def first_live(self):
        return int(np.flatnonzero(~self.zero)[0])


def plateau_bins(bins, lead=False):
    """(top, lower) bin lists of the two plateau recipes."""
    c = chunk(bins)
    top = [c - 1, c, bins - 1]
    if lead:
        top = [c - 8] + top
    lower = list(range(10, 20) if lead else range(0, 10)) + list(range(2 * c - 15, 2 * c + 15))
    assert not set(top) & set(lower) and len(lower) == 40
    return top, lower


def mixed_bins(bins):
    """(vary, plateau) bin lists of the mixed recipe."""
    c = chunk(bins)
    vary = list(range(0, bins, 13)) if bins == 529 else list(range(4, bins, 8))
    plateau = [c - 1, c, c + 1]
    assert not set(vary) & set(plateau)
    return vary, plateau


def craft(base_sd, bins, recipe, mixed_bias=None):
    """A shallow copy of ``base_sd`` with the head layer of ``bins`` bins replaced after ``recipe`` -> Crafted."""
    key = HEADS[bins]
    w0, b0 = np.asarray(base_sd[key + ".weight"], np.float32), np.asarray(base_sd[key + ".bias"], np.float32)
    assert w0.shape[0] == bins and b0.shape == (bins,)
    w = np.zeros_like(w0)
    b = np.full(bins, NEG, np.float32)
    vary, q0 = [], None
    if recipe == "uniform":
        b[:] = 0.0
        plateaus = [list(range(bins))]
    elif recipe == "one_hot":
        q0 = 2 * chunk(bins)
        assert 0 < q0 < bins - 1
        b[q0] = 0.0
        plateaus = [[q0]]
    elif recipe in ("plateau", "plateau_lead"):
        top, lower = plateau_bins(bins, recipe == "plateau_lead")
        b[top] = 0.0
        b[lower] = LOWER
        plateaus = [top, lower]
    elif recipe == "mixed":
        vary, plateau = mixed_bins(bins)
        w[vary] = w0[vary]
        b[vary] = b0[vary]
        b[plateau] = MIXED_BIAS[bins] if mixed_bias is None else mixed_bias
        plateaus = [plateau]
    else:
        raise ValueError(recipe)
    sd = dict(base_sd)
    sd[key + ".weight"], sd[key + ".bias"] = w, b
    return Crafted(sd, bins, recipe, b, plateaus, vary, q0)


def interior(bins, a):
    """The cells in which a constant recipe is constant: all of them on the 529 head, all but the last four rows and columns on the 313 head
    (whose x4 up-sampling blends those with zero padding).  ``a`` [..., Hd, Wd] -> a view."""
    return a if bins == 529 else a[..., :-4, :-4]


def structure(p, c):
    """What a distribution p [n,B,Hd,Wd] float32 shows of the recipe's structure, as counts over all n * Hd * Wd cells:
    zeros: cells in which every zero bin of the recipe is exactly 0.0 and no other bin is; ties: cells in which every plateau is bit-equal;
    one_hot: cells that hold a 1.0; top: cells in which the first plateau holds the cell's maximum."""
    p = np.asarray(p)
    assert p.dtype == np.float32 and p.shape[1] == c.bins
    z = (p == 0)
    zeros = (z[:, c.zero].all(axis=1) & ~z[:, ~c.zero].any(axis=1))
    ties = np.ones(zeros.shape, bool)
    for bins_ in c.plateaus:
        ties &= (p[:, bins_] == p[:, bins_[:1]]).all(axis=1)
    one_hot = (p == 1.0).any(axis=1)
    top = p[:, c.top[0]] == p.max(axis=1)
    return dict(cells=int(zeros.size), zeros=int(zeros.sum()), ties=int(ties.sum()), one_hot=int(one_hot.sum()), top=int(top.sum()),
                zero_bins=int(c.zero.sum()))


def duplicated_centres(centres, targets, live, pdf):
    """Centres [B,2] with one duplicated pair for the score's tie rule (neighbours of equal d^2 go to the lower index): c[i] = c[j] exactly,
    i < j, at the centre of the most frequent bin of ``targets`` (that bin's own centre moves far away).  The probabilities belong to the bin
    INDEX, so i and j are chosen for them: j the highest bin of ``live`` (p > 0), i the highest bin below it whose probability in ``pdf`` [B]
    is another one (j - 1 where all are equal).  With two neighbours a cell at that colour has (i, j), in that order; a device that skipped
    the equal d^2 and took the third centre would read another probability.  -> (centres, i, j, cells of ``targets`` at that colour)."""
    vals, counts = np.unique(targets, return_counts=True)
    t0 = int(vals[np.argmax(counts)])
    j = int(np.flatnonzero(live)[-1])
    other = np.flatnonzero(pdf[:j] != pdf[j])
    i = int(other[-1]) if len(other) else j - 1
    dup = np.array(centres, np.float32)
    if t0 not in (i, j):
        dup[t0] = (1000.0, 1000.0)
    dup[i] = dup[j] = centres[t0]
    return dup, i, j, int(counts.max())


# ---- the inputs both files run the crafted heads on: tests/ragged_ref.py's seeded images through the documented ingestion, painted hints
def images(H, W, n):
    import ragged_ref as R
    sizes = [(37, 41), (H, W), (130, 97)]
    return [R.image(sh, sw, 400 + j) for j, (sh, sw) in enumerate(sizes)][:n]


HINTS = [None, [(4, 6, 20, 30, 30.0, -40.0), (10, 12, 30, 40, -25.0, 55.0)], [(1, 2, 9, 20, 60.0, 10.0)]]


def planes(H, W, n):
    """(L_mc [n,1,H,W], ab [n,2,H,W], mask [n,1,H,W]) of ``images`` and HINTS, on the CPU (tests/ingest_ref.py, oracle/session.py)."""
    import ingest_ref
    from oracle import session
    L, ab, mask = [], [], []
    for img, h in zip(images(H, W, n), HINTS):
        lab = ingest_ref.net_lab(ingest_ref.net_rgb(img, H, W))
        a, m = session.raster_hints(h or [], H, W, mode="ab")
        L.append(lab[:1] - 50.0); ab.append(a); mask.append(m)
    return np.stack(L).astype(np.float32), np.stack(ab), np.stack(mask)
