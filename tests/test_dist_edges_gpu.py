"""GPU checks of the resident-distribution kernels on CRAFTED heads (tests/crafted_heads.py): distributions with exact zeros, bit-equal ties and
one-hot cells, on which every documented tie / zero rule of softmax_nchw_kernel / dist313_kernel's consumers is reached -- dist_entropy_kernel,
dist_decode_kernel, dist_peaks_kernel, suggest_kernel / suggest_batch_kernel, dist_score_kernel / dist_score_finish_kernel.  The sibling files
(test_session_gpu, test_dist_maps_gpu, test_dist_batch_gpu, test_dist_score_gpu) feed them the smooth softmax of seeded random weights only.

A test is one (head, precision, net size, recipe): it loads the crafted head, runs one forward on the resident images, reads ``get_dist`` and
asserts the recipe's PREMISE on it first (counts of exact zeros, bit-equal plateaus, cells equal to 1.0, the mixed recipe's shares; printed),
then walks the kernels.  Handles are shared per (head, precision, size); bf16 runs plateau and mixed only.

Bars: those of the sibling files, none new -- entropy 1e-5 abs, mean decode 2e-2 abs (test_dist_maps_gpu), xent 1e-12 relative
(test_dist_score_gpu); everything else bit for bit: mode decode and conf, peaks against tests/dist_batch_ref.py AND the closed form of a
constant map (the raster lattice of stride r), suggestions with their counts against oracle/session.suggest_colors, the batch against the
single call, target / rank against tests/dist_score_ref.py on the device's own truth_ab with the neighbours ordered by d^2 (no cell excluded),
xent[i] and hits against the documented sums of the device's own maps, the pipelined batch against the blocking calls.
Shapes: 32 x 48 (the 529 grid is 8 x 12 = 96 cells: the second 64-cell workgroup has 32 dead lanes; the 313 grid is 1536 cells: two walks of
the 1024-thread peak kernel) with batch 3, and 64 x 64 with batch 2.
Wall time on an MI355X: 23 s for the 23 tests, the slowest (313 bins, fp32, 32 x 48, uniform: three peak plans of 256 rounds) 1.9 s."""
import numpy as np
import pytest

import crafted_heads as C
import dist_batch_ref as D
import dist_maps_ref as M
import dist_score_ref as S
import eval_ref as E
from interactive_deep_colorization_amd import engine
from oracle import session, weights

pytestmark = pytest.mark.gpu

ENT_TOL, MEAN_TOL, XENT_TOL = 1e-5, 2e-2, 1e-12
FLOOR = -np.log(np.float64(np.finfo(np.float32).tiny))          # xent of a cell whose target bin holds p == 0
_ENG, _BASE, _TRUTH = {}, {}, {}

CASES = [(bins, "fp32", 32, 48, r) for bins in (529, 313) for r in C.RECIPES] + \
        [(bins, "fp32", 64, 64, r) for bins in (529, 313) for r in ("uniform", "plateau", "mixed")] + \
        [(bins, "bf16", 32, 48, r) for bins in (529, 313) for r in ("plateau", "mixed")] + \
        [(bins, "bf16", 64, 64, "mixed") for bins in (529, 313)]


@pytest.fixture(scope="module", autouse=True)
def _forget_the_handles():
    yield
    _ENG.clear()                                                    # tests/conftest.py closes the engines of the module


def _base(bins, make_sd):
    if bins == 529:
        return make_sd(0, "he")
    if bins not in _BASE:
        _BASE[bins] = weights.add_pred313_head(weights.make_state_dict(2, "he", include_class=False), 2)
    return _BASE[bins]


class Case(object):
    pass


def _case(bins, precision, H, W, recipe, make_sd):
    """The shared handle of (head, precision, size) with ``recipe``'s head loaded and one forward of the resident images and hints behind it."""
    key = (bins, precision, H, W)
    if key not in _ENG:
        n = 3 if (H, W) == (32, 48) else 2
        e = engine.HipColorizer(H, W, max_batch=n, precision=precision, dist=bins == 529, dist313=bins == 313)
        e.recipe = None
        _ENG[key] = (e, n)
    e, n = _ENG[key]
    if e.recipe != recipe:
        e.crafted = C.craft(_base(bins, make_sd), bins, recipe)
        e.load_state_dict(e.crafted.sd)
        if bins == 313:
            e.keep_dist(True)
        e.recipe = recipe
    k = Case()
    k.e, k.n, k.bins, k.H, k.W, k.recipe, k.c, k.key = e, n, bins, H, W, recipe, e.crafted, key
    k.s = 4 if bins == 529 else 1
    k.hd, k.wd = H // k.s, W // k.s
    k.centres = S.grid529() if bins == 529 else np.ascontiguousarray(weights.synthetic_ab_centres(2))      # integer coordinates: k-means sums are exact
    k.images = C.images(H, W, n)
    _forward(k)
    k.p = e.get_dist(n)
    k.p.setflags(write=False)
    k.what = "%d %s %dx%d %s" % (bins, precision, H, W, recipe)
    return k


def _forward(k):
    for i, img in enumerate(k.images):
        k.e.set_image_rgb(img, img=i, keep_source=True, want_rgb=False, want_lab=False)
        k.e.set_hints(C.HINTS[i] or [], mode="ab", img=i)
    k.e.forward_resident(k.n, want_rgb=False, want_lab=False)


# ------------------------------------------------------------------------------------------------ the premise, on the device's own distribution
def _premise(k):
    c, p = k.c, k.p
    st_all, st = C.structure(p, c), C.structure(C.interior(k.bins, p), c)
    print("%s: %d cells (%d interior), %d zero bins; zeros exact in %d interior cells, plateaus bit-equal in %d cells, one-hot cells %d, top plateau "
          "in front in %d cells" % (k.what, st_all["cells"], st["cells"], st["zero_bins"], st["zeros"], st_all["ties"], st["one_hot"], st_all["top"]))
    assert st_all["cells"] == k.n * k.hd * k.wd
    assert st["zeros"] == st["cells"], k.what                      # every zero bin exactly 0.0, no other bin 0
    assert st_all["ties"] == st_all["cells"], k.what               # equal biases: bit-equal probabilities, everywhere
    assert st["zero_bins"] == {"uniform": 0, "one_hot": k.bins - 1, "plateau": k.bins - 43, "plateau_lead": k.bins - 44,
                               "mixed": k.bins - 3 - len(c.vary)}[k.recipe]
    assert st["one_hot"] == (st["cells"] if k.recipe == "one_hot" else 0), k.what
    if k.recipe == "mixed":
        share = st_all["top"] / float(st_all["cells"])
        assert 0.25 <= share <= 0.75, (k.what, share)
    else:
        assert st_all["top"] == st_all["cells"], k.what
        inner = C.interior(k.bins, p)
        assert (inner == inner[:1, :, :1, :1]).all(), k.what       # one distribution in every (interior) cell
    if k.recipe == "uniform":
        assert len(np.unique(p)) == 1
    return st_all


def _flat_expected(k):
    """Is the entropy map constant over the WHOLE grid?  The 313 head's border blends a plateau's bias with zero padding."""
    return k.recipe in ("uniform", "one_hot") or (k.bins == 529 and k.recipe != "mixed")


# ------------------------------------------------------------------------------------------------ entropy
def _check_entropy(k):
    ent = k.e.dist_entropy(k.n)
    ref = M.entropy(k.p)
    assert ent.dtype == np.float32 and ent.shape == ref.shape and np.isfinite(ent).all(), k.what          # a cell with zero bins is finite
    err = np.abs(ent - ref).max()
    print("  entropy: max abs err %.3e (range %.4f .. %.4f)" % (err, ref.min(), ref.max()))
    assert err <= ENT_TOL, k.what
    bits = C.interior(k.bins, ent).view(np.uint32)
    if k.recipe != "mixed":
        assert len(np.unique(bits)) == 1, k.what                   # a constant distribution: a bit-constant map
    if k.recipe == "one_hot":
        assert not bits.any(), k.what                              # exactly +0.0
    assert (len(np.unique(ent.view(np.uint32))) == 1) == _flat_expected(k), k.what
    return ent


# ------------------------------------------------------------------------------------------------ decode
def _check_decode(k):
    e, p, c, cen = k.e, k.p, k.c, k.centres
    ab, conf = e.dist_decode(cen, k.n, mode="mode", want_conf=True)
    ab_ref, conf_ref = M.decode_mode(p, cen)
    np.testing.assert_array_equal(ab, ab_ref, err_msg=k.what)
    assert conf.tobytes() == conf_ref.tobytes(), k.what            # conf == p_max bit for bit
    lowest = int(c.top.min())
    front = p[:, lowest] == p.max(axis=1)                          # cells in which the top plateau holds the maximum
    want = np.broadcast_to(cen[lowest].reshape(1, 2, 1, 1), ab.shape)
    assert (ab == want)[np.broadcast_to(front[:, None], ab.shape)].all(), k.what       # ... decode to the LOWEST bin of the plateau
    assert front.all() or k.recipe == "mixed"
    if k.recipe == "uniform":
        assert lowest == 0
    for gamma in (1.0, 13.0):
        mab, mconf = e.dist_decode(cen, k.n, mode="mean", gamma=gamma, want_conf=True)
        ref = M.decode_mean(p, cen, gamma)
        err = np.abs(mab - ref).max()
        print("  mean decode gamma %g: max abs err %.3e" % (gamma, err))
        assert mab.dtype == np.float32 and err <= MEAN_TOL, k.what
        assert mconf.tobytes() == conf_ref.tobytes(), k.what
        if k.recipe == "one_hot":
            inner = C.interior(k.bins, mab)
            assert (inner == cen[c.q0].reshape(1, 2, 1, 1)).all(), k.what                                 # exactly the centre of q0


# ------------------------------------------------------------------------------------------------ peaks
def _lattice(k, P, r, value):
    """The closed form on a constant map: the raster lattice of stride r, then (-1, -1) and +0.0."""
    ny, nx = -(-k.hd // r), -(-k.wd // r)
    m = min(P, ny * nx)
    j = np.arange(m)
    pk = np.full((P, 2), -1, np.int32)
    pk[:m, 0], pk[:m, 1] = (j // nx) * r * k.s + k.s // 2, (j % nx) * r * k.s + k.s // 2
    pe = np.zeros(P, np.float32)
    pe[:m] = value
    return pk, pe, ny * nx


def _check_peaks(k, ent):
    e, n, s = k.e, k.n, k.s
    cells = k.hd * k.wd
    flat = _flat_expected(k)
    plans = [(min(256, -(-k.hd // r) * -(-k.wd // r) + 3), r) for r in (1, 2, 5)] if flat else [(16, 2)]
    for P, r in plans:
        pk, pe = e.dist_peaks(n, P=P, radius=r)
        if flat:
            want, want_e, count = _lattice(k, P, r, ent.flat[0])
            for i in range(n):
                np.testing.assert_array_equal(pk[i], want, err_msg="%s P %d radius %d image %d" % (k.what, P, r, i))
                assert pe[i].tobytes() == want_e.tobytes(), k.what
            if count < P:
                assert (pk[:, count:] == -1).all() and not pe[:, count:].view(np.uint32).any()            # run out: (-1, -1) and +0.0
        if not flat or n * P * cells <= 400000:                    # the plain-loop restatement, where its loops stay short
            ref, ref_e = D.peaks(ent, P, r, s)
            np.testing.assert_array_equal(pk, ref, err_msg=k.what)
            assert pe.tobytes() == ref_e.tobytes(), k.what
    # hinted cells skipped: a mask (set AFTER the forward) that removes cell 0 and a block in the middle
    for i in range(n):
        e.set_hints([(0, 0, 0, 0, 1.0, 1.0), (k.H // 2 - 2, k.W // 2 - 3, k.H // 2 + 1, k.W // 2 + 2, 2.0, 2.0)], mode="ab", img=i)
    mask = np.stack([e.hint_planes(i)[1][0] for i in range(n)])
    P, r = ((-(-k.hd // 2) * -(-k.wd // 2) + 3, 2) if k.bins == 529 else (80, 5)) if flat else (16, 2)
    pk, pe = e.dist_peaks(n, P=P, radius=r, skip_hints=True)
    ref, ref_e = D.peaks(ent, P, r, s, mask)
    np.testing.assert_array_equal(pk, ref, err_msg=k.what + " skip_hints")
    assert pe.tobytes() == ref_e.tobytes(), k.what
    for i in range(n):
        for cy, cx in D.cells(pk[i], s):
            assert mask[i, cy * s:(cy + 1) * s, cx * s:(cx + 1) * s].max() == 0
    if flat:
        assert (pk[:, 0] == (s // 2, s + s // 2)).all(), k.what    # cell 0 is hinted: the lowest candidate is cell 1
    print("  peaks: %s map, %d plans and the masked one" % ("constant" if flat else "varying", len(plans)))


# ------------------------------------------------------------------------------------------------ suggestions
def _check_suggest(k):
    e, p, c, cen, s = k.e, k.p, k.c, k.centres, k.s
    spots = [(0, 0, 0), (k.n - 1, k.H - 1, k.W - 1), (1, 13, 22)]
    if k.recipe == "mixed":                                         # one cell with the plateau in front, one with it behind
        front = p[0, c.top[0]] == p[0].max(axis=0)
        for want in (True, False):
            cy, cx = np.argwhere(front == want)[0]
            spots.append((0, int(cy) * s + s // 2, int(cx) * s))
    combos = {"one_hot": [(K, N, 21 + K) for K in (1, 5, 16) for N in (3, 25000)],
              "uniform": [(5, 25000, 1), (5, 3, 2), (16, 40, 3)],
              "plateau": [(5, 8, C.U0_SEED), (5, 25000, C.U0_SEED), (3, C.U0_I + 1, C.U0_SEED), (3, C.U0_I, C.U0_SEED)],
              "mixed": [(5, 3, 11), (5, 25000, 12), (16, 25000, 13)]}
    combos["plateau_lead"] = combos["plateau"]
    single = {}
    for img, y, x in spots:
        pdf = p[img, :, y // s, x // s]
        np.testing.assert_array_equal(e.dist_at(y, x, img), pdf)
        for K, N, seed in combos[k.recipe]:
            what = "%s image %d (%d, %d) K %d N %d seed %d" % (k.what, img, y, x, K, N, seed)
            got = e.suggest_colors(y, x, cen, K=K, N_draws=N, seed=seed, img=img, want_counts=True)
            ref = session.suggest_colors(pdf, cen, K=K, N=N, seed=seed, return_counts=True)
            np.testing.assert_array_equal(got[2], ref[2], err_msg=what)
            assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes(), what
            assert int(got[2].sum()) == N and not got[2][pdf == 0].any(), what                            # whatever the oracle says
            single[(img, y, x, K, N, seed)] = got
            if k.recipe == "one_hot":
                assert got[1].tolist() == [1.0] + [0.0] * (K - 1) and got[0][0].tolist() == cen[c.q0].tolist() and (got[0][1:] == cen[0]).all(), what
        if k.recipe in ("plateau", "plateau_lead"):                 # the u == 0 draw alone: the first bin with p > 0
            one = single[(img, y, x, 3, C.U0_I + 1, C.U0_SEED)][2].astype(np.int64) - single[(img, y, x, 3, C.U0_I, C.U0_SEED)][2].astype(np.int64)
            first = int(np.flatnonzero(pdf > 0)[0])
            assert first == c.first_live() == (10 if k.recipe == "plateau_lead" else 0)
            assert one.tolist() == np.eye(k.bins, dtype=np.int64)[first].tolist(), k.what
    for K, N, seed in combos[k.recipe][:2]:                         # the batch: the same queries, the empty one in the middle
        queries = [(img, y, x, seed) for img, y, x in spots]
        queries.insert(len(queries) // 2, (1, -1, -1, 5))
        oc, of = e.suggest_colors_batch(queries, cen, K=K, N_draws=N)
        for q, (img, y, x, sd_) in enumerate(queries):
            if (y, x) == (-1, -1):
                assert not oc[q].any() and not of[q].any()
                continue
            one = single[(img, y, x, K, N, seed)]
            assert oc[q].tobytes() == one[0].tobytes() and of[q].tobytes() == one[1].tobytes(), (k.what, q, K, N)
    print("  suggestions: %d spots x %d (K, N, seed), and the batch" % (len(spots), len(combos[k.recipe])))


# ------------------------------------------------------------------------------------------------ score
def _same_score(got, i, ref, what):
    np.testing.assert_array_equal(got.target[i], ref["target"], err_msg=what + " target")
    np.testing.assert_array_equal(got.rank_map[i], ref["rank"], err_msg=what + " rank")
    g, r = got.xent_map[i], ref["xent"]
    rel = np.where(g == r, 0.0, np.abs(g - r) / np.maximum(np.abs(r), np.finfo(np.float64).tiny))
    assert rel.max() <= XENT_TOL, "%s: xent off by %.3g relative" % (what, rel.max())
    return float(rel.max())


def _check_score(k):
    e, n, p, c, cen, s, B = k.e, k.n, k.p, k.c, k.centres, k.s, k.bins
    ranks = (1, B)
    worst, floor_cells = 0.0, 0
    for nn in (1, 2, 16):
        got = e.dist_score(cen, n=n, nn=nn, sigma=5.0, ranks=ranks, want_maps=True)
        if k.key not in _TRUTH:                                     # once per handle: truth_ab is reveal_hints' colour of the cell, bit for bit
            for i in range(n):
                rects = [(cy * s, cx * s, cy * s + s - 1, cx * s + s - 1) for cy in range(k.hd) for cx in range(k.wd)]
                cols = e.reveal_hints(rects, img=i).reshape(k.hd, k.wd, 2).transpose(2, 0, 1)
                assert got.truth_ab[i].tobytes() == np.ascontiguousarray(cols).tobytes(), k.what
                assert E.within_one_ulp(got.truth_ab[i], S.truth(k.images[i], k.H, k.W, s).astype(np.float64)).all(), k.what
            _TRUTH[k.key] = got.truth_ab.copy()
        assert got.truth_ab.tobytes() == _TRUTH[k.key].tobytes()
        for i in range(n):
            ref = S.score(p[i], got.truth_ab[i], cen, nn, 5.0, by="d2")
            worst = max(worst, _same_score(got, i, ref, "%s nn %d image %d" % (k.what, nn, i)))
            assert got.xent[i] == S.image_sum(got.xent_map[i]) and got.hits[i].tolist() == S.hits(got.rank_map[i], ranks)
            assert got.hits[i, 1] == k.hd * k.wd and np.isfinite(got.xent_map[i]).all()
            if nn > 1:
                continue
            t, rank, x = got.target[i].astype(np.int64), got.rank_map[i], got.xent_map[i]
            if k.recipe == "uniform":
                np.testing.assert_array_equal(rank, t)             # all bins tie: the bins of lower index are in front
            zero = p[i] == 0
            dead = np.take_along_axis(zero, t[None], axis=0)[0]     # cells whose target bin holds p == 0
            if dead.any():
                assert (np.abs(x[dead] - FLOOR) <= XENT_TOL * FLOOR).all(), k.what
                below = np.take_along_axis(np.cumsum(zero, axis=0), t[None], axis=0)[0] - 1               # zero bins below the target
                np.testing.assert_array_equal(rank[dead], ((~zero).sum(axis=0) + below)[dead])
            floor_cells += int(dead.sum())
    if k.recipe in ("one_hot", "plateau", "plateau_lead", "mixed"):
        assert floor_cells > 0, k.what
    # a duplicated centre (crafted_heads.duplicated_centres): c[i] = c[j] exactly, i < j, at the colour most cells of image 1 have: j is never the
    # target, and with two neighbours they are (i, j) in that order; the third centre's probability is another one, so skipping the tie would show
    base = e.dist_score(cen, n=n, nn=1, ranks=ranks, want_maps=True).target[1]
    dup, i0, j0, most = C.duplicated_centres(cen, base, ~c.zero, p[1, :, 0, 0])
    pairs = told = 0
    for nn in (1, 2):
        got = e.dist_score(dup, n=n, nn=nn, sigma=5.0, ranks=ranks, want_maps=True)
        assert not (got.target == j0).any(), k.what
        for i in range(n):
            ref = S.score(p[i], got.truth_ab[i], dup, nn, 5.0, by="d2")
            _same_score(got, i, ref, "%s duplicated centre nn %d image %d" % (k.what, nn, i))
            if nn == 2:
                at = ref["q"][..., 0] == i0
                assert (ref["q"][..., 1][at] == j0).all() and (ref["w"][at] == 0.5).all()
                third = S.neighbours(got.truth_ab[i], dup, 3, by="d2")[0][..., 2]
                pairs += int(at.sum())
                told += int((at & (np.take_along_axis(p[i], third[None], axis=0)[0] != p[i, j0])).sum())
    assert pairs >= most and (told > 0 or k.recipe == "uniform"), k.what
    print("  score: largest relative xent difference %.3g; %d cells on the FLT_MIN floor; %d cells with the duplicated pair (%d, %d), the third centre's p differs in %d" %
          (worst, floor_cells, pairs, i0, j0, told))


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("bins,precision,H,W,recipe", CASES)
def test_crafted_head(bins, precision, H, W, recipe, make_sd):
    k = _case(bins, precision, H, W, recipe, make_sd)
    _premise(k)
    ent = _check_entropy(k)
    _check_decode(k)
    _check_suggest(k)
    _check_score(k)
    _check_peaks(k, ent)                                            # last: it paints hints over the resident planes
    np.testing.assert_array_equal(k.e.get_dist(k.n), k.p)          # every call only read the distribution


def test_the_pipelined_taps_equal_the_blocking_calls_on_a_plateau(make_sd):
    """idc_forward_async_dist_score runs the same kernels behind the taps: one batch, every output bit for bit."""
    k = _case(529, "fp32", 32, 48, "plateau", make_sd)
    _premise(k)
    e, n, cen, B = k.e, k.n, k.centres, k.bins
    P, r, K, N = 27, 2, 5, 8
    queries = [(0, 0, 0, C.U0_SEED), (1, -1, -1, 3), (2, k.H - 1, k.W - 1, C.U0_SEED), (1, 13, 22, 9)]
    ent = e.dist_entropy(n)
    pk, pe = e.dist_peaks(n, P=P, radius=r)
    assert (pk[:, 24:] == -1).all() and (pk[:, :24] >= 0).all()     # 4 x 6 lattice points, then run out
    sugg = [e.suggest_colors(y, x, cen, K=K, N_draws=N, seed=seed, img=img) if y >= 0 else (np.zeros((K, 2)), np.zeros(K)) for img, y, x, seed in queries]
    want = e.dist_score(cen, n=n, nn=2, sigma=5.0, ranks=(1, B), want_maps=True)
    b = e.forward_async_dist(0, k.images, C.HINTS[:n], mode="ab", peaks=P, radius=r, queries=queries, K=K, N_draws=N, centres=cen, want_entropy=True,
                             score=dict(centres=cen, nn=2, sigma=5.0, ranks=(1, B), want_maps=True))
    e.wait(0)
    np.testing.assert_array_equal(e.get_dist(n), k.p)
    assert np.array(b.entropy).tobytes() == ent.tobytes()
    np.testing.assert_array_equal(np.array(b.peaks), pk)
    assert np.array(b.peak_ent).tobytes() == pe.tobytes()
    for q, (oc, of) in enumerate(sugg):
        assert np.array(b.sugg_centres)[q].tobytes() == oc.tobytes() and np.array(b.sugg_conf)[q].tobytes() == of.tobytes(), q
    for name in ("xent", "hits", "xent_map", "rank_map", "target", "truth_ab"):
        assert np.asarray(getattr(b.score, name)).tobytes() == np.asarray(getattr(want, name)).tobytes(), name
