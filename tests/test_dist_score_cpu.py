"""CPU checks of the distribution scores (idc_dist_score / idc_forward_async_dist_score; HipColorizer.dist_score / forward_async_dist(score=) /
score_images; evaluate.likelihood_sweep): the restatement tests/dist_score_ref.py (the GPU file's yardstick) against sklearn's nearest
neighbours and the reference's NNEncode expression, its summation order, the exclusion cap on every input of the GPU file, a mutation check of
the comparisons, the ABI, the marshalling on a recording library, and the generators on stub engines."""
import ctypes
import os
import re

import numpy as np
import pytest

import dist_score_ref as S
import ragged_ref as R
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import color_bins, engine, evaluate

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hull():
    return np.ascontiguousarray(np.asarray(color_bins.pts_in_hull(), np.float32))


def _random_truth(rs, hd, wd):
    return (rs.rand(2, hd, wd) * 180.0 - 90.0).astype(np.float32)


def _random_dist(rs, B, hd, wd, levels=0):
    """Probabilities over B bins per cell; ``levels`` > 0 quantises them so that equal probabilities abound."""
    z = rs.rand(B, hd, wd).astype(np.float32) ** 8
    if levels:
        z = np.ceil(z * levels) / np.float32(levels)
    return (z / z.sum(axis=0, keepdims=True)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("nn", [1, 5, 10, 16])
def test_neighbours_and_weights_equal_sklearn_and_the_nnencode_expression(nn):
    """color_quantization.py:7-33: NearestNeighbors(n_neighbors=NN, algorithm='ball_tree').fit(cc); (dists, inds) = kneighbors(pts);
    wts = exp(-dists**2 / (2 * sigma**2)); wts = wts / sum(wts, axis=1)."""
    from sklearn.neighbors import NearestNeighbors
    cc = _hull()
    assert cc.shape == (313, 2)
    rs = np.random.RandomState(nn)
    truth = _random_truth(rs, 24, 40)
    q, d2, margins, _ = S.neighbours(truth, cc, nn)
    w = S.weights(d2, 5.0)
    pts = truth.reshape(2, -1).T.astype(np.float64)
    dists, inds = NearestNeighbors(n_neighbors=nn, algorithm="ball_tree").fit(cc.astype(np.float64)).kneighbors(pts)
    wts = np.exp(-dists ** 2 / (2 * 5.0 ** 2))
    wts = wts / np.sum(wts, axis=1)[:, np.newaxis]
    clear = (margins.reshape(-1, 2).min(axis=1) >= S.MARGIN)
    assert clear.mean() > 0.99
    qf, wf = q.reshape(-1, nn), w.reshape(-1, nn)
    # the same neighbour SET and the same nearest one wherever no margin is a near-tie; the same weight per neighbour
    assert (qf[clear, 0] == inds[clear, 0]).all()
    for a, b, wa, wb in zip(qf[clear], inds[clear], wf[clear], wts[clear]):
        assert sorted(a) == sorted(b)
        np.testing.assert_allclose(wa[np.argsort(a)], wb[np.argsort(b)], rtol=1e-12, atol=0)
    np.testing.assert_allclose(np.sqrt(d2.reshape(-1, nn))[clear][:, 0], dists[clear][:, 0], rtol=1e-12)
    assert abs(wf.sum(axis=1) - 1.0).max() < 1e-14


def test_one_neighbour_weighs_exactly_one_and_ties_go_to_the_lower_index():
    cc = S.grid529()
    truth = np.zeros((2, 1, 3), np.float32)
    truth[:, 0, 0] = (5.0, 0.0)             # halfway between two centres of the grid: a tie in d
    truth[:, 0, 1] = (5.0, 5.0)             # the middle of four
    truth[:, 0, 2] = (-110.0, 110.0)        # a centre itself
    q, d2, margins, second = S.neighbours(truth, cc, 1)
    w = S.weights(d2, 5.0)
    assert w.tobytes() == np.ones((1, 3, 1)).tobytes()
    assert w.tobytes() == S.weights(d2, 1e-3).tobytes()           # whatever sigma: no 0 / 0 for a far centre
    lower = [min(k for k in range(529) if tuple(cc[k]) in want) for want in ({(0.0, 0.0), (10.0, 0.0)}, {(0.0, 0.0), (10.0, 0.0), (0.0, 10.0), (10.0, 10.0)})]
    assert q[0, :2, 0].tolist() == lower and margins[0, 0, 0] == 0 and margins[0, 1, 0] == 0 and d2[0, 2, 0] == 0
    q4 = S.neighbours(truth, cc, 4)[0][0, 1]
    assert q4.tolist() == sorted(q4.tolist())                     # four equal distances: ascending index


def test_rank_counts_the_bins_in_front_with_the_tie_rule():
    p = np.array([0.1, 0.3, 0.3, 0.1, 0.2], np.float32).reshape(5, 1, 1)
    for t, want in ((0, 3), (1, 0), (2, 1), (3, 4), (4, 2)):
        assert S.rank_of(p, np.array([[t]])).tolist() == [[want]]
    assert S.rank_of(p, np.array([[2]]), tie=False).tolist() == [[0]]
    flat = np.full((7, 2, 2), np.float32(1 / 7.0))
    np.testing.assert_array_equal(S.rank_of(flat, np.array([[0, 3], [6, 1]])), [[0, 3], [6, 1]])


def test_the_cross_entropy_floor_is_finite_and_a_sure_head_scores_zero():
    cc = S.grid529()
    truth = np.zeros((2, 1, 2), np.float32)
    truth[:, 0, 1] = (20.0, -30.0)
    dist = np.zeros((529, 1, 2), np.float32)
    t = S.neighbours(truth, cc, 1)[0][0, :, 0]
    dist[t[1], 0, 1] = 1.0                                         # cell 1: all mass on the true bin; cell 0: none anywhere
    r = S.score(dist, truth, cc, 1, 5.0)
    assert r["xent"][0, 1] == 0.0 and not np.signbit(r["xent"][0, 1]) and r["rank"][0, 1] == 0
    assert r["xent"][0, 0] == -np.log(np.float64(np.finfo(np.float32).tiny)) and np.isfinite(r["xent"][0, 0])
    assert r["rank"][0, 0] == t[0]                                 # all equal: the bins of lower index are in front


def test_the_image_sum_folds_in_the_documented_order():
    rs = np.random.RandomState(5)
    for cells in (1, 63, 64, 65, 180, 4096, 64 * 64 + 1, 64 * 130 + 7):
        v = rs.rand(cells) * 10.0 ** rs.randint(-3, 4, cells)
        # the order, spelt out with Python floats
        nblk = (cells + 63) // 64
        padded = [float(x) for x in v] + [0.0] * (nblk * 64 - cells)

        def fold(vals):
            vals = list(vals)
            half = len(vals) // 2
            while half:
                vals = [vals[c] + vals[c + half] for c in range(half)]
                half //= 2
            return vals[0]
        part = [fold(padded[k * 64:(k + 1) * 64]) for k in range(nblk)]
        lanes = [0.0] * 64
        for k, x in enumerate(part):
            lanes[k % 64] = lanes[k % 64] + x
        assert S.image_sum(v) == fold(lanes)
        assert abs(S.image_sum(v) - float(np.sum(v))) <= 1e-12 * float(np.sum(v))
    assert S.hits(np.array([[0, 1, 4], [5, 0, 528]]), (1, 5, 529)) == [2, 4, 6]


# ------------------------------------------------------------------------------------------------ the exclusion cap
@pytest.mark.parametrize("H,W", [(64, 64), (40, 72)])
def test_at_most_a_fifth_of_a_percent_of_the_cells_of_the_gpu_inputs_is_left_out(H, W):
    """Every input of tests/test_dist_score_gpu.py: the 7 MIXED images with seeds 400 + j on both handles, the 529 grid at H/4 x W/4 and the
    313 centres at H x W, nn in {1, 5, 16}."""
    images = [R.image(sh, sw, 400 + j) for j, (sh, sw) in enumerate(R.sizes(R.MIXED, H, W))]
    for centres, s in ((S.grid529(), 4), (_hull(), 1)):
        truths = [S.truth(img, H, W, s) for img in images]
        for nn in (1, 5, 16):
            out = total = 0
            for t in truths:
                m = S.neighbours(t, centres, nn)[2]
                assert np.isfinite(m).all() and (m >= 0).all()
                out += int((m.min(axis=-1) < S.MARGIN).sum())
                total += m.shape[0] * m.shape[1]
            assert total == 7 * (H // s) * (W // s)
            assert out <= S.EXCLUDED_CAP * total, "%d bins nn %d: %d of %d cells excluded" % (len(centres), nn, out, total)


def test_the_truth_of_a_cell_is_the_reveal_rule_on_its_rectangle():
    import eval_ref as E
    img = R.image(37, 41, 402)
    lab = E.lab_of(img, 40, 72)
    t4, t1 = S.truth(img, 40, 72, 4), S.truth(img, 40, 72, 1)
    assert t4.shape == (2, 10, 18) and t1.shape == (2, 40, 72) and t4.dtype == np.float32
    np.testing.assert_array_equal(t1, lab[1:].astype(np.float32))
    for cy, cx in ((0, 0), (3, 7), (9, 17)):
        cols, _ = E.reveal(lab, [(cy * 4, cx * 4, cy * 4 + 3, cx * 4 + 3)])          # row-major mean: the same value up to the order of 16 additions
        assert E.within_one_ulp(t4[:, cy, cx], cols[0]).all()
        vals = [float(v) for v in lab[1, cy * 4:cy * 4 + 4, cx * 4:cx * 4 + 4].ravel()]
        tree = ((((vals[0] + vals[8]) + (vals[4] + vals[12])) + ((vals[2] + vals[10]) + (vals[6] + vals[14]))) +
                (((vals[1] + vals[9]) + (vals[5] + vals[13])) + ((vals[3] + vals[11]) + (vals[7] + vals[15]))))
        assert t4[0, cy, cx] == np.float32(tree / 16.0)


# ------------------------------------------------------------------------------------------------ the comparisons catch a wrong device
@pytest.mark.parametrize("B,nn", [(529, 1), (313, 5), (313, 16)])
def test_the_comparisons_catch_a_dropped_tie_rule_swapped_ab_and_a_wrong_sigma(B, nn):
    rs = np.random.RandomState(B + nn)
    cc = S.grid529() if B == 529 else _hull()
    truth = _random_truth(rs, 12, 20)
    dist = _random_dist(rs, B, 12, 20, levels=6)                    # quantised: equal probabilities in every cell
    ref = S.score(dist, truth, cc, nn, 5.0)
    assert S.compare(dict(target=ref["target"], rank=ref["rank"], xent=ref["xent"]), ref) == 0.0
    mutants = {"no tie rule": S.score(dist, truth, cc, nn, 5.0, tie=False),
               "swapped (a, b)": S.score(dist, truth[::-1], cc, nn, 5.0),
               "swapped centres": S.score(dist, truth, cc[:, ::-1], nn, 5.0),
               "sigma 10": S.score(dist, truth, cc, nn, 10.0)}
    for name, m in mutants.items():
        if name == "sigma 10" and nn == 1:
            assert m["xent"].tobytes() == ref["xent"].tobytes()    # one neighbour: sigma plays no part
            continue
        with pytest.raises(AssertionError):
            S.compare(dict(target=m["target"], rank=m["rank"], xent=m["xent"]), ref, name)
    off = dict(target=ref["target"], rank=ref["rank"], xent=ref["xent"] * (1.0 + 4e-12))
    with pytest.raises(AssertionError):
        S.compare(off, ref)
    assert S.compare(dict(off, xent=ref["xent"] * (1.0 + 4e-16)), ref) <= 1e-15


# ------------------------------------------------------------------------------------------------ ABI
def test_the_symbols_structs_and_constants_match_the_header():
    header = open(os.path.join(REPO, "include", "ideepcolor.h")).read()
    declared = set(re.findall(r"\b(idc_[a-z0-9_]+)\s*\(", header))
    lib = N.load()
    for sym, argc in (("idc_dist_score", 5), ("idc_forward_async_dist_score", 20)):
        assert sym in declared and sym in N.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
        assert len(getattr(lib, sym).argtypes) == argc
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % sym, header).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == argc
    assert re.search(r"typedef struct idc_dist_score_spec \{ int32_t nn; float sigma; int32_t n_ranks; int32_t ranks\[8\]; \} idc_dist_score_spec;", header)
    assert ctypes.sizeof(N.DistScoreSpec) == 44 and [f[0] for f in N.DistScoreSpec._fields_] == ["nn", "sigma", "n_ranks", "ranks"]
    assert (N.DistScoreSpec.sigma.offset, N.DistScoreSpec.n_ranks.offset, N.DistScoreSpec.ranks.offset) == (4, 8, 12)
    body = re.search(r"typedef struct idc_dist_score_out \{(.*?)\} idc_dist_score_out;", header, re.S).group(1)
    names = re.findall(r"\*\s*([a-z_]+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == ["xent", "hits", "xent_map", "rank_map", "target", "truth_ab"]
    by_offset = sorted(N.DistScoreOut._fields_, key=lambda f: getattr(N.DistScoreOut, f[0]).offset)
    assert [f[0] for f in by_offset] == names and ctypes.sizeof(N.DistScoreOut) == 48
    assert re.search(r"#define IDC_SCORE_MAX_NN 16\b", header) and N.IDC_SCORE_MAX_NN == 16
    assert re.search(r"#define IDC_SCORE_MAX_RANKS 8\b", header) and N.IDC_SCORE_MAX_RANKS == 8
    # the existing taps block keeps its layout, and the version does not move: the feature is additive
    assert ctypes.sizeof(N.DistTaps) == 96 and len(lib.idc_forward_async_dist.argtypes) == 17 and lib.idc_version() == 2


def test_a_call_without_a_handle_is_an_invalid_argument():
    lib = N.load()
    spec, out = engine.score_spec(), N.DistScoreOut()
    x = np.zeros(1, np.float64)
    out.xent = x.ctypes.data
    c = np.zeros((529, 2), np.float32)
    cp = c.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.idc_dist_score(None, 1, ctypes.byref(spec), cp, ctypes.byref(out)) == -1
    px = np.zeros(3, np.uint8)
    one = (N.RefImage * 1)()
    one[0].rgb, one[0].h, one[0].w = px.ctypes.data, 1, 1
    assert lib.idc_forward_async_dist_score(None, 0, 1, one, None, None, 0, 1.0, 0.0, 50.0, 0, None, None, None, None, None, None,
                                            ctypes.byref(spec), cp, ctypes.byref(out)) == -1


# ------------------------------------------------------------------------------------------------ marshalling
class _Recorder(object):
    def __init__(self, bins=529):
        self.calls, self.bins = [], bins

    def idc_dist_bins(self, h):
        return self.bins

    @staticmethod
    def _spec(s):
        return (s.nn, s.sigma, s.n_ranks, list(s.ranks))

    @staticmethod
    def _out(o):
        return {f[0]: getattr(o, f[0]) for f in N.DistScoreOut._fields_}

    def idc_dist_score(self, *a):
        centres = np.ctypeslib.as_array(a[3], (self.bins, 2)).copy()
        self.calls.append(("score", a[1], self._spec(a[2]._obj), centres, self._out(a[4]._obj)))
        return 0

    def idc_forward_async_dist(self, *a):
        self.calls.append(("dist", a))
        return 0

    def idc_forward_async_dist_score(self, *a):
        centres = np.ctypeslib.as_array(a[18], (self.bins, 2)).copy()
        self.calls.append(("dist_score", a, None if a[16] is None else a[16]._obj, self._spec(a[17]._obj), centres, self._out(a[19]._obj)))
        return 0


class _Pool(object):
    def take(self, shape, dtype):
        return np.zeros(shape, dtype)


def _engine_over(lib):
    e = engine.HipColorizer.__new__(engine.HipColorizer)
    e.lib, e._h, e.H, e.W, e._in_flight, e._pool, e.max_batch = lib, ctypes.c_void_p(1), 8, 16, {}, _Pool(), 8
    e.close = lambda: None
    return e


def _images():
    return [np.full((5, 7, 3), 1, np.uint8), np.full((1, 1, 3), 2, np.uint8), np.full((9, 4, 3), 3, np.uint8)]


def test_dist_score_marshals_the_spec_and_the_outputs():
    lib = _Recorder()
    e = _engine_over(lib)
    centres = np.arange(1058, dtype=np.float64).reshape(529, 2)
    res = e.dist_score(centres, n=3, nn=5, sigma=2.5, ranks=(1, 5, 10))
    _, n, spec, c, out = lib.calls[0]
    assert n == 3 and spec == (5, 2.5, 3, [1, 5, 10, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(c, centres.astype(np.float32))
    assert res.xent.shape == (3,) and res.xent.dtype == np.float64 and out["xent"] == res.xent.ctypes.data
    assert res.hits.shape == (3, 3) and res.hits.dtype == np.uint32 and out["hits"] == res.hits.ctypes.data
    assert all(out[k] is None for k in ("xent_map", "rank_map", "target", "truth_ab")) and res.xent_map is None and res.cells == 2 * 4
    res = e.dist_score(centres, want_maps=True, ranks=())
    _, n, spec, c, out = lib.calls[1]
    assert n == 1 and spec == (1, 5.0, 0, [0] * 8) and out["hits"] is None and res.hits.shape == (1, 0)
    assert res.xent_map.shape == (1, 2, 4) and res.xent_map.dtype == np.float64 and out["xent_map"] == res.xent_map.ctypes.data
    assert res.rank_map.dtype == np.int32 and res.target.dtype == np.int32 and res.truth_ab.shape == (1, 2, 2, 4) and res.truth_ab.dtype == np.float32
    assert (out["rank_map"], out["target"], out["truth_ab"]) == (res.rank_map.ctypes.data, res.target.ctypes.data, res.truth_ab.ctypes.data)
    res.xent[...] = 16.0
    res.hits = np.array([[4, 8]], np.uint32)
    assert res.mean().tolist() == [2.0] and res.rates().tolist() == [[0.5, 1.0]]
    with pytest.raises(ValueError):
        e.dist_score(centres, ranks=range(1, 10))
    with pytest.raises(ValueError):
        e.dist_score(centres[:313])
    e = _engine_over(_Recorder(313))
    assert e.dist_score(np.zeros((313, 2)), n=2, want_maps=True).truth_ab.shape == (2, 2, 8, 16)


def test_forward_async_dist_marshals_the_score_and_is_unchanged_without_it():
    lib = _Recorder()
    e = _engine_over(lib)
    imgs = _images()
    centres = np.arange(1058, dtype=np.float32).reshape(529, 2)
    e.forward_async_dist(0, imgs, None, peaks=2)
    assert lib.calls[0][0] == "dist" and len(lib.calls[0][1]) == 17          # score=None: the existing entry point, the existing arguments
    res = e.forward_async_dist(1, imgs, [[(0, 0, 1, 1)], None, None], mode="reveal", peaks=2, radius=1, want_entropy=True,
                               score=dict(centres=centres, nn=5, sigma=3.0, ranks=(1, 5), want_maps=True))
    _, a, t, spec, c, out = lib.calls[1]
    assert len(a) == 20 and (a[1], a[2], a[6]) == (1, 3, N.IDC_HINT_REVEAL) and t is not None and (t.n_peaks, t.radius) == (2, 1)
    assert t.entropy == res.entropy.ctypes.data and spec == (5, 3.0, 2, [1, 5, 0, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(c, centres)
    sc = res.score
    assert sc.xent.shape == (3,) and sc.hits.shape == (3, 2) and sc.xent_map.shape == (3, 2, 4) and sc.truth_ab.shape == (3, 2, 2, 4) and sc.cells == 8
    assert (out["xent"], out["hits"], out["xent_map"], out["rank_map"], out["target"], out["truth_ab"]) == \
        (sc.xent.ctypes.data, sc.hits.ctypes.data, sc.xent_map.ctypes.data, sc.rank_map.ctypes.data, sc.target.ctypes.data, sc.truth_ab.ctypes.data)
    assert e._in_flight[1][3] is res
    # no other tap asked for: taps is NULL and only the score runs
    res = e.forward_async_dist(0, imgs, None, peaks=0, score=dict(centres=centres))
    _, a, t, spec, c, out = lib.calls[2]
    assert a[16] is None and t is None and spec == (1, 5.0, 2, [1, 5, 0, 0, 0, 0, 0, 0]) and res.peaks is None and res.score.xent_map is None
    assert out["xent_map"] is None and a[14] is None and a[12] is None
    for bad in (dict(nn=1), dict(centres=centres, k=3)):
        with pytest.raises(ValueError):
            e.forward_async_dist(0, imgs, None, score=bad)


# ------------------------------------------------------------------------------------------------ the generators on stub engines
class _StubEngine(engine.HipColorizer):
    """forward_async_dist over recorded calls.  'The device' answers at the slot's wait: image v = image[0,0,0] gets the xent sum 8 v (8 cells:
    mean v), hits (v, 2 v) and sse (v, 2v, 3v)."""

    def __init__(self, H, W, max_batch):
        self.H, self.W, self.max_batch = H, W, max_batch
        self._pool = _Pool()
        self.calls = []
        self.busy = {}

    def close(self):
        pass

    def _dist_grid(self):
        return (self.H // 4, self.W // 4)

    def forward_async_dist(self, slot, images, hints, **kw):
        assert slot not in self.busy, "slot %d reused before its wait" % slot
        n = len(images)
        res = engine.DistBatch()
        res.sse = np.zeros((n, 3), np.uint64) if kw.get("want_sse") else None
        res.score, _ = engine.score_buffers(n, self._dist_grid(), len(kw["score"]["ranks"]), False, self._pool.take)
        self.calls.append(("run", slot, [tuple(a.shape) for a in images], [None if h is None else [tuple(int(v) for v in r) for r in h] for h in hints], dict(kw)))
        self.busy[slot] = (res, [int(a[0, 0, 0]) for a in images])
        return res

    def wait(self, slot):
        self.calls.append(("wait", slot))
        if slot in self.busy:
            res, vals = self.busy.pop(slot)
            for i, v in enumerate(vals):
                res.score.xent[i] = 8.0 * v
                res.score.hits[i] = [(k + 1) * v for k in range(res.score.hits.shape[1])]
                if res.sse is not None:
                    res.sse[i] = (v, 2 * v, 3 * v)


def _items(count):
    rs = np.random.RandomState(3)
    return [np.full((int(rs.randint(1, 9)), int(rs.randint(1, 9)), 3), k, np.uint8) for k in range(count)]


@pytest.mark.parametrize("count,batch", [(1, 4), (4, 4), (5, 4), (11, 3), (6, None)])
def test_score_images_groups_alternates_slots_and_keeps_the_order(count, batch):
    e = _StubEngine(8, 16, 5)
    imgs = _items(count)
    rect = [(0, 0, 1, 1)]
    items = [a if k % 2 == 0 else (a, rect) for k, a in enumerate(imgs)]
    centres = np.zeros((529, 2), np.float32)
    got = list(e.score_images(iter(items), centres, batch=batch, nn=5, sigma=2.0, ranks=(1, 5), want_psnr=count % 2 == 1))
    assert len(got) == count and not e.busy
    for g, (mean, hits, psnr) in enumerate(got):
        assert mean == float(g) and hits.tolist() == [g, 2 * g]
        assert psnr == (evaluate.psnr_from_sse(np.array([g, 2 * g, 3 * g], np.uint64), 8, 16) if count % 2 == 1 else None)
    b = e.max_batch if batch is None else batch
    runs = [c for c in e.calls if c[0] == "run"]
    assert [len(c[2]) for c in runs] == [min(b, count - j) for j in range(0, count, b)]
    assert [c[1] for c in runs] == [j & 1 for j in range(len(runs))]
    assert [h for c in runs for h in c[3]] == [None if k % 2 == 0 else rect for k in range(count)]
    for c in runs:
        kw = c[4]
        assert kw["mode"] == "reveal" and kw["peaks"] == 0 and kw["want_sse"] == (count % 2 == 1) and kw.get("queries") is None
        assert kw["score"] == dict(centres=centres, nn=5, sigma=2.0, ranks=(1, 5)) and kw["score"]["centres"] is centres
    assert [c[1] for c in e.calls if c[0] == "wait"] == [j & 1 for j in range(len(runs))]
    for j in range(2, len(runs)):                                   # a wait between two uses of a slot
        assert ("wait", j & 1) in e.calls[e.calls.index(runs[j - 2]) + 1:e.calls.index(runs[j])]


def test_score_images_waits_for_both_slots_when_the_consumer_stops_early():
    e = _StubEngine(8, 16, 2)
    gen = e.score_images(iter(_items(9)), np.zeros((529, 2), np.float32), batch=2)
    next(gen)
    assert sorted(e.busy) == [1]
    gen.close()
    assert not e.busy
    with pytest.raises(ValueError):
        list(e.score_images(iter(_items(1)), np.zeros((529, 2), np.float32), batch=3))
    with pytest.raises(ValueError):
        list(e.score_images(iter([np.zeros((4, 4), np.uint8)]), np.zeros((529, 2), np.float32)))


def test_the_likelihood_sweep_uses_the_random_user_of_the_psnr_sweep():
    e = _StubEngine(64, 64, 3)
    imgs = _items(7)
    centres = np.zeros((529, 2), np.float32)
    counts = (0, 1, 5)
    xent, rates = evaluate.likelihood_sweep(e, imgs, centres, counts=counts, seed=3, nn=10, sigma=4.0, ranks=(1, 5, 20), batch=3)
    assert xent.shape == (3, 7) and rates.shape == (3, 7, 3) and not e.busy
    for r in range(3):
        np.testing.assert_array_equal(xent[r], np.arange(7) * 8.0 / 256.0)
        np.testing.assert_array_equal(rates[r], np.arange(7)[:, None] * np.array([1.0, 2.0, 3.0]) / 256.0)
    points = [evaluate.simulate_points(64, 64, 5, np.random.RandomState(3 + j)) for j in range(7)]
    runs = [c for c in e.calls if c[0] == "run"]
    assert len(runs) == 9
    for r, c in enumerate(counts):                                  # pass r reveals the first counts[r] points of psnr_sweep(strategy='random')'s lists
        seen = [h for run in runs[3 * r:3 * r + 3] for h in run[3]]
        assert seen == [[tuple(int(v) for v in q) for q in p[:c]] for p in points]
        for run in runs[3 * r:3 * r + 3]:
            assert run[4]["mode"] == "reveal" and run[4]["score"] == dict(centres=centres, nn=10, sigma=4.0, ranks=(1, 5, 20))
