"""CPU checks of the distribution batches (idc_dist_peaks / idc_suggest_colors_batch / idc_forward_async_dist; HipColorizer.dist_peaks /
suggest_colors_batch / forward_async_dist / suggest_images; evaluate.guided_rects and psnr_sweep(strategy='uncertain')): the properties of the
peak rule as tests/dist_batch_ref.py restates it (the GPU file's yardstick), the ABI, the marshalling on a recording library, and the two
generators on stub engines."""
import ctypes
import os
import re

import numpy as np
import pytest

import dist_batch_ref as D
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import engine, evaluate

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the peak rule
def _random_map(rs, n, Hd, Wd, levels, nan_share):
    """Entropy-like maps (negative) on a few levels, so that exact ties abound, with NaNs sprinkled in."""
    ent = -rs.randint(1, levels + 1, (n, Hd, Wd)).astype(np.float32) / np.float32(4.0)
    ent[rs.rand(n, Hd, Wd) < nan_share] = np.nan
    return ent


def _random_mask(rs, n, H, W, rects):
    mask = np.zeros((n, H, W), np.float32)
    for i in range(n):
        for _ in range(rects):
            y, x = rs.randint(0, H), rs.randint(0, W)
            mask[i, y:y + rs.randint(1, 6), x:x + rs.randint(1, 6)] = 1.0 if rs.rand() < 0.5 else 110.0
    return mask


def _vectorised(ent, P, radius, s, mask):
    """The same rule a second way, whole-array numpy: remaining = candidates not within the radius of an earlier peak; the next peak is the
    first flat index at which ent equals the minimum over the remaining cells."""
    n, Hd, Wd = ent.shape
    yy, xx = np.mgrid[0:Hd, 0:Wd]
    out = np.full((n, P, 2), -1, np.int32)
    for i in range(n):
        left = ~np.isnan(ent[i])
        if mask is not None:
            left &= ~(mask[i].reshape(Hd, s, Wd, s) != 0).any(axis=(1, 3))
        for k in range(P):
            if not left.any():
                break
            at = int(np.flatnonzero(left & (ent[i] == ent[i][left].min()))[0])
            cy, cx = divmod(at, Wd)
            out[i, k] = (cy * s + s // 2, cx * s + s // 2)
            left &= np.maximum(np.abs(yy - cy), np.abs(xx - cx)) >= radius
    return out


@pytest.mark.parametrize("Hd,Wd,s", [(16, 16, 4), (10, 18, 4), (12, 20, 1), (1, 7, 1)])
def test_the_restated_rule_has_the_properties_the_header_states(Hd, Wd, s):
    rs = np.random.RandomState(Hd * 100 + Wd)
    ties = masked_away = ran_out = 0
    for levels, nan_share, rects in ((3, 0.0, 0), (5, 0.1, 3), (40, 0.3, 6), (2, 0.9, 2)):
        ent = _random_map(rs, 3, Hd, Wd, levels, nan_share)
        mask = _random_mask(rs, 3, Hd * s, Wd * s, rects) if rects else None
        for P, radius in ((1, 1), (8, 2), (16, 4), (40, 1)):
            pk, pe = D.peaks(ent, P, radius, s, mask)
            assert pk.shape == (3, P, 2) and pk.dtype == np.int32 and pe.shape == (3, P) and pe.dtype == np.float32
            np.testing.assert_array_equal(pk, _vectorised(ent, P, radius, s, mask))
            for i in range(3):
                cells = D.cells(pk[i], s)
                k = len(cells)
                assert (pk[i, k:] == -1).all() and not pe[i, k:].any() and not np.signbit(pe[i, k:]).any()      # once out, out for good: (-1, -1), +0
                assert (pk[i, :k] >= 0).all()
                vals = [ent[i, cy, cx] for cy, cx in cells]
                assert not np.isnan(vals).any() and pe[i, :k].tobytes() == np.array(vals, np.float32).tobytes()
                assert all(a <= b for a, b in zip(vals, vals[1:]))                                               # most uncertain first
                for a in range(k):
                    for b in range(a + 1, k):
                        assert max(abs(cells[a][0] - cells[b][0]), abs(cells[a][1] - cells[b][1])) >= radius
                        if vals[a] == vals[b] and radius == 1:                                                  # a tie nothing else decides: lowest index first
                            assert cells[a][0] * Wd + cells[a][1] < cells[b][0] * Wd + cells[b][1]
                            ties += 1
                if mask is not None:
                    for cy, cx in cells:
                        assert not mask[i, cy * s:(cy + 1) * s, cx * s:(cx + 1) * s].any()
                    unmasked = D.cells(D.peaks(ent[i:i + 1], P, radius, s, None)[0][0], s)
                    masked_away += cells != unmasked
                ran_out += k < P
                if k:                                                                                           # the first peak: the global minimum at its lowest index
                    ok = ~np.isnan(ent[i]) if mask is None else ~np.isnan(ent[i]) & ~(mask[i].reshape(Hd, s, Wd, s) != 0).any(axis=(1, 3))
                    assert cells[0] == divmod(int(np.flatnonzero(ok & (ent[i] == ent[i][ok].min()))[0]), Wd)
    assert ran_out > 0 and (Hd == 1 or (ties > 0 and masked_away > 0))


def test_a_10_x_18_grid_holds_at_most_15_peaks_at_radius_4():
    """Rows 0, 4, 8 and columns 0, 4, 8, 12, 16: 3 x 5 peaks pairwise at least 4 apart, and no sixteenth anywhere."""
    ent = np.zeros((1, 10, 18), np.float32)
    lattice = [(cy, cx) for cy in (0, 4, 8) for cx in (0, 4, 8, 12, 16)]
    for j, (cy, cx) in enumerate(lattice):
        ent[0, cy, cx] = -10.0 + j * 0.25                # the lattice first, in row-major order; every other cell falls to one of its windows
    pk, pe = D.peaks(ent, 16, 4, 4)
    assert D.cells(pk[0], 4) == lattice                  # the case is constructed: all fifteen fit ...
    assert tuple(pk[0, 15]) == (-1, -1) and pe[0, 15] == 0                                                     # ... and the sixteenth row is empty
    assert tuple(pk[0, 14]) == (8 * 4 + 2, 16 * 4 + 2)
    rs = np.random.RandomState(4)
    for _ in range(20):                                  # whatever the map: never a sixteenth
        pk, _ = D.peaks(_random_map(rs, 1, 10, 18, 50, 0.0), 16, 4, 4)
        assert tuple(pk[0, 15]) == (-1, -1) and len(D.cells(pk[0], 4)) <= 15


def test_guided_rects_clips_and_drops_the_empty_rows():
    pk = np.array([[2, 2], [0, 71], [-1, -1], [39, 0], [-1, -1]], np.int32)
    got = evaluate.guided_rects(pk, 1, 40, 72)
    assert got.dtype == np.int32 and got.tolist() == [[1, 1, 3, 3], [0, 70, 1, 71], [38, 0, 39, 1]]
    assert evaluate.guided_rects(pk, 0, 40, 72).tolist() == [[2, 2, 2, 2], [0, 71, 0, 71], [39, 0, 39, 0]]
    assert evaluate.guided_rects(np.full((3, 2), -1, np.int32), 2, 8, 8).shape == (0, 4)
    assert evaluate.guided_rects(np.zeros((0, 2), np.int32), 2, 8, 8).shape == (0, 4)


# ------------------------------------------------------------------------------------------------ ABI
def test_the_symbols_structs_and_constants_match_the_header():
    header = open(os.path.join(REPO, "include", "ideepcolor.h")).read()
    declared = set(re.findall(r"\b(idc_[a-z0-9_]+)\s*\(", header))
    lib = N.load()
    for sym, argc in (("idc_dist_peaks", 7), ("idc_suggest_colors_batch", 8), ("idc_forward_async_dist", 17)):
        assert sym in declared and sym in N.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
        assert len(getattr(lib, sym).argtypes) == argc
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % sym, header).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == argc
    assert re.search(r"enum \{ IDC_PEAKS_SKIP_HINTS = 1, IDC_TAPS_SUGGEST_AT_PEAKS = 2 \};", header)
    assert (N.IDC_PEAKS_SKIP_HINTS, N.IDC_TAPS_SUGGEST_AT_PEAKS) == (1, 2)
    assert re.search(r"#define IDC_PEAKS_MAX 256\b", header) and N.IDC_PEAKS_MAX == 256
    assert re.search(r"#define IDC_SUGGEST_MAX_QUERIES 4096\b", header) and N.IDC_SUGGEST_MAX_QUERIES == 4096
    # struct layouts as a C compiler lays them out on x86-64: {i32 img, y, x; u32 seed} and the taps block of the header
    assert re.search(r"typedef struct idc_dist_query \{ int32_t img, y, x; uint32_t seed; \} idc_dist_query;", header)
    assert ctypes.sizeof(N.DistQuery) == 16 and [f[0] for f in N.DistQuery._fields_] == ["img", "y", "x", "seed"]
    body = re.search(r"typedef struct idc_dist_taps \{(.*?)\} idc_dist_taps;", header, re.S).group(1)
    names = re.findall(r"\*?\s*([a-z_A-Z]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in N.DistTaps._fields_]
    assert ctypes.sizeof(N.DistTaps) == 96
    offs = {f[0]: getattr(N.DistTaps, f[0]).offset for f in N.DistTaps._fields_}
    assert (offs["flags"], offs["peaks"], offs["entropy"], offs["n_queries"], offs["queries"], offs["K"], offs["seed"], offs["centres"], offs["sugg_conf"]) == \
        (8, 16, 32, 40, 48, 56, 64, 72, 88)
    assert lib.idc_version() == 2                                  # additive: no bump


def test_a_call_without_a_handle_is_an_invalid_argument():
    lib = N.load()
    pk = np.zeros(2, np.int32)
    assert lib.idc_dist_peaks(None, 1, 1, 1, 0, pk.ctypes.data, None) == -1
    q = (N.DistQuery * 1)()
    c, oc = np.zeros((529, 2), np.float32), np.zeros(3, np.float64)
    assert lib.idc_suggest_colors_batch(None, 1, q, 1, 1, c.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), oc.ctypes.data, oc.ctypes.data) == -1
    px = np.zeros(3, np.uint8)
    one = (N.RefImage * 1)()
    one[0].rgb, one[0].h, one[0].w = px.ctypes.data, 1, 1
    t = N.DistTaps()
    assert lib.idc_forward_async_dist(None, 0, 1, one, None, None, 0, 1.0, 0.0, 50.0, 0, None, None, None, None, None, ctypes.byref(t)) == -1


# ------------------------------------------------------------------------------------------------ marshalling
class _Recorder(object):
    def __init__(self, bins=529):
        self.calls, self.bins = [], bins

    def idc_dist_bins(self, h):
        return self.bins

    def idc_forward_async_dist(self, *a):
        t = a[16]._obj
        q = [(t.queries[k].img, t.queries[k].y, t.queries[k].x, t.queries[k].seed) for k in range(t.n_queries)]
        self.calls.append((a, t, q))
        return 0

    def idc_dist_peaks(self, *a):
        self.calls.append(a)
        return 0

    def idc_suggest_colors_batch(self, *a):
        self.calls.append((a, [(a[2][k].img, a[2][k].y, a[2][k].x, a[2][k].seed) for k in range(a[1])]))
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


def test_forward_async_dist_marshals_the_taps():
    lib = _Recorder()
    e = _engine_over(lib)
    imgs = _images()
    centres = np.arange(1058, dtype=np.float32).reshape(529, 2)
    res = e.forward_async_dist(1, imgs, [[(0, 0, 1, 1, 3.0, 4.0)], None, None], peaks=5, radius=3, skip_hints=True, queries="peaks", K=4, N_draws=32,
                               seed=7, centres=centres, want_entropy=True)
    a, t, q = lib.calls[0]
    assert len(a) == 17 and (a[1], a[2], a[6], a[10]) == (1, 3, N.IDC_HINT_AB, 0)
    assert a[12] is None and a[14] is None and a[15] is None                   # no image, no score, no revealed colours unless asked for
    assert (t.n_peaks, t.radius, t.flags) == (5, 3, N.IDC_PEAKS_SKIP_HINTS | N.IDC_TAPS_SUGGEST_AT_PEAKS)
    assert t.n_queries == 0 and not t.queries and q == [] and (t.K, t.N, t.seed) == (4, 32, 7)
    assert res.peaks.shape == (3, 5, 2) and res.peaks.dtype == np.int32 and t.peaks == res.peaks.ctypes.data
    assert res.peak_ent.shape == (3, 5) and res.peak_ent.dtype == np.float32 and t.peak_ent == res.peak_ent.ctypes.data
    assert res.entropy.shape == (3, 2, 4) and t.entropy == res.entropy.ctypes.data                              # the 529 head's grid of an 8 x 16 handle
    assert res.sugg_centres.shape == (15, 4, 2) and res.sugg_conf.shape == (15, 4) and res.sugg_centres.dtype == np.float64
    assert (t.sugg_centres, t.sugg_conf) == (res.sugg_centres.ctypes.data, res.sugg_conf.ctypes.data)
    got = np.ctypeslib.as_array(ctypes.cast(t.centres, ctypes.POINTER(ctypes.c_float)), (529, 2))
    np.testing.assert_array_equal(got, centres)
    assert res.sse is None and res.hint_colours is None and res.out_rgb is None
    assert e._in_flight[1][0][0] is imgs[0] and e._in_flight[1][3] is res      # held until the slot's wait
    # explicit queries, seeds by default seed + row; the score, the images and the revealed colours; no peaks
    res = e.forward_async_dist(0, imgs, [[(0, 0, 1, 1)], None, [(1, 1, 2, 2)]], mode="reveal", want_sse=True, want_rgb=True, peaks=0,
                               queries=[(0, 1, 2), (2, -1, -1, 99), (1, 0, 0)], K=2, N_draws=5, seed=10, centres=centres)
    a, t, q = lib.calls[1]
    assert a[6] == N.IDC_HINT_REVEAL and a[14].value == res.sse.ctypes.data and a[15].value == res.hint_colours.ctypes.data
    assert res.sse.shape == (3, 3) and res.hint_colours.shape == (2, 2) and [o.shape for o in res.out_rgb] == [(8, 16, 3)] * 3
    assert (t.n_peaks, t.flags) == (0, 0) and not t.peaks and not t.peak_ent and not t.entropy and res.peaks is None and res.entropy is None
    assert q == [(0, 1, 2, 10), (2, -1, -1, 99), (1, 0, 0, 12)]
    assert res.sugg_centres.shape == (3, 2, 2) and res.sugg_conf.shape == (3, 2)
    # the 313 head's grid is the image's; no queries at all: nothing of the suggestion block is set
    e = _engine_over(_Recorder(313))
    res = e.forward_async_dist(0, imgs, None, peaks=2, want_entropy=True)
    a, t, q = e.lib.calls[0]
    assert res.entropy.shape == (3, 8, 16) and t.n_queries == 0 and not t.centres and not t.sugg_centres and res.sugg_centres is None
    with pytest.raises(ValueError):
        e.forward_async_dist(0, imgs, None, queries="everywhere")


def test_dist_peaks_and_suggest_colors_batch_marshal_their_arguments():
    lib = _Recorder()
    e = _engine_over(lib)
    pk, pe = e.dist_peaks(3, P=5, radius=2, skip_hints=True)
    a = lib.calls[0]
    assert a[1:5] == (3, 5, 2, N.IDC_PEAKS_SKIP_HINTS) and pk.shape == (3, 5, 2) and pk.dtype == np.int32 and pe.shape == (3, 5)
    assert a[5].value == pk.ctypes.data and a[6].value == pe.ctypes.data
    assert e.dist_peaks()[0].shape == (1, 8, 2) and lib.calls[1][1:5] == (1, 8, 2, 0)
    oc, of = e.suggest_colors_batch([(0, 1, 2, 3), (1, -1, -1, 2 ** 32 + 5)], np.zeros((529, 2), np.float32), K=3, N_draws=9)
    a, q = lib.calls[2]
    assert (a[1], a[3], a[4]) == (2, 3, 9) and q == [(0, 1, 2, 3), (1, -1, -1, 5)]
    assert oc.shape == (2, 3, 2) and of.shape == (2, 3) and a[6].value == oc.ctypes.data and a[7].value == of.ctypes.data


# ------------------------------------------------------------------------------------------------ the generators on stub engines
class _StubEngine(engine.HipColorizer):
    """forward_async_dist over recorded calls.  'The device' answers at the slot's wait: image v = image[0,0,0] gets sse (v, 2v, 3v), peaks
    (4v + k, k) for k < P with every row from ``empty_from`` on (-1, -1), suggestions 1000 v + 10 k + j."""

    def __init__(self, H, W, max_batch, empty_from=99):
        self.H, self.W, self.max_batch, self.empty_from = H, W, max_batch, empty_from
        self._pool = _Pool()
        self.calls = []
        self.busy = {}

    def close(self):
        pass

    def forward_async_dist(self, slot, images, hints, **kw):
        assert slot not in self.busy, "slot %d reused before its wait" % slot
        n, P, K = len(images), kw.get("peaks", 8), kw.get("K", 5)
        res = engine.DistBatch()
        res.sse = np.zeros((n, 3), np.uint64)
        res.out_rgb = [np.zeros(a.shape if kw.get("out") == "source" else (self.H, self.W, 3), np.uint8) for a in images] if kw.get("want_rgb") else None
        if P:
            res.peaks = np.zeros((n, P, 2), np.int32)
        if kw.get("queries") == "peaks":
            res.sugg_centres, res.sugg_conf = np.zeros((n * P, K, 2)), np.zeros((n * P, K))
        self.calls.append(("run", slot, [tuple(a.shape) for a in images], [None if h is None else [tuple(r) for r in h] for h in hints], dict(kw)))
        self.busy[slot] = (res, [int(a[0, 0, 0]) for a in images])
        return res

    def wait(self, slot):
        self.calls.append(("wait", slot))
        if slot in self.busy:
            res, vals = self.busy.pop(slot)
            res.sse[...] = np.array([[v, 2 * v, 3 * v] for v in vals], np.uint64)
            for i, v in enumerate(vals):
                if res.out_rgb is not None:
                    res.out_rgb[i][...] = v
                if res.peaks is not None:
                    for k in range(res.peaks.shape[1]):
                        res.peaks[i, k] = (-1, -1) if k >= self.empty_from else (4 * v + k, k)
                        if res.sugg_centres is not None:
                            res.sugg_centres[i * res.peaks.shape[1] + k] = 1000 * v + 10 * k + np.arange(res.sugg_centres.shape[1])[:, None]
                            res.sugg_conf[i * res.peaks.shape[1] + k] = v + k


def _items(count):
    rs = np.random.RandomState(3)
    return [np.full((int(rs.randint(1, 9)), int(rs.randint(1, 9)), 3), k, np.uint8) for k in range(count)]


@pytest.mark.parametrize("count,batch", [(1, 4), (4, 4), (5, 4), (11, 3), (6, None)])
def test_suggest_images_groups_alternates_slots_and_keeps_the_order(count, batch):
    e = _StubEngine(8, 16, 5)
    imgs = _items(count)
    hint = [(0, 0, 1, 1, 2.0, 3.0)]
    items = [a if k % 2 == 0 else (a, hint) for k, a in enumerate(imgs)]
    centres = np.zeros((529, 2), np.float32)
    got = list(e.suggest_images(iter(items), centres, batch=batch, peaks=3, radius=2, K=2, N_draws=32, seed=100))
    assert len(got) == count and not e.busy
    for g, (rgb, pk, sc, sf) in enumerate(got):
        assert rgb.shape == imgs[g].shape and (rgb == g).all(), "result %d is not image %d's" % (g, g)
        assert pk.tolist() == [[4 * g + k, k] for k in range(3)]
        assert sc.shape == (3, 2, 2) and sf.shape == (3, 2)
        assert sc[:, :, 0].tolist() == [[1000 * g + 10 * k, 1000 * g + 10 * k + 1] for k in range(3)] and (sf == g + np.arange(3)[:, None]).all()
    b = e.max_batch if batch is None else batch
    runs = [c for c in e.calls if c[0] == "run"]
    assert [len(c[2]) for c in runs] == [min(b, count - j) for j in range(0, count, b)]
    assert [c[1] for c in runs] == [j & 1 for j in range(len(runs))]
    assert [h for c in runs for h in c[3]] == [None if k % 2 == 0 else hint for k in range(count)]
    for j, c in enumerate(runs):                                    # peak k of the g-th image of the STREAM draws with seed + g * P + k
        kw = c[4]
        assert kw["queries"] == "peaks" and kw["seed"] == 100 + j * b * 3 and kw["peaks"] == 3 and kw["radius"] == 2 and kw["skip_hints"] is True
        assert kw["want_rgb"] is True and kw["out"] == "source" and kw["K"] == 2 and kw["N_draws"] == 32 and kw["centres"] is centres
    assert [c[1] for c in e.calls if c[0] == "wait"] == [j & 1 for j in range(len(runs))]
    for j in range(2, len(runs)):                                   # a wait between two uses of a slot
        assert ("wait", j & 1) in e.calls[e.calls.index(runs[j - 2]) + 1:e.calls.index(runs[j])]


def test_suggest_images_waits_for_both_slots_when_the_consumer_stops_early():
    e = _StubEngine(8, 16, 2)
    gen = e.suggest_images(iter(_items(9)), np.zeros((529, 2), np.float32), batch=2)
    next(gen)
    assert sorted(e.busy) == [1]
    gen.close()
    assert not e.busy
    with pytest.raises(ValueError):
        list(e.suggest_images(iter(_items(1)), np.zeros((529, 2), np.float32), batch=3))


@pytest.mark.parametrize("counts,empty_from", [((0, 1, 3), 99), ((0, 2, 3, 7), 3), ((2, 4), 99)])
def test_the_guided_sweep_grows_each_hint_list_by_exactly_the_peaks(counts, empty_from):
    e = _StubEngine(64, 64, 3, empty_from=empty_from)
    imgs = _items(7)
    table, rects = evaluate.psnr_sweep(e, imgs, counts=counts, strategy="uncertain", half=1, radius=5, batch=3, return_rects=True)
    assert table.shape == (len(counts), 7) and not e.busy
    passes = ([0] if counts[0] else []) + list(counts)               # points asked for during each pass over the images
    runs = [c for c in e.calls if c[0] == "run"]
    assert len(runs) == 3 * len(passes)
    want = [[] for _ in imgs]                                       # each image's list, grown as the issue states
    for p, have in enumerate(passes):
        more = passes[p + 1] - have if p + 1 < len(passes) else 0
        mine = runs[3 * p:3 * p + 3]
        assert [c[1] for c in mine] == [0, 1, 0] and [len(c[2]) for c in mine] == [3, 3, 1]
        assert [h for c in mine for h in c[3]] == want              # this pass saw exactly the rectangles of the passes before it
        for c in mine:
            kw = c[4]
            assert kw["mode"] == "reveal" and kw["peaks"] == more and kw["skip_hints"] is True and kw["radius"] == 5 and kw["want_sse"] is True
            assert kw.get("queries") is None
        for v in range(7):                                          # the first `more` peaks of THIS pass, (-1, -1) rows dropped, +- half, clipped
            for k in range(min(more, empty_from)):
                y, x = 4 * v + k, k
                want[v] = want[v] + [(max(y - 1, 0), max(x - 1, 0), min(y + 1, 63), min(x + 1, 63))]
    assert [[tuple(r) for r in rr.tolist()] for rr in rects] == want
    if empty_from < 99:
        assert all(len(w) < counts[-1] for w in want)               # an image that ran out keeps fewer points than the count
    for r in range(len(counts)):                                    # each row is the score of its own pass
        for v in range(7):
            assert table[r, v] == evaluate.psnr_from_sse(np.array([v, 2 * v, 3 * v], np.uint64), 64, 64)
    with pytest.raises(ValueError):
        evaluate.psnr_sweep(e, imgs, counts=(3, 1), strategy="uncertain")
    with pytest.raises(ValueError):
        evaluate.psnr_sweep(e, imgs, counts=(0, 1), strategy="greedy")


class _SweepEngine(object):
    H, W, max_batch = 64, 64, 4

    def __init__(self):
        self.seen = []

    def evaluate_images(self, items, **kw):
        items = list(items)
        self.seen.append((sorted(kw.items()), [np.asarray(r).tolist() for _, r in items]))
        for _, r in items:
            yield float(len(r)), np.zeros(3, np.uint64)

    def forward_async_dist(self, *a, **kw):
        raise AssertionError("the default strategy does not touch the distribution head")


def test_the_default_strategy_makes_the_calls_it_made_before():
    imgs = [np.zeros((5, 7, 3), np.uint8), np.zeros((9, 4, 3), np.uint8)]
    counts = (0, 1, 5)
    for kw in ({}, {"strategy": "random"}, {"strategy": "random", "half": 3, "radius": 9}):
        e = _SweepEngine()
        table = evaluate.psnr_sweep(e, imgs, counts=counts, seed=3, batch=2, **kw)
        np.testing.assert_array_equal(table, np.array(counts, np.float64)[:, None] * np.ones((1, 2)))
        points = [evaluate.simulate_points(64, 64, 5, np.random.RandomState(3 + j)) for j in range(2)]
        assert e.seen == [([("batch", 2), ("mode", "reveal"), ("out", "net")], [p[:c].tolist() for p in points]) for c in counts]
