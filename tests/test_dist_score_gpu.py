"""GPU checks of the distribution scores: idc_dist_score and idc_forward_async_dist_score, through HipColorizer (dist_score /
forward_async_dist(score=) / score_images), evaluate.likelihood_sweep and the wrapper classes' score_dist.

What each output is compared with:
  truth_ab       reveal_hints of every cell's rectangle on the same handle, bit for bit;
  target, rank   tests/dist_score_ref.py (numpy float64) applied to get_dist of the SAME resident distribution and to the device's own truth_ab:
                 exact on the cells whose neighbour margins are at least 1e-4 (the CPU file shows that these are all but 0.2 % at most);
  xent_map       the same restatement, within 1e-12 relative (float64 exp and log to about an ulp each, exponent arguments below 40, at most 16
                 terms: a few 1e-14; the bar keeps about 50 x over that).  Largest value observed on an MI355X: 7.0e-16 (313 centres, 64 x 64,
                 nn 16; nn 1: at most 2.2e-16);
  xent[i], hits  the documented-order sum of the device's own xent_map, bit for bit; counts of the device's own rank_map, exactly;
  pipelined      the blocking call on the blocking route's distribution of the same images and hints, every output bit for bit.
Shapes: 64 x 64 handles (grids 16 x 16 and 64 x 64) and 40 x 72 handles (the 529 grid is 10 x 18: no multiple of a wave), bf16, max_batch 8,
tests/ragged_ref.py's MIXED sizes with seeds 400 + j; centres: the 529 grid and color_bins.pts_in_hull(); nn in {1, 5, 16}, sigma 5."""
import ctypes

import numpy as np
import pytest

import dist_score_ref as S
import eval_ref as E
import ragged_ref as R
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import api, color_bins, engine, evaluate, workloads
from oracle import weights
from test_batch_rgb_gpu import HINTS_AB, HINTS_RGB

pytestmark = pytest.mark.gpu

_ENG = {}
_REF = {}
GEOMS = [(529, 64, 64), (529, 40, 72), (313, 64, 64), (313, 40, 72)]
RANKS = (1, 5, 40)


def _sd313():
    return weights.add_pred313_head(weights.make_state_dict(2, "he", include_class=False), 2)


@pytest.fixture(scope="module")
def eng(make_sd):
    def get(bins, H, W):
        key = (bins, H, W)
        if key not in _ENG:
            if bins == 529:
                e = engine.HipColorizer(H, W, max_batch=8, precision="bf16", dist=True)
                e.load_state_dict(make_sd(0, "he"))
                e.centres = S.grid529()
            else:
                e = engine.HipColorizer(H, W, max_batch=8, precision="bf16", dist313=True)
                e.load_state_dict(_sd313())
                e.keep_dist(True)
                e.centres = np.ascontiguousarray(np.asarray(color_bins.pts_in_hull(), np.float32))
            e.s = 4 if bins == 529 else 1
            _ENG[key] = e
        return _ENG[key]
    yield get
    for e in _ENG.values():
        e.close()
    _ENG.clear()
    _REF.clear()


def _images(e, n=7):
    return [R.image(sh, sw, 400 + j) for j, (sh, sw) in enumerate(R.sizes(R.MIXED, e.H, e.W))][:n]


def _blocking(e, images, hints, mode, mask_value=1.0):
    """The blocking route: every image (its source kept) and its hints into the resident planes, one forward_resident(n).  Leaves the
    distribution of images 0..n-1 resident.  -> rgb of the forward"""
    for i, img in enumerate(images):
        e.set_image_rgb(img, img=i, keep_source=True, want_rgb=False, want_lab=False)
        h = (hints[i] if hints is not None else None) or []
        if mode == "reveal":
            e.reveal_hints(h, img=i, mask_value=mask_value)
        else:
            e.set_hints(h, mode=mode, img=i, mask_value=mask_value)
    return e.forward_resident(len(images))[1].copy()


def _same(a, b, what=""):
    for k in ("xent", "hits", "xent_map", "rank_map", "target", "truth_ab"):
        x, y = getattr(a, k) if not isinstance(a, dict) else a[k], getattr(b, k) if not isinstance(b, dict) else b[k]
        assert (x is None) == (y is None), (what, k)
        if x is not None:
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), (what, k)


HINTS7 = [HINTS_AB[1], None, HINTS_AB[3], HINTS_AB[2], None, HINTS_AB[1], HINTS_AB[0]]


# ------------------------------------------------------------------------------------------------ 1. the blocking form against the restatement
@pytest.mark.parametrize("nn", [1, 5, 16])
@pytest.mark.parametrize("bins,H,W", GEOMS)
def test_dist_score_equals_the_restatement(eng, bins, H, W, nn):
    e = eng(bins, H, W)
    s, hd, wd = e.s, H // e.s, W // e.s
    images = _images(e)
    _blocking(e, images, HINTS7, "ab")
    got = e.dist_score(e.centres, n=7, nn=nn, sigma=5.0, ranks=RANKS, want_maps=True)
    key = (bins, H, W)
    if key not in _REF:                                             # once per handle: the distribution and every cell's revealed colour
        cols = []
        for i in range(7):
            rects = [(cy * s, cx * s, cy * s + s - 1, cx * s + s - 1) for cy in range(hd) for cx in range(wd)]
            cols.append(e.reveal_hints(rects, img=i).reshape(hd, wd, 2).transpose(2, 0, 1).copy())
        _REF[key] = (e.get_dist(7), np.stack(cols))
        _blocking(e, images, HINTS7, "ab")                          # the hint planes as they were
    dist, cols = _REF[key]
    np.testing.assert_array_equal(e.get_dist(7), dist)              # the same resident distribution throughout; the score only read it
    assert got.truth_ab.dtype == np.float32 and got.truth_ab.tobytes() == cols.tobytes()       # reveal_hints' colour, bit for bit
    worst = 0.0
    for i in range(7):
        ref = S.score(dist[i], got.truth_ab[i], e.centres, nn, 5.0)
        worst = max(worst, S.compare(dict(target=got.target[i], rank=got.rank_map[i], xent=got.xent_map[i]), ref, "%s nn %d image %d" % (key, nn, i)))
        assert got.xent[i] == S.image_sum(got.xent_map[i]), i      # the documented order, bit for bit
        assert got.hits[i].tolist() == S.hits(got.rank_map[i], RANKS)
        assert np.isfinite(got.xent_map[i]).all() and (got.xent_map[i] >= 0).all() and got.rank_map[i].min() >= 0 and got.rank_map[i].max() < bins
    print("largest relative xent difference, %s nn %d: %.3g" % (key, nn, worst))
    assert len(np.unique(got.target)) > 4 and len(np.unique(got.rank_map)) > 4               # the images have colours: not one bin everywhere
    # an image's rows do not depend on n, nor on which maps are asked for; and the call is deterministic
    three = e.dist_score(e.centres, n=3, nn=nn, sigma=5.0, ranks=RANKS, want_maps=True)
    for k in ("xent", "hits", "xent_map", "rank_map", "target", "truth_ab"):
        assert getattr(three, k).tobytes() == getattr(got, k)[:3].tobytes(), k
    bare = e.dist_score(e.centres, n=7, nn=nn, sigma=5.0, ranks=RANKS)
    assert bare.xent.tobytes() == got.xent.tobytes() and bare.hits.tobytes() == got.hits.tobytes() and bare.xent_map is None
    none = e.dist_score(e.centres, n=7, nn=nn, sigma=5.0, ranks=())
    assert none.xent.tobytes() == got.xent.tobytes() and none.hits.shape == (7, 0)
    if nn > 1:                                                      # sigma matters once there is more than one neighbour
        assert e.dist_score(e.centres, n=7, nn=nn, sigma=2.0, ranks=RANKS).xent.tobytes() != got.xent.tobytes()


# ------------------------------------------------------------------------------------------------ 2. the pipelined form
def _raw_score(e, slot, images, hints, mode, pinned, nn, ranks, with_taps, want_maps=True, mask_value=1.0, sigma=5.0):
    """idc_forward_async_dist_score through the ABI with destinations of the test's own: pinned[k] decides, in turn, for the images, sse, xent,
    hits, xent_map, rank_map, target, truth_ab, entropy.  with_taps: an entropy map and 4 peaks besides; else taps == NULL.  -> dict, valid after wait."""
    n = len(images)
    pin = lambda k: pinned[k % len(pinned)]
    new = lambda shape, dtype, k: e.pinned_empty(shape, dtype) if pin(k) else np.empty(shape, dtype)
    vp = ctypes.c_void_p
    srcs = []
    for a in images:
        src = new(a.shape, np.uint8, 0)
        src[...] = a
        srcs.append(src)
    table = (N.RefImage * n)()
    for i, a in enumerate(srcs):
        table[i].rgb, table[i].h, table[i].w = a.ctypes.data, a.shape[0], a.shape[1]
    if mode == "reveal" and hints is not None:
        hints = [None if h is None else [tuple(r[:4]) + (0.0, 0.0) for r in h] for h in hints]
    offsets, arr = engine.flatten_hints(hints, n)
    hd, wd = e._dist_grid()
    res = dict(sse=new((n, 3), np.uint64, 1), xent=new((n,), np.float64, 2), hits=new((n, len(ranks)), np.uint32, 3) if ranks else None,
               xent_map=None, rank_map=None, target=None, truth_ab=None)
    if want_maps:
        res.update(xent_map=new((n, hd, wd), np.float64, 4), rank_map=new((n, hd, wd), np.int32, 5), target=new((n, hd, wd), np.int32, 6),
                   truth_ab=new((n, 2, hd, wd), np.float32, 7))
    t = None
    if with_taps:
        t = N.DistTaps()
        res["entropy"], res["peaks"] = new((n, hd, wd), np.float32, 8), np.empty((n, 4, 2), np.int32)
        t.n_peaks, t.radius, t.entropy, t.peaks = 4, 2, res["entropy"].ctypes.data, res["peaks"].ctypes.data
    for v in res.values():
        if v is not None:
            v.view(np.uint8)[...] = 0xA5
    spec = engine.score_spec(nn, sigma, ranks)
    out = N.DistScoreOut()
    for k in ("xent", "hits", "xent_map", "rank_map", "target", "truth_ab"):
        if res[k] is not None:
            setattr(out, k, res[k].ctypes.data)
    e._chk(e.lib.idc_forward_async_dist_score(e._h, slot, n, table, offsets.ctypes.data_as(vp), ctypes.cast(arr, vp),
                                              {"ab": 0, "rgb": 1, "reveal": 2}[mode], mask_value, 0.0, 50.0, 0, None, None, None, res["sse"].ctypes.data_as(vp),
                                              None, ctypes.byref(t) if t is not None else None, ctypes.byref(spec),
                                              e.centres.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(out)))
    res["keep"] = (srcs, table, arr, offsets, t, spec, out)
    return res


CASES = [(529, 64, 64, 7, "reveal", 1.0, 5), (529, 40, 72, 7, "ab", 110.0, 16), (313, 64, 64, 3, "rgb", 1.0, 1), (313, 40, 72, 3, "reveal", 1.0, 5)]


@pytest.mark.parametrize("bins,H,W,n,mode,mask_value,nn", CASES)
def test_the_pipelined_score_equals_the_blocking_score_bit_for_bit(eng, bins, H, W, n, mode, mask_value, nn):
    e = eng(bins, H, W)
    images = _images(e, n)
    table = {"ab": HINTS_AB, "rgb": HINTS_RGB, "reveal": [None, E.R1, E.R2, [(1, 1, 16, 16), (2, 20, 17, 36)]]}[mode]
    hints = [table[(i + 1) % 4] for i in range(n)]
    rgb = _blocking(e, images, hints, mode, mask_value)
    dist, ent = e.get_dist(n), e.dist_entropy(n)
    want = e.dist_score(e.centres, n=n, nn=nn, sigma=5.0, ranks=RANKS, want_maps=True)
    want1 = e.dist_score(e.centres, n=n, nn=1, sigma=5.0, ranks=(1,))
    truth = [e.set_image_rgb(img, img=7, keep_source=False, want_rgb=True, want_lab=False)[0][0].copy() for img in images]      # slot 7: not one of the scored ones
    # a: the test's own destinations, pinned and pageable mixed, the other taps besides; b: HipColorizer's call on the other slot, the score alone
    a = _raw_score(e, 0, images, hints, mode, [True, False, False, True, False, True, True, False, True], nn, RANKS, True, mask_value=mask_value)
    b = e.forward_async_dist(1, images, hints, mode=mode, mask_value=mask_value, peaks=0, score=dict(centres=e.centres, nn=nn, ranks=RANKS, want_maps=True))
    e.wait(0)
    e.wait(1)
    np.testing.assert_array_equal(e.get_dist(n), dist)              # the resident distribution is this batch's
    _same(a, want, "raw, slot 0")
    _same(b.score, want, "engine, slot 1")
    assert a["entropy"].tobytes() == ent.tobytes()                  # the other taps ran as they do without the score
    np.testing.assert_array_equal(a["peaks"], e.dist_peaks(n, P=4, radius=2)[0])
    assert [a["sse"][i].tolist() for i in range(n)] == [E.sse(rgb[i], truth[i]) for i in range(n)]
    assert b.peaks is None and b.sse is None
    # the other way round: slot 1 with the other pinning and taps == NULL, no maps, one neighbour; slot 0 through the engine with the other taps
    c = _raw_score(e, 1, images, hints, mode, [False, True], 1, (1,), False, want_maps=False, mask_value=mask_value)
    d = e.forward_async_dist(0, images, hints, mode=mode, mask_value=mask_value, peaks=4, radius=2, want_entropy=True,
                             score=dict(centres=e.centres, nn=nn, ranks=RANKS))
    e.wait(1)
    e.wait(0)
    _same(c, want1, "raw, slot 1, taps NULL")
    assert np.array(d.score.xent).tobytes() == want.xent.tobytes() and np.array(d.score.hits).tobytes() == want.hits.tobytes() and d.score.xent_map is None
    assert np.array(d.entropy).tobytes() == ent.tobytes()


@pytest.mark.parametrize("bins,H,W", [(529, 40, 72), (313, 64, 64)])
def test_two_batches_in_flight_are_each_scored_on_their_own_distribution(eng, bins, H, W):
    """Slot 0 and slot 1 carry different batches, submitted back to back before either wait: the score of the first runs before the network of
    the second replaces the handle's distribution, and each reads its own slot's source images."""
    e = eng(bins, H, W)
    imgs = _images(e, 7)
    batches = [(imgs[:3], [HINTS_AB[1], None, HINTS_AB[3]]), (imgs[3:7][::-1], [None, HINTS_AB[2], HINTS_AB[1], None])]
    want = []
    for images, hints in batches:
        _blocking(e, images, hints, "ab")
        want.append(e.dist_score(e.centres, n=len(images), nn=5, ranks=RANKS, want_maps=True))
    assert want[0].xent[0] != want[1].xent[0]
    got = [e.forward_async_dist(slot, images, hints, mode="ab", peaks=0, score=dict(centres=e.centres, nn=5, ranks=RANKS, want_maps=True))
           for slot, (images, hints) in enumerate(batches)]
    e.wait(0)
    e.wait(1)
    for slot in (0, 1):
        _same(got[slot].score, want[slot], "slot %d" % slot)


def test_score_images_yields_each_image_its_own_score(eng):
    e = eng(529, 64, 64)
    imgs = _images(e, 7)
    rects = [E.LISTS[i % 4] for i in range(7)]
    got = list(e.score_images(zip(imgs, rects), e.centres, batch=3, nn=5, ranks=RANKS, want_psnr=True))
    assert len(got) == 7 and not e._in_flight
    for first in (0, 3, 6):
        group = list(range(first, min(first + 3, 7)))
        rgb = _blocking(e, [imgs[g] for g in group], [rects[g] for g in group], "reveal")
        want = e.dist_score(e.centres, n=len(group), nn=5, ranks=RANKS)
        for i, g in enumerate(group):
            truth = e.set_image_rgb(imgs[g], img=7, keep_source=False, want_rgb=True, want_lab=False)[0][0]
            assert got[g][0] == want.xent[i] / 256.0 and got[g][1].tolist() == want.hits[i].tolist()
            assert got[g][2] == evaluate.psnr_from_sse(np.array(E.sse(rgb[i], truth), np.uint64), 64, 64)


# ------------------------------------------------------------------------------------------------ 3. the sweep
def test_the_likelihood_sweep_equals_a_step_by_step_blocking_loop(eng):
    e = eng(529, 64, 64)
    imgs = _images(e, 7)[2:6]
    counts = (0, 2, 10)
    xent, rates = evaluate.likelihood_sweep(e, imgs, e.centres, counts=counts, seed=5, nn=5, sigma=5.0, ranks=(1, 5), batch=3)
    points = [evaluate.simulate_points(64, 64, 10, np.random.RandomState(5 + j)) for j in range(4)]
    for r, c in enumerate(counts):
        _blocking(e, imgs, [[tuple(int(v) for v in q) for q in p[:c]] for p in points], "reveal")
        want = e.dist_score(e.centres, n=4, nn=5, sigma=5.0, ranks=(1, 5))
        np.testing.assert_array_equal(xent[r], want.xent / 256.0)
        np.testing.assert_array_equal(rates[r], want.hits / 256.0)
    assert np.isfinite(xent).all() and (xent[0] != xent[2]).all()    # the hints move the distribution


# ------------------------------------------------------------------------------------------------ 4. status
def test_every_status_of_the_table(eng, make_sd):
    INVALID, NO_WEIGHTS, BATCH, UNSUPPORTED = -1, -4, -6, -7
    e = eng(529, 40, 72)
    lib, h = e.lib, e._h
    images = _images(e, 3)
    _blocking(e, images, None, "ab")                                # 3 images resident, their sources kept
    FP = ctypes.POINTER(ctypes.c_float)
    cen = e.centres.ctypes.data_as(FP)
    xent, hits = np.zeros(8, np.float64), np.zeros((8, 8), np.uint32)
    maps = np.zeros((8, 2, 10, 18), np.float64)

    def spec(nn=1, sigma=5.0, ranks=(1, 5)):
        s = N.DistScoreSpec()
        s.nn, s.sigma, s.n_ranks = nn, sigma, len(ranks) if not isinstance(ranks, int) else ranks
        for j, r in enumerate(() if isinstance(ranks, int) else ranks[:8]):
            s.ranks[j] = r
        return s

    def outs(x=xent.ctypes.data, hh=hits.ctypes.data, m=None):
        o = N.DistScoreOut()
        o.xent, o.hits, o.xent_map, o.rank_map, o.target, o.truth_ab = x, hh, m, m, m, m
        return o

    def score(n=3, s=None, c=cen, o=None, hh=h, null_spec=False, null_out=False):
        s, o = spec() if s is None else s, outs() if o is None else o
        return lib.idc_dist_score(hh, n, None if null_spec else ctypes.byref(s), c, None if null_out else ctypes.byref(o))
    before = e.dist_score(e.centres, n=3, want_maps=True)
    dist = e.get_dist(3)
    assert score() == 0 and score(o=outs(m=maps.ctypes.data)) == 0 and score(s=spec(ranks=()), o=outs(hh=None)) == 0
    assert score(s=spec(nn=16, ranks=(1, 529, 2, 3, 4, 5, 6, 7))) == 0
    for kw, code in ((dict(null_spec=True), INVALID), (dict(null_out=True), INVALID), (dict(o=outs(x=None)), INVALID), (dict(c=None), INVALID),
                     (dict(s=spec(nn=0)), INVALID), (dict(s=spec(nn=17)), INVALID), (dict(s=spec(sigma=0.0)), INVALID), (dict(s=spec(sigma=-1.0)), INVALID),
                     (dict(s=spec(sigma=float("inf"))), INVALID), (dict(s=spec(sigma=float("nan"))), INVALID), (dict(s=spec(ranks=-1)), INVALID),
                     (dict(s=spec(ranks=9)), INVALID), (dict(s=spec(ranks=(0,))), INVALID), (dict(s=spec(ranks=(1, 530))), INVALID),
                     (dict(o=outs(hh=None)), INVALID), (dict(n=0), BATCH), (dict(n=4), BATCH), (dict(hh=None), INVALID)):
        assert score(**kw) == code, kw
    e.set_image_rgb(images[1], img=1, keep_source=False)           # slot 1 loses its source: images 0..1 cannot be scored, image 0 can
    assert score(n=2) == UNSUPPORTED and b"no resident source" in lib.idc_last_error(h) and score(n=1) == 0
    e.set_image_rgb(images[1], img=1, keep_source=True)
    e.set_range_audit(True)
    assert score() == UNSUPPORTED
    e.set_range_audit(False)
    assert score() == 0

    # the pipelined form
    srcs = [np.ascontiguousarray(a) for a in images]
    table = (N.RefImage * 3)()
    for i, a in enumerate(srcs):
        table[i].rgb, table[i].h, table[i].w = a.ctypes.data, a.shape[0], a.shape[1]
    pk = np.zeros((8, 4, 2), np.int32)

    def call(slot=0, n=3, mode=0, tab=table, flags=0, hh=h, taps=False, s=None, c=cen, o=None, null_spec=False, null_out=False):
        s, o = spec() if s is None else s, outs() if o is None else o
        t = N.DistTaps()
        t.n_peaks, t.radius, t.peaks = 4, 2, pk.ctypes.data
        return lib.idc_forward_async_dist_score(hh, slot, n, tab, None, None, mode, 1.0, 0.0, 50.0, flags, None, None, None, None, None,
                                                ctypes.byref(t) if taps else None, None if null_spec else ctypes.byref(s), c,
                                                None if null_out else ctypes.byref(o))

    def ok(**kw):
        assert call(**kw) == 0, kw
        e.wait(kw.get("slot", 0))
    ok()
    ok(slot=1, taps=True)
    ok(mode=2)
    ok(mode=1, o=outs(m=maps.ctypes.data))
    ok(s=spec(ranks=()), o=outs(hh=None))
    for kw, code in ((dict(slot=2), INVALID), (dict(n=0), BATCH), (dict(n=9), BATCH), (dict(tab=None), INVALID), (dict(mode=3), INVALID), (dict(flags=2), INVALID),
                     (dict(null_spec=True), INVALID), (dict(null_out=True), INVALID), (dict(o=outs(x=None)), INVALID), (dict(c=None), INVALID),
                     (dict(s=spec(nn=0)), INVALID), (dict(s=spec(nn=17)), INVALID), (dict(s=spec(sigma=0.0)), INVALID), (dict(s=spec(sigma=float("nan"))), INVALID),
                     (dict(s=spec(ranks=9)), INVALID), (dict(s=spec(ranks=(530,))), INVALID), (dict(o=outs(hh=None)), INVALID)):
        assert call(**kw) == code, kw
    t_bad = N.DistTaps()
    t_bad.n_peaks = 4                                               # peaks without a destination: the taps' own table still holds
    assert lib.idc_forward_async_dist_score(h, 0, 3, table, None, None, 0, 1.0, 0.0, 50.0, 0, None, None, None, None, None, ctypes.byref(t_bad),
                                            ctypes.byref(spec()), cen, ctypes.byref(outs())) == INVALID
    assert call(slot=1) == 0 and call(slot=1) == INVALID            # still in flight
    e.wait(1)
    e.set_range_audit(True)
    assert call() == UNSUPPORTED
    e.set_range_audit(False)
    # a refused call leaves slot and handle as they were: the slots are free, the distribution and the blocking score are what they were
    ok()
    ok(slot=1)
    _blocking(e, images, None, "ab")
    np.testing.assert_array_equal(e.get_dist(3), dist)
    _same(e.dist_score(e.centres, n=3, want_maps=True), before)
    # no distribution head; a 313 head whose distribution is not kept; nothing resident yet; no weights
    plain = engine.HipColorizer(64, 64, max_batch=8, precision="bf16")
    plain.load_state_dict(make_sd(0, "he"))
    L, ab, mask = workloads.random_batch(1, 64, seed=3)
    plain.forward(L, ab, mask, 0.0)
    assert score(hh=plain._h, n=1) == UNSUPPORTED and call(hh=plain._h) == UNSUPPORTED
    plain.close()
    e313 = eng(313, 64, 64)
    c313 = e313.centres.ctypes.data_as(FP)
    _blocking(e313, _images(e313, 3), None, "ab")
    e313.keep_dist(False)
    assert score(hh=e313._h, c=c313) == UNSUPPORTED and call(hh=e313._h, c=c313) == UNSUPPORTED
    e313.keep_dist(True)
    assert score(hh=e313._h, c=c313, s=spec(ranks=(1, 313))) == 0 and score(hh=e313._h, c=c313, s=spec(ranks=(314,))) == INVALID
    assert call(hh=e313._h, c=c313) == 0
    e313.wait(0)
    fresh = engine.HipColorizer(64, 64, max_batch=2, precision="bf16", dist=True)
    assert score(hh=fresh._h, n=1) == UNSUPPORTED and b"Need to set prediction first" in lib.idc_last_error(fresh._h)
    assert call(hh=fresh._h, n=1) == NO_WEIGHTS
    fresh.close()


# ------------------------------------------------------------------------------------------------ 5. the wrapper classes
@pytest.mark.parametrize("cls", ["torch529", "caffe313"])
def test_wrapper_score_dist(cls, make_sd):
    import os
    rgb = np.load(os.path.join(os.path.dirname(__file__), "golden", "mortar_pestle_256_rgb.npy"))[::4, ::4].copy()
    if cls == "torch529":
        m = api.ColorizeImageTorchDist(Xd=64, maskcent=True)
        m.prep_net(path="", state_dict=dict(make_sd(0, "he")))
    else:
        m = api.ColorizeImageCaffeDist(Xd=64)
        m.prep_net(0, state_dict=dict(_sd313()))
    assert m.score_dist() == 0                                      # 'Need to set prediction first'
    m.set_image_device(rgb)
    m.net_forward_hints([(10, 12, 14, 16, 200, 30, 40)])
    mean, rates = m.score_dist(nn=5, sigma=5.0, ranks=(1, 5, 40))
    want = m.net.dist_score(m._bin_centres(), 1, nn=5, sigma=5.0, ranks=(1, 5, 40), want_maps=True)
    assert mean == want.mean()[0] and rates.tolist() == want.rates()[0].tolist() and np.isfinite(mean) and mean > 0
    assert (np.diff(rates) >= 0).all() and rates[-1] <= 1.0
    mean2, rates2, maps = m.score_dist(nn=5, sigma=5.0, ranks=(1, 5, 40), return_maps=True)
    assert mean2 == mean and rates2.tolist() == rates.tolist()
    assert maps["xent"].shape == (64, 64) and maps["rank"].shape == (64, 64) and maps["target"].dtype == np.int32 and maps["truth_ab"].shape == (2, 64, 64)
    r = m._dist_rep
    np.testing.assert_array_equal(maps["xent"][::r, ::r], want.xent_map[0])
    np.testing.assert_array_equal(maps["xent"][r - 1::r, r - 1::r], want.xent_map[0])
    np.testing.assert_array_equal(maps["truth_ab"][:, ::r, ::r], want.truth_ab[0])
    input_ab, mask = workloads.hints_config2(64, 5, 3, 0)
    m.net_forward(input_ab, mask)                                   # a forward that is handed the L plane: the engine lets the source go ...
    mean3, rates3 = m.score_dist(nn=5, sigma=5.0, ranks=(1, 5, 40))                           # ... and the wrapper, which has the image, brings it back
    want3 = m.net.dist_score(m._bin_centres(), 1, nn=5, sigma=5.0, ranks=(1, 5, 40), want_maps=True)
    assert mean3 == want3.mean()[0] and rates3.tolist() == want3.rates()[0].tolist() and mean3 != mean
    assert want3.truth_ab.tobytes() == want.truth_ab.tobytes()     # the same image
    m.set_image(rgb)                                               # the host route: no source on the device
    m.net_forward(input_ab, mask)
    with pytest.raises(RuntimeError):
        m.score_dist()
