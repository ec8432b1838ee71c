"""GPU checks of the distribution batches: idc_suggest_colors_batch, idc_dist_peaks and idc_forward_async_dist, through HipColorizer
(suggest_colors_batch / dist_peaks / forward_async_dist / suggest_images), evaluate.psnr_sweep(strategy='uncertain') and the wrapper classes.

Every comparison is bit for bit against a call the project already has, on the same handle:
  suggestions    idc_suggest_colors with the same arguments, one pixel per call;
  peaks          tests/dist_batch_ref.py (plain loops) applied to e.dist_entropy(n) of the SAME resident distribution and to the masks
                 idc_get_hint_planes returns;
  pipelined      the blocking route at the same n: set_image_rgb per image, set_hints / reveal_hints, forward_resident(n), then dist_entropy,
                 dist_peaks, suggest_colors, get_dist; the score against tests/eval_ref.py's integer sums of the blocking images.
Shapes: 64 x 64 handles (grids 16 x 16 and 64 x 64) and 40 x 72 handles (the 529 grid is 10 x 18: no multiple of a wave, and (16, 4) runs out of
cells there), bf16, max_batch 8, tests/ragged_ref.py's MIXED sizes with seeds 400 + j."""
import ctypes

import numpy as np
import pytest

import dist_batch_ref as D
import eval_ref as E
import ragged_ref as R
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import api, engine, evaluate, workloads
from oracle import weights
from test_batch_rgb_gpu import HINTS_AB, HINTS_RGB

pytestmark = pytest.mark.gpu

_ENG = {}
PR = [(1, 1), (8, 2), (16, 4)]


def _grid529():
    axis = np.arange(-110, 120, 10)
    return np.ascontiguousarray(np.array(np.meshgrid(axis, axis)).reshape((2, 529)).T.astype(np.float32))      # C order: the ABI reads [B][2]


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
                e.centres = _grid529()
            else:
                sd = _sd313()
                e = engine.HipColorizer(H, W, max_batch=8, precision="bf16", dist313=True)
                e.load_state_dict(sd)
                e.keep_dist(True)
                e.centres = np.ascontiguousarray(sd["pred.pred_ab.weight"][:, :, 0, 0].T)
            e.s = 4 if bins == 529 else 1
            _ENG[key] = e
        return _ENG[key]
    yield get
    for e in _ENG.values():
        e.close()
    _ENG.clear()


def _images(e, n=7):
    return [R.image(sh, sw, 400 + j) for j, (sh, sw) in enumerate(R.sizes(R.MIXED, e.H, e.W))][:n]


def _blocking(e, images, hints, mode, mask_value=1.0):
    """The blocking route: every image and its hints into the resident planes, one forward_resident(n).  Leaves the distribution of images
    0..n-1 resident.  -> (out_ab, rgb, revealed colours | None, net-size ground truth)."""
    truth, cols = [], []
    for i, img in enumerate(images):
        rgb_net, _ = e.set_image_rgb(img, img=i, keep_source=True, want_rgb=True, want_lab=False)
        truth.append(rgb_net[0].copy())
        h = (hints[i] if hints is not None else None) or []
        if mode == "reveal":
            cols.append(e.reveal_hints(h, img=i, mask_value=mask_value).copy())
        else:
            e.set_hints(h, mode=mode, img=i, mask_value=mask_value)
    ab, rgb, _ = e.forward_resident(len(images))
    return ab.copy(), rgb.copy(), (np.concatenate(cols) if mode == "reveal" else None), truth


def _masks(e, n):
    return np.stack([e.hint_planes(i)[1][0] for i in range(n)])


# ------------------------------------------------------------------------------------------------ 1. batched suggestions
@pytest.mark.parametrize("bins,H,W", [(529, 64, 64), (529, 40, 72), (313, 64, 64)])
def test_suggest_colors_batch_equals_suggest_colors_bit_for_bit(eng, bins, H, W):
    e = eng(bins, H, W)
    _blocking(e, _images(e, 3), [HINTS_AB[1], None, HINTS_AB[3]], "ab")
    # seven queries over three images: two at one pixel with different seeds, one empty, the last pixel of the image, a cell border of the 529 head
    queries = [(0, 5, 9, 11), (1, 20, 30, 12), (2, H - 1, W - 1, 13), (1, 20, 30, 99), (0, -1, -1, 5), (2, 3, 4, 0), (1, 4, 8, 2 ** 31 + 7)]
    for K in (1, 5, 16):
        for Nd in (1, 25000):
            oc, of = e.suggest_colors_batch(queries, e.centres, K=K, N_draws=Nd)
            assert oc.shape == (7, K, 2) and of.shape == (7, K) and oc.dtype == np.float64
            for q, (img, y, x, seed) in enumerate(queries):
                what = "K %d N %d query %d" % (K, Nd, q)
                if (y, x) == (-1, -1):
                    assert not oc[q].any() and not of[q].any(), what
                    continue
                c1, f1 = e.suggest_colors(y, x, e.centres, K=K, N_draws=Nd, seed=seed, img=img)
                assert oc[q].tobytes() == c1.tobytes() and of[q].tobytes() == f1.tobytes(), what
            if Nd > 1:
                assert oc[1].tobytes() != oc[3].tobytes() or of[1].tobytes() != of[3].tobytes()      # the seed matters
                assert abs(of.sum(axis=1)[[0, 1, 2, 3, 5, 6]] - 1.0).max() < 1e-12
            oc2, of2 = e.suggest_colors_batch(queries, e.centres, K=K, N_draws=Nd)
            assert oc2.tobytes() == oc.tobytes() and of2.tobytes() == of.tobytes()


# ------------------------------------------------------------------------------------------------ 2. uncertainty peaks
@pytest.mark.parametrize("bins,H,W", [(529, 64, 64), (529, 40, 72), (313, 64, 64), (313, 40, 72)])
def test_dist_peaks_equals_the_restated_rule(eng, bins, H, W):
    e = eng(bins, H, W)
    s = e.s
    _blocking(e, _images(e, 3), [None, HINTS_AB[1], None], "ab")
    ent = e.dist_entropy(3)
    assert np.isfinite(ent).all() and len(np.unique(ent[0])) > 4
    first = D.peaks(ent[:1], 1, 1, s)[0][0, 0]                       # the unmasked arg-min of image 0 ...
    ran_out = 0
    for hinted in (False, True):
        if hinted:                                                   # ... under a hint set AFTER the forward: the resident mask as it is at the call
            e.set_hints([(int(first[0]) - 1, int(first[1]) - 1, int(first[0]) + 1, int(first[1]) + 1, 10.0, 10.0)], mode="ab", img=0, mask_value=110.0)
            e.set_hints([(0, 0, H // 2, W - 1, 5.0, 5.0), (H - 3, 2, H - 1, 9, 1.0, 1.0)], mode="ab", img=2)
        mask = _masks(e, 3)
        assert (mask[0] != 0).any() == hinted and (mask[1] != 0).any()
        np.testing.assert_array_equal(e.dist_entropy(3), ent)       # the same resident distribution throughout
        for P, radius in PR:
            what = "%d bins %dx%d P %d radius %d hinted %s" % (bins, H, W, P, radius, hinted)
            pk, pe = e.dist_peaks(3, P=P, radius=radius)
            want, want_e = D.peaks(ent, P, radius, s)
            np.testing.assert_array_equal(pk, want, err_msg=what)
            assert pe.tobytes() == want_e.tobytes(), what
            pk_s, pe_s = e.dist_peaks(3, P=P, radius=radius, skip_hints=True)
            want_s, want_se = D.peaks(ent, P, radius, s, mask)
            np.testing.assert_array_equal(pk_s, want_s, err_msg=what)
            assert pe_s.tobytes() == want_se.tobytes(), what
            for i in range(3):                                       # peak_ent is the map at the peak, bit for bit
                for k, (cy, cx) in enumerate(D.cells(pk_s[i], s)):
                    assert pe_s[i, k].tobytes() == ent[i, cy, cx].tobytes() and mask[i, cy * s:(cy + 1) * s, cx * s:(cx + 1) * s].max() == 0
            assert tuple(pk[0, 0]) == tuple(first)
            if hinted:
                assert tuple(pk_s[0, 0]) != tuple(first), what      # skipping changes the answer
            one, one_e = e.dist_peaks(1, P=P, radius=radius, skip_hints=True)
            assert one[0].tobytes() == pk_s[0].tobytes() and one_e[0].tobytes() == pe_s[0].tobytes()      # n = 1 and n = 3: image 0's rows
            ran_out += int((pk == -1).any())
    if (bins, H, W) == (529, 40, 72):
        assert ran_out > 0                                           # 10 x 18 holds at most 15 peaks at radius 4


# ------------------------------------------------------------------------------------------------ 3. the pipelined form
def _raw_dist(e, slot, images, hints, mode, pinned, P=0, radius=1, flags=0, queries=None, K=5, Nd=32, seed=0, want_entropy=False, mask_value=1.0):
    """idc_forward_async_dist through the ABI with destinations of the test's own: pinned[k] decides, in turn, for the images, out_ab, sse,
    hint_colours, peaks, peak_ent, entropy, sugg_centres, sugg_conf.  -> dict of arrays, valid after wait."""
    n = len(images)
    pin = lambda k: pinned[k % len(pinned)]
    new = lambda shape, dtype, k: e.pinned_empty(shape, dtype) if pin(k) else np.empty(shape, dtype)
    vp = ctypes.c_void_p
    srcs = []
    for a in images:
        s = new(a.shape, np.uint8, 0)
        s[...] = a
        srcs.append(s)
    table = (N.RefImage * n)()
    outs = (vp * n)()
    res = dict(rgb=[new((e.H, e.W, 3), np.uint8, 0 if i % 2 else 1) for i in range(n)], ab=new((n, 2, e.H, e.W), np.float32, 1), sse=new((n, 3), np.uint64, 2))
    for i, a in enumerate(srcs):
        table[i].rgb, table[i].h, table[i].w = a.ctypes.data, a.shape[0], a.shape[1]
        outs[i] = res["rgb"][i].ctypes.data
    if mode == "reveal" and hints is not None:
        hints = [None if h is None else [tuple(r[:4]) + (0.0, 0.0) for r in h] for h in hints]
    offsets, arr = engine.flatten_hints(hints, n)
    res["cols"] = new((int(offsets[-1]), 2), np.float32, 3) if mode == "reveal" else None
    hd, wd = e._dist_grid()
    t = N.DistTaps()
    t.n_peaks, t.radius, t.flags = P, radius, flags
    if P:
        res["peaks"], res["peak_ent"] = new((n, P, 2), np.int32, 4), new((n, P), np.float32, 5)
        t.peaks, t.peak_ent = res["peaks"].ctypes.data, res["peak_ent"].ctypes.data
    if want_entropy:
        res["entropy"] = new((n, hd, wd), np.float32, 6)
        t.entropy = res["entropy"].ctypes.data
    qarr = engine.dist_queries(queries, seed)
    Q = n * P if flags & N.IDC_TAPS_SUGGEST_AT_PEAKS else (len(qarr) if qarr is not None else 0)
    if Q:
        t.n_queries = len(qarr) if qarr is not None else 0
        if qarr is not None:
            t.queries = qarr
        t.K, t.N, t.seed, t.centres = K, Nd, seed, e.centres.ctypes.data
        res["sc"], res["sf"] = new((Q, K, 2), np.float64, 7), new((Q, K), np.float64, 8)
        t.sugg_centres, t.sugg_conf = res["sc"].ctypes.data, res["sf"].ctypes.data
    for v in res.values():
        for a in (v if isinstance(v, list) else [v]):
            if a is not None:
                a.view(np.uint8)[...] = 0xA5
    e._chk(e.lib.idc_forward_async_dist(e._h, slot, n, table, offsets.ctypes.data_as(vp), ctypes.cast(arr, vp),
                                        {"ab": 0, "rgb": 1, "reveal": 2}[mode], mask_value, 0.0, 50.0, 0, None, outs, res["ab"].ctypes.data_as(vp),
                                        res["sse"].ctypes.data_as(vp), res["cols"].ctypes.data_as(vp) if res["cols"] is not None and res["cols"].size else None,
                                        ctypes.byref(t)))
    res["keep"] = (srcs, table, outs, arr, offsets, qarr, t)
    return res


def _want_taps(e, n, P, radius, skip, queries, K, Nd):
    """What the blocking calls read off the resident distribution."""
    ent = e.dist_entropy(n)
    pk, pe = e.dist_peaks(n, P=P, radius=radius, skip_hints=skip)
    sc = np.zeros((len(queries), K, 2)), np.zeros((len(queries), K))
    for q, (img, y, x, seed) in enumerate(queries):
        if (y, x) != (-1, -1):
            sc[0][q], sc[1][q] = e.suggest_colors(y, x, e.centres, K=K, N_draws=Nd, seed=seed, img=img)
    return ent, pk, pe, sc[0], sc[1]


def _peak_queries(pk, seed):
    n, P = pk.shape[:2]
    return [(i, int(pk[i, k, 0]), int(pk[i, k, 1]), seed + i * P + k) for i in range(n) for k in range(P)]


CASES = [(529, 64, 64, 7, "reveal", 1.0), (529, 40, 72, 7, "ab", 110.0), (313, 64, 64, 3, "rgb", 1.0), (313, 40, 72, 3, "reveal", 1.0)]


@pytest.mark.parametrize("bins,H,W,n,mode,mask_value", CASES)
def test_forward_async_dist_equals_the_blocking_route_bit_for_bit(eng, bins, H, W, n, mode, mask_value):
    e = eng(bins, H, W)
    images = _images(e, n)
    table = {"ab": HINTS_AB, "rgb": HINTS_RGB, "reveal": [None, E.R1, E.R2, [(1, 1, 16, 16), (2, 20, 17, 36)]]}[mode]
    hints = [table[(i + 1) % 4] for i in range(n)]
    hints[2] = [(0, 0, 1000, 1000) + {"ab": (20.0, -30.0), "rgb": (10, 200, 30), "reveal": ()}[mode]]      # image 2 is hinted all over
    P, radius, K, Nd, seed = (16, 4, 3, 32, 77) if (H, W) == (40, 72) else (8, 2, 5, 1000, 2 ** 32 - 3)
    explicit = [(0, 3, 5, 1), (n - 1, H - 1, W - 1, 2), (1, -1, -1, 3), (1, 9, 9, 4), (1, 9, 9, 5)]
    ab, rgb, cols, truth = _blocking(e, images, hints, mode, mask_value)
    dist = e.get_dist(n)
    ent, pk, pe, sc, sf = _want_taps(e, n, P, radius, True, explicit, K, Nd)
    _, pk_all, _, sc_p, sf_p = _want_taps(e, n, P, radius, False, _peak_queries(e.dist_peaks(n, P=P, radius=radius)[0], seed & 0xFFFFFFFF), K, Nd)
    assert (pk[2] == -1).all() and (pk_all[2, 0] >= 0).all() and not sc[2].any()          # skipping reads THIS batch's masks: image 2 has no cell left
    if (bins, H, W) == (529, 40, 72):
        assert (pk_all == -1).any() and not sc_p[n * P - 1].any()                      # run out: empty queries at the peaks give zeros
    sse = [E.sse(rgb[i], truth[i]) for i in range(n)]
    # a: the test's own destinations, pinned and pageable mixed, explicit queries, hinted cells skipped; b: HipColorizer's call, at the peaks
    a = _raw_dist(e, 0, images, hints, mode, [True, False, False, True, False, True, True, False, False], P=P, radius=radius,
                  flags=N.IDC_PEAKS_SKIP_HINTS, queries=explicit, K=K, Nd=Nd, want_entropy=True, mask_value=mask_value)
    b = e.forward_async_dist(1, images, hints, mode=mode, mask_value=mask_value, want_rgb=True, want_sse=True, out_ab=np.empty((n, 2, H, W), np.float32),
                             peaks=P, radius=radius, queries="peaks", K=K, N_draws=Nd, seed=seed, centres=e.centres, want_entropy=True)
    e.wait(0)
    e.wait(1)
    np.testing.assert_array_equal(e.get_dist(n), dist)                                 # the resident distribution is this batch's
    np.testing.assert_array_equal(a["ab"], ab)
    np.testing.assert_array_equal(b.out_ab, ab)
    for i in range(n):
        np.testing.assert_array_equal(a["rgb"][i], rgb[i], err_msg="image %d" % i)
        np.testing.assert_array_equal(b.out_rgb[i], rgb[i], err_msg="image %d" % i)
        assert a["sse"][i].tolist() == sse[i] and np.array(b.sse)[i].tolist() == sse[i]
    if mode == "reveal":
        assert a["cols"].tobytes() == cols.tobytes() and np.array(b.hint_colours).tobytes() == cols.tobytes()
    assert a["entropy"].tobytes() == ent.tobytes() and np.array(b.entropy).tobytes() == ent.tobytes()
    np.testing.assert_array_equal(a["peaks"], pk)
    np.testing.assert_array_equal(np.array(b.peaks), pk_all)
    assert a["peak_ent"].tobytes() == pe.tobytes()
    assert a["sc"].tobytes() == sc.tobytes() and a["sf"].tobytes() == sf.tobytes()
    assert np.array(b.sugg_centres).tobytes() == sc_p.tobytes() and np.array(b.sugg_conf).tobytes() == sf_p.tobytes()
    # the other way round: slot 1 with the other pinning, slot 0 at the peaks with the hinted cells skipped; no images, no score
    c = _raw_dist(e, 1, images, hints, mode, [False, True], P=P, radius=radius, flags=N.IDC_PEAKS_SKIP_HINTS | N.IDC_TAPS_SUGGEST_AT_PEAKS, K=K, Nd=Nd,
                  seed=5, mask_value=mask_value)
    e.wait(1)
    _, _, _, sc_s, sf_s = _want_taps(e, n, P, radius, True, _peak_queries(pk, 5), K, Nd)
    np.testing.assert_array_equal(c["peaks"], pk)
    assert c["sc"].tobytes() == sc_s.tobytes() and c["sf"].tobytes() == sf_s.tobytes()
    d = e.forward_async_dist(0, images, hints, mode=mode, mask_value=mask_value, peaks=0)
    e.wait(0)
    assert d.peaks is None and d.sse is None and d.out_rgb is None
    np.testing.assert_array_equal(e.get_dist(n), dist)


@pytest.mark.parametrize("bins,H,W", [(529, 40, 72), (313, 64, 64)])
def test_two_batches_in_flight_each_read_their_own_distribution(eng, bins, H, W):
    """Slot 0 and slot 1 carry different batches, submitted back to back before either wait: the taps of the first run before the network of
    the second replaces the handle's distribution."""
    e = eng(bins, H, W)
    imgs = _images(e, 7)
    batches = [(imgs[:3], [HINTS_AB[1], None, HINTS_AB[3]]), (imgs[3:7][::-1], [None, HINTS_AB[2], HINTS_AB[1], None])]
    want = []
    for images, hints in batches:
        ab, _, _, _ = _blocking(e, images, hints, "ab")
        n = len(images)
        pk = e.dist_peaks(n, P=8, radius=2, skip_hints=True)[0]
        want.append((ab, e.get_dist(n)) + _want_taps(e, n, 8, 2, True, _peak_queries(pk, 40), 4, 64))
    assert want[0][2][0].tobytes() != want[1][2][0].tobytes()
    got = [e.forward_async_dist(slot, images, hints, mode="ab", out_ab=np.empty((len(images), 2, H, W), np.float32), peaks=8, radius=2, skip_hints=True,
                                queries="peaks", K=4, N_draws=64, seed=40, centres=e.centres, want_entropy=True)
           for slot, (images, hints) in enumerate(batches)]
    e.wait(0)
    e.wait(1)
    for g, (ab, dist, ent, pk, pe, sc, sf) in zip(got, want):
        np.testing.assert_array_equal(g.out_ab, ab)
        assert np.array(g.entropy).tobytes() == ent.tobytes()
        np.testing.assert_array_equal(np.array(g.peaks), pk)
        assert np.array(g.peak_ent).tobytes() == pe.tobytes()
        assert np.array(g.sugg_centres).tobytes() == sc.tobytes() and np.array(g.sugg_conf).tobytes() == sf.tobytes()
    np.testing.assert_array_equal(e.get_dist(4), want[1][1])                          # the last batch enqueued stays resident


def test_suggest_images_yields_each_image_with_its_peaks_and_suggestions(eng):
    e = eng(529, 64, 64)
    imgs = _images(e, 7)
    hints = [HINTS_AB[i % 4] for i in range(7)]
    got = list(e.suggest_images(zip(imgs, hints), e.centres, batch=3, out="net", peaks=4, radius=3, K=3, N_draws=500, seed=9))
    assert len(got) == 7 and not e._in_flight
    for first in (0, 3, 6):
        group = list(range(first, min(first + 3, 7)))
        _, rgb, _, _ = _blocking(e, [imgs[g] for g in group], [hints[g] for g in group], "ab")
        pk = e.dist_peaks(len(group), P=4, radius=3, skip_hints=True)[0]
        for i, g in enumerate(group):
            np.testing.assert_array_equal(got[g][0], rgb[i])
            np.testing.assert_array_equal(got[g][1], pk[i])
            for k in range(4):
                c1, f1 = e.suggest_colors(int(pk[i, k, 0]), int(pk[i, k, 1]), e.centres, K=3, N_draws=500, seed=9 + g * 4 + k, img=i)
                assert got[g][2][k].tobytes() == c1.tobytes() and got[g][3][k].tobytes() == f1.tobytes()


# ------------------------------------------------------------------------------------------------ 4. the guided sweep
def test_the_guided_sweep_equals_a_step_by_step_blocking_loop(eng):
    e = eng(529, 64, 64)
    imgs = _images(e, 7)[2:6]
    counts = (0, 1, 3)
    table, rects = evaluate.psnr_sweep(e, imgs, counts=counts, strategy="uncertain", half=1, radius=2, batch=4, return_rects=True)
    mine = [np.zeros((0, 4), np.int32) for _ in imgs]
    want = np.zeros((3, 4))
    for r, c in enumerate(counts):
        _, rgb, _, truth = _blocking(e, imgs, [[tuple(int(v) for v in q) for q in m] for m in mine], "reveal")
        for j in range(4):
            want[r, j] = evaluate.psnr_from_sse(np.array(E.sse(rgb[j], truth[j]), np.uint64), 64, 64)
        if r + 1 < len(counts):
            more = counts[r + 1] - c
            pk = e.dist_peaks(4, P=more, radius=2, skip_hints=True)[0]
            mine = [np.concatenate([m, evaluate.guided_rects(pk[j], 1, 64, 64)]) for j, m in enumerate(mine)]
    np.testing.assert_array_equal(table, want)
    assert [r.tolist() for r in rects] == [m.tolist() for m in mine] and all(len(m) == 3 for m in mine)
    assert np.isfinite(table).all() and (table[0] != table[2]).all()
    t3, r3 = evaluate.psnr_sweep(e, imgs, counts=counts, strategy="uncertain", half=1, radius=2, batch=3, return_rects=True)      # both slots
    np.testing.assert_array_equal(t3, table)
    assert [r.tolist() for r in r3] == [m.tolist() for m in mine]


# ------------------------------------------------------------------------------------------------ 5. status
def test_every_status_of_the_table(eng, make_sd):
    INVALID, NO_WEIGHTS, BATCH, UNSUPPORTED = -1, -4, -6, -7
    e = eng(529, 40, 72)
    lib, h = e.lib, e._h
    images = _images(e, 3)
    _blocking(e, images, None, "ab")                                # 3 images resident
    vp, FP = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)
    pk, pe = np.zeros((8, 300, 2), np.int32), np.zeros((8, 300), np.float32)
    oc, of = np.zeros((5000, 16, 2)), np.zeros((5000, 16))
    cen = e.centres.ctypes.data_as(FP)
    peaks = lambda n=3, P=4, radius=2, flags=0, p=pk.ctypes.data, hh=h: lib.idc_dist_peaks(hh, n, P, radius, flags, p, pe.ctypes.data)
    assert peaks() == 0 and peaks(p=pk.ctypes.data) == 0 and lib.idc_dist_peaks(h, 3, 4, 2, 1, pk.ctypes.data, None) == 0
    for kw, code in ((dict(n=0), BATCH), (dict(n=4), BATCH), (dict(P=0), INVALID), (dict(P=257), INVALID), (dict(P=256), 0), (dict(radius=0), INVALID),
                     (dict(radius=19), INVALID), (dict(radius=18), 0), (dict(flags=2), INVALID), (dict(flags=4), INVALID), (dict(p=None), INVALID)):
        assert peaks(**kw) == code, kw

    def batch(q, nq=None, K=5, Nd=32, c=cen, o1=oc.ctypes.data, o2=of.ctypes.data, hh=h):
        arr = engine.dist_queries(q)
        return lib.idc_suggest_colors_batch(hh, len(q) if nq is None else nq, arr, K, Nd, c, o1, o2)
    good = [(0, 1, 1, 0), (2, 39, 71, 1), (1, -1, -1, 2)]
    assert batch(good) == 0
    for kw, code in ((dict(q=[(3, 1, 1, 0)]), BATCH), (dict(q=[(-1, 1, 1, 0)]), BATCH), (dict(q=[(0, 40, 1, 0)]), INVALID), (dict(q=[(0, 1, 72, 0)]), INVALID),
                     (dict(q=[(0, -1, 5, 0)]), INVALID), (dict(q=[(0, -2, -2, 0)]), INVALID), (dict(q=good, nq=0), INVALID), (dict(q=good, nq=-1), INVALID),
                     (dict(q=[(0, 1, 1, 0)] * 4097), INVALID), (dict(q=[(0, 1, 1, 0)] * 4096, K=1, Nd=1), 0), (dict(q=good, K=0), INVALID),
                     (dict(q=good, K=17), INVALID), (dict(q=good, Nd=0), INVALID), (dict(q=good, c=None), INVALID), (dict(q=good, o1=None), INVALID),
                     (dict(q=good, o2=None), INVALID)):
        assert batch(**kw) == code, {k: (v if k != "q" else v[:2]) for k, v in kw.items()}
    assert lib.idc_suggest_colors_batch(h, 2, None, 5, 32, cen, oc.ctypes.data, of.ctypes.data) == INVALID

    # the pipelined form
    srcs = [np.ascontiguousarray(a) for a in images]
    table = (N.RefImage * 3)()
    for i, a in enumerate(srcs):
        table[i].rgb, table[i].h, table[i].w = a.ctypes.data, a.shape[0], a.shape[1]
    sse, cols = np.zeros((3, 3), np.uint64), np.zeros((4, 2), np.float32)
    ent = np.zeros((3, 10, 18), np.float32)
    q3 = engine.dist_queries(good)

    def taps(P=4, radius=2, flags=0, p=pk.ctypes.data, nq=3, q=q3, K=5, Nd=32, c=e.centres.ctypes.data, o1=oc.ctypes.data, o2=of.ctypes.data,
             en=ent.ctypes.data):
        t = N.DistTaps()
        t.n_peaks, t.radius, t.flags, t.peaks, t.peak_ent, t.entropy = P, radius, flags, p, pe.ctypes.data, en
        t.n_queries, t.K, t.N, t.seed, t.centres, t.sugg_centres, t.sugg_conf = nq, K, Nd, 1, c, o1, o2
        if q is not None:
            t.queries = q
        return t

    def call(t=None, slot=0, n=3, mode=0, tab=table, s=sse.ctypes.data, hc=None, flags=0, hh=h, null_taps=False):
        t = taps() if t is None else t
        return lib.idc_forward_async_dist(hh, slot, n, tab, None, None, mode, 1.0, 0.0, 50.0, flags, None, None, None, s, hc, None if null_taps else ctypes.byref(t))

    def ok(**kw):
        assert call(**kw) == 0, kw
        e.wait(kw.get("slot", 0))
    ok()
    ok(slot=1, s=None)                                              # the score is optional
    ok(mode=2, hc=cols.ctypes.data)                                 # all three hint modes
    ok(mode=1)
    ok(t=taps(P=0, p=None))
    ok(t=taps(nq=0, q=None, c=None, o1=None, o2=None))
    ok(t=taps(flags=3, nq=0, q=None))
    ok(t=taps(P=256, radius=18, nq=0, q=None))
    for kw, code in ((dict(slot=2), INVALID), (dict(n=0), BATCH), (dict(n=9), BATCH), (dict(tab=None), INVALID), (dict(mode=3), INVALID),
                     (dict(flags=2), INVALID), (dict(mode=0, hc=cols.ctypes.data), INVALID), (dict(null_taps=True), INVALID)):
        assert call(**kw) == code, kw
    q_bad_img, q_bad_pos = engine.dist_queries([(3, 1, 1, 0)]), engine.dist_queries([(0, 40, 0, 0)])
    many = engine.dist_queries([(0, 1, 1, 0)] * 4097)
    for kw, code in ((dict(P=-1), INVALID), (dict(P=257), INVALID), (dict(radius=0), INVALID), (dict(radius=19), INVALID), (dict(flags=4), INVALID),
                     (dict(p=None), INVALID), (dict(P=0, flags=2, nq=0, q=None), INVALID), (dict(flags=2), INVALID), (dict(nq=-1), INVALID),
                     (dict(nq=4097, q=many), INVALID), (dict(nq=1, q=q_bad_img), BATCH), (dict(nq=1, q=q_bad_pos), INVALID), (dict(K=0), INVALID),
                     (dict(K=17), INVALID), (dict(Nd=0), INVALID), (dict(c=None), INVALID), (dict(o1=None), INVALID), (dict(o2=None), INVALID),
                     (dict(q=None), INVALID), (dict(P=200, flags=2, nq=0, q=None), 0)):
        got = call(t=taps(**kw))
        assert got == code, kw
        if got == 0:
            e.wait(0)
    assert call(t=taps(P=256, flags=2, nq=0, q=None, en=None), n=8, s=None, tab=(N.RefImage * 8)(*([table[0]] * 8))) == 0       # 2048 suggestions at the peaks
    e.wait(0)
    e.set_range_audit(True)
    assert call() == UNSUPPORTED
    e.set_range_audit(False)
    ok()
    # no distribution head; a 313 head whose distribution is not kept; nothing resident yet; no weights
    plain = engine.HipColorizer(64, 64, max_batch=8, precision="bf16")
    plain.load_state_dict(make_sd(0, "he"))
    L, ab, mask = workloads.random_batch(1, 64, seed=3)
    plain.forward(L, ab, mask, 0.0)
    assert call(hh=plain._h) == UNSUPPORTED and peaks(hh=plain._h) == UNSUPPORTED and batch(good, hh=plain._h) == UNSUPPORTED
    plain.close()
    e313 = eng(313, 64, 64)
    e313.keep_dist(False)
    c313 = e313.centres.ctypes.data
    assert call(t=taps(c=c313, en=None), hh=e313._h) == UNSUPPORTED and peaks(hh=e313._h) == UNSUPPORTED
    e313.keep_dist(True)
    assert call(t=taps(c=c313, en=None, nq=0, q=None), hh=e313._h) == 0
    e313.wait(0)
    fresh = engine.HipColorizer(64, 64, max_batch=2, precision="bf16", dist=True)
    assert peaks(hh=fresh._h, n=1) == UNSUPPORTED and batch(good[:1], hh=fresh._h) == UNSUPPORTED
    assert b"Need to set prediction first" in lib.idc_last_error(fresh._h)
    assert call(hh=fresh._h, n=1) == NO_WEIGHTS
    fresh.close()


# ------------------------------------------------------------------------------------------------ 6. the wrapper classes
@pytest.mark.parametrize("cls", ["torch529", "caffe313"])
def test_wrapper_multi_point_suggestions_and_uncertain_points(cls, make_sd):
    import os
    rgb = np.load(os.path.join(os.path.dirname(__file__), "golden", "mortar_pestle_256_rgb.npy"))[::4, ::4].copy()
    if cls == "torch529":
        m = api.ColorizeImageTorchDist(Xd=64, maskcent=True)
        m.prep_net(path="", state_dict=dict(make_sd(0, "he")))
    else:
        m = api.ColorizeImageCaffeDist(Xd=64)
        m.prep_net(0, state_dict=dict(_sd313()))
    assert m.get_uncertain_points() == 0 and m.get_ab_reccs_multi([(1, 1)]) == 0      # 'Need to set prediction first'
    m.set_image(rgb)
    input_ab, mask = workloads.hints_config2(64, 5, 3, 0)
    m.net_forward(input_ab, mask)
    points = [(20, 30), (5, 60), (-1, -1), (63, 63)]
    np.random.seed(11)
    cen, conf = m.get_ab_reccs_multi(points, K=4, N=5000, return_conf=True)
    assert cen.shape == (4, 4, 2) and conf.shape == (4, 4) and not cen[2].any()
    np.random.seed(11)
    np.testing.assert_array_equal(m.get_ab_reccs_multi(points, K=4, N=5000), cen)
    np.random.seed(11)
    base = int(np.random.randint(0, 2 ** 31 - 1))                  # the one draw get_ab_reccs makes; point q draws with that seed + q
    for q, (y, x) in enumerate(points):
        if y >= 0:
            c1, f1 = m.net.suggest_colors(y, x, m._bin_centres(), K=4, N_draws=5000, seed=base + q)       # what get_ab_reccs hands the engine
            assert cen[q].tobytes() == c1.tobytes() and conf[q].tobytes() == f1.tobytes(), q
    np.random.seed(11)
    np.testing.assert_array_equal(m.get_ab_reccs(20, 30, K=4, N=5000), cen[0])          # row 0: get_ab_reccs from the same RNG state
    pts = m.get_uncertain_points(P=6, radius=3)
    np.testing.assert_array_equal(pts, m.net.dist_peaks(1, P=6, radius=3)[0][0])
    assert pts.shape == (6, 2) and (pts >= 0).all() and (pts < 64).all()
    np.testing.assert_array_equal(m.get_uncertain_points(P=6, radius=3, skip_hints=True), m.net.dist_peaks(1, P=6, radius=3, skip_hints=True)[0][0])
