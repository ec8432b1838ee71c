"""GPU checks of antialiased ingestion (idc_set_ingest_filter): the pre-pass kernel through every route that brings a source to the net size.
The references are tests/resample_ref.py (the rule in plain numpy float64), the oracle's rgb2lab, the device's own net-size image ingested
again as a net-size source (the identity), the filter-off handle for sources that are not down-scaled, and the blocking route per image
for the pipelined calls -- never the call under test.

Bars (tests/resample_ref.py holds them; tests/test_resample_cpu.py shows that they catch six mutants of the rule):
  rgb_net / gray_net   exact, every sample: the inputs keep every value before rounding further than 1e-6 from a tie
  lab_net / l_net      1e-9 absolute, the project's bar for float64 colour arithmetic
  L plane              out_ab of forward_resident bit-identical to the one after set_image_l(float32(L - 50)) of the call's own L
  identity, off, pipelined, switching back    bit for bit
  references           counts exact; saturation to one fp32 ulp of the existing route (tests/test_glob_ref_gpu.py's bar)
Shapes: a 64 x 64 net, bf16, seeded weights, max_batch 4; the sources of resample_ref.CASES.  Section 3b runs resample_ref.NET_CASES on nets of
their own -- (16, 8), (24, 16) and (8, 24) for the one-column tiles that walk their span in 2, 3 and 4 chunks (three channels only, W <= 24;
the one-channel 3 x 16384 planes fill one chunk exactly and are not chunked), (64, 64) for three-channel sources with several column tiles,
(40, 72) and (72, 40) because a swap of H and W is invisible on a square net, (16, 24) for one chunked job among small ones in ONE pipelined
call -- as blocking ingestions without a forward, and two pipelined calls held to the blocking route and to the rule.

Wall time of this file on an MI355X, as measured there: 4.0 s for its 49 tests (pytest's own figure); the slowest test takes 0.6 s, every case of
section 3b is below 0.25 s."""
import ctypes

import numpy as np
import pytest

import glob_ref
import gray_ref as G
import ingest_ref
import resample_ref as R
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import engine
from oracle import weights

pytestmark = pytest.mark.gpu

HINTS = G.HINTS[:3]
RECTS = [(2, 3, 20, 30), (16, 25, 50, 60), (40, 2, 62, 20), (0, 50, 10, 63), (70, 70, 80, 80)]      # the last lies outside the image


@pytest.fixture(scope="module")
def engines(make_sd):
    made = {}

    def get(name="a", **kw):
        if name not in made:
            e = engine.HipColorizer(R.H, R.W, max_batch=4, precision="bf16", **kw)
            if kw.get("global_hints"):              # (the weights of test_glob_ref_gpu._glob_sd)
                e.load_state_dict(weights.add_global_branch(weights.make_state_dict(3, "he", include_class=False), 3))
            else:
                e.load_state_dict(make_sd(0, "he"))
            made[name] = e
        return made[name]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture
def e(engines):
    eng = engines("a", dist=True)
    eng.set_ingest_filter("bilinear")
    eng.set_batch_upsample("linear")
    yield eng
    eng.set_ingest_filter("bilinear")
    eng.set_batch_upsample("linear")


def _centres(e):
    rs = np.random.RandomState(5)
    return np.ascontiguousarray(rs.uniform(-100, 100, (e.dist_bins(), 2)).astype(np.float32))


def _is_gray(src):
    return src.ndim == 2


def _ingest(e, src, gray=None, **kw):
    return e.set_image_gray(src, **kw) if (_is_gray(src) if gray is None else gray) else e.set_image_rgb(src, **kw)


def _forward(e, hints=HINTS):
    e.set_hints(hints or [], mode="ab")
    out = e.forward_resident(1)
    assert np.isfinite(out[0]).all() and np.abs(out[0]).max() > 0
    return [np.array(x) for x in out]


# ------------------------------------------------------------------------------------------------ 1. blocking calls against the rule
@pytest.mark.parametrize("name", sorted(R.DOWN))
def test_blocking_ingestion_is_the_rule(e, name):
    src, _, want = R.case(name)
    e.set_ingest_filter("antialias")
    net, lab = _ingest(e, src, keep_source=True)
    net, lab = np.array(net), np.array(lab)
    assert net.dtype == src.dtype and net.shape == (1,) + want.shape
    bad = int((net[0] != want).sum())
    print("%s: %d of %d samples differ from the rule" % (name, bad, want.size))
    np.testing.assert_array_equal(net[0], want)
    if _is_gray(src):
        l_want = G.lightness(want)
        err = float(np.abs(lab[0] - l_want).max())
        L = lab[0]
    else:
        err = float(np.abs(lab[0] - ingest_ref.net_lab(want)).max())
        L = lab[0, 0]
    print("%s: Lab off by %.3e" % (name, err))
    assert err <= R.L_TOL
    # the resident L plane is the float32 of it
    got = _forward(e)
    e.set_image_l((L - 50.0).astype(np.float32))
    for a, b in zip(got, _forward(e)):
        np.testing.assert_array_equal(a, b)
    # two images in one call, into slots 1 and 2, not kept: each is the image alone (the second turned upside down)
    if src.nbytes <= 300000:
        pair = np.stack([src, src[::-1]])
        net2, lab2 = _ingest(e, pair, gray=_is_gray(src), img=1)
        np.testing.assert_array_equal(net2[0], want)
        np.testing.assert_array_equal(net2[1], R.resample(np.ascontiguousarray(src[::-1]))[1])
        np.testing.assert_array_equal(np.array(lab2[0]), lab[0])


# ------------------------------------------------------------------------------------------------ 2. the identity
@pytest.mark.parametrize("name", ["rgb_211x83", "rgb_100x40", "rgb_700x1000", "gray16_211x83", "gray8_65x16384"])
def test_the_devices_own_net_image_ingested_again_gives_the_same_bits(e, engines, name):
    src = R.case(name)[0]
    b = engines("b", dist=True)
    b.set_ingest_filter("antialias")
    e.set_ingest_filter("antialias")
    c = _centres(e)
    outs = []
    for eng, image in ((e, src), (b, None)):
        if image is None:
            image = np.ascontiguousarray(outs[0][0][0])        # the first handle's own rgb_net / gray_net, a net-size source
            assert image.shape[:2] == (R.H, R.W)
        net, lab = _ingest(eng, image, keep_source=True)
        res = [np.array(net), np.array(lab)]
        if _is_gray(src):
            res += _forward(eng)
        else:
            cols = np.array(eng.reveal_hints(RECTS))
            assert np.abs(cols[:4]).max() > 0 and not cols[4].any()
            fwd = eng.forward_resident(1)
            score = eng.dist_score(c, n=1, want_maps=True)
            res += [cols] + [np.array(x) for x in fwd] + [np.array(score.target), np.array(score.truth_ab), np.array(score.xent)]
        outs.append(res)
    assert len(outs[0]) == len(outs[1]) >= 5
    for k, (x, y) in enumerate(zip(*outs)):
        np.testing.assert_array_equal(x, y, err_msg="%s: result %d" % (name, k))
    b.set_ingest_filter("bilinear")


@pytest.mark.parametrize("name", sorted(R.SAME) + ["gray16_23x31"])
def test_sources_that_are_not_downscaled_are_the_filter_off_bits(e, engines, name):
    src = G.gray16(23, 31) if name == "gray16_23x31" else R.case(name)[0]
    off = engines("b", dist=True)
    off.set_ingest_filter("bilinear")
    e.set_ingest_filter("antialias")
    res = []
    for eng in (e, off):
        net, lab = _ingest(eng, src, keep_source=True)
        r = [np.array(net), np.array(lab)]
        if not _is_gray(src):
            r.append(np.array(eng.reveal_hints(RECTS)))
        r += _forward(eng, None if not _is_gray(src) else HINTS)
        r.append(np.array(eng.fullres_rgb("output_ab", "joint")))
        res.append(r)
    for x, y in zip(*res):
        np.testing.assert_array_equal(x, y)
    if name in R.SAME:
        np.testing.assert_array_equal(res[0][0][0], R.case(name)[2])


# ------------------------------------------------------------------------------------------------ 3. pipelined calls against the blocking route
_BLOCK = {}


def _blocking(e, filt, src, hints, interp, out):
    """(image, out_ab) of one source by the blocking route under ``filt``; the handle's filter is left as it was."""
    k = (e.H, e.W, filt, src.shape, src.dtype.str, src.tobytes(), repr(hints), interp, out)
    if k not in _BLOCK:
        prev = e._ingest_filter
        e.set_ingest_filter(filt)
        _ingest(e, src, keep_source=True)
        e.set_hints(hints or [], mode="ab")
        raw, rgb, _ = e.forward_resident(1)
        img = np.array(rgb[0]) if out == "net" else np.array(e.fullres_rgb("output_ab", interp, "image"))
        img.setflags(write=False)
        _BLOCK[k] = (img, np.array(raw[0]))
        e.set_ingest_filter(prev)
    return _BLOCK[k]


def _small(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _ragged():
    """Down-scaled and not, mixed; the image starts (in pixels) cover every residue mod 4."""
    imgs = [_small(1, 1, 1), R.case("rgb_211x83")[0], _small(5, 5, 2), R.case("rgb_100x40")[0]]
    assert sorted(s % 4 for s in G.starts([i.shape[:2] for i in imgs])) == [0, 1, 2, 3]
    return [np.ascontiguousarray(i) for i in imgs]


def _hint_lists(n):
    return [HINTS[:i % 3 + 1] if i != 2 else None for i in range(n)]


@pytest.mark.parametrize("upsample", ["linear", "joint"])
def test_ragged_batches_equal_the_blocking_route_with_one_batch_of_each_setting_in_flight(e, upsample):
    e.set_batch_upsample(upsample)
    for out in ("net", "source"):
        for order in (1, -1):
            imgs = _ragged()[::order]
            hints = _hint_lists(len(imgs))
            ab = [np.empty((len(imgs), 2, R.H, R.W), np.float32) for _ in range(2)]
            filt = ("antialias", "bilinear")[::order]               # either slot takes either setting
            e.set_ingest_filter(filt[0])
            o0 = e.forward_async_images(0, imgs, hints, out_ab=ab[0], out=out)
            e.set_ingest_filter(filt[1])                            # while slot 0 is in flight: it keeps what it was enqueued with
            o1 = e.forward_async_images(1, imgs, hints, out_ab=ab[1], out=out)
            e.wait(0); e.wait(1)
            assert np.isfinite(e.pipeline_times(0)).all() and np.isfinite(e.pipeline_times(1)).all()
            for slot, outs in ((0, o0), (1, o1)):
                for i, src in enumerate(imgs):
                    want, raw = _blocking(e, filt[slot], src, hints[i], upsample, out)
                    assert outs[i].shape == want.shape
                    np.testing.assert_array_equal(outs[i], want, err_msg="image %d, %s, slot %d, %s" % (i, out, slot, filt[slot]))
                    np.testing.assert_array_equal(ab[slot][i], raw)
            d = R.case("rgb_211x83")[0]
            assert (_blocking(e, "antialias", d, hints[1], upsample, out)[1] != _blocking(e, "bilinear", d, hints[1], upsample, out)[1]).any()


@pytest.mark.parametrize("name", ["rgb_128x128", "rgb_100x40", "rgb_30x50"])
def test_same_size_batches_equal_the_blocking_route(e, name):
    src = R.case(name)[0]
    batch = np.ascontiguousarray(np.stack([src, src[::-1], src[:, ::-1]]))
    hints = _hint_lists(3)
    for upsample in ("linear", "joint"):
        e.set_batch_upsample(upsample)
        for slot, out in ((0, "net"), (1, "source")):
            e.set_ingest_filter("antialias")
            got = np.zeros(batch.shape if out == "source" else (3, R.H, R.W, 3), np.uint8)
            ab = np.empty((3, 2, R.H, R.W), np.float32)
            e.forward_async_rgb(slot, batch, hints, got, out_ab=ab, out=out)
            e.set_ingest_filter("bilinear")
            e.wait(slot)
            for i in range(3):
                want, raw = _blocking(e, "antialias", np.ascontiguousarray(batch[i]), hints[i], upsample, out)
                np.testing.assert_array_equal(got[i], want, err_msg="image %d, %s, %s" % (i, out, upsample))
                np.testing.assert_array_equal(ab[i], raw)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_grey_batches_equal_the_blocking_route(e, dtype):
    big = R.case("gray16_211x83")[0]
    big = big if dtype == np.uint16 else (big >> 8).astype(np.uint8)
    make = G.gray16 if dtype == np.uint16 else G.gray8
    imgs = [make(2, 3), big, make(23, 31), np.ascontiguousarray(big[:100, :40])]
    hints = _hint_lists(4)
    for upsample in ("linear", "joint"):
        e.set_batch_upsample(upsample)
        for slot, out in ((0, "source"), (1, "net")):
            e.set_ingest_filter("antialias")
            ab = np.empty((4, 2, R.H, R.W), np.float32)
            outs = e.forward_async_gray(slot, imgs, hints, out_ab=ab, out=out)
            e.set_ingest_filter("bilinear")
            e.wait(slot)
            for i, src in enumerate(imgs):
                want, raw = _blocking(e, "antialias", src, hints[i], upsample, out)
                np.testing.assert_array_equal(outs[i], want, err_msg="image %d, %s, %s" % (i, out, upsample))
                np.testing.assert_array_equal(ab[i], raw)


def test_revealed_colours_and_score_targets_of_a_batch_equal_the_blocking_route(e):
    imgs = _ragged()
    c = _centres(e)
    rects = [list(RECTS[:i + 2]) for i in range(len(imgs))]
    e.set_ingest_filter("antialias")
    res = e.forward_async_dist(1, imgs, rects, mode="reveal", out="net", want_sse=True, want_rgb=True, peaks=0,
                               score=dict(centres=c, want_maps=True))
    e.wait(1)
    cols = np.array(res.hint_colours)
    at = 0
    for i, src in enumerate(imgs):
        e.set_image_rgb(src, keep_source=True)
        want_cols = e.reveal_hints(rects[i])
        _, rgb, _ = e.forward_resident(1)
        s = e.dist_score(c, n=1, want_maps=True)
        np.testing.assert_array_equal(cols[at:at + len(rects[i])], want_cols)
        at += len(rects[i])
        np.testing.assert_array_equal(res.out_rgb[i], rgb[0])
        np.testing.assert_array_equal(res.score.target[i], s.target[0])
        np.testing.assert_array_equal(res.score.truth_ab[i], s.truth_ab[0])
        assert res.score.xent[i] == s.xent[0]
        truth = R.resample(src)[1] if max(src.shape[:2]) > R.H else None
        if truth is not None:                                       # the net-size truth of sse is the rule's image
            d = res.out_rgb[i].astype(np.int64) - truth.astype(np.int64)
            assert [int(v) for v in res.sse[i]] == [sum(int(x) * int(x) for x in d[..., ch].ravel()) for ch in range(3)]


def test_evaluate_images_scores_against_the_rules_net_image(e):
    imgs = [R.case("rgb_211x83")[0], R.case("rgb_40x100")[0], R.case("rgb_128x128")[0]]
    items = [(im, RECTS[:3]) for im in imgs]
    e.set_ingest_filter("antialias")
    sse, _, outs = e.forward_async_eval(0, imgs, [RECTS[:3]] * 3, out="net", want_rgb=True)
    e.wait(0)
    sse, outs = np.array(sse), [np.array(o) for o in outs]
    e.set_ingest_filter("bilinear")
    got = list(e.evaluate_images(items, out="net", ingest="antialias"))
    assert e._ingest_filter == "bilinear" and len(got) == 3
    plain = list(e.evaluate_images(items, out="net"))
    for i, im in enumerate(imgs):
        d = outs[i].astype(np.int64) - R.case(["rgb_211x83", "rgb_40x100", "rgb_128x128"][i])[2].astype(np.int64)
        want = [sum(int(x) * int(x) for x in d[..., ch].ravel()) for ch in range(3)]
        assert [int(v) for v in sse[i]] == want
        assert [int(v) for v in got[i][1]] == want
        assert [int(v) for v in plain[i][1]] != want                 # the bilinear truth is another image


# ------------------------------------------------------------------------------------------------ 3b. nets of their own: the rare tilings
# (tests/resample_ref.py NET_CASES; tests/test_resample_cpu.py asserts the path each takes.)  The blocking cases run no forward: the handles of
# the 8-wide nets get no weights at all.
@pytest.fixture(scope="module")
def net_engines(make_sd):
    made = {}

    def get(net, weights=False):
        if net not in made:
            made[net] = [engine.HipColorizer(net[0], net[1], max_batch=4, precision="bf16"), False]
        if weights and not made[net][1]:
            made[net][0].load_state_dict(make_sd(0, "he"))
            made[net][1] = True
        made[net][0].set_ingest_filter("bilinear")
        made[net][0].set_batch_upsample("linear")
        return made[net][0]
    yield get
    for x, _ in made.values():
        x.close()


def _net_lab(want):
    return G.lightness(want) if want.ndim == 2 else ingest_ref.net_lab(want)


@pytest.mark.parametrize("name", sorted(n for n in R.NET_CASES if not n.startswith("n16x24")))
def test_blocking_ingestion_on_a_net_of_its_own_is_the_rule(net_engines, name):
    net = R.spec(name)[0]
    x = net_engines(net)
    assert (x.H, x.W) == net
    src, _, want = R.case(name)
    x.set_ingest_filter("antialias")
    got, lab = _ingest(x, src)
    x.set_ingest_filter("bilinear")
    got, lab = np.array(got), np.array(lab)
    assert got.dtype == src.dtype and got.shape == (1,) + want.shape
    print("%s: %d of %d samples differ from the rule" % (name, int((got[0] != want).sum()), want.size))
    np.testing.assert_array_equal(got[0], want)
    err = float(np.abs(lab[0] - _net_lab(want)).max())
    print("%s: Lab off by %.3e" % (name, err))
    assert err <= R.L_TOL


def _check_pipelined_against_blocking(x, imgs, hints, names):
    """One forward_async_images call under the filter: every image bit for bit the blocking route's, the named ones' net image the rule's."""
    n = len(imgs)
    for out in ("net", "source"):
        ab = np.empty((n, 2, x.H, x.W), np.float32)
        x.set_ingest_filter("antialias")
        outs = x.forward_async_images(0, imgs, hints, out_ab=ab, out=out)
        x.set_ingest_filter("bilinear")
        x.wait(0)
        assert np.isfinite(x.pipeline_times(0)).all()
        for i, src in enumerate(imgs):
            want, raw = _blocking(x, "antialias", src, hints[i], "linear", out)
            assert outs[i].shape == want.shape
            np.testing.assert_array_equal(outs[i], want, err_msg="image %d, %s" % (i, out))
            np.testing.assert_array_equal(ab[i], raw, err_msg="image %d, %s" % (i, out))
    x.set_ingest_filter("antialias")
    for i, name in enumerate(names):
        if name is not None:
            np.testing.assert_array_equal(np.array(x.set_image_rgb(imgs[i])[0][0]), R.case(name)[2], err_msg=name)
    x.set_ingest_filter("bilinear")


def _net_hints(net, n):
    rows = [(1, 2, net[0] // 2, net[1] // 2, 35.0, -50.0), (net[0] // 3, net[1] // 4, net[0] - 2, net[1] - 1, -30.0, 45.0)]
    return [rows[:i % 2 + 1] if i != 2 else None for i in range(n)]


def test_a_ragged_batch_on_the_40x72_net_equals_the_blocking_route(net_engines):
    x = net_engines((40, 72), weights=True)
    names = ["n40x72_rgb_211x83", "n40x72_rgb_100x40", None, "n40x72_rgb_50x200"]
    imgs = [_small(7, 9, 3) if nm is None else np.ascontiguousarray(R.case(nm)[0]) for nm in names]
    _check_pipelined_against_blocking(x, imgs, _net_hints((40, 72), 4), names)


def test_one_chunked_job_among_small_ones_on_the_16x24_net_equals_the_blocking_route(net_engines):
    """One job of 24 one-column tiles of up to two chunks beside a job of one tile and an image that skips the pre-pass: the workgroups past an
    image's own tile count return, at the widest spread the job table has."""
    x = net_engines((16, 24), weights=True)
    names = ["n16x24_rgb_3x16384", "n16x24_rgb_30x50", None]
    imgs = [_small(7, 9, 4) if nm is None else np.ascontiguousarray(R.case(nm)[0]) for nm in names]
    _check_pipelined_against_blocking(x, imgs, _net_hints((16, 24), 3), names)
    _check_pipelined_against_blocking(x, imgs[::-1], _net_hints((16, 24), 3), names[::-1])


# ------------------------------------------------------------------------------------------------ 4. references
def test_reference_statistics_follow_the_filter(engines):
    g = engines("g", global_hints=True)
    c = glob_ref.centres()
    refs = [R.case("rgb_211x83")[0], R.case("rgb_30x50")[0], R.case("rgb_700x1000")[0], R.case("rgb_64x64")[0]]
    g.set_ingest_filter("bilinear")
    hist_off, _ = g.global_stats_rgb(refs, c)
    g.set_ingest_filter("antialias")
    try:
        hist, sat = g.global_stats_rgb(refs, c)
        nblk = (R.H // 4) * (R.W // 4)
        for k, r in enumerate(refs):
            net = R.resample(r)[1]
            old_h, old_s = g.global_histogram(net, c)
            np.testing.assert_array_equal(np.rint(hist[k].astype(np.float64) * nblk), np.rint(old_h[0].astype(np.float64) * nblk))
            np.testing.assert_array_equal(hist[k], old_h[0])
            print("reference %s: s_avg %.9g, existing route on the rule's image %.9g" % (r.shape, sat[k], old_s[0]))
            assert abs(float(sat[k]) - float(old_s[0])) <= float(np.spacing(old_s[0]))
        assert (hist[0] != hist_off[0]).any() and (hist[2] != hist_off[2]).any()
        np.testing.assert_array_equal(hist[1], hist_off[1])
        np.testing.assert_array_equal(hist[3], hist_off[3])
        h1, s1 = g.global_stats_rgb([refs[2]], c)                   # alone: the very bits
        np.testing.assert_array_equal(h1[0], hist[2])
        assert s1.view(np.uint32)[0] == sat.view(np.uint32)[2]
        # a batch that brings its references equals the blocking route: set_global_refs, ingest, forward
        imgs = np.ascontiguousarray(np.stack([R.case("rgb_128x128")[0], R.case("rgb_128x128")[0][::-1]]))
        idx = [2, 0]
        got = np.zeros((2, R.H, R.W, 3), np.uint8)
        ab = np.empty((2, 2, R.H, R.W), np.float32)
        g.forward_async_rgb(1, imgs, [HINTS, None], got, out_ab=ab, refs=refs, ref_index=idx, centres=c, saturation=True)
        g.wait(1)
        g.set_global_refs(refs, c, ref_index=idx, saturation=True)
        g.set_image_rgb(imgs)
        g.set_hints(HINTS, img=0)
        g.set_hints([], img=1)
        raw, rgb, _ = g.forward_resident(2)
        np.testing.assert_array_equal(ab, raw)
        np.testing.assert_array_equal(got, rgb)
        g.set_ingest_filter("bilinear")
        g.set_global_refs(refs, c, ref_index=idx, saturation=True)
        g.set_ingest_filter("antialias")
        g.set_image_rgb(imgs)
        assert (g.forward_resident(2)[0] != raw).any()             # the references were read, and under the filter
    finally:
        g.set_ingest_filter("bilinear")
        g.clear_global_hints()


# ------------------------------------------------------------------------------------------------ 5. what it is for, and switching back
def test_stripes_on_the_device(e):
    s = R.stripes()
    e.set_ingest_filter("antialias")
    aa = np.array(e.set_image_gray(s)[0][0])
    rgb = np.array(e.set_image_rgb(np.repeat(s[..., None], 3, 2))[0][0])
    e.set_ingest_filter("bilinear")
    bl = np.array(e.set_image_gray(s)[0][0])
    print("stripes on the device: bilinear %d..%d, antialias %d..%d" % (bl.min(), bl.max(), aa.min(), aa.max()))
    assert aa.min() >= 123 and aa.max() <= 132
    assert bl.min() == 16 and bl.max() == 239
    np.testing.assert_array_equal(rgb, np.repeat(aa[..., None], 3, 2))


def _fixed_calls(x):
    """Every output of a fixed set of calls on handle x."""
    big, small = R.case("rgb_211x83")[0], R.case("rgb_30x50")[0]
    res = [np.array(a) for a in x.set_image_rgb(big, keep_source=True)]
    res += _forward(x) + [np.array(x.fullres_rgb("output_ab", "joint")), np.array(x.reveal_hints(RECTS))]
    res += [np.array(a) for a in x.set_image_gray(R.case("gray16_211x83")[0])]
    for out in ("net", "source"):
        ab = np.empty((2, 2, R.H, R.W), np.float32)
        outs = x.forward_async_images(0, [big, small], [HINTS, None], out_ab=ab, out=out)
        x.wait(0)
        res += [np.array(o) for o in outs] + [ab]
    return res


def test_switching_back_restores_every_bit_and_statuses(engines):
    x = engines("x")                                                # a handle whose filter was never set
    before = _fixed_calls(x)
    x.set_ingest_filter("antialias")
    during = _fixed_calls(x)
    assert (during[0] != before[0]).any()
    lib, h = x.lib, x._h
    # an unknown value is refused and changes nothing: the state stays ANTIALIAS
    for bad in (2, -1, 7):
        assert lib.idc_set_ingest_filter(h, bad) == -1
    assert b"filter" in lib.idc_last_error(h)
    for a, b in zip(during, _fixed_calls(x)):
        np.testing.assert_array_equal(a, b)
    assert lib.idc_set_ingest_filter(h, N.IDC_FILTER_BILINEAR) == 0
    x._ingest_filter = "bilinear"
    for a, b in zip(before, _fixed_calls(x)):
        np.testing.assert_array_equal(a, b)
    # a refused pipelined call leaves its slot usable, under the filter too
    x.set_ingest_filter("antialias")
    try:
        big = R.case("rgb_211x83")[0]
        tab = (N.RefImage * 2)()
        out = np.zeros((2, R.H, R.W, 3), np.uint8)
        outs = (ctypes.c_void_p * 2)(out[0].ctypes.data, out[1].ctypes.data)
        for i in range(2):
            tab[i].rgb, tab[i].h, tab[i].w = big.ctypes.data, big.shape[0], big.shape[1]
        tab[1].h = 16385
        assert lib.idc_forward_async_images(h, 1, 2, tab, None, None, 0, 1.0, 0.0, 50.0, 0, None, outs, None) == -1
        assert lib.idc_forward_async_images(h, 1, 2, tab, None, None, 0, 1.0, 0.0, 50.0, 8, None, outs, None) == -1
        tab[1].h = big.shape[0]
        assert lib.idc_forward_async_images(h, 1, 2, tab, None, None, 0, 1.0, 0.0, 50.0, 0, None, outs, None) == 0
        assert lib.idc_forward_async_images(h, 1, 2, tab, None, None, 0, 1.0, 0.0, 50.0, 0, None, outs, None) == -1     # in flight
        assert lib.idc_wait(h, 1) == 0
        x.set_image_rgb(big)
        x.set_hints([])
        np.testing.assert_array_equal(out[0], x.forward_resident(1)[1][0])
        np.testing.assert_array_equal(out[1], out[0])
    finally:
        x.set_ingest_filter("bilinear")
