"""GPU checks of the temporal ab filter: idc_temporal_apply (the rule alone), idc_set_temporal_filter on every pipelined entry point, the
sequence state and its ordering, through HipColorizer and the C ABI.  The reference is tests/temporal_ref.py -- the rule of
include/ideepcolor.h in numpy float64 -- applied per frame from the device's OWN previous output; the pipelined routes are held against
idc_temporal_apply on a second handle of the raw out_ab the same call returns with the filter off.  tests/test_temporal_cpu.py shows that the
first case's scenario catches ten mutants of the rule and that its bar is not tighter than one ulp of exp.

The images are held, bit for bit, against the device's own BLOCKING colour step on the filtered map: ``lab2rgb(L, y)`` for the net-size image
(it leaves the refreshed Lab resident), then ``fullres_rgb('output_ab', ...)`` from the sources kept by ``set_image_*(keep_source=True)`` for
the source-size one, linear, joint and 16-bit.  ``lab2rgb`` takes L itself as float32, the pipelined epilogue the slot's plane
(float)(L - l_cent) plus l_cent; the two are the same bits only if l_cent is 0, so every pipelined call of these cases is made with
l_cent = 0 (the network then sees L uncentred: other numbers, the same code).

Shapes: the rule alone on 8 x 8 (radius 3 is clipped at every pixel), 40 x 72 (six tiles, ragged last ones, an H / W swap shows) and 64 x 64
nets, max_batch 8, no weights.  The pipelined cases: a 64 x 64 net, max_batch 8, bf16, seeded weights, the sources of tests/test_ycc_gpu.py."""
import ctypes

import numpy as np
import pytest

import glob_ref
import gray_ref as G
import ingest_ref
import joint_ref as J
import ragged_ref
import temporal_ref as R
import ycc_ref
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import engine
from oracle import weights

pytestmark = pytest.mark.gpu

H = W = 64
L_CENT = 0.0                      # of every pipelined call whose image is checked: see the docstring
SIZES = ragged_ref.sizes(ragged_ref.MIXED, H, W) + [(83, 211)]      # 8 sources: one full batch
HINTS = [(3, 4, 10, 12, 20.0, -30.0), (50, 40, 55, 70, -15.0, 25.0), (20, 20, 22, 60, 40.0, 40.0)]
RECTS = [(3, 4, 10, 12), (50, 40, 55, 70), (0, 0, 63, 63)]
# the pipelined cases: no cut (the sources are different photographs: every frame would pass) and a wide sigma, so that every frame is blended
BLEND = dict(strength=0.6, sigma=100.0, radius=2, cut=0.0)
VP = ctypes.c_void_p


@pytest.fixture(scope="module")
def e(make_sd):
    x = engine.HipColorizer(H, W, max_batch=8, precision="bf16")
    x.load_state_dict(make_sd(0, "he"))
    yield x
    x.close()


@pytest.fixture(scope="module")
def eg():
    x = engine.HipColorizer(H, W, max_batch=8, precision="bf16", global_hints=True)
    x.load_state_dict(weights.add_global_branch(weights.make_state_dict(3, "he", include_class=False), 3))
    yield x
    x.close()


@pytest.fixture(scope="module")
def ed(make_sd):
    x = engine.HipColorizer(H, W, max_batch=8, precision="bf16", dist=True)
    x.load_state_dict(make_sd(0, "he"))
    yield x
    x.close()


@pytest.fixture(scope="module")
def e2():
    """The second handle: the rule alone, no weights."""
    x = engine.HipColorizer(H, W, max_batch=8, precision="bf16")
    yield x
    x.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ 1. the rule alone
class _Dev(object):
    """temporal_ref.play's view of an engine"""

    def __init__(self, x):
        self.x = x

    def set(self, **p):
        self.x.set_temporal_filter(**p)

    def reset(self):
        self.x.temporal_reset()

    def state(self):
        return self.x.temporal_state()

    def apply(self, ab, l):
        return self.x.temporal_apply(ab, l)


@pytest.mark.parametrize("net", R.NETS, ids=str)
def test_the_rule_alone(net):
    x = engine.HipColorizer(net[0], net[1], max_batch=R.MAX_BATCH, precision="bf16")
    try:
        assert x.temporal_state()[2] is False
        frames = R.play(_Dev(x), net[0], net[1])
        print("%dx%d: %d frames within the bar" % (net[0], net[1], frames))
        # the rule runs whether `on` is set or not
        x.set_temporal_filter(None)
        ab, l = R.frames(net[0], net[1], 2, 9)
        before = x.temporal_state()
        y, cut, D = x.temporal_apply(ab, l)
        R.verify_call(before, ab, l, R.DEFAULT, y, cut, D, "filter off")
    finally:
        x.close()


# ------------------------------------------------------------------------------------------------ 2. split invariance, device against device
def _run_parts(x, srcs, hints, parts, out, in_flight):
    """The frames as calls of `parts` images on alternating slots -> (out_ab, images, cut, D, state)."""
    x.temporal_reset()
    held, at = [], 0
    abs_, imgs, cuts, Ds = [], [], [], []

    def collect(slot, res, ab, n):
        x.wait(slot)
        c, d = x.temporal_info(slot, n)
        abs_.append(np.array(ab)); imgs.extend(np.array(r) for r in res); cuts.append(c); Ds.append(d)

    for k, n in enumerate(parts):
        slot = k & 1
        ab = x.pinned_empty((n, 2, H, W), np.float32)
        res = x.forward_async_images(slot, srcs[at:at + n], hints[at:at + n], None, ab, out=out)
        held.append((slot, res, ab, n))
        at += n
        if not in_flight or len(held) == 2:
            for hld in held:
                collect(*hld)
            held = []
    for hld in held:
        collect(*hld)
    return np.concatenate(abs_), imgs, np.concatenate(cuts), np.concatenate(Ds), x.temporal_state()


@pytest.mark.parametrize("out", ["net", "source"])
def test_a_sequence_gives_the_same_bits_however_it_is_split(e, out):
    rs = np.random.RandomState(4)
    base = ingest_ref.source_image(83, 101, 7).astype(np.int16)
    srcs = [np.ascontiguousarray(np.clip(base + rs.randint(-6, 7, base.shape), 0, 255).astype(np.uint8)) for _ in range(7)]       # one shot with grain
    hints = [[(3, 4, 30, 40, 40.0, -30.0)] if k % 2 else [(3, 4, 30, 40, -20.0, 50.0)] for k in range(7)]
    e.set_temporal_filter()
    try:
        whole = _run_parts(e, srcs, hints, [7], out, False)
        assert whole[2].tolist() == [1, 0, 0, 0, 0, 0, 0] and whole[3][0] == 0 and (whole[3][1:] > 0).all()
        for parts, in_flight in (([3, 4], True), ([1] * 7, False)):
            got = _run_parts(e, srcs, hints, parts, out, in_flight)
            assert _same(got[0], whole[0]), parts
            assert all(np.array_equal(a, b) for a, b in zip(got[1], whole[1])), parts
            assert got[2].tolist() == whole[2].tolist() and got[3].tolist() == whole[3].tolist(), parts      # D: the same bits
            assert _same(got[4][0], whole[4][0]) and _same(got[4][1], whole[4][1]) and got[4][2] is True, parts
        assert _same(whole[4][0], whole[0][-1])
    finally:
        e.set_temporal_filter(None)


# ------------------------------------------------------------------------------------------------ 3. the pipelined routes
def _sources():
    return [ragged_ref.image(h, w, 11 + i) for i, (h, w) in enumerate(SIZES)]


def _grid529():
    axis = np.arange(-110, 120, 10)
    return np.ascontiguousarray(np.array(np.meshgrid(axis, axis)).reshape((2, 529)).T.astype(np.float32))


def _call(x, kind, slot, out, srcs):
    """Enqueue one batch of `kind` on `slot` with l_cent = L_CENT and wait -> (images, every other result, the sources as the call saw them)."""
    n = len(srcs)
    hints = [None if i % 3 == 0 else HINTS[i % 3:] for i in range(n)]
    ab = x.pinned_empty((n, 2, H, W), np.float32)
    ex = {"ab": ab}
    kw = dict(out=out, l_cent=L_CENT)
    if kind in ("rgb", "rgb_ref"):
        batch = np.ascontiguousarray(np.stack([srcs[5]] * 3))
        d = batch.shape[1:3] if out == "source" else (H, W)
        dst = np.empty((3, d[0], d[1], 3), np.uint8)
        ab3 = x.pinned_empty((3, 2, H, W), np.float32)
        if kind == "rgb_ref":
            kw.update(refs=glob_ref.refs64()[:2], ref_index=[1, -1, 0], centres=glob_ref.centres(), saturation=True)
        x.forward_async_rgb(slot, batch, hints[:3], dst, ab3, **kw)
        x.wait(slot)
        return [dst[i] for i in range(3)], {"ab": ab3}, [srcs[5]] * 3
    seen = srcs
    if kind == "images":
        res = x.forward_async_images(slot, srcs, hints, None, ab, **kw)
    elif kind == "images_ref":
        res = x.forward_async_images(slot, srcs, hints, None, ab, refs=glob_ref.refs64()[:2], ref_index=[1, -1, 0, 1, 0, -1, 1, 0][:n],
                                     centres=glob_ref.centres(), **kw)
    elif kind == "eval":
        sse, cols, res = x.forward_async_eval(slot, srcs, [None if i % 3 == 0 else RECTS[i % 3:] for i in range(n)], None, ab, mode="reveal",
                                              want_rgb=True, **kw)
        ex.update(sse=sse, colours=cols)
    elif kind in ("dist", "dist_score"):
        c = _grid529()
        score = dict(centres=c, nn=2, sigma=5.0, ranks=(1, 5)) if kind == "dist_score" else None
        db = x.forward_async_dist(slot, srcs, hints, None, ab, want_sse=True, peaks=3, radius=2, skip_hints=True, queries="peaks", K=4, N_draws=64,
                                  seed=40, centres=c, want_entropy=True, score=score, want_rgb=True, **kw)
        res = db.out_rgb
        ex.update(sse=db.sse, peaks=db.peaks, peak_ent=db.peak_ent, entropy=db.entropy, sc=db.sugg_centres, sf=db.sugg_conf)
        if score:
            ex.update(xent=db.score.xent, hits=db.score.hits)
    elif kind == "gray8":
        seen = [np.ascontiguousarray(s[..., 1]) for s in srcs]
        res = x.forward_async_gray(slot, seen, hints, None, ab, **kw)
    elif kind == "layers":
        rs = np.random.RandomState(3)
        lays = [None if i % 2 else np.ascontiguousarray(rs.randint(0, 256, (9 + 5 * i, 12 + 3 * i, 4)).astype(np.uint8)) for i in range(n)]
        res, cells = x.forward_async_layers(slot, srcs, lays, [None if h is None else [r[:4] + (200.0, 30.0, 90.0) for r in h] for h in hints],
                                            None, ab, mode="rgb", **kw)
        ex.update(cells=cells)
    else:
        raise AssertionError(kind)
    x.wait(slot)
    return list(res), ex, seen


def _ingest_kept(x, seen):
    """The blocking ingestion of the frames into image slots 0 .. n-1, sources kept -> (the slots' fp32 L planes [n,H,W], the net-size images)."""
    ls, nets = [], []
    for i, s in enumerate(seen):
        if s.ndim == 2:
            net, l_net = x.set_image_gray(s, img=i, l_cent=L_CENT, keep_source=True, want_net=True, want_l=True)
            ls.append(G.l_plane(np.array(l_net[0]), L_CENT))
        else:
            net, lab = x.set_image_rgb(s, img=i, l_cent=L_CENT, keep_source=True, want_rgb=True, want_lab=True)
            ls.append((np.array(lab[0, 0]) - np.float64(np.float32(L_CENT))).astype(np.float32))
        nets.append(np.array(net[0]))
    return np.stack(ls), nets


def _blocking_images(x, l, y, n, out, interp="linear", depth=8):
    """The blocking colour step of the same handle on the map y: the net-size images of ``lab2rgb``, which leaves the refreshed Lab resident,
    and from it ``fullres_rgb`` of the sources ``_ingest_kept`` kept."""
    net, _ = x.lab2rgb(np.ascontiguousarray(l[:, None]), y, want_lab=True)
    if out == "net":
        return [np.array(net[i]) for i in range(n)]
    return [np.array(x.fullres_rgb("output_ab", interp, "image", img=i, depth=depth)) for i in range(n)]


def _sse(img, truth):
    d = np.asarray(img).astype(np.int64) - np.asarray(truth).astype(np.int64)
    return [int((d[..., c] ** 2).sum()) for c in range(3)]


KINDS = ["rgb", "rgb_ref", "images", "images_ref", "eval", "dist", "dist_score", "gray8", "layers"]


@pytest.mark.parametrize("out", ["net", "source"])
@pytest.mark.parametrize("kind", KINDS)
def test_pipelined_routes(e, eg, ed, e2, kind, out):
    x = eg if kind.endswith("_ref") else ed if kind.startswith("dist") else e
    srcs = _sources()
    # the filter off: the raw map, and everything the filter must leave alone
    x.set_temporal_filter(None)
    imgs0, ex0, seen = _call(x, kind, 0, out, srcs)
    imgs0 = [np.array(r) for r in imgs0]
    raw = np.array(ex0["ab"])
    n = raw.shape[0]
    ex0 = {k: (None if v is None else np.array(v)) for k, v in ex0.items()}
    l, nets = _ingest_kept(x, seen)
    # the rule alone on the second handle
    e2.set_temporal_filter(**BLEND)
    e2.temporal_reset()
    want_y, want_cut, want_D = e2.temporal_apply(raw, l)
    assert want_cut.tolist() == [1] + [0] * (n - 1)
    try:
        x.set_temporal_filter(**BLEND)
        x.temporal_reset()
        imgs, ex1, _ = _call(x, kind, 1, out, srcs)
        imgs = [np.array(r) for r in imgs]
        cut, D = x.temporal_info(1)
    finally:
        x.set_temporal_filter(None)
    y = np.array(ex1["ab"])
    assert _same(y, want_y), "%s %s: out_ab is not idc_temporal_apply of the raw map (%d values differ)" % (kind, out, int((_bits(y) != _bits(want_y)).sum()))
    assert not _same(y, raw) and _same(y[0], raw[0])
    assert cut.tolist() == want_cut.tolist() and D.tolist() == want_D.tolist()
    # the images: the blocking colour step on the filtered map, bit for bit -- and on the raw map it gives the filter-off call's (the check's own check)
    for i, (got, want) in enumerate(zip(imgs, _blocking_images(x, l, y, n, out))):
        assert np.array_equal(got, want), "%s %s image %d: %d bytes differ" % (kind, out, i, int((got != want).sum()))
    for i, (got, want) in enumerate(zip(imgs0, _blocking_images(x, l, raw, n, out))):
        assert np.array_equal(got, want), (kind, out, i)
    assert np.array_equal(imgs[0], imgs0[0]) and not all(np.array_equal(a, b) for a, b in zip(imgs, imgs0))
    # what stays on the raw network: bit for bit the filter-off call's
    for key in ("peaks", "peak_ent", "entropy", "sc", "sf", "xent", "hits", "cells", "colours"):
        if ex0.get(key) is not None:
            assert np.array_equal(np.array(ex1[key]), ex0[key]), (kind, out, key)
    if ex0.get("sse") is not None:          # the score reads the filtered image
        sse = np.array(ex1["sse"])
        for i in range(n):
            truth = seen[i] if out == "source" else nets[i]
            assert [int(v) for v in sse[i]] == _sse(imgs[i], truth), (kind, out, i)
        assert not np.array_equal(sse, ex0["sse"])


def _seq(x, gray, items, hints, out, depth=8, upsample=None, fmt=None):
    """One call on slot 0 from a fresh sequence, under the handle's filter setting -> (images, out_ab)."""
    x.temporal_reset()
    if upsample:
        x.set_batch_upsample(upsample)
    if fmt:
        x.set_batch_output(fmt, "bt709")
    try:
        ab = x.pinned_empty((len(items), 2, H, W), np.float32)
        if gray:
            res = x.forward_async_gray(0, items, hints, None, ab, out=out, depth=depth, l_cent=L_CENT)
        else:
            res = x.forward_async_images(0, items, hints, None, ab, out=out, l_cent=L_CENT)
        x.wait(0)
        return [np.array(r) for r in res], np.array(ab)
    finally:
        x.set_batch_upsample("linear")
        x.set_batch_output("rgb")


def test_sixteen_bit_grey_and_nv12_see_the_filtered_map(e, e2):
    n = 4
    planes = [G.gray16(97, 75, 20 + i) for i in range(n)]
    hints = G.hint_lists(n)
    e.set_temporal_filter(None)
    raw = _seq(e, True, planes, hints, "source")[1]
    l, _ = _ingest_kept(e, planes)
    e2.set_temporal_filter(**BLEND)
    e2.temporal_reset()
    want_y = e2.temporal_apply(raw, l)[0]
    e.set_temporal_filter(**BLEND)
    try:
        img8, y8 = _seq(e, True, planes, hints, "source")
        img16, y16 = _seq(e, True, planes, hints, "source", depth=16)
        blocks, yn = _seq(e, True, planes, hints, "source", fmt="nv12")
    finally:
        e.set_temporal_filter(None)
    assert _same(y8, want_y) and _same(y16, want_y) and _same(yn, want_y) and not _same(want_y, raw)
    want8 = _blocking_images(e, l, want_y, n, "source")
    want16 = _blocking_images(e, l, want_y, n, "source", depth=16)
    for i in range(n):
        # both depths: the blocking getter on the filtered map, bit for bit
        assert img8[i].dtype == np.uint8 and np.array_equal(img8[i], want8[i]), i
        assert img16[i].dtype == np.uint16 and np.array_equal(img16[i], want16[i]), i
        # NV12: the block of that RGB image, exactly
        assert np.array_equal(np.asarray(blocks[i]).reshape(-1), ycc_ref.block(img8[i], "nv12", "bt709")), i


def test_the_joint_upsampling_sees_the_filtered_map(e, e2):
    n = 3
    srcs = [J.source(97, 75), J.source(60, 111), J.source(97, 75)]
    hints = [J.HINTS, None, J.HINTS[:2]]
    e.set_temporal_filter(None)
    rawj, raw = _seq(e, False, srcs, hints, "source", upsample="joint")
    l, _ = _ingest_kept(e, srcs)
    e2.set_temporal_filter(**BLEND)
    e2.temporal_reset()
    want_y = e2.temporal_apply(raw, l)[0]
    e.set_temporal_filter(**BLEND)
    try:
        imgj, yj = _seq(e, False, srcs, hints, "source", upsample="joint")
    finally:
        e.set_temporal_filter(None)
    assert _same(yj, want_y)
    want = _blocking_images(e, l, want_y, n, "source", interp="joint")
    for i in range(n):       # fullres_rgb(interp='joint') of the blocking route on the filtered map, bit for bit
        assert np.array_equal(imgj[i], want[i]), (i, int((imgj[i] != want[i]).sum()))
        assert (i == 0) == bool(np.array_equal(imgj[i], rawj[i])), i      # frame 0 passes; the others are made of another map


# ------------------------------------------------------------------------------------------------ 4. state and ordering
def _frames_of_one_shot(n, seed=0):
    rs = np.random.RandomState(seed)
    base = ingest_ref.source_image(64, 64, 3).astype(np.int16)
    return [np.ascontiguousarray(np.clip(base + rs.randint(-5, 6, base.shape), 0, 255).astype(np.uint8)) for _ in range(n)]


def _enqueue(x, slot, srcs, hints=None):
    ab = x.pinned_empty((len(srcs), 2, H, W), np.float32)
    res = x.forward_async_images(slot, srcs, hints if hints is not None else [[(5, 5, 20, 20, 30.0, -20.0)]] * len(srcs), None, ab, out="net")
    return res, ab


def _state_same(a, b):
    return a[2] == b[2] and _same(a[0], b[0]) and _same(a[1], b[1])


def test_reset_in_flight_parameters_in_flight_and_what_leaves_the_state_alone(e, e2):
    srcs = _frames_of_one_shot(6)
    e.set_temporal_filter(None)
    # the parent's bytes: the filter has never been on for these two calls' results
    res, ab = _enqueue(e, 0, srcs[:3])
    e.wait(0)
    plain = ([np.array(r) for r in res], np.array(ab))
    res, ab = _enqueue(e, 1, srcs[3:])
    e.wait(1)
    plain2 = np.array(ab)
    l = np.stack([(np.array(e.set_image_rgb(s, want_rgb=False, want_lab=True)[1][0, 0]) - 50.0).astype(np.float32) for s in srcs])
    p1, p2 = dict(strength=0.5, sigma=8.0, radius=1, cut=12.0), dict(strength=0.9, sigma=2.0, radius=3, cut=0.0)
    try:
        # two batches in flight each keep the parameters they were enqueued with
        e.set_temporal_filter(**p1)
        e.temporal_reset()
        _, a = _enqueue(e, 0, srcs[:3])
        e.set_temporal_filter(**p2)
        _, b = _enqueue(e, 1, srcs[3:])
        with pytest.raises(N.IdcError) as err:             # a slot still in flight has nothing to report yet
            e.temporal_info(0, 3)
        assert err.value.status == -1
        e.wait(0), e.wait(1)
        e2.temporal_reset()
        e2.set_temporal_filter(**p1)
        ya = e2.temporal_apply(plain[1], l[:3])[0]
        e2.set_temporal_filter(**p2)
        yb, cb, Db = e2.temporal_apply(plain2, l[3:])
        assert _same(np.array(a), ya) and _same(np.array(b), yb) and not _same(yb, plain2)
        assert e.temporal_info(1, 3)[0].tolist() == cb.tolist() == [0, 0, 0] and e.temporal_info(1, 3)[1].tolist() == Db.tolist()
        # a reset between two calls in flight starts a new sequence
        e.set_temporal_filter(**p1)
        _, a = _enqueue(e, 0, srcs[:3])
        e.temporal_reset()
        _, b = _enqueue(e, 1, srcs[3:])
        e.wait(0), e.wait(1)
        cut, D = e.temporal_info(1, 3)
        assert cut.tolist() == [1, 0, 0] and D[0] == 0 and _same(np.array(b)[0], plain2[0]) and not _same(np.array(b)[1], plain2[1])
        assert e.temporal_info(0, 3)[0].tolist() == [0, 0, 0]
        state = e.temporal_state()
        assert state[2] and _same(state[0], np.array(b)[-1]) and _same(state[1], l[5])
        # a refused call leaves the state as it was: a slot in flight, too many images, a NULL image table
        _, a = _enqueue(e, 0, srcs[:3])
        with pytest.raises(N.IdcError):
            _enqueue(e, 0, srcs[3:])
        e.wait(0)
        state = e.temporal_state()
        assert e.lib.idc_forward_async_images(e._h, 1, 9, None, None, None, N.IDC_HINT_AB, 1.0, 0.0, 50.0, 0, None, None, None) == -6
        assert e.lib.idc_forward_async_images(e._h, 1, 2, None, None, None, N.IDC_HINT_AB, 1.0, 0.0, 50.0, 0, None, None, None) == -1
        assert _state_same(e.temporal_state(), state)
        # idc_forward_async (the caller's planes) and the blocking forwards are no sequences; the first leaves nothing to report on its slot
        z = np.zeros((2, 1, H, W), np.float32)
        o = e.pinned_empty((2, 2, H, W), np.float32)
        e.forward_async(1, z, np.zeros((2, 2, H, W), np.float32), z, o)
        e.wait(1)
        assert e.lib.idc_temporal_info(e._h, 1, np.zeros(8, np.int32).ctypes.data_as(VP), None) == -1
        e.forward(z, np.zeros((2, 2, H, W), np.float32), z)
        e.set_image_rgb(srcs[0], keep_source=True)
        e.set_hints([(5, 5, 20, 20, 30.0, -20.0)])
        e.forward_resident(1)
        e.fullres_rgb("output_ab", "linear", "image")
        assert _state_same(e.temporal_state(), state)
        # a call with the filter off leaves the state as it was, reports nothing, and every byte of it is the parent's again
        e.set_temporal_filter(None)
        res, ab = _enqueue(e, 0, srcs[:3])
        e.wait(0)
        assert _same(np.array(ab), plain[1]) and all(np.array_equal(r, q) for r, q in zip(res, plain[0]))
        assert _state_same(e.temporal_state(), state)
        with pytest.raises(N.IdcError) as err:
            e.temporal_info(0, 3)
        assert err.value.status == -1
        # ... and the sequence goes on where it stood
        e.set_temporal_filter(**p1)
        _, a = _enqueue(e, 0, srcs[:3])
        e.wait(0)
        assert e.temporal_info(0, 3)[0].tolist() == [0, 0, 0] and not _same(np.array(a)[0], plain[1][0])
    finally:
        e.set_temporal_filter(None)


def test_every_status_of_the_table(e2):
    lib, h = e2.lib, e2._h
    e2.set_temporal_filter(0.5, sigma=4.0, radius=1, cut=12.0)
    nan = float("nan")
    for bad in [(2, 0.6, 4.0, 1, 12.0), (-1, 0.6, 4.0, 1, 12.0), (1, -0.1, 4.0, 1, 12.0), (1, 0.96, 4.0, 1, 12.0), (1, nan, 4.0, 1, 12.0),
                (1, 0.6, 0.4, 1, 12.0), (1, 0.6, 101.0, 1, 12.0), (1, 0.6, nan, 1, 12.0), (1, 0.6, 4.0, -1, 12.0), (1, 0.6, 4.0, 4, 12.0),
                (1, 0.6, 4.0, 1, -1.0), (1, 0.6, 4.0, 1, 100.5), (1, 0.6, 4.0, 1, nan)]:
        assert lib.idc_set_temporal_filter(h, *bad) == -1, bad
    for good in [(1, 0.0, 0.5, 0, 0.0), (0, 0.95, 100.0, 3, 100.0), (1, 0.5, 4.0, 1, 12.0)]:
        assert lib.idc_set_temporal_filter(h, *good) == 0, good
    # a refused call changed nothing: identical planes still blend with strength 0.5 exactly
    ab, l = R.frames(H, W, 2, 1, still=np.zeros((H, W), np.float32))
    e2.temporal_reset()
    y = e2.temporal_apply(ab, l)[0]
    want = (ab[1].astype(np.float64) + 0.5 * (ab[0].astype(np.float64) - ab[1].astype(np.float64))).astype(np.float32)
    assert _same(y[1], want)
    f = np.zeros((9, 2, H, W), np.float32)
    p = f.ctypes.data_as(VP)
    assert lib.idc_temporal_apply(h, 0, p, p, p, None, None) == -6 and lib.idc_temporal_apply(h, 9, p, p, p, None, None) == -6
    assert lib.idc_temporal_apply(h, 1, None, p, p, None, None) == -1 and lib.idc_temporal_apply(h, 1, p, None, p, None, None) == -1
    assert lib.idc_temporal_apply(h, 1, p, p, None, None, None) == -1
    assert lib.idc_temporal_apply(h, 1, p, p, p, None, None) == 0            # cut and D are optional
    c = np.zeros(8, np.int32).ctypes.data_as(VP)
    assert lib.idc_temporal_info(h, 2, c, None) == -1 and lib.idc_temporal_info(h, -1, c, None) == -1
    assert lib.idc_temporal_info(h, 0, None, None) == -1
    assert lib.idc_temporal_info(h, 0, c, None) == -1                        # a slot that never ran
    assert lib.idc_temporal_state(h, None, None, None) == 0                  # every pointer may be NULL
    assert lib.idc_temporal_reset(h) == 0 and e2.temporal_state()[2] is False
    e2.set_temporal_filter(None)


def test_more_frames_than_one_chunk_of_flags():
    """The blend kernel keeps the cut flags of 1024 frames in LDS at a time: a call of 1030 frames, with a cut on either side of the boundary."""
    n = 1030
    x = engine.HipColorizer(8, 8, max_batch=n, precision="bf16")
    try:
        ab, l = R.frames(8, 8, n, 3, cuts=(1023, 1024, 1029))
        y, cut, D = x.temporal_apply(ab, l)
        R.verify_call((ab[0], l[0], False), ab, l, R.DEFAULT, y, cut, D, "1030 frames")         # every frame, from the device's previous output
        assert cut[1023] == 1 and cut[1024] == 1 and cut[1029] == 1 and 0 in cut[:1023] and 0 in cut[1025:1029]
    finally:
        x.close()


# ------------------------------------------------------------------------------------------------ 5. the flicker claim
def test_the_flicker_of_a_toggled_hint_shrinks_by_the_closed_form(e):
    """One image, identical L in every frame, a hint toggled on alternate frames: 40 frames as five calls of eight.  g = s exactly, so the
    steady-state swing of out_ab is (1 - s) / (1 + s) of the raw swing, to temporal_ref.swing_tolerance: the float32 rounding of the
    recursion and what is left of the transient, s^39."""
    s = 0.6
    src = ingest_ref.source_image(64, 64, 11)
    hints = [[(10, 10, 40, 40, 60.0, -40.0)] if k % 2 else None for k in range(8)]

    def run():
        frames = []
        for k in range(5):
            _, ab = _enqueue(e, k & 1, [src] * 8, hints)
            e.wait(k & 1)
            frames.append(np.array(ab))
        return np.concatenate(frames)

    e.set_temporal_filter(None)
    raw = run()
    A, B = raw[0], raw[1]
    assert all(_same(raw[k], raw[k % 2]) for k in range(40)) and float(np.abs(A - B).max()) > 1.0
    e.set_temporal_filter(strength=s)
    e.temporal_reset()
    try:
        y = run()
    finally:
        e.set_temporal_filter(None)
    swing = np.abs(y[39].astype(np.float64) - y[38].astype(np.float64))
    want = (1.0 - s) / (1.0 + s) * np.abs(A.astype(np.float64) - B.astype(np.float64))
    tol = R.swing_tolerance(A, B, s, 39)
    err = np.abs(swing - want)
    moved = np.abs(A - B) > 1e-3
    print("raw swing up to %.3f, filtered / raw %.6f on %d values, worst error / tolerance %.3g" %
          (float(np.abs(A - B).max()), float((swing[moved] / np.abs(A.astype(np.float64) - B)[moved]).mean()), int(moved.sum()), float((err / tol).max())))
    assert (err <= tol).all()
