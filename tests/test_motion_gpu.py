"""GPU checks of the block-matched motion compensation of the temporal ab filter: idc_set_temporal_motion / idc_temporal_vectors, through
idc_temporal_apply (the rule alone) and every pipelined entry point, through HipColorizer and the C ABI.  The reference is
tests/motion_ref.py -- the rule of include/ideepcolor.h in numpy float64 -- applied per frame from the device's OWN previous output: the
vectors exactly, y at the temporal file's bar (one float32 ulp, 99.9 % bit-equal, the flags equal, D to 1e-12).  The pipelined routes are held
against idc_temporal_apply + idc_temporal_vectors(-1) on a second handle of the raw out_ab the same call returns with the filter off, and their
images against the device's own blocking colour step on the filtered map (tests/test_temporal_gpu.py's method, l_cent = 0).
tests/test_motion_cpu.py shows that the first case's scenario catches twelve mutants of the rule.

Shapes: the rule alone on 8 x 8 (one block: only (0, 0) is valid), 8 x 72 (one block row: every dy != 0 is invalid), 40 x 72 (ragged tiles, an
H / W swap shows) and 64 x 64 nets, max_batch 8, no weights.  The pipelined cases: a 64 x 64 net, max_batch 8, bf16, seeded weights."""
import ctypes

import numpy as np
import pytest

import ingest_ref
import motion_ref as M
import temporal_ref as R
import test_temporal_gpu as TG
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import engine
from oracle import weights

pytestmark = pytest.mark.gpu

H = W = 64
VP = ctypes.c_void_p
BLEND = TG.BLEND
_bits, _same = TG._bits, TG._same


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


# ------------------------------------------------------------------------------------------------ 1. the rule alone
class _Dev(object):
    """motion_ref.play's view of an engine"""

    def __init__(self, x):
        self.x = x

    def set(self, **p):
        self.x.set_temporal_filter(**p)

    def motion(self, **mp):
        self.x.set_temporal_motion(**mp)

    def reset(self):
        self.x.temporal_reset()

    def state(self):
        return self.x.temporal_state()

    def apply(self, ab, l):
        y, cut, D = self.x.temporal_apply(ab, l)
        return y, cut, D, self.x.temporal_vectors(-1)


@pytest.mark.parametrize("net", M.NETS, ids=str)
def test_the_rule_alone(net):
    x = engine.HipColorizer(net[0], net[1], max_batch=M.MAX_BATCH, precision="bf16")
    try:
        frames = M.play(_Dev(x), net[0], net[1])
        print("%dx%d: %d frames: the vectors exact, y within the bar" % (net[0], net[1], frames))
        if net == (8, 8):        # one block, only (0, 0) valid: the plain filter bit for bit, whatever moves
            ab, l = R.frames(8, 8, 4, 3)
            x.set_temporal_filter(**dict(R.DEFAULT, cut=0.0))     # (the wandering patch is a ninth of this plane: every frame would be a cut)
            x.temporal_reset()
            y, cut, D = x.temporal_apply(ab, l)
            assert not x.temporal_vectors(-1).any()
            x.set_temporal_motion(None)
            x.temporal_reset()
            y0, cut0, D0 = x.temporal_apply(ab, l)
            assert _same(y, y0) and cut.tolist() == cut0.tolist() and D.tolist() == D0.tolist() and not _same(y, ab)
    finally:
        x.close()


# ------------------------------------------------------------------------------------------------ 2. search 0 is the plain filter
def test_search_zero_is_the_plain_filter_bit_for_bit_on_the_rule_alone():
    Hn, Wn = 40, 72
    x = engine.HipColorizer(Hn, Wn, max_batch=8, precision="bf16")
    try:
        calls = [R.frames(Hn, Wn, 1, 1), R.frames(Hn, Wn, 5, 2, cuts=(2,)), M.pan(Hn, Wn, 3, 3, (1, 2)), R.frames(Hn, Wn, 1, 4)]
        got = {}
        for motion in (False, True):
            x.set_temporal_filter(**R.DEFAULT)
            if motion:
                x.set_temporal_motion(search=0, penalty=0.5)
            else:
                x.set_temporal_motion(None)
            x.temporal_reset()
            out = []
            for ab, l in calls:
                y, cut, D = x.temporal_apply(ab, l)
                out.append((y, cut.tolist(), D.tolist(), x.temporal_state()))
                if motion:
                    assert not x.temporal_vectors(-1).any()
            got[motion] = out
        for (y, cut, D, st), (y0, cut0, D0, st0) in zip(got[True], got[False]):
            assert _same(y, y0) and cut == cut0 and D == D0                       # D: the same bits, not 1e-12
            assert _same(st[0], st0[0]) and _same(st[1], st0[1]) and st[2] == st0[2]
        assert any(0 in c[1] for c in got[False]) and any(1 in c[1][1:] for c in got[False])      # blended frames and a cut among them
    finally:
        x.close()


# ------------------------------------------------------------------------------------------------ 3. split invariance, device against device
def _pan_sources(n, step=(1, 2), seed=9):
    """n crops of one noise image, the window moving ``step`` pixels a frame: a pan at the net size (the crops are net-sized: no resampling)."""
    big = ingest_ref.source_image(H + 16, W + 24, seed)
    return [np.ascontiguousarray(big[f * step[0]:f * step[0] + H, f * step[1]:f * step[1] + W]) for f in range(n)]


def _run_parts(x, srcs, hints, parts, out, in_flight):
    """The frames as calls of `parts` images on alternating slots -> (out_ab, images, cut, D, vectors, state)."""
    x.temporal_reset()
    held, at = [], 0
    abs_, imgs, cuts, Ds, vs = [], [], [], [], []

    def collect(slot, res, ab, n):
        x.wait(slot)
        c, d = x.temporal_info(slot, n)
        abs_.append(np.array(ab)); imgs.extend(np.array(r) for r in res); cuts.append(c); Ds.append(d); vs.append(x.temporal_vectors(slot, n))

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
    return np.concatenate(abs_), imgs, np.concatenate(cuts), np.concatenate(Ds), np.concatenate(vs), x.temporal_state()


@pytest.mark.parametrize("out", ["net", "source"])
def test_a_sequence_gives_the_same_bits_however_it_is_split(e, out):
    srcs = _pan_sources(7)
    hints = [[(3, 4, 30, 40, 40.0, -30.0)] if k % 2 else [(3, 4, 30, 40, -20.0, 50.0)] for k in range(7)]
    e.set_temporal_filter(**dict(R.DEFAULT, cut=0.0))
    e.set_temporal_motion()
    try:
        whole = _run_parts(e, srcs, hints, [7], out, False)
        assert whole[2].tolist() == [1, 0, 0, 0, 0, 0, 0] and not whole[4][0].any()
        inner = whole[4][1:, 1:-1, 1:-1]
        assert (inner == np.array([1, 2], np.int8)).all(-1).mean() > 0.5, "the pan does not show in the vectors"
        for parts, in_flight in (([3, 4], True), ([1] * 7, False)):
            got = _run_parts(e, srcs, hints, parts, out, in_flight)
            assert _same(got[0], whole[0]), parts
            assert all(np.array_equal(a, b) for a, b in zip(got[1], whole[1])), parts
            assert got[2].tolist() == whole[2].tolist() and got[3].tolist() == whole[3].tolist(), parts      # D: the same bits
            assert np.array_equal(got[4], whole[4]), parts
            assert _same(got[5][0], whole[5][0]) and _same(got[5][1], whole[5][1]) and got[5][2] is True, parts
        assert _same(whole[5][0], whole[0][-1])
    finally:
        e.set_temporal_motion(None)
        e.set_temporal_filter(None)


def test_search_zero_is_the_plain_filter_on_a_pipelined_call(e):
    srcs = _pan_sources(5)
    hints = [[(3, 4, 30, 40, 40.0, -30.0)]] * 5
    e.set_temporal_filter(**BLEND)
    try:
        e.set_temporal_motion(None)
        plain = _run_parts_plain(e, srcs, hints)
        e.set_temporal_motion(search=0, penalty=0.0)
        got = _run_parts(e, srcs, hints, [5], "net", False)
        assert _same(got[0], plain[0]) and all(np.array_equal(a, b) for a, b in zip(got[1], plain[1]))
        assert got[2].tolist() == plain[2].tolist() and got[3].tolist() == plain[3].tolist() and not got[4].any()
        assert _same(got[5][0], plain[4][0]) and _same(got[5][1], plain[4][1])
    finally:
        e.set_temporal_motion(None)
        e.set_temporal_filter(None)


def _run_parts_plain(x, srcs, hints):
    """One call with motion off -> (out_ab, images, cut, D, state); idc_temporal_vectors then refuses the slot."""
    x.temporal_reset()
    n = len(srcs)
    ab = x.pinned_empty((n, 2, H, W), np.float32)
    res = x.forward_async_images(0, srcs, hints, None, ab, out="net")
    x.wait(0)
    c, d = x.temporal_info(0, n)
    with pytest.raises(N.IdcError) as err:
        x.temporal_vectors(0, n)
    assert err.value.status == -1
    return np.array(ab), [np.array(r) for r in res], c, d, x.temporal_state()


# ------------------------------------------------------------------------------------------------ 4. the pipelined routes
ROUTES = [(k, "net") for k in TG.KINDS] + [("images", "source"), ("gray8", "source")]
MOTION = dict(search=3, penalty=0.25)


@pytest.mark.parametrize("kind,out", ROUTES)
def test_pipelined_routes(e, eg, ed, e2, kind, out):
    x = eg if kind.endswith("_ref") else ed if kind.startswith("dist") else e
    srcs = TG._sources()
    # the filter off: the raw map, and everything the filter must leave alone
    x.set_temporal_filter(None)
    imgs0, ex0, seen = TG._call(x, kind, 0, out, srcs)
    raw = np.array(ex0["ab"])
    n = raw.shape[0]
    ex0 = {k: (None if v is None else np.array(v)) for k, v in ex0.items()}
    l, nets = TG._ingest_kept(x, seen)
    # the rule alone on the second handle
    e2.set_temporal_filter(**BLEND)
    e2.set_temporal_motion(**MOTION)
    e2.temporal_reset()
    try:
        want_y, want_cut, want_D = e2.temporal_apply(raw, l)
        want_v = e2.temporal_vectors(-1)
    finally:
        e2.set_temporal_motion(None)
    assert want_cut.tolist() == [1] + [0] * (n - 1)
    try:
        x.set_temporal_filter(**BLEND)
        x.set_temporal_motion(**MOTION)
        x.temporal_reset()
        imgs, ex1, _ = TG._call(x, kind, 1, out, srcs)
        imgs = [np.array(r) for r in imgs]
        cut, D = x.temporal_info(1)
        v = x.temporal_vectors(1)
    finally:
        x.set_temporal_motion(None)
        x.set_temporal_filter(None)
    y = np.array(ex1["ab"])
    assert np.array_equal(v, want_v) and v.shape == (n, H // 8, W // 8, 2) and not v[0].any()
    if kind not in ("rgb", "rgb_ref"):       # (those two send one image three times: nothing moves)
        assert v[1:].any()
    assert _same(y, want_y), "%s %s: out_ab is not idc_temporal_apply of the raw map (%d values differ)" % (kind, out, int((_bits(y) != _bits(want_y)).sum()))
    assert not _same(y, raw) and _same(y[0], raw[0])
    assert cut.tolist() == want_cut.tolist() and D.tolist() == want_D.tolist()
    # the images: the blocking colour step on the filtered map, bit for bit
    for i, (got, want) in enumerate(zip(imgs, TG._blocking_images(x, l, y, n, out))):
        assert np.array_equal(got, want), "%s %s image %d: %d bytes differ" % (kind, out, i, int((got != want).sum()))
    # what stays on the raw network: bit for bit the filter-off call's
    for key in ("peaks", "peak_ent", "entropy", "sc", "sf", "xent", "hits", "cells", "colours"):
        if ex0.get(key) is not None:
            assert np.array_equal(np.array(ex1[key]), ex0[key]), (kind, out, key)
    if ex0.get("sse") is not None:          # the score reads the filtered image
        sse = np.array(ex1["sse"])
        for i in range(n):
            truth = seen[i] if out == "source" else nets[i]
            assert [int(s) for s in sse[i]] == TG._sse(imgs[i], truth), (kind, out, i)


# ------------------------------------------------------------------------------------------------ 5. parameters in flight, statuses
def _enqueue(x, slot, srcs):
    ab = x.pinned_empty((len(srcs), 2, H, W), np.float32)
    res = x.forward_async_images(slot, srcs, [[(5, 5, 20, 20, 30.0, -20.0)]] * len(srcs), None, ab, out="net")
    return res, ab


def test_parameters_in_flight_motion_off_after_on_and_a_refused_call(e, e2):
    srcs = _pan_sources(6)
    e.set_temporal_filter(None)
    _, ab = _enqueue(e, 0, srcs)
    e.wait(0)
    raw = np.array(ab)
    l = np.stack([(np.array(e.set_image_rgb(s, want_rgb=False, want_lab=True)[1][0, 0]) - 50.0).astype(np.float32) for s in srcs])
    p = dict(R.DEFAULT, cut=0.0)
    m1, m2 = dict(search=2, penalty=0.0), dict(search=7, penalty=2.0)
    try:
        e.set_temporal_filter(**p)
        # the parent's bytes with the filter on: motion has never been on for this call
        e.temporal_reset()
        res, ab = _enqueue(e, 0, srcs[:3])
        e.wait(0)
        plain = ([np.array(r) for r in res], np.array(ab), e.temporal_info(0, 3))
        # two batches in flight each keep the motion parameters they were enqueued with
        e.temporal_reset()
        e.set_temporal_motion(**m1)
        _, a = _enqueue(e, 0, srcs[:3])
        e.set_temporal_motion(**m2)
        _, b = _enqueue(e, 1, srcs[3:])
        with pytest.raises(N.IdcError) as err:             # a slot still in flight has nothing to report yet
            e.temporal_vectors(0, 3)
        assert err.value.status == -1
        e.wait(0), e.wait(1)
        e2.set_temporal_filter(**p)
        e2.temporal_reset()
        e2.set_temporal_motion(**m1)
        ya = e2.temporal_apply(raw[:3], l[:3])[0]
        va = e2.temporal_vectors(-1)
        e2.set_temporal_motion(**m2)
        yb = e2.temporal_apply(raw[3:], l[3:])[0]
        vb = e2.temporal_vectors(-1)
        assert _same(np.array(a), ya) and _same(np.array(b), yb)
        assert np.array_equal(e.temporal_vectors(0, 3), va) and np.array_equal(e.temporal_vectors(1, 3), vb)
        assert np.abs(vb).max() <= 7 and np.abs(va).max() <= 2 and va[1:].any() and vb.any()
        # a refused setting changes nothing; a refused call (a slot in flight) leaves the slot usable and the state as it was
        assert e.lib.idc_set_temporal_motion(e._h, 1, 8, 0.5) == -1
        e.temporal_reset()
        _, a = _enqueue(e, 0, srcs[:3])
        with pytest.raises(N.IdcError):
            _enqueue(e, 0, srcs[3:])
        e.wait(0)
        e2.temporal_reset()
        ya = e2.temporal_apply(raw[:3], l[:3])[0]
        assert _same(np.array(a), ya) and np.array_equal(e.temporal_vectors(0, 3), e2.temporal_vectors(-1))
        _, b = _enqueue(e, 0, srcs[3:])
        e.wait(0)
        assert _same(np.array(b), e2.temporal_apply(raw[3:], l[3:])[0]) and np.array_equal(e.temporal_vectors(0, 3), e2.temporal_vectors(-1))
        # motion off after motion on: every byte is the parent's again, and the slot has no vectors to report
        e.set_temporal_motion(None)
        e.temporal_reset()
        res, ab = _enqueue(e, 0, srcs[:3])
        e.wait(0)
        assert _same(np.array(ab), plain[1]) and all(np.array_equal(r, q) for r, q in zip(res, plain[0]))
        assert e.temporal_info(0, 3)[0].tolist() == plain[2][0].tolist() and e.temporal_info(0, 3)[1].tolist() == plain[2][1].tolist()
        assert e.lib.idc_temporal_vectors(e._h, 0, np.zeros(1024, np.int8).ctypes.data_as(VP)) == -1
        # with the filter off motion does nothing: the raw map
        e.set_temporal_motion(**m1)
        e.set_temporal_filter(None)
        _, ab = _enqueue(e, 0, srcs)
        e.wait(0)
        assert _same(np.array(ab), raw)
        assert e.lib.idc_temporal_vectors(e._h, 0, np.zeros(1024, np.int8).ctypes.data_as(VP)) == -1
    finally:
        e.set_temporal_motion(None)
        e.set_temporal_filter(None)
        e2.set_temporal_motion(None)
        e2.set_temporal_filter(None)


def test_every_status_of_the_table():
    x = engine.HipColorizer(H, W, max_batch=4, precision="bf16")
    try:
        lib, h = x.lib, x._h
        nan = float("nan")
        x.set_temporal_motion(search=2, penalty=0.0)
        for bad in [(2, 4, 0.5), (-1, 4, 0.5), (1, -1, 0.5), (1, 8, 0.5), (1, 4, -0.1), (1, 4, 1.1e6), (1, 4, nan), (1, 4, float("inf"))]:
            assert lib.idc_set_temporal_motion(h, *bad) == -1, bad
        # a refused call changed nothing: search is still 2
        ab, l = M.pan(H, W, 2, 1, (0, 5))
        x.set_temporal_filter(**dict(R.DEFAULT, cut=0.0))
        buf = np.zeros((4, H // 8, W // 8, 2), np.int8)
        vp = buf.ctypes.data_as(VP)
        assert lib.idc_temporal_vectors(h, -2, vp) == -1 and lib.idc_temporal_vectors(h, 2, vp) == -1
        assert lib.idc_temporal_vectors(h, -1, None) == -1 and lib.idc_temporal_vectors(h, 0, None) == -1
        assert lib.idc_temporal_vectors(h, -1, vp) == -1                          # no idc_temporal_apply yet
        assert lib.idc_temporal_vectors(h, 0, vp) == -1                           # a slot that never ran
        x.temporal_apply(ab, l)
        v = x.temporal_vectors(-1)
        assert np.abs(v).max() <= 2 and v.shape == (2, H // 8, W // 8, 2)
        for good in [(1, 0, 0.0), (0, 7, 1e6), (1, 7, 1e6), (1, 5, 0.5)]:
            assert lib.idc_set_temporal_motion(h, *good) == 0, good
        x.temporal_reset()
        x.temporal_apply(ab, l)
        v = x.temporal_vectors(-1)
        assert (v[1, :, :-1] == np.array([0, 5], np.int8)).all() and not v[0].any()
        x.set_temporal_motion(None)
        x.temporal_apply(ab, l)
        assert lib.idc_temporal_vectors(h, -1, vp) == -1                          # the last apply ran without motion
    finally:
        x.close()


# ------------------------------------------------------------------------------------------------ 6. the claim
def test_the_flicker_on_a_moving_object_shrinks_by_the_closed_form():
    """The issue's sequence (motion_ref.claim_inputs): on the object's pixels whose chain kept the true vector and m == 0 in every frame, g = s
    exactly along the chain, so frame 11 against frame 10, FOLLOWED ALONG THE VECTOR, differs by (1 - s) / (1 + s) = 0.25 of the raw swing, to
    temporal_ref.swing_tolerance (the float32 rounding of the recursion and what is left of the transient, s^10).  With motion off the filter
    lets go on the object: at least 0.9 of the raw swing is left (median)."""
    c = M.CLAIM
    s, size, n = c["s"], c["size"], c["n"]
    ab, l, pos, (A_bg, B_bg, A_obj, B_obj) = M.claim_inputs()
    p = dict(R.DEFAULT, strength=s, cut=0.0)
    keep = M.claim_set(l, pos, p, M.DEFAULT)
    assert keep.sum() >= size * size // 4, "the claim set is only %d pixels" % int(keep.sum())
    x = engine.HipColorizer(c["H"], c["W"], max_batch=M.MAX_BATCH, precision="bf16")
    try:
        x.set_temporal_filter(**p)
        ys = {}
        for motion in (True, False):
            if motion:
                x.set_temporal_motion()
            else:
                x.set_temporal_motion(None)
            x.temporal_reset()
            y = np.concatenate([x.temporal_apply(ab[:8], l[:8])[0], x.temporal_apply(ab[8:], l[8:])[0]])
            ys[motion] = y
        raw = np.abs(A_obj.astype(np.float64) - B_obj.astype(np.float64))
        swing = {}
        for motion in (True, False):
            (ya, xa), (yb, xb) = pos[n - 1], pos[n - 2]
            last = ys[motion][n - 1][:, ya:ya + size, xa:xa + size].astype(np.float64)
            before = ys[motion][n - 2][:, yb:yb + size, xb:xb + size].astype(np.float64)
            swing[motion] = np.abs(last - before)
        want = (1.0 - s) / (1.0 + s) * raw
        tol = R.swing_tolerance(A_obj, B_obj, s, n - 1)
        err = np.abs(swing[True] - want)
        moved = raw > 1e-3
        ratio_on = float(np.median((swing[True] / raw)[moved & keep[None]]))
        ratio_off = float(np.median((swing[False] / raw)[moved & keep[None]]))
        print("claim set %d of %d pixels; filtered / raw swing: motion on %.6f, motion off %.6f; worst error / tolerance %.3g" %
              (int(keep.sum()), size * size, ratio_on, ratio_off, float((err / tol)[:, keep].max())))
        assert (err <= tol)[:, keep].all()
        assert ratio_off >= 0.9
    finally:
        x.close()
