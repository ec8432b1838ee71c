"""GPU checks of the hint tracking along the motion vectors: idc_set_hint_tracking / idc_tracked_hints / idc_track_hints_apply, through
HipColorizer and the C ABI.  The reference is tests/track_ref.py -- the RECURSION of the rule of include/ideepcolor.h frame by frame in plain
loops, with tests/motion_ref.py's vectors -- and every comparison of planes, ages and vectors is bit for bit.  The pipelined routes are held to
it on the call's own inputs (the own planes: what the same device wrote for each frame alone, as the first frame of a sequence, where tracked =
own; the L planes: the blocking ingestion's) and the device's OWN previous state, and their out_ab to the same handle's network on the tracked
planes (idc_forward_async: the caller's planes, no sequence) followed by the filter on a second handle.
tests/test_track_cpu.py holds the inputs to their conditions and shows which mutants of the rule each of them tells apart.

The pipelined sources are net-sized (64 x 64) crops, so that the pan is exact at the net size and L repeats bit for bit along the vectors:
out='source' on the _images and _gray routes therefore runs the source-size kernels at scale 1 only.  What tracking changes ends at the net-size
out_ab; the source-size kernels behind it at other scales are tests/test_temporal_gpu.py's and tests/test_motion_gpu.py's ground.

Shapes: the rule alone on 8 x 8 (one block: the vector is (0, 0)), 8 x 72 (one block row), 40 x 72 (ragged tiles, an H / W swap shows) and
64 x 64 nets, max_batch 8 (12 for the claim), no weights.  The pipelined cases: a 64 x 64 net, max_batch 8, bf16, seeded weights."""
import ctypes

import numpy as np
import pytest

import dist_batch_ref as DB
import glob_ref
import motion_ref as M
import temporal_ref as R
import test_temporal_gpu as TG
import track_ref as T
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import engine
from oracle import weights

pytestmark = pytest.mark.gpu

H = W = 64
VP = ctypes.c_void_p
FILTER = dict(R.DEFAULT, cut=0.0)
_same = TG._same


def _same3(got, want):
    """(A, M, G) against (A, M, G): the floats by their bits, the ages by value."""
    return _same(got[0], want[0]) and _same(got[1], want[1]) and got[2].dtype == np.int32 and np.array_equal(got[2], want[2])


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
    """The second handle: the rules alone, no weights."""
    x = engine.HipColorizer(H, W, max_batch=8, precision="bf16")
    yield x
    x.close()


# ------------------------------------------------------------------------------------------------ 1. the rule alone
@pytest.mark.parametrize("net", T.NETS, ids=str)
def test_the_rule_alone(net):
    x = engine.HipColorizer(net[0], net[1], max_batch=T.MAX_BATCH, precision="bf16")
    try:
        before = x.temporal_state()
        frames = closed = 0
        for c in T.cases(net[0], net[1]):
            x.set_temporal_motion(**c["mp"])
            x.set_hint_tracking(**c["tp"])
            A, Mk, G, v = x.track_hints_apply(c["l"], c["ab"], c["mask"], vectors=True)
            want_v = T.call_vectors(c["l"], None, c["mp"])
            assert np.array_equal(v, want_v), "%s: %s: the vectors are not the motion rule's" % (net, c["name"])
            want = T.sequence(c["l"], c["ab"], c["mask"], want_v, None, c["tp"]["life"], c["tp"]["tol"], rule=T.frame_loops)
            assert _same3((A, Mk, G), want), "%s: %s: %d mask values, %d ages differ" % (net, c["name"], int((Mk != want[1]).sum()), int((G != want[2]).sum()))
            closed += T.check_case(c, A, Mk, G, v)
            frames += c["l"].shape[0]
        print("%dx%d: %d frames bit for bit, closed forms on %d" % (net[0], net[1], frames, closed))
        assert closed >= (100 if net[0] >= 40 else 10)
        # the handle's sequence state was neither read nor written, and the rule runs with the switch off as well
        assert x.temporal_state()[2] is False and before[2] is False
        x.set_hint_tracking(None)
        c = T.cases(net[0], net[1])[0]
        x.set_temporal_motion(**c["mp"])
        got = x.track_hints_apply(c["l"], c["ab"], c["mask"])
        assert _same3(got, T.sequence(c["l"], c["ab"], c["mask"], T.call_vectors(c["l"], None, c["mp"]), None, 0, 8.0))
    finally:
        x.close()


# ------------------------------------------------------------------------------------------------ 2. the pipelined routes
_sources = T.grey_pan_sources
RECT_A, RECT_B = T.RECT_A, T.RECT_B
KINDS = ["rgb", "rgb_ref", "images", "eval", "dist", "dist_score", "gray8", "layers"]


def _enqueue(x, kind, slot, out, srcs, hints):
    """One batch of ``kind`` on ``slot`` with l_cent = 0, NOT waited for -> (images, out_ab, what else came back, the sources as the call saw them).
    hints: per frame None or a list of (y0, x0, y1, x1, a, b) rows."""
    n = len(srcs)
    ab = x.pinned_empty((n, 2, H, W), np.float32)
    ex, seen = {}, srcs
    kw = dict(out=out, l_cent=TG.L_CENT)
    if kind in ("rgb", "rgb_ref"):
        batch = np.ascontiguousarray(np.stack(srcs))
        dst = np.empty((n, H, W, 3), np.uint8)
        if kind == "rgb_ref":
            kw.update(refs=glob_ref.refs64()[:2], ref_index=[1, -1, 0, 1, 0, -1, 1, 0][:n], centres=glob_ref.centres(), saturation=True)
        x.forward_async_rgb(slot, batch, hints, dst, ab, **kw)
        res = [dst[i] for i in range(n)]
    elif kind == "images":
        res = x.forward_async_images(slot, srcs, hints, None, ab, **kw)
    elif kind == "eval":
        sse, cols, res = x.forward_async_eval(slot, srcs, [None if h is None else [r[:4] for r in h] for h in hints], None, ab, mode="reveal",
                                              want_rgb=True, **kw)
        ex.update(colours=cols)
    elif kind in ("dist", "dist_score"):
        c = TG._grid529()
        score = dict(centres=c, nn=2, sigma=5.0, ranks=(1, 5)) if kind == "dist_score" else None
        db = x.forward_async_dist(slot, srcs, hints, None, ab, peaks=256, radius=1, skip_hints=True, centres=c, want_entropy=True, score=score,
                                  want_rgb=True, **kw)
        res = db.out_rgb
        ex.update(peaks=db.peaks, entropy=db.entropy)
    elif kind == "gray8":
        seen = [np.ascontiguousarray(s[..., 1]) for s in srcs]
        res = x.forward_async_gray(slot, seen, hints, None, ab, **kw)
    elif kind == "layers":
        lays = []
        for h in hints:         # a painted blob beside the first rectangle: the layer kernel writes the own planes too
            if h is None or h[0] != RECT_A:
                lays.append(None)
                continue
            lay = np.zeros((16, 16, 4), np.uint8)
            lay[8:11, 10:13] = (200, 30, 90, 255)          # net rows 32..43, columns 40..51: clear of both rectangles' paths and of the border blocks
            lays.append(lay)
        res, cells = x.forward_async_layers(slot, srcs, lays, [None if h is None else [r[:4] + (30.0, 200.0, 90.0) for r in h] for h in hints], None, ab,
                                            mode="rgb", **kw)
        ex.update(cells=cells)
    else:
        raise AssertionError(kind)
    return list(res), ab, ex, seen


def _call(x, kind, slot, out, srcs, hints):
    res, ab, ex, seen = _enqueue(x, kind, slot, out, srcs, hints)
    x.wait(slot)
    return [np.array(r) for r in res], np.array(ab), {k: (None if v is None else np.array(v)) for k, v in ex.items()}, seen


def _own_planes(x, kind, srcs, hints):
    """What the device's prologue (and layer kernel, and revealed colours) writes for each frame: the tracked planes of the frame ALONE, as the
    first frame of a sequence, where the rule says tracked = own."""
    abs_, masks = [], []
    for s, h in zip(srcs, hints):
        x.temporal_reset()
        _call(x, kind, 0, "net", [s], [h])
        A, Mk, G = x.tracked_hints(0, 1)
        assert not G.any() and (Mk != 0).any() == (h is not None)
        abs_.append(A[0]), masks.append(Mk[0])
    return np.stack(abs_), np.stack(masks)


def _network_on(x, l, A, Mk):
    """The same handle's network on the planes (A, Mk) as own hints, no sequence and no tracking: idc_forward_async, the caller's planes."""
    n = l.shape[0]
    out = x.pinned_empty((n, 2, H, W), np.float32)
    x.forward_async(0, np.ascontiguousarray(l[:, None]), np.ascontiguousarray(A), np.ascontiguousarray(Mk[:, None]), out)
    x.wait(0)
    return np.array(out)


def _planes_as_hints(A, Mk):
    """Tracked planes (A [n,2,H,W], Mk [n,H,W]) as per-frame hint lists in 'ab' mode: one one-row rectangle per run of equal (a, b) -- the
    planes bit for bit, since every mask value here is mask_value = 1.0 and a hint's floats are stored as they are."""
    out = []
    for a, m in zip(A, Mk):
        assert set(np.unique(m).tolist()) <= {0.0, 1.0}
        rows = []
        for y in range(H):
            x = 0
            while x < W:
                if m[y, x] == 0:
                    x += 1
                    continue
                x1 = x
                while x1 + 1 < W and m[y, x1 + 1] != 0 and a[0, y, x1 + 1] == a[0, y, x] and a[1, y, x1 + 1] == a[1, y, x]:
                    x1 += 1
                rows.append((y, x, y, x1, float(a[0, y, x]), float(a[1, y, x])))
                x = x1 + 1
        out.append(rows or None)
    return out


AB_KINDS = ("rgb", "rgb_ref", "images", "dist", "dist_score", "gray8")      # their hints are (a, b) rectangles: planes can be fed as hints


@pytest.mark.parametrize("kind,out", [(k, "net") for k in KINDS] + [("images", "source"), ("gray8", "source")])
def test_pipelined_routes(e, eg, ed, e2, kind, out):
    x = eg if kind.endswith("_ref") else ed if kind.startswith("dist") else e
    srcs = _sources(6)
    hints = [[RECT_A], None, [RECT_B], None, None, None]
    mp, tp = dict(M.DEFAULT), dict(T.DEFAULT)
    x.set_temporal_filter(**FILTER)
    x.set_temporal_motion(**mp)
    x.set_hint_tracking(**tp)
    try:
        own_ab, own_mask = _own_planes(x, kind, srcs, hints)
        # the sequence as two calls, both in flight: the second call's frame 0 reads the state the first one leaves
        x.temporal_reset()
        first = _enqueue(x, kind, 0, out, srcs[:3], hints[:3])
        second = _enqueue(x, kind, 1, out, srcs[3:], hints[3:])
        with pytest.raises(N.IdcError) as err:             # a slot still in flight has nothing to report yet
            x.tracked_hints(1, 3)
        assert err.value.status == -1
        x.wait(0), x.wait(1)
        got = [x.tracked_hints(0, 3), x.tracked_hints(1, 3)]
        vs = [x.temporal_vectors(0, 3), x.temporal_vectors(1, 3)]
        y = np.concatenate([np.array(first[1]), np.array(second[1])])
        imgs = [np.array(r) for r in first[0] + second[0]]
        ex = {k: np.array(v) for k, v in second[2].items() if v is not None}
        seen = first[3] + second[3]
    finally:
        x.set_hint_tracking(None)
        x.set_temporal_motion(None)
        x.set_temporal_filter(None)
    l, nets = TG._ingest_kept(x, seen)
    # tracked_hints: the recursion on the call's own inputs from the device's own previous state
    want_v = T.call_vectors(l[:3], None, mp)
    assert np.array_equal(vs[0], want_v) and not vs[0][0].any()
    assert _same3(got[0], T.sequence(l[:3], own_ab[:3], own_mask[:3], want_v, None, tp["life"], tp["tol"], rule=T.frame_loops)), kind
    state = T.Prev(got[0][0][-1], got[0][1][-1], got[0][2][-1], l[2])
    want_v = T.call_vectors(l[3:], l[2], mp)
    assert np.array_equal(vs[1], want_v) and (vs[1][:, 1:-1, 1:-1] == np.array([1, 2], np.int8)).all(), "the pan does not show in the vectors"
    assert _same3(got[1], T.sequence(l[3:], own_ab[3:], own_mask[3:], want_v, state, tp["life"], tp["tol"], rule=T.frame_loops)), kind
    A, Mk, G = [np.concatenate([got[0][k], got[1][k]]) for k in range(3)]
    assert G[5].max() == 5 and (G[5] == 3).any() and not own_mask[3:].any()          # both hints crossed the boundary between the calls
    for f in range(1, 6):                                                            # ... and moved with the pan, by (-1, -2) a frame
        at = np.zeros((H, W), bool)                                                  # (frame 0's own hints: the rectangle, and a layer's blob)
        at[:H - f, :W - 2 * f] = own_mask[0][f:, 2 * f:] != 0
        assert at[RECT_A[0] - f:RECT_A[2] - f + 1, RECT_A[1] - 2 * f:RECT_A[3] - 2 * f + 1].all()
        inner = np.s_[:H - 8, :W - 8]               # (the last block row and column cannot report (1, 2): it would leave the plane)
        assert (G[f][at] == f).all() and np.array_equal(((G[f] == f) & (Mk[f] != 0))[inner], at[inner]), (kind, f)
    # out_ab: the same handle's network fed the tracked planes as own hints, then the filter (the second handle: the rule alone)
    if kind != "rgb_ref":                                # (idc_forward_async has no references to give the global branch: the next block)
        raw = np.concatenate([_network_on(x, l[:3], A[:3], Mk[:3]), _network_on(x, l[3:], A[3:], Mk[3:])])
        e2.set_temporal_filter(**FILTER)
        e2.set_temporal_motion(**mp)
        e2.temporal_reset()
        try:
            want_y = np.concatenate([e2.temporal_apply(raw[:3], l[:3])[0], e2.temporal_apply(raw[3:], l[3:])[0]])
        finally:
            e2.set_temporal_motion(None)
            e2.set_temporal_filter(None)
        assert _same(y, want_y), "%s %s: out_ab is not the network on the tracked planes (%d values differ)" % (kind, out, int((y != want_y).sum()))
        held = np.concatenate([_network_on(x, l[:3], own_ab[:3], own_mask[:3]), _network_on(x, l[3:], own_ab[3:], own_mask[3:])])
        assert _same(held[0], raw[0]) and not _same(held[1], raw[1])                 # the network does see the carried hints
    # ... and in the issue's own words: the SAME entry point of the same handle with tracking (and the filter) off, fed the tracked planes
    # as own hints -- with its references, where the route has them -- gives the raw map whose filtered form is this call's out_ab
    if kind in AB_KINDS:
        as_hints = _planes_as_hints(A, Mk)
        raw2 = np.concatenate([_call(x, kind, 0, "net", srcs[:3], as_hints[:3])[1], _call(x, kind, 0, "net", srcs[3:], as_hints[3:])[1]])
        e2.set_temporal_filter(**FILTER)
        e2.set_temporal_motion(**mp)
        e2.temporal_reset()
        try:
            want_y = np.concatenate([e2.temporal_apply(raw2[:3], l[:3])[0], e2.temporal_apply(raw2[3:], l[3:])[0]])
        finally:
            e2.set_temporal_motion(None)
            e2.set_temporal_filter(None)
        assert _same(y, want_y), "%s %s: out_ab is not the tracking-off call on the tracked planes (%d values differ)" % (kind, out, int((y != want_y).sum()))
        own_hints = _planes_as_hints(own_ab, own_mask)
        held2 = _call(x, kind, 0, "net", srcs[:3], own_hints[:3])[1]
        assert _same(held2[0], raw2[0]) and not _same(held2[1], raw2[1])             # the references route's network sees the carried hints too
    # the images: the blocking colour step of the same handle on that map
    for i, (g, w) in enumerate(zip(imgs, TG._blocking_images(x, l, y, 6, out))):
        assert np.array_equal(g, w), "%s %s image %d: %d bytes differ" % (kind, out, i, int((g != w).sum()))
    if "peaks" in ex:        # skip_hints reads the TRACKED mask: the restated peaks from this call's own entropy map, with either mask
        s = H // ex["entropy"].shape[1]
        with_tracked = DB.peaks(ex["entropy"], 256, 1, s, mask=Mk[3:])[0]
        with_own = DB.peaks(ex["entropy"], 256, 1, s, mask=own_mask[3:])[0]
        assert np.array_equal(ex["peaks"], with_tracked) and not np.array_equal(with_tracked, with_own)
        assert (ex["peaks"][:, -1] == -1).all() and (with_own[:, -1] != -1).all()    # hinted cells are no candidates; the own masks are empty
    if "cells" in ex:
        assert ex["cells"].tolist() == [0, 0, 0]                                    # unchanged: the layers' own count (frames 3..5 have none)
        assert np.array(first[2]["cells"]).tolist()[0] > 0


# ------------------------------------------------------------------------------------------------ 3. split invariance, device against device
def _run_parts(x, srcs, hints, parts, out, in_flight):
    """The frames as calls of `parts` images on alternating slots -> (A, M, G, vectors, out_ab, images)."""
    x.temporal_reset()
    held, at = [], 0
    trk, vs, abs_, imgs = [], [], [], []

    def collect(slot, res, ab, n):
        x.wait(slot)
        trk.append(x.tracked_hints(slot, n)); vs.append(x.temporal_vectors(slot, n)); abs_.append(np.array(ab)); imgs.extend(np.array(r) for r in res)

    for k, n in enumerate(parts):
        slot = k & 1
        ab = x.pinned_empty((n, 2, H, W), np.float32)
        res = x.forward_async_images(slot, srcs[at:at + n], hints[at:at + n], None, ab, out=out, l_cent=TG.L_CENT)
        held.append((slot, res, ab, n))
        at += n
        if not in_flight or len(held) == 2:
            for hld in held:
                collect(*hld)
            held = []
    for hld in held:
        collect(*hld)
    return [np.concatenate([t[k] for t in trk]) for k in range(3)] + [np.concatenate(vs), np.concatenate(abs_), imgs]


@pytest.mark.parametrize("out", ["net", "source"])
def test_a_sequence_gives_the_same_bits_however_it_is_split(e, out):
    srcs = _sources(7)
    hints = [[RECT_A], None, None, [RECT_B], None, None, None]
    e.set_temporal_filter(**FILTER)
    e.set_temporal_motion()
    e.set_hint_tracking()
    try:
        whole = _run_parts(e, srcs, hints, [7], out, False)
        assert whole[2][6].max() == 6 and (whole[2][6] == 3).any()                   # a chain over all seven frames
        for parts, in_flight in (([3, 4], True), ([1] * 7, False), ([2, 2, 3], True)):
            got = _run_parts(e, srcs, hints, parts, out, in_flight)
            assert _same3(got[:3], whole[:3]), parts
            assert np.array_equal(got[3], whole[3]) and _same(got[4], whole[4]), parts
            assert all(np.array_equal(a, b) for a, b in zip(got[5], whole[5])), parts
    finally:
        e.set_hint_tracking(None)
        e.set_temporal_motion(None)
        e.set_temporal_filter(None)


# ------------------------------------------------------------------------------------------------ 4. parameters, resets, drops, refusals
def _images_call(x, slot, srcs, hints):
    ab = x.pinned_empty((len(srcs), 2, H, W), np.float32)
    res = x.forward_async_images(slot, srcs, hints, None, ab, out="net", l_cent=TG.L_CENT)
    return res, ab


def test_parameters_in_flight_a_reset_a_drop_tracking_off_and_a_refused_call(e):
    srcs = _sources(6)
    hints = [[RECT_A], None, None, None, [RECT_B], None]
    mp = dict(M.DEFAULT)
    e.set_temporal_filter(**FILTER)
    e.set_temporal_motion(**mp)
    try:
        # the parent's bytes: tracking has never been on for this call
        e.temporal_reset()
        res, ab = _images_call(e, 0, srcs[:3], hints[:3])
        e.wait(0)
        parent = ([np.array(r) for r in res], np.array(ab), e.temporal_info(0, 3), e.temporal_vectors(0, 3))
        assert e.lib.idc_tracked_hints(e._h, 0, np.zeros(3 * 2 * H * W, np.float32).ctypes.data_as(VP), None, None) == -1
        e.set_hint_tracking()
        own_ab, own_mask = _own_planes(e, "images", srcs, hints)
        l, _ = TG._ingest_kept(e, srcs)
        # two batches in flight each keep the tracking parameters they were enqueued with
        p1, p2 = dict(life=1, tol=8.0), dict(life=0, tol=100.0)
        e.temporal_reset()
        e.set_hint_tracking(**p1)
        _images_call(e, 0, srcs[:3], hints[:3])
        e.set_hint_tracking(**p2)
        _images_call(e, 1, srcs[3:], hints[3:])
        e.wait(0), e.wait(1)
        a, b = e.tracked_hints(0, 3), e.tracked_hints(1, 3)
        va = T.call_vectors(l[:3], None, mp)
        assert _same3(a, T.sequence(l[:3], own_ab[:3], own_mask[:3], va, None, rule=T.frame_loops, **p1))
        assert (a[1][1] != 0).any() and not a[1][2].any()                           # life 1: gone at frame 2 ...
        vb = T.call_vectors(l[3:], l[2], mp)
        state = T.Prev(a[0][-1], a[1][-1], a[2][-1], l[2])
        assert _same3(b, T.sequence(l[3:], own_ab[3:], own_mask[3:], vb, state, rule=T.frame_loops, **p2)) and not b[1][0].any()     # ... and stays gone
        # a reset between two calls: the second starts a sequence, tracked = own and the vectors are zeros
        e.set_hint_tracking()
        e.temporal_reset()
        _images_call(e, 0, srcs[:3], hints[:3])
        e.temporal_reset()
        _images_call(e, 1, srcs[3:], hints[3:])
        e.wait(0), e.wait(1)
        b = e.tracked_hints(1, 3)
        assert _same(b[0][0], own_ab[3]) and not b[1][0].any() and not e.temporal_vectors(1, 3)[0].any()
        assert _same3(b, T.sequence(l[3:], own_ab[3:], own_mask[3:], T.call_vectors(l[3:], None, mp), None, 0, 8.0, rule=T.frame_loops))
        # a motion-off call drops the state: the next tracking call's frame 0 has a predecessor and vectors, and carries nothing
        e.temporal_reset()
        _images_call(e, 0, srcs[:2], hints[:2])
        e.wait(0)
        assert (e.tracked_hints(0, 2)[1][1] != 0).any()
        e.set_temporal_motion(None)
        _images_call(e, 0, srcs[2:3], hints[2:3])
        e.wait(0)
        assert e.lib.idc_tracked_hints(e._h, 0, None, np.zeros(H * W, np.float32).ctypes.data_as(VP), None) == -1
        e.set_temporal_motion(**mp)
        _images_call(e, 1, srcs[3:], hints[3:])
        e.wait(1)
        b = e.tracked_hints(1, 3)
        assert np.array_equal(e.temporal_vectors(1, 3), vb) and vb[0].any() and not b[1][0].any() and (b[2][2] == 1).any() and b[2].max() == 1
        assert _same3(b, T.sequence(l[3:], own_ab[3:], own_mask[3:], vb, T._NoTrack(l[2]), 0, 8.0, rule=T.frame_loops))
        # idc_temporal_apply moves l_prev on without hints, so it drops the tracked planes as well
        e.temporal_reset()
        _images_call(e, 0, srcs[:2], hints[:2])
        e.wait(0)
        e.temporal_apply(np.zeros((1, 2, H, W), np.float32), l[2:3])
        _images_call(e, 1, srcs[3:], hints[3:])
        e.wait(1)
        b = e.tracked_hints(1, 3)
        assert np.array_equal(e.temporal_vectors(1, 3), vb) and not b[1][0].any()
        assert _same3(b, T.sequence(l[3:], own_ab[3:], own_mask[3:], vb, T._NoTrack(l[2]), 0, 8.0, rule=T.frame_loops))
        # a refused setting changes nothing; a refused call (a slot in flight) leaves the slot usable and the state as it was
        assert e.lib.idc_set_hint_tracking(e._h, 1, 65536, 8.0) == -1 and e.lib.idc_set_hint_tracking(e._h, 1, 0, float("nan")) == -1
        e.temporal_reset()
        _images_call(e, 0, srcs[:3], hints[:3])
        with pytest.raises(N.IdcError):
            _images_call(e, 0, srcs[3:], hints[3:])
        e.wait(0)
        a = e.tracked_hints(0, 3)
        assert _same3(a, T.sequence(l[:3], own_ab[:3], own_mask[:3], va, None, 0, 8.0, rule=T.frame_loops))
        _images_call(e, 0, srcs[3:], hints[3:])
        e.wait(0)
        state = T.Prev(a[0][-1], a[1][-1], a[2][-1], l[2])
        assert _same3(e.tracked_hints(0, 3), T.sequence(l[3:], own_ab[3:], own_mask[3:], vb, state, 0, 8.0, rule=T.frame_loops))
        # tracking off after tracking on: every byte is the parent's again, and the slot has no tracked planes to report
        e.set_hint_tracking(None)
        e.temporal_reset()
        res, ab = _images_call(e, 0, srcs[:3], hints[:3])
        e.wait(0)
        assert _same(np.array(ab), parent[1]) and all(np.array_equal(r, q) for r, q in zip(res, parent[0]))
        info = e.temporal_info(0, 3)
        assert info[0].tolist() == parent[2][0].tolist() and info[1].tolist() == parent[2][1].tolist() and np.array_equal(e.temporal_vectors(0, 3), parent[3])
        assert e.lib.idc_tracked_hints(e._h, 0, None, np.zeros(3 * H * W, np.float32).ctypes.data_as(VP), None) == -1
        # with the filter off tracking does nothing, and leaves the state alone
        e.set_hint_tracking()
        e.temporal_reset()
        _images_call(e, 0, srcs[:3], hints[:3])
        e.wait(0)
        a = e.tracked_hints(0, 3)
        e.set_temporal_filter(None)
        res, ab = _images_call(e, 1, srcs[:3], hints[:3])
        e.wait(1)
        assert e.lib.idc_tracked_hints(e._h, 1, None, np.zeros(3 * H * W, np.float32).ctypes.data_as(VP), None) == -1
        e.set_temporal_filter(**FILTER)
        _images_call(e, 1, srcs[3:], hints[3:])
        e.wait(1)
        state = T.Prev(a[0][-1], a[1][-1], a[2][-1], l[2])
        assert _same3(e.tracked_hints(1, 3), T.sequence(l[3:], own_ab[3:], own_mask[3:], vb, state, 0, 8.0, rule=T.frame_loops))
    finally:
        e.set_hint_tracking(None)
        e.set_temporal_motion(None)
        e.set_temporal_filter(None)


def test_every_status_of_the_table():
    x = engine.HipColorizer(H, W, max_batch=4, precision="bf16")
    try:
        lib, h = x.lib, x._h
        nan = float("nan")
        x.set_hint_tracking(life=2, tol=3.0)
        for bad in [(2, 0, 8.0), (-1, 0, 8.0), (1, -1, 8.0), (1, 65536, 8.0), (1, 0, -0.1), (1, 0, 100.5), (1, 0, nan), (1, 0, float("inf"))]:
            assert lib.idc_set_hint_tracking(h, *bad) == -1, bad
        assert lib.idc_set_hint_tracking(None, 1, 0, 8.0) == -1
        # a refused call changed nothing: life is still 2
        c = [k for k in T.cases(H, W) if k["name"].startswith("life 0")][0]
        x.set_temporal_motion(**c["mp"])
        got = x.track_hints_apply(c["l"][:4], c["ab"][:4], c["mask"][:4])
        assert (got[1][2] != 0).any() and not got[1][3].any() and got[2].max() == 2
        for good in [(1, 0, 0.0), (0, 65535, 100.0), (1, 1, 8.0), (1, 0, 8.0)]:
            assert lib.idc_set_hint_tracking(h, *good) == 0, good
        f = np.zeros((5, 2, H, W), np.float32)
        p = f.ctypes.data_as(VP)
        g = np.zeros((5, H, W), np.int32).ctypes.data_as(VP)
        assert lib.idc_track_hints_apply(h, 0, p, p, p, p, p, g, None) == -6 and lib.idc_track_hints_apply(h, 5, p, p, p, p, p, g, None) == -6
        for k in range(6):
            args = [p, p, p, p, p, g]
            args[k] = None
            assert lib.idc_track_hints_apply(h, 1, *(args + [None])) == -1, k
        assert lib.idc_track_hints_apply(h, 1, p, p, p, p, p, g, None) == 0              # the vectors are optional
        assert lib.idc_track_hints_apply(None, 1, p, p, p, p, p, g, None) == -1
        # idc_tracked_hints: the slot range, all pointers NULL, [in flight: the pipelined cases], a slot that never ran
        assert lib.idc_tracked_hints(h, -1, p, p, g) == -1 and lib.idc_tracked_hints(h, 2, p, p, g) == -1
        assert lib.idc_tracked_hints(h, 0, None, None, None) == -1
        assert lib.idc_tracked_hints(h, 0, p, p, g) == -1 and lib.idc_tracked_hints(None, 0, p, p, g) == -1
    finally:
        x.close()


# ------------------------------------------------------------------------------------------------ 5. the claim
def test_a_hint_made_once_stays_on_the_moving_object():
    """The issue's sequence (track_ref.claim_inputs): a 32 x 32 textured object moving (1, 2) pixels a frame, hinted at frame 0 only, 12 frames.
    With tracking every interior pixel of the hint is still hinted at frame 11, 11 * (1, 2) away and on the object; held at its net
    coordinates, as colorize_video does without tracking, the rectangle is wholly on the background by then."""
    c = T.CLAIM
    l, ab, mask, pos = T.claim_inputs()
    x = engine.HipColorizer(c["H"], c["W"], max_batch=c["n"], precision="bf16")
    try:
        x.set_temporal_motion()
        x.set_hint_tracking()
        A, Mk, G, v = x.track_hints_apply(l, ab, mask, vectors=True)
        assert _same3((A, Mk, G), T.sequence(l, ab, mask, T.call_vectors(l, None, M.DEFAULT), None, 0, 8.0, rule=T.frame_loops))
        inner, of, held_on_object = T.claim_counts(Mk, pos)
        print("frame 11: %d of %d interior pixels of the hint still hinted on the object; %d pixels of the held rectangle on the object" %
              (inner, of, held_on_object))
        assert inner == of == 36 and held_on_object == 0
        y0, x0, y1, x1 = c["rect"][:4]
        on = Mk[11] != 0
        oy, ox = pos[11]
        assert on[oy:oy + c["size"], ox:ox + c["size"]].sum() == on.sum() > 0        # nothing of it is on the background
        assert (G[11][on] == 11).all() and (A[11][0][on] == np.float32(c["rect"][4])).all()
    finally:
        x.close()
