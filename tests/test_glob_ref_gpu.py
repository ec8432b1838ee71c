"""GPU checks of the reference-image global hints: idc_global_stats_rgb, idc_set_global_refs and idc_forward_async_rgb_ref through
HipColorizer (global_stats_rgb / set_global_refs / forward_async_rgb(refs=...) / colorize_stream) and ColorizeImageCaffeGlobDist.

References are never the code under test: tests/glob_ref.py (host resize, the oracle's rgb2lab, float64 pooling and nearest centre; its
inputs satisfy the knife-edge margin that tests/test_glob_ref_cpu.py asserts, so COUNTS are compared exactly and no block is left out), the
existing idc_global_histogram route, and the blocking route on the same handle.

Shapes: a 32 x 48 handle (H != W: an h/4 - w/4 swap shows; 96 blocks = 6 workgroups a reference) with m = 7 references from 1 x 1 to
131 x 200; 64 x 64 Global-Hints handles, max_batch 3, for what needs the network."""
import ctypes

import numpy as np
import pytest

import glob_ref as G
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import api, engine, workloads
from oracle import weights

pytestmark = pytest.mark.gpu

H32, W32 = G.NET
HINTS = [None, [(4, 6, 20, 30, 30.0, -40.0), (10, 12, 30, 40, -25.0, 55.0)], [(-5, -9, 3, 8, 20.0, 20.0), (30, 50, 90, 200, -30.0, 35.0)]]
_SD = {}


def _glob_sd(seed):
    """The weights of test_caffe_branches_gpu._glob_sd."""
    if seed not in _SD:
        _SD[seed] = weights.add_global_branch(weights.make_state_dict(seed, "he", include_class=False), seed)
    return _SD[seed]


@pytest.fixture(scope="module")
def e32():
    e = engine.HipColorizer(H32, W32, max_batch=3, precision="bf16")          # statistics need no weights and no Global-Hints branch
    yield e
    e.close()


@pytest.fixture(scope="module")
def eg():
    made = {}

    def get(precision="bf16"):
        if precision not in made:
            e = engine.HipColorizer(64, 64, max_batch=3, precision=precision, global_hints=True)
            e.load_state_dict(_glob_sd(3))
            made[precision] = e
        return made[precision]
    yield get
    for e in made.values():
        e.close()


def _ulps32(got, want64):
    """Distance of fp32 ``got`` from the float64 value, in ulps of the fp32 number nearest to it."""
    return abs(float(got) - want64) / float(np.spacing(np.float32(want64)))


def _counts(hist, nblk):
    return np.rint(np.asarray(hist, np.float64) * nblk).astype(np.int64)


# ------------------------------------------------------------------------------------------------ 1. against tests/glob_ref.py
def test_stats_equal_the_reference_and_do_not_depend_on_the_neighbours(e32):
    refs, c = G.refs_net(), G.centres()
    m, nblk = len(refs), (H32 // 4) * (W32 // 4)
    assert m == 7
    hist, sat = e32.global_stats_rgb(refs, c)
    assert hist.shape == (m, 313) and hist.dtype == np.float32 and sat.shape == (m,) and sat.dtype == np.float32
    for k in range(m):
        want = G.stats_of("net", k, H32, W32)
        got = _counts(hist[k], nblk)
        print("reference %s: %d bins, margin %.3g, s_avg %.8f against %.8f (%.2f ulp)"
              % (G.SIZES[k], want["bins"], want["margin"], sat[k], want["s_avg"], _ulps32(sat[k], want["s_avg"])))
        np.testing.assert_array_equal(got, want["counts"], err_msg="counts of reference %s" % (G.SIZES[k],))
        np.testing.assert_array_equal(hist[k], want["hist"])
        assert got.sum() == nblk and abs(float(hist[k].astype(np.float64).sum()) - 1.0) <= 1e-6
        assert _ulps32(sat[k], want["s_avg"]) <= 2.0
    # the same references in reverse order, and each alone: the very bits
    rhist, rsat = e32.global_stats_rgb(refs[::-1], c)
    np.testing.assert_array_equal(rhist[::-1], hist)
    np.testing.assert_array_equal(rsat[::-1].view(np.uint32), sat.view(np.uint32))
    for k in range(m):
        h1, s1 = e32.global_stats_rgb([refs[k]], c)
        np.testing.assert_array_equal(h1[0], hist[k])
        assert s1.view(np.uint32)[0] == sat.view(np.uint32)[k], "s_avg of reference %d alone" % k
    # twice in a row
    hist2, sat2 = e32.global_stats_rgb(refs, c)
    np.testing.assert_array_equal(hist2, hist)
    np.testing.assert_array_equal(sat2.view(np.uint32), sat.view(np.uint32))
    h3, none = e32.global_stats_rgb(refs[:2], c, want_sat=False)               # s_avg is optional
    assert none is None
    np.testing.assert_array_equal(h3, hist[:2])


# ------------------------------------------------------------------------------------------------ 2. against the existing route
def test_stats_equal_idc_global_histogram(e32):
    """hist bit for bit.  s_avg to one fp32 ulp: the existing kernel adds its per-block float64 saturation sums with atomics, in whatever
    order they arrive, the new one in a fixed order, so the float64 sums may differ in their last bits before the one rounding to fp32."""
    refs, c = G.refs_net(), G.centres()
    hist, sat = e32.global_stats_rgb(refs, c)
    for k in (0, 1, 3, 4, 6):                                       # the net size itself, then resized ones: up, down, one pixel
        src = refs[k]
        if src.shape[:2] == (H32, W32):
            net = src
        else:
            net = e32.set_image_rgb(src, want_lab=False)[0][0]      # the net-size image the existing route would be handed
        old_h, old_s = e32.global_histogram(net, c)
        np.testing.assert_array_equal(hist[k], old_h[0], err_msg="reference %s" % (G.SIZES[k],))
        ulp = float(np.spacing(old_s[0]))
        print("reference %s: s_avg %.9g, existing route %.9g" % (G.SIZES[k], sat[k], old_s[0]))
        assert abs(float(sat[k]) - float(old_s[0])) <= ulp


# ------------------------------------------------------------------------------------------------ 3. install equals the host route
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_install_equals_set_global_hints(eg, precision):
    e = eg(precision)
    refs, c = G.refs64()[:2], G.centres()
    hist, sat = e.global_stats_rgb(refs, c)
    for k in range(2):                                              # the 64 x 64 statistics are right as well (256 blocks, 16 workgroups)
        np.testing.assert_array_equal(_counts(hist[k], 256), G.stats_of("64", k, 64, 64)["counts"])
    L, ab, mask = workloads.random_batch(3, 64, seed=21, max_points=4, max_p=3)
    idx = [1, -1, 0]
    e.set_global_refs(refs, c, ref_index=idx)
    got = e.forward(L, ab, mask).copy()
    c43 = e.activation("conv4_3", 3).copy()
    e.set_global_hints(G.glob_rows(hist, idx))
    want = e.forward(L, ab, mask).copy()
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    np.testing.assert_array_equal(got, want)
    # the hint arrives: conv4_3 differs from the no-reference forward where an image has a reference, and only there
    e.clear_global_hints()
    e.forward(L, ab, mask)
    c43_none = e.activation("conv4_3", 3)
    assert np.abs(c43[0] - c43_none[0]).max() > 0 and np.abs(c43[2] - c43_none[2]).max() > 0
    np.testing.assert_array_equal(c43[1], c43_none[1])
    # a second install at img = 2, n = 1 leaves rows 0 and 1 as the first install wrote them
    e.set_global_refs(refs, c, ref_index=idx)
    e.set_global_refs([refs[1]], c, img=2)
    got = e.forward(L, ab, mask).copy()
    e.set_global_hints(G.glob_rows(hist, [1, -1, 1]))
    np.testing.assert_array_equal(got, e.forward(L, ab, mask))
    assert np.abs(got[2] - want[2]).max() > 0                      # ... and row 2 did change
    # saturation: s_avg_mask = [s_avg, 1]; another flag value travels too
    e.set_global_refs(refs, c, ref_index=idx, saturation=True, hist_flag=0.5)
    got = e.forward(L, ab, mask).copy()
    g, s = G.glob_rows(hist, idx, flag=0.5, s_avg=sat)
    e.set_global_hints(g, s)
    np.testing.assert_array_equal(got, e.forward(L, ab, mask))
    e.set_global_hints(g)                                           # without the saturation input the output is another
    assert np.abs(got[0] - e.forward(L, ab, mask)[0]).max() > 0
    e.clear_global_hints()


# ------------------------------------------------------------------------------------------------ 4. pipelined
def _batch(n, sh, sw, seed):
    return np.ascontiguousarray(np.stack([G.noise(sh, sw, seed + j) if j % 2 else G.ramp(sh, sw, seed + j) for j in range(n)]))


def _blocking(e, batch, hints, refs, idx, c, saturation=False):
    """set_image_rgb + set_hints + set_global_refs + forward -> (out_ab, rgb net-size, rgb source-size), copies.  Leaves the handle's global
    hints cleared."""
    n = batch.shape[0]
    e.set_image_rgb(batch, keep_source=True, want_rgb=False, want_lab=False)
    for i in range(n):
        e.set_hints((hints[i] if hints is not None else None) or [], mode="ab", img=i, mask_value=1.0)
    if refs:
        e.set_global_refs(refs, c, ref_index=idx, saturation=saturation)
    else:
        e.clear_global_hints()
    ab, rgb, _ = e.forward_resident(n)
    full = np.stack([e.fullres_rgb("output_ab", "linear", "image", img=i) for i in range(n)])
    e.clear_global_hints()
    return ab.copy(), rgb.copy(), full


def test_both_slots_carry_their_own_references(eg):
    e = eg("bf16")
    c, r = G.centres(), G.refs64()
    jobs = [  # batch, hints, refs, ref_index, saturation
        (_batch(3, 37, 41, 50), HINTS, [r[0], r[1]], [1, -1, 0], False),
        (_batch(2, 64, 64, 60), None, [r[2]], [0, 0], True),
        (_batch(3, 5, 7, 70), [HINTS[1], None, HINTS[2]], [r[3], r[0], r[1]], None, True),       # NULL index: the identity
        (_batch(2, 37, 41, 80), None, [], None, False),                                             # m = 0: nobody has a reference
    ]
    wants = [_blocking(e, b, h, rf, ix, c, s) for b, h, rf, ix, s in jobs]
    assert np.abs(wants[0][0][0] - _blocking(e, jobs[0][0], jobs[0][1], [], None, c)[0][0]).max() > 0      # the references matter
    # the handle's own global hints, set the old way, and what a blocking forward makes of them
    own = workloads.global_hint_config5(3, seed=5)[0]
    e.set_global_hints(own)
    L, ab, mask = workloads.random_batch(3, 64, seed=22, max_points=4, max_p=3)
    before = e.forward(L, ab, mask).copy()
    for out in ("net", "source"):
        for first in (0, 2):                                        # jobs (0, 1), then (2, 3): slot 1 enqueued before slot 0 is waited for
            res = []
            for slot in (0, 1):
                b, h, rf, ix, s = jobs[first + slot]
                dst = np.full(b.shape if out == "source" else (b.shape[0], 64, 64, 3), 7, np.uint8)
                dab = np.empty((b.shape[0], 2, 64, 64), np.float32)
                e.forward_async_rgb(slot, b, h, dst, out_ab=dab, out=out, refs=rf, ref_index=ix, centres=c, saturation=s)
                res.append((dst, dab))
            for slot in (0, 1):
                e.wait(slot)
                t = e.pipeline_times(slot)
                assert np.all(np.diff(t) >= -1e-3), t               # h2d start <= h2d end <= compute start <= ... <= d2h end
                want = wants[first + slot]
                what = "job %d, out=%s" % (first + slot, out)
                np.testing.assert_array_equal(res[slot][1], want[0], err_msg="out_ab: " + what)
                np.testing.assert_array_equal(res[slot][0], want[2] if out == "source" else want[1], err_msg="rgb_out: " + what)
    # the handle's own global inputs were neither read (above) nor written
    np.testing.assert_array_equal(e.forward(L, ab, mask), before)
    e.clear_global_hints()


def test_refs_none_still_reads_the_handles_global_hints(eg):
    e = eg("bf16")
    batch = _batch(3, 37, 41, 90)
    own = workloads.global_hint_config5(3, seed=6)[0]

    def blocking():
        e.set_image_rgb(batch, keep_source=True, want_rgb=False, want_lab=False)
        for i in range(3):
            e.set_hints(HINTS[i] or [], mode="ab", img=i, mask_value=1.0)
        return e.forward_resident(3)[1].copy()

    none = blocking()
    e.set_global_hints(own)
    want = blocking()
    assert np.abs(want.astype(int) - none.astype(int)).max() > 0
    dst = np.zeros((3, 64, 64, 3), np.uint8)
    e.forward_async_rgb(0, batch, HINTS, dst)
    e.wait(0)
    np.testing.assert_array_equal(dst, want)
    # a batch with references on the other slot in between changes nothing of that
    dst2 = np.zeros((3, 64, 64, 3), np.uint8)
    e.forward_async_rgb(1, batch, HINTS, dst2, refs=[G.refs64()[0]], ref_index=[0, 0, 0], centres=G.centres())
    dst3 = np.zeros((3, 64, 64, 3), np.uint8)
    e.forward_async_rgb(0, batch, HINTS, dst3, refs=None)
    e.wait(1); e.wait(0)
    np.testing.assert_array_equal(dst3, want)
    assert np.abs(dst2.astype(int) - want.astype(int)).max() > 0
    e.clear_global_hints()


@pytest.mark.parametrize("out", ["net", "source"])
def test_colorize_stream_with_references(eg, out):
    e = eg("bf16")
    c, r = G.centres(), G.refs64()
    items, wants = [], []
    for k in range(3):
        n = 3 if k % 2 else 2
        b = _batch(n, 37, 41, 100 + 10 * k)
        h = [HINTS[(i + k) % 3] for i in range(n)]
        items.append((b, h, [r[k]] * n))                             # one object for every image of the item
        per_image = [_blocking(e, b[i:i + 1], h[i:i + 1], [r[k]], [0], c) for i in range(n)]
        wants.append(np.concatenate([w[2] if out == "source" else w[1] for w in per_image]))
    got = list(e.colorize_stream(iter(items), out=out, centres=c))
    assert len(got) == 3
    for k in range(3):
        np.testing.assert_array_equal(got[k], wants[k], err_msg="item %d" % k)


# ------------------------------------------------------------------------------------------------ 5. the wrapper
def test_wrapper_takes_a_reference_photograph_as_it_comes():
    sd = dict(_glob_sd(0))
    sd["model1.0.weight"] = (sd["model1.0.weight"][:, :1] / np.float32(100.0)).astype(np.float32)      # as test_glob_dist_api_class
    model = api.ColorizeImageCaffeGlobDist(Xd=64, precision="fp32")
    model.prep_net(0, state_dict=sd)
    model.set_image(G.ramp(64, 64, 3))
    ref = G.refs64()[0]
    assert ref.shape == (97, 61, 3)
    hist = model.get_global_histogram(ref)
    np.testing.assert_array_equal(hist, G.stats_of("64", 0, 64, 64)["hist"])
    own = G.refs64()[1]                                              # an Xd x Xd reference keeps the existing call: the same numbers
    np.testing.assert_array_equal(model.get_global_histogram(own), G.stats_of("64", 1, 64, 64)["hist"])
    zero_ab, zero_m = np.zeros((2, 64, 64)), np.zeros((1, 64, 64))
    want = model.net_forward(zero_ab, zero_m, hist).copy()
    none = model.net_forward(zero_ab, zero_m).copy()
    got = model.net_forward_reference(zero_ab, zero_m, ref)
    assert got.shape == (64, 64, 3) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, want)
    assert np.abs(want.astype(int) - none.astype(int)).max() > 0
    # the edit-list form, and glob_dist keeps working after a reference was installed
    hints = [(10, 12, 30, 40, 200, 30, 60)]
    want_h = model.net_forward_hints(hints, mode='rgb', glob_dist=hist).copy()
    np.testing.assert_array_equal(model.net_forward_hints(hints, mode='rgb', ref_rgb=ref), want_h)
    np.testing.assert_array_equal(model.net_forward(zero_ab, zero_m), none)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_statuses_and_refused_calls_change_nothing(eg, make_sd):
    vp, fp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)
    e = eg("bf16")
    lib, h = e.lib, e._h
    c = G.centres()
    r = G.refs64()
    INVALID, BATCH, UNSUPPORTED = -1, -6, -7
    px = np.zeros(64, np.uint8)

    def table(*entries):                                            # (array or None, h, w) -> idc_ref_image[]
        arr = (N.RefImage * max(len(entries), 1))()
        for k, (a, hh, ww) in enumerate(entries):
            arr[k].rgb, arr[k].h, arr[k].w = (a.ctypes.data if a is not None else None), hh, ww
        return arr

    good = table((r[0], 97, 61), (r[1], 64, 64))
    I = lambda *v: np.array(v, np.int32)
    P = lambda a: a.ctypes.data_as(vp) if a is not None else None
    CP = c.ctypes.data_as(fp)
    hist = np.zeros((2, 313), np.float32)

    own = workloads.global_hint_config5(3, seed=7)[0]
    e.set_global_hints(own)
    L, ab, mask = workloads.random_batch(3, 64, seed=23, max_points=4, max_p=3)
    before = e.forward(L, ab, mask).copy()

    def install(img=0, n=3, m=2, refs=good, idx=I(1, -1, 0), centres=CP, flag=1.0, flags=0, handle=h):
        return lib.idc_set_global_refs(handle, img, n, m, refs, P(idx), centres, flag, flags)

    def stats(m=2, refs=good, centres=CP, out=hist.ctypes.data_as(fp), handle=h):
        return lib.idc_global_stats_rgb(handle, m, refs, centres, out, None)

    batch = _batch(3, 5, 7, 110)
    dst = np.empty((3, 64, 64, 3), np.uint8)

    def piped(slot=0, n=3, m=2, refs=good, idx=I(1, -1, 0), centres=CP, flag=1.0, rflags=0, handle=h, sh=5, flags=0):
        return lib.idc_forward_async_rgb_ref(handle, slot, n, sh, 7, P(batch), None, None, 0, 1.0, 0.0, 50.0, flags, m, refs, P(idx), centres,
                                             flag, rflags, P(dst), None)

    huge = table((px, 16384, 16384), (px, 16384, 16384))             # 2 x 768 MiB: refused before a byte is read
    for name, call in (("install", install), ("piped", piped)):
        assert call(m=0 if name == "install" else -1) == INVALID, name
        assert call(m=N.IDC_REF_MAX + 1) == INVALID, name
        assert call(refs=None) == INVALID, name
        assert call(refs=table((r[0], 97, 61), (None, 64, 64))) == INVALID, name
        for hh, ww in ((0, 61), (97, 0), (16385, 61), (97, 16385), (-1, 61)):
            assert call(refs=table((r[0], hh, ww), (r[1], 64, 64))) == INVALID, (name, hh, ww)
        assert call(refs=huge) == INVALID, name
        assert call(idx=I(2, -1, 0)) == INVALID and call(idx=I(1, -2, 0)) == INVALID, name
        assert call(idx=None) == INVALID, name                      # NULL index with m = 2, n = 3
        assert call(centres=None) == INVALID, name
        assert call(**{"flags" if name == "install" else "rflags": 2}) == INVALID, name
        assert call(flag=float("nan")) == INVALID and call(flag=float("inf")) == INVALID, name
    assert install(img=1) == BATCH and install(img=3, n=1, idx=I(0)) == BATCH and install(n=0) == BATCH and install(img=-1) == BATCH
    assert piped(n=0) == BATCH and piped(n=4, idx=I(0, 0, 0, 0)) == BATCH
    assert piped(slot=2) == INVALID and piped(sh=0) == INVALID and piped(flags=2) == INVALID      # the shared arguments keep their codes
    assert stats(m=0) == INVALID and stats(m=N.IDC_REF_MAX + 1) == INVALID and stats(refs=None) == INVALID and stats(centres=None) == INVALID
    assert stats(out=None) == INVALID and stats(refs=table((None, 4, 4), (r[1], 64, 64))) == INVALID and stats(refs=huge) == INVALID
    assert stats(refs=table((r[0], 0, 61), (r[1], 64, 64))) == INVALID
    plain = engine.HipColorizer(64, 64, max_batch=3, precision="bf16")
    plain.load_state_dict(make_sd(0, "he"))
    assert install(handle=plain._h) == UNSUPPORTED and piped(handle=plain._h) == UNSUPPORTED
    assert stats(handle=plain._h) == 0                               # the statistics need no Global-Hints branch
    plain.close()
    # nothing was enqueued or written: both slots are idle, the handle's hints are the ones set before, and everything still works
    assert lib.idc_wait(h, 0) == 0 and lib.idc_wait(h, 1) == 0
    np.testing.assert_array_equal(e.forward(L, ab, mask), before)
    assert stats() == 0
    np.testing.assert_array_equal(_counts(hist[0], 256), G.stats_of("64", 0, 64, 64)["counts"])
    want = _blocking(e, batch, None, [r[0], r[1]], [1, -1, 0], c)[1]
    e.set_global_hints(own)
    for slot in (0, 1):                                              # a slot refused above accepts a valid batch next
        dst[...] = 0
        assert piped(slot=slot) == 0
        assert piped(slot=slot) == INVALID                           # still in flight
        e.wait(slot)
        np.testing.assert_array_equal(dst, want)
    assert piped(m=0, refs=None, idx=None, centres=None) == 0        # m = 0: nothing but the images is needed
    e.wait(0)
    np.testing.assert_array_equal(dst, _blocking(e, batch, None, [], None, c)[1])
    e.set_global_hints(own)
    np.testing.assert_array_equal(e.forward(L, ab, mask), before)
    assert install() == 0                                            # ... and a valid install goes through
    e.clear_global_hints()
