"""GPU checks of the pipelined batches of images of individual sizes: idc_forward_async_images (one pointer and one size per image in, one
colourised image per image out, at the net size or at each image's own) through HipColorizer.forward_async_images / colorize_images.

The reference is never the new call.  It is
  (a) the existing forward_async_rgb with n = 1 per image on the same handle,
  (b) the blocking route of test_batch_rgb_gpu.py (_blocking) per image,
  (c) tests/ingest_ref.py with the oracle's colour conversions.
(a) and (b) are bit for bit (out_ab, net-size and source-size rgb_out): the new kernels run the device functions of the existing ones on
the same operands, and a handle's kernel choice follows max_batch, not the call's n (test_net_gpu.py::test_batching_is_exactly_per_image).
(c) has the bar of test_batch_matches_the_oracle_colour_conversions, on that test's inputs: at most one uint8 level on at most 2e-4 of the
values; on the 105-value (5,7) output that admits no differing value.
Shapes: 64 x 64 and 40 x 72 handles, bf16 (one case fp32), max_batch 8; the size lists are tests/ragged_ref.py's, whose structure
(start residues mod 4, groups that span images, the byte tail) tests/test_ragged_batch_cpu.py shows."""
import ctypes

import numpy as np
import pytest

import glob_ref as G
import ingest_ref
import ragged_ref as R
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import engine, workloads
from oracle import colorspace as ocs
from test_batch_rgb_gpu import FRAC, HINTS_AB, HINTS_RGB, _batch, _blocking, _check_u8, _hint_lists
from test_glob_ref_gpu import _glob_sd

pytestmark = pytest.mark.gpu

_ENG = {}
_REF_A = {}


@pytest.fixture(scope="module")
def eng(make_sd):
    def get(H, W, precision="bf16"):
        key = (H, W, precision)
        if key not in _ENG:
            e = engine.HipColorizer(H, W, max_batch=8, precision=precision)
            e.load_state_dict(make_sd(0, "he"))
            e.key = key
            _ENG[key] = e
        return _ENG[key]
    yield get
    for e in _ENG.values():
        e.close()
    _ENG.clear()
    _REF_A.clear()


def _ref_a(e, img, hints, mode, mask_value):
    """Reference (a): forward_async_rgb with n = 1 on this image -> (out_ab [2,H,W], net-size rgb, source-size rgb).  Computed once per
    (handle, image, hint list, mode, mask_value) and not written to afterwards."""
    key = (e.key, img.shape, img.tobytes(), repr(hints), mode, mask_value)
    if key not in _REF_A:
        one = np.ascontiguousarray(img[None])
        net, full = np.empty((1, e.H, e.W, 3), np.uint8), np.empty(one.shape, np.uint8)
        ab, ab2 = np.empty((1, 2, e.H, e.W), np.float32), np.empty((1, 2, e.H, e.W), np.float32)
        hl = None if hints is None else [hints]
        e.forward_async_rgb(0, one, hl, net, out_ab=ab, mode=mode, mask_value=mask_value, out="net")
        e.forward_async_rgb(1, one, hl, full, out_ab=ab2, mode=mode, mask_value=mask_value, out="source")
        e.wait(0); e.wait(1)
        np.testing.assert_array_equal(ab, ab2)
        assert np.isfinite(ab).all()
        for a in (ab, net, full):
            a.setflags(write=False)
        _REF_A[key] = (ab[0], net[0], full[0])
    return _REF_A[key]


def _images(e, lst, seed):
    return [R.image(sh, sw, seed + j) for j, (sh, sw) in enumerate(R.sizes(lst, e.H, e.W))]


def _run(e, images, hints, mode, mask_value, out, slot=0, pinned=False):
    """The call under test -> (list of rgb outputs, out_ab); ``pinned``: False, True, or a per-image list."""
    n = len(images)
    pins = [pinned] * n if isinstance(pinned, bool) else list(pinned)
    new = lambda shape, p, dtype=np.uint8: e.pinned_empty(shape, dtype) if p else np.empty(shape, dtype)
    srcs = []
    for a, p in zip(images, pins):
        s = new(a.shape, p)
        s[...] = a
        srcs.append(s)
    outs = [new(a.shape if out == "source" else (e.H, e.W, 3), not p if not isinstance(pinned, bool) else p) for a, p in zip(images, pins)]
    for o in outs:
        o[...] = 7
    ab = new((n, 2, e.H, e.W), pins[0], np.float32)
    got = e.forward_async_images(slot, srcs, hints, outs, out_ab=ab, mode=mode, mask_value=mask_value, out=out)
    e.wait(slot)
    assert all(g is o for g, o in zip(got, outs))
    return outs, ab


def _check_against_a(e, images, hints, mode, mask_value, net=None, full=None, abs_=(), what=""):
    for i, img in enumerate(images):
        want_ab, want_net, want_full = _ref_a(e, img, None if hints is None else hints[i], mode, mask_value)
        w = "%s image %d (%dx%d)" % (what, i, img.shape[0], img.shape[1])
        for ab in abs_:
            np.testing.assert_array_equal(ab[i], want_ab, err_msg="out_ab: " + w)
        if net is not None:
            np.testing.assert_array_equal(net[i], want_net, err_msg="net-size rgb_out: " + w)
        if full is not None:
            np.testing.assert_array_equal(full[i], want_full, err_msg="source-size rgb_out: " + w)


# ------------------------------------------------------------------------------------------------ 1. the mixed batch
@pytest.mark.parametrize("mask_value", [1.0, 110.0])
@pytest.mark.parametrize("mode", ["ab", "rgb"])
@pytest.mark.parametrize("H,W,precision", [(64, 64, "bf16"), (40, 72, "bf16")])
def test_mixed_batch_equals_the_same_size_call_per_image(eng, H, W, precision, mode, mask_value):
    e = eng(H, W, precision)
    images = _images(e, R.MIXED, 400)
    table = HINTS_AB if mode == "ab" else HINTS_RGB
    hints = [table[i % 4] for i in range(len(images))]
    assert np.abs(_ref_a(e, images[2], hints[2], mode, mask_value)[0]).max() > 0
    for order in (1, -1):                                        # reversed: the image starts fall on other residues mod 4
        imgs, hl = images[::order], hints[::order]
        net, ab = _run(e, imgs, hl, mode, mask_value, "net", slot=0, pinned=order < 0)
        full, ab2 = _run(e, imgs, hl, mode, mask_value, "source", slot=1, pinned=order > 0)
        _check_against_a(e, imgs, hl, mode, mask_value, net, full, (ab, ab2), "order %+d," % order)
    for i in (2, 4, 6):                                          # ... and (b), the blocking route, for three of them
        want_ab, want_net, want_full = _blocking(e, images[i][None], [hints[i]], mode, mask_value)
        np.testing.assert_array_equal(ab[6 - i], want_ab[0])
        np.testing.assert_array_equal(net[6 - i], want_net[0])
        np.testing.assert_array_equal(full[6 - i], want_full[0])


def test_mixed_batch_fp32(eng):
    e = eng(64, 64, "fp32")
    images = _images(e, R.MIXED, 400)
    hints = [HINTS_RGB[i % 4] for i in range(len(images))]
    net, ab = _run(e, images, hints, "rgb", 110.0, "net")
    full, ab2 = _run(e, images, hints, "rgb", 110.0, "source", slot=1, pinned=True)
    _check_against_a(e, images, hints, "rgb", 110.0, net, full, (ab, ab2))
    want_ab, want_net, want_full = _blocking(e, images[4][None], [hints[4]], "rgb", 110.0)
    np.testing.assert_array_equal(ab[4], want_ab[0])
    np.testing.assert_array_equal(full[4], want_full[0])


# ------------------------------------------------------------------------------------------------ 2. groups that span many images
@pytest.mark.parametrize("case", range(len(R.SPANS)), ids=["four_in_one_group", "tail_is_an_image", "three_boundaries"])
@pytest.mark.parametrize("H,W", [(64, 64), (40, 72)])
def test_groups_that_span_many_images(eng, H, W, case):
    e = eng(H, W)
    images = _images(e, R.SPANS[case], 500 + 20 * case)
    hints = [HINTS_AB[(i + 1) % 4] for i in range(len(images))]
    for pinned in (False, True):
        full, ab = _run(e, images, hints, "ab", 1.0, "source", slot=int(pinned), pinned=pinned)
        _check_against_a(e, images, hints, "ab", 1.0, None, full, (ab,), "pinned %s," % pinned)


# ------------------------------------------------------------------------------------------------ 3. position and neighbours
def test_an_image_does_not_depend_on_its_position_or_its_neighbours(eng):
    e = eng(64, 64)
    me, hint = R.image(37, 41, 402), HINTS_AB[1]
    first = [me, R.image(203, 187, 611)]
    last = [R.image(130, 97, 620 + j) for j in range(7)] + [me]
    res = []
    for imgs, at in ((first, 0), (last, 7)):
        hl = [HINTS_AB[2]] * len(imgs)
        hl[at] = hint
        net, ab = _run(e, imgs, hl, "ab", 1.0, "net")
        full, _ = _run(e, imgs, hl, "ab", 1.0, "source", slot=1)
        res.append((ab[at].copy(), net[at].copy(), full[at].copy()))
    for got in res:
        for g, w in zip(got, _ref_a(e, me, hint, "ab", 1.0)):
            np.testing.assert_array_equal(g, w)
    for a, b in zip(*res):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ 4. a uniform batch
def test_uniform_batch_equals_the_same_size_call(eng):
    e = eng(40, 72)
    batch = _batch(4, 130, 97, 640)
    hints = _hint_lists(4, "rgb", 1)
    for out in ("net", "source"):
        want = np.empty(batch.shape if out == "source" else (4, 40, 72, 3), np.uint8)
        want_ab = np.empty((4, 2, 40, 72), np.float32)
        e.forward_async_rgb(0, batch, hints, want, out_ab=want_ab, mode="rgb", mask_value=110.0, out=out)
        e.wait(0)
        got, ab = _run(e, list(batch), hints, "rgb", 110.0, out, slot=1)
        np.testing.assert_array_equal(np.stack(got), want)
        np.testing.assert_array_equal(ab, want_ab)


# ------------------------------------------------------------------------------------------------ 5. an independent reference
def test_mixed_batch_matches_the_oracle_colour_conversions(eng):
    e = eng(64, 64)
    groups = [_batch(3, sh, sw, 30) for sh, sw in ((5, 7), (130, 97))]
    images = [g[i] for i in range(3) for g in groups]                         # interleaved: all six in ONE call
    hints = [h for h in _hint_lists(3, "ab", 0) for _ in groups]
    net, out_ab = _run(e, images, hints, "ab", 1.0, "net")
    full, _ = _run(e, images, hints, "ab", 1.0, "source", slot=1)
    assert np.isfinite(out_ab).all() and np.abs(out_ab).max() > 0
    for i, img in enumerate(images):
        sh, sw = img.shape[:2]
        lab = ingest_ref.net_lab(ingest_ref.net_rgb(img, 64, 64))
        L = np.float32(lab[0] - 50).astype(np.float64) + 50                   # the slot's fp32 L plane, + l_cent
        _check_u8(net[i], ocs.lab2rgb_transpose(L[None], out_ab[i].astype(np.float64)), "net-size image %d of %dx%d sources" % (i, sh, sw))
        refreshed_ab = ingest_ref.net_lab(net[i])[1:]
        _check_u8(full[i], ingest_ref.fullres(img, refreshed_ab, 1), "source-size image %d of %dx%d sources" % (i, sh, sw))
    assert FRAC * 105 < 1                                                     # the (5,7) outputs admit no differing value


# ------------------------------------------------------------------------------------------------ 6. the pipeline
SIZE_POOL = [(1, 1), (5, 7), (37, 41), (64, 64), (130, 97), (203, 187), (2, 3), (40, 72)]


def _mixed_jobs(e):
    """Six mixed batches, n in 1..8, the sizes shuffled per batch."""
    rs = np.random.RandomState(77)
    jobs = []
    for k, n in enumerate((5, 8, 1, 3, 7, 2)):
        sz = [SIZE_POOL[j] for j in rs.permutation(8)[:n]]
        images = [R.image(sh, sw, 700 + 10 * k + j) for j, (sh, sw) in enumerate(sz)]
        hints = [HINTS_RGB[(j + k) % 4] for j in range(n)]
        jobs.append((images, hints, "source" if k in (1, 2, 5) else "net"))
    return jobs


@pytest.mark.parametrize("memory", ["pinned", "pageable", "mixed"])
def test_six_mixed_batches_through_two_slots_between_other_batches(eng, memory):
    e = eng(64, 64)
    new = lambda shape, p, dtype=np.uint8: e.pinned_empty(shape, dtype) if p else np.empty(shape, dtype)
    planes = workloads.random_batch(3, 64, seed=61)
    planes_ref = e.forward(*planes, 0.0).copy()
    same = _batch(3, 37, 41, 760)
    same_hints = _hint_lists(3, "rgb", 2)
    same_ref = [_ref_a(e, same[i], same_hints[i], "rgb", 110.0) for i in range(3)]
    queue = []                                                   # (kind, submit(slot), check())
    for k, (images, hints, out) in enumerate(_mixed_jobs(e)):
        pin_in = [memory == "pinned" or (memory == "mixed" and (j + k) % 2 == 0) for j in range(len(images))]
        pin_out = [memory == "pinned" or (memory == "mixed" and (j + k) % 3 == 0) for j in range(len(images))]
        srcs = [new(a.shape, p) for a, p in zip(images, pin_in)]
        for s, a in zip(srcs, images):
            s[...] = a
        outs = [new(a.shape if out == "source" else (64, 64, 3), p) for a, p in zip(images, pin_out)]
        dab = new((len(images), 2, 64, 64), memory == "pinned", np.float32)

        def submit(slot, srcs=srcs, hints=hints, outs=outs, dab=dab, out=out):
            e.forward_async_images(slot, srcs, hints, outs, out_ab=dab, mode="rgb", mask_value=110.0, out=out)

        def check(images=images, hints=hints, outs=outs, dab=dab, out=out, k=k):
            _check_against_a(e, images, hints, "rgb", 110.0, outs if out == "net" else None, outs if out == "source" else None, (dab,),
                             "%s, batch %d," % (memory, k))
        queue.append(("images", submit, check))
        if k == 1:                                               # a plain forward_async batch takes the next slot in between ...
            arrs = [new(x.shape, memory == "pinned", np.float32) for x in planes] + [new(planes_ref.shape, memory == "pinned", np.float32)]
            for d, s in zip(arrs[:3], planes):
                d[...] = s
            queue.append(("planes", lambda slot, arrs=arrs: e.forward_async(slot, arrs[0], arrs[1], arrs[2], arrs[3], 0.0),
                          lambda arrs=arrs: np.testing.assert_array_equal(arrs[3], planes_ref)))
        if k == 3:                                               # ... and a same-size forward_async_rgb batch
            dst, dab3 = new((3, 64, 64, 3), memory == "pinned"), new((3, 2, 64, 64), memory == "pinned", np.float32)

            def check_same(dst=dst, dab3=dab3):
                for i in range(3):
                    np.testing.assert_array_equal(dab3[i], same_ref[i][0])
                    np.testing.assert_array_equal(dst[i], same_ref[i][1])
            queue.append(("rgb", lambda slot, dst=dst, dab3=dab3: e.forward_async_rgb(slot, same, same_hints, dst, out_ab=dab3, mode="rgb",
                                                                                      mask_value=110.0), check_same))
    times = {}
    for k, (kind, submit, _) in enumerate(queue):
        slot = k & 1
        if k >= 2:
            e.wait(slot)
            times[k - 2] = e.pipeline_times(slot)
        submit(slot)
    for k in (len(queue) - 2, len(queue) - 1):
        e.wait(k & 1)
        times[k] = e.pipeline_times(k & 1)
    for k, (kind, _, check) in enumerate(queue):
        check()
        t = times[k]
        print("job %d (%s): h2d %.3f ms, compute %.3f ms, d2h %.3f ms" % (k, kind, t[1] - t[0], t[3] - t[2], t[5] - t[4]))
        assert t.shape == (6,) and np.isfinite(t).all()
        assert np.all(np.diff(t) >= -1e-3), t                    # h2d start <= h2d end <= compute start <= ... <= d2h end
        if k:
            assert t[3] > times[k - 1][3]                        # job k computed after job k - 1


@pytest.mark.parametrize("out", ["net", "source"])
def test_colorize_images_yields_every_image_in_order(eng, out):
    e = eng(64, 64)
    rs = np.random.RandomState(19)
    sz = [SIZE_POOL[j] for j in rs.randint(0, 8, 19)]
    images = [R.image(sh, sw, 800 + j) for j, (sh, sw) in enumerate(sz)]
    hints = [HINTS_AB[j % 4] for j in range(19)]
    items = [(a, h) if j % 5 else ((a, h) if h is not None else a) for j, (a, h) in enumerate(zip(images, hints))]
    got = list(e.colorize_images(iter(items), batch=8, out=out, mode="ab", mask_value=1.0))
    assert len(got) == 19
    assert [g.shape for g in got] == [a.shape if out == "source" else (64, 64, 3) for a in images]
    _check_against_a(e, images, hints, "ab", 1.0, got if out == "net" else None, got if out == "source" else None)
    assert not e._in_flight


# ------------------------------------------------------------------------------------------------ 7. references
def test_mixed_batch_with_references_of_individual_sizes():
    e = engine.HipColorizer(64, 64, max_batch=8, precision="bf16", global_hints=True)
    e.load_state_dict(_glob_sd(3))
    c, r = G.centres(), G.refs64()
    assert len(set(x.shape for x in r[:3])) > 1                  # references of individual sizes
    images = [R.image(sh, sw, 900 + j) for j, (sh, sw) in enumerate([(37, 41), (5, 7), (130, 97), (64, 64)])]
    hints = [HINTS_AB[1], None, HINTS_AB[2], HINTS_AB[3]]
    refs, index = [r[0], r[1], r[2]], [1, -1, 0, 1]              # one image without, one reference shared by two images
    own = workloads.global_hint_config5(8, seed=5)[0]
    e.set_global_hints(own)
    L, ab, mask = workloads.random_batch(8, 64, seed=22, max_points=4, max_p=3)
    before = e.forward(L, ab, mask).copy()
    want = []
    for i, img in enumerate(images):                             # forward_async_rgb(refs=...) with n = 1 per image
        one = np.ascontiguousarray(img[None])
        net, full = np.empty((1, 64, 64, 3), np.uint8), np.empty(one.shape, np.uint8)
        wab = np.empty((1, 2, 64, 64), np.float32)
        rf, ix = ([refs[index[i]]], [0]) if index[i] >= 0 else ([], None)
        e.forward_async_rgb(0, one, [hints[i]], net, out_ab=wab, refs=rf, ref_index=ix, centres=c, saturation=True)
        e.forward_async_rgb(1, one, [hints[i]], full, out="source", refs=rf, ref_index=ix, centres=c, saturation=True)
        e.wait(0); e.wait(1)
        want.append((wab[0], net[0], full[0]))
    assert np.abs(want[0][0] - want[1][0]).max() > 0
    for slot, out in ((0, "net"), (1, "source")):
        outs = [np.full(a.shape if out == "source" else (64, 64, 3), 7, np.uint8) for a in images]
        dab = np.empty((4, 2, 64, 64), np.float32)
        e.forward_async_images(slot, images, hints, outs, out_ab=dab, out=out, refs=refs, ref_index=index, centres=c, saturation=True)
        e.wait(slot)
        assert np.all(np.diff(e.pipeline_times(slot)) >= -1e-3)
        for i in range(4):
            np.testing.assert_array_equal(dab[i], want[i][0], err_msg="out_ab of image %d, out=%s" % (i, out))
            np.testing.assert_array_equal(outs[i], want[i][2 if out == "source" else 1], err_msg="rgb_out of image %d, out=%s" % (i, out))
    # without the references the same batch is another: they were read
    plain = [np.empty((64, 64, 3), np.uint8) for _ in images]
    e.clear_global_hints()
    e.forward_async_images(0, images, hints, plain)
    e.wait(0)
    assert np.abs(plain[0].astype(int) - want[0][1].astype(int)).max() > 0
    # the handle's own global inputs were neither read (above) nor written
    e.set_global_hints(own)
    np.testing.assert_array_equal(e.forward(L, ab, mask), before)
    e.close()


# ------------------------------------------------------------------------------------------------ 8. nothing else moved
def test_resident_state_is_untouched_by_mixed_batches_on_both_slots(make_sd):
    e = engine.HipColorizer(64, 64, max_batch=8, precision="bf16")
    e.load_state_dict(make_sd(0, "he"))
    L, ab, mask = workloads.random_batch(1, 64, seed=9, max_points=4, max_p=3)
    l_out = np.random.RandomState(3).uniform(0, 100, (90, 75))
    src = ingest_ref.source_image(130, 97, 16)
    e.set_image_rgb(src, img=1, keep_source=True)
    e.set_hints(HINTS_AB[1], mode="ab", img=1, mask_value=110.0)

    def everything():
        out = e.forward(L, ab, mask).copy()
        rgb = e.forward_rgb_lazy(L, ab, mask).copy()
        up = e.upsample_lab2rgb(l_out, "output_ab", "linear").copy()
        kept = e.fullres_rgb("input_ab", "nearest", "mask50", img=1).copy()    # the kept source, the resident hint planes, hint_mask_value
        hab, hm = e.hint_planes(1)
        return out, rgb, up, kept, hab, hm

    before = everything()
    assert before[3].any() and before[5].max() == 110.0
    results = []
    for slot, out in ((0, "net"), (1, "source")):
        images = [R.image(sh, sw, 70 + slot) for sh, sw in ((37, 41), (5, 7), (130, 97))]
        results.append(e.forward_async_images(slot, images, [HINTS_AB[1 + slot]] * 3, mode="ab", mask_value=1.0, out=out))
    e.wait(0); e.wait(1)
    assert all(r.any() for res in results for r in res)
    assert [r.shape for r in results[1]] == [(37, 41, 3), (5, 7, 3), (130, 97, 3)]
    # the resident results are still the last blocking forward's, before any other blocking call refreshes them
    np.testing.assert_array_equal(e.upsample_lab2rgb(l_out, "output_ab", "linear"), before[2])
    np.testing.assert_array_equal(e.fullres_rgb("input_ab", "nearest", "mask50", img=1), before[3])
    for a, b in zip(e.hint_planes(1), before[4:]):
        np.testing.assert_array_equal(a, b)
    # a mixed batch in flight with pageable outputs is drained by the blocking calls
    dst = [np.zeros((64, 64, 3), np.uint8), np.zeros((64, 64, 3), np.uint8)]
    e.forward_async_images(0, [R.image(5, 7, 80), R.image(2, 3, 81)], None, dst)
    after = everything()
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    assert dst[0].any() and dst[1].any()                         # ... and both results were delivered
    e.close()


# ------------------------------------------------------------------------------------------------ 9. statuses
def test_statuses_and_a_refused_call_leaves_the_slot_usable(eng, make_sd):
    vp = ctypes.c_void_p
    e = eng(64, 64)
    lib, h = e.lib, e._h
    images = [R.image(5, 7, 90), R.image(37, 41, 91)]
    hl = [[(3, 4, 20, 30, 40.0, -30.0)], [(3, 4, 20, 30, 40.0, -30.0)]]
    want = [_ref_a(e, images[i], hl[i], "ab", 1.0) for i in range(2)]
    dst = [np.empty((64, 64, 3), np.uint8) for _ in range(2)]
    offs = np.array([0, 1, 2], np.int32)
    hints = (N.Hint * 2)()
    for k in range(2):
        hints[k].y0, hints[k].x0, hints[k].y1, hints[k].x1, hints[k].c0, hints[k].c1, hints[k].c2 = 3, 4, 20, 30, 40.0, -30.0, 0.0
    P = lambda a: a.ctypes.data_as(vp)
    HP = ctypes.cast(hints, vp)

    def table(*entries):                                         # (pointer or None, h, w) -> idc_ref_image[]
        t = (N.RefImage * max(len(entries), 1))()
        for k, (p, sh, sw) in enumerate(entries):
            t[k].rgb, t[k].h, t[k].w = p, sh, sw
        return t

    def pointers(*ps):
        return (vp * max(len(ps), 1))(*ps)

    good = table((images[0].ctypes.data, 5, 7), (images[1].ctypes.data, 37, 41))
    small = images[0].ctypes.data
    OUT = pointers(dst[0].ctypes.data, dst[1].ctypes.data)
    c = G.centres()
    ref = G.refs64()[0]
    rtab = table((ref.ctypes.data, ref.shape[0], ref.shape[1]))
    bad_offs = [np.array(x, np.int32) for x in ([1, 1, 2], [0, 2, 1], [0, 1, (1 << 20) + 1])]     # not from 0, decreasing, beyond 2^20 hints
    i00, i01 = np.array([0, 0], np.int32), np.array([0, 1], np.int32)

    def call(slot=0, n=2, imgs=good, offsets=P(offs), hp=HP, mode=0, flags=0, refs=None, out=OUT, handle=h):
        return lib.idc_forward_async_images(handle, slot, n, imgs, offsets, hp, mode, 1.0, 0.0, 50.0, flags, refs, out, None)

    def after_a_refusal(slot):
        got = [np.empty((64, 64, 3), np.uint8) for _ in range(2)]
        assert call(slot=slot, out=pointers(got[0].ctypes.data, got[1].ctypes.data)) == 0
        e.wait(slot)
        for i in range(2):
            np.testing.assert_array_equal(got[i], want[i][1])

    INVALID, NO_WEIGHTS, BATCH, UNSUPPORTED = -1, -4, -6, -7
    refusals = [
        # the codes of idc_forward_async_rgb for the shared arguments
        (dict(slot=-1), INVALID), (dict(slot=2), INVALID), (dict(flags=2), INVALID), (dict(flags=0x80000001), INVALID),
        (dict(mode=2), INVALID), (dict(mode=-1), INVALID), (dict(hp=None), INVALID),
        (dict(offsets=P(bad_offs[0])), INVALID), (dict(offsets=P(bad_offs[1])), INVALID),
        (dict(offsets=P(bad_offs[2])), INVALID), (dict(n=0), BATCH), (dict(n=9), BATCH),
        # the images and their outputs
        (dict(imgs=None), INVALID), (dict(out=None), INVALID),
        (dict(imgs=table((small, 5, 7), (None, 37, 41))), INVALID), (dict(out=pointers(dst[0].ctypes.data, None)), INVALID),
        (dict(imgs=table((small, 0, 7), (small, 5, 7))), INVALID), (dict(imgs=table((small, 5, 7), (small, 5, 0))), INVALID),
        (dict(imgs=table((small, 16385, 7), (small, 5, 7))), INVALID), (dict(imgs=table((small, 5, 7), (small, 5, 16385))), INVALID),
        (dict(imgs=table((small, 5, -1), (small, 5, 7))), INVALID),
        # 768 MiB + 768 MiB claimed over one valid 105-byte buffer: above IDC_BATCH_MAX_SOURCE_BYTES, refused before a byte is read
        (dict(imgs=table((small, 16384, 16384), (small, 16384, 16384))), INVALID),
        # the reference block: idc_forward_async_rgb_ref's codes
        (dict(refs=ctypes.byref(N.BatchRefs(1, rtab, None, c.ctypes.data, 1.0, 0))), INVALID),            # NULL ref_index needs m == n
        (dict(refs=ctypes.byref(N.BatchRefs(-1, rtab, None, c.ctypes.data, 1.0, 0))), INVALID),
        (dict(refs=ctypes.byref(N.BatchRefs(1, None, None, c.ctypes.data, 1.0, 0))), INVALID),
        (dict(refs=ctypes.byref(N.BatchRefs(1, rtab, i01.ctypes.data, c.ctypes.data, 1.0, 0))), INVALID),
        (dict(refs=ctypes.byref(N.BatchRefs(1, rtab, i00.ctypes.data, None, 1.0, 0))), INVALID),
        (dict(refs=ctypes.byref(N.BatchRefs(1, rtab, i00.ctypes.data, c.ctypes.data, 1.0, 2))), INVALID),
        (dict(refs=ctypes.byref(N.BatchRefs(1, rtab, i00.ctypes.data, c.ctypes.data, float("nan"), 0))), INVALID),
        (dict(refs=ctypes.byref(N.BatchRefs(1, rtab, i00.ctypes.data, c.ctypes.data, 1.0, 0))), UNSUPPORTED),   # no IDC_FLAG_GLOBAL_HINTS
    ]
    for k, (kw, code) in enumerate(refusals):
        assert call(slot=kw.pop("slot", k & 1), **kw) == code, (k, kw)
        after_a_refusal(k & 1)
    e.set_range_audit(True)
    assert call() == UNSUPPORTED
    e.set_range_audit(False)
    after_a_refusal(0)
    bare = engine.HipColorizer(64, 64, max_batch=8, precision="bf16")
    assert call(handle=bare._h) == NO_WEIGHTS
    bare.close()
    assert call(offsets=None, hp=None) == 0                      # NULL offsets: hints is not looked at
    assert call(slot=0) == INVALID                               # still in flight
    e.wait(0)
    after_a_refusal(0)
    full, ab = _run(e, images, hl, "ab", 1.0, "source", slot=1)
    _check_against_a(e, images, hl, "ab", 1.0, None, full, (ab,))
