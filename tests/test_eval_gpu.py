"""GPU checks of the evaluation batches: idc_reveal_hints (a hint's colour = the mean ground-truth ab under its rectangle, from the slot's kept
source) and idc_forward_async_eval (idc_forward_async_images that reveals its hints on the device and scores its result against the ground
truth, sse [n,3] uint64), through HipColorizer.reveal_hints / forward_async_eval / evaluate_images and ColorizeImageBase.net_forward_reveal.

References, none of them the code under test:
  tests/eval_ref.py     float64 means over tests/ingest_ref.py's Lab, planes painted in list order, SSE in Python integers;
  the blocking route    set_image_rgb(keep_source=True), reveal_hints, forward_resident, fullres_rgb per image (for the pipelined call);
  forward_async_images  in 'ab' mode, fed the colours the eval call reported (an existing call).
Bars: a revealed float32 is np.float32 of eval_ref's float64 mean or one of its two float32 neighbours -- the float64 error of any summation
order and of the last bits of cbrt / pow is far below a float32 ulp (tests/test_eval_cpu.py shows the orders agree), so one ulp is the whole
allowance; masks, unpainted pixels, 1 x 1 rectangles (against the device's own lab_net), repeated runs, pipelined against blocking, and every
sse are bit for bit / exact.
Shapes: 64 x 64 and 40 x 72 handles, bf16 (one case fp32), max_batch 8, tests/ragged_ref.py's MIXED sizes with seeds 400 + j."""
import ctypes

import numpy as np
import pytest

import eval_ref as E
import ingest_ref
import ragged_ref as R
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import api, engine, evaluate, workloads
from test_batch_rgb_gpu import HINTS_AB, HINTS_RGB

pytestmark = pytest.mark.gpu

_ENG = {}
_LAB = {}
_BLOCKING = {}


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
    _LAB.clear()
    _BLOCKING.clear()


def _images(e):
    return [R.image(sh, sw, 400 + j) for j, (sh, sw) in enumerate(R.sizes(R.MIXED, e.H, e.W))]


def _lists(n, shift=0):
    return [E.LISTS[(i + shift) % 4] for i in range(n)]


def _lab(j, H, W):
    """eval_ref's float64 Lab of image j of the mixed batch, made once and not written to."""
    if (j, H, W) not in _LAB:
        sh, sw = R.sizes(R.MIXED, H, W)[j]
        lab = E.lab_of(R.image(sh, sw, 400 + j), H, W)
        lab.setflags(write=False)
        _LAB[(j, H, W)] = lab
    return _LAB[(j, H, W)]


def _blocking(e, j, rects, mask_value=1.0):
    """The blocking route for image j of the mixed batch -> (colours, out_ab [2,H,W], net-size rgb, source-size rgb); once per case."""
    key = (e.key, j, repr(rects), mask_value)
    if key not in _BLOCKING:
        img = _images(e)[j]
        e.set_image_rgb(img, img=0, keep_source=True, want_rgb=False, want_lab=False)
        cols = e.reveal_hints(rects or [], img=0, mask_value=mask_value)
        ab, rgb, _ = e.forward_resident(1)
        full = e.fullres_rgb("output_ab", "linear", "image", img=0)
        res = (cols.copy(), ab[0].copy(), rgb[0].copy(), full.copy())
        for a in res:
            a.setflags(write=False)
        _BLOCKING[key] = res
    return _BLOCKING[key]


def _eval(e, images, hints, mode="reveal", out="net", slot=0, pinned=False, want_rgb=True, mask_value=1.0, want_ab=True):
    """The call under test -> (sse (n,3), hint_colours | None, list of rgb outputs | None, out_ab | None), the caller's own copies."""
    n = len(images)
    pins = [pinned] * n if isinstance(pinned, bool) else list(pinned)
    new = lambda shape, p, dtype=np.uint8: e.pinned_empty(shape, dtype) if p else np.empty(shape, dtype)
    srcs = []
    for a, p in zip(images, pins):
        s = new(a.shape, p)
        s[...] = a
        srcs.append(s)
    outs = None
    if want_rgb:
        outs = [new(a.shape if out == "source" else (e.H, e.W, 3), not p) for a, p in zip(images, pins)]
        for o in outs:
            o[...] = 7
    ab = new((n, 2, e.H, e.W), pins[0], np.float32) if want_ab else None
    sse, cols, got = e.forward_async_eval(slot, srcs, hints, outs, out_ab=ab, mode=mode, mask_value=mask_value, out=out)
    e.wait(slot)
    assert (got is None) == (outs is None)
    return np.array(sse), None if cols is None else np.array(cols), outs, ab


def _split(cols, hints):
    """The per-image slices of hint_colours."""
    res, at = [], 0
    for h in hints:
        k = len(h or [])
        res.append(cols[at:at + k])
        at += k
    assert at == len(cols)
    return res


# ------------------------------------------------------------------------------------------------ 1. reveal against float64
@pytest.mark.parametrize("mask_value", [1.0, 110.0])
@pytest.mark.parametrize("H,W", [(64, 64), (40, 72)])
def test_reveal_hints_against_float64(eng, H, W, mask_value):
    e = eng(H, W)
    painted_values = 0
    for j, img in enumerate(_images(e)):
        _, lab_dev = e.set_image_rgb(img, img=1, keep_source=True)
        lab_dev = lab_dev[0].copy()
        for li, rects in enumerate((E.R1, E.R2, E.R3)):
            what = "%dx%d handle, image %d %s, list R%d" % (H, W, j, img.shape, li + 1)
            cols = e.reveal_hints(rects, img=1, mask_value=mask_value)
            ab, mask = e.hint_planes(1)
            want_ab, want_mask = E.planes(_lab(j, H, W), rects, mask_value)
            want_cols, clipped = E.reveal(_lab(j, H, W), rects)
            on = want_mask[0] > 0
            assert mask.tobytes() == want_mask.tobytes(), what                       # the mask, bit for bit
            assert not ab[:, ~on].any() and not np.signbit(ab[:, ~on]).any(), what   # unpainted pixels: +0
            assert E.within_one_ulp(ab[:, on], want_ab[:, on]).all(), what
            painted_values += int(on.sum())
            # colours: one pair per input rectangle, (0, 0) for a dropped one; the planes hold exactly these values, the later hint on top
            assert cols.shape == (len(rects), 2) and cols.dtype == np.float32
            mine = np.zeros((2, H, W), np.float32)
            for k, c in enumerate(clipped):
                if c is None:
                    assert cols[k].tobytes() == np.zeros(2, np.float32).tobytes(), what
                    continue
                assert E.within_one_ulp(cols[k], want_cols[k]).all(), what
                mine[:, c[0]:c[2] + 1, c[1]:c[3] + 1] = cols[k][:, None, None]
                if (c[0], c[1]) == (c[2], c[3]):                                    # 1 x 1: the device's own Lab of that pixel, rounded once
                    assert cols[k].tobytes() == lab_dev[1:, c[0], c[1]].astype(np.float32).tobytes(), what
            assert ab.tobytes() == mine.tobytes(), what
    assert painted_values > 7 * H * W                                               # R3 alone paints every pixel of every image


# ------------------------------------------------------------------------------------------------ 2. a rectangle's value is its own
@pytest.mark.parametrize("H,W", [(64, 64), (40, 72)])
def test_a_rectangle_reveals_the_same_bits_on_every_route(eng, H, W):
    e = eng(H, W)
    images = _images(e)
    rects = E.R1 + E.R2 + E.R3
    alone = []
    for img in images:
        e.set_image_rgb(img, img=3, keep_source=True, want_rgb=False, want_lab=False)
        alone.append(e.reveal_hints(rects, img=3).copy())
    assert np.abs(alone[2]).max() > 0 and (alone[2] != alone[4]).any()
    runs = []
    for order, slot, shift in ((1, 0, 0), (-1, 1, 0), (1, 1, 0), (-1, 0, 1)):
        # forwards: image j at position j (the 1 x 1 image at position 0); reversed: at 6 - j (the 1 x 1 image at position 6)
        hl = [rects if (i + shift) % 2 == 0 else rects[::-1] for i in range(7)]     # also at another place in the list, among other rectangles
        sse, cols, _, _ = _eval(e, images[::order], hl, slot=slot, want_rgb=False, want_ab=False, pinned=order < 0)
        per = _split(cols, hl)[::order]
        runs.append([c if (i + shift) % 2 == 0 else c[::-1] for i, c in zip(range(7)[::order], per)])
    for run in runs:
        for j in range(7):
            assert run[j].tobytes() == alone[j].tobytes(), "image %d" % j


# ------------------------------------------------------------------------------------------------ 3. pipelined equals blocking
@pytest.mark.parametrize("H,W,precision,mask_value", [(64, 64, "bf16", 1.0), (40, 72, "bf16", 110.0), (64, 64, "fp32", 1.0)])
def test_eval_batch_equals_the_blocking_route_bit_for_bit(eng, H, W, precision, mask_value):
    e = eng(H, W, precision)
    images = _images(e)
    hints = _lists(7)
    want = [_blocking(e, j, hints[j], mask_value) for j in range(7)]
    assert np.abs(want[0][1]).max() > 0 and all(np.isfinite(w[1]).all() for w in want)
    mixed = [j % 2 == 0 for j in range(7)]                          # sources pinned / outputs pageable and the other way round, image by image
    sse_n, cols, net, ab = _eval(e, images, hints, out="net", slot=0, pinned=mixed, mask_value=mask_value)
    sse_s, cols2, full, ab2 = _eval(e, images, hints, out="source", slot=1, pinned=[not m for m in mixed], mask_value=mask_value)
    assert cols.tobytes() == cols2.tobytes()
    for j, c in enumerate(_split(cols, hints)):
        what = "image %d" % j
        assert c.tobytes() == want[j][0].tobytes(), what
        np.testing.assert_array_equal(ab[j], want[j][1], err_msg=what)
        np.testing.assert_array_equal(ab2[j], want[j][1], err_msg=what)
        np.testing.assert_array_equal(net[j], want[j][2], err_msg=what)
        np.testing.assert_array_equal(full[j], want[j][3], err_msg=what)
    # ... and the existing batch call in 'ab' mode, fed the colours the eval call reported
    given = [None if h is None else [tuple(r) + (float(c[0]), float(c[1])) for r, c in zip(h, cs)] for h, cs in zip(hints, _split(cols, hints))]
    for out, got, got_ab, slot in (("net", net, ab, 0), ("source", full, ab2, 1)):
        dab = np.empty((7, 2, H, W), np.float32)
        ref = e.forward_async_images(slot, images, given, out_ab=dab, mode="ab", mask_value=mask_value, out=out)
        e.wait(slot)
        np.testing.assert_array_equal(got_ab, dab)
        for j in range(7):
            np.testing.assert_array_equal(got[j], ref[j], err_msg="out=%s, image %d" % (out, j))


# ------------------------------------------------------------------------------------------------ 4. the score
def _truth(e, img, out):
    return img if out == "source" else ingest_ref.net_rgb(img, e.H, e.W)


@pytest.mark.parametrize("out", ["net", "source"])
@pytest.mark.parametrize("H,W", [(64, 64), (40, 72)])
def test_sse_is_exact(eng, H, W, out):
    e = eng(H, W)
    images = _images(e)
    seen = {}
    for order in (1, -1):                                            # reversed: the image starts fall on other residues mod 4
        imgs, hints = images[::order], _lists(7)[::order]
        sse, _, outs, _ = _eval(e, imgs, hints, out=out, slot=int(order < 0), pinned=order > 0)
        assert sse.shape == (7, 3) and sse.dtype == np.uint64
        for i, (img, o) in enumerate(zip(imgs, outs)):
            assert sse[i].tolist() == E.sse(o, _truth(e, img, out)), "order %+d, image %d %s" % (order, i, img.shape)
        quiet, _, none, _ = _eval(e, imgs, hints, out=out, slot=int(order > 0), want_rgb=False, want_ab=False)
        assert none is None and quiet.tobytes() == sse.tobytes()    # no image left the device: the same score
        seen[order] = sse
    np.testing.assert_array_equal(seen[1], seen[-1][::-1])          # an image's score does not depend on where it lay
    assert seen[1].max() > 0 and int(seen[1][5].sum()) > 0
    # not vacuous: revealing colours changes the score of the same image
    j = 5
    a, _, _, _ = _eval(e, [images[j]], [E.R3], out=out, want_rgb=False, want_ab=False)
    b, _, _, _ = _eval(e, [images[j]], [None], out=out, slot=1, want_rgb=False, want_ab=False)
    assert a.tolist() != b.tolist()
    h, w = images[j].shape[:2] if out == "source" else (H, W)
    print("%dx%d handle, %s, image %s: PSNR %.3f dB without hints, %.3f dB with R3" % (H, W, out, images[j].shape,
                                                                                      evaluate.psnr_from_sse(b[0], h, w), evaluate.psnr_from_sse(a[0], h, w)))


@pytest.mark.parametrize("mode", ["ab", "rgb"])
def test_sse_scores_a_given_hint_list(eng, mode):
    e = eng(40, 72)
    images = _images(e)
    table = HINTS_AB if mode == "ab" else HINTS_RGB
    hints = [table[i % 4] for i in range(7)]
    for out, slot in (("net", 0), ("source", 1)):
        sse, cols, outs, ab = _eval(e, images, hints, mode=mode, out=out, slot=slot, mask_value=110.0)
        assert cols is None
        dab = np.empty((7, 2, 40, 72), np.float32)
        ref = e.forward_async_images(1 - slot, images, hints, out_ab=dab, mode=mode, mask_value=110.0, out=out)
        e.wait(1 - slot)
        np.testing.assert_array_equal(ab, dab)
        for i in range(7):
            np.testing.assert_array_equal(outs[i], ref[i])
            assert sse[i].tolist() == E.sse(ref[i], _truth(e, images[i], out))


def test_evaluate_images_and_psnr_sweep(eng):
    e = eng(64, 64)
    images = _images(e) + _images(e)[:4]                             # 11 images: two batches of 4 and one of 3
    hints = _lists(11, 1)
    got = list(e.evaluate_images(zip(images, hints), batch=4, out="source"))
    assert len(got) == 11 and not e._in_flight
    sse, _, outs, _ = _eval(e, images[:7], hints[:7], out="source")
    for i in range(7):
        psnr, s = got[i]
        assert s.tolist() == sse[i].tolist()
        assert abs(psnr - E.psnr(outs[i], images[i])) <= 1e-12 * abs(psnr)
    table = evaluate.psnr_sweep(e, images[2:6], counts=(0, 2, 10), seed=1, batch=3)
    assert table.shape == (3, 4) and np.isfinite(table).all() and (table > 0).all()
    assert (table[0] != table[2]).any()
    np.testing.assert_array_equal(table, evaluate.psnr_sweep(e, images[2:6], counts=(0, 2, 10), seed=1, batch=4))


# ------------------------------------------------------------------------------------------------ 5. nothing else moved
def test_resident_state_is_untouched_by_eval_batches_on_both_slots(make_sd):
    e = engine.HipColorizer(64, 64, max_batch=8, precision="bf16")
    e.load_state_dict(make_sd(0, "he"))
    L, ab, mask = workloads.random_batch(1, 64, seed=9, max_points=4, max_p=3)
    l_out = np.random.RandomState(3).uniform(0, 100, (90, 75))
    src = ingest_ref.source_image(130, 97, 16)
    e.set_image_rgb(src, img=1, keep_source=True)
    e.reveal_hints(E.R1, img=1, mask_value=110.0)

    def everything():
        out = e.forward(L, ab, mask).copy()
        rgb = e.forward_rgb_lazy(L, ab, mask).copy()
        up = e.upsample_lab2rgb(l_out, "output_ab", "linear").copy()
        kept = e.fullres_rgb("input_ab", "nearest", "mask50", img=1).copy()    # the kept source, the resident hint planes, hint_mask_value
        hab, hm = e.hint_planes(1)
        return out, rgb, up, kept, hab, hm

    before = everything()
    assert before[3].any() and before[5].max() == 110.0 and np.abs(before[4]).max() > 0
    results = []
    for slot, out in ((0, "net"), (1, "source")):
        images = [R.image(sh, sw, 70 + slot) for sh, sw in ((37, 41), (5, 7), (130, 97))]
        results.append(e.forward_async_eval(slot, images, [E.R1, E.R3, None], out=out, want_rgb=True))
    e.wait(0); e.wait(1)
    assert all(int(r[0].sum()) > 0 and np.abs(r[1]).max() > 0 and all(o.any() for o in r[2]) for r in results)
    # the resident results are still the last blocking forward's, before any other blocking call refreshes them
    np.testing.assert_array_equal(e.upsample_lab2rgb(l_out, "output_ab", "linear"), before[2])
    np.testing.assert_array_equal(e.fullres_rgb("input_ab", "nearest", "mask50", img=1), before[3])
    for a, b in zip(e.hint_planes(1), before[4:]):
        np.testing.assert_array_equal(a, b)
    # an eval batch in flight with pageable results is drained by the blocking calls
    sse, cols = np.zeros((2, 3), np.uint64), np.zeros((1, 2), np.float32)
    imgs = [R.image(5, 7, 80), R.image(37, 41, 82)]
    table = (N.RefImage * 2)()
    for i, a in enumerate(imgs):
        table[i].rgb, table[i].h, table[i].w = a.ctypes.data, a.shape[0], a.shape[1]
    offs = np.array([0, 0, 1], np.int32)
    rect = (N.Hint * 1)()
    rect[0].y0, rect[0].x0, rect[0].y1, rect[0].x1 = 3, 4, 20, 30
    vp = ctypes.c_void_p
    assert e.lib.idc_forward_async_eval(e._h, 0, 2, table, offs.ctypes.data_as(vp), ctypes.cast(rect, vp), N.IDC_HINT_REVEAL, 1.0, 0.0, 50.0, 0,
                                        None, None, None, sse.ctypes.data_as(vp), cols.ctypes.data_as(vp)) == 0
    after = everything()
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    assert sse.all() and cols.all()                                  # ... and both results were delivered
    e.close()


# ------------------------------------------------------------------------------------------------ 6. statuses
def test_statuses_and_a_refused_call_leaves_the_slot_usable(eng):
    vp = ctypes.c_void_p
    e = eng(64, 64)
    lib, h = e.lib, e._h
    images = [R.image(5, 7, 90), R.image(37, 41, 91)]
    rl = [[(3, 4, 20, 30)], [(3, 4, 20, 30)]]
    want_sse, want_cols, _, _ = _eval(e, images, rl, want_rgb=False, want_ab=False)
    assert want_sse.all() and want_cols.all()
    dst = [np.empty((64, 64, 3), np.uint8) for _ in range(2)]
    offs = np.array([0, 1, 2], np.int32)
    hints = (N.Hint * 2)()
    for k in range(2):
        hints[k].y0, hints[k].x0, hints[k].y1, hints[k].x1, hints[k].c0, hints[k].c1, hints[k].c2 = 3, 4, 20, 30, 300.0, -30.0, 0.0
    P = lambda a: a.ctypes.data_as(vp)
    HP = ctypes.cast(hints, vp)

    def table(*entries):
        t = (N.RefImage * max(len(entries), 1))()
        for k, (p, sh, sw) in enumerate(entries):
            t[k].rgb, t[k].h, t[k].w = p, sh, sw
        return t

    def pointers(*ps):
        return (vp * max(len(ps), 1))(*ps)

    good = table((images[0].ctypes.data, 5, 7), (images[1].ctypes.data, 37, 41))
    small = images[0].ctypes.data
    sse, cols = np.zeros((2, 3), np.uint64), np.zeros((2, 2), np.float32)
    bad_offs = [np.array(x, np.int32) for x in ([1, 1, 2], [0, 2, 1], [0, 1, (1 << 20) + 1])]

    def call(slot=0, n=2, imgs=good, offsets=P(offs), hp=HP, mode=2, flags=0, out=None, s=P(sse), c=P(cols), handle=h):
        return lib.idc_forward_async_eval(handle, slot, n, imgs, offsets, hp, mode, 1.0, 0.0, 50.0, flags, None, out, None, s, c)

    def after_a_refusal(slot):
        sse[...] = 0; cols[...] = 0
        assert call(slot=slot) == 0                                  # rgb_out == NULL is allowed
        e.wait(slot)
        assert sse.tobytes() == want_sse.tobytes() and cols.tobytes() == want_cols.tobytes()

    INVALID, NO_WEIGHTS, BATCH, UNSUPPORTED = -1, -4, -6, -7
    refusals = [
        # the codes of idc_forward_async_images
        (dict(slot=-1), INVALID), (dict(slot=2), INVALID), (dict(flags=2), INVALID), (dict(mode=3), INVALID), (dict(mode=-1), INVALID),
        (dict(hp=None), INVALID), (dict(offsets=P(bad_offs[0])), INVALID), (dict(offsets=P(bad_offs[1])), INVALID),
        (dict(offsets=P(bad_offs[2])), INVALID), (dict(n=0), BATCH), (dict(n=9), BATCH), (dict(imgs=None), INVALID),
        (dict(imgs=table((small, 5, 7), (None, 37, 41))), INVALID), (dict(imgs=table((small, 0, 7), (small, 5, 7))), INVALID),
        (dict(imgs=table((small, 5, 7), (small, 5, 16385))), INVALID),
        (dict(imgs=table((small, 16384, 16384), (small, 16384, 16384))), INVALID),
        # its own: a NULL entry in a non-NULL rgb_out, a NULL sse, hint_colours without IDC_HINT_REVEAL, RGB colours outside 0..255
        (dict(out=pointers(dst[0].ctypes.data, None)), INVALID), (dict(s=None), INVALID),
        (dict(mode=0), INVALID), (dict(mode=1), INVALID), (dict(mode=1, c=None), INVALID),
    ]
    for k, (kw, code) in enumerate(refusals):
        assert call(slot=kw.pop("slot", k & 1), **kw) == code, (k, kw)
        after_a_refusal(k & 1)
    # the range check is IDC_HINT_RGB's alone: the same list is an ab list, and a list of rectangles
    assert call(mode=0, c=None) == 0
    e.wait(0)
    assert call(mode=2, c=None, out=pointers(dst[0].ctypes.data, dst[1].ctypes.data)) == 0
    e.wait(0)
    e.set_range_audit(True)
    assert call() == UNSUPPORTED
    e.set_range_audit(False)
    after_a_refusal(0)
    bare = engine.HipColorizer(64, 64, max_batch=8, precision="bf16")
    assert call(handle=bare._h) == NO_WEIGHTS
    # idc_reveal_hints: the codes of idc_set_hints, and no resident source
    col2 = np.zeros((2, 2), np.float32)
    fp = col2.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.idc_reveal_hints(bare._h, 0, 2, hints, 1.0, fp) == UNSUPPORTED
    bare.close()
    e.set_image_rgb(images[1], img=2, keep_source=True, want_rgb=False, want_lab=False)
    e.set_image_rgb(images[1], img=3, keep_source=False, want_rgb=False, want_lab=False)
    assert lib.idc_reveal_hints(h, -1, 2, hints, 1.0, fp) == BATCH
    assert lib.idc_reveal_hints(h, 8, 2, hints, 1.0, fp) == BATCH
    assert lib.idc_reveal_hints(h, 2, -1, hints, 1.0, fp) == INVALID
    assert lib.idc_reveal_hints(h, 2, 2, None, 1.0, fp) == INVALID
    assert lib.idc_reveal_hints(h, 3, 2, hints, 1.0, fp) == UNSUPPORTED
    assert b"no resident source" in lib.idc_last_error(h)
    assert lib.idc_reveal_hints(h, 2, 2, hints, 1.0, None) == 0     # NULL colours: the planes only
    assert lib.idc_reveal_hints(h, 2, 0, None, 1.0, None) == 0      # an empty list clears the planes
    assert not e.hint_planes(2)[1].any()
    assert lib.idc_reveal_hints(h, 2, 2, hints, 1.0, fp) == 0
    assert col2[0].tobytes() == want_cols[1].tobytes() == col2[1].tobytes()     # the image and the rectangle of the batch's second
    assert call(slot=0) == 0
    assert call(slot=0) == INVALID                                   # still in flight
    e.wait(0)
    after_a_refusal(0)


# ------------------------------------------------------------------------------------------------ 7. the wrapper
def test_net_forward_reveal_on_the_wrapper(make_sd):
    model = api.ColorizeImageTorch(Xd=64, precision="bf16")
    model.prep_net(path="", state_dict=make_sd(0, "he"))
    img = R.image(64, 64, 403)
    model.set_image(img)
    with pytest.raises(RuntimeError, match="load_image_device / set_image_device"):
        model.net_forward_reveal(E.R1)                               # the source is on the host only
    model.set_image_device(img)
    rgb = model.net_forward_reveal(E.R1).copy()
    assert rgb.shape == (64, 64, 3) and rgb.dtype == np.uint8
    lab = E.lab_of(img, 64, 64)
    want_cols, clipped = E.reveal(lab, E.R1)
    assert model.revealed_hint_colors.shape == (6, 2) and E.within_one_ulp(model.revealed_hint_colors, want_cols).all()
    hab, hm = model.net.hint_planes(0)
    want_ab, want_mask = E.planes(lab, E.R1, model.mask_mult)
    on = want_mask[0] > 0
    assert hm.tobytes() == want_mask.tobytes() and not hab[:, ~on].any() and E.within_one_ulp(hab[:, on], want_ab[:, on]).all()
    out_ab = model.output_ab_raw.copy()
    # net_forward with those planes on the host: the same network input, the same result
    ref32 = want_ab.astype(np.float32)
    planes = ref32 if hab.tobytes() == ref32.tobytes() else hab      # eval_ref's planes wherever the device rounded as numpy did
    rgb2 = model.net_forward(planes, hm / np.float32(model.mask_mult))
    np.testing.assert_array_equal(rgb2, rgb)
    np.testing.assert_array_equal(model.output_ab_raw, out_ab)
