"""CPU checks of the evaluation batches (idc_reveal_hints / idc_forward_async_eval; HipColorizer.reveal_hints / forward_async_eval /
evaluate_images; interactive_deep_colorization_amd/evaluate.py): the ABI, the marshalling on a recording library, evaluate_images on a stub
engine, the PSNR expression, the simulated user, and that the float32 a rectangle reveals does not depend on the order its float64 values are
summed in for the images and rectangle lists of tests/test_eval_gpu.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import eval_ref as E
import ragged_ref as R
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import engine, evaluate

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ ABI
def test_the_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "ideepcolor.h")).read()
    declared = set(re.findall(r"\b(idc_[a-z0-9_]+)\s*\(", header))
    lib = N.load()
    for sym, argc in (("idc_reveal_hints", 6), ("idc_forward_async_eval", 16)):
        assert sym in declared and sym in N.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
        assert len(getattr(lib, sym).argtypes) == argc
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % sym, header).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == argc       # header and binding in step
    assert re.search(r"enum \{ IDC_HINT_REVEAL = 2 \};", header) and N.IDC_HINT_REVEAL == 2
    assert lib.idc_version() == 2                                  # additive: no bump


def test_a_call_without_a_handle_is_an_invalid_argument():
    lib = N.load()
    px, sse = np.zeros(3, np.uint8), np.zeros(3, np.uint64)
    one = (N.RefImage * 1)()
    one[0].rgb, one[0].h, one[0].w = px.ctypes.data, 1, 1
    assert lib.idc_forward_async_eval(None, 0, 1, one, None, None, 2, 1.0, 0.0, 50.0, 0, None, None, None, sse.ctypes.data, None) == -1
    assert lib.idc_reveal_hints(None, 0, 0, None, 1.0, None) == -1


# ------------------------------------------------------------------------------------------------ marshalling
class _Recorder(object):
    def __init__(self):
        self.calls = []

    def idc_forward_async_eval(self, *a):
        n = a[2]
        table = [(a[3][i].rgb, a[3][i].h, a[3][i].w) for i in range(n)]
        outs = [a[12][i] for i in range(n)] if a[12] is not None else None
        total = int(np.ctypeslib.as_array(ctypes.cast(a[4], ctypes.POINTER(ctypes.c_int32)), (n + 1,))[n]) if a[4] is not None else 0
        rows = ctypes.cast(a[5], ctypes.POINTER(N.Hint)) if a[5] is not None else None
        hints = [(rows[k].y0, rows[k].x0, rows[k].y1, rows[k].x1, rows[k].c0, rows[k].c1, rows[k].c2) for k in range(total)]
        self.calls.append((a, table, outs, hints))
        return 0

    def idc_reveal_hints(self, *a):
        self.calls.append((a, [(a[3][k].y0, a[3][k].x0, a[3][k].y1, a[3][k].x1) for k in range(a[2])]))
        ctypes.cast(a[5], ctypes.POINTER(ctypes.c_float))[0] = 5.0
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


def test_forward_async_eval_marshals_the_sixteen_arguments():
    lib = _Recorder()
    e = _engine_over(lib)
    imgs = _images()
    rects = [[(0, 0, 1, 1)], None, [(1, 1, 2, 2, 9.0, 9.0), (2, 2, 3, 3)]]       # colours given to a reveal call are dropped
    dab = np.zeros((3, 2, 8, 16), np.float32)
    sse, cols, outs = e.forward_async_eval(1, imgs, rects, out_ab=dab, mask_value=110.0, maskcent=0.5, l_cent=50.0)
    a, table, ptrs, hints = lib.calls[0]
    assert len(a) == 16 and (a[1], a[2], a[6], a[7], a[8], a[9], a[10]) == (1, 3, N.IDC_HINT_REVEAL, 110.0, 0.5, 50.0, 0)
    assert table == [(x.ctypes.data, x.shape[0], x.shape[1]) for x in imgs]
    assert np.ctypeslib.as_array(ctypes.cast(a[4], ctypes.POINTER(ctypes.c_int32)), (4,)).tolist() == [0, 1, 1, 3]
    assert hints == [(0, 0, 1, 1, 0.0, 0.0, 0.0), (1, 1, 2, 2, 0.0, 0.0, 0.0), (2, 2, 3, 3, 0.0, 0.0, 0.0)]
    assert a[11] is None and a[12] is None and ptrs is None and outs is None       # NULL rgb_out: no image leaves the device
    assert a[13].value == dab.ctypes.data
    assert sse.shape == (3, 3) and sse.dtype == np.uint64 and a[14].value == sse.ctypes.data
    assert cols.shape == (3, 2) and cols.dtype == np.float32 and a[15].value == cols.ctypes.data
    held = e._in_flight[1]
    assert held[0][0] is imgs[0] and held[1] is None and held[2] is dab and held[3] is sse and held[4] is cols
    # a given list: its mode, no hint_colours; images asked for: from the pool at the images' own sizes
    given = [[(0, 0, 1, 1, 1.0, 2.0)], None, None]
    sse, cols, outs = e.forward_async_eval(0, imgs, given, mode="ab", out="source", want_rgb=True)
    a, table, ptrs, hints = lib.calls[1]
    assert a[6] == N.IDC_HINT_AB and a[10] == N.IDC_BATCH_OUT_SOURCE and a[15] is None and cols is None
    assert hints == [(0, 0, 1, 1, 1.0, 2.0, 0.0)]
    assert [o.shape for o in outs] == [x.shape for x in imgs] and ptrs == [o.ctypes.data for o in outs]
    assert all(x is y for x, y in zip(e._in_flight[0][1], outs))
    # the caller's own output arrays; no hints at all
    mine = [np.zeros((8, 16, 3), np.uint8) for _ in imgs]
    sse, cols, outs = e.forward_async_eval(0, imgs, None, out_rgb=mine, mode="rgb")
    a, table, ptrs, hints = lib.calls[2]
    assert a[6] == N.IDC_HINT_RGB and a[4] is None and a[5] is None and ptrs == [o.ctypes.data for o in mine] and all(x is y for x, y in zip(outs, mine))
    sse, cols, outs = e.forward_async_eval(0, imgs, None)
    assert lib.calls[3][0][15] is None and cols.shape == (0, 2)


def test_forward_async_eval_validates_as_forward_async_images_does():
    lib = _Recorder()
    e = _engine_over(lib)
    good = _images()
    for bad in ([good[0].astype(np.float32)] + good[1:], [good[0][:, ::2]] + good[1:], [good[0][..., 0]] + good[1:]):
        with pytest.raises(ValueError):
            e.forward_async_eval(0, bad, None)
    with pytest.raises(ValueError):
        e.forward_async_eval(0, good, None, out_rgb=[np.zeros(g.shape, np.uint8) for g in good])        # out='net' wants (H,W,3)
    with pytest.raises(ValueError):
        e.forward_async_eval(0, good, None, out_ab=np.zeros((3, 2, 8, 16), np.float64))
    with pytest.raises(ValueError):
        e.forward_async_eval(0, good, [None])                                                          # one list per image
    with pytest.raises(KeyError):
        e.forward_async_eval(0, good, None, mode="mean")
    with pytest.raises(KeyError):
        e.forward_async_images(0, good, None, mode="reveal")                                           # the older call has no such mode
    assert not lib.calls and not e._in_flight


def test_reveal_hints_marshals_rectangles_and_returns_the_colours():
    lib = _Recorder()
    e = _engine_over(lib)
    cols = e.reveal_hints([(1, 2, 3, 4), (5, 6, 7, 8, 1.0, 2.0)], img=2, mask_value=110.0)
    a, rects = lib.calls[0]
    assert (a[1], a[2], a[4]) == (2, 2, 110.0) and rects == [(1, 2, 3, 4), (5, 6, 7, 8)]
    assert cols.shape == (2, 2) and cols.dtype == np.float32 and cols[0, 0] == 5.0


# ------------------------------------------------------------------------------------------------ evaluate_images on a stub
class _StubEngine(engine.HipColorizer):
    """evaluate_images over recorded calls: 'the device' writes (v, 2v, 3v), v = image[0,0,0], into the image's sse when the slot is waited for."""

    def __init__(self, H, W, max_batch):
        self.H, self.W, self.max_batch = H, W, max_batch
        self._pool = _Pool()
        self.calls = []
        self.busy = {}

    def close(self):
        pass

    def forward_async_eval(self, slot, images, hints, **kw):
        assert slot not in self.busy, "slot %d reused before its wait" % slot
        sse = np.zeros((len(images), 3), np.uint64)
        self.calls.append(("run", slot, [tuple(a.shape) for a in images], list(hints), dict(kw)))
        self.busy[slot] = (sse, [int(a[0, 0, 0]) for a in images])
        return sse, None, None

    def wait(self, slot):
        self.calls.append(("wait", slot))
        if slot in self.busy:
            sse, vals = self.busy.pop(slot)
            sse[...] = np.array([[v, 2 * v, 3 * v] for v in vals], np.uint64)


def _items(count):
    rs = np.random.RandomState(3)
    return [np.full((int(rs.randint(1, 9)), int(rs.randint(1, 9)), 3), k, np.uint8) for k in range(count)]


@pytest.mark.parametrize("count,batch", [(1, 4), (4, 4), (5, 4), (19, 8), (7, 1), (6, None)])
@pytest.mark.parametrize("out", ["net", "source"])
def test_evaluate_images_groups_alternates_slots_and_keeps_the_order(count, batch, out):
    e = _StubEngine(8, 16, 5)
    if batch is not None and batch > 5:
        e.max_batch = 8
    imgs = _items(count)
    rect = [(0, 0, 1, 1)]
    items = [a if k % 3 == 0 else ((a, rect) if k % 3 == 1 else (a, None)) for k, a in enumerate(imgs)]
    got = list(e.evaluate_images(iter(items), batch=batch, out=out))
    assert len(got) == count and not e.busy
    for k, (psnr, sse) in enumerate(got):
        assert sse.tolist() == [k, 2 * k, 3 * k], "result %d is not image %d's" % (k, k)
        h, w = imgs[k].shape[:2] if out == "source" else (8, 16)
        assert psnr == (math.inf if k == 0 else 20 * math.log10(255.0 / math.sqrt(6.0 * k / (3 * h * w))))
    b = e.max_batch if batch is None else batch
    runs = [c for c in e.calls if c[0] == "run"]
    assert [len(c[2]) for c in runs] == [count - j if count - j < b else b for j in range(0, count, b)]
    assert [c[1] for c in runs] == [j & 1 for j in range(len(runs))]
    assert [s for c in runs for s in c[2]] == [a.shape for a in imgs]
    assert [h for c in runs for h in c[3]] == [rect if k % 3 == 1 else None for k in range(count)]
    assert all(c[4] == {"out": out, "mode": "reveal", "want_rgb": False} for c in runs)
    assert [c[1] for c in e.calls if c[0] == "wait"] == [j & 1 for j in range(len(runs))]
    for j in range(2, len(runs)):                                   # a wait between two uses of a slot
        assert ("wait", j & 1) in e.calls[e.calls.index(runs[j - 2]) + 1:e.calls.index(runs[j])]


def test_evaluate_images_waits_for_both_slots_when_the_consumer_stops_early():
    e = _StubEngine(8, 16, 2)
    gen = e.evaluate_images(iter(_items(9)), batch=2)
    next(gen)                                                       # batches 0 and 1 were submitted; batch 0 was waited for
    assert sorted(e.busy) == [1]
    gen.close()
    assert not e.busy

    def broken():                                                   # the stream fails with both slots in flight
        for a in _items(5):
            yield a
        raise IOError("no more images")

    e = _StubEngine(8, 16, 2)
    with pytest.raises(IOError):
        list(e.evaluate_images(broken(), batch=2))
    assert not e.busy
    assert [c for c in e.calls if c[0] == "wait"] == [("wait", 0), ("wait", 1)]
    with pytest.raises(ValueError):
        list(e.evaluate_images(iter(_items(1)), batch=3))           # batch beyond max_batch
    with pytest.raises(ValueError):
        list(e.evaluate_images(iter([np.zeros((2, 2), np.uint8)])))


# ------------------------------------------------------------------------------------------------ the metric
def test_psnr_from_sse_is_get_result_psnr():
    rs = np.random.RandomState(5)
    for k, (h, w) in enumerate([(1, 1), (5, 7), (64, 64), (40, 72), (203, 187)]):
        truth = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        result = rs.randint(0, 256, (h, w, 3)).astype(np.uint8) if k % 2 == 0 else (truth ^ (rs.randint(0, 40, (h, w, 3)) == 0)).astype(np.uint8)
        sse = E.sse(result, truth)
        want = E.psnr(result, truth)
        got = evaluate.psnr_from_sse(np.array(sse, np.uint64), h, w)
        assert abs(got - want) <= 1e-12 * abs(want), (h, w, got, want)
        assert evaluate.psnr_from_sse(sum(sse), h, w) == got
    assert evaluate.psnr_from_sse(np.zeros(3, np.uint64), 5, 7) == math.inf
    # sums beyond 2^53 and beyond 2^63 are added as integers
    big = np.array([2 ** 63, 2 ** 62, 5], np.uint64)
    assert evaluate.psnr_from_sse(big, 16384, 16384) == 20 * math.log10(255.0 / math.sqrt(float(2 ** 63 + 2 ** 62 + 5) / (3 * 16384 * 16384)))


# ------------------------------------------------------------------------------------------------ the simulated user
def test_simulate_points_is_deterministic_inside_and_prefix_closed():
    for H, W in ((64, 64), (40, 72), (256, 256)):
        a = evaluate.simulate_points(H, W, 100, np.random.RandomState(7))
        b = evaluate.simulate_points(H, W, 100, np.random.RandomState(7))
        c = evaluate.simulate_points(H, W, 100, np.random.RandomState(8))
        assert a.shape == (100, 4) and a.dtype == np.int32
        np.testing.assert_array_equal(a, b)
        assert (a != c).any()
        side_y, side_x = a[:, 2] - a[:, 0] + 1, a[:, 3] - a[:, 1] + 1
        np.testing.assert_array_equal(side_y, side_x)
        assert side_y.min() >= 1 and side_y.max() <= 9 and len(set(side_y.tolist())) == 9
        cy, cx = a[:, 0] + side_y // 2, a[:, 1] + side_x // 2      # the centre the patch was drawn around
        assert (cy >= 0).all() and (cy < H).all() and (cx >= 0).all() and (cx < W).all()
        odd = side_y % 2 == 1                                       # put_point's extent [c - p, c + p]
        np.testing.assert_array_equal(a[odd, 2] - cy[odd], cy[odd] - a[odd, 0])
        for count in (0, 1, 2, 5, 10, 20, 50):
            np.testing.assert_array_equal(evaluate.simulate_points(H, W, count, np.random.RandomState(7)), a[:count])
        # spread: sigma = (H/4, W/4) around the centre
        assert abs(cy.mean() - H / 2.0) < H / 8.0 and abs(cx.mean() - W / 2.0) < W / 8.0


class _SweepEngine(object):
    H, W = 64, 64

    def __init__(self):
        self.seen = []

    def evaluate_images(self, items, batch=None, out="net", mode="reveal"):
        items = list(items)
        self.seen.append([np.asarray(r) for _, r in items])
        for _, r in items:
            yield float(len(r)), np.zeros(3, np.uint64)


def test_psnr_sweep_uses_prefixes_of_one_point_list_per_image():
    e = _SweepEngine()
    imgs = [np.zeros((5, 7, 3), np.uint8), np.zeros((9, 4, 3), np.uint8)]
    counts = (0, 1, 5, 20)
    table = evaluate.psnr_sweep(e, imgs, counts=counts, seed=3)
    assert table.shape == (4, 2) and table.dtype == np.float64
    np.testing.assert_array_equal(table, np.array(counts, np.float64)[:, None] * np.ones((1, 2)))
    for j in range(2):
        full = evaluate.simulate_points(64, 64, 20, np.random.RandomState(3 + j))
        for r, c in enumerate(counts):
            np.testing.assert_array_equal(e.seen[r][j], full[:c])
    assert (e.seen[3][0] != e.seen[3][1]).any()                     # each image has its own points


# ------------------------------------------------------------------------------------------------ summation order
def test_the_revealed_float32_does_not_depend_on_the_summation_order():
    """Row-major summation, math.fsum and ndarray.mean (pairwise) give the same float32 for every rectangle of the GPU file's cases, so the
    kernel's own fixed order -- any order: float64 errors lie far below a float32 ulp -- can be held to that float32 and its neighbours."""
    cases = 0
    for H, W in ((64, 64), (40, 72)):
        for j, (sh, sw) in enumerate(R.sizes(R.MIXED, H, W)):
            lab = E.lab_of(R.image(sh, sw, 400 + j), H, W)
            for rects in (E.R1, E.R2, E.R3):
                for r in rects:
                    c = E.clip(r, H, W)
                    if c is None:
                        continue
                    for vals in E.rect_values(lab, c):
                        a = np.float32(E.mean_row_major(vals))
                        assert a == np.float32(math.fsum(vals) / len(vals)) == np.float32(np.array(vals).mean())
                        cases += 1
    assert cases == 322
