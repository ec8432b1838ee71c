"""CPU checks of the pipelined batches of images of individual sizes (idc_forward_async_images / HipColorizer.forward_async_images /
colorize_images): the symbol in header, binding and library; the marshalling of the image table, the output pointers, the hint offsets,
the flags and the reference block over a recording library; colorize_images' grouping and slot order over a stub engine; and the arithmetic
of the size lists the GPU file uses (tests/ragged_ref.py), so that what is claimed for them there is shown here."""
import ctypes
import os
import re

import numpy as np
import pytest

import ragged_ref as R
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ ABI
def test_the_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "ideepcolor.h")).read()
    sym = "idc_forward_async_images"
    assert sym in set(re.findall(r"\b(idc_[a-z0-9_]+)\s*\(", header)) and sym in N.EXPORTED_SYMBOLS
    lib = N.load()
    assert hasattr(lib, sym)
    assert len(getattr(lib, sym).argtypes) == 14
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % sym, header).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == 14            # header and binding in step
    assert re.search(r"typedef struct idc_batch_refs \{ int32_t m; const idc_ref_image\* refs; const int32_t\* ref_index; const float\* centres;"
                     r"\s*float hist_flag; uint32_t flags; \} idc_batch_refs;", header)
    assert ctypes.sizeof(N.BatchRefs) == 40
    assert [getattr(N.BatchRefs, f).offset for f in ("m", "refs", "ref_index", "centres", "hist_flag", "flags")] == [0, 8, 16, 24, 32, 36]
    assert lib.idc_version() == 2                                  # additive: no bump


def test_a_call_without_a_handle_is_an_invalid_argument():
    lib = N.load()
    px, dst = np.zeros(3, np.uint8), np.zeros(3, np.uint8)
    one = (N.RefImage * 1)()
    one[0].rgb, one[0].h, one[0].w = px.ctypes.data, 1, 1
    outs = (ctypes.c_void_p * 1)(dst.ctypes.data)
    assert lib.idc_forward_async_images(None, 0, 1, one, None, None, 0, 1.0, 0.0, 50.0, 0, None, outs, None) == -1


# ------------------------------------------------------------------------------------------------ marshalling
class _Recorder(object):
    """Stands in for the ctypes library: records the call."""

    def __init__(self):
        self.calls = []

    def idc_forward_async_images(self, *a):
        # the table and the pointer array are the caller's until the call returns: read them now
        n = a[2]
        table = [(a[3][i].rgb, a[3][i].h, a[3][i].w) for i in range(n)]
        outs = [a[12][i] for i in range(n)]
        refs = a[11]._obj if a[11] is not None else None
        self.calls.append((a, table, outs, refs))
        return 0


class _Pool(object):
    def take(self, shape, dtype):
        return np.empty(shape, dtype)


def _engine_over(lib):
    e = engine.HipColorizer.__new__(engine.HipColorizer)
    e.lib, e._h, e.H, e.W, e._in_flight, e._pool, e.max_batch = lib, ctypes.c_void_p(1), 8, 16, {}, _Pool(), 8
    e.close = lambda: None
    return e


def _images():
    return [np.full((5, 7, 3), 1, np.uint8), np.full((1, 1, 3), 2, np.uint8), np.full((9, 4, 3), 3, np.uint8)]


def test_forward_async_images_marshals_table_outputs_offsets_and_flags():
    lib = _Recorder()
    e = _engine_over(lib)
    imgs = _images()
    hints = [[(0, 0, 1, 1, 1.0, 2.0)], None, [(1, 1, 2, 2, 3.0, 4.0), (2, 2, 3, 3, 5.0, 6.0)]]
    outs = [np.zeros((8, 16, 3), np.uint8) for _ in imgs]
    dab = np.zeros((3, 2, 8, 16), np.float32)
    got = e.forward_async_images(1, imgs, hints, outs, out_ab=dab, mode="rgb", mask_value=110.0, maskcent=0.5, l_cent=50.0)
    assert all(g is o for g, o in zip(got, outs))
    a, table, ptrs, refs = lib.calls[0]
    assert len(a) == 14 and (a[1], a[2], a[6], a[7], a[8], a[9], a[10]) == (1, 3, N.IDC_HINT_RGB, 110.0, 0.5, 50.0, 0)
    assert table == [(x.ctypes.data, x.shape[0], x.shape[1]) for x in imgs]
    assert ptrs == [o.ctypes.data for o in outs]
    assert np.ctypeslib.as_array(ctypes.cast(a[4], ctypes.POINTER(ctypes.c_int32)), (4,)).tolist() == [0, 1, 1, 3]
    assert refs is None and a[11] is None                          # no references: a NULL block
    assert a[13].value == dab.ctypes.data
    assert e._in_flight[1][0][0] is imgs[0] and e._in_flight[1][1][2] is outs[2] and e._in_flight[1][2] is dab
    # out='source': the flag, outputs of the images' own shapes; out_rgb=None: taken from the pool, returned, and kept until wait
    got = e.forward_async_images(0, imgs, None, out="source")
    a, table, ptrs, refs = lib.calls[1]
    assert a[10] == N.IDC_BATCH_OUT_SOURCE and a[4] is None and a[5] is None and a[13] is None
    assert [g.shape for g in got] == [x.shape for x in imgs] and all(g.dtype == np.uint8 and g.flags.c_contiguous for g in got)
    assert ptrs == [g.ctypes.data for g in got]
    assert all(x is y for x, y in zip(e._in_flight[0][1], got))
    for i, g in enumerate(got):                                    # slices of one block that do not overlap
        for o in got[i + 1:]:
            assert not np.shares_memory(g, o)


def test_forward_async_images_marshals_the_reference_block():
    lib = _Recorder()
    e = _engine_over(lib)
    imgs = _images()
    ref = np.full((9, 5, 3), 9, np.uint8)
    c = np.zeros((313, 2), np.float32)
    e.forward_async_images(0, imgs, None, out="source", refs=[ref], ref_index=[0, -1, 0], centres=c, hist_flag=2.0, saturation=True)
    refs = lib.calls[0][3]
    assert refs.m == 1 and (refs.refs[0].rgb, refs.refs[0].h, refs.refs[0].w) == (ref.ctypes.data, 9, 5)
    assert np.ctypeslib.as_array(ctypes.cast(refs.ref_index, ctypes.POINTER(ctypes.c_int32)), (3,)).tolist() == [0, -1, 0]
    assert refs.centres == c.ctypes.data and refs.hist_flag == 2.0 and refs.flags == N.IDC_REF_SATURATION
    with pytest.raises(ValueError):
        e.forward_async_images(0, imgs, None, refs=[ref], ref_index=[0], centres=c)         # n entries
    e.forward_async_images(1, imgs, None, refs=[])                                           # m = 0: a block, nothing in it
    refs = lib.calls[1][3]
    assert refs.m == 0 and not refs.refs and refs.ref_index is None and refs.centres is None and refs.flags == 0


def test_forward_async_images_refuses_malformed_arrays_before_the_library_sees_them():
    lib = _Recorder()
    e = _engine_over(lib)
    good = _images()
    net = lambda: [np.zeros((8, 16, 3), np.uint8) for _ in good]
    bad_sets = [
        [good[0].astype(np.float32)] + good[1:],                   # not uint8
        [good[0][:, ::2]] + good[1:],                              # not contiguous
        [good[0][..., 0]] + good[1:],                              # not (h,w,3)
        [np.zeros((2, 5, 7, 3), np.uint8)] + good[1:],             # a batch where an image belongs
    ]
    for bad in bad_sets:
        with pytest.raises(ValueError):
            e.forward_async_images(0, bad, None, net())
    with pytest.raises(ValueError):
        e.forward_async_images(0, good, None, [np.zeros(g.shape, np.uint8) for g in good])              # out='net' wants (H,W,3)
    with pytest.raises(ValueError):
        e.forward_async_images(0, good, None, net(), out="source")                                       # out='source' wants the image's shape
    with pytest.raises(ValueError):
        e.forward_async_images(0, good, None, net()[:2])                                                 # one output per image
    with pytest.raises(ValueError):
        e.forward_async_images(0, good, None, net(), out_ab=np.zeros((3, 2, 8, 16), np.float64))
    with pytest.raises(ValueError):
        e.forward_async_images(0, good, [None], net())                                                   # one hint list per image
    assert not lib.calls and not e._in_flight


# ------------------------------------------------------------------------------------------------ colorize_images on a stub
class _StubEngine(engine.HipColorizer):
    """colorize_images over recorded calls: 'the device' writes image[0,0,0] + 1 into the image's whole result when the slot is waited for."""

    def __init__(self, H, W, max_batch):
        self.H, self.W, self.max_batch = H, W, max_batch
        self._pool = _Pool()
        self.calls = []
        self.busy = {}

    def close(self):
        pass

    def forward_async_images(self, slot, images, hints, out_rgb=None, **kw):
        assert slot not in self.busy, "slot %d reused before its wait" % slot
        out = kw.get("out", "net")
        res = [np.zeros(a.shape if out == "source" else (self.H, self.W, 3), np.uint8) for a in images]
        self.calls.append(("run", slot, [tuple(a.shape) for a in images], list(hints), dict(kw)))
        self.busy[slot] = [(int(a[0, 0, 0]) + 1, r) for a, r in zip(images, res)]
        return res

    def wait(self, slot):
        self.calls.append(("wait", slot))
        for v, dst in self.busy.pop(slot, []):
            dst[...] = v


def _items(count):
    rs = np.random.RandomState(3)
    return [np.full((int(rs.randint(1, 9)), int(rs.randint(1, 9)), 3), k, np.uint8) for k in range(count)]


@pytest.mark.parametrize("count,batch", [(1, 4), (4, 4), (5, 4), (19, 8), (7, 1), (6, None)])
@pytest.mark.parametrize("out", ["net", "source"])
def test_colorize_images_groups_alternates_slots_and_keeps_the_order(count, batch, out):
    e = _StubEngine(8, 16, 5)
    if batch is not None and batch > 5:
        e.max_batch = 8
    imgs = _items(count)
    hint = [(0, 0, 1, 1, 1.0, 2.0)]
    items = [a if k % 3 == 0 else ((a, hint) if k % 3 == 1 else (a, None)) for k, a in enumerate(imgs)]   # the bare array and the tuple forms
    got = list(e.colorize_images(iter(items), batch=batch, out=out, mode="ab"))
    assert len(got) == count and not e.busy
    for k, res in enumerate(got):
        assert res.shape == (imgs[k].shape if out == "source" else (8, 16, 3)) and res.dtype == np.uint8
        assert (res == k + 1).all(), "result %d is not image %d's" % (k, k)
    for a, b in zip(got, got[1:]):                                  # the caller's own arrays
        assert not np.shares_memory(a, b)
    b = e.max_batch if batch is None else batch
    runs = [c for c in e.calls if c[0] == "run"]
    want = [count - j if count - j < b else b for j in range(0, count, b)]
    assert [len(c[2]) for c in runs] == want                        # batches of `batch`, the last one shorter
    assert [c[1] for c in runs] == [j & 1 for j in range(len(runs))]
    assert [s for c in runs for s in c[2]] == [a.shape for a in imgs]
    assert [h for c in runs for h in c[3]] == [hint if k % 3 == 1 else None for k in range(count)]
    assert all(c[4] == {"out": out, "mode": "ab"} for c in runs)   # no item had a reference: the plain call
    assert [c[1] for c in e.calls if c[0] == "wait"] == [j & 1 for j in range(len(runs))]
    for j in range(2, len(runs)):                                   # a wait between two uses of a slot
        assert ("wait", j & 1) in e.calls[e.calls.index(runs[j - 2]) + 1:e.calls.index(runs[j])]


def test_colorize_images_dedupes_references_per_batch():
    e = _StubEngine(8, 16, 3)
    imgs = _items(5)
    shared, other = np.zeros((9, 5, 3), np.uint8), np.zeros((2, 7, 3), np.uint8)
    c = np.zeros((313, 2), np.float32)
    items = [(imgs[0], None, shared), (imgs[1], None, None), (imgs[2], None, shared), (imgs[3], None, other), imgs[4]]
    got = list(e.colorize_images(iter(items), batch=3, centres=c, saturation=True))
    assert [g.shape for g in got] == [a.shape for a in imgs]        # out defaults to 'source'
    kw = [x[4] for x in e.calls if x[0] == "run"]
    assert [id(r) for r in kw[0]["refs"]] == [id(shared)] and kw[0]["ref_index"].tolist() == [0, -1, 0]
    assert [id(r) for r in kw[1]["refs"]] == [id(other)] and kw[1]["ref_index"].tolist() == [0, -1]
    assert all(k["centres"] is c and k["saturation"] is True and k["out"] == "source" for k in kw)


def test_colorize_images_waits_for_both_slots_when_the_consumer_stops():
    e = _StubEngine(8, 8, 2)
    gen = e.colorize_images((np.zeros((3, 4, 3), np.uint8) for _ in range(9)), batch=2)
    next(gen)                                                       # slot 0 was waited for to deliver batch 0; batch 1 is in flight on slot 1
    assert sorted(e.busy) == [1]
    gen.close()
    assert not e.busy and [c[1] for c in e.calls if c[0] == "wait"] == [0, 1]
    gen = e.colorize_images((np.zeros((3, 4, 3), np.uint8) for _ in range(9)), batch=2)
    for _ in range(3):                                              # batch 0 delivered and batch 2 enqueued on its slot: a result of batch 1 in hand
        next(gen)
    assert sorted(e.busy) == [0]
    e.calls[:] = []
    gen.close()
    assert not e.busy and ("wait", 0) in e.calls
    with pytest.raises(ValueError):
        list(e.colorize_images([np.zeros((3, 4, 3), np.uint8)], batch=3))                  # more than max_batch
    with pytest.raises(ValueError):
        list(e.colorize_images([np.zeros((1, 3, 4, 3), np.uint8)]))                        # a batch where an image belongs


# ------------------------------------------------------------------------------------------------ the GPU file's size lists
def test_image_starts_cover_all_four_residues():
    seen = set()
    for H, W in ((64, 64), (40, 72)):
        for order in (R.MIXED, R.MIXED[::-1]):
            at = R.starts(R.sizes(order, H, W))
            assert at[-1] == sum(h * w * 3 for h, w in R.sizes(order, H, W))
            seen |= set(int(x) % 4 for x in at[:-1])
        fwd = set(int(x) % 4 for x in R.starts(R.sizes(R.MIXED, H, W))[:-1])
        rev = set(int(x) % 4 for x in R.starts(R.sizes(R.MIXED[::-1], H, W))[:-1])
        assert fwd | rev == {0, 1, 2, 3} and rev - fwd, (fwd, rev)  # the reversed order adds residues the forward order does not have
    assert seen == {0, 1, 2, 3}


def test_the_span_cases_have_the_structure_claimed_for_them():
    full, tail = R.groups(R.FOUR_IN_ONE)
    assert full[0].tolist() == [0, 1, 2, 3]                         # four images in the first group
    assert all(len(set(g)) == 1 for g in full[1:].tolist())
    full, tail = R.groups(R.TAIL_IMAGE)
    assert sum(h * w for h, w in R.TAIL_IMAGE) == 37 and len(full) == 9
    assert full[-1].tolist() == [0, 0, 0, 1] and tail.tolist() == [2]                      # the byte-access tail is the last 1 x 1 image
    full, tail = R.groups(R.THREE_BOUNDARIES)
    # images start at pixels 0, 6, 8, 9 and 12: group 1 carries once, group 2 (pixels 8..11) has three boundaries -- it begins on the start
    # of image 2, carries into image 3 after one pixel, and uses image 3 up exactly at its end, where image 4 begins
    assert (np.cumsum([0] + [h * w for h, w in R.THREE_BOUNDARIES])[:-1] == [0, 6, 8, 9, 12]).all()
    assert full[:4].tolist() == [[0, 0, 0, 0], [0, 0, 1, 1], [2, 3, 3, 3], [4, 4, 4, 4]]
    first_big = 3
    assert (full[first_big:] == 4).all() and len(full) - first_big > 3 * 256              # then more than three workgroups of one image
    assert tail.size == (12 + 203 * 187) % 4


def test_the_mixed_batch_has_groups_across_every_boundary_kind():
    for H, W in ((64, 64), (40, 72)):
        for order in (R.MIXED, R.MIXED[::-1]):
            sz = R.sizes(order, H, W)
            full, tail = R.groups(sz)
            assert full.shape[0] * 4 + tail.size == sum(h * w for h, w in sz)
            assert max(len(set(g)) for g in full.tolist()) >= 2     # some group straddles two images
