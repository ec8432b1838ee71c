"""Reference-image global hints, the parts that need no GPU: the knife-edge condition of tests/glob_ref.py for every array the GPU tests
use, glob_ref.py itself against the oracle's global_stats, the three C-ABI symbols in header, binding and library, the de-duplication of
references by object identity and colorize_stream's slot order with three-entry items on a stub engine, and that ``refs=None`` makes the
call it made before."""
import ctypes
import os
import re

import numpy as np
import pytest

import glob_ref
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import engine
from oracle import colorspace as ocs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the inputs are no knife edges
@pytest.mark.parametrize("k", range(len(glob_ref.SIZES)), ids=lambda k: "%dx%d" % glob_ref.SIZES[k][:2])
def test_margin_of_the_net_size_inputs(k):
    H, W = glob_ref.NET
    s = glob_ref.stats_of("net", k, H, W)
    print("reference %s at %dx%d: margin %.4g, %d bins, s_avg %.6f" % (glob_ref.SIZES[k], H, W, s["margin"], s["bins"], s["s_avg"]))
    assert s["margin"] >= glob_ref.MARGIN
    assert s["counts"].sum() == (H // 4) * (W // 4)
    if glob_ref.SIZES[k][:2] != (1, 1):
        assert s["bins"] >= 10                                    # not one grey bin


@pytest.mark.parametrize("k", range(len(glob_ref.SIZES64)), ids=lambda k: "%dx%d" % glob_ref.SIZES64[k][:2])
def test_margin_of_the_64x64_inputs(k):
    s = glob_ref.stats_of("64", k, 64, 64)
    print("reference %s at 64x64: margin %.4g, %d bins" % (glob_ref.SIZES64[k], s["margin"], s["bins"]))
    assert s["margin"] >= glob_ref.MARGIN and s["bins"] >= 10 and s["counts"].sum() == 256


def test_the_inputs_are_what_the_issue_asks_for():
    refs = glob_ref.refs_net()
    assert [r.shape for r in refs] == [(h, w, 3) for h, w, _ in glob_ref.SIZES] and all(r.dtype == np.uint8 for r in refs)
    assert sorted(r.shape[:2] for r in refs) == sorted([(32, 48), (20, 27), (33, 49), (97, 61), (131, 200), (7, 300), (1, 1)])
    kinds = [s % 2 for _, _, s in glob_ref.SIZES]
    assert 0 in kinds and 1 in kinds                              # noise and ramps
    assert glob_ref.centres().shape == (313, 2) and glob_ref.centres().dtype == np.float32


# ------------------------------------------------------------------------------------------------ the reference against the oracle
@pytest.mark.parametrize("k", [0, 1])
def test_reference_equals_the_oracle_on_a_net_size_image(k):
    """On a net-size image the resize is the identity and glob_ref.stats must count what oracle.colorspace.global_stats counts (which
    rounds the pooled values to fp32 as Caffe does: the margin makes that immaterial)."""
    src = glob_ref.make_ref(32, 48, (2, 3)[k])
    s = glob_ref.stats(src, 32, 48)
    assert s["margin"] >= glob_ref.MARGIN
    hist, s_avg = ocs.global_stats(src, glob_ref.centres())
    np.testing.assert_array_equal(np.rint(hist.astype(np.float64) * 96).astype(np.int64), s["counts"])
    np.testing.assert_array_equal(hist, s["hist"])
    assert abs(s_avg - s["s_avg"]) <= 1e-12


def test_glob_rows_builds_the_host_rows():
    hists = np.arange(2 * 313, dtype=np.float32).reshape(2, 313)
    g, s = glob_ref.glob_rows(hists, [1, -1, 0], s_avg=[0.25, 0.5])
    assert g.shape == (3, 314) and s.shape == (3, 2)
    np.testing.assert_array_equal(g[0, :313], hists[1]); assert g[0, 313] == 1.0
    assert not g[1].any() and not s[1].any()
    np.testing.assert_array_equal(s[[0, 2]], [[0.5, 1.0], [0.25, 1.0]])
    assert glob_ref.glob_rows(hists, [0]).shape == (1, 314)


# ------------------------------------------------------------------------------------------------ ABI
NEW = {"idc_global_stats_rgb": 6, "idc_set_global_refs": 9, "idc_forward_async_rgb_ref": 21}


def test_abi_declares_binds_and_exports_the_three_symbols():
    header = open(os.path.join(REPO, "include", "ideepcolor.h")).read()
    declared = set(re.findall(r"\b(idc_[a-z0-9_]+)\s*\(", header))
    lib = N.load()
    for sym, nargs in NEW.items():
        assert sym in declared and sym in N.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
        assert len(getattr(lib, sym).argtypes) == nargs, sym
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % sym, header).group(1)
        assert len(decl.split(",")) == nargs, (sym, decl)          # header and binding in step
    assert re.search(r"\bIDC_REF_SATURATION\s*=\s*1\b", header) and N.IDC_REF_SATURATION == 1
    assert re.search(r"#define\s+IDC_REF_MAX\s+4096\b", header) and N.IDC_REF_MAX == 4096
    assert re.search(r"typedef struct idc_ref_image \{ const uint8_t\* rgb; int32_t h, w; \} idc_ref_image;", header)
    assert ctypes.sizeof(N.RefImage) == 16 and N.RefImage.h.offset == 8 and N.RefImage.w.offset == 12
    assert lib.idc_version() == 2                                  # additive: no bump
    px = np.zeros(3, np.uint8)
    one = (N.RefImage * 1)()
    one[0].rgb, one[0].h, one[0].w = px.ctypes.data, 1, 1
    c = glob_ref.centres()
    fp = ctypes.POINTER(ctypes.c_float)
    hist = np.zeros(313, np.float32)
    assert lib.idc_global_stats_rgb(None, 1, one, c.ctypes.data_as(fp), hist.ctypes.data_as(fp), None) == -1
    assert lib.idc_set_global_refs(None, 0, 1, 1, one, None, c.ctypes.data_as(fp), 1.0, 0) == -1
    assert lib.idc_forward_async_rgb_ref(None, 0, 1, 1, 1, px.ctypes.data, None, None, 0, 1.0, 0.0, 50.0, 0, 1, one, None,
                                         c.ctypes.data_as(fp), 1.0, 0, px.ctypes.data, None) < 0


# ------------------------------------------------------------------------------------------------ Python plumbing
def test_references_are_deduplicated_by_object_identity():
    a, b = glob_ref.noise(3, 4, 1), glob_ref.noise(5, 2, 2)
    twin = a.copy()                                                # equal content, another object: uploaded on its own
    uniq, idx = engine.dedupe_refs([a, None, b, a, twin, b], 6)
    assert [id(u) for u in uniq] == [id(a), id(b), id(twin)]
    assert idx.dtype == np.int32 and idx.tolist() == [0, -1, 1, 0, 2, 1]
    uniq, idx = engine.dedupe_refs([None, None], 2)
    assert uniq == [] and idx.tolist() == [-1, -1]
    with pytest.raises(ValueError):
        engine.dedupe_refs([a], 2)


def test_ref_images_describes_each_array():
    a, b = glob_ref.noise(3, 4, 1), glob_ref.noise(5, 2, 2)[:, ::-1]              # the second is not contiguous: a copy is described
    arr, keep = engine.ref_images([a, b])
    assert len(arr) == 2 and (arr[0].h, arr[0].w, arr[1].h, arr[1].w) == (3, 4, 5, 2)
    assert arr[0].rgb == a.ctypes.data and arr[1].rgb == keep[1].ctypes.data and keep[1].flags.c_contiguous
    np.testing.assert_array_equal(keep[1], b)
    arr, keep = engine.ref_images([])
    assert keep == [] and len(arr) == 1                            # never a zero-length ctypes array
    for bad in (np.zeros((3, 4), np.uint8), np.zeros((3, 4, 4), np.uint8), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            engine.ref_images([bad])


class _Pool(object):
    def take(self, shape, dtype):
        return np.empty(shape, dtype)


class _StubEngine(engine.HipColorizer):
    """The stub of test_batch_rgb_cpu.py, restated: colorize_stream over recorded calls; 'the device' writes batch[0,0,0,0] + 1 into the
    whole result when the slot is waited for."""

    def __init__(self, H, W):
        self.H, self.W = H, W
        self._pool = _Pool()
        self.calls = []
        self.busy = {}

    def close(self):
        pass

    def forward_async_rgb(self, slot, rgb, hints, out_rgb, out_ab=None, **kw):
        assert slot not in self.busy, "slot %d reused before its wait" % slot
        self.calls.append(("run", slot, tuple(rgb.shape), hints, dict(kw)))
        self.busy[slot] = (int(rgb[0, 0, 0, 0]) + 1, out_rgb)

    def wait(self, slot):
        self.calls.append(("wait", slot))
        if slot in self.busy:
            v, dst = self.busy.pop(slot)
            dst[...] = v


def test_colorize_stream_with_three_entry_items_on_the_stub():
    e = _StubEngine(8, 16)
    c = glob_ref.centres()
    shared, other = glob_ref.noise(9, 5, 3), glob_ref.noise(2, 7, 4)
    items = [
        (np.full((3, 5, 7, 3), 0, np.uint8), None, [shared, shared, shared]),            # one object for the whole item: uploaded once
        (np.full((2, 4, 4, 3), 10, np.uint8), [[(0, 0, 1, 1, 1.0, 2.0)], None]),          # a two-entry item in between: the plain call
        (np.full((4, 6, 3, 3), 20, np.uint8), None, [other, None, shared, other]),
        (np.full((1, 8, 16, 3), 30, np.uint8), None, [None]),                              # nobody has a reference
    ]
    got = list(e.colorize_stream(iter(items), out="net", centres=c, saturation=True))
    assert len(got) == 4
    for k, res in enumerate(got):
        assert res.shape == (items[k][0].shape[0], 8, 16, 3) and (res == 10 * k + 1).all(), "result %d is not item %d's" % (k, k)
    runs = [x for x in e.calls if x[0] == "run"]
    assert [x[1] for x in runs] == [0, 1, 0, 1]                                            # slot order
    assert [x[1] for x in e.calls if x[0] == "wait"] == [0, 1, 0, 1]
    kw = [x[4] for x in runs]
    assert [id(r) for r in kw[0]["refs"]] == [id(shared)] and kw[0]["ref_index"].tolist() == [0, 0, 0]
    assert "refs" not in kw[1] and "ref_index" not in kw[1] and kw[1]["out"] == "net"
    assert [id(r) for r in kw[2]["refs"]] == [id(other), id(shared)] and kw[2]["ref_index"].tolist() == [0, -1, 1, 0]
    assert kw[3]["refs"] == [] and kw[3]["ref_index"].tolist() == [-1]
    for k in (0, 2, 3):
        assert kw[k]["centres"] is c and kw[k]["saturation"] is True and kw[k]["out"] == "net"
    with pytest.raises(ValueError):                                                         # n entries, no fewer
        list(e.colorize_stream(iter([(np.zeros((2, 4, 4, 3), np.uint8), None, [shared])]), centres=c))


class _Recorder(object):
    """Stands in for the ctypes library: records which entry point was called with what."""

    def __init__(self):
        self.calls = []

    def idc_forward_async_rgb(self, *a):
        self.calls.append(("idc_forward_async_rgb", a))
        return 0

    def idc_forward_async_rgb_ref(self, *a):
        self.calls.append(("idc_forward_async_rgb_ref", a))
        return 0


def _engine_over(lib):
    e = engine.HipColorizer.__new__(engine.HipColorizer)
    e.lib, e._h, e.H, e.W, e._in_flight = lib, ctypes.c_void_p(1), 8, 16, {}
    e.close = lambda: None
    return e


def test_refs_none_makes_the_old_ctypes_call():
    lib = _Recorder()
    e = _engine_over(lib)
    rgb, dst = np.zeros((2, 5, 7, 3), np.uint8), np.zeros((2, 8, 16, 3), np.uint8)
    hints = [[(0, 0, 1, 1, 1.0, 2.0)], None]
    e.forward_async_rgb(1, rgb, hints, dst, mode="ab", mask_value=110.0, maskcent=0.5, l_cent=50.0)
    e.forward_async_rgb(0, rgb, hints, dst, mode="ab", mask_value=110.0, maskcent=0.5, l_cent=50.0, refs=None, ref_index=[0, 0],
                        centres=glob_ref.centres(), hist_flag=3.0, saturation=True)        # without refs the rest is not looked at
    assert [c[0] for c in lib.calls] == ["idc_forward_async_rgb"] * 2
    a = lib.calls[0][1]
    assert len(a) == 15
    assert (a[1], a[2], a[3], a[4], a[8], a[9], a[10], a[11], a[12]) == (1, 2, 5, 7, N.IDC_HINT_AB, 110.0, 0.5, 50.0, 0)
    assert a[5].value == rgb.ctypes.data and a[13].value == dst.ctypes.data and a[14] is None
    assert np.ctypeslib.as_array(ctypes.cast(a[6], ctypes.POINTER(ctypes.c_int32)), (3,)).tolist() == [0, 1, 1]
    assert 1 in e._in_flight and 0 in e._in_flight


def test_refs_make_the_new_ctypes_call():
    lib = _Recorder()
    e = _engine_over(lib)
    rgb, dst = np.zeros((2, 5, 7, 3), np.uint8), np.zeros((2, 5, 7, 3), np.uint8)
    ref = glob_ref.noise(9, 5, 3)
    c = glob_ref.centres()
    e.forward_async_rgb(0, rgb, None, dst, out="source", refs=[ref], ref_index=[0, -1], centres=c, hist_flag=2.0, saturation=True)
    name, a = lib.calls[0]
    assert name == "idc_forward_async_rgb_ref" and len(a) == 21
    assert a[12] == N.IDC_BATCH_OUT_SOURCE and a[13] == 1 and (a[14][0].h, a[14][0].w, a[14][0].rgb) == (9, 5, ref.ctypes.data)
    assert np.ctypeslib.as_array(ctypes.cast(a[15], ctypes.POINTER(ctypes.c_int32)), (2,)).tolist() == [0, -1]
    assert ctypes.cast(a[16], ctypes.c_void_p).value == c.ctypes.data and a[17] == 2.0 and a[18] == N.IDC_REF_SATURATION
    assert a[19].value == dst.ctypes.data and a[20] is None
    with pytest.raises(ValueError):
        e.forward_async_rgb(0, rgb, None, dst, out="source", refs=[ref], ref_index=[0], centres=c)      # n entries
    e.forward_async_rgb(1, rgb, None, dst, out="source", refs=[])                                        # m = 0: no centres needed
    name, a = lib.calls[1]
    assert name == "idc_forward_async_rgb_ref" and a[13] == 0 and a[14] is None and a[15] is None and a[16] is None
