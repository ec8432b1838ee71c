"""Painted hint layers without a device: the footprints of the rule (tests/layer_ref.py, plain loops and numpy float64) against a brute-force
interval-overlap test, the net-size identity against the oracle's rgb2lab, the conditions the GPU inputs have to meet, eight mutants of the
rule that the GPU file's comparisons catch on the GPU file's inputs, csrc/idc_layer.h and the batch plan through a stand-alone program
(plain and under ASan + UBSan: a host program, nothing is loaded into Python), the ABI, and the Python plumbing on stub engines.  Section 1b: the
cases of the 40 x 72 net (layer_ref.NET) -- the form of each from the restated threshold, hinted and covered cells under the one live wave of
the last pass, and three mutants of the walk (H and W swapped, the partial pass left alone, the count of one wave) caught on every case they
concern; the first two are invisible on the 64 x 64 net."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import layer_ref as R
from conftest import REPO
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import engine
from oracle import colorspace as oracle_colorspace

CSRC = os.path.join(REPO, "interactive_deep_colorization_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CASES = list(range(len(R.SIZES)))


# ------------------------------------------------------------------------------------------------ 1. the rule
@pytest.mark.parametrize("out", [8, 64, 256])
def test_footprints_are_the_overlapping_pixels(out):
    for l in range(1, 201):
        covered = np.zeros(l, bool)
        for i in range(out):
            # pixel k covers [k * out, (k + 1) * out) and cell i covers [i * l, (i + 1) * l) of the common lattice: open-interval overlap
            brute = [k for k in range(l) if k * out < (i + 1) * l and (k + 1) * out > i * l]
            lo, hi = R.footprint(i, l, out)
            assert brute and list(range(lo, hi)) == brute, (l, out, i)
            assert hi - lo <= R.span_bound(l, out)
            covered[lo:hi] = True
        assert covered.all()


def test_the_form_threshold():
    assert not R.wave_form(1000, 700) and R.wave_form(65, 16384) and not R.wave_form(1024, 768, 256, 256)
    assert [R.wave_form(*s) for s in R.SIZES] == [False] * 8 + [True]
    text = open(os.path.join(CSRC, "idc_layer.h")).read()
    assert "kLayerThreadMaxPixels = %d" % R.THREAD_MAX in text and "THE THRESHOLD" in text


def test_the_colour_is_the_oracles_rgb2lab_for_every_painted_colour():
    seen = 0
    for k in CASES:
        rgba, alpha_min, _, _ = R.case(k)
        cols = np.unique(rgba[rgba[..., 3] >= alpha_min][:, :3], axis=0)
        cols = np.concatenate([cols, np.array([r[4:7] for r in R.RECTS], np.uint8)])
        want = oracle_colorspace.rgb2lab(cols[None])[0, :, 1:]
        np.testing.assert_allclose(R.rgb_to_ab(cols), want, rtol=0, atol=1e-10)
        seen += len(cols)
    assert seen > 1000


def test_a_net_size_layer_is_its_rectangle_list():
    rgba, alpha_min, _, _ = R.case(R.SIZES.index((64, 64)))
    rects = R.rects_of_layer(rgba, alpha_min)
    assert 100 < len(rects) < R.H * R.W
    got = R.layer_hints(rgba, alpha_min, 0)
    ab, mask = R.raster_rects(rects, "rgb", R.MASK_VALUE)
    assert got["cells"] == len(rects) and got["single"].sum() == len(rects)
    np.testing.assert_array_equal(got["ab"].view(np.int32), ab.view(np.int32))
    np.testing.assert_array_equal(got["mask"], mask)


@pytest.mark.parametrize("k", CASES)
def test_gpu_inputs_meet_their_conditions(k):
    rgba, alpha_min, cover, want = R.case(k)
    assert rgba.shape == R.SIZES[k] + (4,) and rgba.dtype == np.uint8 and (alpha_min, cover) == R.PARAMS[k % 4]
    alphas = set(np.unique(rgba[..., 3]))
    assert alphas <= {0, alpha_min - 1, alpha_min, 255}
    if rgba.shape[0] * rgba.shape[1] > 1000:
        assert alphas == {0, alpha_min - 1, alpha_min, 255}
    cnt, tot = want["cnt"], want["tot"]
    assert (tot >= 1).all() and tot.max() <= (R.THREAD_MAX if not R.wave_form(*R.SIZES[k]) else 1 << 28)
    equal = (cnt >= 1) & (255 * cnt == cover * tot)
    if cover == 255:             # the one case that tests equality on purpose: a fully painted footprint
        assert equal.any() and (equal == (cnt == tot)).all()
    else:
        assert not equal.any()
    covered = R.raster_rects(R.RECTS, "rgb", R.MASK_VALUE)[1][0] != 0
    hinted = (cnt >= 1) & (255 * cnt >= cover * tot)
    assert want["cells"] == int((hinted & ~covered).sum()) > 0
    assert not (hinted & ~covered).all()


def test_the_cases_reach_every_part_of_the_rule():
    multi = [k for k in CASES if (R.case(k)[3]["cnt"] > 1).any()]
    single = [k for k in CASES if R.case(k)[3]["single"].any()]
    assert len(multi) >= 5 and len(single) >= 4 and set(R.PARAMS[k % 4] for k in CASES) == set(R.PARAMS)
    covered = R.raster_rects(R.RECTS, "rgb", R.MASK_VALUE)[1][0] != 0
    under = [k for k in CASES if ((R.case(k)[3]["cnt"] >= 1) & covered).any()]       # rectangles lie over painted cells
    assert len(under) >= 6


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_comparisons_catch_the_mutant(mutant):
    assert len(R.MUTANTS) >= 7
    for k in CASES:
        rgba, alpha_min, cover, want = R.case(k)
        assert R.compare(want["ab"], want["mask"], want["cells"], want) == []
        got = R.layer_hints(rgba, alpha_min, cover, R.RECTS, mutant=mutant)
        bad = R.compare(got["ab"], got["mask"], got["cells"], want)
        if bad:
            print("%s: caught at %dx%d: %s" % (mutant, R.SIZES[k][0], R.SIZES[k][1], "; ".join(bad)))
            return
    pytest.fail("no GPU case catches the mutant %s" % mutant)


# ------------------------------------------------------------------------------------------------ 1b. the 40 x 72 net
NET_CASES = list(range(len(R.NET_SIZES)))


def test_the_net_cases_take_the_forms_they_are_named_for():
    H, W = R.NET
    assert [R.wave_form(lh, lw, H, W) for lh, lw in R.NET_SIZES] == R.NET_WAVE
    assert R.span_bound(640, H) * R.span_bound(1152, W) == R.THREAD_MAX and R.span_bound(641, H) * R.span_bound(1152, W) == 18 * 16
    assert (R.span_bound(65, H), R.span_bound(16384, W)) == (3, 229)
    # the thread form: 3 workgroups of 4 x 256 cells, the last pass of the last one holds TAIL cells = one wave; the wave form: no partial pass
    cells = H * W
    assert cells == 2880 and -(-cells // 1024) == 3 and cells - 11 * 256 == R.TAIL == 64 and cells % 16 == 0
    assert (64 * 64) % 1024 == 0                    # ... which the 64 x 64 net cannot show: four full workgroups


@pytest.mark.parametrize("k", NET_CASES)
def test_the_net_cases_meet_their_conditions(k):
    H, W = R.NET
    rgba, alpha_min, cover, want = R.net_case(k)
    assert rgba.shape == R.NET_SIZES[k] + (4,) and rgba.dtype == np.uint8 and want["ab"].shape == (2, H, W) and want["mask"].shape == (1, H, W)
    assert set(np.unique(rgba[..., 3])) <= {0, alpha_min - 1, alpha_min, 255}
    cnt, tot = want["cnt"], want["tot"]
    assert (tot >= 1).all() and tot.max() <= (R.THREAD_MAX if not R.NET_WAVE[k] else 1 << 28)
    if R.NET_SIZES[k] == (640, 1152):
        assert tot.max() == R.THREAD_MAX            # the largest footprint a thread walks
    equal = (cnt >= 1) & (255 * cnt == cover * tot)
    assert equal.any() and (equal == (cnt == tot)).all() if cover == 255 else not equal.any()
    covered = R.raster_rects(R.NET_RECTS, "rgb", R.MASK_VALUE, H, W)[1][0] != 0
    hinted = (cnt >= 1) & (255 * cnt >= cover * tot)
    assert want["cells"] == int((hinted & ~covered).sum()) > 0
    # hinted cells among the last TAIL cells of the net, some of them under a rectangle and some not
    tail_h, tail_c = hinted.ravel()[-R.TAIL:], covered.ravel()[-R.TAIL:]
    assert (tail_h & ~tail_c).sum() >= 8 and (tail_h & tail_c).sum() >= 4
    assert R.compare(want["ab"], want["mask"], want["cells"], want) == []


def test_a_net_size_layer_on_the_net_is_its_rectangle_list():
    H, W = R.NET
    rgba, alpha_min, _, _ = R.net_case(R.NET_SIZES.index(R.NET))
    rects = R.rects_of_layer(rgba, alpha_min)
    assert 60 < len(rects) < H * W and any(r[0] == H - 1 and r[1] >= W - R.TAIL for r in rects)
    got = R.layer_hints(rgba, alpha_min, 0, H_=H, W_=W)
    ab, mask = R.raster_rects(rects, "rgb", R.MASK_VALUE, H, W)
    assert got["cells"] == len(rects) and got["single"].sum() == len(rects)
    np.testing.assert_array_equal(got["ab"].view(np.int32), ab.view(np.int32))
    np.testing.assert_array_equal(got["mask"], mask)


@pytest.mark.parametrize("mutant", R.NET_MUTANTS)
def test_every_net_case_catches_the_mutants_of_the_walk(mutant):
    H, W = R.NET
    for k in NET_CASES:
        rgba, alpha_min, cover, want = R.net_case(k)
        got = R.layer_hints(rgba, alpha_min, cover, R.NET_RECTS, H_=H, W_=W, mutant=mutant)
        bad = R.compare(got["ab"], got["mask"], got["cells"], want)
        print("%s at %dx%d: %s" % (mutant, R.NET_SIZES[k][0], R.NET_SIZES[k][1], "; ".join(bad) or "not caught"))
        if mutant == "tail_unhinted" and R.NET_WAVE[k]:
            assert bad == []                        # (the wave form has no partial pass on this net: the mutant is no mutant there)
        elif mutant == "transposed_net" and R.NET_SIZES[k] == (1, 1):
            assert bad == []                        # (one pixel under every cell, whichever way the net is read)
        elif mutant == "count_first_wave":
            assert bad and all(b.startswith("cells") for b in bad)
        else:
            assert bad
    # the 64 x 64 net sees none of them: H == W, and its 4096 cells are full workgroups (the count mutant aside, which any net shows)
    if mutant != "count_first_wave":
        for k in CASES[3:7]:
            rgba, alpha_min, cover, want = R.case(k)
            got = R.layer_hints(rgba, alpha_min, cover, R.RECTS, mutant=mutant)
            assert R.compare(got["ab"], got["mask"], got["cells"], want) == []


# ------------------------------------------------------------------------------------------------ 2. the header and the plan
def _make(target, out, san):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc (%s): tools/%s.cpp cannot be compiled" % (HIPCC, target))
    cmd = ["make", "-C", CSRC, target, "BINDIR=" + out, "HIPCC=" + HIPCC] + (["SAN=1"] if san else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return os.path.join(out, target)


@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan_ubsan"])
def test_spans_form_and_plan(tmp_path, san):
    run = subprocess.run([_make("layer_selftest", str(tmp_path), san)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert lines[0] == "spans: %d checked" % (16384 * (8 + 64 + 256)) and lines[-1] == "layer_selftest: ok (8 calls)", run.stdout + run.stderr


def test_the_tool_includes_the_two_headers_only_and_the_header_is_plain_cpp():
    tool = open(os.path.join(REPO, "tools", "layer_selftest.cpp")).read()
    assert re.findall(r"#include\s*\"([^\"]+)\"", tool) == ["idc_layer.h", "idc_batch.h"] and re.search(r"\bint main\(\)", tool)
    text = open(os.path.join(CSRC, "idc_layer.h")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", text) == [] and "__global__" not in text and not re.search(r"\bhip[A-Z]\w+\(", text)


def test_the_kernel_keeps_to_its_brief():
    text = open(os.path.join(CSRC, "idc_layer.hip")).read()
    assert "grid_blocks" not in text and "gridDim" not in text and "GridTag" not in text          # an exact grid: no cap, no tag, no stride loop
    assert len(re.findall(r"hipLaunchKernelGGL\(", text)) == 1 and "asm" not in text
    assert "atomicAdd(&cells" in text and len(re.findall(r"atomic\w*\(", text)) == 1              # one integer atomic, no float atomic
    assert text.count("#pragma clang fp contract(off)") >= 2
    tags = open(os.path.join(CSRC, "idc_grid.h")).read()
    assert "layer" not in tags.lower()


# ------------------------------------------------------------------------------------------------ 3. the ABI
def test_abi_symbols_and_structs():
    header = open(os.path.join(REPO, "include", "ideepcolor.h")).read()
    assert re.search(r"typedef struct idc_hint_layer \{ const uint8_t\* rgba; int32_t h, w; \} idc_hint_layer;", header)
    assert re.search(r"typedef struct idc_batch_layers \{ const idc_hint_layer\* layers[^;]*; int32_t alpha_min, cover; int32_t\* cells[^;]*; \} idc_batch_layers;",
                     header)
    for sym in ("idc_set_hints_layer", "idc_forward_async_layers"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, header) and sym in N.EXPORTED_SYMBOLS
    assert ctypes.sizeof(N.HintLayer) == 16 and ctypes.sizeof(N.BatchLayers) == 24
    assert (N.HintLayer.rgba.offset, N.HintLayer.h.offset, N.HintLayer.w.offset) == (0, 8, 12)
    assert (N.BatchLayers.layers.offset, N.BatchLayers.alpha_min.offset, N.BatchLayers.cover.offset, N.BatchLayers.cells.offset) == (0, 8, 12, 16)
    lib = N.load()
    for sym in ("idc_set_hints_layer", "idc_forward_async_layers"):
        assert hasattr(lib, sym)
    assert lib.idc_set_hints_layer(None, 0, 0, None, N.IDC_HINT_RGB, 1.0, None, 128, 0, None) == -1        # a null handle, without a device
    assert lib.idc_forward_async_layers(None, 0, 1, 0, None, None, None, None, N.IDC_HINT_RGB, 1.0, 0.0, 50.0, 0, None, None, None) == -1
    for line in ("r0 = (y*lh)/H", "r1 = ((y+1)*lh + H-1)/H", "255*cnt >= cover*tot", "A >= alpha_min"):
        assert line in header, line


# ------------------------------------------------------------------------------------------------ 4. the Python plumbing
class _Lib(object):
    """Records what reaches the two entry points, decoded from the ctypes arguments."""

    def __init__(self, fail_after=None):
        self.calls, self.filters, self.fail_after = [], [], fail_after

    def idc_set_ingest_filter(self, h, f):
        self.filters.append(f)
        return 0

    def idc_set_hints_layer(self, h, img, n_hints, hints, mode, mask_value, layer, alpha_min, cover, cells):
        lay = None if layer is None else layer._obj
        self.calls.append(dict(img=img, rows=[(hints[i].y0, hints[i].x0, hints[i].y1, hints[i].x1, hints[i].c0, hints[i].c1, hints[i].c2)
                                              for i in range(n_hints)],
                               mode=mode, mask_value=mask_value, layer=None if lay is None else (lay.rgba, lay.h, lay.w), alpha_min=alpha_min,
                               cover=cover))
        ctypes.cast(cells, ctypes.POINTER(ctypes.c_int32))[0] = 41
        return 0

    def idc_forward_async_layers(self, h, slot, n, bits, images, layers, offsets, hints, mode, mask_value, maskcent, l_cent, flags, refs, outs,
                                 out_ab):
        if self.fail_after is not None and len(self.calls) >= self.fail_after:
            return -2
        tab = ctypes.cast(images, ctypes.POINTER(N.GrayImage if bits else N.RefImage))
        rec = dict(slot=slot, n=n, bits=bits, images=[((tab[i].pix if bits else tab[i].rgb), tab[i].h, tab[i].w) for i in range(n)], mode=mode,
                   mask_value=mask_value, flags=flags, outs=[outs[i] for i in range(n)], layers=None,
                   offsets=None if offsets is None else list(np.ctypeslib.as_array(ctypes.cast(offsets, ctypes.POINTER(ctypes.c_int32)), (n + 1,))))
        if layers is not None:
            b = layers._obj
            rec.update(layers=[(b.layers[i].rgba, b.layers[i].h, b.layers[i].w) for i in range(n)], alpha_min=b.alpha_min, cover=b.cover, cells=b.cells)
            np.ctypeslib.as_array(ctypes.cast(b.cells, ctypes.POINTER(ctypes.c_int32)), (n,))[:] = np.arange(n) + 10 * slot
        self.calls.append(rec)
        return 0


class _Pool(object):
    def take(self, shape, dtype):
        return np.zeros(shape, dtype)


class _Stub(engine.HipColorizer):
    """The engine's own marshalling and generator over a library that launches nothing."""

    def __init__(self, fail_after=None):
        self.H, self.W, self.max_batch = 8, 8, 2
        self._batch_upsample, self._ingest_filter = "linear", "bilinear"
        self._pool, self.lib, self._h, self._in_flight = _Pool(), _Lib(fail_after), None, {}
        self.events = []

    def __del__(self):
        pass

    def _chk(self, rc):
        if rc != 0:
            raise RuntimeError("status %d" % rc)
        if self.lib.calls and "slot" in self.lib.calls[-1] and not self.lib.calls[-1].get("seen"):
            self.lib.calls[-1]["seen"] = (self._ingest_filter, self._batch_upsample)
            self.events.append(("submit", self.lib.calls[-1]["slot"]))

    def set_batch_upsample(self, interp="linear"):
        if interp not in ("linear", "joint"):
            raise ValueError(interp)
        self._batch_upsample = interp

    def _pinned_slices(self, shapes):
        return [np.zeros(s, np.uint8) for s in shapes]

    def wait(self, slot):
        self.events.append(("wait", slot))


def test_set_hint_layer_marshals_its_arguments():
    e = _Stub()
    rgba = np.zeros((5, 9, 4), np.uint8)
    assert e.set_hint_layer(rgba, [(1, 2, 3, 4, 200, 100, 50)], img=1, mask_value=2.0, alpha_min=7, cover=9) == 41
    c = e.lib.calls[-1]
    assert c["layer"] == (rgba.ctypes.data, 5, 9) and (c["alpha_min"], c["cover"], c["img"], c["mode"], c["mask_value"]) == (7, 9, 1, N.IDC_HINT_RGB, 2.0)
    assert c["rows"] == [(1, 2, 3, 4, 200.0, 100.0, 50.0)]
    e.set_hint_layer(rgba[:, ::2])                                       # a view: a contiguous copy travels
    c = e.lib.calls[-1]
    assert c["layer"][1:] == (5, 5) and c["layer"][0] != rgba.ctypes.data and (c["alpha_min"], c["cover"], c["rows"]) == (128, 0, [])
    e.set_hint_layer(None, [(0, 0, 1, 1, 1.0, 2.0)], mode="ab")
    assert e.lib.calls[-1]["layer"] is None and e.lib.calls[-1]["mode"] == N.IDC_HINT_AB
    for bad in (np.zeros((5, 9, 3), np.uint8), np.zeros((5, 9, 4), np.float32), np.zeros((0, 9, 4), np.uint8), np.zeros((5, 9), np.uint8)):
        with pytest.raises(ValueError):
            e.set_hint_layer(bad)
    assert len(e.lib.calls) == 3


def test_forward_async_layers_tells_the_image_kinds_apart():
    e = _Stub()
    rgb, g8, g16 = np.zeros((5, 7, 3), np.uint8), np.zeros((5, 7), np.uint8), np.zeros((6, 4), np.uint16)
    lay = np.zeros((3, 2, 4), np.uint8)
    outs, cells = e.forward_async_layers(1, [rgb, rgb], [lay, None], [None, [(0, 0, 1, 1, 9, 8, 7)]], alpha_min=3, cover=200, out="source")
    c = e.lib.calls[-1]
    assert (c["slot"], c["n"], c["bits"], c["flags"], c["mode"]) == (1, 2, 0, N.IDC_BATCH_OUT_SOURCE, N.IDC_HINT_RGB)
    assert c["images"] == [(rgb.ctypes.data, 5, 7)] * 2 and c["layers"] == [(lay.ctypes.data, 3, 2), (None, 0, 0)] and c["offsets"] == [0, 0, 1]
    assert (c["alpha_min"], c["cover"]) == (3, 200) and c["cells"] == cells.ctypes.data and cells.dtype == np.int32 and list(cells) == [10, 11]
    assert [o.shape for o in outs] == [(5, 7, 3)] * 2 and c["outs"] == [o.ctypes.data for o in outs]
    outs, cells = e.forward_async_layers(0, [g8], None, None)
    c = e.lib.calls[-1]
    assert (c["bits"], c["layers"], c["flags"]) == (8, None, 0) and cells is None and outs[0].shape == (8, 8, 3) and outs[0].dtype == np.uint8
    outs, cells = e.forward_async_layers(0, [g16], [lay], None, out="source", depth=16)
    c = e.lib.calls[-1]
    assert (c["bits"], c["flags"]) == (16, N.IDC_BATCH_OUT_SOURCE | N.IDC_BATCH_OUT_RGB16) and outs[0].shape == (6, 4, 3) and outs[0].dtype == np.uint16
    n = len(e.lib.calls)
    for images, layers, kw in (([rgb, g8], None, {}), ([g8, g16], None, {}), ([rgb.astype(np.float32)], None, {}), ([], None, {}),
                               ([rgb], [lay, lay], {}), ([rgb], [lay[..., :3]], {}), ([g8], None, dict(depth=16, out="source")),
                               ([g16], None, dict(depth=16)), ([rgb[:, ::2]], None, {})):
        with pytest.raises(ValueError):
            e.forward_async_layers(0, images, layers, None, **kw)
    assert len(e.lib.calls) == n


def _items(k=5):
    img = np.zeros((5, 7, 3), np.uint8)
    lay = np.full((3, 3, 4), 255, np.uint8)
    return [(img, lay if i % 2 == 0 else None, None) for i in range(k)]


def test_colorize_layers_alternates_the_slots_and_yields_in_order():
    e = _Stub()
    res = list(e.colorize_layers(_items(5)))
    assert [c["slot"] for c in e.lib.calls] == [0, 1, 0] and [c["n"] for c in e.lib.calls] == [2, 2, 1]
    assert [r[1] for r in res] == [0, 1, 10, 11, 0] and all(r[0].shape == (5, 7, 3) for r in res)
    assert e.events == [("submit", 0), ("submit", 1), ("wait", 0), ("submit", 0), ("wait", 1), ("wait", 0)]
    assert [[l[1:] for l in c["layers"]] for c in e.lib.calls] == [[(3, 3), (0, 0)], [(3, 3), (0, 0)], [(3, 3)]]
    # a change of image kind closes the group
    e = _Stub()
    g = np.zeros((4, 4), np.uint16)
    items = _items(1) + [(g, None, None), (g, None, None), (g.astype(np.uint8), None, None)]
    res = list(e.colorize_layers(items, mode="ab", alpha_min=9))
    assert [(c["bits"], c["n"], c["alpha_min"], c["mode"]) for c in e.lib.calls] == [(0, 1, 9, 0), (16, 2, 9, 0), (8, 1, 9, 0)] and len(res) == 4
    with pytest.raises(ValueError):
        list(e.colorize_layers([(g, None)]))
    with pytest.raises(ValueError):
        list(e.colorize_layers(_items(1), depth=16, out="net"))


def test_colorize_layers_scopes_upsample_and_ingest():
    e = _Stub()
    list(e.colorize_layers(_items(5), upsample="joint", ingest="antialias"))
    assert [c["seen"] for c in e.lib.calls] == [("antialias", "joint")] * 3
    assert (e._ingest_filter, e._batch_upsample) == ("bilinear", "linear") and e.lib.filters == [1, 0]
    # a consumer that walks away: both slots are waited for, the settings go back
    e = _Stub()
    g = e.colorize_layers(_items(5), upsample="joint", ingest="antialias")
    assert e.lib.calls == [] and e.lib.filters == []
    next(g)
    assert (e._ingest_filter, e._batch_upsample) == ("antialias", "joint") and [c["slot"] for c in e.lib.calls] == [0, 1]
    g.close()
    assert e.events == [("submit", 0), ("submit", 1), ("wait", 0), ("wait", 1)]           # nothing stays in flight, nothing new is submitted
    assert (e._ingest_filter, e._batch_upsample) == ("bilinear", "linear")
    # an exception on the way: restored as well
    e = _Stub(fail_after=1)
    with pytest.raises(RuntimeError):
        list(e.colorize_layers(_items(5), upsample="joint", ingest="antialias"))
    assert len(e.lib.calls) == 1 and ("wait", 0) in e.events and (e._ingest_filter, e._batch_upsample) == ("bilinear", "linear")
