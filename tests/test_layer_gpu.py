"""GPU checks of painted hint layers: idc_set_hints_layer and the pipelined idc_forward_async_layers, through HipColorizer and the wrapper.
The references are tests/layer_ref.py (the rule in plain loops and numpy float64), the 1 x 1 IDC_HINT_RGB rectangle list a net-size layer
equals, idc_set_hints, the layer-free pipelined calls, and for a pipelined batch the blocking route per image -- never the call under test.

Bars (tests/layer_ref.py holds them; tests/test_layer_cpu.py shows that they catch eight mutants of the rule on these inputs):
  against the rule   mask plane and cells exact; ab within one float32 ulp everywhere, bit for bit in cells with one painted pixel
  everything else    bit for bit
Shapes: a 64 x 64 net, max_batch 8, bf16.  Layers layer_ref.SIZES -- 1 x 1, one row, one column, the net size, 32 x 32 (a pixel to 2 x 2 cells),
48 x 80 (up on rows, down on columns), 211 x 83 (ragged), 1000 x 700 (thread-form footprints of 204 pixels) and 65 x 16384 (256-wide
footprints: the wave form) -- with (alpha_min, cover) of layer_ref.PARAMS in turn, over the rectangles layer_ref.RECTS.  Section 3b runs
layer_ref.NET_SIZES on the 40 x 72 net (2880 cells: the thread form's last workgroup ends on a pass with one live wave, under which the layers
are painted and a rectangle lies; a swap of H and W shows): 1 x 1, the net size, 72 x 40, 211 x 83, 1000 x 700 and 65 x 16384 (wave), and 640 x 1152 /
641 x 1152 on either side of the form threshold, with a pipelined call of RGB and of uint16 sources.

Wall time of this file on an MI355X, as measured there: 3.4 s for its 42 tests (pytest's own figure); the slowest test takes 0.5 s, every case of
section 3b is below 0.2 s."""
import ctypes

import numpy as np
import pytest

import glob_ref
import gray_ref as G
import joint_ref as J
import layer_ref as R
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import api, engine

pytestmark = pytest.mark.gpu

CASES = list(range(len(R.SIZES)))
AB_HINTS = [(3, 4, 10, 12, 20.0, -30.0), (50, 40, 55, 70, -15.0, 25.0)]


@pytest.fixture(scope="module")
def e(make_sd):
    x = engine.HipColorizer(R.H, R.W, max_batch=8, precision="bf16")
    x.load_state_dict(make_sd(0, "he"))
    yield x
    x.close()


def _planes(e, img=0):
    ab, mask = e.hint_planes(img)
    return np.array(ab), np.array(mask)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ 1. against the rule
@pytest.mark.parametrize("k", CASES, ids=["%dx%d" % s for s in R.SIZES])
def test_blocking_call_is_the_rule(e, k):
    rgba, alpha_min, cover, want = R.case(k)
    cells = e.set_hint_layer(rgba, R.RECTS, mode="rgb", alpha_min=alpha_min, cover=cover, mask_value=R.MASK_VALUE)
    ab, mask = _planes(e)
    bad = R.compare(ab, mask, cells, want)
    print("%dx%d (alpha_min %d, cover %d): %d cells, %d of them from one pixel; %s" % (R.SIZES[k] + (alpha_min, cover, cells, int(want["single"].sum()),
                                                                                               "; ".join(bad) or "equal")))
    assert bad == []


def test_a_net_size_layer_is_its_rectangle_list_bit_for_bit(e):
    rgba, alpha_min, _, _ = R.case(R.SIZES.index((64, 64)))
    rects = R.rects_of_layer(rgba, alpha_min)
    cells = e.set_hint_layer(rgba, alpha_min=alpha_min, cover=0, mask_value=0.5)
    ab, mask = _planes(e)
    e.set_hints(rects, mode="rgb", mask_value=0.5)
    want_ab, want_mask = _planes(e)
    assert cells == len(rects) == int((want_mask != 0).sum()) > 100
    np.testing.assert_array_equal(_bits(ab), _bits(want_ab))
    np.testing.assert_array_equal(mask, want_mask)


# ------------------------------------------------------------------------------------------------ 2. composition
@pytest.mark.parametrize("mode,hints", [("rgb", R.RECTS), ("ab", AB_HINTS)])
def test_rectangles_lie_over_the_layer(e, mode, hints):
    rgba, alpha_min, _, _ = R.case(R.SIZES.index((211, 83)))
    e.set_hints(hints, mode=mode, mask_value=2.0)
    r_ab, r_mask = _planes(e)
    e.set_hint_layer(rgba, alpha_min=alpha_min, cover=0, mask_value=2.0)
    l_ab, l_mask = _planes(e)
    cells = e.set_hint_layer(rgba, hints, mode=mode, alpha_min=alpha_min, cover=0, mask_value=2.0)
    ab, mask = _planes(e)
    cov = r_mask[0] != 0
    assert cov.any() and (cov & (l_mask[0] != 0)).any()
    np.testing.assert_array_equal(_bits(ab), _bits(np.where(cov, r_ab, l_ab)))
    np.testing.assert_array_equal(mask, np.where(cov, r_mask, l_mask))
    assert cells == int(((l_mask[0] != 0) & ~cov).sum())
    assert set(np.unique(mask)) == {0.0, 2.0}


def test_a_transparent_layer_and_no_layer_are_set_hints(e):
    e.set_hints(R.RECTS, mode="rgb", mask_value=1.5)
    want = _planes(e)
    clear = np.array(R.case(5)[0])
    clear[..., 3] = 127
    assert e.set_hint_layer(clear, R.RECTS, alpha_min=128, mask_value=1.5) == 0
    got = _planes(e)
    e.set_hints([], mode="ab")
    assert not _planes(e)[1].any()
    assert e.set_hint_layer(None, R.RECTS, mask_value=1.5) == 0
    none = _planes(e)
    for g in (got, none):
        np.testing.assert_array_equal(_bits(g[0]), _bits(want[0]))
        np.testing.assert_array_equal(g[1], want[1])
    # without a layer the call is idc_set_hints in what it accepts, too: a zero mask_value and the range audit
    assert e.set_hint_layer(None, R.RECTS, mask_value=0.0) == 0 and not _planes(e)[1].any()


# ------------------------------------------------------------------------------------------------ 3. pipelined against blocking
_BLOCK = {}


def _layers(e, pinned_mask=0b0101):
    """Five entries, one without a layer; the starts of the four in the packed run (in pixels) fall on every residue mod 4; pinned and
    pageable buffers mixed."""
    one = np.array([[[250, 20, 30, 255]]], np.uint8)
    nine = np.array(R.draw_layer(3, 3, 128, 7))
    nine[1, 1, 3] = 255
    lays = [one, np.array(R.case(6)[0]), None, nine, np.array(R.case(5)[0])]
    starts = np.cumsum([0] + [l.shape[0] * l.shape[1] for l in lays if l is not None])[:-1]
    assert sorted(int(s) % 4 for s in starts) == [0, 1, 2, 3]
    out = []
    for i, l in enumerate(lays):
        if l is not None and (pinned_mask >> i) & 1:
            p = e.pinned_empty(l.shape, np.uint8)
            np.copyto(p, l)
            l = p
        out.append(l)
    return out


def _sources(kind):
    sizes = [(37, 41), (13, 17), (64, 64), (211, 83), (5, 9)]
    if kind == "rgb":
        return [np.ascontiguousarray(J.source(h, w)) for h, w in sizes]
    return [np.ascontiguousarray((G.gray16 if kind == "gray16" else G.gray8)(h, w)) for h, w in sizes]


def _hint_lists(mode):
    rows = R.RECTS if mode == "rgb" else AB_HINTS
    return [rows[:1], None, rows, rows[1:], None]


def _ingest(e, src):
    if src.ndim == 3:
        e.set_image_rgb(src, keep_source=True, want_rgb=False, want_lab=False)
    else:
        e.set_image_gray(src, keep_source=True, want_net=False, want_l=False)


def _blocking(e, src, layer, hints, mode, params, interp, out, depth=8, filt="bilinear", ref=None):
    """(image, out_ab, cells, hint planes) of one image by the blocking route; the handle's filter is left as it was."""
    k = (e.H, e.W, src.shape, src.dtype.str, src.tobytes(), None if layer is None else (layer.shape, np.asarray(layer).tobytes()), repr(hints), mode, params,
         interp, out, depth, filt, None if ref is None else ref[1])
    if k not in _BLOCK:
        prev = e._ingest_filter
        e.set_ingest_filter(filt)
        _ingest(e, src)
        e.set_ingest_filter(prev)
        if ref is not None:
            e.set_global_refs(ref[0], glob_ref.centres(), ref_index=[ref[1]], saturation=True)
        cells = e.set_hint_layer(layer, hints or [], mode=mode, alpha_min=params[0], cover=params[1], mask_value=params[2])
        raw, rgb, _ = e.forward_resident(1)
        img = np.array(rgb[0]) if out == "net" else np.array(e.fullres_rgb("output_ab", interp, "image", depth=depth))
        img.setflags(write=False)
        _BLOCK[k] = (img, np.array(raw[0]), cells, _planes(e))
    return _BLOCK[k]


def _check_batch(e, slot, srcs, lays, hints, mode, params, interp, out, outs, cells, ab, depth=8, filt="bilinear", refs=None, ref_index=None):
    for i, src in enumerate(srcs):
        ref = None if refs is None else (refs, ref_index[i])
        want, raw, want_cells, _ = _blocking(e, src, lays[i], hints[i], mode, params, interp, out, depth, filt, ref)
        assert outs[i].dtype == want.dtype and outs[i].shape == want.shape
        np.testing.assert_array_equal(outs[i], want, err_msg="image %d, slot %d, %s, %s" % (i, slot, out, interp))
        np.testing.assert_array_equal(_bits(ab[i]), _bits(raw), err_msg="image %d" % i)
        assert int(cells[i]) == want_cells, (i, slot)


@pytest.mark.parametrize("upsample", ["linear", "joint"])
@pytest.mark.parametrize("kind", ["rgb", "gray8", "gray16"])
def test_batches_equal_the_blocking_route_with_two_batches_in_flight(e, kind, upsample):
    e.set_batch_upsample(upsample)
    try:
        srcs = _sources(kind)
        n = len(srcs)
        jobs = [(0, "source", 8, "rgb", (128, 0, 1.0), 0b01010), (1, "net", 8, "ab", (200, 100, 0.5), 0b10001)]
        if kind == "gray16":
            jobs[0] = (0, "source", 16, "rgb", (128, 0, 1.0), 0b01010)
        got = []
        for slot, out, depth, mode, params, pinned in jobs:                   # both are enqueued before either is waited for
            lays = _layers(e, pinned)[::1 if slot == 0 else -1]
            assert [l is None for l in lays].count(True) == 1
            ab = np.empty((n, 2, R.H, R.W), np.float32)
            outs, cells = e.forward_async_layers(slot, srcs, lays, _hint_lists(mode), out_ab=ab, mode=mode, mask_value=params[2], out=out,
                                                 depth=depth, alpha_min=params[0], cover=params[1])
            got.append((lays, outs, cells, ab))
        e.wait(0); e.wait(1)
        for (slot, out, depth, mode, params, _), (lays, outs, cells, ab) in zip(jobs, got):
            t = e.pipeline_times(slot)
            assert t.shape == (6,) and np.isfinite(t).all() and np.all(np.diff(t) >= -1e-3)
            _check_batch(e, slot, srcs, lays, _hint_lists(mode), mode, params, upsample, out, [np.array(o) for o in outs], np.array(cells), ab, depth)
            assert np.array(cells)[[l is None for l in lays].index(True)] == 0 and np.array(cells).sum() > 0
        # the layers were read: without them the batch is another one
        plain = np.empty((n, 2, R.H, R.W), np.float32)
        e.forward_async_layers(0, srcs, None, _hint_lists("rgb"), out_ab=plain, mode="rgb")
        e.wait(0)
        assert (plain != got[0][3]).any()
    finally:
        e.set_batch_upsample("linear")


def test_batches_with_the_antialias_filter_equal_the_blocking_route(e):
    srcs, lays, hints, params = _sources("rgb"), _layers(e), _hint_lists("rgb"), (128, 0, 1.0)
    ab = np.empty((len(srcs), 2, R.H, R.W), np.float32)
    e.set_ingest_filter("antialias")
    try:
        outs, cells = e.forward_async_layers(1, srcs, lays, hints, out_ab=ab, out="source")
    finally:
        e.set_ingest_filter("bilinear")
    e.wait(1)
    _check_batch(e, 1, srcs, lays, hints, "rgb", params, "linear", "source", [np.array(o) for o in outs], np.array(cells), ab, filt="antialias")
    d = srcs[3]
    assert (_blocking(e, d, lays[3], hints[3], "rgb", params, "linear", "source", filt="antialias")[1]
            != _blocking(e, d, lays[3], hints[3], "rgb", params, "linear", "source")[1]).any()


def test_batches_with_references_equal_the_blocking_route():
    from test_glob_ref_gpu import _glob_sd
    x = engine.HipColorizer(R.H, R.W, max_batch=8, precision="bf16", global_hints=True)
    try:
        x.load_state_dict(_glob_sd(3))
        c, r = glob_ref.centres(), glob_ref.refs64()
        srcs, lays, hints, params = _sources("rgb"), _layers(x), _hint_lists("rgb"), (128, 0, 1.0)
        index = [1, -1, 0, 1, 0]
        ab = np.empty((len(srcs), 2, R.H, R.W), np.float32)
        outs, cells = x.forward_async_layers(0, srcs, lays, hints, out_ab=ab, out="source", refs=[r[0], r[1]], ref_index=index, centres=c,
                                             saturation=True)
        x.wait(0)
        _check_batch(x, 0, srcs, lays, hints, "rgb", params, "linear", "source", [np.array(o) for o in outs], np.array(cells), ab,
                     refs=[r[0], r[1]], ref_index=index)
        x.clear_global_hints()
        plain = np.empty_like(ab)
        x.forward_async_layers(1, srcs, lays, hints, out_ab=plain, out="source")
        x.wait(1)
        assert (plain != ab).any()                                              # the references were read
    finally:
        x.close()


@pytest.mark.parametrize("kind", ["rgb", "gray8", "gray16"])
def test_without_layers_the_call_is_the_layer_free_one(e, kind):
    srcs = _sources(kind)
    n = len(srcs)
    for slot, out, mode in ((0, "source", "ab"), (1, "net", "rgb")):
        depth = 16 if kind == "gray16" and out == "source" else 8
        ab, want_ab = np.empty((n, 2, R.H, R.W), np.float32), np.empty((n, 2, R.H, R.W), np.float32)
        outs, cells = e.forward_async_layers(slot, srcs, None, _hint_lists(mode), out_ab=ab, mode=mode, out=out, depth=depth, mask_value=0.0)
        e.wait(slot)
        outs = [np.array(o) for o in outs]
        if kind == "rgb":
            want = e.forward_async_images(slot, srcs, _hint_lists(mode), out_ab=want_ab, mode=mode, out=out, mask_value=0.0)
        else:
            want = e.forward_async_gray(slot, srcs, _hint_lists(mode), out_ab=want_ab, mode=mode, out=out, depth=depth, mask_value=0.0)
        e.wait(slot)
        assert cells is None
        for i in range(n):
            assert outs[i].dtype == want[i].dtype
            np.testing.assert_array_equal(outs[i], want[i])
        np.testing.assert_array_equal(_bits(ab), _bits(want_ab))
        # a table without a layer: the same image, and zero counts
        outs2, cells2 = e.forward_async_layers(slot, srcs, [None] * n, _hint_lists(mode), out_ab=ab, mode=mode, out=out, depth=depth,
                                               mask_value=0.0)
        e.wait(slot)
        assert not np.array(cells2).any()
        for i in range(n):
            np.testing.assert_array_equal(outs2[i], want[i])


def test_the_generator_yields_what_the_blocking_route_gives(e):
    srcs, lays, hints = _sources("rgb"), _layers(e, 0), _hint_lists("rgb")
    g16 = _sources("gray16")
    items = [(s, l, h) for s, l, h in zip(srcs, lays, hints)] + [(g16[0], lays[0], None), (g16[1], None, None), (srcs[0], lays[4], None)]
    res = list(e.colorize_layers(items, batch=3, mode="rgb", alpha_min=128, cover=0))
    assert len(res) == len(items)
    for (src, lay, h), (rgb, cells) in zip(items, res):
        want, _, want_cells, _ = _blocking(e, src, lay, h, "rgb", (128, 0, 1.0), "linear", "source")
        np.testing.assert_array_equal(rgb, want)
        assert cells == want_cells


# ------------------------------------------------------------------------------------------------ 3b. a net that is not square (40 x 72)
# layer_ref.NET: 2880 cells, so the thread form's last workgroup ends on a pass with ONE live wave, under which the cases paint hinted cells and
# NET_RECTS[2] covers some; tests/test_layer_cpu.py shows that these cases catch a swap of H and W, an unhinted tail and a count of one wave.
NET_CASES = list(range(len(R.NET_SIZES)))


@pytest.fixture(scope="module")
def en(make_sd):
    x = engine.HipColorizer(R.NET[0], R.NET[1], max_batch=8, precision="bf16")
    x.load_state_dict(make_sd(0, "he"))
    yield x
    x.close()


@pytest.mark.parametrize("k", NET_CASES, ids=["%dx%d" % s for s in R.NET_SIZES])
def test_blocking_call_on_the_40x72_net_is_the_rule(en, k):
    rgba, alpha_min, cover, want = R.net_case(k)
    assert (en.H, en.W) == R.NET and R.wave_form(rgba.shape[0], rgba.shape[1], en.H, en.W) == R.NET_WAVE[k]
    cells = en.set_hint_layer(rgba, R.NET_RECTS, mode="rgb", alpha_min=alpha_min, cover=cover, mask_value=R.MASK_VALUE)
    ab, mask = _planes(en)
    bad = R.compare(ab, mask, cells, want)
    print("%dx%d (alpha_min %d, cover %d): %d cells (want %d); %s" % (R.NET_SIZES[k] + (alpha_min, cover, cells, want["cells"], "; ".join(bad) or "equal")))
    assert bad == []


def test_a_net_size_layer_on_the_40x72_net_is_its_rectangle_list_bit_for_bit(en):
    rgba, alpha_min, _, _ = R.net_case(R.NET_SIZES.index(R.NET))
    rects = R.rects_of_layer(rgba, alpha_min)
    cells = en.set_hint_layer(rgba, alpha_min=alpha_min, cover=0, mask_value=0.5)
    ab, mask = _planes(en)
    en.set_hints(rects, mode="rgb", mask_value=0.5)
    want_ab, want_mask = _planes(en)
    assert cells == len(rects) == int((want_mask != 0).sum()) > 60
    np.testing.assert_array_equal(_bits(ab), _bits(want_ab))
    np.testing.assert_array_equal(mask, want_mask)


@pytest.mark.parametrize("kind", ["rgb", "gray16"])
def test_a_batch_on_the_40x72_net_equals_the_blocking_route(en, kind):
    sizes = [(37, 41), (40, 72), (211, 83), (5, 9)]
    srcs = [np.ascontiguousarray(J.source(h, w) if kind == "rgb" else G.gray16(h, w)) for h, w in sizes]
    lays = [np.array(R.net_case(3)[0]), None, np.array(R.net_case(5)[0]), np.array(R.net_case(6)[0])]      # thread, none, wave, thread (16 x 16)
    hints = [R.NET_RECTS[:1], None, R.NET_RECTS, R.NET_RECTS[1:]]
    params, depth = (128, 0, 1.0), 16 if kind == "gray16" else 8
    ab = np.empty((4, 2, en.H, en.W), np.float32)
    outs, cells = en.forward_async_layers(1, srcs, lays, hints, out_ab=ab, mode="rgb", out="source", depth=depth, alpha_min=params[0], cover=params[1])
    en.wait(1)
    cells = np.array(cells)
    _check_batch(en, 1, srcs, lays, hints, "rgb", params, "linear", "source", [np.array(o) for o in outs], cells, ab, depth)
    assert cells[1] == 0 and (cells[[0, 2, 3]] > 0).all()
    for i in (0, 2, 3) if kind == "rgb" else ():    # ... and the blocking route's planes and count are the rule's, under these parameters too
        _, _, want_cells, (b_ab, b_mask) = _blocking(en, srcs[i], lays[i], hints[i], "rgb", params, "linear", "source", depth)
        assert R.compare(b_ab, b_mask, want_cells, R.layer_hints(lays[i], params[0], params[1], hints[i], H_=en.H, W_=en.W)) == []


# ------------------------------------------------------------------------------------------------ 4. the resident state
def test_the_blocking_call_writes_the_hint_planes_and_nothing_else(e):
    src = _sources("rgb")[3]
    rgba, alpha_min, cover, _ = R.case(6)
    e.set_image_rgb(src, keep_source=True, want_rgb=False, want_lab=False)
    e.set_hints(AB_HINTS, mode="ab")
    raw0, rgb0, _ = e.forward_resident(1)
    raw0, rgb0, full0 = np.array(raw0), np.array(rgb0), np.array(e.fullres_rgb("output_ab", "linear", "image"))
    in0 = np.array(e.fullres_rgb("input_ab", "linear", "image"))
    e.set_hint_layer(rgba, AB_HINTS, mode="ab", alpha_min=alpha_min, cover=cover)
    # the result of the last forward and the kept source are as they were; input_ab shows the new planes
    np.testing.assert_array_equal(np.array(e.fullres_rgb("output_ab", "linear", "image")), full0)
    assert (np.array(e.fullres_rgb("input_ab", "linear", "image")) != in0).any()
    raw1 = np.array(e.forward_resident(1)[0])
    assert (raw1 != raw0).any()                                                 # the network saw the layer
    # rectangle-only calls after layer calls, blocking and pipelined: the bytes they gave before
    e.set_hints(AB_HINTS, mode="ab")
    raw2, rgb2, _ = e.forward_resident(1)
    np.testing.assert_array_equal(np.array(raw2), raw0)
    np.testing.assert_array_equal(np.array(rgb2), rgb0)
    np.testing.assert_array_equal(np.array(e.fullres_rgb("output_ab", "linear", "image")), full0)
    srcs = _sources("rgb")
    before = e.forward_async_images(0, srcs, _hint_lists("ab"), out="source")
    e.wait(0)
    before = [np.array(o) for o in before]
    e.forward_async_layers(0, srcs, _layers(e), _hint_lists("rgb"), out="source")
    e.wait(0)
    after = e.forward_async_images(0, srcs, _hint_lists("ab"), out="source")
    e.wait(0)
    for b, a in zip(before, after):
        np.testing.assert_array_equal(a, b)


def test_the_wrapper_forwards_a_layer(make_sd):
    model = api.ColorizeImageTorch(Xd=R.H, precision="bf16")
    model.prep_net(0, state_dict=make_sd(0, "he"))
    model.set_image(J.source(R.H, R.W))
    rgba, alpha_min, cover, want = R.case(6)
    out = model.net_forward_layer(rgba, R.RECTS, alpha_min=alpha_min, cover=cover)
    assert out.shape == (R.H, R.W, 3) and model.layer_cells == want["cells"]
    assert R.compare(np.asarray(model.input_ab, np.float32), np.asarray(model.input_mask, np.float32), model.layer_cells, want) == []
    plain = model.net_forward_hints(R.RECTS)
    assert (np.asarray(plain) != np.asarray(out)).any()


# ------------------------------------------------------------------------------------------------ 5. statuses
def test_blocking_statuses_and_a_refused_call_changes_nothing(e):
    lib, h = e.lib, e._h
    px = np.full((4, 4, 4), 255, np.uint8)
    e.set_hints(AB_HINTS, mode="ab", mask_value=3.0)
    before = _planes(e)

    def call(h_=4, w_=4, rgba=px.ctypes.data, alpha_min=128, cover=0, mask_value=1.0, mode=N.IDC_HINT_AB, img=0):
        lay = N.HintLayer(rgba, h_, w_)
        cells = ctypes.c_int32(-5)
        rc = lib.idc_set_hints_layer(h, img, 0, None, mode, mask_value, ctypes.byref(lay), alpha_min, cover, ctypes.cast(ctypes.byref(cells), ctypes.c_void_p))
        return rc, cells.value

    for kw in (dict(h_=0), dict(h_=16385), dict(w_=0), dict(w_=16385), dict(alpha_min=0), dict(alpha_min=256), dict(cover=-1), dict(cover=256),
               dict(rgba=None), dict(mask_value=0.0), dict(mask_value=float("inf")), dict(mask_value=float("nan")), dict(mode=N.IDC_HINT_REVEAL),
               dict(mode=7)):
        assert call(**kw) == (-1, -5), kw
    assert call(img=8)[0] == -6
    e.set_range_audit(True)
    try:
        assert call() == (-7, -5)
        e.set_hint_layer(None, AB_HINTS, mode="ab", mask_value=3.0)             # without a layer it is idc_set_hints, which the audit allows
    finally:
        e.set_range_audit(False)
    after = _planes(e)
    np.testing.assert_array_equal(_bits(after[0]), _bits(before[0]))
    np.testing.assert_array_equal(after[1], before[1])
    assert call() == (0, R.H * R.W) and call(alpha_min=255, cover=255) == (0, R.H * R.W)
    assert b"" != lib.idc_last_error(h)


def test_pipelined_statuses_and_a_refused_call_leaves_the_slot_usable(e):
    lib, h, vp = e.lib, e._h, ctypes.c_void_p
    px, out = np.zeros(64, np.uint16), np.zeros(256, np.uint16)
    rgba = np.full((4, 4, 4), 255, np.uint8)
    cells = np.full(2, -5, np.int32)
    SRC = N.IDC_BATCH_OUT_SOURCE

    def call(bits=0, n=2, flags=SRC, mode=0, slot=0, lh=4, lw=4, lpx=rgba.ctypes.data, alpha_min=128, cover=0, mask_value=1.0, null_table=False,
             no_layers=False, want_cells=True):
        tab = ((N.GrayImage if bits else N.RefImage) * 2)()
        outs, lays = (vp * 2)(), (N.HintLayer * 2)()
        for i in range(2):
            if bits:
                tab[i].pix = px.ctypes.data
            else:
                tab[i].rgb = px.ctypes.data
            tab[i].h, tab[i].w = 2, 3
            outs[i] = out.ctypes.data
        lays[0].rgba, lays[0].h, lays[0].w = lpx, lh, lw
        block = N.BatchLayers(None if null_table else lays, alpha_min, cover, cells.ctypes.data if want_cells else None)
        return lib.idc_forward_async_layers(h, slot, n, bits, ctypes.cast(tab, vp), None if no_layers else ctypes.byref(block), None, None, mode,
                                            mask_value, 0.0, 50.0, flags, None, outs, None)

    for kw in (dict(lh=0), dict(lh=16385), dict(lw=0), dict(lw=16385), dict(alpha_min=0), dict(alpha_min=256), dict(cover=-1), dict(cover=256),
               dict(null_table=True), dict(mask_value=0.0), dict(mask_value=float("inf")), dict(mask_value=float("nan")), dict(bits=12), dict(bits=-1),
               dict(bits=24), dict(mode=N.IDC_HINT_REVEAL), dict(bits=8, mode=N.IDC_HINT_REVEAL), dict(flags=4), dict(slot=2)):
        assert call(**kw) == -1, kw
    assert call(n=0) == -6 and call(n=9) == -6
    # layer bytes above the bound in all: the plan adds the sizes up, the bytes are never touched
    big = (N.HintLayer * 2)()
    for i in range(2):
        big[i].rgba, big[i].h, big[i].w = rgba.ctypes.data, 16384, 16384
    tab, outs = (N.RefImage * 2)(), (vp * 2)()
    for i in range(2):
        tab[i].rgb, tab[i].h, tab[i].w, outs[i] = px.ctypes.data, 2, 3, out.ctypes.data
    block = N.BatchLayers(big, 128, 0, None)
    assert lib.idc_forward_async_layers(h, 0, 2, 0, ctypes.cast(tab, vp), ctypes.byref(block), None, None, 0, 1.0, 0.0, 50.0, SRC, None, outs, None) == -1
    e.set_range_audit(True)
    try:
        assert call() == -7
    finally:
        e.set_range_audit(False)
    assert (cells == -5).all() and b"" != lib.idc_last_error(h)
    # nothing was enqueued by any of them: the slot takes the next call, which runs, and refuses a second one until it is waited for
    assert call() == 0
    assert call() == -1
    assert lib.idc_wait(h, 0) == 0
    assert list(cells) == [R.H * R.W, 0]
    # an image without a layer needs no mask_value; neither does a call without the block; NULL cells is allowed
    assert call(lpx=None, mask_value=0.0) == 0 and lib.idc_wait(h, 0) == 0 and list(cells) == [0, 0]
    assert call(no_layers=True, mask_value=0.0, bits=8) == 0 and lib.idc_wait(h, 0) == 0
    assert call(want_cells=False, bits=16, slot=1) == 0 and lib.idc_wait(h, 1) == 0


# ------------------------------------------------------------------------------------------------ 6. the exact grid
def test_the_exact_grid_ignores_the_grid_cap(e):
    rgba, alpha_min, cover, want = R.case(R.SIZES.index((65, 16384)))
    assert R.wave_form(*rgba.shape[:2])
    engine.set_option("grid_cap", 1)
    try:
        cells = e.set_hint_layer(rgba, R.RECTS, alpha_min=alpha_min, cover=cover)
        ab, mask = _planes(e)
    finally:
        engine.set_option("grid_cap", 0)
    assert R.compare(ab, mask, cells, want) == []
    assert "layer" not in " ".join(engine.grid_tags()).lower() and len(engine.grid_tags()) == 21


def test_the_wave_form_with_several_images_under_the_cap(e):
    rgba, alpha_min, cover, want = R.case(R.SIZES.index((65, 16384)))
    small = R.case(5)
    srcs = _sources("rgb")[:3]
    lays = [np.array(rgba), np.array(small[0]), np.array(rgba)]
    hints = [R.RECTS, R.RECTS, None]
    ab = np.empty((3, 2, R.H, R.W), np.float32)
    engine.set_option("grid_cap", 1)
    try:
        outs, cells = e.forward_async_layers(1, srcs, lays, hints, out_ab=ab, alpha_min=alpha_min, cover=cover)
        e.wait(1)
    finally:
        engine.set_option("grid_cap", 0)
    cells = np.array(cells)
    assert cells[0] == want["cells"] and cells[2] == int(((want["cnt"] >= 1) & (255 * want["cnt"] >= cover * want["tot"])).sum())
    for i in range(3):
        w = _blocking(e, srcs[i], lays[i], hints[i], "rgb", (alpha_min, cover, 1.0), "linear", "net")
        np.testing.assert_array_equal(_bits(ab[i]), _bits(w[1]))
        assert cells[i] == w[2]
