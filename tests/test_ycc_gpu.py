"""GPU checks of the YCbCr 4:2:0 output planes: idc_rgb_to_ycc420, idc_fullres_ycc and idc_set_batch_output on every pipelined entry point,
through HipColorizer and the C ABI.  The reference is tests/ycc_ref.py -- the rule of include/ideepcolor.h in plain Python integers -- applied
to the uint8 RGB image the same call returns with IDC_OUT_RGB on the same handle; never the call under test.  Every comparison is exact
(tests/test_ycc_cpu.py shows that it catches eight mutants of the rule on the inputs of the first case).

Shapes: a 64 x 64 net, max_batch 8, bf16.  The conversion case holds ycc_ref.inputs() in ONE call: 1 x 1 up to 65 x 16384, the size lists of
tests/ragged_ref.py (image starts on every residue mod 4), painted primaries with hard edges at odd coordinates, flat 0 and 255.  The pipelined
cases take sources of ragged_ref.MIXED and 83 x 211, at the net size and at the source size, on both slots, pinned and pageable destinations
mixed, each under I420 / JFIF and under NV12 / BT.709."""
import ctypes

import numpy as np
import pytest

import glob_ref
import ragged_ref
import ycc_ref as R
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import engine

pytestmark = pytest.mark.gpu

FMT = {"i420": N.IDC_OUT_I420, "nv12": N.IDC_OUT_NV12}
MAT = {"jfif": N.IDC_YCC_JFIF, "bt709": N.IDC_YCC_BT709_VIDEO}
PAIRS = [("i420", "jfif"), ("nv12", "bt709")]
SIZES = ragged_ref.sizes(ragged_ref.MIXED, R.H, R.W) + [(83, 211)]                  # 8 images: one full batch
HINTS = [(3, 4, 10, 12, 20.0, -30.0), (50, 40, 55, 70, -15.0, 25.0), (20, 20, 22, 60, 40.0, 40.0)]
RECTS = [(3, 4, 10, 12), (50, 40, 55, 70), (0, 0, 63, 63)]


@pytest.fixture(scope="module")
def e(make_sd):
    x = engine.HipColorizer(R.H, R.W, max_batch=8, precision="bf16")
    x.load_state_dict(make_sd(0, "he"))
    yield x
    x.close()


@pytest.fixture(scope="module")
def eg():
    from test_glob_ref_gpu import _glob_sd
    x = engine.HipColorizer(R.H, R.W, max_batch=8, precision="bf16", global_hints=True)
    x.load_state_dict(_glob_sd(3))
    yield x
    x.close()


@pytest.fixture(scope="module")
def ed(make_sd):
    x = engine.HipColorizer(R.H, R.W, max_batch=8, precision="bf16", dist=True)
    x.load_state_dict(make_sd(0, "he"))
    yield x
    x.close()


def _grid529():
    axis = np.arange(-110, 120, 10)
    return np.ascontiguousarray(np.array(np.meshgrid(axis, axis)).reshape((2, 529)).T.astype(np.float32))


def _sources():
    return [ragged_ref.image(h, w, 11 + i) for i, (h, w) in enumerate(SIZES)]


def _hint_lists(n):
    return [None if i % 3 == 0 else HINTS[i % 3:] for i in range(n)]


def _check_block(got, rgb, fmt, matrix, what):
    want = R.block(np.ascontiguousarray(rgb), fmt, matrix)
    got = np.asarray(got).reshape(-1)
    assert got.size == want.size == R.nbytes(*rgb.shape[:2]), what
    bad = int((got != want).sum())
    assert bad == 0, "%s: %d of %d bytes differ, first at %d" % (what, bad, want.size, int(np.flatnonzero(got != want)[0]))


# ------------------------------------------------------------------------------------------------ 1. the conversion alone
@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("matrix", sorted(R.MATRICES))
def test_conversion_alone_is_the_rule(e, fmt, matrix):
    ins = R.inputs()
    n = len(ins)
    table = (N.RefImage * n)()
    outs = (ctypes.c_void_p * n)()
    bufs = []
    for i, (_, a) in enumerate(ins):
        nb = R.nbytes(*a.shape[:2])
        assert e.lib.idc_ycc420_bytes(a.shape[0], a.shape[1]) == nb
        # pinned and pageable destinations mixed; two guard bytes behind each: nothing is written past a block
        buf = e.pinned_empty((nb + 2,), np.uint8) if i % 3 == 1 else np.empty(nb + 2, np.uint8)
        buf[:] = 0xEE
        bufs.append(buf)
        table[i].rgb, table[i].h, table[i].w = a.ctypes.data, a.shape[0], a.shape[1]
        outs[i] = buf.ctypes.data
    assert e.lib.idc_rgb_to_ycc420(e._h, n, table, FMT[fmt], MAT[matrix], outs) == 0
    for (name, a), buf in zip(ins, bufs):
        _check_block(buf[:-2], a, fmt, matrix, name)
        assert buf[-1] == 0xEE and buf[-2] == 0xEE, name
    # the Python form, one image and a list
    one = e.rgb_to_ycc420(ins[9][1], fmt, matrix)
    _check_block(one.buf, ins[9][1], fmt, matrix, ins[9][0])
    y, cb, cr = R.planes(ins[9][1], matrix)
    np.testing.assert_array_equal(one.y, y)
    if fmt == "i420":
        np.testing.assert_array_equal(one.cb, cb)
        np.testing.assert_array_equal(one.cr, cr)
    else:
        np.testing.assert_array_equal(one.cbcr[..., 0], cb)
        np.testing.assert_array_equal(one.cbcr[..., 1], cr)


# ------------------------------------------------------------------------------------------------ 2. blocking: idc_fullres_ycc
COMBOS = [("output_ab", "linear", "image"), ("output_ab", "cubic", "image"), ("output_ab", "nearest", "image"), ("output_ab", "joint", "image"),
          ("input_ab", "linear", "image"), ("input_ab", "cubic", "mask50"), ("no_ab", "linear", "image"), ("no_ab", "nearest", "mask50"),
          ("output_ab", "linear", "mask50"), ("input_ab", "joint", "image")]


@pytest.mark.parametrize("kind", ["rgb", "gray8", "gray16"])
def test_fullres_ycc_is_the_rule_of_fullres_rgb(e, kind):
    src = ragged_ref.image(77, 131, 5)
    if kind == "rgb":
        e.set_image_rgb(src, keep_source=True, want_rgb=False, want_lab=False)
    else:
        g = src[..., 1] if kind == "gray8" else (src[..., 1].astype(np.uint16) * 251 + src[..., 0])
        e.set_image_gray(np.ascontiguousarray(g), keep_source=True, want_net=False, want_l=False)
    e.set_hints(HINTS, mode="ab", mask_value=1.0)
    e.forward_resident(1)
    for k, (source, interp, l_mode) in enumerate(COMBOS):
        fmt, matrix = PAIRS[k % 2]
        rgb = np.array(e.fullres_rgb(source, interp, l_mode))
        assert rgb.shape == (77, 131, 3)
        got = e.fullres_ycc(source, interp, l_mode, format=fmt, matrix=matrix)
        _check_block(got.buf, rgb, fmt, matrix, "%s %s %s %s" % (kind, source, interp, l_mode))
    # a pinned destination, through the C ABI
    rgb = np.array(e.fullres_rgb("output_ab", "linear", "image"))
    pin = e.pinned_empty((R.nbytes(77, 131),), np.uint8)
    assert e.lib.idc_fullres_ycc(e._h, 0, N.IDC_SRC_OUTPUT_AB, N.IDC_INTERP_LINEAR, N.IDC_L_IMAGE, N.IDC_OUT_NV12, N.IDC_YCC_JFIF,
                                 pin.ctypes.data_as(ctypes.c_void_p)) == 0
    _check_block(pin, rgb, "nv12", "jfif", "pinned")


# ------------------------------------------------------------------------------------------------ 3. pipelined
def _dims(srcs, out):
    return [tuple(s.shape[:2]) if out == "source" else (R.H, R.W) for s in srcs]


def _outs(x, srcs, out, flip=0):
    """One destination per image under the engine's output format in force: pinned and pageable mixed."""
    shapes = x._out_shapes([d + (3,) for d in _dims(srcs, out)])
    return [x.pinned_empty(s, np.uint8) if (i + flip) % 2 == 0 else np.empty(s, np.uint8) for i, s in enumerate(shapes)]


def _call(x, kind, slot, out, srcs):
    """Enqueue one batch of `kind` on `slot`; -> (images, extras): what comes back as images, and every other result, after wait(slot)."""
    n = len(srcs)
    hints = _hint_lists(n)
    ab = x.pinned_empty((n, 2, R.H, R.W), np.float32)
    ex = {"ab": ab}
    if kind in ("rgb", "rgb_ref"):
        batch = np.ascontiguousarray(np.stack([srcs[5]] * 3))
        d = _dims([srcs[5]], out)[0]
        dst = np.empty((3, d[0], d[1], 3) if x._out_format == "rgb" else (3, R.nbytes(*d)), np.uint8)
        ab3 = x.pinned_empty((3, 2, R.H, R.W), np.float32)
        kw = dict(refs=glob_ref.refs64()[:2], ref_index=[1, -1, 0], centres=glob_ref.centres(), saturation=True) if kind == "rgb_ref" else {}
        x.forward_async_rgb(slot, batch, hints[:3], dst, ab3, out=out, **kw)
        x.wait(slot)
        return [dst[i] for i in range(3)], {"ab": ab3}, [d] * 3
    if kind == "images":
        res = x.forward_async_images(slot, srcs, hints, _outs(x, srcs, out, slot), ab, out=out)
    elif kind == "images_ref":
        res = x.forward_async_images(slot, srcs, hints, _outs(x, srcs, out, slot), ab, out=out, refs=glob_ref.refs64()[:2],
                                     ref_index=[1, -1, 0, 1, 0, -1, 1, 0][:n], centres=glob_ref.centres())
    elif kind == "eval":
        sse, cols, res = x.forward_async_eval(slot, srcs, [None if i % 3 == 0 else RECTS[i % 3:] for i in range(n)], _outs(x, srcs, out, slot), ab,
                                              mode="reveal", out=out)
        ex.update(sse=sse, colours=cols)
    elif kind in ("dist", "dist_score"):
        c = _grid529()
        score = dict(centres=c, nn=2, sigma=5.0, ranks=(1, 5)) if kind == "dist_score" else None
        db = x.forward_async_dist(slot, srcs, hints, _outs(x, srcs, out, slot), ab, out=out, want_sse=True, peaks=3, radius=2, skip_hints=True,
                                  queries="peaks", K=4, N_draws=64, seed=40, centres=c, want_entropy=True, score=score)
        res = db.out_rgb
        ex.update(sse=db.sse, peaks=db.peaks, peak_ent=db.peak_ent, entropy=db.entropy, sc=db.sugg_centres, sf=db.sugg_conf)
        if score:
            ex.update(xent=db.score.xent, hits=db.score.hits)
    elif kind in ("gray8", "gray16"):
        planes = [np.ascontiguousarray(s[..., 1] if kind == "gray8" else s[..., 1].astype(np.uint16) * 257) for s in srcs]
        res = x.forward_async_gray(slot, planes, hints, _outs(x, srcs, out, slot), ab, out=out)
    elif kind == "layers":
        rs = np.random.RandomState(3)
        lays = [None if i % 2 else np.ascontiguousarray(rs.randint(0, 256, (9 + 5 * i, 12 + 3 * i, 4)).astype(np.uint8)) for i in range(n)]
        res, cells = x.forward_async_layers(slot, srcs, lays, [None if h is None else [r[:4] + (200.0, 30.0, 90.0) for r in h] for h in hints],
                                            _outs(x, srcs, out, slot), ab, out=out, mode="rgb")
        ex.update(cells=cells)
    else:
        raise AssertionError(kind)
    x.wait(slot)
    return list(res), ex, _dims(srcs, out)


def _same_extras(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        if a[k] is None:
            assert b[k] is None
            continue
        np.testing.assert_array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8), err_msg="%s: %s" % (what, k))


KINDS = ["rgb", "rgb_ref", "images", "images_ref", "eval", "dist", "dist_score", "gray8", "gray16", "layers"]


@pytest.mark.parametrize("out", ["net", "source"])
@pytest.mark.parametrize("kind", KINDS)
def test_pipelined_call_returns_the_rule_of_its_rgb_images(e, eg, ed, kind, out):
    x = eg if kind.endswith("_ref") else ed if kind.startswith("dist") else e
    srcs = _sources()
    try:
        x.set_batch_output("rgb")
        rgbs, extras, dims = _call(x, kind, 0, out, srcs)
        rgbs, extras = [np.array(r) for r in rgbs], {k: (None if v is None else np.array(v)) for k, v in extras.items()}
        assert [r.shape for r in rgbs] == [d + (3,) for d in dims]
        for slot, (fmt, matrix) in zip((1, 0), PAIRS):                                  # both slots
            x.set_batch_output(fmt, matrix)
            blocks, ex, _ = _call(x, kind, slot, out, srcs)
            for i, (b, r) in enumerate(zip(blocks, rgbs)):
                _check_block(b, r, fmt, matrix, "%s %s image %d (%dx%d) %s/%s" % (kind, out, i, r.shape[0], r.shape[1], fmt, matrix))
            _same_extras(ex, extras, "%s %s %s" % (kind, out, fmt))                    # out_ab, sse, colours, taps, scores, cells: bit for bit
        # after switching back every byte is what it was before the first YCbCr call
        x.set_batch_output("rgb")
        again, ex, _ = _call(x, kind, 1, out, srcs)
        for a, r in zip(again, rgbs):
            np.testing.assert_array_equal(np.asarray(a), r)
        _same_extras(ex, extras, "%s %s rgb again" % (kind, out))
    finally:
        x.set_batch_output("rgb")


def test_with_the_antialias_filter_and_joint_upsampling(e):
    srcs = _sources()
    try:
        e.set_batch_upsample("joint")
        e.set_ingest_filter("antialias")
        rgbs, extras, _ = _call(e, "images", 0, "source", srcs)
        rgbs, extras = [np.array(r) for r in rgbs], {k: np.array(v) for k, v in extras.items()}
        e.set_batch_upsample("linear")
        e.set_ingest_filter("bilinear")
        plain, _, _ = _call(e, "images", 1, "source", srcs)
        assert any((np.asarray(p) != r).any() for p, r in zip(plain, rgbs))            # the two settings were in force
        e.set_batch_upsample("joint")
        e.set_ingest_filter("antialias")
        e.set_batch_output("nv12", "jfif")
        blocks, ex, _ = _call(e, "images", 1, "source", srcs)
        for i, (b, r) in enumerate(zip(blocks, rgbs)):
            _check_block(b, r, "nv12", "jfif", "image %d" % i)
        _same_extras(ex, extras, "joint + antialias")
    finally:
        e.set_batch_output("rgb")
        e.set_batch_upsample("linear")
        e.set_ingest_filter("bilinear")


def test_two_batches_in_flight_keep_their_own_format_and_the_generator_yields_planes(e):
    srcs = _sources()
    hints = _hint_lists(len(srcs))
    try:
        rgb_src, rgb_net = e.forward_async_images(0, srcs, hints, out="source"), e.forward_async_images(1, srcs[::-1], hints, out="net")
        e.wait(0)
        e.wait(1)
        rgb_src, rgb_net = [np.array(r) for r in rgb_src], [np.array(r) for r in rgb_net]
        e.set_batch_output("i420", "jfif")
        a = e.forward_async_images(0, srcs, hints, out="source")
        e.set_batch_output("nv12", "bt709")                                            # slot 0 is in flight: it keeps I420 / JFIF
        b = e.forward_async_images(1, srcs[::-1], hints, out="net")
        e.set_batch_output("rgb")
        e.wait(0)
        e.wait(1)
        for i in range(len(srcs)):
            _check_block(a[i], rgb_src[i], "i420", "jfif", "slot 0 image %d" % i)
            _check_block(b[i], rgb_net[i], "nv12", "bt709", "slot 1 image %d" % i)
        # the generator: a YCC420 per image, in order, the setting back afterwards
        got = list(e.colorize_images(list(zip(srcs, hints)), batch=3, out="source", out_format="i420", out_matrix="bt709"))
        assert len(got) == len(srcs) and e._out_format == "rgb"
        for i, t in enumerate(got):
            assert isinstance(t, engine.YCC420) and t.y.shape == srcs[i].shape[:2]
            _check_block(t.buf, rgb_src[i], "i420", "bt709", "generator image %d" % i)
        back = list(e.colorize_images(list(zip(srcs, hints)), batch=3, out="source"))
        for r, w in zip(back, rgb_src):
            np.testing.assert_array_equal(r, w)
    finally:
        e.set_batch_output("rgb")


# ------------------------------------------------------------------------------------------------ 5. statuses
def test_refused_calls_leave_handle_and_slot_usable(e):
    lib, h, vp = e.lib, e._h, ctypes.c_void_p
    srcs = _sources()[:3]
    want = e.forward_async_images(0, srcs, None, out="source")
    e.wait(0)
    want = [np.array(r) for r in want]
    try:
        # idc_set_batch_output: an unknown value changes nothing
        e.set_batch_output("nv12", "bt709")
        for f, m in [(3, 0), (-1, 0), (1, 2), (2, -1)]:
            assert lib.idc_set_batch_output(h, f, m) == -1
        got = e.forward_async_images(0, srcs, None, out="source")
        e.wait(0)
        for g, w in zip(got, want):
            _check_block(g, w, "nv12", "bt709", "after refused settings")
        # IDC_BATCH_OUT_RGB16 with a YCbCr format: IDC_ERR_UNSUPPORTED before anything is enqueued, and the slot stays usable
        g16 = [np.ascontiguousarray(s[..., 0].astype(np.uint16) * 257) for s in srcs]
        with pytest.raises(N.IdcError) as ei:
            e.forward_async_gray(1, g16, None, out="source", depth=16)
        assert ei.value.status == -7
        got = e.forward_async_images(1, srcs, None, out="source")
        e.wait(1)
        for g, w in zip(got, want):
            _check_block(g, w, "nv12", "bt709", "slot 1 after the refusal")
        e.set_batch_output("rgb")
        full = e.forward_async_gray(1, g16, None, out="source", depth=16)             # with the format off the 16-bit result is served
        e.wait(1)
        assert full[0].dtype == np.uint16
        # idc_fullres_ycc
        e.set_image_rgb(srcs[1], keep_source=True, want_rgb=False, want_lab=False)
        e.set_hints([], mode="ab")
        e.forward_resident(1)
        buf = np.empty(R.nbytes(*srcs[1].shape[:2]), np.uint8)
        p = buf.ctypes.data_as(vp)
        args = (N.IDC_SRC_OUTPUT_AB, N.IDC_INTERP_LINEAR, N.IDC_L_IMAGE)
        assert lib.idc_fullres_ycc(h, 0, *args, N.IDC_OUT_RGB, N.IDC_YCC_JFIF, p) == -1          # RGB is no plane format
        assert lib.idc_fullres_ycc(h, 0, *args, 3, N.IDC_YCC_JFIF, p) == -1
        assert lib.idc_fullres_ycc(h, 0, *args, N.IDC_OUT_I420, 2, p) == -1
        assert lib.idc_fullres_ycc(h, 0, *args, N.IDC_OUT_I420, N.IDC_YCC_JFIF, None) == -1
        assert lib.idc_fullres_ycc(h, 5, *args, N.IDC_OUT_I420, N.IDC_YCC_JFIF, p) == -7          # no resident source in slot 5
        assert lib.idc_fullres_ycc(h, 8, *args, N.IDC_OUT_I420, N.IDC_YCC_JFIF, p) == -6          # the codes of idc_fullres_rgb
        assert lib.idc_fullres_ycc(h, 0, *args, N.IDC_OUT_I420, N.IDC_YCC_JFIF, p) == 0
        _check_block(buf, np.array(e.fullres_rgb("output_ab", "linear", "image")), "i420", "jfif", "after the refusals")
        # idc_rgb_to_ycc420
        table = (N.RefImage * 1)()
        outs = (vp * 1)()
        table[0].rgb, table[0].h, table[0].w = srcs[1].ctypes.data, srcs[1].shape[0], srcs[1].shape[1]
        outs[0] = buf.ctypes.data
        for n in (0, -1, 4097):
            assert lib.idc_rgb_to_ycc420(h, n, table, N.IDC_OUT_I420, N.IDC_YCC_JFIF, outs) == -6
        assert lib.idc_rgb_to_ycc420(h, 1, None, N.IDC_OUT_I420, N.IDC_YCC_JFIF, outs) == -1
        assert lib.idc_rgb_to_ycc420(h, 1, table, N.IDC_OUT_RGB, N.IDC_YCC_JFIF, outs) == -1
        assert lib.idc_rgb_to_ycc420(h, 1, table, N.IDC_OUT_NV12, 7, outs) == -1
        table[0].h = 16385
        assert lib.idc_rgb_to_ycc420(h, 1, table, N.IDC_OUT_I420, N.IDC_YCC_JFIF, outs) == -1
        table[0].h = srcs[1].shape[0]
        outs[0] = None
        assert lib.idc_rgb_to_ycc420(h, 1, table, N.IDC_OUT_I420, N.IDC_YCC_JFIF, outs) == -1
        outs[0] = buf.ctypes.data
        assert lib.idc_rgb_to_ycc420(h, 1, table, N.IDC_OUT_NV12, N.IDC_YCC_BT709_VIDEO, outs) == 0
        _check_block(buf, srcs[1], "nv12", "bt709", "conversion after the refusals")
    finally:
        e.set_batch_output("rgb")


# ------------------------------------------------------------------------------------------------ 6. the wrapper
def test_wrapper_get_img_fullres_ycc(make_sd):
    from interactive_deep_colorization_amd import api, workloads
    src = ragged_ref.image(150, 201, 7)
    hab, hm = workloads.hints_config2(64, 5, 3, 0)
    model = api.ColorizeImageTorch(Xd=64, precision="bf16")
    model.prep_net(path="", state_dict=make_sd(0, "he"))
    model.set_image(np.ascontiguousarray(src[:64, :64]))                        # the host route: no source on the device, no device getter
    model.net_forward(hab, hm)
    with pytest.raises(RuntimeError):
        model.get_img_fullres_ycc()
    model.set_image_device(src)
    model.net_forward(hab, hm)
    rgb = np.array(model.get_img_fullres())
    assert rgb.shape == (150, 201, 3)
    got = model.get_img_fullres_ycc()
    assert isinstance(got, engine.YCC420) and got.y.shape == (150, 201) and got.cb.shape == (75, 101)
    _check_block(got.buf, rgb, "i420", "jfif", "wrapper, linear")
    got = model.get_img_fullres_ycc(format="nv12", matrix="bt709", interp="joint")
    assert isinstance(got, engine.NV12)
    _check_block(got.buf, np.array(model.get_img_fullres_joint()), "nv12", "bt709", "wrapper, joint")
    model.net.close()
