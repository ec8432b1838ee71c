"""GPU checks of the joint bilateral ab upsampling: idc_fullres_ab, idc_fullres_rgb with IDC_INTERP_JOINT, idc_set_joint_upsample and
idc_set_batch_upsample, through HipColorizer.  The reference is tests/joint_ref.py (the rule in numpy float64, colours through the oracle)
and, for the pipelined calls, the blocking route per image -- never the call under test.

Bars:
  ab        1e-9 absolute against joint_ref, the project's bar for float64 colour arithmetic: a pixel's sums are at most 81 products of
            weights <= 1 with |ab| <= 128, and exp differs in its last bits (2^-52 relative) between the two sides, so 1e-9 leaves more than
            three decades.  The same bar for linear / nearest against scipy's zoom: the same float64 expressions on both sides.
  cubic     2e-3 against the oracle's cv2 restatement.  cv2's Keys coefficients are float32 Horner polynomials; the device contracts each
            step into an FMA and numpy rounds product and sum separately, so a step differs by at most half an ulp of its product (2^-24,
            2^-22, 2^-22 for products below 1.5, 6 and 7.5), carried through the later steps' factors (x + 1) <= 2: 4 * 2^-24 + 2 * 2^-22 +
            2^-22 = 2^-20 per coefficient, three times that for c3 = 1 - c0 - c1 - c2, 6e-6 for the four of an axis.  The result is
            sum cy * sum cx * v with sum |c| <= 1.25 and |v| <= 128: 128 * 2 * 1.25 * 6e-6 = 1.9e-3.  (Exact where the coefficients are
            0 and 1: the net size.)  The cubic rule itself is not this change's; the check is that idc_fullres_ab hands it the right pixel.
  rgb       at most one uint8 level everywhere (a last bit of pow can move a value across a truncation boundary)
  pipelined bit for bit the blocking route: one kernel, the same float64 operands
  step edge joint_ref.STEP_BOUND / LINEAR_MISS, as in tests/test_joint_cpu.py
Shapes: handles of 32 x 48 (bf16) and 64 x 64 (fp32, bf16), max_batch 8; sources joint_ref.SIZES: 1 x 1, one row, one column, smaller than
the net (13 x 17: a tile's footprint exceeds the LDS block, the global-tap branch), the net size, 37 x 41 and 233 x 351 (7.3x: several tiles,
ragged last tiles on both axes); batches of tests/ragged_ref.py's sizes, whose image starts cover every residue mod 4."""
import ctypes

import numpy as np
import pytest

import ingest_ref
import joint_ref as J
import ragged_ref as R
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import engine
from oracle import colorspace as ocs
from oracle import display

pytestmark = pytest.mark.gpu

TOL = 1e-9
CUBIC_TOL = 2e-3
_ENG = {}


@pytest.fixture(scope="module")
def eng(make_sd):
    def get(H, W, precision="bf16"):
        key = (H, W, precision)
        if key not in _ENG:
            e = engine.HipColorizer(H, W, max_batch=8, precision=precision)
            e.load_state_dict(make_sd(0, "he"))
            _ENG[key] = e
        return _ENG[key]
    yield get
    for e in _ENG.values():
        e.close()
    _ENG.clear()


def _status(ei):
    return ei.value.status


def _resident(e, src, hints):
    """Ingest, hint and run one image on slot 0 -> the three pairs of net-size planes the sources name."""
    e.set_image_rgb(src, keep_source=True, want_rgb=False, want_lab=False)
    e.set_hints(hints, mode="ab")
    raw, _, lab_q = e.forward_resident(1)
    in_ab, _ = e.hint_planes(0)
    assert np.isfinite(raw).all() and np.abs(raw).max() > 0
    return {"output_ab": np.array(lab_q[0, 1:]), "output_ab_raw": np.array(raw[0]), "input_ab": np.array(in_ab)}


# ------------------------------------------------------------------------------------------------ 1. the ab map
@pytest.mark.parametrize("size", J.SIZES)
def test_fullres_ab_joint_matches_the_rule(eng, size):
    e = eng(J.H, J.W)
    src = J.source(*size)
    planes = _resident(e, src, J.HINTS)
    np.testing.assert_array_equal(planes["input_ab"], J.raster(J.HINTS))        # what the CPU file ran its checks on
    L, L_lo = J.source_l(src), J.guide(src)
    worst = 0.0
    try:
        for params in J.PARAMS:
            e.set_joint_upsample(*params)
            for name, ab_lo in planes.items():
                want, den = J.joint_ab(L, ab_lo[0], ab_lo[1], L_lo, *params, want_den=True)
                assert den >= 1e-12, (size, params, name, den)
                got = e.fullres_ab(name, "joint")
                assert got.shape == (2,) + size and got.dtype == np.float64
                err = float(np.abs(got - want).max())
                worst = max(worst, err)
                assert err <= TOL, (size, params, name, err)
    finally:
        e.set_joint_upsample()
    print("%dx%d: largest ab error %.3e over %d parameter sets x 3 sources" % (size[0], size[1], worst, len(J.PARAMS)))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_fullres_ab_joint_on_the_64x64_handle(eng, precision):
    e = eng(64, 64, precision)
    for size in [(37, 41), (150, 201)]:                                         # smaller than this net: global taps; 2.3x / 3.1x: staged
        src = J.source(*size)
        planes = _resident(e, src, J.HINTS)
        L, L_lo = J.source_l(src), J.guide(src, 64, 64)
        for name, ab_lo in planes.items():
            err = float(np.abs(e.fullres_ab(name, "joint") - J.joint_ab(L, ab_lo[0], ab_lo[1], L_lo)).max())
            print("%s %dx%d %s: ab error %.3e" % (precision, size[0], size[1], name, err))
            assert err <= TOL, (size, name, err)


@pytest.mark.parametrize("size", [(1, 1), (1, 300), (13, 17), (32, 48), (233, 351)])
def test_fullres_ab_of_the_other_interps_matches_their_references(eng, size):
    e = eng(J.H, J.W)
    src = J.source(*size)
    planes = _resident(e, src, J.HINTS)
    for name, ab_lo in planes.items():
        want = {"linear": ingest_ref.zoom_to(ab_lo, size[0], size[1], 1), "nearest": ingest_ref.zoom_to(ab_lo, size[0], size[1], 0),
                "cubic": np.stack([display.resize_cubic_cv2(p.astype(np.float64), size[0], size[1]) for p in ab_lo])}
        for interp, w in want.items():
            err = float(np.abs(e.fullres_ab(name, interp) - w).max())
            print("%dx%d %s %s: ab error %.3e" % (size[0], size[1], name, interp, err))
            assert err <= (CUBIC_TOL if interp == "cubic" else TOL), (size, name, interp, err)
    np.testing.assert_array_equal(e.fullres_ab("no_ab", "joint"), np.zeros((2,) + size))


# ------------------------------------------------------------------------------------------------ 2. the image
def _levels(got, want):
    return int(np.abs(got.astype(np.int32) - want.astype(np.int32)).max())


@pytest.mark.parametrize("size", [(1, 1), (300, 1), (13, 17), (37, 41), (233, 351)])
def test_fullres_rgb_joint(eng, size):
    e = eng(J.H, J.W)
    src = J.source(*size)
    planes = _resident(e, src, J.HINTS)
    L, L_lo = J.source_l(src), J.guide(src)
    names = ["output_ab"] if size[0] * size[1] > 10000 else list(planes)        # (the oracle's Lab -> RGB is a Python loop per pixel)
    for name in names:
        ab_lo = planes[name]
        got = e.fullres_rgb(name, "joint", "image")
        assert got.shape == src.shape and got.dtype == np.uint8
        d_ref = _levels(got, J.joint_rgb(src, ab_lo[0], ab_lo[1], L_lo))
        assert d_ref <= 1, (size, name, d_ref)
        if size[0] * size[1] <= 10000:
            d_own = _levels(got, ocs.lab2rgb_transpose(L[None], e.fullres_ab(name, "joint")))
            assert d_own <= 1, (size, name, d_own)
    np.testing.assert_array_equal(e.fullres_rgb("no_ab", "joint", "image"), e.fullres_rgb("no_ab", "linear", "image"))


# ------------------------------------------------------------------------------------------------ 3. the step edge
@pytest.mark.parametrize("offset", [0, 2])
def test_step_edge_on_the_device(offset):
    e = engine.HipColorizer(J.H, J.W, max_batch=1, precision="bf16")            # no weights: input_ab is painted by the hints
    src, edge = J.step_source(offset)
    e.set_image_rgb(src, keep_source=True, want_rgb=False, want_lab=False)
    e.set_hints(J.STEP_HINTS, mode="ab")
    want = np.where(np.arange(src.shape[1]) < edge, J.STEP_AB[0], J.STEP_AB[1])[None, None, :]
    j_err = float(np.abs(e.fullres_ab("input_ab", "joint") - want).max())
    l_err = float(np.abs(e.fullres_ab("input_ab", "linear") - want).max())
    print("edge offset %d: device joint off by %.4f, device linear by %.2f" % (offset, j_err, l_err))
    assert j_err <= J.STEP_BOUND
    assert l_err > J.LINEAR_MISS
    e.close()


# ------------------------------------------------------------------------------------------------ 4. pipelined
_BLOCK = {}


def _blocking(e, key, img, hints, interp, params=J.DEFAULT):
    """The blocking route of one image -> its source-size image by ``interp``; made once per case and not written to."""
    k = (key, img.shape, img.tobytes(), repr(hints), interp, params)
    if k not in _BLOCK:
        e.set_image_rgb(img, keep_source=True, want_rgb=False, want_lab=False)
        e.set_hints(hints or [], mode="ab")
        e.forward_resident(1)
        e.set_joint_upsample(*params)
        out = np.array(e.fullres_rgb("output_ab", interp, "image"))
        e.set_joint_upsample()
        out.setflags(write=False)
        _BLOCK[k] = out
    return _BLOCK[k]


def _ragged(e, lst, seed):
    return [R.image(sh, sw, seed + j) for j, (sh, sw) in enumerate(R.sizes(lst, e.H, e.W))]


def _hint_lists(n):
    return [None if i % 3 == 0 else J.HINTS[i % 4:] for i in range(n)]


@pytest.mark.parametrize("H,W,precision", [(64, 64, "bf16"), (32, 48, "bf16"), (64, 64, "fp32")])
def test_pipelined_joint_equals_the_blocking_route(eng, H, W, precision):
    e = eng(H, W, precision)
    key = (H, W, precision)
    residues = set()
    e.set_batch_upsample("joint")
    try:
        images = _ragged(e, R.MIXED, 700)
        hints = _hint_lists(len(images))
        for slot, order in ((0, 1), (1, -1)):                                   # reversed: the image starts fall on other residues mod 4
            imgs, hl = images[::order], hints[::order]
            residues |= set(int(s) % 4 for s in R.starts([a.shape[:2] for a in imgs])[:-1])
            outs = e.forward_async_images(slot, [np.ascontiguousarray(a) for a in imgs], hl, out="source")
            e.wait(slot)
            for i, (img, h, got) in enumerate(zip(imgs, hl, outs)):
                np.testing.assert_array_equal(got, _blocking(e, key, img, h, "joint"), err_msg="slot %d image %d %s" % (slot, i, img.shape))
        assert residues == {0, 1, 2, 3}, residues
        for slot, (sh, sw) in ((0, (37, 41)), (1, (5, 7))):                     # the same-size call: 3 x 1517 and 3 x 35 pixels
            batch = np.ascontiguousarray(np.stack([R.image(sh, sw, 720 + j) for j in range(3)]))
            dst = np.full(batch.shape, 7, np.uint8)
            e.forward_async_rgb(slot, batch, hints[:3], dst, out="source")
            e.wait(slot)
            for i in range(3):
                np.testing.assert_array_equal(dst[i], _blocking(e, key, batch[i], hints[i], "joint"), err_msg="same-size slot %d image %d" % (slot, i))
    finally:
        e.set_batch_upsample("linear")


def test_two_batches_in_flight_keep_their_own_settings(eng):
    e = eng(64, 64)
    key = (64, 64, "bf16")
    images = _ragged(e, R.THREE_BOUNDARIES, 740)
    hints = _hint_lists(len(images))
    narrow = (1, 0.5, 2.0)
    try:
        e.set_batch_upsample("joint")
        e.set_joint_upsample(*narrow)
        a = e.forward_async_images(0, images, hints, out="source")
        e.set_joint_upsample()                                                  # the defaults ...
        b_src = [np.ascontiguousarray(x) for x in images]
        e.set_batch_upsample("linear")                                          # ... and linear, while slot 0 is in flight
        b = e.forward_async_images(1, b_src, hints, out="source")
        e.set_batch_upsample("joint")
        e.wait(0); e.wait(1)
        c = e.forward_async_images(0, images, hints, out="source")
        e.wait(0)
    finally:
        e.set_batch_upsample("linear")
        e.set_joint_upsample()
    for i, img in enumerate(images):
        np.testing.assert_array_equal(a[i], _blocking(e, key, img, hints[i], "joint", narrow), err_msg="slot 0, narrow joint, image %d" % i)
        np.testing.assert_array_equal(b[i], _blocking(e, key, img, hints[i], "linear"), err_msg="slot 1, linear, image %d" % i)
        np.testing.assert_array_equal(c[i], _blocking(e, key, img, hints[i], "joint"), err_msg="slot 0 again, default joint, image %d" % i)
    assert any(not np.array_equal(a[i], c[i]) for i in range(len(images)))


def test_evaluation_scores_the_joint_image_and_linear_comes_back_unchanged(make_sd):
    e = engine.HipColorizer(64, 64, max_batch=8, precision="bf16")              # a fresh handle: its setting was never touched
    e.load_state_dict(make_sd(0, "he"))
    key = ("fresh", 64, 64)
    images = _ragged(e, R.MIXED, 760)
    hints = _hint_lists(len(images))
    items = [(img, h) for img, h in zip(images, hints)]
    before = [np.array(x) for x in e.colorize_images(items, batch=4)]
    before_sse = [s for _, s in e.evaluate_images(items, batch=4, out="source", mode="ab")]
    joint = [np.array(x) for x in e.colorize_images(items, batch=4, upsample="joint")]
    joint_sse = [s for _, s in e.evaluate_images(items, batch=4, out="source", mode="ab", upsample="joint")]
    assert e._batch_upsample == "linear"
    after = [np.array(x) for x in e.colorize_images(items, batch=4)]
    after_sse = [s for _, s in e.evaluate_images(items, batch=4, out="source", mode="ab")]
    for i, img in enumerate(images):
        np.testing.assert_array_equal(joint[i], _blocking(e, key, img, hints[i], "joint"), err_msg="image %d" % i)
        np.testing.assert_array_equal(before[i], _blocking(e, key, img, hints[i], "linear"), err_msg="image %d" % i)
        np.testing.assert_array_equal(after[i], before[i])
        np.testing.assert_array_equal(after_sse[i], before_sse[i])
        for got, out in ((joint_sse[i], joint[i]), (before_sse[i], before[i])):
            d = out.astype(np.int64) - img.astype(np.int64)
            want = [sum(int(v) * int(v) for v in d[..., c].ravel()) for c in range(3)]      # Python integers
            assert [int(v) for v in got] == want, (i, got, want)
    assert any(not np.array_equal(j, b) for j, b in zip(joint, before))
    e.close()


def test_wrapper_get_img_fullres_joint(make_sd):
    from interactive_deep_colorization_amd import api, workloads
    src = J.source(150, 201)
    hab, hm = workloads.hints_config2(64, 5, 3, 0)
    model = api.ColorizeImageTorch(Xd=64, precision="bf16")
    model.prep_net(path="", state_dict=make_sd(0, "he"))
    model.set_image(np.ascontiguousarray(src[:64, :64]))                        # the host route: no source on the device, no joint getter
    model.net_forward(hab, hm)
    with pytest.raises(RuntimeError):
        model.get_img_fullres_joint()
    model.set_image_device(src)
    model.net_forward(hab, hm)
    got = model.get_img_fullres_joint()
    assert got.shape == src.shape and got.dtype == np.uint8
    assert model._src_resident
    np.testing.assert_array_equal(got, model.net.fullres_rgb("output_ab", "joint", "image"))
    linear = np.array(model.get_img_fullres())                                  # the reference's getter is what it was
    ab_lo = np.array(model.output_ab)                                           # the refreshed map, float64
    assert _levels(got, J.joint_rgb(src, ab_lo[0], ab_lo[1], J.guide(src, 64, 64))) <= 1
    assert _levels(linear, ingest_ref.fullres(src, ab_lo, 1)) <= 1
    model.net.close()


# ------------------------------------------------------------------------------------------------ 5. statuses
def test_statuses_and_refused_calls_change_nothing(eng):
    e = eng(J.H, J.W)
    lib, h, vp = e.lib, e._h, ctypes.c_void_p
    src = J.source(37, 41)
    _resident(e, src, J.HINTS)
    ref_ab = np.array(e.fullres_ab("output_ab", "joint"))
    nan, inf = float("nan"), float("inf")
    for args in [(0, 1.0, 8.0), (5, 1.0, 8.0), (-1, 1.0, 8.0), (2, 0.2, 8.0), (2, 8.5, 8.0), (2, nan, 8.0), (2, inf, 8.0), (2, 1.0, 0.4),
                 (2, 1.0, 101.0), (2, 1.0, nan), (2, 1.0, -inf)]:
        assert lib.idc_set_joint_upsample(h, args[0], args[1], args[2]) == -1, args
    np.testing.assert_array_equal(e.fullres_ab("output_ab", "joint"), ref_ab)   # the parameters are still the defaults
    for args in [(1, 0.25, 0.5), (4, 8.0, 100.0), (2, 1.0, 8.0)]:               # the corners of the ranges are inside
        assert lib.idc_set_joint_upsample(h, args[0], args[1], args[2]) == 0, args
    for interp in (N.IDC_INTERP_CUBIC, N.IDC_INTERP_NEAREST, 4, -1):
        assert lib.idc_set_batch_upsample(h, interp) == -1, interp
    with pytest.raises(ValueError):
        e.set_batch_upsample("cubic")
    assert e._batch_upsample == "linear"
    img = np.ascontiguousarray(src)
    got = e.forward_async_images(0, [img], [J.HINTS], out="source")
    e.wait(0)
    np.testing.assert_array_equal(got[0], _blocking(e, (J.H, J.W, "bf16"), img, J.HINTS, "linear"))       # ... and the batches are still linear
    assert lib.idc_set_batch_upsample(h, N.IDC_INTERP_JOINT) == 0 and lib.idc_set_batch_upsample(h, N.IDC_INTERP_LINEAR) == 0
    _resident(e, src, J.HINTS)
    rgb = np.zeros(src.shape, np.uint8)
    ab = np.zeros((2,) + src.shape[:2], np.float64)
    p_rgb, p_ab = rgb.ctypes.data_as(vp), ab.ctypes.data_as(vp)
    J3 = N.IDC_INTERP_JOINT
    assert lib.idc_fullres_rgb(h, 0, N.IDC_SRC_OUTPUT_AB, J3, N.IDC_L_MASK50, p_rgb) == -1                # the joint mode needs IDC_L_IMAGE
    assert lib.idc_fullres_rgb(h, 0, N.IDC_SRC_OUTPUT_AB, 4, N.IDC_L_IMAGE, p_rgb) == -1                  # interp beyond 3
    assert lib.idc_fullres_rgb(h, 0, N.IDC_SRC_OUTPUT_AB, J3, N.IDC_L_IMAGE, None) == -1
    assert lib.idc_fullres_rgb(h, 0, N.IDC_SRC_OUTPUT_AB, J3, N.IDC_L_IMAGE, p_rgb) == 0
    assert lib.idc_upsample_lab2rgb(h, 0, N.IDC_SRC_OUTPUT_AB, J3, 37, 41, p_ab, p_rgb) == -1             # no guide there: still refused
    assert lib.idc_fullres_ab(h, 0, 4, J3, p_ab) == -1                                                    # unknown source
    assert lib.idc_fullres_ab(h, 0, N.IDC_SRC_OUTPUT_AB, 4, p_ab) == -1 and lib.idc_fullres_ab(h, 0, N.IDC_SRC_OUTPUT_AB, -1, p_ab) == -1
    assert lib.idc_fullres_ab(h, 0, N.IDC_SRC_OUTPUT_AB, J3, None) == -1
    assert lib.idc_fullres_ab(h, 8, N.IDC_SRC_OUTPUT_AB, J3, p_ab) == -6                                  # slot outside the handle
    e.set_image_rgb(src, img=1, want_rgb=False, want_lab=False)                                           # slot 1: ingested, its source not kept
    assert lib.idc_fullres_ab(h, 1, N.IDC_SRC_NO_AB, J3, p_ab) == -7
    assert lib.idc_fullres_ab(h, 0, N.IDC_SRC_OUTPUT_AB, J3, p_ab) == 0
    np.testing.assert_array_equal(ab, ref_ab)                                                             # ... after all the refusals
    e.set_image_rgb(np.stack([src, src]), keep_source=True, want_rgb=False, want_lab=False)
    assert lib.idc_fullres_ab(h, 1, N.IDC_SRC_OUTPUT_AB, J3, p_ab) == -7                                  # the last forward did not cover slot 1
    assert lib.idc_fullres_ab(h, 1, N.IDC_SRC_INPUT_AB, J3, p_ab) == 0
    e.set_image_l(np.zeros((J.H, J.W), np.float32), img=0)                                                # the guide's plane is gone, and so is the source
    assert lib.idc_fullres_ab(h, 0, N.IDC_SRC_INPUT_AB, J3, p_ab) == -7
    with pytest.raises(N.IdcError) as ei:
        e.fullres_ab("input_ab", "joint", img=0)
    assert _status(ei) == -7
