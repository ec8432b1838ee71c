"""GPU checks of image ingestion on the device: idc_set_image_rgb (uint8 RGB -> net-size RGB, Lab and the resident L plane, one
launch for all images) and idc_fullres_rgb (the full-resolution getters from the resident uint8 source), through HipColorizer and the
wrapper's load_image_device.  The reference is tests/ingest_ref.py: colorspace.resize_bilinear_u8, the oracle's rgb2lab /
lab2rgb_transpose and scipy.ndimage.zoom -- never the code under test.

Bars:
  rgb_net   bit-identical to the reference resize: every operation of the rule is one correctly rounded IEEE double operation, in the
            same order on both sides (contraction is off in the kernel), and the clamped taps are the same integers
  lab_net   1e-9 abs against the reference rgb2lab of that rgb_net: pow / cbrt differ in their last bits (~2^-52 relative), amplified
            by at most 500 (the a channel), i.e. ~1e-13; three orders of margin, far below the step between neighbouring uint8 colours
  L plane   out_ab of forward_resident bit-identical to the one after set_image_l(float32(lab_net[0] - 50)) of the call's own lab_net
  fullres   the bar of test_upsample_lab2rgb_display_and_fullres: at most one uint8 level on at most 2e-4 of the values (the same
            float64 arithmetic on both sides; pow / cbrt last bits can move a value across a truncation boundary).  The (1,257) source
            has 771 values and the (64,64) one 12 288: there the fraction allows 0 and 2 values.
Shapes: 64 x 64 and 40 x 72 handles; sources (1,1) (every tap clamped), (3,500), (37,41) (up-scaling), the handle's own size (the
identity), (130,97), (203,187) (odd, more than one workgroup); full resolution (1,257) (an output dimension of 1, 257 = 64 * 4 + 1: the
scalar tail), (64,64), (203,187) and (300,280) (pixel counts with remainders 1, 0, 1, 0 modulo 4 and 3 through (37,41) in the wrapper
test)."""
import ctypes

import numpy as np
import pytest

import ingest_ref
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import api, engine, workloads

pytestmark = pytest.mark.gpu

LAB_TOL = 1e-9
FRAC = 2e-4
HINTS = [(5, 7, 11, 13, 30.0, -40.0), (20, 30, 22, 33, -25.0, 55.0), (33, 2, 39, 20, 60.0, 10.0)]     # (y0, x0, y1, x1, a, b): inside 40 x 72 too


def _status(excinfo):
    return excinfo.value.status


def _check_u8(got, want, what):
    mx, frac = ingest_ref.close_u8(got, want)
    print("%s: max level difference %d on %.3g of %d values" % (what, mx, frac, want.size))
    assert got.shape == want.shape and got.dtype == np.uint8
    assert mx <= 1 and frac <= FRAC, (what, mx, frac)


# ------------------------------------------------------------------------------------------------ 1. ingest
@pytest.mark.parametrize("H,W", [(64, 64), (40, 72)])
def test_ingest_matches_the_reference_resize_and_rgb2lab(H, W):
    e = engine.HipColorizer(H, W, max_batch=4, precision="bf16")               # no weights needed: ingestion runs no layer
    sizes = [(1, 1), (3, 500), (37, 41), (H, W), (130, 97), (203, 187)]
    if (H, W) != (64, 64):
        sizes.append((64, 64))
    for k, (sh, sw) in enumerate(sizes):
        batch = np.stack([ingest_ref.source_image(sh, sw, 10 * k + j) for j in range(3)])
        want_rgb = np.stack([ingest_ref.net_rgb(s, H, W) for s in batch])
        want_lab = np.stack([ingest_ref.net_lab(r) for r in want_rgb])
        rgb3, lab3 = e.set_image_rgb(batch, img=1)
        rgb1, lab1 = e.set_image_rgb(batch[0], img=1)
        assert rgb3.shape == (3, H, W, 3) and lab3.shape == (3, 3, H, W) and rgb1.shape == (1, H, W, 3) and lab1.shape == (1, 3, H, W)
        np.testing.assert_array_equal(rgb3, want_rgb, err_msg="rgb_net of a %dx%d source" % (sh, sw))
        err = float(np.abs(lab3 - want_lab).max())
        print("source %dx%d -> %dx%d: lab_net max abs error %.3e" % (sh, sw, H, W, err))
        assert err <= LAB_TOL, (sh, sw, err)
        np.testing.assert_array_equal(rgb1[0], rgb3[0])                         # a slot's result does not depend on n
        np.testing.assert_array_equal(lab1[0], lab3[0])
        if (sh, sw) == (H, W):
            np.testing.assert_array_equal(rgb3, batch)                          # set_image's case: not resized
    # the outputs are optional
    assert e.set_image_rgb(batch[0], img=3, want_rgb=False, want_lab=False) == (None, None)
    only_rgb, none = e.set_image_rgb(batch[0], img=0, want_lab=False)
    assert none is None
    np.testing.assert_array_equal(only_rgb[0], want_rgb[0])
    e.close()


# ------------------------------------------------------------------------------------------------ 2. the resident L plane
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_ingested_l_plane_is_the_one_set_image_l_would_upload(make_sd, precision):
    e = engine.HipColorizer(64, 64, max_batch=1, precision=precision)
    e.load_state_dict(make_sd(0, "he"))
    src = ingest_ref.source_image(130, 97, 6)
    _, lab = e.set_image_rgb(src)
    e.set_hints(HINTS, mode="ab")
    got = e.forward_resident(1, want_rgb=False)[0].copy()
    e.set_image_l(np.float32(lab[0, 0] - 50))
    e.set_hints(HINTS, mode="ab")
    want = e.forward_resident(1, want_rgb=False)[0]
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    np.testing.assert_array_equal(got, want)
    e.close()


# ------------------------------------------------------------------------------------------------ 3. full resolution
@pytest.fixture(scope="module")
def net64(make_sd):
    e = engine.HipColorizer(64, 64, max_batch=1, precision="bf16")
    e.load_state_dict(make_sd(0, "he"))
    yield e
    e.close()


@pytest.mark.parametrize("sh,sw", [(203, 187), (64, 64), (1, 257), (300, 280)])
def test_fullres_rgb_matches_the_reference_getters(net64, sh, sw):
    e = net64
    src = ingest_ref.source_image(sh, sw, 2 * (sh + sw))
    e.set_image_rgb(src, keep_source=True, want_rgb=False, want_lab=False)
    e.set_hints(HINTS, mode="ab")
    _, _, lab_q = e.forward_resident(1)
    out_ab = lab_q[0, 1:]                                                       # the refreshed output_ab, float64
    in_ab, in_mask = e.hint_planes(0)
    assert in_mask.any() and not in_mask.all()
    _check_u8(e.fullres_rgb("output_ab", "linear", "image"), ingest_ref.fullres(src, out_ab, 1), "get_img_fullres %dx%d" % (sh, sw))
    _check_u8(e.fullres_rgb("input_ab", "linear", "image"), ingest_ref.fullres(src, in_ab, 1), "get_input_img_fullres %dx%d" % (sh, sw))
    _check_u8(e.fullres_rgb("input_ab", "nearest", "mask50"), ingest_ref.fullres(src, in_ab, 0, mask=in_mask), "get_sup_fullres %dx%d" % (sh, sw))
    _check_u8(e.fullres_rgb("no_ab", "linear", "image"), ingest_ref.fullres(src), "get_img_gray_fullres %dx%d" % (sh, sw))


def test_mask50_uses_the_mask_value_of_the_last_set_hints():
    e = engine.HipColorizer(64, 64, max_batch=2, precision="bf16")
    src = ingest_ref.source_image(37, 41, 8)
    e.set_image_rgb(np.stack([src, src]), keep_source=True, want_rgb=False, want_lab=False)
    e.set_hints(HINTS, mode="ab", img=1, mask_value=110.0)                      # the Caffe nets' mask_mult
    in_ab, in_mask = e.hint_planes(1)
    assert in_mask.max() == 110.0
    _check_u8(e.fullres_rgb("input_ab", "nearest", "mask50", img=1), ingest_ref.fullres(src, in_ab, 0, mask=in_mask, mask_value=110.0), "mask 110")
    black = e.fullres_rgb("input_ab", "nearest", "mask50", img=0)               # slot 0 never had hints: L = 0, a = b = 0
    assert black.shape == src.shape and not black.any()
    e.close()


def test_wrapper_fullres_after_load_image_device_agrees_with_load_image(make_sd, tmp_path):
    from PIL import Image
    src = ingest_ref.source_image(203, 187, 12)
    path = str(tmp_path / "src.png")
    Image.fromarray(src).save(path)
    hab, hm = workloads.hints_config2(64, 5, 3, 0)
    model = api.ColorizeImageTorch(Xd=64, precision="bf16")
    model.prep_net(path="", state_dict=make_sd(0, "he"))
    model.load_image_device(path)
    np.testing.assert_array_equal(model.img_rgb, ingest_ref.net_rgb(src, 64, 64))
    model.net_forward(hab, hm)
    dev_full = model.get_img_fullres()
    dev_gray = model.get_img_gray_fullres()
    assert model._src_resident and model._fullres_lab_pending                   # the device route: no full-resolution Lab was made on the host
    model.load_image(path)
    model.net_forward(hab, hm)
    _check_u8(dev_full, model.get_img_fullres(), "wrapper get_img_fullres")
    _check_u8(dev_gray, model.get_img_gray_fullres(), "wrapper get_img_gray_fullres")
    # the edit-list route: hints on the device only
    hints = [(10 + 7 * i, 6 + 9 * i, 16 + 7 * i, 12 + 9 * i, 30 * i % 256, 200 - 20 * i, 40 + 15 * i) for i in range(5)]
    small = src[:37, :41].copy()                                                # 1517 pixels: remainder 1 modulo 4
    model.load_image_device(_save(tmp_path, small))
    model.net_forward_hints(hints)
    dev_in, dev_sup = model.get_input_img_fullres(), model.get_sup_fullres()
    assert model._src_resident and model._fullres_lab_pending
    model.load_image(_save(tmp_path, small))
    model.net_forward_hints(hints)
    _ = model.input_ab                                                          # read back: the host route from here on
    _check_u8(dev_in, model.get_input_img_fullres(), "wrapper get_input_img_fullres")
    _check_u8(dev_sup, model.get_sup_fullres(), "wrapper get_sup_fullres")
    model.net.close()


def _save(tmp_path, img):
    from PIL import Image
    path = str(tmp_path / ("img_%dx%d.png" % img.shape[:2]))
    Image.fromarray(img).save(path)
    return path


# ------------------------------------------------------------------------------------------------ 4. residency and errors
def test_source_residency_and_argument_errors(make_sd):
    e = engine.HipColorizer(64, 64, max_batch=2, precision="bf16")
    e.load_state_dict(make_sd(0, "he"))
    src = ingest_ref.source_image(37, 41, 3)
    L, ab, mask = workloads.random_batch(1, 64, seed=5, max_points=3, max_p=2)

    def unsupported(img=0):
        with pytest.raises(N.IdcError) as ei:
            e.fullres_rgb("no_ab", "linear", "image", img=img)
        assert _status(ei) == -7, str(ei.value)

    unsupported()                                                               # before any ingest
    e.set_image_rgb(src)
    unsupported()                                                               # ingested without KEEP_SOURCE
    e.set_image_rgb(src, keep_source=True)
    assert e.fullres_rgb("no_ab").shape == (37, 41, 3)
    e.set_image_rgb(src)                                                        # a later call without the flag releases it
    unsupported()
    e.set_image_rgb(np.stack([src, src]), keep_source=True)
    e.set_image_l(np.zeros((64, 64), np.float32), img=0)
    unsupported(0)
    assert e.fullres_rgb("no_ab", img=1).shape == (37, 41, 3)                   # the other slot keeps its source
    e.set_image_rgb(np.stack([src, src]), keep_source=True)
    e.forward(L, ab, mask)                                                      # host L_mc for slot 0 only
    unsupported(0)
    assert e.fullres_rgb("no_ab", img=1).shape == (37, 41, 3)
    with pytest.raises(N.IdcError) as ei:                                       # output_ab of a slot the last forward did not cover
        e.fullres_rgb("output_ab", img=1)
    assert _status(ei) == -7
    with pytest.raises(N.IdcError) as ei:
        e.set_image_rgb(np.stack([src, src]), img=1)                            # img + n > max_batch
    assert _status(ei) == -6
    with pytest.raises(N.IdcError) as ei:
        e.set_image_rgb(src, img=2)
    assert _status(ei) == -6
    assert e.fullres_rgb("no_ab", img=1).shape == (37, 41, 3)                   # refused calls changed nothing
    px = np.zeros(3, np.uint8)
    vp = ctypes.c_void_p
    lib, h = e.lib, e._h
    assert lib.idc_set_image_rgb(h, 0, 1, 0, 5, px.ctypes.data_as(vp), 50.0, 0, None, None) == -1           # src_h = 0
    assert lib.idc_set_image_rgb(h, 0, 1, 1, 16385, px.ctypes.data_as(vp), 50.0, 0, None, None) == -1       # src_w beyond the limit
    assert lib.idc_set_image_rgb(h, 0, 1, 1, 1, px.ctypes.data_as(vp), 50.0, 2, None, None) == -1           # unknown flag bit
    assert lib.idc_set_image_rgb(h, 0, 1, 1, 1, None, 50.0, 0, None, None) == -1                            # null rgb
    assert lib.idc_set_image_rgb(h, 0, 0, 1, 1, px.ctypes.data_as(vp), 50.0, 0, None, None) == -6           # n = 0
    assert lib.idc_fullres_rgb(h, 1, 4, 1, 0, px.ctypes.data_as(vp)) == -1                                  # unknown source
    assert lib.idc_fullres_rgb(h, 1, 3, 1, 2, px.ctypes.data_as(vp)) == -1                                  # unknown l_mode
    assert lib.idc_fullres_rgb(h, 2, 3, 1, 0, px.ctypes.data_as(vp)) == -6                                  # slot outside the handle
    assert lib.idc_set_image_rgb(h, 0, 1, 1, 1, px.ctypes.data_as(vp), 50.0, 0, None, None) == 0            # ... and a 1 x 1 image is fine
    e.close()


# ------------------------------------------------------------------------------------------------ 5. nothing else moved
def test_other_calls_are_unchanged_by_an_ingest_on_another_slot(make_sd):
    from interactive_deep_colorization_amd import color_bins
    e = engine.HipColorizer(64, 64, max_batch=2, precision="bf16")
    e.load_state_dict(make_sd(0, "he"))
    L, ab, mask = workloads.random_batch(1, 64, seed=9, max_points=4, max_p=3)
    ref_img = ingest_ref.source_image(64, 64, 14)
    centres = color_bins.pts_in_hull().astype(np.float32)
    l_out = np.random.RandomState(3).uniform(0, 100, (90, 75))

    def everything():
        out = e.forward(L, ab, mask).copy()
        rgb = e.forward_rgb_lazy(L, ab, mask).copy()
        up = e.upsample_lab2rgb(l_out, "output_ab", "linear").copy()
        hist, sat = e.global_histogram(ref_img, centres)
        return out, rgb, up, hist.copy(), sat.copy()

    before = everything()
    src = ingest_ref.source_image(130, 97, 16)
    e.set_image_rgb(src, img=1, keep_source=True)
    _check_u8(e.fullres_rgb("no_ab", img=1), ingest_ref.fullres(src), "slot 1 gray")
    up_again = e.upsample_lab2rgb(l_out, "output_ab", "linear")                 # the resident result of slot 0 is still the last forward's
    np.testing.assert_array_equal(up_again, before[2])
    after = everything()
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    _check_u8(e.fullres_rgb("no_ab", img=1), ingest_ref.fullres(src), "slot 1 gray, after the forwards on slot 0")
    e.close()
