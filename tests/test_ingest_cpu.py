"""Image ingestion on the device, the parts that need no GPU: the two C-ABI symbols (idc_set_image_rgb, idc_fullres_rgb) exist and
refuse a null handle, and the wrapper's opt-in route (load_image_device / set_image_device and the four full-resolution getters) does its
bookkeeping right against a fake engine whose set_image_rgb is the reference of tests/ingest_ref.py."""
import os
import re

import numpy as np
import pytest

from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import api, colorspace

import ingest_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_declares_exports_and_guards_both_symbols():
    header = open(os.path.join(REPO, "include", "ideepcolor.h")).read()
    declared = set(re.findall(r"\b(idc_[a-z0-9_]+)\s*\(", header))
    lib = N.load()
    for sym in ("idc_set_image_rgb", "idc_fullres_rgb"):
        assert sym in declared and sym in N.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    for name, value in (("IDC_INGEST_KEEP_SOURCE", 1), ("IDC_SRC_NO_AB", 3), ("IDC_L_IMAGE", 0), ("IDC_L_MASK50", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), header), name
        assert getattr(N, name) == value
    assert lib.idc_version() == 2                                  # additive: no bump
    px = np.zeros(3, np.uint8)
    assert lib.idc_set_image_rgb(None, 0, 1, 1, 1, px.ctypes.data, 50.0, 0, None, None) == -1
    assert lib.idc_fullres_rgb(None, 0, 0, 1, 0, px.ctypes.data) == -1


# ------------------------------------------------------------------------------------------------ wrapper, fake engine
class FakeEngine(object):
    """Stands where HipColorizer stands: records what the wrapper asks, computes set_image_rgb with the reference, moves l_serial as the
    engine does (set_image_l, set_image_rgb, fullres_rgb and every forward bump it)."""

    def __init__(self, X):
        self.X = X
        self.calls = []
        self.l_serial = 0
        self.fail_fullres = False

    def set_image_rgb(self, rgb, img=0, l_cent=50., keep_source=False, want_rgb=True, want_lab=True):
        rgb = np.asarray(rgb)
        assert rgb.dtype == np.uint8 and rgb.ndim == 3
        self.calls.append(("set_image_rgb", rgb.shape[:2], img, l_cent, keep_source))
        self.l_serial += 1
        self.source = rgb.copy()
        net = ingest_ref.net_rgb(rgb, self.X, self.X)
        return net[None], ingest_ref.net_lab(net)[None]

    def fullres_rgb(self, source="output_ab", interp="linear", l_mode="image", img=0):
        self.calls.append(("fullres_rgb", source, interp, l_mode, img))
        self.l_serial += 1
        if self.fail_fullres:
            raise N.IdcError(-7, "no resident source")
        return np.full(self.source.shape, 7, np.uint8)

    def set_image_l(self, L_mc, img=0):
        self.calls.append(("set_image_l",))
        self.l_serial += 1

    def set_hints(self, hints, mode="ab", img=0, mask_value=1.0):
        self.calls.append(("set_hints",))

    def hint_planes(self, img=0):
        self.calls.append(("hint_planes",))
        return np.zeros((2, self.X, self.X), np.float32), np.zeros((1, self.X, self.X), np.float32)

    def forward_resident(self, n=1, maskcent=0.0, l_cent=50.0, want_ab=True, want_rgb=True, want_lab=True):
        self.calls.append(("forward_resident",))
        self.l_serial += 1
        X = self.X
        return np.zeros((n, 2, X, X), np.float32), np.zeros((n, X, X, 3), np.uint8), np.zeros((n, 3, X, X))

    def upsample_lab2rgb(self, L_out, source="output_ab", interp="cubic", img=0):
        self.calls.append(("upsample_lab2rgb", source, interp))
        L_out = np.asarray(L_out)
        return np.full(L_out.shape[-2:] + (3,), 9, np.uint8)

    def count(self, name):
        return sum(1 for c in self.calls if c[0] == name)


X = 16


def _model(with_net=True):
    m = api.ColorizeImageTorch(Xd=X)
    if with_net:
        m.net = FakeEngine(X)
        m.net_set = True
    return m


@pytest.fixture()
def png(tmp_path):
    from PIL import Image
    src = ingest_ref.source_image(37, 41, 2)
    path = str(tmp_path / "src.png")
    Image.fromarray(src).save(path)
    return path, src


def _count_rgb2lab(monkeypatch):
    shapes = []
    real = colorspace.rgb2lab

    def counted(rgb):
        shapes.append(np.asarray(rgb).shape)
        return real(rgb)
    monkeypatch.setattr(colorspace, "rgb2lab", counted)
    return shapes


def test_load_image_device_is_one_engine_call_and_defers_the_fullres_lab(png, monkeypatch):
    path, src = png
    host = _model()
    host.load_image(path)
    shapes = _count_rgb2lab(monkeypatch)
    m = _model()
    m.load_image_device(path)
    assert m.net.calls == [("set_image_rgb", (37, 41), 0, 50., True)]
    assert shapes == []                                            # no host rgb2lab at all: neither the net-size nor the full-resolution one
    assert m.img_l_set and m._l_resident and m._src_resident
    np.testing.assert_array_equal(m.img_rgb_fullres, src)
    for name in ("img_rgb", "img_lab", "img_l", "img_ab", "img_lab_mc", "img_l_mc", "_img_l_mc_f32"):
        a, b = getattr(m, name), getattr(host, name)
        assert a.shape == b.shape and a.dtype == b.dtype, name
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-9, err_msg=name)      # (the fake's Lab is the oracle's, the host route's is colorspace's)
    assert shapes == []
    l_full = m.img_l_fullres                                       # first read: now the host conversion runs, once, on the full-resolution copy
    assert shapes == [(37, 41, 3)]
    np.testing.assert_array_equal(l_full, host.img_l_fullres)
    np.testing.assert_array_equal(m.img_ab_fullres, host.img_ab_fullres)
    np.testing.assert_array_equal(m.img_lab_fullres, host.img_lab_fullres)
    assert shapes == [(37, 41, 3)]
    # the L plane is resident: a click uploads nothing
    m.net_forward_hints([(1, 1, 3, 3, 255, 0, 0)])
    assert m.net.count("set_image_l") == 0 and m.net.count("forward_resident") == 1


def test_set_image_device_keeps_the_image_as_it_is(monkeypatch):
    img = ingest_ref.source_image(X, X, 4)
    host = _model()
    host.set_image(img)
    m = _model()
    m.set_image_device(img)
    assert m.net.calls == [("set_image_rgb", (X, X), 0, 50., True)]
    np.testing.assert_array_equal(m.img_rgb, img)
    np.testing.assert_array_equal(m.img_rgb_fullres, img)
    np.testing.assert_allclose(m.img_l_mc, host.img_l_mc, rtol=0, atol=1e-9)
    np.testing.assert_array_equal(m.img_l_fullres, host.img_l_fullres)


def test_device_route_needs_a_net_and_an_engine_that_can():
    m = _model(with_net=False)
    with pytest.raises(RuntimeError):
        m.set_image_device(np.zeros((X, X, 3), np.uint8))

    class OlderEngine(object):                                     # an injected engine without set_image_rgb
        pass
    m.net, m.net_set = OlderEngine(), True
    with pytest.raises(RuntimeError):
        m.set_image_device(np.zeros((X, X, 3), np.uint8))
    assert not m.img_l_set


def test_source_beyond_xfullres_max_takes_the_host_route(png, monkeypatch):
    path, src = png
    host = _model()
    host.Xfullres_max = 30
    host.load_image(path)
    m = _model()
    m.Xfullres_max = 30                                            # the 37 x 41 source is beyond it
    shapes = _count_rgb2lab(monkeypatch)
    m.load_image_device(path)
    assert m.net.calls == [] and not m._src_resident and not m._l_resident
    assert len(shapes) == 2                                        # today's two host conversions
    assert m.img_rgb_fullres.shape == host.img_rgb_fullres.shape and max(m.img_rgb_fullres.shape) <= 30
    np.testing.assert_array_equal(m.img_l_fullres, host.img_l_fullres)
    np.testing.assert_array_equal(m.img_l_mc, host.img_l_mc)


def _with_result(m):
    """A forward whose result and hint planes are 'on the device' for the getters."""
    assert isinstance(m.net_forward_hints([(1, 1, 3, 3, 255, 0, 0)]), np.ndarray)
    assert m._out_on_device() and m._in_on_device()


def test_getters_call_fullres_rgb_with_their_arguments(png):
    path, src = png
    m = _model()
    m.load_image_device(path)
    _with_result(m)
    m.net.calls = []
    for getter, args in ((m.get_img_fullres, ("output_ab", "linear", "image", 0)),
                         (m.get_input_img_fullres, ("input_ab", "linear", "image", 0)),
                         (m.get_sup_fullres, ("input_ab", "nearest", "mask50", 0))):
        out = getter()
        assert out.shape == src.shape and (out == 7).all()
        assert m.net.calls[-1] == ("fullres_rgb",) + args
    out = m.get_img_gray_fullres()
    assert (out == 7).all() and m.net.calls[-1][:2] == ("fullres_rgb", "no_ab") and m.net.calls[-1][3:] == ("image", 0)
    assert m.net.count("fullres_rgb") == 4 and m.net.count("upsample_lab2rgb") == 0
    assert m.__dict__.get("_fullres_lab_pending")                  # none of them needed the full-resolution Lab on the host
    # ... and the source is still there for the next click: no L upload
    m.net_forward_hints([(2, 2, 4, 4, 0, 255, 0)])
    assert m.net.count("set_image_l") == 0


def test_getters_fall_back_when_the_engine_refuses(png):
    path, src = png
    m = _model()
    m.load_image_device(path)
    _with_result(m)
    m.net.fail_fullres = True
    m.net.calls = []
    out = m.get_img_fullres()                                      # today's code: the display upsample with the host L plane
    assert [c[0] for c in m.net.calls] == ["fullres_rgb", "upsample_lab2rgb"] and (out == 9).all()
    assert not m._src_resident
    m.get_input_img_fullres()
    m.get_sup_fullres()
    assert m.net.count("fullres_rgb") == 1                         # not asked again
    gray = m.get_img_gray_fullres()
    assert gray.shape == src.shape and m.net.count("fullres_rgb") == 1
    host = _model()
    host.load_image(path)
    np.testing.assert_array_equal(gray, host.get_img_gray_fullres())


def test_getters_fall_back_when_l_serial_has_moved(png):
    path, src = png
    m = _model()
    m.load_image_device(path)
    _with_result(m)
    m.net.set_image_l(np.zeros((X, X)))                            # something else used the engine behind the wrapper's back
    m.net.calls = []
    out = m.get_img_fullres()
    assert [c[0] for c in m.net.calls] == ["upsample_lab2rgb"] and (out == 9).all()
    assert m.net.count("fullres_rgb") == 0
    m.net_forward_hints([(1, 1, 3, 3, 255, 0, 0)])                 # and the next click uploads the L plane again
    assert m.net.count("set_image_l") == 1


def test_host_route_without_a_resident_source_never_asks_the_engine(png):
    path, _ = png
    m = _model()
    m.load_image(path)
    _with_result(m)
    m.get_img_fullres(); m.get_input_img_fullres(); m.get_sup_fullres(); m.get_img_gray_fullres()
    assert m.net.count("fullres_rgb") == 0 and m.net.count("set_image_rgb") == 0


def test_load_image_after_the_device_route_leaves_every_attribute_as_today(png):
    path, _ = png
    a = _model()
    a.load_image_device(path)
    _ = a.img_l_fullres
    a.load_image(path)
    b = _model()
    b.load_image(path)
    skip = {"net", "_l_serial"}                                    # the engine object; the serial the device route remembered (only read while _src_resident)
    keys_a, keys_b = set(vars(a)) - skip, set(vars(b)) - skip
    assert keys_a == keys_b, keys_a ^ keys_b
    for k in sorted(keys_a):
        va, vb = vars(a)[k], vars(b)[k]
        if isinstance(vb, np.ndarray):
            assert isinstance(va, np.ndarray) and va.dtype == vb.dtype and va.shape == vb.shape, k
            np.testing.assert_array_equal(va, vb, err_msg=k)
        else:
            assert va == vb, k
    assert not a._src_resident and not a._l_resident and not a._fullres_lab_pending
    a.net.calls = []
    a.net_forward_hints([(1, 1, 3, 3, 255, 0, 0)])
    assert a.net.count("set_image_l") == 1                         # the host route's plane goes up, as today
