"""GPU checks of the two read-outs of the device-resident colour distribution (idc_dist_entropy, idc_dist_decode) and of
the wrapper methods built on them.  Every comparison is against tests/dist_maps_ref.py (float64 numpy) applied to
``e.get_dist(n)`` of the SAME forward, so no bar depends on the precision the network ran at.

Bars:
  entropy      1e-5 abs -- each term carries logf's <= 1 ulp plus the conversions, the fp64 sum adds nothing: about
               4 * 2^-24 * ln 529 = 1.5e-6, plus one rounding to fp32 of a value <= 6.3 (2.4e-7); a dropped bin moves it by ~1e-2
  mode decode  bit-equal to centres[argmax p] and p.max()
  mean decode  2e-2 abs on the +-110 scale, the bar of the fp32 pred_ab decode in test_caffe_branches_gpu.test_dist313_head (the fp32
               expf / logf weights at gamma = 13 are of that order in the worst case; an indexing error is tens of units)
Shapes: 64 x 64 (batch 1 of 1) and 40 x 72 (batch 2 of 3: the 529 head's grid is 10 x 18 = 180 pixels, neither a multiple of a wave nor
of the 64-pixel workgroup; 529 and 313 bins are no multiple of the 8-way bin split either), both heads."""
import ctypes
import os

import numpy as np
import pytest

import dist_maps_ref
from interactive_deep_colorization_amd import _native, api, engine, workloads
from oracle import weights

pytestmark = pytest.mark.gpu

ENT_TOL, MEAN_TOL = 1e-5, 2e-2
S = 0.2                                                   # the 313 head's default temperature (dist_ab_S = softmax(S l))
CASES = {                                                 # name: (bins, H, W, n, max_batch, precision)
    "529_64": (529, 64, 64, 1, 1, "fp32"),
    "529_40x72": (529, 40, 72, 2, 3, "fp32"),
    "313_64": (313, 64, 64, 1, 1, "fp32"),
    "313_40x72": (313, 40, 72, 2, 3, "fp32"),
    "529_64_bf16": (529, 64, 64, 1, 1, "bf16"),
}
_STATE = {}
FP = ctypes.POINTER(ctypes.c_float)


def _grid529():
    axis = np.arange(-110, 120, 10)
    return np.array(np.meshgrid(axis, axis)).reshape((2, 529)).T.astype(np.float32)


def _sd313():
    return weights.add_pred313_head(weights.make_state_dict(2, "he", include_class=False), 2)


def _case(name, make_sd):
    """One engine per case with a forward's distribution resident, the host copy p of it and the centres: made once, then only read."""
    if name not in _STATE:
        bins, H, W, n, nb, precision = CASES[name]
        L, ab, mask = workloads.random_batch(n, H, W, seed=17, max_points=4, max_p=2)
        if bins == 529:
            e = engine.HipColorizer(H, W, max_batch=nb, precision=precision, dist=True)
            e.load_state_dict(make_sd(0, "he"))
            e.forward_dist(L, ab, mask, 0.0, want_dist=False)
            centres = _grid529()
        else:
            sd = _sd313()
            e = engine.HipColorizer(H, W, max_batch=nb, precision=precision, dist313=True)
            e.load_state_dict(sd)
            e.keep_dist(True)
            e.forward_dist313(L, ab, mask, 0.0, want_dist=False)
            centres = np.ascontiguousarray(sd["pred.pred_ab.weight"][:, :, 0, 0].T)
        p = e.get_dist(n)
        p.setflags(write=False)
        _STATE[name] = (e, n, p, centres)
    return _STATE[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_entropy(name, make_sd):
    e, n, p, _ = _case(name, make_sd)
    ent = e.dist_entropy(n)
    ref = dist_maps_ref.entropy(p)
    assert ent.shape == ref.shape and ent.dtype == np.float32
    err = np.abs(ent - ref).max()
    print("entropy %s: max abs err %.3e (range %.3f .. %.3f)" % (name, err, ref.min(), ref.max()))
    assert ref.max() < 0 and ref.min() < -1.0            # a real distribution, not a one-hot or a blank
    assert err <= ENT_TOL


@pytest.mark.parametrize("name", sorted(CASES))
def test_mode_decode(name, make_sd):
    e, n, p, centres = _case(name, make_sd)
    ab, conf = e.dist_decode(centres, n, mode="mode", want_conf=True)
    ab_ref, conf_ref = dist_maps_ref.decode_mode(p, centres)
    np.testing.assert_array_equal(ab, ab_ref)
    np.testing.assert_array_equal(conf, conf_ref)
    np.testing.assert_array_equal(e.dist_decode(centres, n, mode="mode"), ab)          # conf = NULL
    assert len(np.unique(np.argmax(p, axis=1))) > 1


@pytest.mark.parametrize("gamma", [1.0, 2.6 / S])
@pytest.mark.parametrize("name", sorted(CASES))
def test_mean_decode(name, gamma, make_sd):
    e, n, p, centres = _case(name, make_sd)
    ab, conf = e.dist_decode(centres, n, mode="mean", gamma=gamma, want_conf=True)
    ref = dist_maps_ref.decode_mean(p, centres, gamma)
    assert ab.shape == ref.shape and ab.dtype == np.float32
    err = np.abs(ab - ref).max()
    print("mean decode %s gamma %g: max abs err %.3e (|ab| up to %.1f)" % (name, gamma, err, np.abs(ref).max()))
    assert err <= MEAN_TOL
    np.testing.assert_array_equal(conf, p.max(axis=1))


@pytest.mark.parametrize("name", ["529_40x72", "313_40x72"])
def test_result_of_an_image_does_not_depend_on_n(name, make_sd):
    e, n, p, centres = _case(name, make_sd)
    assert n == 2
    np.testing.assert_array_equal(e.dist_entropy(2)[0], e.dist_entropy(1)[0])
    for mode, gamma in (("mode", 1.0), ("mean", 1.0), ("mean", 2.6 / S)):
        ab2, c2 = e.dist_decode(centres, 2, mode=mode, gamma=gamma, want_conf=True)
        ab1, c1 = e.dist_decode(centres, 1, mode=mode, gamma=gamma, want_conf=True)
        np.testing.assert_array_equal(ab2[0], ab1[0])
        np.testing.assert_array_equal(c2[0], c1[0])
    np.testing.assert_array_equal(e.get_dist(2), p)                                     # read-only: the resident tensor is as it was


def test_dist313_golden_entropy_and_pred_ab(golden):
    """On the golden of test_dist313_head (fp32): -ent within that test's 1e-3 of the stored entropy, and the mean decode at
    gamma = 2.6 / S within its 2e-2 of pred_ab minus the layer's bias, from the same forward."""
    g = golden("dist313_64_he_s2")
    sd = weights.add_pred313_head(weights.make_state_dict(int(g["weight_seed"]), "he", include_class=False), int(g["weight_seed"]))
    e = engine.HipColorizer(64, 64, max_batch=1, precision="fp32", dist313=True)
    e.load_state_dict(sd)
    e.keep_dist(True)
    _, pred, _ = e.forward_dist313(g["L_mc"], g["ab"], g["mask"], 0.0, want_dist=False)
    ent = e.dist_entropy(1)
    err_e = np.abs(-ent[0] - g["dist_entropy"].reshape(64, 64)).max()
    centres = np.ascontiguousarray(sd["pred.pred_ab.weight"][:, :, 0, 0].T)
    ab = e.dist_decode(centres, 1, mode="mean", gamma=2.6 / S)
    err_p = np.abs(ab - (pred - sd["pred.pred_ab.bias"].reshape(1, 2, 1, 1))).max()
    print("golden 313: entropy err %.3e, decode vs pred_ab - bias %.3e" % (err_e, err_p))
    assert err_e <= 1e-3
    assert err_p <= 2e-2
    e.close()


def _status(call):
    with pytest.raises(_native.IdcError) as ex:
        call()
    return ex.value.status


def test_errors(make_sd):
    UNSUPPORTED, BATCH, INVALID = -7, -6, -1
    c = _grid529()
    e = engine.HipColorizer(64, 64, max_batch=1, precision="fp32", dist=True)           # before any forward
    assert _status(lambda: e.dist_entropy(1)) == UNSUPPORTED
    assert _status(lambda: e.dist_decode(c, 1)) == UNSUPPORTED
    with pytest.raises(_native.IdcError, match="Need to set prediction first"):
        e.dist_entropy(1)
    e.close()
    L, ab, mask = workloads.random_batch(1, 64, seed=3)
    e = engine.HipColorizer(64, 64, max_batch=1, precision="fp32")                      # no distribution head
    e.load_state_dict(make_sd(0, "he"))
    e.forward(L, ab, mask, 0.0)
    assert _status(lambda: e.dist_entropy(1)) == UNSUPPORTED
    out = np.empty((1, 2, 16, 16), np.float32)                                          # (dist_bins() is 0 here: the ABI directly)
    assert e.lib.idc_dist_decode(e._h, 1, 0, 1.0, c.ctypes.data_as(FP), out.ctypes.data_as(FP), None) == UNSUPPORTED
    e.close()
    e = engine.HipColorizer(64, 64, max_batch=1, precision="fp32", dist313=True)        # 313 head, distribution not kept
    e.load_state_dict(_sd313())
    e.forward_dist313(L, ab, mask, 0.0, want_dist=False)
    assert _status(lambda: e.dist_entropy(1)) == UNSUPPORTED
    assert _status(lambda: e.dist_decode(np.zeros((313, 2), np.float32), 1)) == UNSUPPORTED
    e.close()
    e, n, _, c = _case("529_40x72", make_sd)                                           # 2 images resident of max_batch 3
    assert _status(lambda: e.dist_entropy(3)) == BATCH
    assert _status(lambda: e.dist_decode(c, 3)) == BATCH
    assert _status(lambda: e.dist_entropy(0)) == BATCH
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert _status(lambda: e.dist_decode(c, 1, mode="mean", gamma=bad)) == INVALID
    out = np.empty((1, 2, 10, 18), np.float32)
    assert e.lib.idc_dist_decode(e._h, 1, 2, 1.0, c.ctypes.data_as(FP), out.ctypes.data_as(FP), None) == INVALID      # unknown mode
    assert e.lib.idc_dist_decode(e._h, 1, 0, 1.0, None, out.ctypes.data_as(FP), None) == INVALID
    assert e.lib.idc_dist_entropy(e._h, 1, None) == INVALID


@pytest.mark.parametrize("cls", ["torch529", "caffe313"])
def test_api_classes(cls, make_sd):
    """compute_entropy() on the device leaves dist_ab on the device; the decode getters; none of them disturbs the resident tensor."""
    rgb = np.load(os.path.join(os.path.dirname(__file__), "golden", "mortar_pestle_256_rgb.npy"))[::4, ::4].copy()
    if cls == "torch529":
        m = api.ColorizeImageTorchDist(Xd=64, maskcent=True)
        m.prep_net(path="", state_dict=dict(make_sd(0, "he")))
    else:
        m = api.ColorizeImageCaffeDist(Xd=64)
        m.prep_net(0, state_dict=dict(_sd313()))
    m.set_image(rgb)
    input_ab, mask = workloads.hints_config2(64, 5, 3, 0)
    m.net_forward(input_ab, mask)
    np.random.seed(11)
    reccs_before = m.get_ab_reccs(20, 30, K=4, N=5000)
    m.compute_entropy()
    assert m._dist_on_device and m.__dict__.get("_lazy_dist_ab") is None                # not materialised
    ent = m.dist_entropy
    assert ent.shape == (64, 64) and ent.dtype == np.float32
    ab, conf = m.get_dist_decode(return_conf=True)
    assert ab.shape == (2, 64, 64) and conf.shape == (64, 64) and ab.dtype == np.float32
    mean = m.get_dist_decode(mode="mean", gamma=2.0)
    assert mean.shape == (2, 64, 64) and np.abs(mean - ab).max() > 0
    img = m.get_img_dist_decode()
    assert img.shape == (64, 64, 3) and img.dtype == np.uint8
    np.random.seed(11)
    np.testing.assert_array_equal(m.get_ab_reccs(20, 30, K=4, N=5000), reccs_before)
    with np.errstate(divide="ignore", invalid="ignore"):
        host = np.sum(m.dist_ab * np.log(m.dist_ab), axis=0)                            # materialises dist_ab: the host route from here on
    # a bin that underflowed to 0 makes the reference's expression NaN at that pixel, the device counts it as 0 (the Caffe-scaled net on
    # seeded weights saturates at most pixels): the host expression is the yardstick wherever it is a number, the restatement everywhere
    zero = (m.dist_ab == 0).any(axis=0)
    np.testing.assert_array_equal(np.isnan(host), zero)
    assert np.isfinite(ent).all()
    err = np.abs(ent - host)[~zero].max() if (~zero).any() else 0.0
    err0 = np.abs(ent - dist_maps_ref.entropy(m.dist_ab[None])[0]).max()
    print("api %s: device vs host entropy %.3e on %d pixels; vs the restatement on all (%d with a p == 0 bin) %.3e" % (cls, err, (~zero).sum(), zero.sum(), err0))
    assert err <= ENT_TOL and err0 <= ENT_TOL
    centres = m._bin_centres()
    idx = np.argmax(m.dist_ab, axis=0)
    np.testing.assert_array_equal(ab, np.moveaxis(np.asarray(centres, np.float32)[idx], -1, 0))
    np.testing.assert_array_equal(conf, m.dist_ab.max(axis=0))
    with np.errstate(divide="ignore", invalid="ignore"):
        m.compute_entropy()
    np.testing.assert_array_equal(m.dist_entropy, host)
