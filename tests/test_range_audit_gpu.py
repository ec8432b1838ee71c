"""GPU tests of the range audit (idc_audit.hip behind idc_set_range_audit) and of calibrated activation exponents for precision 'fp16x3'.

The "hot" checkpoints compute the SAME function as the seeded weights they are made from (ReLU is positively homogeneous and powers of two are
exact), with one tensor 2^20 times larger -- far outside fp16's +-65504:
  hot 'conv6_1': model6.0 weight and bias * 2^K, model6.2 weight * 2^-K;
  hot 'conv2_2': BatchNorm model2.4 weight and bias * 2^K, model3.0 AND model2short9.0 weights * 2^-K (two consumers, one of them the shortcut
                 conv inside the fused deconv + shortcut launch);
  hot 'conv8_3': BatchNorm model8.5 weight and bias * 2^K, model9up.0 weight * 2^-K (the deconv side of that launch).
Expected ab map: the float64 oracle forward of the UNMODIFIED weights.  Bounds: tests/bounds.py FP32_TOL on the ab map (what the existing fp16x3
network tests use), 2e-4 * (1 + max|ref|) per activation (tests/test_round6_gpu.py test_split_network_layer_by_layer)."""
import warnings

import numpy as np
import pytest
import torch

from interactive_deep_colorization_amd import api, engine, workloads
from oracle import siggraph_torch
from tests import bounds
from tests.conftest import state_dict_for

pytestmark = pytest.mark.gpu
K = 20
PRECISIONS = ["fp32", "bf16", "bf16x6", "fp16x3", "fp16"]
CONV_ROWS = [n for n in engine.layer_table_names() if n not in ("glob_branch", "head", "dist_softmax")]


def hot_state_dict(sd, spot, k=K):
    out = dict(sd)
    up, down = np.float32(2.0 ** k), np.float32(2.0 ** -k)
    if spot == "conv6_1":
        out["model6.0.weight"] = sd["model6.0.weight"] * up; out["model6.0.bias"] = sd["model6.0.bias"] * up
        out["model6.2.weight"] = sd["model6.2.weight"] * down
    elif spot == "conv2_2":
        out["model2.4.weight"] = sd["model2.4.weight"] * up; out["model2.4.bias"] = sd["model2.4.bias"] * up
        out["model3.0.weight"] = sd["model3.0.weight"] * down; out["model2short9.0.weight"] = sd["model2short9.0.weight"] * down
    elif spot == "conv8_3":
        out["model8.5.weight"] = sd["model8.5.weight"] * up; out["model8.5.bias"] = sd["model8.5.bias"] * up
        out["model9up.0.weight"] = sd["model9up.0.weight"] * down
    else:
        raise KeyError(spot)
    return out


def _inputs(n, H, W, seed):
    return workloads.random_batch(n, H, W, seed=seed, max_points=5, max_p=3)


_ORACLE = {}


def _oracle(seed, style, n, H, W, in_seed, maskcent=0.5):
    key = (seed, style, n, H, W, in_seed, maskcent)
    if key not in _ORACLE:
        L, ab, m = _inputs(n, H, W, in_seed)
        out, _, acts = siggraph_torch.forward(state_dict_for(seed, style), L, ab, m, maskcent, dtype=torch.float64, return_acts=True)
        _ORACLE[key] = (out, {k_: acts[k_] for k_ in ("conv6_1", "conv2_2", "conv8_3")})
    return _ORACLE[key]


# ---------------------------------------------------------------------------------------------- audit against the stored tensors
# every precision at 64x64 and at the ragged 32x48, batch 2; one 256x256 N = 4 case (throughput tiles, fused deconv launches) for the operand-split
# forms the calibration relies on and for bf16
AUDIT_CASES = [(p, s) for p in PRECISIONS for s in ((2, 64, 64), (2, 32, 48))] + [(p, (4, 256, 256)) for p in ("fp16x3", "bf16x6", "bf16")]


@pytest.mark.parametrize("precision,shape", AUDIT_CASES)
def test_audit_matches_the_stored_activations(precision, shape):
    n, H, W = shape
    sd = state_dict_for(1, "he")
    L, ab, m = _inputs(n, H, W, 11)
    e = engine.HipColorizer(H, W, max_batch=n, precision=precision)
    try:
        e.load_state_dict(sd)
        assert [r["name"] for r in e.layer_table()] == engine.layer_table_names()
        e.set_range_audit(True)
        e.forward(L, ab, m, 0.5)
        rep = e.range_report()
        e.set_range_audit(False)
        assert [r["name"] for r in rep] == engine.layer_table_names()
        audited = 0
        for r in rep:
            assert r["n_saturated"] == 0 and r["n_nonfinite"] == 0 and r["act_exp"] == 0, r
            if r["n_values"] == 0:
                assert r["max_abs"] == 0.0 and r["storage"] is None, r
                if r["name"] in CONV_ROWS:                      # nothing stored: the activation getter says the same
                    with pytest.raises(Exception):
                        e.activation(r["name"], n)
                continue
            audited += 1
            got = e.activation(r["name"], n)
            assert r["n_values"] == got.size, (r, got.shape)
            mx = float(np.abs(got).max())
            print("%s %s %-14s %-7s max_abs %.9g (activation %.9g) tiny %d" % (precision, shape, r["name"], r["storage"], r["max_abs"], mx, r["n_tiny"]))
            if r["storage"].endswith("x3"):
                assert abs(r["max_abs"] - mx) <= 2.0 ** -22 * mx, r         # three parts summed: the one place a last-bit difference is allowed
            else:
                assert r["max_abs"] == mx, (r, mx)
            assert r["n_tiny"] == int(np.count_nonzero((got != 0) & (np.abs(got) < 2.0 ** -14))), r
        assert audited >= 25, audited                           # 29 conv layers, at most conv1_1 / the shortcut convs / conv10_2 ride in other launches
        stored = {r["name"]: r["storage"] for r in rep if r["storage"]}
        want = {"fp32": "fp32", "bf16": "bf16", "bf16x6": "bf16x3", "fp16x3": "fp16x2", "fp16": "fp16"}[precision]
        assert stored["conv6_1"] == want, stored
    finally:
        e.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_audit_changes_no_output_bit_and_is_sticky(precision):
    sd = state_dict_for(1, "torch")
    L, ab, m = _inputs(2, 64, 64, 12)
    L2, ab2, m2 = _inputs(2, 64, 64, 13)
    e = engine.HipColorizer(64, 64, max_batch=2, precision=precision)
    try:
        e.load_state_dict(sd)
        off = e.forward(L, ab, m, 0.5).copy()
        e.set_range_audit(True)
        on = e.forward(L, ab, m, 0.5).copy()
        assert np.array_equal(off, on)
        r1 = e.range_report()
        e.forward(L2, ab2, m2, 0.5)
        r2 = e.range_report()
        out = np.empty_like(off)
        with pytest.raises(Exception):                         # the pipelined slots are not audited: refused while the audit is on
            e.forward_async(0, L, ab, m, out, 0.5)
        e.set_range_audit(False)
        assert np.array_equal(e.forward(L, ab, m, 0.5), off)
        r3 = e.range_report()                                  # audit off: the records stay, nothing is added
        for a, b, c in zip(r1, r2, r3):
            assert b["n_values"] == 2 * a["n_values"] and b["max_abs"] >= a["max_abs"] and b["n_tiny"] >= a["n_tiny"], (a, b)
            assert c == b
        assert any(b["max_abs"] > a["max_abs"] for a, b in zip(r1, r2))
        e.range_reset()
        for r in e.range_report():
            assert r["n_values"] == 0 and r["max_abs"] == 0.0 and r["n_tiny"] == 0 and r["n_saturated"] == 0, r
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------- the hot checkpoint, found and fixed
@pytest.mark.parametrize("style", ["torch", "he"])
def test_hot_checkpoint_is_found(style):
    """fp16x3 without exponents on the hot 'conv6_1' checkpoint: the forward answers IDC_OK, the audit names conv6_1 (and nothing upstream of it),
    and check_ranges() through the reference-API class warns.  (How wrong the ab map is is not asserted.)"""
    sd = state_dict_for(1, style)
    hot = hot_state_dict(sd, "conv6_1")
    L, ab, m = _inputs(2, 64, 64, 21)
    # the premise, from the oracle alone: same function, conv6_1 2^K times larger and mostly beyond fp16
    ref, _, acts = siggraph_torch.forward(sd, L, ab, m, 0.5, dtype=torch.float64, return_acts=True)
    ref_hot, _, acts_hot = siggraph_torch.forward(hot, L, ab, m, 0.5, dtype=torch.float64, return_acts=True)
    assert np.array_equal(ref, ref_hot)
    c61 = acts_hot["conv6_1"]
    assert np.count_nonzero(c61 > 65504) > 0.5 * np.count_nonzero(c61), (np.count_nonzero(c61 > 65504), np.count_nonzero(c61))
    e = engine.HipColorizer(64, 64, max_batch=2, precision="fp16x3")
    try:
        e.load_state_dict(hot)
        e.set_range_audit(True)
        e.forward(L, ab, m, 0.5)
        rep = {r["name"]: r for r in e.range_report()}
    finally:
        e.close()
    assert rep["conv6_1"]["n_saturated"] > 0 and rep["conv6_1"]["max_abs"] >= 65504.0      # (hi and lo both clamp: a stored sum can read 2 x 65504)
    for name in CONV_ROWS[:CONV_ROWS.index("conv6_1")]:
        assert rep[name]["n_saturated"] == 0, rep[name]
    cls = api.ColorizeImageTorch(Xd=64, maskcent=True, precision="fp16x3")
    cls.set_image(np.random.RandomState(3).randint(0, 256, (64, 64, 3)).astype(np.uint8))
    cls.prep_net(state_dict=hot)
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            report = cls.check_ranges()
        msgs = [str(x.message) for x in w if "saturate" in str(x.message)]
        assert len(msgs) == 1 and "conv6_1" in msgs[0] and "conv5_3" not in msgs[0], msgs
        assert {r["name"]: r for r in report}["conv6_1"]["n_saturated"] > 0
    finally:
        cls.net.close()


PARENT_FP16X3_HE_N4_256 = 3.4808e-3     # plain fp16x3 (no exponents: the parent commit's path, bit for bit), he-style seed 1, inputs of the (4, 256, 256) case


def _run_calibrated(sd_run, sd_ref_key, spot, n, H, W, fuse):
    """Exponents calibrated on ONE image of another seed, then a forward of the tested batch: (out, report, activation of `spot`, exponents)."""
    style_seed, style = sd_ref_key
    Lc, abc, mc = _inputs(1, H, W, 77)
    a = engine.calibrate_activation_exponents(sd_run, Lc, abc, mc, 0.5)
    L, ab, m = _inputs(n, H, W, 21)
    engine.set_option("split_ds_fuse", fuse)
    e = engine.HipColorizer(H, W, max_batch=n, precision="fp16x3")
    try:
        e.load_state_dict(sd_run, act_exp=a)
        e.set_range_audit(True)
        out = e.forward(L, ab, m, 0.5).copy()
        rep = e.range_report()
        act = e.activation(spot, n)
        kernels = {r["name"]: r["kernel"] for r in e.layer_table()}
        assert ("conv_ds_fused_ms" in kernels["conv9_1"]) == bool(fuse), kernels["conv9_1"]
    finally:
        e.close()
        engine.set_option("split_ds_fuse", 1)
    return out, rep, act, dict(zip(engine.layer_table_names(), a))


@pytest.mark.parametrize("style", ["torch", "he"])
@pytest.mark.parametrize("spot,fuse,shape", [("conv6_1", 1, (2, 64, 64)), ("conv6_1", 1, (2, 32, 48)), ("conv6_1", 1, (4, 256, 256)),
                                             ("conv2_2", 1, (2, 64, 64)), ("conv2_2", 0, (2, 64, 64)),
                                             ("conv8_3", 1, (2, 64, 64)), ("conv8_3", 0, (2, 64, 64))])
def test_hot_checkpoint_with_calibrated_exponents(style, spot, fuse, shape):
    """Bound on the ab map: tests/bounds.py FP32_TOL (1e-3 torch-init, 3e-3 he-style).  Measured on MI355X, max |out - float64 oracle|:
    64x64 / 32x48 batch 2: 1.2e-5 .. 1.5e-5 torch-init, 3.6e-4 .. 8.7e-4 he-style (every hot spot, fused and unfused); 256x256 N = 4 torch-init
    1.9e-5.  The he-style 256x256 N = 4 case does not fit 3e-3 -- and neither does the path it is compared with: the parent commit's plain fp16x3
    on the UNMODIFIED weights at the same inputs measures 3.481e-3 (bf16x6 2.75e-3, the exact-fp32 kernels 1.43e-3), the calibrated hot checkpoint
    3.828e-3.  That case is therefore held to the parent's figure plus 25 % (4.351e-3), the margin tests/bounds.py gives the bf16 bounds."""
    n, H, W = shape
    sd = state_dict_for(1, style)
    ref, acts = _oracle(1, style, n, H, W, 21)
    hot_ref = acts[spot] * 2.0 ** K                            # exact in float64: the hot tensor is 2^K times the unmodified one
    assert np.count_nonzero(np.abs(hot_ref) > 65504) > 0.5 * np.count_nonzero(hot_ref)
    out, rep, act, a = _run_calibrated(hot_state_dict(sd, spot), (1, style), spot, n, H, W, fuse)
    err = float(np.abs(out - ref).max())
    aerr = float(np.abs(act - hot_ref).max())
    print("calibrated %s %s fuse=%d %s: ab err %.3e (tol %.1e), %s err %.3e / max|ref| %.3e, exponent %d" %
          (spot, style, fuse, shape, err, bounds.FP32_TOL[style], spot, aerr, np.abs(hot_ref).max(), a[spot]))
    assert a[spot] < 0
    follows = {"conv3_3_short": "conv8_1", "conv2_2_short": "conv9_1", "conv1_2_short": "conv10_1"}      # a shortcut conv takes its deconv's exponent
    for r in rep:
        assert r["n_saturated"] == 0 and r["n_nonfinite"] == 0, r
        want = 0 if r["name"] in ("conv1_1", "conv10_2") else a[follows.get(r["name"], r["name"])]
        assert r["act_exp"] == want, (r, want)
    tol = PARENT_FP16X3_HE_N4_256 * 1.25 if (style, shape) == ("he", (4, 256, 256)) else bounds.FP32_TOL[style]
    assert err <= tol, (err, tol)
    assert aerr <= 2e-4 * (1 + np.abs(hot_ref).max()), (aerr, np.abs(hot_ref).max())


@pytest.mark.parametrize("style", ["torch", "he"])
def test_exponents_are_neutral_on_the_unmodified_weights(style):
    sd = state_dict_for(1, style)
    n, H, W = 2, 64, 64
    L, ab, m = _inputs(n, H, W, 21)
    ref, _ = _oracle(1, style, n, H, W, 21)
    outs = {}
    Lc, abc, mc = _inputs(1, H, W, 77)
    cal = engine.calibrate_activation_exponents(sd, Lc, abc, mc, 0.5)
    assert any(cal)
    for tag, kw in (("plain", {}), ("zeros", dict(act_exp=[0] * len(engine.layer_table_names()))), ("calibrated", dict(act_exp=cal))):
        e = engine.HipColorizer(H, W, max_batch=n, precision="fp16x3")
        try:
            e.load_state_dict(sd, **kw)
            outs[tag] = e.forward(L, ab, m, 0.5).copy()
        finally:
            e.close()
    assert np.array_equal(outs["plain"], outs["zeros"])
    e_plain, e_cal = float(np.abs(outs["plain"] - ref).max()), float(np.abs(outs["calibrated"] - ref).max())
    print("neutrality %s: plain %.3e calibrated %.3e (tol %.1e)" % (style, e_plain, e_cal, bounds.FP32_TOL[style]))
    assert e_cal <= bounds.FP32_TOL[style]


def test_unsupported_combinations_are_refused():
    sd = state_dict_for(1, "he")
    for precision in ("bf16", "fp16"):
        e = engine.HipColorizer(64, 64, max_batch=1, precision=precision)
        try:
            with pytest.raises(Exception) as ei:
                e.load_state_dict(sd, act_exp={"conv6_1": -3})
            assert getattr(ei.value, "status", None) == -7
        finally:
            e.close()
    e = engine.HipColorizer(64, 64, max_batch=1, precision="fp16x3")
    try:
        blob = engine.pack_weights(sd, "fp16x3", act_exp={"conv6_1": -3})
        e.set_weights_blob(blob)                               # a blob packed elsewhere carries its exponents in the header
        assert {r["name"]: r["act_exp"] for r in e.range_report()}["conv6_1"] == -3
    finally:
        e.close()
    e = engine.HipColorizer(64, 64, max_batch=1, precision="bf16x6")
    try:
        with pytest.raises(Exception):
            e.set_weights_blob(blob)
    finally:
        e.close()


# Bytes of the uint8 image (of 49152) that differ from the fp32 class's, Xd = 128, he-style seed 1, one 5x5 hint, measured on MI355X:
#   8  plain fp16x3 class on the UNMODIFIED weights (the parent commit's path, bit for bit: test_exponents_are_neutral_on_the_unmodified_weights)
#   9  fp16x3 class with prep_net(calibrate=True) on the hot 'conv6_1' checkpoint
FLIPS_PARENT = 8


def test_prep_net_calibrate_end_to_end():
    """ColorizeImageTorch(precision='fp16x3').prep_net(calibrate=True) on the hot checkpoint returns the fp32 class's image except where the uint8
    quantisation flips.  Cap: the flips the plain fp16x3 class (the parent commit's path, bit for bit) shows against the fp32 class on the
    unmodified weights at the same inputs (8 bytes, measured), plus 25 %; the calibrated hot checkpoint shows 9."""
    sd = state_dict_for(1, "he")
    hot = hot_state_dict(sd, "conv6_1")
    X = 128
    img = np.random.RandomState(5).randint(0, 256, (X, X, 3)).astype(np.uint8)
    ab = np.zeros((2, X, X), np.float32); mask = np.zeros((1, X, X), np.float32)
    ab[0, 40:45, 60:65], ab[1, 40:45, 60:65], mask[0, 40:45, 60:65] = 35.0, -20.0, 1.0
    images = {}
    for tag, precision, weights, kw in (("fp32", "fp32", sd, {}), ("plain", "fp16x3", sd, {}), ("calibrated", "fp16x3", hot, dict(calibrate=True))):
        cls = api.ColorizeImageTorch(Xd=X, maskcent=True, precision=precision)
        cls.set_image(img)
        cls.prep_net(state_dict=weights, **kw)
        try:
            images[tag] = cls.net_forward(ab, mask).copy()
            if tag == "calibrated":
                with warnings.catch_warnings(record=True) as w:
                    warnings.simplefilter("always")
                    rep = cls.check_ranges()
                assert not [x for x in w if "saturate" in str(x.message)]
                assert {r["name"]: r["act_exp"] for r in rep}["conv6_1"] < 0
        finally:
            cls.net.close()
    parent = int(np.count_nonzero(images["plain"] != images["fp32"]))
    got = int(np.count_nonzero(images["calibrated"] != images["fp32"]))
    print("uint8 bytes that differ from the fp32 class (of %d): plain fp16x3 / unmodified weights %d, calibrated fp16x3 / hot weights %d" % (images["fp32"].size, parent, got))
    assert got <= FLIPS_PARENT * 1.25, (got, FLIPS_PARENT)
    assert int(np.abs(images["calibrated"].astype(int) - images["fp32"].astype(int)).max()) <= 1
