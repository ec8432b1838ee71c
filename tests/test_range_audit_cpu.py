"""CPU tests of the range audit's ABI surface and of the activation exponents of precision 'fp16x3' (pack time, host code only).

The fp16x3 blob layout is re-derived here from the layer list tests/test_abi_cpu.py keeps (the same source test_pack_weights_layout uses), with
what csrc/idc_pack.hip make_blob_plan adds for the operand-split precisions: conv1_1 is an fp32 island, every other layer carries two fp16
weight parts and ONE fp32 accumulator-scale word ("wscale")."""
import os
import re
import warnings

import numpy as np
import pytest

from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import api, engine
from tests.test_abi_cpu import LAYERS, _al

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["idc_set_range_audit", "idc_range_reset", "idc_range_report", "idc_pack_weights_ex", "idc_load_weights_ex"]
NAME_OF = {"model6.0": "conv6_1", "model6.2": "conv6_2", "model2.2": "conv2_2", "model8.3": "conv8_3", "model9up.0": "conv9_1",
           "model2short9.0": "conv2_2_short", "model3.0": "conv3_1", "model10.1": "conv10_2", "model1.0": "conv1_1", "model10up.0": "conv10_1"}


def _plan_fp16x3():
    off, plan = 64, {}
    for wkey, bnkey, kind, cin, cout in LAYERS:
        if wkey == "model_class.0":
            continue
        cpad = 64 if cout <= 64 else _al(cout, 128)
        island = kind == "im2col"
        kc = 32 if island else 64
        nkc = (64 // kc) if island else -(-cin // kc)
        ntap = {"c3": 9, "dc": 16, "c1": 1, "im2col": 1}[kind]
        e = dict(wkey=wkey, cout=cout, cpad=cpad)
        off = _al(off); e["w_off"] = off; off += ntap * nkc * (cpad // 64) * 8192 * (1 if island else 2)
        off = _al(off); e["b_off"] = off; off += cpad * 4
        if bnkey:
            off = _al(off); e["s_off"] = off; off += cpad * 4
            off = _al(off); e["t_off"] = off; off += cpad * 4
        if kind == "dc":
            off = _al(off); e["fb_off"] = off; off += cpad * 4
        if not island:
            off = _al(off); e["ws_off"] = off; off += 4
        plan[wkey] = e
    off = _al(off) + 1024
    off = _al(off) + 8
    return plan, _al(off)


def _word(blob, off):
    return float(blob[off:off + 4].view(np.float32)[0])


def test_new_symbols_declared_listed_exported():
    lib = N.load()
    header = open(os.path.join(REPO, "include", "ideepcolor.h")).read()
    declared = set(re.findall(r"\b(idc_[a-z0-9_]+)\s*\(", header))
    for sym in NEW_SYMBOLS:
        assert sym in declared and sym in N.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    assert "idc_range_info" in header and lib.idc_version() == 2


@pytest.mark.parametrize("throughput_blob", [False, True])
def test_no_exponents_is_the_plain_blob(make_sd, throughput_blob):
    sd = make_sd(0, "he")
    plain = engine.pack_weights(sd, "fp16x3", throughput_blob=throughput_blob)
    n_rows = len(engine.layer_table_names())
    assert np.array_equal(plain, engine.pack_weights(sd, "fp16x3", throughput_blob=throughput_blob, act_exp=None))
    assert np.array_equal(plain, engine.pack_weights(sd, "fp16x3", throughput_blob=throughput_blob, act_exp=[0] * n_rows))
    assert plain.size == _plan_fp16x3()[1] == N.load().idc_weights_blob_bytes(N.IDC_FP16X3, N.IDC_FLAG_THROUGHPUT_BLOB if throughput_blob else 0)


def test_exponent_errors(make_sd):
    sd = make_sd(0, "he")
    n_rows = len(engine.layer_table_names())
    for precision in ("bf16", "fp32", "bf16x6", "fp16"):
        assert engine.pack_weights(sd, precision, act_exp=[0] * n_rows).size > 0          # all zeros: accepted everywhere
        with pytest.raises(N.IdcError) as ei:
            engine.pack_weights(sd, precision, act_exp={"conv6_1": 3})
        assert ei.value.status == -7, precision                                          # IDC_ERR_UNSUPPORTED
    for bad in (n_rows - 1, n_rows + 1):
        with pytest.raises(N.IdcError) as ei:
            engine.pack_weights(sd, "fp16x3", act_exp=[0] * bad)
        assert ei.value.status == -1                                                     # IDC_ERR_INVALID_ARG
    with pytest.raises(N.IdcError) as ei:
        engine.pack_weights(sd, "fp16x3", act_exp={"conv6_1": 25})
    assert ei.value.status == -1
    with pytest.raises(N.IdcError) as ei:                                                # the 529-bin head reads conv8_3: refused, and the message says which flag
        engine.pack_weights(sd, "fp16x3", dist=True, act_exp={"conv6_1": 3})
    assert ei.value.status == -7 and "IDC_FLAG_DIST_HEAD" in str(ei.value)
    with pytest.raises(KeyError):
        engine.pack_weights(sd, "fp16x3", act_exp={"conv6_9": 3})


@pytest.mark.parametrize("a", [-8, 5])
def test_one_exponent_touches_only_its_layer_and_its_consumer(make_sd, a):
    """conv6_1 (no BatchNorm) stored as value * 2^a: the scale goes into conv6_1's own epilogue numbers -- its bias vector and its accumulator-scale
    word (ReLU is positively homogeneous: relu(acc s + b) 2^a = relu(acc s 2^a + b 2^a)) -- and comes out in conv6_2's accumulator-scale word.
    Nothing else in the blob moves but the header (flag bit 0x100, the exponent table in its padding, the checksum)."""
    sd = make_sd(0, "he")
    plan, total = _plan_fp16x3()
    plain = engine.pack_weights(sd, "fp16x3")
    blob = engine.pack_weights(sd, "fp16x3", act_exp={"conv6_1": a})
    assert blob.size == plain.size == total
    diff = np.nonzero(plain != blob)[0]
    e61, e62 = plan["model6.0"], plan["model6.2"]
    allowed = np.zeros(total, bool)
    allowed[12:16] = True; allowed[24:64] = True                                         # header: flags, checksum, exponent table
    allowed[e61["b_off"]:e61["b_off"] + 512 * 4] = True
    allowed[e61["ws_off"]:e61["ws_off"] + 4] = True
    allowed[e62["ws_off"]:e62["ws_off"] + 4] = True
    assert allowed[diff].all(), diff[~allowed[diff]][:10]
    assert int(blob[12:16].view(np.uint32)[0]) == 0x100 and int(plain[12:16].view(np.uint32)[0]) == 0
    names = engine.layer_table_names()
    table = blob[32:64].view(np.int8)
    assert table[names.index("conv6_1") - 1] == a and np.count_nonzero(table) == 1
    np.testing.assert_array_equal(blob[e61["b_off"]:e61["b_off"] + 2048].view(np.float32), np.ldexp(plain[e61["b_off"]:e61["b_off"] + 2048].view(np.float32), a))
    assert _word(blob, e61["ws_off"]) == _word(plain, e61["ws_off"]) * 2.0 ** a
    assert _word(blob, e62["ws_off"]) == _word(plain, e62["ws_off"]) * 2.0 ** -a


def test_batchnorm_layer_carries_the_scale_in_its_affine(make_sd):
    sd = make_sd(0, "he")
    plan, total = _plan_fp16x3()
    plain = engine.pack_weights(sd, "fp16x3")
    blob = engine.pack_weights(sd, "fp16x3", act_exp={"conv6_3": 7})
    e = plan["model6.4"]
    for key in ("s_off", "t_off"):
        np.testing.assert_array_equal(blob[e[key]:e[key] + 2048].view(np.float32)[:512], np.ldexp(plain[e[key]:e[key] + 2048].view(np.float32)[:512], 7))
    np.testing.assert_array_equal(blob[e["b_off"]:e["b_off"] + 2048], plain[e["b_off"]:e["b_off"] + 2048])
    assert _word(blob, e["ws_off"]) == _word(plain, e["ws_off"])
    assert _word(blob, plan["model7.0"]["ws_off"]) == _word(plain, plan["model7.0"]["ws_off"]) * 2.0 ** -7


def test_forced_zero_layers(make_sd):
    """conv1_1 (fp32 island) and conv10_2 (read by the head inside its own launch) cannot carry an exponent: asking for one changes nothing."""
    sd = make_sd(0, "he")
    plain = engine.pack_weights(sd, "fp16x3")
    assert np.array_equal(plain, engine.pack_weights(sd, "fp16x3", act_exp={"conv1_1": 4, "conv10_2": -3}))


@pytest.mark.parametrize("a22,a83", [(6, -9), (-11, 4), (3, 3)])
def test_deconv_and_shortcut_share_one_accumulator_scale(make_sd, a22, a83):
    """conv9_1 = model9up(conv8_3) + model2short9(conv2_2) is ONE launch with ONE accumulator scale: with different exponents on its two inputs the
    packer lowers one weight exponent until wexp + a[input] agree -- the two layers' words are then the same number."""
    sd = make_sd(0, "he")
    plan, _ = _plan_fp16x3()
    plain = engine.pack_weights(sd, "fp16x3")
    blob = engine.pack_weights(sd, "fp16x3", act_exp={"conv2_2": a22, "conv8_3": a83})
    wd, ws = _word(blob, plan["model9up.0"]["ws_off"]), _word(blob, plan["model2short9.0"]["ws_off"])
    assert wd == ws and wd > 0 and np.log2(wd) == round(np.log2(wd))
    assert _word(plain, plan["model9up.0"]["ws_off"]) == _word(plain, plan["model2short9.0"]["ws_off"])
    # wexp + a[input] of the pair = -log2(word); it is the smaller of the two sides' (own weight exponent + input exponent)
    from_plain = -np.log2(_word(plain, plan["model9up.0"]["ws_off"]))
    assert -np.log2(wd) <= from_plain + max(a22, a83) and -np.log2(wd) >= from_plain + min(a22, a83) - 40
    # the other consumer of conv2_2 (conv3_1) takes a22 out on its own
    assert _word(blob, plan["model3.0"]["ws_off"]) == _word(plain, plan["model3.0"]["ws_off"]) * 2.0 ** -a22
    # an exponent on the deconv's OUTPUT goes onto both layers' words and biases alike (the shortcut conv follows the deconv it is summed into)
    blob2 = engine.pack_weights(sd, "fp16x3", act_exp={"conv9_1": 5, "conv2_2_short": -2})
    for key in ("model9up.0", "model2short9.0"):
        assert _word(blob2, plan[key]["ws_off"]) == _word(plain, plan[key]["ws_off"]) * 32.0
        np.testing.assert_array_equal(blob2[plan[key]["b_off"]:plan[key]["b_off"] + 512].view(np.float32),
                                      plain[plan[key]["b_off"]:plan[key]["b_off"] + 512].view(np.float32) * 32.0)
    fb = plan["model9up.0"]["fb_off"]
    np.testing.assert_array_equal(blob2[fb:fb + 512].view(np.float32), plain[fb:fb + 512].view(np.float32) * 32.0)
    names = engine.layer_table_names()
    table = blob2[32:64].view(np.int8)
    assert table[names.index("conv9_1") - 1] == 5 and table[names.index("conv2_2_short") - 1] == 5


def _row(name, max_abs, n_values=100, act_exp=0):
    return dict(index=0, name=name, storage="bf16x3", act_exp=act_exp, max_abs=max_abs, n_values=n_values, n_saturated=0, n_tiny=0, n_nonfinite=0)


def test_exponents_from_report_arithmetic():
    T = engine.TARGET_EXP
    assert T == 12 and engine.ACT_EXP_RANGE == (-24, 24)
    rep = [_row("a", 1.0), _row("b", 1.5), _row("c", 2.0), _row("d", 3000.0), _row("e", 4096.0), _row("f", 4097.0), _row("g", 6.4e6),
           _row("h", 0.0), _row("i", 5.0, n_values=0), _row("j", 2.0 ** -40), _row("k", 3.0e38), _row("l", float("nan")), _row("m", 0.75, act_exp=3)]
    got = engine.exponents_from_report(rep)
    #            1 -> 2^12   1.5 -> ceil 1   2 -> 2^1   3000 -> 2^12   4096 = 2^12   4097 -> 2^13   6.4e6 -> 2^23
    assert got[:7] == [12, 11, 11, 0, 0, -1, -11]
    assert got[7:] == [0, 0, 24, -24, 0, 15]            # zeros / nothing stored / clipped both ways / NaN / a scaled report: 12 - 0 + 3
    for mx, a in zip([r["max_abs"] for r in rep[:7]], got[:7]):
        assert 2.0 ** (T - 1) < mx * 2.0 ** a <= 2.0 ** T


class _StubEngine(object):
    """Stands where calibrate_activation_exponents builds its temporary bf16x6 engine."""
    made = []

    def __init__(self, H, W, max_batch=1, precision=None, **kw):
        self.args = dict(H=H, W=W, max_batch=max_batch, precision=precision, kw=kw)
        self.calls = []
        _StubEngine.made.append(self)

    def set_io_scales(self, **kw):
        self.calls.append(("scales", kw))

    def load_state_dict(self, sd):
        self.calls.append(("load", sd))

    def set_range_audit(self, on):
        self.calls.append(("audit", on))

    def forward(self, L, ab, m, maskcent):
        self.calls.append(("forward", L.shape, maskcent))

    def range_report(self):
        names = engine.layer_table_names()
        return [_row(nm, {"conv6_1": 6.4e6, "conv2_2": 10.0}.get(nm, 0.0), n_values=0 if nm in ("glob_branch", "head", "dist_softmax", "conv1_1") else 7) for nm in names]

    def close(self):
        self.calls.append(("close",))


def test_calibration_drives_a_bf16x6_engine_with_the_audit_on():
    _StubEngine.made = []
    L = np.zeros((3, 1, 32, 40), np.float32)
    a = engine.calibrate_activation_exponents({"k": 1}, L, np.zeros((3, 2, 32, 40)), np.zeros((3, 1, 32, 40)), 0.5, engine_factory=_StubEngine)
    st = _StubEngine.made[0]
    assert st.args["precision"] == "bf16x6" and (st.args["H"], st.args["W"], st.args["max_batch"]) == (32, 40, 3)
    assert [c[0] for c in st.calls] == ["load", "audit", "forward", "close"] and st.calls[2] == ("forward", (3, 1, 32, 40), 0.5)
    names = engine.layer_table_names()
    assert len(a) == len(names)
    want = dict((nm, 0) for nm in names)
    want.update(conv6_1=12 - 23, conv2_2=12 - 4)
    assert dict(zip(names, a)) == want


class _AuditStub(object):
    def __init__(self, hot):
        self.hot, self.calls = hot, []

    def set_range_audit(self, on):
        self.calls.append(("audit", bool(on)))

    def range_reset(self):
        self.calls.append(("reset",))

    def forward(self, L, ab, m, maskcent):
        self.calls.append(("forward", L.shape, float(np.abs(ab).max()), float(np.abs(m).max())))

    def range_report(self):
        return [dict(_row(nm, 1.0), n_saturated=5 if nm in self.hot else 0) for nm in engine.layer_table_names()]

    def close(self):
        pass


def test_check_ranges_host_logic():
    m = api.ColorizeImageTorch(Xd=32, precision="fp16x3")
    with pytest.raises(RuntimeError):
        m.check_ranges()
    m.set_image(np.random.RandomState(0).randint(0, 256, (32, 32, 3)).astype(np.uint8))
    m._new_engine(_AuditStub({"conv6_1", "conv6_2"}))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        rep = m.check_ranges()
    assert len(w) == 1 and "conv6_1" in str(w[0].message) and "conv6_2" in str(w[0].message) and "conv5_3" not in str(w[0].message)
    assert "bf16x6" in str(w[0].message) and "calibrate" in str(w[0].message)
    assert [c[0] for c in m.net.calls] == ["audit", "reset", "forward", "audit"] and m.net.calls[-1] == ("audit", False)
    assert m.net.calls[2] == ("forward", (1, 1, 32, 32), 0.0, 0.0) and len(rep) == len(engine.layer_table_names())
    m._new_engine(_AuditStub(set()))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m.check_ranges()
    assert len(w) == 0


def test_calibrate_is_for_fp16x3_only():
    from oracle import weights as oweights  # noqa: F401
    for precision in ("fp32", "bf16", "bf16x6"):
        m = api.ColorizeImageTorch(Xd=32, precision=precision)
        m.set_image(np.zeros((32, 32, 3), np.uint8))
        with pytest.raises(ValueError):
            m.prep_net(state_dict={}, calibrate=True)
    m = api.ColorizeImageTorch(Xd=32, precision="fp16x3")
    with pytest.raises(RuntimeError):                     # calibrate=True without an image
        m.prep_net(state_dict={}, calibrate=True)
    c = api.ColorizeImageCaffe(Xd=32, precision="fp32")
    c.set_image(np.zeros((32, 32, 3), np.uint8))
    with pytest.raises(ValueError):
        c.prep_net(0, state_dict={}, calibrate=True)
