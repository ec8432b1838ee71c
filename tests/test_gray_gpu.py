"""GPU checks of greyscale sources: idc_set_image_gray, idc_fullres_rgb / idc_fullres_ab on a kept plane, idc_fullres_rgb16 and the
pipelined idc_forward_async_gray, through HipColorizer and the wrapper classes.  The references are the RGB route fed the plane three times
(I8), the uint8 plane g for the uint16 plane 257 g (I16), tests/gray_ref.py (the rule in numpy float64) and, for the pipelined uint16
batches, the blocking route per image -- never the call under test.

Bars (tests/gray_ref.py holds them; tests/test_gray_cpu.py shows that they catch four mutants of the rule):
  (I8), (I16)  bit for bit: the same device functions on the same operands
  gray_net     exact: the GPU inputs keep every unrounded sample further than 1e-6 from a rounding boundary
  l_net, ab    1e-9 absolute, the project's bar for float64 colour arithmetic (tests/test_joint_gpu.py, the same quantities)
  8-bit image  at most one level off the reference's Lab -> RGB of the device's own fullres_ab
  16-bit image equal wherever the reference's s * 65535 is further than 1e-6 from an integer, at most one level off elsewhere, differing
               pixels at most 0.1 % of an image
  pipelined    bit for bit the RGB pipelined call on the replicated planes (I8) and the blocking grey route per image (GRAY16)
Shapes: a 64 x 64 net, max_batch 8, bf16 and fp32; sources gray_ref.SIZES: 1 x 1, one row, one column, 2 x 3, smaller than the net (23 x 31),
the net size and 211 x 83 (several ragged joint tiles, non-integer ratios); their pixel counts cover every residue mod 4.  Section 8c runs planes of
23 x 31, 40 x 72 and 211 x 83, of both widths, on the 40 x 72 net (gray_ref.NET: a swap of H and W anywhere on the grey route shows): the
comparisons and bars of section 3, and one pipelined batch per depth pairing against the blocking route.

Wall time of this file on an MI355X, as measured there: 4.3 s for its 52 tests (pytest's own figure); the slowest test takes 0.8 s, every case of
section 8c is below 0.05 s."""
import ctypes

import numpy as np
import pytest

import glob_ref
import gray_ref as G
import ingest_ref
import joint_ref as J
import ragged_ref as R
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import api, engine, workloads

pytestmark = pytest.mark.gpu

_ENG = {}
SOURCES = ["output_ab", "output_ab_raw", "input_ab", "no_ab"]
INTERPS = ["cubic", "linear", "nearest", "joint"]


@pytest.fixture(scope="module")
def eng(make_sd):
    def get(precision="bf16"):
        if precision not in _ENG:
            e = engine.HipColorizer(G.H, G.W, max_batch=8, precision=precision)
            e.load_state_dict(make_sd(0, "he"))
            _ENG[precision] = e
        return _ENG[precision]
    yield get
    for e in _ENG.values():
        e.close()
    _ENG.clear()


def _rep(g):
    return np.repeat(g[..., None], 3, 2)


def _run(e, ingest):
    """Ingest through ``ingest`` (which keeps the source), hint and run slot 0 -> the raw output and the net-size planes by name."""
    net = ingest()
    e.set_hints(G.HINTS, mode="ab")
    raw, _, lab_q = e.forward_resident(1)
    in_ab, _ = e.hint_planes(0)
    assert np.isfinite(raw).all() and np.abs(raw).max() > 0
    return net, {"output_ab": np.array(lab_q[0, 1:]), "output_ab_raw": np.array(raw[0]), "input_ab": np.array(in_ab)}


def _getters(e, depth=8):
    """Every full-resolution image and ab map the slot's kept source serves, by (source, interp, l_mode)."""
    out = {}
    for source in SOURCES:
        for interp in INTERPS:
            for l_mode in ("image", "mask50"):
                if (interp == "joint" or depth == 16) and l_mode == "mask50":
                    continue
                out[(source, interp, l_mode)] = np.array(e.fullres_rgb(source, interp, l_mode, depth=depth))
            out[(source, interp, "ab")] = np.array(e.fullres_ab(source, interp))
    return out


# ------------------------------------------------------------------------------------------------ 1. (I8)
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("size", G.SIZES)
def test_i8_a_uint8_plane_is_the_rgb_route_of_its_replication(eng, size, precision):
    e = eng(precision)
    g = G.gray8(*size)
    (rgb_net, lab_net), planes_rgb = _run(e, lambda: e.set_image_rgb(_rep(g), keep_source=True))
    rgb_net, lab_net = np.array(rgb_net), np.array(lab_net)
    want = _getters(e)
    (gray_net, l_net), planes = _run(e, lambda: e.set_image_gray(g, keep_source=True))
    assert gray_net.dtype == np.uint8 and gray_net.shape == (1, G.H, G.W) and l_net.shape == (1, G.H, G.W)
    np.testing.assert_array_equal(gray_net, rgb_net[..., 0])
    np.testing.assert_array_equal(l_net, lab_net[:, 0])
    for k in planes:
        np.testing.assert_array_equal(planes[k], planes_rgb[k], err_msg=k)          # the L plane is the same, so the forward is
    got = _getters(e)
    assert sorted(got) == sorted(want) and len(got) == 4 * (3 * 2 + 1 + 4)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=repr(k))
    # several images in one call, into slots 1.., without keeping them
    gs = np.stack([g, g[::-1, ::-1]])
    net2, l2 = e.set_image_gray(gs, img=1)
    rgb2, lab2 = e.set_image_rgb(np.stack([_rep(gs[0]), _rep(gs[1])]), img=1)
    np.testing.assert_array_equal(net2, rgb2[..., 0])
    np.testing.assert_array_equal(l2, lab2[:, 0])


# ------------------------------------------------------------------------------------------------ 2. (I16)
def test_i16_at_the_net_size_257_g_is_g(eng):
    e = eng()
    g = G.gray8(G.H, G.W)
    g16 = (257 * g.astype(np.uint32)).astype(np.uint16)
    (net8, l8), planes8 = _run(e, lambda: e.set_image_gray(g, keep_source=True))
    net8, l8 = np.array(net8), np.array(l8)
    want = _getters(e)
    (net16, l16), planes16 = _run(e, lambda: e.set_image_gray(g16, keep_source=True))
    np.testing.assert_array_equal(net16[0], g16)
    np.testing.assert_array_equal(net8[0], g)
    np.testing.assert_array_equal(G.l_plane(l16), G.l_plane(l8))
    np.testing.assert_array_equal(l16, l8)
    for k in planes8:
        np.testing.assert_array_equal(planes16[k], planes8[k], err_msg=k)
    got = _getters(e)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=repr(k))


# ------------------------------------------------------------------------------------------------ 3. GRAY16 against the rule
@pytest.mark.parametrize("size", G.SIZES)
def test_gray16_matches_the_rule(eng, size):
    e = eng()
    g = G.gray16(*size)
    (net, l_net), planes = _run(e, lambda: e.set_image_gray(g, keep_source=True))
    want_net = G.resize(g)
    ok, _ = G.same(net[0], want_net)
    assert ok, size
    ok, fig = G.close(l_net[0], G.lightness(want_net), G.L_TOL)
    print("%dx%d: l_net off by %.3e" % (size[0], size[1], fig["err"]))
    assert ok, (size, fig)
    L, L_lo = G.lightness(g), G.guide(G.lightness(want_net))
    for name, ab_lo in planes.items():
        for interp, want in (("linear", ingest_ref.zoom_to(ab_lo, size[0], size[1], 1)), ("joint", J.joint_ab(L, ab_lo[0], ab_lo[1], L_lo))):
            ab = np.array(e.fullres_ab(name, interp))
            ok, fig = G.close(ab, want, G.AB_TOL)
            print("%dx%d %s %s: ab off by %.3e" % (size[0], size[1], name, interp, fig["err"]))
            assert ok, (size, name, interp, fig)
            ok, fig = G.within_one_level(e.fullres_rgb(name, interp), G.image(g, ab, 8))
            assert ok, (size, name, interp, fig)
            got16 = e.fullres_rgb(name, interp, depth=16)
            assert got16.dtype == np.uint16 and got16.shape == size + (3,)
            ok, fig = G.image16_matches(got16, g, ab)
            print("%dx%d %s %s: 16-bit image %s" % (size[0], size[1], name, interp, fig))
            assert ok, (size, name, interp, fig)
    for interp in INTERPS:                                                          # no ab: a grey image, whatever the interp
        ok, fig = G.image16_matches(e.fullres_rgb("no_ab", interp, depth=16), g, np.zeros((2,) + size))
        assert ok, (size, interp, fig)


# ------------------------------------------------------------------------------------------------ 4. the 16 bits matter
def test_a_ramp_of_300_codes_survives_only_the_16_bit_route(eng):
    e = eng()
    r = G.ramp16()
    e.set_image_gray(r, keep_source=True, want_net=False, want_l=False)
    out16 = e.fullres_rgb("no_ab", "linear", depth=16)
    distinct16 = [len(np.unique(out16[..., c])) for c in range(3)]
    e.set_image_gray((r >> 8).astype(np.uint8), keep_source=True, want_net=False, want_l=False)
    out8 = e.fullres_rgb("no_ab", "linear")
    distinct8 = [len(np.unique(out8[..., c])) for c in range(3)]
    print("distinct values per channel: 16-bit route %s, 8-bit route %s" % (distinct16, distinct8))
    assert max(distinct16) > 256
    assert max(distinct8) <= 2


# ------------------------------------------------------------------------------------------------ 5. no leakage
def test_rgb_calls_give_the_same_bytes_after_grey_calls(eng):
    e = eng()
    src = J.source(37, 41)

    def rgb_route():
        net, planes = _run(e, lambda: e.set_image_rgb(src, keep_source=True))
        return [np.array(net[0]), np.array(net[1])] + [planes[k] for k in sorted(planes)] + \
               [np.array(e.fullres_rgb("output_ab", i, "image")) for i in INTERPS] + [np.array(e.fullres_ab("output_ab", "joint"))]

    before = rgb_route()
    for g in (G.gray16(23, 31), G.gray8(211, 83)):
        e.set_image_gray(g, keep_source=True)
        e.fullres_rgb("input_ab", "joint")
        e.fullres_ab("input_ab", "linear")
    e.fullres_rgb("no_ab", "linear")
    after = rgb_route()
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 6. statuses
def test_statuses(eng, make_sd):
    e = eng()
    lib, h, vp = e.lib, e._h, ctypes.c_void_p
    px = np.zeros(64, np.uint16)
    p = px.ctypes.data_as(vp)
    odd = vp(px.ctypes.data + 1)
    assert lib.idc_set_image_gray(h, 0, 1, 1, 1, 12, p, 50.0, 0, None, None) == -1           # bits
    assert lib.idc_set_image_gray(h, 0, 1, 1, 1, 0, p, 50.0, 0, None, None) == -1
    assert lib.idc_set_image_gray(h, 0, 1, 1, 1, 16, None, 50.0, 0, None, None) == -1        # null pix
    assert lib.idc_set_image_gray(h, 0, 1, 1, 1, 16, odd, 50.0, 0, None, None) == -1         # odd pix at 16 bits ...
    assert lib.idc_set_image_gray(h, 0, 1, 1, 1, 8, odd, 50.0, 0, None, None) == 0           # ... is fine at 8
    assert lib.idc_set_image_gray(h, 0, 1, 1, 1, 16, p, 50.0, 2, None, None) == -1           # unknown flag bit
    assert lib.idc_set_image_gray(h, 0, 1, 0, 5, 16, p, 50.0, 0, None, None) == -1           # src_h = 0
    assert lib.idc_set_image_gray(h, 0, 1, 1, 16385, 16, p, 50.0, 0, None, None) == -1       # src_w beyond the limit
    assert lib.idc_set_image_gray(h, 0, 0, 1, 1, 16, p, 50.0, 0, None, None) == -6           # n = 0
    assert lib.idc_set_image_gray(h, 7, 2, 1, 1, 16, p, 50.0, 0, None, None) == -6           # slots 7..8 of 8
    out = np.zeros(64, np.uint16)
    po, po_odd = out.ctypes.data_as(vp), vp(out.ctypes.data + 1)
    L, LIN = N.IDC_SRC_NO_AB, N.IDC_INTERP_LINEAR
    # idc_fullres_rgb16 wants a kept 16-bit plane: not a slot without a source, not an RGB source, not a uint8 plane, not one that was not kept
    e.set_image_gray(np.zeros((2, 2), np.uint16))
    assert lib.idc_fullres_rgb16(h, 0, L, LIN, po) == -7
    e.set_image_rgb(np.zeros((2, 2, 3), np.uint8), keep_source=True)
    assert lib.idc_fullres_rgb16(h, 0, L, LIN, po) == -7
    e.set_image_gray(np.zeros((2, 2), np.uint8), keep_source=True)
    assert lib.idc_fullres_rgb16(h, 0, L, LIN, po) == -7
    with pytest.raises(N.IdcError) as ei:
        e.fullres_rgb("no_ab", "linear", depth=16)
    assert ei.value.status == -7
    assert e.fullres_rgb("no_ab", "linear").shape == (2, 2, 3)                               # ... and the uint8 plane is still served
    e.set_image_gray(np.full((2, 2), 40000, np.uint16), keep_source=True)
    assert lib.idc_fullres_rgb16(h, 0, L, LIN, None) == -1
    assert lib.idc_fullres_rgb16(h, 0, L, LIN, po_odd) == -1
    assert lib.idc_fullres_rgb16(h, 0, 4, LIN, po) == -1                                     # the codes of idc_fullres_rgb: unknown source,
    assert lib.idc_fullres_rgb16(h, 0, L, 4, po) == -1                                       # interp beyond 3,
    assert lib.idc_fullres_rgb16(h, 8, L, LIN, po) == -6                                     # slot outside the handle
    assert lib.idc_fullres_rgb16(h, 0, L, LIN, po) == 0
    flat = np.full((2, 2), 40000, np.uint16)                                                 # the 2 x 2 image, and not a byte more
    assert G.image16_matches(out[:12].reshape(2, 2, 3), flat, np.zeros((2, 2, 2)))[0] and out[12] == 0
    # a grey source has no colour to reveal or to score against
    with pytest.raises(N.IdcError) as ei:
        e.reveal_hints([(0, 0, 3, 3)], img=0)
    assert ei.value.status == -7 and "greyscale" in str(ei.value)
    # writing the slot's L plane by another route drops the kept plane, as it drops an RGB source
    e.set_image_l(np.zeros((G.H, G.W), np.float32))
    assert lib.idc_fullres_rgb16(h, 0, L, LIN, po) == -7
    d = engine.HipColorizer(G.H, G.W, max_batch=2, precision="bf16", dist=True)
    try:
        d.load_state_dict(make_sd(0, "he"))
        d.set_image_gray(G.gray16(23, 31), keep_source=True)
        d.set_hints([], mode="ab")
        d.forward_resident(1)
        with pytest.raises(N.IdcError) as ei:
            d.dist_score(np.zeros((d.dist_bins(), 2), np.float32), n=1)
        assert ei.value.status == -7 and "greyscale" in str(ei.value)
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 7. pipelined: (I8)
def _planes(dtype, order=1, seed=0):
    make = G.gray8 if dtype == np.uint8 else G.gray16
    return [make(sh, sw, seed) for sh, sw in G.BATCH[::order]]


def _pair(e, slot, g8, hints, out, **kw):
    """The grey call and the RGB call on the replicated planes, one after the other on one slot -> (rgb_out, out_ab) of each."""
    n = len(g8)
    res = []
    for call, images in ((e.forward_async_gray, g8), (e.forward_async_images, [np.ascontiguousarray(_rep(g)) for g in g8])):
        ab = np.full((n, 2, G.H, G.W), 7, np.float32)
        outs = call(slot, images, hints, out_ab=ab, out=out, **kw)
        e.wait(slot)
        res.append(([np.array(o) for o in outs], ab))
    return res


@pytest.mark.parametrize("upsample", ["linear", "joint"])
def test_i8_pipelined_is_the_rgb_call_on_the_replicated_planes(eng, upsample):
    e = eng()
    e.set_batch_upsample(upsample)
    try:
        for slot, order in ((0, 1), (1, -1)):
            g8 = _planes(np.uint8, order)
            n = len(g8)
            if order == 1:                                                      # (reversed, the starts fall on other residues again)
                assert sorted(set(s % 4 for s in G.starts([g.shape for g in g8]))) == [0, 1, 2, 3]
            for mode, rows in (("ab", G.HINTS), ("rgb", G.RGB_HINTS)):
                for out in ("net", "source"):
                    (got, got_ab), (want, want_ab) = _pair(e, slot, g8, G.hint_lists(n, rows), out, mode=mode)
                    np.testing.assert_array_equal(got_ab, want_ab)
                    assert np.abs(got_ab).max() > 0
                    for i in range(n):
                        assert got[i].dtype == np.uint8 and got[i].shape == (g8[i].shape + (3,) if out == "source" else (G.H, G.W, 3))
                        np.testing.assert_array_equal(got[i], want[i], err_msg="image %d, %s, %s, slot %d" % (i, mode, out, slot))
            assert np.isfinite(e.pipeline_times(slot)).all()
        # pinned and pageable buffers mixed within a call: every other plane and every third result pinned
        g8 = _planes(np.uint8)
        src = [g if i % 2 else e.pinned_empty(g.shape, np.uint8) for i, g in enumerate(g8)]
        for s, g in zip(src, g8):
            s[...] = g
        outs = [np.zeros(g.shape + (3,), np.uint8) if i % 3 else e.pinned_empty(g.shape + (3,), np.uint8) for i, g in enumerate(g8)]
        e.forward_async_gray(0, src, G.hint_lists(len(g8)), out_rgb=outs, out="source")
        e.wait(0)
        want = e.forward_async_images(1, [np.ascontiguousarray(_rep(g)) for g in g8], G.hint_lists(len(g8)), out="source")
        e.wait(1)
        for i in range(len(g8)):
            np.testing.assert_array_equal(outs[i], want[i], err_msg="image %d" % i)
    finally:
        e.set_batch_upsample("linear")


def test_i8_pipelined_with_references():
    from test_glob_ref_gpu import _glob_sd
    e = engine.HipColorizer(G.H, G.W, max_batch=8, precision="bf16", global_hints=True)
    try:
        e.load_state_dict(_glob_sd(3))
        c, r = glob_ref.centres(), glob_ref.refs64()
        g8 = _planes(np.uint8)[3:]
        index = [1, -1, 0, 1]
        kw = dict(refs=[r[0], r[1]], ref_index=index, centres=c, saturation=True)
        (got, got_ab), (want, want_ab) = _pair(e, 1, g8, G.hint_lists(4), "source", **kw)
        np.testing.assert_array_equal(got_ab, want_ab)
        for i in range(4):
            np.testing.assert_array_equal(got[i], want[i])
        (_, plain_ab), _ = _pair(e, 0, g8, G.hint_lists(4), "source")
        assert np.abs(plain_ab - got_ab).max() > 0                                  # the references were read
    finally:
        e.close()


def _grid529():
    axis = np.arange(-110, 120, 10)
    return np.ascontiguousarray(np.array(np.meshgrid(axis, axis)).reshape((2, 529)).T.astype(np.float32))


def test_i8_taps_are_forward_async_dists(make_sd):
    e = engine.HipColorizer(G.H, G.W, max_batch=8, precision="bf16", dist=True)
    try:
        e.load_state_dict(make_sd(0, "he"))
        c = _grid529()
        g8 = _planes(np.uint8)
        n, hints = len(g8), G.hint_lists(len(g8))
        kw = dict(peaks=3, radius=2, skip_hints=True, queries="peaks", K=4, N_draws=64, seed=40)
        got = e.forward_async_gray(0, g8, hints, out="source", bin_centres=c, **kw)
        e.wait(0)
        got = [np.array(x) for x in (got.peaks, got.peak_ent, got.sugg_centres, got.sugg_conf)] + [np.array(o) for o in got.out_rgb]
        want = e.forward_async_dist(1, [np.ascontiguousarray(_rep(g)) for g in g8], hints, out="source", want_rgb=True, centres=c, **kw)
        e.wait(1)
        want = [np.array(x) for x in (want.peaks, want.peak_ent, want.sugg_centres, want.sugg_conf)] + [np.array(o) for o in want.out_rgb]
        assert got[0].shape == (n, 3, 2) and got[2].shape == (n * 3, 4, 2) and (got[0] >= 0).any()
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
        # the generator: the same peaks and suggestions per image, whatever the grouping
        res = list(e.suggest_gray(g8, c, batch=3, peaks=3, radius=2, skip_hints=True, K=4, N_draws=64, seed=40))
        assert len(res) == n
        plain = list(e.suggest_gray(g8, c, batch=8, peaks=3, radius=2, skip_hints=True, K=4, N_draws=64, seed=40))
        for i in range(n):
            assert res[i][0].shape == g8[i].shape + (3,)
            for a, b in zip(res[i], plain[i]):
                np.testing.assert_array_equal(a, b)
        # without a result pointer nothing is colourised for the caller
        only = e.forward_async_gray(0, g8, None, want_rgb=False, peaks=2)
        e.wait(0)
        assert only.out_rgb is None and np.array(only.peaks).shape == (n, 2, 2)
        # a handle without a distribution head refuses the taps and stays usable
        p = engine.HipColorizer(G.H, G.W, max_batch=8, precision="bf16")
        p.load_state_dict(make_sd(0, "he"))
        with pytest.raises(N.IdcError) as ei:
            p.forward_async_gray(0, g8, None, peaks=2)
        assert ei.value.status == -7
        assert len(p.forward_async_gray(0, g8, None)) == n
        p.wait(0)
        p.close()
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 8. pipelined: GRAY16 is the blocking route
_BLOCK = {}


def _blocking(e, g, hints, interp, depth):
    k = (e.H, e.W, g.shape, g.dtype.str, g.tobytes(), repr(hints), interp, depth)
    if k not in _BLOCK:
        e.set_image_gray(g, keep_source=True, want_net=False, want_l=False)
        e.set_hints(hints or [], mode="ab")
        raw = np.array(e.forward_resident(1)[0][0])
        out = np.array(e.fullres_rgb("output_ab", interp, "image", depth=depth))
        out.setflags(write=False)
        _BLOCK[k] = (out, raw)
    return _BLOCK[k]


@pytest.mark.parametrize("upsample", ["linear", "joint"])
def test_gray16_pipelined_equals_blocking(eng, upsample):
    e = eng()
    e.set_batch_upsample(upsample)
    try:
        for depth in (8, 16):
            for slot, order in ((0, 1), (1, -1)):
                g16 = _planes(np.uint16, order)
                hints = G.hint_lists(len(g16))
                ab = np.empty((len(g16), 2, G.H, G.W), np.float32)
                outs = e.forward_async_gray(slot, g16, hints, out_ab=ab, out="source", depth=depth)
                e.wait(slot)
                outs = [np.array(o) for o in outs]
                for i, g in enumerate(g16):
                    want, raw = _blocking(e, g, hints[i], upsample, depth)
                    assert outs[i].dtype == want.dtype and outs[i].shape == want.shape
                    np.testing.assert_array_equal(outs[i], want, err_msg="image %d depth %d slot %d" % (i, depth, slot))
                    np.testing.assert_array_equal(ab[i], raw)
        # two batches in flight, one of each width, each keeping its own format
        g16, g8 = _planes(np.uint16), _planes(np.uint8, -1)
        o16 = e.forward_async_gray(0, g16, None, out="source", depth=16)
        o8 = e.forward_async_gray(1, g8, None, out="source")
        e.wait(0); e.wait(1)
        for i, g in enumerate(g16):
            np.testing.assert_array_equal(o16[i], _blocking(e, g, None, upsample, 16)[0])
        for i, g in enumerate(g8):
            np.testing.assert_array_equal(o8[i], _blocking(e, g, None, upsample, 8)[0])
        for slot in (0, 1):
            t = e.pipeline_times(slot)
            assert t.shape == (6,) and np.isfinite(t).all() and np.all(np.diff(t) >= -1e-3)
        # the generators: a change of dtype closes a group, the order is the input's
        items = [g16[1], g16[4], g8[2], g8[0], g16[6]]
        res = list(e.colorize_gray(items, batch=4))
        assert [r.shape for r in res] == [g.shape + (3,) for g in items]
        for r, g in zip(res, items):
            np.testing.assert_array_equal(r, _blocking(e, g, None, upsample, 8)[0])
        res = list(e.colorize_gray([g16[4], g16[6]], depth=16))
        for r, g in zip(res, [g16[4], g16[6]]):
            np.testing.assert_array_equal(r, _blocking(e, g, None, upsample, 16)[0])
    finally:
        e.set_batch_upsample("linear")


# ------------------------------------------------------------------------------------------------ 8b. pipelined: groups that span many planes
_ALONE = {}


def _alone(e, g, hints, depth):
    """The plane sent alone (n = 1) through the pipelined call -> (source-size image, out_ab [2,H,W]).  Made once, never written to."""
    k = (g.shape, g.dtype.str, g.tobytes(), repr(hints), depth)
    if k not in _ALONE:
        ab = np.empty((1, 2, G.H, G.W), np.float32)
        outs = e.forward_async_gray(1, [g], [hints], out_ab=ab, out="source", depth=depth)
        e.wait(1)
        out = np.array(outs[0])
        for a in (out, ab):
            a.setflags(write=False)
        _ALONE[k] = (out, ab[0])
    return _ALONE[k]


@pytest.mark.parametrize("dtype,depth", [(np.uint8, 8), (np.uint16, 8), (np.uint16, 16)], ids=["u8_to_u8", "u16_to_u8", "u16_to_u16"])
@pytest.mark.parametrize("case", range(len(R.SPANS)), ids=["four_in_one_group", "tail_is_an_image", "three_boundaries"])
def test_groups_that_span_many_planes(eng, case, dtype, depth):
    """test_ragged_batch_gpu.py::test_groups_that_span_many_images for planes: four 1 x 1 images in one 4-pixel group, a byte-access tail that
    is an image of its own, three boundaries in one group.  The carry into the next image is the RGB kernel's; which source dword a pixel's
    sample sits in and which result dwords take its three values depend on the format.  Each image equals the plane sent alone, bit for bit."""
    e = eng()
    assert (e.H, e.W) == (64, 64)
    make = G.gray8 if dtype == np.uint8 else G.gray16
    planes = [make(sh, sw, 500 + 20 * case + j) for j, (sh, sw) in enumerate(R.sizes(R.SPANS[case], G.H, G.W))]
    n = len(planes)
    hints = [G.HINTS[(i + 1) % 4:] for i in range(n)]
    assert any(len(set(grp)) > 1 for grp in R.groups([p.shape for p in planes])[0])       # a group does span images
    outs = [np.full(p.shape + (3,), 7, np.uint16 if depth == 16 else np.uint8) for p in planes]
    ab = np.full((n, 2, G.H, G.W), 7, np.float32)
    got = e.forward_async_gray(0, planes, hints, out_rgb=outs, out_ab=ab, out="source", depth=depth)
    e.wait(0)
    assert all(g is o for g, o in zip(got, outs))
    assert np.abs(ab).max() > 0
    for i, p in enumerate(planes):
        want, want_ab = _alone(e, p, hints[i], depth)
        assert outs[i].dtype == want.dtype and outs[i].shape == want.shape
        np.testing.assert_array_equal(outs[i], want, err_msg="image %d (%dx%d)" % ((i,) + p.shape))
        np.testing.assert_array_equal(ab[i], want_ab, err_msg="out_ab of image %d" % i)


# ------------------------------------------------------------------------------------------------ 8c. a net that is not square (40 x 72)
# gray_ref.NET: every kernel of the grey route takes (H, W) -- the resize, net_sample, zoom_nearest, interp_ab, the joint tile -- and a swap of
# the two is invisible on 64 x 64 (tests/test_gray_cpu.py shows both).  The same comparisons and bars as section 3, for both sample widths.
@pytest.fixture(scope="module")
def en(make_sd):
    x = engine.HipColorizer(G.NET[0], G.NET[1], max_batch=8, precision="bf16")
    x.load_state_dict(make_sd(0, "he"))
    yield x
    x.close()


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("size", G.NET_SIZES, ids=["%dx%d" % s for s in G.NET_SIZES])
def test_a_plane_on_the_40x72_net_matches_the_rule(en, size, dtype):
    H, W = G.NET
    assert (en.H, en.W) == (H, W)
    g = (G.gray8 if dtype == np.uint8 else G.gray16)(*size, net=G.NET)
    net, l_net = en.set_image_gray(g, keep_source=True)
    en.set_hints(G.NET_HINTS, mode="ab")
    raw, _, lab_q = en.forward_resident(1)
    assert np.isfinite(raw).all() and np.abs(raw).max() > 0
    planes = {"output_ab": np.array(lab_q[0, 1:]), "input_ab": np.array(en.hint_planes(0)[0])}
    want_net = G.resize(g, H, W)
    ok, _ = G.same(net[0], want_net)
    assert ok, size
    ok, fig = G.close(l_net[0], G.lightness(want_net), G.L_TOL)
    print("%dx%d %s: l_net off by %.3e" % (size[0], size[1], g.dtype, fig["err"]))
    assert ok, (size, fig)
    L, L_lo = G.lightness(g), G.guide(G.lightness(want_net))
    for name, ab_lo in planes.items():
        assert ab_lo.shape == (2, H, W)
        for interp, want in (("linear", ingest_ref.zoom_to(ab_lo, size[0], size[1], 1)), ("joint", J.joint_ab(L, ab_lo[0], ab_lo[1], L_lo))):
            ab = np.array(en.fullres_ab(name, interp))
            ok, fig = G.close(ab, want, G.AB_TOL)
            print("%dx%d %s %s %s: ab off by %.3e" % (size[0], size[1], g.dtype, name, interp, fig["err"]))
            assert ok, (size, name, interp, fig)
            ok, fig = G.within_one_level(en.fullres_rgb(name, interp), G.image(g, ab, 8))
            assert ok, (size, name, interp, fig)
            if dtype == np.uint16:
                got16 = en.fullres_rgb(name, interp, depth=16)
                assert got16.dtype == np.uint16 and got16.shape == size + (3,)
                ok, fig = G.image16_matches(got16, g, ab)
                print("%dx%d %s %s: 16-bit image %s" % (size[0], size[1], name, interp, fig))
                assert ok, (size, name, interp, fig)


@pytest.mark.parametrize("dtype,depth", [(np.uint8, 8), (np.uint16, 8), (np.uint16, 16)], ids=["u8_to_u8", "u16_to_u8", "u16_to_u16"])
def test_a_batch_on_the_40x72_net_equals_the_blocking_route(en, dtype, depth):
    planes = [(G.gray8 if dtype == np.uint8 else G.gray16)(sh, sw, net=G.NET) for sh, sw in G.NET_SIZES]
    hints = [G.NET_HINTS[1:], None, G.NET_HINTS]
    try:
        for slot, upsample in ((0, "linear"), (1, "joint")):
            en.set_batch_upsample(upsample)
            ab = np.empty((len(planes), 2, en.H, en.W), np.float32)
            outs = en.forward_async_gray(slot, planes, hints, out_ab=ab, out="source", depth=depth)
            en.wait(slot)
            for i, g in enumerate(planes):
                want, raw = _blocking(en, g, hints[i], upsample, depth)
                assert outs[i].dtype == want.dtype and outs[i].shape == want.shape == g.shape + (3,)
                np.testing.assert_array_equal(outs[i], want, err_msg="image %d, %s" % (i, upsample))
                np.testing.assert_array_equal(ab[i], raw)
    finally:
        en.set_batch_upsample("linear")


# ------------------------------------------------------------------------------------------------ 9. pipelined: leakage and statuses
def test_rgb_batches_give_the_same_bytes_after_grey_batches(eng):
    e = eng()
    images = [J.source(37, 41), J.source(13, 17), J.source(64, 64)]

    def rgb_batch(slot, out):
        ab = np.empty((3, 2, G.H, G.W), np.float32)
        outs = e.forward_async_images(slot, images, G.hint_lists(3), out_ab=ab, out=out)
        e.wait(slot)
        return [np.array(o) for o in outs] + [ab]

    before = [rgb_batch(s, o) for s in (0, 1) for o in ("net", "source")]
    for slot in (0, 1):
        e.forward_async_gray(slot, _planes(np.uint16), None, out="source", depth=16)
        e.wait(slot)
        e.forward_async_gray(slot, _planes(np.uint8), G.hint_lists(7), out="net")
        e.wait(slot)
    after = [rgb_batch(s, o) for s in (0, 1) for o in ("net", "source")]
    for b, a in zip(before, after):
        for x, y in zip(b, a):
            np.testing.assert_array_equal(x, y)


def test_pipelined_statuses_and_a_refused_call_leaves_the_slot_usable(eng):
    e = eng()
    lib, h, vp = e.lib, e._h, ctypes.c_void_p
    px, out = np.zeros(64, np.uint16), np.zeros(256, np.uint16)
    SRC, R16 = N.IDC_BATCH_OUT_SOURCE, N.IDC_BATCH_OUT_RGB16

    def call(bits=16, n=2, pix=px.ctypes.data, outp=out.ctypes.data, flags=SRC, mode=0, slot=0, null_images=False, null_outs=False, hw=(2, 3)):
        tab = (N.GrayImage * 2)()
        outs = (vp * 2)()
        for i in range(2):
            tab[i].pix, tab[i].h, tab[i].w = pix, hw[0], hw[1]
            outs[i] = outp
        return lib.idc_forward_async_gray(h, slot, n, bits, None if null_images else tab, None, None, mode, 1.0, 0.0, 50.0, flags, None,
                                          None if null_outs else outs, None, None)

    assert call(bits=12) == -1 and call(bits=0) == -1 and call(bits=24) == -1
    assert call(mode=N.IDC_HINT_REVEAL) == -1
    assert call(bits=8, flags=SRC | R16) == -1                      # 16-bit out of 8-bit samples
    assert call(flags=R16) == -1                                    # 16-bit out at the net size
    assert call(flags=4) == -1 and call(flags=SRC | 8) == -1        # unknown flag bits
    assert call(pix=px.ctypes.data + 1) == -1                       # odd pix at 16 bits
    assert call(flags=SRC | R16, outp=out.ctypes.data + 1) == -1    # odd rgb_out at 16 bits out
    assert call(null_images=True) == -1 and call(null_outs=True) == -1
    assert call(hw=(0, 3)) == -1 and call(hw=(2, 16385)) == -1
    assert call(slot=2) == -1
    assert call(n=0) == -6 and call(n=9) == -6
    assert b"" != lib.idc_last_error(h)
    # nothing was enqueued by any of them: the slot takes the next call, which runs, and refuses a second one until it is waited for
    assert call(bits=8, pix=px.ctypes.data + 1, outp=out.ctypes.data + 1) == 0        # uint8 samples and results lie anywhere
    assert call(bits=8) == -1
    assert lib.idc_wait(h, 0) == 0
    assert call(flags=SRC | R16) == 0
    assert lib.idc_wait(h, 0) == 0
    assert not out[18:].any()                                       # 2 x 3 pixels of three uint16 (both images at one address), and not a byte more
    # the existing calls keep refusing planes and the new flag
    with pytest.raises(ValueError):
        e.forward_async_images(0, [np.zeros((4, 4), np.uint8)], None)
    tab = (N.RefImage * 1)()
    tab[0].rgb, tab[0].h, tab[0].w = px.ctypes.data, 2, 2
    outs = (vp * 1)(out.ctypes.data)
    assert lib.idc_forward_async_images(h, 0, 1, tab, None, None, 0, 1.0, 0.0, 50.0, R16, None, outs, None) == -1


# ------------------------------------------------------------------------------------------------ 10. the wrapper
def test_wrapper_single_channel_route(make_sd, tmp_path):
    from PIL import Image
    g16, g8 = G.gray16(211, 83), G.gray8(23, 31)
    hab, hm = workloads.hints_config2(64, 5, 3, 0)
    model = api.ColorizeImageTorch(Xd=64, precision="bf16")
    model.prep_net(path="", state_dict=make_sd(0, "he"))
    e = model.net
    # a 16-bit PNG stays single-channel and 16-bit all the way
    path = str(tmp_path / "scan16.png")
    Image.fromarray(g16).save(path)
    with Image.open(path) as im:
        assert im.mode.startswith("I;16")
    model.load_image_device(path)
    np.testing.assert_array_equal(model.img_gray_fullres, g16)
    assert model.img_rgb.shape == (64, 64, 3) and model.img_rgb_fullres.shape == (211, 83, 3) and model.img_rgb_fullres.dtype == np.uint8
    assert float(np.abs(model.img_l[0] - G.lightness(G.resize(g16))).max()) <= G.L_TOL
    model.net_forward(hab, hm)
    out16, out8, joint16 = model.get_img_fullres(depth=16), model.get_img_fullres(), model.get_img_fullres_joint(depth=16)
    assert model._src_resident and model._fullres_lab_pending                   # the device route: no full-resolution Lab was made on the host
    assert out16.dtype == np.uint16 and out16.shape == (211, 83, 3) and out8.dtype == np.uint8 and joint16.dtype == np.uint16
    np.testing.assert_array_equal(out16, e.fullres_rgb("output_ab", "linear", "image", depth=16))
    np.testing.assert_array_equal(joint16, e.fullres_rgb("output_ab", "joint", "image", depth=16))
    ok, fig = G.image16_matches(out16, g16, np.array(e.fullres_ab("output_ab", "linear")))
    assert ok, fig
    assert float(np.abs(model.img_l_fullres[0] - G.lightness(g16)).max()) <= 1e-12      # the lazy host Lab comes from the 16-bit samples
    with pytest.raises(RuntimeError):
        model.net_forward_reveal([(0, 0, 5, 5)])
    # an 8-bit plane through set_image_device; depth=16 is refused for it
    model.set_image_device(g8)
    model.net_forward(hab, hm)
    np.testing.assert_array_equal(model.get_img_fullres(), e.fullres_rgb("output_ab", "linear", "image"))
    np.testing.assert_array_equal(model.img_rgb[..., 1], G.resize(g8))
    with pytest.raises(RuntimeError):
        model.get_img_fullres(depth=16)
    path8 = str(tmp_path / "scan8.png")
    Image.fromarray(g8).save(path8)
    model.load_image_device(path8)
    np.testing.assert_array_equal(model.img_gray_fullres, g8)
    for bad in (np.zeros((4, 4), np.float32), np.zeros((4, 4), np.int32)):
        with pytest.raises(ValueError):
            model.set_image_device(bad)
    # an RGB image afterwards: the colour route as before
    rgb = J.source(37, 41)
    model.set_image_device(rgb)
    assert not model._src_gray_bits
    model.net_forward(hab, hm)
    assert model.get_img_fullres().shape == (37, 41, 3)
    with pytest.raises(RuntimeError):
        model.get_img_fullres(depth=16)
    e.close()
    d = api.ColorizeImageTorchDist(Xd=64, precision="bf16")
    d.prep_net(path="", state_dict=make_sd(0, "he"))
    d.set_image_device(g16)
    d.net_forward(hab, hm)
    with pytest.raises(RuntimeError) as ei:
        d.score_dist()
    assert "single-channel" in str(ei.value)
    d.net.close()
