"""GPU checks of the colour picker on the device: idc_gamut_map (abGrid.update_gamut for n lightnesses in one launch) and idc_snap_colors
(snap_ab for n colours in one launch), through HipColorizer, the wrapper (get_gamut, net_forward_hints(snap=True)) and lab_gamut with an
engine bound.  The reference is tests/gamut_ref.py -- the oracle's rgb2lab / lab2rgb in plain loops -- never the code under test;
tests/test_gamut_cpu.py asserts that the inputs used here keep the REFERENCE 1e-6 away from the mask threshold and the stop rule and 1e-9
away from every truncation and rounding edge, so a differing device result is a wrong formula, not a last-bit coincidence.

Bars:
  pts_rgb / rgb_out   the display kernels' bar: at most one uint8 level on at most 2e-4 of the values (the same float64 arithmetic on both
                      sides; pow / cbrt last bits could move a value across an edge -- with the input conditions above the expected count is 0)
  mask                equal to the reference wherever the point's three pts_rgb values are the reference's and the reference distance is
                      1e-6 or more from 1.0; the points left out that way number at most 1e-4 of the grid (at L = 0 the point (a, b) =
                      (-1, 0) maps to black and has d == 1.0 exactly: it is the one left out)
  masked_rgb          exactly where(mask, pts_rgb, 255) of the call's own outputs
  iters               equal to the reference for every pair
  lab_out             1e-9 abs wherever rgb_out equals the reference (the colour kernels' Lab bar; measured ~1e-13)
  a row of a batch    bit-identical to the same input sent alone or in a batch of another size
Shapes: grids (110,1) = 48 841 points, 190 full workgroups and a ragged one; (110,10) = 23 x 23; (5,3), where D does not divide the span;
(1,1).  2103 colours = 8 full workgroups and a ragged one, 257 = one and a single thread, and 1.

Measured on one MI355X: 5.6 s for the file.  The slowest case is the (110,1) grid at 2.6 s, nearly all of it the reference's Python loops
over 4 x 48 841 points (computed once per process: tests/test_gamut_cpu.py shares gamut_ref's cache when both run together); the L = 0 map
takes 0.65 s for the same reason, the resident-state test 1.1 s (it loads weights), every other case under 0.2 s."""
import ctypes

import numpy as np
import pytest

import gamut_ref
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import api, engine, lab_gamut, workloads

pytestmark = pytest.mark.gpu

LAB_TOL = 1e-9
FRAC = 2e-4
EDGE = 1e-6
MASK_EXCLUDED = 1e-4


@pytest.fixture(scope="module")
def eng():
    e = engine.HipColorizer(64, 64, max_batch=1, precision="bf16")             # no weights needed: neither call runs a layer
    yield e
    e.close()


def _check_u8(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, what
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    mx, frac = int(diff.max()), float((diff != 0).mean())
    print("%s: max level difference %d on %.3g of %d values" % (what, mx, frac, want.size))
    assert mx <= 1 and frac <= FRAC, (what, mx, frac)


def _check_map(pts, masked, mask, ref, what):
    """One (A,B) map of a call against the reference's, by the bars above.  Returns the number of points left out of the mask comparison."""
    assert mask.dtype == np.bool_ and mask.shape == ref["mask"].shape
    _check_u8(pts, ref["pts_rgb"], what + " pts_rgb")
    compared = (pts == ref["pts_rgb"]).all(axis=2) & (np.abs(ref["d"] - 1.0) >= EDGE)
    excluded = int((~compared).sum())
    wrong = int((mask != ref["mask"])[compared].sum())
    print("%s: mask compared at %d of %d points, %d differ" % (what, int(compared.sum()), mask.size, wrong))
    assert wrong == 0, (what, np.argwhere((mask != ref["mask"]) & compared)[:5])
    assert excluded <= MASK_EXCLUDED * mask.size, (what, excluded)
    np.testing.assert_array_equal(masked, np.where(mask[..., None], pts, np.uint8(255)), err_msg=what)
    return excluded


# ------------------------------------------------------------------------------------------------ 1. gamut map
@pytest.mark.parametrize("grid", gamut_ref.GRIDS)
def test_gamut_map_matches_the_reference(eng, grid):
    gs, D = grid
    A = len(gamut_ref.grid_axis(gs, D))
    masked, mask, pts = eng.gamut_map(gamut_ref.L_VALUES, gs, D, want_pts=True)
    assert pts.shape == masked.shape == (4, A, A, 3) and mask.shape == (4, A, A)
    for k, L in enumerate(gamut_ref.L_VALUES):
        _check_map(pts[k], masked[k], mask[k], gamut_ref.gamut(L, gs, D), "grid %s L %g" % (grid, L))
    masked1, mask1, pts1 = eng.gamut_map(50.0, gs, D, want_pts=True)            # a scalar is n = 1; the leading axis stays
    assert pts1.shape == (1, A, A, 3) and mask1.shape == (1, A, A)
    k50 = gamut_ref.L_VALUES.index(50.0)
    np.testing.assert_array_equal(pts1[0], pts[k50])
    np.testing.assert_array_equal(mask1[0], mask[k50])
    np.testing.assert_array_equal(masked1[0], masked[k50])
    two = eng.gamut_map(50.0, gs, D)                                            # the default: no pts_rgb
    assert len(two) == 2
    np.testing.assert_array_equal(two[0], masked1)
    np.testing.assert_array_equal(two[1], mask1)


def test_gamut_map_at_l_zero_leaves_out_the_exact_threshold_point_only(eng):
    ref = gamut_ref.gamut(0.0, 110, 1)
    masked, mask, pts = eng.gamut_map(0.0, 110, 1, want_pts=True)
    excluded = _check_map(pts[0], masked[0], mask[0], ref, "grid (110, 1) L 0")
    near = np.argwhere(np.abs(ref["d"] - 1.0) < EDGE)
    assert near.tolist() == [[109, 110]] and ref["d"][109, 110] == 1.0          # (a, b) = (-1, 0) -> black -> d = |a| exactly
    assert excluded == 1                                                        # the other 48 840 were compared


def test_gamut_map_rows_are_a_and_columns_are_b(eng):
    ref = gamut_ref.gamut(50.0, 110, 10)
    assert not np.array_equal(ref["pts_rgb"], ref["pts_rgb"].transpose(1, 0, 2))          # the gamut is not symmetric in a <-> b
    _, _, pts = eng.gamut_map(50.0, 110, 10, want_pts=True)
    axis = gamut_ref.grid_axis(110, 10)
    i, j = list(axis).index(80), list(axis).index(-40)                         # (a, b) = (80, -40): a magenta, (-40, 80) is a green
    np.testing.assert_array_equal(pts[0, i, j], ref["pts_rgb"][i, j])
    assert pts[0, i, j, 0] > pts[0, i, j, 1] and pts[0, j, i, 1] > pts[0, j, i, 0]
    assert np.array_equal(pts[0], ref["pts_rgb"]) and not np.array_equal(pts[0], ref["pts_rgb"].transpose(1, 0, 2))


# ------------------------------------------------------------------------------------------------ 2. snap
def test_snap_colors_matches_the_reference_and_rows_do_not_depend_on_n(eng):
    ref = gamut_ref.snap_set()
    ls, rgbs = ref["ls"], ref["rgbs"]
    rgb, lab, its = eng.snap_colors(ls, rgbs, want_lab=True, want_iters=True)
    assert rgb.shape == (2103, 3) and rgb.dtype == np.uint8 and lab.shape == (2103, 3) and lab.dtype == np.float64
    assert its.shape == (2103,) and its.dtype == np.int32
    bad = np.flatnonzero(its != ref["iters"])
    assert bad.size == 0, [(int(k), float(ls[k]), rgbs[k].tolist(), int(its[k]), int(ref["iters"][k])) for k in bad[:5]]
    _check_u8(rgb, ref["rgb"], "snap rgb_out")
    same = (rgb == ref["rgb"]).all(axis=1)
    err = float(np.abs(lab - ref["lab"])[same].max())
    print("snap lab_out: max abs error %.3e over %d of 2103 colours" % (err, int(same.sum())))
    assert err <= LAB_TOL
    for lo, hi in ((0, 257), (1, 2)):                                           # 257 = a workgroup and one thread; one colour ((0,0,255) at L = 0: 20 rounds)
        r, la, it = eng.snap_colors(ls[lo:hi], rgbs[lo:hi], want_lab=True, want_iters=True)
        np.testing.assert_array_equal(r, rgb[lo:hi])
        np.testing.assert_array_equal(la, lab[lo:hi])
        np.testing.assert_array_equal(it, its[lo:hi])
    assert rgbs[1].tolist() == [0, 0, 255] and ls[1] == 0.0 and its[1] == 20
    one = eng.snap_colors(50.0, np.array([255, 128, 0], np.uint8))             # a scalar L and one colour: n = 1, the leading axis stays
    assert one.shape == (1, 3) and one.dtype == np.uint8
    np.testing.assert_array_equal(one[0], gamut_ref.snap(50.0, (255, 128, 0))["rgb"])
    only_it = eng.snap_colors(ls[:5], rgbs[:5], want_iters=True)
    assert len(only_it) == 2
    np.testing.assert_array_equal(only_it[1], its[:5])


# ------------------------------------------------------------------------------------------------ 3. status codes
def test_invalid_arguments_are_refused_and_leave_the_handle_usable(eng):
    lib, h = eng.lib, eng._h
    vp = ctypes.c_void_p
    L = np.full(65537, 50.0)
    rgb = np.zeros((65537, 3), np.uint8)
    out = np.zeros(65537 * 3, np.uint8)
    Lp, rp, op = L.ctypes.data_as(vp), rgb.ctypes.data_as(vp), out.ctypes.data_as(vp)
    nan, inf = np.array([50.0, np.nan]), np.array([-np.inf])
    good_map = eng.gamut_map(50.0, 5, 3)
    good_snap = eng.snap_colors(50.0, [255, 0, 0])

    def refused(status, word):
        assert status == -1, (status, word)
        msg = lib.idc_last_error(h).decode()
        assert word in msg, (word, msg)
        np.testing.assert_array_equal(eng.gamut_map(50.0, 5, 3)[0], good_map[0])        # the handle still works
        np.testing.assert_array_equal(eng.snap_colors(50.0, [255, 0, 0]), good_snap)

    refused(lib.idc_gamut_map(h, 0, Lp, 5, 1, op, None, None), "0 maps")
    refused(lib.idc_gamut_map(h, 65, Lp, 5, 1, op, None, None), "65 maps")
    refused(lib.idc_gamut_map(h, 1, None, 5, 1, op, None, None), "null L")
    refused(lib.idc_gamut_map(h, 2, nan.ctypes.data_as(vp), 5, 1, op, None, None), "L[1] is not finite")
    refused(lib.idc_gamut_map(h, 1, inf.ctypes.data_as(vp), 5, 1, op, None, None), "L[0] is not finite")
    refused(lib.idc_gamut_map(h, 1, Lp, 0, 1, op, None, None), "gamut_size 0")
    refused(lib.idc_gamut_map(h, 1, Lp, 513, 1, op, None, None), "gamut_size 513")
    refused(lib.idc_gamut_map(h, 1, Lp, 5, 0, op, None, None), "D 0")
    refused(lib.idc_gamut_map(h, 1, Lp, 5, 6, op, None, None), "D 6")
    refused(lib.idc_gamut_map(h, 1, Lp, 5, 1, None, None, None), "every output is null")
    refused(lib.idc_snap_colors(h, 0, Lp, rp, op, None, None), "0 colours")
    refused(lib.idc_snap_colors(h, 65537, Lp, rp, op, None, None), "65537 colours")
    refused(lib.idc_snap_colors(h, 1, None, rp, op, None, None), "null L or rgb")
    refused(lib.idc_snap_colors(h, 1, Lp, None, op, None, None), "null L or rgb")
    refused(lib.idc_snap_colors(h, 2, nan.ctypes.data_as(vp), rp, op, None, None), "L[1] is not finite")
    refused(lib.idc_snap_colors(h, 1, Lp, rp, None, None, None), "every output is null")
    with pytest.raises(N.IdcError) as ei:
        eng.gamut_map(np.nan)
    assert ei.value.status == -1
    # the limits themselves are fine: 64 maps, 65536 colours, each output alone
    masked, mask = eng.gamut_map(np.linspace(1, 99, 64), 1, 1)
    assert mask.shape == (64, 3, 3)
    assert eng.snap_colors(L[:65536], rgb[:65536]).shape == (65536, 3)
    m = np.zeros(9, np.uint8)
    assert lib.idc_gamut_map(h, 1, Lp, 1, 1, None, None, m.ctypes.data_as(vp)) == 0
    np.testing.assert_array_equal(m.reshape(3, 3), eng.gamut_map(50.0, 1, 1)[1][0])
    it = np.zeros(1, np.int32)
    assert lib.idc_snap_colors(h, 1, Lp, rp, None, None, it.ctypes.data_as(vp)) == 0 and 1 <= it[0] <= 20


# ------------------------------------------------------------------------------------------------ 4. resident state
def test_the_two_calls_leave_the_resident_state_alone(make_sd):
    e = engine.HipColorizer(64, 64, max_batch=1, precision="fp32")
    e.load_state_dict(make_sd(0, "he"))
    L, ab, mask = workloads.random_batch(1, 64, seed=7, max_points=4, max_p=3)
    l_out = np.random.RandomState(4).uniform(0, 100, (90, 75))
    rgb0 = e.forward_rgb_lazy(L, ab, mask).copy()
    out0, lab0 = (a.copy() for a in e.fetch_outputs(1))
    up0 = e.upsample_lab2rgb(l_out, "output_ab", "cubic").copy()
    assert np.isfinite(out0).all() and np.abs(out0).max() > 0

    rgb1 = e.forward_rgb_lazy(L, ab, mask).copy()
    serials = (e.l_serial, e.forward_serial)
    e.gamut_map(gamut_ref.L_VALUES, 110, 1, want_pts=True)                      # grows the staging buffer past its first size
    ref = gamut_ref.snap_set()
    e.snap_colors(ref["ls"], ref["rgbs"], want_lab=True, want_iters=True)
    assert (e.l_serial, e.forward_serial) == serials
    out1, lab1 = e.fetch_outputs(1)
    np.testing.assert_array_equal(rgb1, rgb0)
    np.testing.assert_array_equal(out1, out0)
    np.testing.assert_array_equal(lab1, lab0)
    np.testing.assert_array_equal(e.upsample_lab2rgb(l_out, "output_ab", "cubic"), up0)
    np.testing.assert_array_equal(e.forward_rgb_lazy(L, ab, mask), rgb0)
    e.close()


# ------------------------------------------------------------------------------------------------ 5. wrapper and lab_gamut
class _Counting(object):
    """Passes everything on to the engine and counts the two calls."""

    def __init__(self, e):
        self._e, self.n_map, self.n_snap = e, 0, 0

    def gamut_map(self, *a, **kw):
        self.n_map += 1
        return self._e.gamut_map(*a, **kw)

    def snap_colors(self, *a, **kw):
        self.n_snap += 1
        return self._e.snap_colors(*a, **kw)


def test_wrapper_snap_and_lab_gamut_with_an_engine_bound(make_sd):
    m = api.ColorizeImageTorch(Xd=64, precision="bf16")
    m.prep_net(path="", state_dict=make_sd(0, "he"))
    m.set_image(np.random.RandomState(11).randint(0, 256, (64, 64, 3)).astype(np.uint8))
    edits = [(10, 12, 16, 18, 255, 0, 255), (58, 60, 70, 72, 0, 255, 0), (30, 5, 24, 9, 0, 0, 255)]    # the second is clipped by the image edge
    centres = [(13, 15), (60, 61), (27, 7)]
    pre = []
    for (y, x), e in zip(centres, edits):
        r = gamut_ref.snap(float(m.img_l[0, y, x]), e[4:])
        assert min(abs(d - 1.0) for d in r["difs"]) >= EDGE and np.abs(r["s"] - np.floor(r["s"]) - 0.5).min() >= 1e-9   # clear of the knife edges
        pre.append(r["rgb"])
    pre = np.array(pre)
    assert (pre != np.array([e[4:] for e in edits])).any(axis=1).all()          # out of gamut: every colour moved
    got = m.net_forward_hints(edits, snap=True).copy()
    got_ab = m.input_ab.copy()
    np.testing.assert_array_equal(m.snapped_hint_colors, pre)
    want = m.net_forward_hints([e[:4] + tuple(int(v) for v in c) for e, c in zip(edits, pre)])
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_ab, m.input_ab)
    assert not np.array_equal(want, m.net_forward_hints(edits))                 # ... and snapping mattered

    masked, mask = m.get_gamut(13, 15)
    dm, dk = m.net.gamut_map(float(m.img_l[0, 13, 15]))
    np.testing.assert_array_equal(masked, dm[0])
    np.testing.assert_array_equal(mask, dk[0])
    np.testing.assert_array_equal(m.snap_color(13, 15, np.array(edits[0][4:], np.uint8)), pre[0])

    L = float(m.img_l[0, 13, 15])
    colour = np.array([255, 0, 255], np.uint8)
    grid = lab_gamut.abGrid()
    host_masked, host_mask = (a.copy() for a in grid.update_gamut(L))
    host_snap = lab_gamut.snap_ab(L, colour)
    count = _Counting(m.net)
    lab_gamut.set_engine(count)
    try:
        dev_masked, dev_mask = grid.update_gamut(L)
        assert count.n_map == 1
        np.testing.assert_array_equal(dev_masked, dm[0])
        np.testing.assert_array_equal(dev_mask, dk[0])
        np.testing.assert_array_equal(grid.pts_rgb, m.net.gamut_map(L, want_pts=True)[2][0])
        np.testing.assert_array_equal(lab_gamut.snap_ab(L, colour), m.net.snap_colors(L, colour)[0])
        np.testing.assert_array_equal(lab_gamut.snap_ab(L, colour, 'lab'), m.net.snap_colors(L, colour, want_lab=True)[1][0])
        assert count.n_snap == 2
    finally:
        lab_gamut.set_engine(None)
    again_masked, again_mask = grid.update_gamut(L)
    np.testing.assert_array_equal(again_masked, host_masked)
    np.testing.assert_array_equal(again_mask, host_mask)
    np.testing.assert_array_equal(lab_gamut.snap_ab(L, colour), host_snap)
    assert (count.n_map, count.n_snap) == (1, 2)
    m.net.close()
