"""Joint bilateral ab upsampling, the parts that need no device: properties of the numpy restatement (tests/joint_ref.py), the edge claim it
is built for, a mutation check of the GPU file's 1e-9 comparison on that file's own inputs, the C ABI, the ``upsample=`` keyword of the
streaming generators on a stub engine, and the conditions the GPU inputs have to meet.

The inputs are the ones tests/test_joint_gpu.py runs that can be made without a device: joint_ref.SIZES sources on the 32 x 48 net, guided
by joint_ref.guide, with the planes joint_ref.raster(HINTS) (what input_ab holds there).  The network's own output is not available here;
the GPU file asserts the same input conditions on it before it compares."""
import ctypes
import os
import re

import numpy as np
import pytest

import ingest_ref
import joint_ref as J
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9

_CASES = {}


def _case(size):
    """(source L, a_lo, b_lo, L_lo) of one GPU input, made once and never written to."""
    if size not in _CASES:
        src = J.source(*size)
        ab = J.raster(J.HINTS)
        _CASES[size] = (J.source_l(src), ab[0], ab[1], J.guide(src), src)
        for a in _CASES[size]:
            a.setflags(write=False)
    return _CASES[size]


# ------------------------------------------------------------------------------------------------ 1. properties
def _tap_range(plane, h, w, R):
    """[h,w] min and max of the plane over every output pixel's in-image taps."""
    Hn, Wn = plane.shape
    j0 = np.floor((np.arange(h) + 0.5) * (float(Hn) / h) - 0.5 + 0.5).astype(int)
    i0 = np.floor((np.arange(w) + 0.5) * (float(Wn) / w) - 0.5 + 0.5).astype(int)
    lo, hi = np.full((h, w), np.inf), np.full((h, w), -np.inf)
    for y in range(h):
        rows = plane[max(j0[y] - R, 0):j0[y] + R + 1]
        for x in range(w):
            win = rows[:, max(i0[x] - R, 0):i0[x] + R + 1]
            lo[y, x], hi[y, x] = win.min(), win.max()
    return lo, hi


@pytest.mark.parametrize("params", [J.DEFAULT] + J.CORNERS)
def test_output_is_a_finite_convex_combination_of_its_taps(params):
    rs = np.random.RandomState(3)
    for size in [(1, 1), (13, 17), (32, 48), (37, 41), (60, 90)]:
        src = ingest_ref.source_image(size[0], size[1], 11)            # odd seed: noise, every range weight is exercised
        L, L_lo = J.source_l(src), J.guide(src)
        a_lo, b_lo = rs.uniform(-110, 110, (2, J.H, J.W))
        ab, den = J.joint_ab(L, a_lo, b_lo, L_lo, *params, want_den=True)
        assert np.isfinite(ab).all() and den > 0, (size, params, den)
        for ch, plane in enumerate((a_lo, b_lo)):
            lo, hi = _tap_range(plane, size[0], size[1], params[0])
            assert (ab[ch] >= lo - 1e-12).all() and (ab[ch] <= hi + 1e-12).all(), (size, params, ch)


def test_at_the_net_size_a_narrow_kernel_stays_at_the_centre_tap():
    """h = H, w = W, sigma_s = 0.25, sigma_r = 100: u = j exactly, so the centre tap has spatial weight 1, its four edge neighbours e^-8 and
    the four diagonal ones e^-16.  The range factor lies in (eps, 1 + eps], so the neighbours hold at most 4 e^-8 + 4 e^-16 of the weight
    the centre holds times (1 + eps) / (exp(-d^2 / 2e4) + eps) <= (1 + eps) / exp(-0.5) for |d| <= 100; the result is a convex
    combination, so it moves from the centre value by at most that share of the value range."""
    rs = np.random.RandomState(5)
    src = J.source(J.H, J.W)
    L, L_lo = J.source_l(src), J.guide(src)
    a_lo, b_lo = rs.uniform(-110, 110, (2, J.H, J.W))
    ab = J.joint_ab(L, a_lo, b_lo, L_lo, 1, 0.25, 100.0)
    share = (4 * np.exp(-8.0) + 4 * np.exp(-16.0)) * (1 + J.EPS) / np.exp(-0.5)
    bound = share * 220.0
    err = max(np.abs(ab[0] - a_lo).max(), np.abs(ab[1] - b_lo).max())
    print("largest move from the centre value %.4f, bound %.4f" % (err, bound))
    assert 0 < err <= bound


def test_an_image_does_not_depend_on_its_neighbours_in_a_batch():
    """The rule reads one image's source, planes and guide: restating a batch is restating each image, whatever lies next to it."""
    sizes = [(13, 17), (37, 41)]
    alone = [J.joint_ab(*_case(s)[:4]) for s in sizes]
    for order in ([0, 1], [1, 0]):
        batch = [J.joint_ab(*_case(sizes[k])[:4]) for k in order]
        for k, got in zip(order, batch):
            np.testing.assert_array_equal(got, alone[k])


# ------------------------------------------------------------------------------------------------ 2. the edge claim
@pytest.mark.parametrize("offset", [0, 2])
def test_joint_keeps_each_side_of_a_step_edge_and_the_linear_zoom_does_not(offset):
    src, edge = J.step_source(offset)
    ab_lo = J.raster(J.STEP_HINTS)
    L, L_lo = J.source_l(src), J.guide(src)
    want = np.where(np.arange(src.shape[1]) < edge, J.STEP_AB[0], J.STEP_AB[1])[None, None, :]
    joint = J.joint_ab(L, ab_lo[0], ab_lo[1], L_lo)
    linear = ingest_ref.zoom_to(ab_lo, src.shape[0], src.shape[1], 1)
    j_err, l_err = float(np.abs(joint - want).max()), float(np.abs(linear - want).max())
    print("edge offset %d: joint off by %.4f, linear zoom by %.2f" % (offset, j_err, l_err))
    assert j_err <= J.STEP_BOUND
    assert l_err > J.LINEAR_MISS


# ------------------------------------------------------------------------------------------------ 3. mutation check
@pytest.mark.parametrize("variant", ["corner", "replicate", "no_eps", "no_l_cent", "swap_f32"])
def test_the_1e9_comparison_catches_each_mistake_on_the_gpu_inputs(variant):
    caught = []
    for size in J.SIZES:
        L, a_lo, b_lo, L_lo, src = _case(size)
        for params in J.PARAMS:
            want = J.joint_ab(L, a_lo, b_lo, L_lo, *params)
            if variant == "no_l_cent":
                got = J.joint_ab(L, a_lo, b_lo, J.guide(src, with_l_cent=False), *params)
            else:
                got = J.joint_ab(L, a_lo, b_lo, L_lo, *params, variant=variant)
            with np.errstate(invalid="ignore"):
                if not (np.abs(got - want) <= TOL).all():       # (a NaN of 0/0 is a miss too)
                    caught.append((size, params))
    print("%s: caught on %d of %d (size, parameter) cases" % (variant, len(caught), len(J.SIZES) * len(J.PARAMS)))
    assert caught, variant


# ------------------------------------------------------------------------------------------------ 4. ABI
NEW = ("idc_set_joint_upsample", "idc_fullres_ab", "idc_set_batch_upsample")


def test_the_symbols_and_constants_match_the_header():
    header = open(os.path.join(REPO, "include", "ideepcolor.h")).read()
    declared = set(re.findall(r"\b(idc_[a-z0-9_]+)\s*\(", header))
    lib = N.load()
    for sym in NEW:
        assert sym in declared and sym in N.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    assert re.search(r"enum\s*\{\s*IDC_INTERP_JOINT\s*=\s*3\s*\}", header) and N.IDC_INTERP_JOINT == 3
    assert re.search(r"#define\s+IDC_JOINT_EPS\s+1e-6", header) and N.IDC_JOINT_EPS == J.EPS == 1e-6
    for phrase in ("half-pixel centres", "A tap outside [0, H) x [0, W) is skipped", "NOBODY HAS", "fp contract(off)"):
        assert phrase in header, phrase


def test_null_handle_statuses():
    lib = N.load()
    buf = np.zeros(6, np.float64)
    assert lib.idc_set_joint_upsample(None, 2, 1.0, 8.0) == -1
    assert lib.idc_set_batch_upsample(None, N.IDC_INTERP_JOINT) == -1
    assert lib.idc_fullres_ab(None, 0, 0, N.IDC_INTERP_JOINT, buf.ctypes.data_as(ctypes.c_void_p)) == -1
    assert lib.idc_fullres_rgb(None, 0, 0, N.IDC_INTERP_JOINT, 0, buf.ctypes.data_as(ctypes.c_void_p)) == -1


class _Pool(object):
    def take(self, shape, dtype):
        return np.zeros(shape, dtype)


class _Stub(engine.HipColorizer):
    """The streaming generators over an engine that launches nothing: every enqueue records the upsampling in force."""

    def __init__(self):
        self.H, self.W, self.max_batch = 8, 8, 2
        self._batch_upsample = "linear"
        self._pool = _Pool()
        self.calls, self.seen = [], []

    def __del__(self):
        pass

    def set_batch_upsample(self, interp="linear"):
        if interp not in ("linear", "joint"):
            raise ValueError(interp)
        self.calls.append(interp)
        self._batch_upsample = interp

    def _pinned_slices(self, shapes):
        return [np.zeros(s, np.uint8) for s in shapes]

    def wait(self, slot):
        pass

    def dist_bins(self):
        return 313

    def forward_async_rgb(self, slot, rgb, hints, out_rgb, **kw):
        self.seen.append(self._batch_upsample)

    def forward_async_images(self, slot, images, hints, **kw):
        self.seen.append(self._batch_upsample)
        return [np.zeros(a.shape, np.uint8) for a in images]

    def forward_async_eval(self, slot, images, hints, **kw):
        self.seen.append(self._batch_upsample)
        return np.zeros((len(images), 3), np.uint64), None, None

    def forward_async_dist(self, slot, images, hints, **kw):
        self.seen.append(self._batch_upsample)
        n, res = len(images), engine.DistBatch()
        res.out_rgb = [np.zeros(a.shape, np.uint8) for a in images]
        res.peaks, res.sugg_centres, res.sugg_conf = np.zeros((n, 2, 2), np.int32), np.zeros((n * 2, 3, 2)), np.zeros((n * 2, 3))
        res.sse, res.score = np.zeros((n, 3), np.uint64), engine.DistScore()
        res.score.xent, res.score.hits, res.score.cells = np.zeros(n), np.zeros((n, 2), np.uint32), 4
        return res


def _generators(e, upsample):
    img = np.zeros((5, 7, 3), np.uint8)
    items = [img] * 5                                       # three batches of at most two
    c = np.zeros((313, 2), np.float32)
    return {
        "colorize_stream": lambda: e.colorize_stream([(img[None], None)] * 3, out="source", upsample=upsample),
        "colorize_images": lambda: e.colorize_images(items, upsample=upsample),
        "evaluate_images": lambda: e.evaluate_images(items, out="source", upsample=upsample),
        "suggest_images": lambda: e.suggest_images(items, c, peaks=2, K=3, upsample=upsample),
        "score_images": lambda: e.score_images(items, c, upsample=upsample),
    }


@pytest.mark.parametrize("name", ["colorize_stream", "colorize_images", "evaluate_images", "suggest_images", "score_images"])
def test_the_upsample_keyword_sets_and_restores_the_state(name):
    # run to the end: set before the first batch, every batch sees it, the previous setting is back afterwards
    e = _Stub()
    results = list(_generators(e, "joint")[name]())
    assert len(results) in (3, 5) and e.seen == ["joint"] * 3 and e.calls == ["joint", "linear"] and e._batch_upsample == "linear"
    # a previous 'joint' is what comes back, and None touches nothing
    e = _Stub()
    e.set_batch_upsample("joint")
    list(_generators(e, "linear")[name]())
    assert e.calls == ["joint", "linear", "joint"] and set(e.seen) == {"linear"}
    e.calls, e.seen = [], []
    list(_generators(e, None)[name]())
    assert e.calls == [] and set(e.seen) == {"joint"}
    # abandoned after the first result: restored when the generator is closed
    e = _Stub()
    g = _generators(e, "joint")[name]()
    assert e.calls == []                                    # nothing happens before the first next()
    next(g)
    assert e._batch_upsample == "joint"
    g.close()
    assert e.calls == ["joint", "linear"] and e._batch_upsample == "linear"
    # a value that is neither is refused before anything is enqueued
    e = _Stub()
    with pytest.raises(ValueError):
        next(_generators(e, "cubic")[name]())
    assert e.seen == [] and e._batch_upsample == "linear"


# ------------------------------------------------------------------------------------------------ 5. the GPU inputs
@pytest.mark.parametrize("size", J.SIZES)
def test_gpu_inputs_keep_den_away_from_zero_and_bytes_away_from_rounding_edges(size):
    L, a_lo, b_lo, L_lo, _ = _case(size)
    for params in J.PARAMS:
        ab, den = J.joint_ab(L, a_lo, b_lo, L_lo, *params, want_den=True)
        assert den >= 1e-12, (size, params, den)
    if size[0] * size[1] <= 37 * 41:                        # (the oracle's Lab -> RGB is a Python loop per pixel: the small sources)
        frac = J.near_rounding_edge(L, J.joint_ab(L, a_lo, b_lo, L_lo))
        print("%dx%d: %.4f of the bytes within 1e-6 of a rounding edge" % (size[0], size[1], frac))
        assert frac <= 0.02, (size, frac)


def test_step_inputs_meet_the_same_conditions():
    for offset in (0, 2):
        src, _ = J.step_source(offset)
        ab_lo = J.raster(J.STEP_HINTS)
        ab, den = J.joint_ab(J.source_l(src), ab_lo[0], ab_lo[1], J.guide(src), want_den=True)
        assert den >= 1e-12 and np.isfinite(ab).all()
