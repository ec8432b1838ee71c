"""What a call returns does not depend on the sizes earlier calls on the handle used: the handle's grow-on-demand buffers (hint list, display
upsample, ingest upload and full-resolution result, split-K slice sums, activation scratch, colour picker) and its first-use buffers.

Every case runs a small - large - small sequence on ONE handle and compares each result, bit for bit, with a FRESH handle that makes only that
call (plus the forward it needs).  The calls are deterministic, so the bar is equality.  The last test creates, uses and closes three handles in
one process, each touching every lazily allocated family (post buffers, bin centres, distribution maps, ingest, picker, the transfer pipeline,
profiling events): the three must return the same.  Results only -- free device memory is not read, other tenants of the card move it.

Shapes: 64 x 64 fp32 handles, max_batch = 2.  The weights are packed once per module (throughput blob: 136 MB instead of 384 MB to checksum and
upload per handle); a handle takes them with set_weights_blob."""
import ctypes

import numpy as np
import pytest

import ingest_ref
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import engine, workloads

pytestmark = pytest.mark.gpu

H = W = 64
NB = 2


@pytest.fixture(scope="module")
def blob(make_sd):
    b = engine.pack_weights(make_sd(0, "he"), precision="fp32", throughput_blob=True)
    b.setflags(write=False)
    return b


@pytest.fixture(scope="module")
def blob_dist(make_sd):
    b = engine.pack_weights(make_sd(0, "he"), precision="fp32", dist=True, throughput_blob=True)
    b.setflags(write=False)
    return b


@pytest.fixture(scope="module")
def batch():
    return workloads.random_batch(NB, H, seed=23, max_points=4, max_p=2)


def _handle(blob=None, **kw):
    e = engine.HipColorizer(H, W, max_batch=NB, precision="fp32", throughput_blob=True, **kw)
    if blob is not None:
        e.set_weights_blob(blob)
    return e


def _small_large_small(steps, prepare, call):
    """steps: the arguments of three calls.  One handle runs them in a row; a fresh handle runs each alone.  prepare(e) readies a handle
    (weights, a forward); call(e, step) returns an array or a tuple of arrays, copied here (results may sit in recycled pinned buffers)."""
    def run(e, step):
        r = call(e, step)
        return tuple(np.array(a) for a in (r if isinstance(r, tuple) else (r,)))

    worn = prepare()
    try:
        got = [run(worn, s) for s in steps]
    finally:
        worn.close()
    for k, s in enumerate(steps):
        fresh = prepare()
        try:
            want = run(fresh, s)
        finally:
            fresh.close()
        assert len(got[k]) == len(want)
        for g, w in zip(got[k], want):
            assert g.shape == w.shape and g.dtype == w.dtype
            np.testing.assert_array_equal(g, w, err_msg="call %d of the sequence differs from a fresh handle's" % k)
    return got


def _rects(n, seed):
    rs = np.random.RandomState(seed)
    y0, x0 = rs.randint(0, H - 8, n), rs.randint(0, W - 8, n)
    dy, dx = rs.randint(0, 8, n), rs.randint(0, 8, n)
    a, b = rs.uniform(-90, 90, n), rs.uniform(-90, 90, n)
    return [(int(y0[i]), int(x0[i]), int(y0[i] + dy[i]), int(x0[i] + dx[i]), float(a[i]), float(b[i])) for i in range(n)]


# ------------------------------------------------------------------------------------------------ hint list: 256 entries, then 2 x n
def test_hint_list_growth_does_not_change_the_planes():
    def call(e, rects):
        e.set_hints(rects, mode="ab")
        return e.hint_planes(0)

    got = _small_large_small([_rects(1, 1), _rects(300, 2), _rects(2, 3)], _handle, call)
    assert all(mask.any() and not mask.all() for _, mask in got)
    assert got[1][1].sum() > got[0][1].sum()                                      # 300 rectangles cover more than one


# ------------------------------------------------------------------------------------------------ display upsample staging
def test_upsample_staging_growth_does_not_change_the_image(blob, batch):
    L, ab, mask = (x[:1] for x in batch)

    def prepare():
        e = _handle(blob)
        e.forward_rgb(L, ab, mask)
        return e

    def call(e, l_out):
        return e.upsample_lab2rgb(l_out, "output_ab", "linear")

    rs = np.random.RandomState(4)
    got = _small_large_small([rs.uniform(0, 100, s) for s in [(16, 16), (90, 75), (16, 16)]], prepare, call)
    assert got[1][0].shape == (90, 75, 3) and len(np.unique(got[1][0])) > 16


# ------------------------------------------------------------------------------------------------ ingest upload, kept sources, full resolution
SOURCES = [(20, 20, 1), (120, 90, 2), (20, 20, 1)]                                 # (h, w, images in the call)


def _sources():
    return [np.stack([ingest_ref.source_image(h, w, 2 * (31 * k + j) + 1) for j in range(n)]) for k, (h, w, n) in enumerate(SOURCES)]


def test_ingest_upload_growth_does_not_change_the_results():
    def call(e, src):
        return e.set_image_rgb(src)

    got = _small_large_small(_sources(), _handle, call)
    assert got[1][0].shape == (2, H, W, 3) and got[1][1].shape == (2, 3, H, W)
    assert all(len(np.unique(rgb)) > 16 for rgb, _ in got)


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_fullres_result_growth_does_not_change_the_image(pinned):
    """keep_source: every slot's source is its own allocation, the result buffer grows with the source; a pageable result goes through the
    handle's pinned staging (grown with it), a pinned one is written in place."""
    def prepare():
        e = _handle()
        e.set_hints(_rects(5, 7), mode="ab")
        return e

    def call(e, src):
        rgb_net, lab_net = e.set_image_rgb(src, keep_source=True)
        shape = src.shape[1:]
        full = e.pinned_empty(shape, np.uint8) if pinned else np.empty(shape, np.uint8)
        e._chk(e.lib.idc_fullres_rgb(e._h, 0, N.IDC_SRC_INPUT_AB, N.IDC_INTERP_LINEAR, N.IDC_L_IMAGE, full.ctypes.data_as(ctypes.c_void_p)))
        return rgb_net, lab_net, full

    got = _small_large_small(_sources(), prepare, call)
    assert got[1][2].shape == (120, 90, 3) and all(len(np.unique(full)) > 16 for _, _, full in got)


# ------------------------------------------------------------------------------------------------ split-K slice sums
def test_splitk_partial_growth_does_not_change_the_forward(blob, batch):
    L, ab, mask = batch

    def call(e, n):
        return e.forward(L[:n], ab[:n], mask[:n])

    engine.set_splitk_policy("always")
    try:
        got = _small_large_small([1, 2, 1], lambda: _handle(blob), call)
    finally:
        engine.set_splitk_policy("auto")
    assert np.isfinite(got[1][0]).all() and np.abs(got[1][0]).max() > 0
    np.testing.assert_array_equal(got[0][0], got[2][0])


# ------------------------------------------------------------------------------------------------ activation scratch
def test_activation_scratch_growth_does_not_change_the_tensor(blob, batch):
    L, ab, mask = (x[:1] for x in batch)

    def prepare():
        e = _handle(blob)
        e.forward(L, ab, mask)
        return e

    got = _small_large_small(["conv8_3", "conv1_2", "conv8_3"], prepare, lambda e, name: e.activation(name, 1))
    assert got[0][0].shape == (1, 256, 16, 16) and got[1][0].shape == (1, 64, 64, 64)
    assert np.abs(got[0][0]).max() > 0 and np.abs(got[1][0]).max() > 0


# ------------------------------------------------------------------------------------------------ colour picker: 65536 bytes, then the call's own
def test_picker_buffer_growth_does_not_change_the_maps():
    rgb = np.array([[250, 10, 10], [10, 250, 10], [128, 128, 128]], np.uint8)

    def call(e, step):
        gamut_size, want_pts = step
        snapped = e.snap_colors([30.0, 50.0, 70.0], rgb, want_lab=True, want_iters=True)
        return tuple(e.gamut_map([50.0], gamut_size, 1, want_pts=want_pts)) + tuple(snapped)

    got = _small_large_small([(5, False), (110, True), (5, False)], _handle, call)
    assert got[0][0].shape == (1, 11, 11, 3) and got[1][0].shape == (1, 221, 221, 3) and got[1][2].shape == (1, 221, 221, 3)
    assert 8 + 221 * 221 * 7 > 65536                                               # the large call's inputs + three results: past the first buffer
    assert got[1][1].any() and not got[1][1].all()


# ------------------------------------------------------------------------------------------------ create, use, close: three times
def test_three_handles_in_a_row_return_the_same(blob_dist, batch):
    L, ab, mask = batch
    axis = np.arange(-110, 120, 10)
    centres = np.array(np.meshgrid(axis, axis)).reshape((2, 529)).T.astype(np.float32)
    src = ingest_ref.source_image(37, 41, 5)

    def use(e):
        r = {}
        r["forward"] = e.forward(L, ab, mask).copy()
        out, rgb, labq = e.forward_rgb(L[:1], ab[:1], mask[:1])                                   # post buffers
        r["rgb"], r["labq"] = rgb.copy(), labq.copy()
        e.forward_dist(L, ab, mask, want_dist=False)
        r["sugg"], r["conf"] = e.suggest_colors(20, 30, centres, K=3, N_draws=2000, seed=1)      # bin centres, suggestion results
        r["entropy"] = e.dist_entropy(NB)                                                         # distribution maps
        r["decode"] = e.dist_decode(centres, NB, mode="mean", gamma=2.0)
        rgb_net, lab_net = e.set_image_rgb(src, keep_source=True)                                 # ingest
        r["rgb_net"], r["lab_net"] = rgb_net.copy(), lab_net.copy()
        r["full"] = e.fullres_rgb("no_ab").copy()
        r["masked"], r["mask"] = e.gamut_map([40.0], 20, 2)                                       # picker
        outs = [np.empty((NB, 2, H, W), np.float32), e.pinned_empty((NB, 2, H, W))]               # pipeline: a staged and an in-place result
        for slot in (0, 1):
            e.forward_async(slot, L, ab, mask, outs[slot])
        for slot in (0, 1):
            e.wait(slot)
            r["async%d" % slot] = outs[slot].copy()
        e.set_profiling(True)                                                                     # profiling events
        r["profiled"] = e.forward(L, ab, mask).copy()
        assert (e.layer_times_ms() >= 0).all()
        e.set_profiling(False)
        return r

    rounds = []
    for _ in range(3):
        e = _handle(blob_dist, dist=True)
        try:
            rounds.append(use(e))
        finally:
            e.close()
    first = rounds[0]
    assert np.isfinite(first["forward"]).all() and np.abs(first["forward"]).max() > 0
    for key in ("async0", "async1", "profiled"):
        np.testing.assert_array_equal(first[key], first["forward"], err_msg=key)
    for k, r in enumerate(rounds[1:], 2):
        assert r.keys() == first.keys()
        for key in first:
            np.testing.assert_array_equal(r[key], first[key], err_msg="handle %d: %s" % (k, key))
