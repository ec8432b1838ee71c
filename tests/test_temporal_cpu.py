"""The temporal ab filter without a device: tests/temporal_ref.py (the rule of include/ideepcolor.h in numpy float64) against plain loops and
against the rule's closed forms, the perturbation bound behind the GPU file's bar, the mutants the GPU file's inputs catch,
tools/temporal_selftest.cpp plain and under ASan + UBSan, and the ABI and Python plumbing on a stub engine.  Nothing here needs a device."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import temporal_ref as R
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "interactive_deep_colorization_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


# ------------------------------------------------------------------------------------------------ 1. the restatement itself
@pytest.mark.parametrize("H,W", [(8, 8), (5, 11), (16, 24)])
def test_the_whole_plane_window_is_the_plain_loops(H, W):
    rs = np.random.RandomState(H * W)
    e = rs.uniform(0, 900, (H, W))
    for radius in range(4):
        assert np.array_equal(R.window_mean(e, radius), R.window_mean_loops(e, radius)), radius
    # a clipped window, not a replicated one, and the mean, not the sum
    assert not np.array_equal(R.window_mean(e, 1, "replicate"), R.window_mean(e, 1))
    assert np.array_equal(R.window_mean(e, 1, "replicate")[1:-1, 1:-1], R.window_mean(e, 1)[1:-1, 1:-1])
    assert R.window_mean(np.full((H, W), 7.0), 3).tolist() == np.full((H, W), 7.0).tolist()


# ------------------------------------------------------------------------------------------------ 2. closed forms
def test_closed_forms():
    H, W = 8, 16
    ab, l = R.frames(H, W, 3, 5)
    state = (ab[0], l[0], True)
    # s = 0 gives x
    y, cut, D, _ = R.frame(ab[1], l[1], *state, dict(R.DEFAULT, strength=0.0))
    assert np.array_equal(y, ab[1]) and cut == 0 and D > 0
    # identical L planes give g = s exactly
    y, cut, D, g = R.frame(ab[1], l[0], *state, R.DEFAULT)
    assert (g == 0.6).all() and D == 0.0 and cut == 0
    # no previous frame: y = x, cut = 1, D = 0
    y, cut, D, g = R.frame(ab[1], l[1], ab[0], l[0], False, R.DEFAULT)
    assert np.array_equal(y, ab[1]) and (cut, D, g) == (1, 0.0, None)
    # a cut passes the frame, whatever the window says
    y, cut, D, _ = R.frame(ab[1], l[0] + np.float32(13.0), *state, R.DEFAULT)
    assert np.array_equal(y, ab[1]) and cut == 1 and abs(D - 169.0) < 1e-4      # (l + 13 is rounded to float32)
    y, cut, D, _ = R.frame(ab[1], l[0] + np.float32(13.0), *state, dict(R.DEFAULT, cut=0.0))
    assert cut == 0 and not np.array_equal(y, ab[1])


@pytest.mark.parametrize("s", [0.6, 0.3, 0.95])
def test_steady_state_swing(s):
    """Identical L, x alternating between A and B: the swing of y settles at (1 - s) / (1 + s) of the raw one -- 0.25 at s = 0.6 -- to the
    float32 rounding of the recursion (``swing_tolerance``, the bound the GPU file's flicker case uses)."""
    H, W, frames = 8, 8, 40 if s < 0.9 else 400
    rs = np.random.RandomState(3)
    A, B = rs.uniform(-80, 80, (2, H, W)).astype(np.float32), rs.uniform(-80, 80, (2, H, W)).astype(np.float32)
    sim = R.Sim(H, W)
    sim.set(**dict(R.DEFAULT, strength=s))
    l = np.zeros((1, H, W), np.float32)
    ys = [sim.apply((A if k % 2 == 0 else B)[None], l)[0][0] for k in range(frames)]
    swing = np.abs(ys[-1].astype(np.float64) - ys[-2].astype(np.float64))
    want = (1.0 - s) / (1.0 + s) * np.abs(A.astype(np.float64) - B.astype(np.float64))
    err = np.abs(swing - want)
    tol = R.swing_tolerance(A, B, s, frames - 1)
    print("s %.2f: ratio %.9f, worst error / tolerance %.3g" % (s, float((swing / np.abs(A.astype(np.float64) - B)).mean()), float((err / tol).max())))
    assert (err <= tol).all()
    if s == 0.6:
        assert abs(float((swing / np.abs(A.astype(np.float64) - B)).mean()) - 0.25) < 1e-6


# ------------------------------------------------------------------------------------------------ 3. the GPU file's bar and inputs
def test_one_ulp_of_exp_stays_inside_the_bar():
    """exp on the device and numpy's may differ in the last place.  Shifting EVERY exp by one ulp either way, on the GPU file's inputs, leaves
    each output within one float32 ulp and differing on fewer values than the bar allows: the bar is not tighter than the arithmetic."""
    H, W = 40, 72
    ab, l = R.frames(H, W, 12, 1000 * H + W + 3, cuts=(5,))
    worst = 1.0
    for f in range(1, 12):
        base = R.frame(ab[f], l[f], ab[f - 1], l[f - 1], True, R.DEFAULT)[0]
        for shift in (-1, 1):
            moved = R.frame(ab[f], l[f], ab[f - 1], l[f - 1], True, R.DEFAULT, exp_shift=shift)[0]
            within, share = R.ulp_check(moved, base)
            worst = min(worst, share)
            assert within and share >= R.BIT_EQUAL_SHARE, (f, shift, share)
    print("bit-equal share under a one-ulp shift of every exp: %.6f at worst" % worst)


@pytest.mark.parametrize("H,W", R.NETS)
def test_the_scenario_passes_on_the_rule(H, W):
    assert R.play(R.Sim(H, W), H, W) >= 40


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_scenario_catches_the_mutant(mutant):
    caught = []
    for H, W in R.NETS:
        try:
            R.play(R.Sim(H, W, mutant), H, W)
        except AssertionError as ex:
            caught.append(((H, W), str(ex)[:90]))
    print("%s: caught on %s" % (mutant, caught))
    assert caught
    if mutant == "swap_hw":
        assert [c[0] for c in caught] == [(40, 72)]          # a square net cannot show it
    else:
        assert len(caught) == len(R.NETS)


def _run_split(sim, ab, l, parts):
    sim.reset()
    out, at = [], 0
    for n in parts:
        out.append(sim.apply(ab[at:at + n], l[at:at + n])[0])
        at += n
    return np.concatenate(out), sim.state()


def test_a_float64_state_shows_in_the_split_sequence():
    """The state is the stored floats: 7 frames give the same bits as one call, as 3 + 4 and as seven calls of one.  A kernel that carried y in
    float64 from frame to frame inside a call would not."""
    H, W = 40, 72
    ab, l = R.frames(H, W, 7, 77)
    for mutant, same in ((None, True), ("f64_state", False)):
        whole, st = _run_split(R.Sim(H, W, mutant), ab, l, [7])
        for parts in ([3, 4], [1] * 7):
            got, st2 = _run_split(R.Sim(H, W, mutant), ab, l, parts)
            equal = np.array_equal(got.view(np.uint32), whole.view(np.uint32)) and np.array_equal(st[0].view(np.uint32), st2[0].view(np.uint32))
            assert equal == same, (mutant, parts)


# ------------------------------------------------------------------------------------------------ 4. the header, the kernels' brief, the plan
def _make(target, out, san):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc (%s): tools/%s.cpp cannot be compiled" % (HIPCC, target))
    cmd = ["make", "-C", CSRC, target, "BINDIR=" + out, "HIPCC=" + HIPCC] + (["SAN=1"] if san else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return os.path.join(out, target)


@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan_ubsan"])
def test_tiles_partials_scratch_and_plan(tmp_path, san):
    run = subprocess.run([_make("temporal_selftest", str(tmp_path), san)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert re.match(r"temporal_selftest: ok \(16384 nets x radii, 8 calls\)", run.stdout.splitlines()[-1]), run.stdout + run.stderr


def test_the_header_is_plain_cpp_and_the_kernels_keep_to_their_brief():
    text = open(os.path.join(CSRC, "idc_temporal.h")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", text) == ["stddef.h"] and "__global__" not in text and not re.search(r"\bhip[A-Z]\w+\(", text)
    tool = open(os.path.join(REPO, "tools", "temporal_selftest.cpp")).read()
    assert [i for i in re.findall(r"#include\s*\"([^\"]+)", tool)] == ["idc_temporal.h", "idc_batch.h"]
    kern = open(os.path.join(CSRC, "idc_temporal.hip")).read()
    body = kern.split("#include <hip/hip_runtime.h>")[1]
    assert "grid_blocks" not in body and "GridTag" not in body                     # exact grids: no cap, no tag
    assert len(re.findall(r"hipLaunchKernelGGL\(", body)) == 2 and len(re.findall(r"__global__", body)) == 2
    assert "atomic" not in body and "asm" not in body                              # a fixed summation order, plain C++ stores
    assert body.count("#pragma clang fp contract(off)") >= 3
    header = open(os.path.join(REPO, "include", "ideepcolor.h")).read()
    for phrase in ("g = s * exp(-m / (2 sigma^2))", "y_prev <- y", "NOBODY HAS MEASURED THEM ON TRAINED WEIGHTS"):
        assert phrase in header
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS := .*\bidc_temporal\b", mk, re.M) and "idc_temporal.h ../../include/ideepcolor.h" in mk


# ------------------------------------------------------------------------------------------------ 5. the ABI
def test_abi_symbols_prototypes_and_null_statuses():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ideepcolor.h")).read(), flags=re.S)      # (the shapes stand in comments)
    assert re.search(r"\bint\s+idc_set_temporal_filter\s*\(\s*idc_handle\s+h\s*,\s*int\s+on\s*,\s*double\s+strength\s*,\s*double\s+sigma\s*,\s*int\s+radius\s*,"
                     r"\s*double\s+cut\s*\)\s*;", header)
    assert re.search(r"\bint\s+idc_temporal_reset\s*\(\s*idc_handle\s+h\s*\)\s*;", header)
    assert re.search(r"\bint\s+idc_temporal_info\s*\(\s*idc_handle\s+h\s*,\s*int\s+slot\s*,\s*int32_t\s*\*\s*cut[^,]*,\s*double\s*\*\s*D[^)]*\)\s*;", header)
    assert re.search(r"\bint\s+idc_temporal_apply\s*\(\s*idc_handle\s+h\s*,\s*int\s+n\s*,\s*const\s+float\s*\*\s*ab[^,]*,\s*const\s+float\s*\*\s*l[^,]*,"
                     r"\s*float\s*\*\s*y[^,]*,\s*int32_t\s*\*\s*cut[^,]*,\s*double\s*\*\s*D[^)]*\)\s*;", header)
    assert re.search(r"\bint\s+idc_temporal_state\s*\(\s*idc_handle\s+h\s*,\s*float\s*\*\s*y_prev[^,]*,\s*float\s*\*\s*l_prev[^,]*,\s*int32_t\s*\*\s*have\s*\)\s*;",
                     header)
    names = ("idc_set_temporal_filter", "idc_temporal_reset", "idc_temporal_info", "idc_temporal_apply", "idc_temporal_state")
    for s in names:
        assert s in N.EXPORTED_SYMBOLS
    lib = N.load()
    assert lib.idc_set_temporal_filter(None, 1, 0.6, 4.0, 1, 12.0) == -1            # a null handle, without a device
    assert lib.idc_temporal_reset(None) == -1
    assert lib.idc_temporal_info(None, 0, None, None) == -1
    assert lib.idc_temporal_apply(None, 1, None, None, None, None, None) == -1
    assert lib.idc_temporal_state(None, None, None, None) == -1


# ------------------------------------------------------------------------------------------------ 6. the Python plumbing
class _Lib(object):
    def __init__(self):
        self.calls = []

    def idc_set_temporal_filter(self, h, on, s, sigma, radius, cut):
        self.calls.append(("set", on, s, sigma, radius, cut))
        return 0

    def idc_temporal_reset(self, h):
        self.calls.append(("reset",))
        return 0

    def idc_temporal_info(self, h, slot, cut, D):
        self.calls.append(("info", slot))
        return 0

    def idc_set_batch_output(self, h, f, m):
        return 0

    def idc_set_ingest_filter(self, h, f):
        return 0


class _Pool(object):
    def take(self, shape, dtype):
        return np.zeros(shape, dtype)


class _Stub(engine.HipColorizer):
    """The streaming generators over an engine that launches nothing: every enqueue records the temporal setting in force and what it was given."""

    def __init__(self, fail_after=None):
        self.H, self.W, self.max_batch = 8, 8, 2
        self._batch_upsample, self._ingest_filter = "linear", "bilinear"
        self._pool, self.lib, self._h = _Pool(), _Lib(), None
        self._in_flight = {}
        self.seen, self.fail_after = [], fail_after

    def __del__(self):
        pass

    def _chk(self, rc):
        assert rc == 0

    def set_batch_upsample(self, interp="linear"):
        self._batch_upsample = interp

    def _pinned_slices(self, shapes):
        return [np.zeros(s, np.uint8) for s in shapes]

    def wait(self, slot):
        self.lib.calls.append(("wait", slot))

    def _enqueue(self, kind, images, hints):
        if self.fail_after is not None and len(self.seen) >= self.fail_after:
            raise RuntimeError("enqueue refused")
        self.seen.append((kind, None if self._temporal is None else dict(self._temporal), [int(np.asarray(a).flat[0]) for a in images], list(hints)))
        self.lib.calls.append(("enqueue", kind))

    def _outs(self, images):
        return [np.full(a.shape[:2] + (3,), np.asarray(a).flat[0], np.uint8) for a in images]

    def forward_async_rgb(self, slot, rgb, hints, out_rgb, **kw):
        self._enqueue("rgb", rgb, hints or [])

    def forward_async_images(self, slot, images, hints, **kw):
        self._enqueue("images", images, hints)
        return self._outs(images)

    def forward_async_layers(self, slot, images, layers, hints, **kw):
        self._enqueue("layers", images, hints)
        return self._outs(images), np.zeros(len(images), np.int32)

    def forward_async_gray(self, slot, images, hints, **kw):
        self._enqueue("gray", images, hints)
        return self._outs(images)

    def forward_async_eval(self, slot, images, hints, **kw):
        self._enqueue("eval", images, hints)
        return np.zeros((len(images), 3), np.uint64), None, None


GENERATORS = ["colorize_stream", "colorize_images", "colorize_gray", "colorize_layers", "evaluate_images"]


def _generator(e, name, **kw):
    img, g = np.zeros((5, 7, 3), np.uint8), np.zeros((5, 7), np.uint8)
    items = [img] * 5                                            # three batches of at most two
    return {
        "colorize_stream": lambda: e.colorize_stream([(np.stack([img, img]), None)] * 3, out="source", **kw),
        "colorize_images": lambda: e.colorize_images(items, **kw),
        "colorize_gray": lambda: e.colorize_gray([g] * 5, **kw),
        "colorize_layers": lambda: e.colorize_layers([(img, None, None)] * 5, **kw),
        "evaluate_images": lambda: e.evaluate_images(items, out="source", **kw),
    }[name]()


def test_set_temporal_filter_reaches_the_library():
    e = _Stub()
    e.set_temporal_filter()
    e.set_temporal_filter(0.3, sigma=2.0, radius=3, cut=0.0)
    e.set_temporal_filter(None)
    e.temporal_reset()
    assert e.lib.calls == [("set", 1, 0.6, 4.0, 1, 12.0), ("set", 1, 0.3, 2.0, 3, 0.0), ("set", 0, 0.3, 2.0, 3, 0.0), ("reset",)]
    assert e._temporal is None


@pytest.mark.parametrize("name", GENERATORS)
def test_the_temporal_keyword_sets_resets_and_restores(name):
    on = dict(R.DEFAULT)
    # run to the end: set and reset before the first batch, every batch sees it, off again behind the last wait
    e = _Stub()
    results = list(_generator(e, name, temporal=True))
    assert len(results) in (3, 5) and [s[1] for s in e.seen] == [on] * 3 and e._temporal is None
    calls = e.lib.calls
    assert calls[0] == ("set", 1, 0.6, 4.0, 1, 12.0) and calls[1] == ("reset",) and calls[2][0] == "enqueue"
    assert calls[-1] == ("set", 0, 0.6, 4.0, 1, 12.0) and calls[-2][0] == "wait"
    assert sum(1 for c in calls if c[0] == "reset") == 1
    # a dict of parameters; the previous setting is what comes back
    e = _Stub()
    e.set_temporal_filter(0.2)
    mine = dict(strength=0.5, sigma=2.0, radius=2, cut=0.0)
    list(_generator(e, name, temporal=mine))
    assert [s[1] for s in e.seen] == [mine] * 3 and e._temporal == dict(R.DEFAULT, strength=0.2)
    # False switches a filter that is on off for the stream; None touches nothing, not even the sequence
    e.seen, e.lib.calls = [], []
    list(_generator(e, name, temporal=False))
    assert [s[1] for s in e.seen] == [None] * 3 and e._temporal == dict(R.DEFAULT, strength=0.2)
    e.seen, e.lib.calls = [], []
    list(_generator(e, name))
    assert [s[1] for s in e.seen] == [dict(R.DEFAULT, strength=0.2)] * 3 and not [c for c in e.lib.calls if c[0] in ("set", "reset")]
    # abandoned after the first result: both slots waited for, then restored
    e = _Stub()
    g = _generator(e, name, temporal=True)
    assert e.lib.calls == []                                # nothing happens before the first next()
    next(g)
    assert e._temporal == on
    g.close()
    assert e._temporal is None and e.lib.calls[-1][0] == "set" and e.lib.calls[-2][0] == "wait"
    # an exception on the way: restored as well
    e = _Stub(fail_after=1)
    with pytest.raises(RuntimeError):
        list(_generator(e, name, temporal=True, upsample="joint"))
    assert e._temporal is None and e._batch_upsample == "linear"
    # parameters the engine refuses are refused before anything is enqueued
    e = _Stub()
    with pytest.raises(TypeError):
        next(_generator(e, name, temporal=dict(gain=1.0)))
    assert e.seen == [] and e._temporal is None


def _video_frames(kinds):
    out = []
    for k, kind in enumerate(kinds):
        shape = {"rgb": (5, 7, 3), "g8": (5, 7), "g16": (5, 7)}[kind]
        out.append(np.full(shape, k + 1, np.uint16 if kind == "g16" else np.uint8))
    return out


def test_colorize_video_orders_frames_and_holds_key_frame_hints():
    e = _Stub()
    e.temporal_info = lambda slot, n=None: (np.array([1, 0][:n], np.int32), np.zeros(n))
    a, b = [(0, 0, 1, 1, 10.0, 20.0)], [(2, 2, 3, 3, -5.0, 5.0)]
    frames = _video_frames(["rgb"] * 5 + ["g8"] * 2 + ["g16"])
    results = list(e.colorize_video(iter(frames), hints={1: a, 4: b}))
    # every frame once, in order (the stub paints each result with its frame's first sample), with the cut flag of its place in its call
    assert [int(r[0].flat[0]) for r in results] == [1, 2, 3, 4, 5, 6, 7, 8]
    assert [r[1] for r in results] == [True, False, True, False, True, True, False, True]
    # the batches: two frames at most, closed by a change of kind or dtype; a key frame's hints hold until the next key
    assert [(s[0], s[2]) for s in e.seen] == [("images", [1, 2]), ("images", [3, 4]), ("images", [5]), ("gray", [6, 7]), ("gray", [8])]
    assert [s[3] for s in e.seen] == [[None, a], [a, a], [b], [b, b], [b]]
    assert all(s[1] == R.DEFAULT for s in e.seen) and e._temporal is None
    assert [c for c in e.lib.calls if c[0] in ("set", "reset")] == [("set", 1, 0.6, 4.0, 1, 12.0), ("reset",), ("set", 0, 0.6, 4.0, 1, 12.0)]
    # one list for every frame; no hints; the filter off: no flag is asked for, every cut is False
    e = _Stub()
    e.temporal_info = None
    results = list(e.colorize_video(_video_frames(["g8"] * 3), hints=a, temporal=False))
    assert [s[3] for s in e.seen] == [[a, a], [a]] and [r[1] for r in results] == [False] * 3
    e = _Stub()
    list(e.colorize_video(_video_frames(["rgb"] * 2), temporal=None))
    assert [s[3] for s in e.seen] == [[None, None]] and not [c for c in e.lib.calls if c[0] in ("set", "reset")]
    with pytest.raises(ValueError):
        next(e.colorize_video(_video_frames(["rgb"]), hints="red"))
    with pytest.raises(ValueError):
        next(e.colorize_video(_video_frames(["rgb"]), depth=16, out="net"))
    with pytest.raises(ValueError):
        list(e.colorize_video(_video_frames(["g8"]), depth=16))


def test_temporal_apply_checks_its_shapes():
    e = _Stub()
    with pytest.raises(ValueError):
        e.temporal_apply(np.zeros((2, 2, 8, 9), np.float32), np.zeros((2, 8, 9), np.float32))
    with pytest.raises(ValueError):
        e.temporal_apply(np.zeros((2, 2, 8, 8), np.float32), np.zeros((3, 8, 8), np.float32))
