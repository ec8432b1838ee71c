"""The motion compensation of the temporal ab filter without a device: tests/motion_ref.py (the rule of include/ideepcolor.h in numpy float64)
against its own plain loops, the conditions its inputs must meet, the mutants the GPU file's scenario catches, the claim set of the flicker
claim, tools/motion_selftest.cpp plain and under ASan + UBSan, and the ABI and Python plumbing on stub engines.  Nothing here needs a device."""
import os
import re
import subprocess

import numpy as np
import pytest

import motion_ref as M
import temporal_ref as R
import test_temporal_cpu as TC
from interactive_deep_colorization_amd import _native as N

REPO, CSRC = TC.REPO, TC.CSRC


# ------------------------------------------------------------------------------------------------ 1. the restatement itself
@pytest.mark.parametrize("H,W,S,lam", [(8, 8, 3, 0.5), (16, 24, 2, 0.0), (24, 16, 7, 0.3), (8, 40, 5, 1e6)])
def test_the_whole_plane_twin_gives_the_loops_bits(H, W, S, lam):
    rs = np.random.RandomState(H * W + S)
    l, lp = rs.uniform(-50, 50, (H, W)).astype(np.float32), rs.uniform(-50, 50, (H, W)).astype(np.float32)
    v, J, ok = M.vectors_loops(l, lp, S, lam)
    J2, ok2, cands = M.costs(l, lp, S, lam)
    assert np.array_equal(ok, ok2) and ok[0].all()                                   # (0, 0) is always valid
    assert np.array_equal(J[ok].view(np.uint64), J2[ok2].view(np.uint64))            # the same bits
    assert np.array_equal(v, M.choose(J2, ok2, cands)) and np.array_equal(v, M.vectors(l, lp, S, lam))
    assert cands[0] == (0, 0) and len(cands) == (2 * S + 1) ** 2
    if S >= 1:
        assert cands[1:5] == [(-1, 0), (0, -1), (0, 1), (1, 0)]


def test_the_choice_on_ties_nans_and_borders():
    H, W = 16, 24
    flat = np.full((H, W), 3.25, np.float32)
    assert not M.vectors(flat, flat, 7, 0.0).any()                                   # every candidate ties: rank 0
    rs = np.random.RandomState(1)
    lp = rs.uniform(-50, 50, (H, W)).astype(np.float32)
    l = np.roll(lp, (-1, -2), (0, 1))                                                # l[p] = lp[p + (1, 2)]
    v = M.vectors(l, lp, 3, 0.5)
    assert (v[0, :2] == np.array([1, 2], np.int8)).all() and not (v[1, 2] == np.array([1, 2], np.int8)).all()       # invalid at the bottom right
    assert (M.warp(lp, v)[:8, :16] == l[:8, :16]).all()
    bad = l.copy()
    bad[3, 3] = np.nan                                                               # rank 0 of block (0, 0) is a NaN: nothing replaces it
    assert M.vectors(bad, lp, 3, 0.5)[0, 0].tolist() == [0, 0]
    badp = lp.copy()
    badp[4, 5] = np.nan                                                              # l[3, 3]'s true match: that candidate's J is a NaN and never wins
    got = M.vectors(l, badp, 3, 0.5)
    assert got[0, 0].tolist() != [1, 2] and np.array_equal(got[0, 0], M.vectors_loops(l, badp, 3, 0.5)[0][0, 0])
    assert not M.vectors(l, lp, 3, 1e6).any() and not M.vectors(l, lp, 0, 0.0).any()


def test_frame_calls_the_temporal_rule_on_the_warped_state():
    H, W = 16, 24
    ab, l = M.pan(H, W, 2, 3, (1, -2))
    p, mp = dict(R.DEFAULT, cut=0.0), dict(M.DEFAULT)
    y, cut, D, v, ex = M.frame(ab[1], l[1], ab[0], l[0], True, p, mp)
    want = R.frame(ab[1], l[1], M.warp(ab[0], v), M.warp(l[0], v), True, p)
    assert np.array_equal(y, want[0]) and (cut, D) == (want[1], want[2]) and v.any()
    y, cut, D, v, _ = M.frame(ab[1], l[1], ab[0], l[0], False, p, mp)                # no predecessor: y = x, v = 0
    assert np.array_equal(y, ab[1]) and (cut, D) == (1, 0.0) and not v.any()
    y0 = M.frame(ab[1], l[1], ab[0], l[0], True, p, dict(mp, search=0))[0]           # search 0 is the plain rule
    assert np.array_equal(y0, R.frame(ab[1], l[1], ab[0], l[0], True, p)[0])


# ------------------------------------------------------------------------------------------------ 2. the GPU file's inputs and what they catch
@pytest.mark.parametrize("H,W", M.NETS)
def test_the_scenario_passes_on_the_rule(H, W):
    """... and with it the conditions on the inputs that ``verify_call`` asserts on the way: every D clear of cut^2 by CUT_MARGIN, and the
    best candidate MARGIN_REL clear of the second wherever a case names the vector it expects."""
    assert M.play(M.Sim(H, W), H, W) >= 120


def test_the_pans_are_far_from_a_tie():
    worst = np.inf
    for S, step in ((4, (4, -4)), (7, (0, 7)), (1, (-1, 0))):
        ab, l = M.pan(40, 72, 2, 7 + S, step)
        mask = np.array([[M.valid(by, bx, step[0], step[1], 40, 72) for bx in range(9)] for by in range(5)])
        J, ok, _ = M.costs(l[1], l[0], S, 0.5)
        srt = np.sort(np.where(ok, J, np.inf), axis=0)
        worst = min(worst, float((srt[1] - srt[0])[mask].min()))
        assert M.margins(l[1], l[0], S, 0.5)[mask].min() >= M.MARGIN_REL
    print("best to second J on the texture pans: at least %.1f" % worst)
    assert worst >= 14.0          # (the issue's draft: >= 14 absolute)


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_the_scenario_catches_the_mutant(mutant):
    order = [(40, 72), (8, 72), (64, 64), (8, 8)]
    caught = []
    for H, W in order:
        try:
            M.play(M.Sim(H, W, mutant), H, W)
        except AssertionError as ex:
            caught.append(((H, W), str(ex)[:90]))
            if mutant != "swap_hw" and len(caught) == 1:
                break                                    # one net is enough (and keeps this file quick)
    print("%s: caught on %s" % (mutant, caught))
    assert caught
    if mutant == "swap_hw":
        assert [c[0] for c in caught] == [(40, 72), (8, 72)]          # a square net cannot show it


def test_the_claim_set_and_the_closed_form_on_the_rule():
    """The flicker claim of the GPU file on the restatement: the set is at least a quarter of the object, the swing on it is 0.25 of the raw
    one within ``swing_tolerance``, and with motion off at least 0.9 of the raw swing is left."""
    c = M.CLAIM
    s, size, n = c["s"], c["size"], c["n"]
    ab, l, pos, (A_bg, B_bg, A_obj, B_obj) = M.claim_inputs()
    p = dict(R.DEFAULT, strength=s, cut=0.0)
    keep = M.claim_set(l, pos, p, M.DEFAULT)
    print("claim set: %d of %d pixels" % (int(keep.sum()), size * size))
    assert keep.sum() >= size * size // 4
    # the object's blocks choose their vector far from a tie
    for f in (1, n - 1):
        y0, x0 = pos[f]
        inner = np.zeros((c["H"] // 8, c["W"] // 8), bool)
        inner[(y0 + 7) // 8:(y0 + size) // 8, (x0 + 7) // 8:(x0 + size) // 8] = True
        assert inner.sum() >= 9 and M.margins(l[f], l[f - 1], 4, 0.5)[inner].min() >= M.MARGIN_REL
    raw = np.abs(A_obj.astype(np.float64) - B_obj.astype(np.float64))
    ratios = {}
    for motion in (True, False):
        sim = M.Sim(c["H"], c["W"])
        sim.set(**p)
        sim.motion(**(M.DEFAULT if motion else dict(search=0, penalty=0.0)))
        y = sim.apply(ab, l)[0]
        (ya, xa), (yb, xb) = pos[n - 1], pos[n - 2]
        swing = np.abs(y[n - 1][:, ya:ya + size, xa:xa + size].astype(np.float64) - y[n - 2][:, yb:yb + size, xb:xb + size].astype(np.float64))
        ratios[motion] = float(np.median((swing / raw)[:, keep]))
        if motion:
            err = np.abs(swing - (1.0 - s) / (1.0 + s) * raw)
            assert (err <= R.swing_tolerance(A_obj, B_obj, s, n - 1))[:, keep].all()
    print("filtered / raw swing on the claim set: motion on %.6f, off %.6f" % (ratios[True], ratios[False]))
    assert abs(ratios[True] - 0.25) < 0.02 and ratios[False] >= 0.9


# ------------------------------------------------------------------------------------------------ 3. the header, the kernels' brief, the plan
@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan_ubsan"])
def test_ranks_validity_lds_dealing_scratch_and_plan(tmp_path, san):
    run = subprocess.run([TC._make("motion_selftest", str(tmp_path), san)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert re.match(r"motion_selftest: ok \(32768 nets x searches, 8 calls\)", run.stdout.splitlines()[-1]), run.stdout + run.stderr


def test_the_header_is_plain_cpp_and_the_kernels_keep_to_their_brief():
    text = open(os.path.join(CSRC, "idc_motion.h")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", text) == ["stddef.h", "stdint.h", "idc_temporal.h"]
    assert "__global__" not in text and not re.search(r"\bhip[A-Z]\w+\(", text)
    tool = open(os.path.join(REPO, "tools", "motion_selftest.cpp")).read()
    assert [i for i in re.findall(r"#include\s*\"([^\"]+)", tool)] == ["idc_motion.h", "idc_batch.h"]
    kern = open(os.path.join(CSRC, "idc_motion.hip")).read()
    body = kern.split("#include <hip/hip_runtime.h>")[1]
    assert "grid_blocks" not in body and "GridTag" not in body                     # exact grids: no cap, no tag
    assert len(re.findall(r"hipLaunchKernelGGL\(", body)) == 3
    assert re.findall(r"void (\w+_kernel)\(", body) == ["motion_search_kernel", "motion_diff_kernel", "motion_blend_kernel"]
    assert "atomic" not in body and "asm" not in body and "while" not in body      # a fixed order, plain C++ stores, no waiting on another workgroup
    assert body.count("#pragma clang fp contract(off)") >= 4
    ex = open(os.path.join(CSRC, "idc_exec.hip")).read()
    run = ex.split("static int run_temporal(")[1].split("\n}\n")[0]
    assert "if (mp.on)" in run and "launch_temporal_diff" in run and "launch_temporal_blend" in run       # off: the two launches as they were
    assert run.count("hipMemcpyDeviceToDevice") == 2                               # the state: two copies behind the last blend
    header = open(os.path.join(REPO, "include", "ideepcolor.h")).read()
    for phrase in ("RANKED by (dy^2 + dx^2, dy, dx) ascending", "a NaN\n *                     never wins", "l_prev <- l (UNWARPED)",
                   "search 4, penalty 0.5: plausible values.  NOBODY HAS MEASURED THEM ON TRAINED WEIGHTS"):
        assert phrase in header, phrase
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS := .*\bidc_motion\b", mk, re.M) and "idc_motion.h idc_temporal.h ../../include/ideepcolor.h" in mk
    assert "csrc/motion_selftest" in open(os.path.join(REPO, ".gitignore")).read()


# ------------------------------------------------------------------------------------------------ 4. the ABI
def test_abi_symbols_prototypes_and_null_statuses():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ideepcolor.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+idc_set_temporal_motion\s*\(\s*idc_handle\s+h\s*,\s*int\s+on\s*,\s*int\s+search\s*,\s*double\s+penalty\s*\)\s*;", header)
    assert re.search(r"\bint\s+idc_temporal_vectors\s*\(\s*idc_handle\s+h\s*,\s*int\s+slot\s*,\s*int8_t\s*\*\s*v[^)]*\)\s*;", header)
    # the five of the filter keep their prototypes
    assert re.search(r"\bint\s+idc_set_temporal_filter\s*\(\s*idc_handle\s+h\s*,\s*int\s+on\s*,\s*double\s+strength\s*,\s*double\s+sigma\s*,\s*int\s+radius\s*,"
                     r"\s*double\s+cut\s*\)\s*;", header)
    assert re.search(r"\bint\s+idc_temporal_apply\s*\(\s*idc_handle\s+h\s*,\s*int\s+n\s*,\s*const\s+float\s*\*\s*ab[^,]*,\s*const\s+float\s*\*\s*l[^,]*,"
                     r"\s*float\s*\*\s*y[^,]*,\s*int32_t\s*\*\s*cut[^,]*,\s*double\s*\*\s*D[^)]*\)\s*;", header)
    for s in ("idc_set_temporal_motion", "idc_temporal_vectors"):
        assert s in N.EXPORTED_SYMBOLS
    lib = N.load()
    assert lib.idc_set_temporal_motion(None, 1, 4, 0.5) == -1            # a null handle, without a device
    assert lib.idc_temporal_vectors(None, 0, None) == -1


# ------------------------------------------------------------------------------------------------ 5. the Python plumbing
class _Lib(TC._Lib):
    def idc_set_temporal_motion(self, h, on, search, penalty):
        self.calls.append(("motion", on, search, penalty))
        return 0

    def idc_temporal_vectors(self, h, slot, v):
        self.calls.append(("vectors", slot))
        return 0


class _Stub(TC._Stub):
    def __init__(self, fail_after=None):
        TC._Stub.__init__(self, fail_after)
        self.lib = _Lib()

    def _enqueue(self, kind, images, hints):
        TC._Stub._enqueue(self, kind, images, hints)
        self.seen[-1] = self.seen[-1] + (self.__dict__.get("_motion"),)


def _motion_calls(e):
    return [c for c in e.lib.calls if c[0] == "motion"]


def test_set_temporal_motion_reaches_the_library():
    e = _Stub()
    e.set_temporal_motion()
    e.set_temporal_motion(7, penalty=0.0)
    e.set_temporal_motion(None)
    e.set_temporal_motion(None)
    assert e.lib.calls == [("motion", 1, 4, 0.5), ("motion", 1, 7, 0.0), ("motion", 0, 7, 0.0), ("motion", 0, 4, 0.5)]
    assert e.__dict__["_motion"] is None and e._temporal is None              # the filter's own record is untouched
    e.set_temporal_filter()
    assert e._temporal == dict(R.DEFAULT)                                     # ... and stays the four-key dict
    v = e.temporal_vectors(1, 2)
    assert v.shape == (2, 1, 1, 2) and v.dtype == np.int8 and e.lib.calls[-1] == ("vectors", 1)
    with pytest.raises(ValueError):
        e.temporal_vectors(-1)                                                # no temporal_apply yet, and no count given


@pytest.mark.parametrize("name", TC.GENERATORS)
def test_the_motion_key_sets_and_restores_with_the_filter(name):
    on = dict(M.DEFAULT)
    # no motion asked for: no motion call reaches the library, whatever the temporal keyword
    for temporal in (None, True, False, dict(R.DEFAULT), dict(strength=0.3, sigma=2.0, radius=0, cut=0.0, motion=False)):
        e = _Stub()
        list(TC._generator(e, name, temporal=temporal))
        assert _motion_calls(e) == [] and len(e.seen) == 3, temporal
    # motion=True: set behind the filter and before the reset and the first batch, every batch sees it, off again behind the last wait
    e = _Stub()
    list(TC._generator(e, name, temporal=dict(motion=True)))
    calls = e.lib.calls
    assert calls[:3] == [("set", 1, 0.6, 4.0, 1, 12.0), ("motion", 1, 4, 0.5), ("reset",)] and calls[3][0] == "enqueue"
    assert calls[-2:] == [("motion", 0, 4, 0.5), ("set", 0, 0.6, 4.0, 1, 12.0)] and calls[-3][0] == "wait"
    assert [s[1] for s in e.seen] == [dict(R.DEFAULT)] * 3 and [s[4] for s in e.seen] == [on] * 3
    assert e._temporal is None and e.__dict__.get("_motion") is None
    # a dict of parameters beside the filter's; the previous settings are what comes back
    e = _Stub()
    e.set_temporal_filter(0.2)
    e.set_temporal_motion(2, 3.0)
    mine = dict(strength=0.5, sigma=2.0, radius=2, cut=0.0)
    list(TC._generator(e, name, temporal=dict(mine, motion=dict(search=7, penalty=0.0))))
    assert [s[1] for s in e.seen] == [mine] * 3 and [s[4] for s in e.seen] == [dict(search=7, penalty=0.0)] * 3
    assert e._temporal == dict(R.DEFAULT, strength=0.2) and e.__dict__["_motion"] == dict(search=2, penalty=3.0)
    assert _motion_calls(e)[-1] == ("motion", 1, 2, 3.0)
    # motion=False switches a motion that is on off for the stream; without the key it stands as it is
    e.seen, e.lib.calls = [], []
    list(TC._generator(e, name, temporal=dict(mine, motion=False)))
    assert [s[4] for s in e.seen] == [None] * 3 and e.__dict__["_motion"] == dict(search=2, penalty=3.0)
    assert _motion_calls(e) == [("motion", 0, 2, 3.0), ("motion", 1, 2, 3.0)]
    e.seen, e.lib.calls = [], []
    list(TC._generator(e, name, temporal=True))
    assert [s[4] for s in e.seen] == [dict(search=2, penalty=3.0)] * 3 and _motion_calls(e) == []
    # abandoned after the first result, and an exception on the way: restored as well
    e = _Stub()
    g = TC._generator(e, name, temporal=dict(motion=True))
    next(g)
    assert e.__dict__["_motion"] == on
    g.close()
    assert e.__dict__["_motion"] is None and e._temporal is None and e.lib.calls[-1][0] == "set" and e.lib.calls[-2][0] == "motion"
    e = _Stub(fail_after=1)
    with pytest.raises(RuntimeError):
        list(TC._generator(e, name, temporal=dict(motion=True)))
    assert e.__dict__["_motion"] is None and e._temporal is None
    # parameters the engine refuses are refused before anything is enqueued, and the filter comes back
    e = _Stub()
    with pytest.raises(TypeError):
        next(TC._generator(e, name, temporal=dict(motion=dict(radius=2))))
    assert e.seen == [] and e._temporal is None and e.__dict__.get("_motion") is None
    with pytest.raises(TypeError):
        next(TC._generator(e, name, temporal=dict(gain=1.0)))
    assert e.seen == [] and e._temporal is None


def test_colorize_video_yields_the_vectors():
    e = _Stub()
    e.temporal_info = lambda slot, n=None: (np.array([1, 0][:n], np.int32), np.zeros(n))
    asked = []

    def vectors(slot, n=None):
        asked.append((slot, n))
        return np.full((n, 1, 1, 2), slot + 1, np.int8)
    e.temporal_vectors = vectors
    frames = TC._video_frames(["rgb"] * 3)
    results = list(e.colorize_video(iter(frames), temporal=dict(motion=True), vectors=True))
    assert [len(r) for r in results] == [3, 3, 3] and [r[1] for r in results] == [True, False, True]
    assert [r[2].tolist() for r in results] == [[[[1, 1]]], [[[1, 1]]], [[[2, 2]]]] and asked == [(0, 2), (1, 1)]
    assert _motion_calls(e) == [("motion", 1, 4, 0.5), ("motion", 0, 4, 0.5)]
    # the filter on without motion, and the filter off: zeros, and nothing is asked of the library
    for temporal in (True, False):
        e = _Stub()
        e.temporal_info = lambda slot, n=None: (np.zeros(n, np.int32), np.zeros(n))
        e.temporal_vectors = None
        results = list(e.colorize_video(iter(TC._video_frames(["g8"] * 3)), temporal=temporal, vectors=True))
        assert all(r[2].shape == (1, 1, 2) and not r[2].any() for r in results) and _motion_calls(e) == []
    # the default: pairs, as before
    e = _Stub()
    e.temporal_info = lambda slot, n=None: (np.zeros(n, np.int32), np.zeros(n))
    assert [len(r) for r in e.colorize_video(iter(TC._video_frames(["rgb"] * 2)))] == [2, 2]
