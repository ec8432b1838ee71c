"""The hint tracking along the motion vectors without a device: tests/track_ref.py (the recursion of include/ideepcolor.h's rule in plain loops)
against its whole-plane twin and against the walk the kernel uses, the conditions the GPU file's inputs must meet, the mutants they tell
apart, the claim's pixel counts, tools/track_selftest.cpp plain and under ASan + UBSan, and the ABI and Python plumbing on stub engines.
Nothing here needs a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import motion_ref as M
import temporal_ref as R
import test_temporal_cpu as TC
import track_ref as T
from interactive_deep_colorization_amd import _native as N

REPO, CSRC = TC.REPO, TC.CSRC


def _same3(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
               for x, y in zip(a[:3], b[:3]))


# ------------------------------------------------------------------------------------------------ 1. the restatement itself
@pytest.mark.parametrize("H,W,life,tol", [(8, 8, 0, 8.0), (16, 24, 2, 8.0), (24, 16, 0, 0.0), (8, 40, 1, 100.0)])
def test_the_walk_equals_the_recursion_on_random_planes(H, W, life, tol):
    """Random quarter-step L planes (so that |dl| often IS tol), random valid vectors that differ block by block, hints sprinkled over every
    frame, one call from a fresh sequence and the same frames as 2 + 1 + 3 from the state: the loops, their twin and the walk give the same bits."""
    rs = np.random.RandomState(H * W + life)
    n = 6
    l = np.cumsum(rs.choice([0.0, 0.25, 0.5, 8.0, -8.25, 20.0], (n, H, W), p=[0.3, 0.2, 0.2, 0.1, 0.1, 0.1]), 0) + rs.randint(-200, 200, (H, W)) * 0.25
    l = l.astype(np.float32)
    l[3, H // 2, W // 2] = np.nan
    v = np.zeros((n, H // 8, W // 8, 2), np.int8)
    for f in range(n):
        for by in range(H // 8):
            for bx in range(W // 8):
                dy, dx = rs.randint(-3, 4, 2)
                v[f, by, bx] = (dy if M.valid(by, bx, dy, 0, H, W) else 0, dx if M.valid(by, bx, 0, dx, H, W) else 0)
    mask = np.where(rs.uniform(size=(n, H, W)) < np.array([0.3] + [0.05] * (n - 1))[:, None, None], rs.choice([1.0, 0.5], (n, H, W)), 0.0).astype(np.float32)
    ab = (rs.uniform(-80, 80, (n, 2, H, W)) * (mask[:, None] != 0)).astype(np.float32)
    whole = T.sequence(l, ab, mask, v, None, life, tol, rule=T.frame_loops)
    assert _same3(whole, T.sequence(l, ab, mask, v, None, life, tol, rule=T.frame)) and _same3(whole, T.walk(ab, mask, l, v, None, life, tol))
    assert (whole[2] > 1).any() or life == 1
    state, parts = None, []
    for a, b in ((0, 2), (2, 3), (3, 6)):
        got = T.walk(ab[a:b], mask[a:b], l[a:b], v[a:b], state, life, tol)
        assert _same3(got, T.sequence(l[a:b], ab[a:b], mask[a:b], v[a:b], state, life, tol, rule=T.frame_loops))
        state = T.Prev(got[0][-1], got[1][-1], got[2][-1], l[b - 1])
        parts.append(got)
    assert _same3([np.concatenate([p[k] for p in parts]) for k in range(3)], whole)
    # a predecessor whose tracked planes were dropped: vectors, and nothing carried into frame 0
    got = T.walk(ab[3:], mask[3:], l[3:], v[3:], T._NoTrack(l[2]), life, tol)
    assert _same3(got, T.sequence(l[3:], ab[3:], mask[3:], v[3:], T._NoTrack(l[2]), life, tol, rule=T.frame_loops))
    assert np.array_equal(got[1][0], mask[3])


# ------------------------------------------------------------------------------------------------ 2. the GPU file's inputs
def _inputs(H, W):
    out = [(c["name"], c) for c in T.cases(H, W)]
    if (H, W) == (64, 64):
        l, ab, mask, _ = T.claim_inputs()
        out.append(("the claim", dict(name="the claim", l=l, ab=ab, mask=mask, mp=dict(M.DEFAULT), tp=dict(T.DEFAULT))))
    return out


def _rule(c, mutant=None):
    sim = T.Sim(mutant)
    sim.motion(**c["mp"])
    sim.set(**c["tp"])
    return sim.apply(c["l"], c["ab"], c["mask"])


@pytest.mark.parametrize("H,W", T.NETS)
def test_the_inputs_meet_their_conditions_and_the_twin_gives_the_loops_bits(H, W):
    """Every |dl| the rule compares is exactly tol (only where the case says so) or TOL_MARGIN_REL away from it; the vectors a closed form names
    are MARGIN_REL clear of the second-best J; the twin that carries the mutants is the loops bit for bit; the closed forms hold on the rule."""
    worst, closed = np.inf, 0
    for name, c in _inputs(H, W):
        A, Mk, G, v = _rule(c)
        want = T.sequence(c["l"], c["ab"], c["mask"], v, None, c["tp"]["life"], c["tp"]["tol"], rule=T.frame_loops)
        assert _same3((A, Mk, G), want), name
        margin, ties = T.tol_margin(c["l"], None, v, c["tp"]["tol"])
        assert margin >= T.TOL_MARGIN_REL and (ties > 0) == bool(c.get("ties")), (name, margin, ties)
        worst = min(worst, margin)
        if name != "the claim":
            closed += T.check_case(c, A, Mk, G, v)
        named = c["pan"][0] if "pan" in c else (-1, -2) if "object" in c else None
        if named is not None:
            for f in range(1, c["l"].shape[0]):
                right = (v[f] == np.array(named, np.int8)).all(-1)
                if right.any():
                    assert M.margins(c["l"][f], c["l"][f - 1], int(c["mp"]["search"]), float(c["mp"]["penalty"]))[right].min() >= M.MARGIN_REL, (name, f)
    print("%dx%d: every |dl| at least %.3g (relative) from tol; closed forms on %d frames" % (H, W, worst, closed))
    assert closed >= (100 if H >= 40 else 10)


def test_the_pipelined_inputs_meet_their_conditions():
    """Grey sources of eight levels: along the vectors L repeats exactly, and two different levels are more than tol + 1 apart, far more than
    the last bits in which the device's L plane may differ from this host's."""
    srcs = T.grey_pan_sources(7)
    l = T.grey_l(srcs)
    levels = np.unique(l)
    assert len(levels) == 8 and np.diff(levels).min() > 9.0
    v = T.call_vectors(l, None, M.DEFAULT)
    assert (v[1:, 1:-1, 1:-1] == np.array([1, 2], np.int8)).all()
    for f in range(1, 7):
        assert M.margins(l[f], l[f - 1], 4, 0.5)[1:-1, 1:-1].min() >= 0.5
    margin, ties = T.tol_margin(l, None, v, 8.0)
    assert margin > 0.12 and ties == 0
    l7, ab, mask = T.pipeline_inputs()
    whole = T.play_parts(T.Sim(), l7, ab, mask, [7])
    assert whole[2][6].max() == 6 and (whole[2][6] == 3).any()
    for parts in ([3, 4], [1] * 7, [2, 2, 3]):
        assert _same3(T.play_parts(T.Sim(), l7, ab, mask, parts), whole), parts


# ------------------------------------------------------------------------------------------------ 3. the mutants
def _table(H, W):
    table = {}
    for name, c in _inputs(H, W):
        want = _rule(c)
        table[name] = [m for m in T.MUTANTS if m not in ("state_not_carried", "state_early") and not _same3(_rule(c, m), want)]
    return table


def test_every_mutant_is_caught_and_every_input_tells_one_apart():
    tables = {net: _table(*net) for net in T.NETS}
    for net, table in tables.items():
        for name, caught in table.items():
            # a single frame has no predecessor: no mutant of the carry can show on it -- it is there for the path without one
            assert caught or name == "n = 1", "%s: %s tells no mutant apart" % (net, name)
    for m in T.MUTANTS:
        if m in ("state_not_carried", "state_early"):
            continue
        where = [(net, name) for net, table in tables.items() for name, caught in table.items() if m in caught]
        print("%s: caught by %d inputs" % (m, len(where)))
        assert where, m
    # H and W swapped: on 40 x 72 and 8 x 72 only -- a square net cannot show it
    assert any("swap_hw" in c for c in tables[(40, 72)].values()) and any("swap_hw" in c for c in tables[(8, 72)].values())
    assert not any("swap_hw" in c for net in ((8, 8), (64, 64)) for c in tables[net].values())
    # what each named case is there for
    t = tables[(64, 64)]
    assert "lt_for_le" in t["steps of exactly tol and of tol + 1"] and "carried_over_own" in t["an own hint over a carried one"]
    assert "life_off_by_one" in t["life 3 of 6 frames"] and "raw_prev_only" in t["life 0 over max_batch frames"]
    assert "tol_uncompensated" in t["search 4, a pan by (4, -4)"] and "warp_minus" in t["search 1, a pan by (0, 1)"]
    assert "p_block_chain" in t["a hint straddling blocks with different vectors"] and "p_block_chain" in t["the claim"]
    # the state: the split-invariance sequence of the GPU file, whole against split
    l, ab, mask = T.pipeline_inputs()
    whole = T.play_parts(T.Sim(), l, ab, mask, [7])
    for m, parts in (("state_not_carried", [3, 4]), ("state_early", [1] * 7)):
        assert _same3(T.play_parts(T.Sim(m), l, ab, mask, [7]), whole), m       # one call never reads the state
        assert not _same3(T.play_parts(T.Sim(m), l, ab, mask, parts), whole), m


def test_the_claims_pixel_counts_on_the_rule():
    c = T.CLAIM
    l, ab, mask, pos = T.claim_inputs()
    assert int((mask[0] != 0).sum()) == 64 and not mask[1:].any()                   # hinted at frame 0 only
    sim = T.Sim()
    A, Mk, G, v = sim.apply(l, ab, mask)
    inner, of, held_on_object = T.claim_counts(Mk, pos)
    print("frame 11: %d of %d interior pixels still hinted; %d pixels of the held rectangle on the object" % (inner, of, held_on_object))
    assert inner == of == 36 and held_on_object == 0
    on = Mk[11] != 0
    oy, ox = pos[11]
    assert on[oy:oy + c["size"], ox:ox + c["size"]].sum() == on.sum() == 64 and (G[11][on] == 11).all()
    # with motion off (search 0) the hint dies where the object's texture moves from under it
    sim.motion(search=0, penalty=0.5)
    assert (sim.apply(l, ab, mask)[1][11] != 0).sum() < 8


# ------------------------------------------------------------------------------------------------ 4. the header, the kernel's brief, the plan
@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan_ubsan"])
def test_params_scratch_walk_and_plan(tmp_path, san):
    run = subprocess.run([TC._make("track_selftest", str(tmp_path), san)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert re.match(r"track_selftest: ok \(4096 nets, 216 walked calls, 8 plans\)", run.stdout.splitlines()[-1]), run.stdout + run.stderr


def test_the_header_is_plain_cpp_and_the_kernel_keeps_to_its_brief():
    text = open(os.path.join(CSRC, "idc_track.h")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", text) == ["math.h", "stddef.h", "stdint.h", "idc_motion.h"]
    assert "__global__" not in text and not re.search(r"\bhip[A-Z]\w+\(", text)
    tool = open(os.path.join(REPO, "tools", "track_selftest.cpp")).read()
    assert [i for i in re.findall(r"#include\s*\"([^\"]+)", tool)] == ["idc_track.h", "idc_batch.h"]
    kern = open(os.path.join(CSRC, "idc_track.hip")).read()
    body = kern.split("#include <hip/hip_runtime.h>")[1]
    assert len(re.findall(r"hipLaunchKernelGGL\(", body)) == 1 and re.findall(r"void (\w+_kernel)\(", body) == ["track_hints_kernel"]
    assert "atomic" not in body and "asm" not in body and "while" not in body and "__syncthreads" not in body      # no thread waits on another
    assert "track_walk(" in body                                                    # the function the selftest holds to the recursion
    ex = open(os.path.join(CSRC, "idc_exec.hip")).read()
    col = ex.split("static int batch_colourise(")[1].split("\n}\n")[0]
    order = [col.index(s) for s in ("launch_prologue(", "launch_hint_layers(", "if (tracking) {", "launch_motion_search(", "launch_track_hints(", "run_graph(",
                                    "run_temporal(")]
    assert order == sorted(order)                                                   # prologue, layers, search, track, network, filter
    assert col.count("launch_track_hints(") == 1                                   # one launch for all n frames
    run = ex.split("static int run_temporal(")[1].split("\n}\n")[0]
    assert "if (!searched) HIPCHK(h, launch_motion_search(" in run                  # tracking off: the parent's launches, in the parent's order
    header = open(os.path.join(REPO, "include", "ideepcolor.h")).read()
    for phrase in ("HINT TRACKING along those vectors (idc_set_hint_tracking)", "An own hint always wins", "a NaN\n *                     carries nothing",
                   "life 0, tol 8.0: plausible values.  NOBODY HAS MEASURED THEM ON TRAINED WEIGHTS", "Hints that follow the vectors: the next section"):
        assert phrase in header, phrase
    assert "idc_temporal_vectors gives a caller what it needs" not in header
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS := .*\bidc_track\b", mk, re.M) and re.search(r"^track_selftest:", mk, re.M)
    assert "csrc/track_selftest" in open(os.path.join(REPO, ".gitignore")).read()


# ------------------------------------------------------------------------------------------------ 5. the ABI
def test_abi_symbols_prototypes_and_null_statuses():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ideepcolor.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+idc_set_hint_tracking\s*\(\s*idc_handle\s+h\s*,\s*int\s+on\s*,\s*int\s+life\s*,\s*double\s+tol\s*\)\s*;", header)
    assert re.search(r"\bint\s+idc_tracked_hints\s*\(\s*idc_handle\s+h\s*,\s*int\s+slot\s*,\s*float\s*\*\s*ab\s*,\s*float\s*\*\s*mask\s*,\s*int32_t\s*\*\s*age\s*\)\s*;", header)
    assert re.search(r"\bint\s+idc_track_hints_apply\s*\(\s*idc_handle\s+h\s*,\s*int\s+n\s*,\s*const\s+float\s*\*\s*l\s*,\s*const\s+float\s*\*\s*ab\s*,"
                     r"\s*const\s+float\s*\*\s*mask\s*,\s*float\s*\*\s*ab_out\s*,\s*float\s*\*\s*mask_out\s*,\s*int32_t\s*\*\s*age_out\s*,\s*int8_t\s*\*\s*v_out\s*\)\s*;",
                     header)
    # the motion pair keeps its prototypes
    assert re.search(r"\bint\s+idc_set_temporal_motion\s*\(\s*idc_handle\s+h\s*,\s*int\s+on\s*,\s*int\s+search\s*,\s*double\s+penalty\s*\)\s*;", header)
    assert re.search(r"\bint\s+idc_temporal_vectors\s*\(\s*idc_handle\s+h\s*,\s*int\s+slot\s*,\s*int8_t\s*\*\s*v[^)]*\)\s*;", header)
    for s in ("idc_set_hint_tracking", "idc_tracked_hints", "idc_track_hints_apply"):
        assert s in N.EXPORTED_SYMBOLS
    lib = N.load()
    assert lib.idc_set_hint_tracking(None, 1, 0, 8.0) == -1              # a null handle, without a device
    assert lib.idc_tracked_hints(None, 0, None, None, None) == -1
    assert lib.idc_track_hints_apply(None, 1, None, None, None, None, None, None, None) == -1
    assert lib.idc_set_hint_tracking.argtypes[1:] == [ctypes.c_int, ctypes.c_int, ctypes.c_double]
    assert len(lib.idc_tracked_hints.argtypes) == 5 and len(lib.idc_track_hints_apply.argtypes) == 9


# ------------------------------------------------------------------------------------------------ 6. the Python plumbing
class _Lib(TC._Lib):
    def idc_set_temporal_motion(self, h, on, search, penalty):
        self.calls.append(("motion", on, search, penalty))
        return 0

    def idc_set_hint_tracking(self, h, on, life, tol):
        self.calls.append(("track", on, life, tol))
        return 0

    def idc_tracked_hints(self, h, slot, ab, mask, age):
        self.calls.append(("tracked", slot))
        self.nulls = (ab is None, mask is None, age is None)
        n = 2                                            # this library's own frame count: the planes come back packed
        if mask is not None:
            ctypes.memmove(mask, np.arange(n * 64, dtype=np.float32).ctypes.data, n * 64 * 4)
        if age is not None:
            ctypes.memmove(age, np.arange(n * 64, dtype=np.int32).ctypes.data, n * 64 * 4)
        return 0

    def idc_track_hints_apply(self, h, n, l, ab, mask, ab_out, mask_out, age_out, v_out):
        self.calls.append(("apply", n, v_out is not None))
        ctypes.memmove(mask_out, mask, n * 64 * 4)
        return 0


class _Stub(TC._Stub):
    def __init__(self, fail_after=None):
        TC._Stub.__init__(self, fail_after)
        self.lib = _Lib()

    def _enqueue(self, kind, images, hints):
        TC._Stub._enqueue(self, kind, images, hints)
        self.seen[-1] = self.seen[-1] + (self.__dict__.get("_motion"), self.__dict__.get("_track"))


def _calls(e, what):
    return [c for c in e.lib.calls if c[0] == what]


def test_the_three_calls_marshal_their_arguments():
    e = _Stub()
    e.set_hint_tracking()
    e.set_hint_tracking(life=3, tol=2.5)
    e.set_hint_tracking(None)
    e.set_hint_tracking(False)
    assert e.lib.calls == [("track", 1, 0, 8.0), ("track", 1, 3, 2.5), ("track", 0, 3, 2.5), ("track", 0, 0, 8.0)]
    assert e.__dict__["_track"] is None and e._temporal is None and e.__dict__.get("_motion") is None
    ab, mask, age = e.tracked_hints(1, 2)
    assert ab.shape == (2, 2, 8, 8) and mask.shape == (2, 8, 8) and age.shape == (2, 8, 8) and age.dtype == np.int32 and e.lib.calls[-1] == ("tracked", 1)
    assert mask[1, 0, 0] == 64.0 and age[1, 7, 7] == 127                   # frame 1 starts one plane in, whatever max_batch is
    with pytest.raises(ValueError):
        e.tracked_hints(0)                                                # nothing enqueued on the slot, and no count given
    ab, mask, age = e.tracked_hints(1, 2, want=("mask",))                 # a plane that is not wanted is a NULL pointer and comes back as None
    assert ab is None and age is None and mask.shape == (2, 8, 8) and mask[1, 0, 0] == 64.0 and e.lib.nulls == (True, False, True)
    with pytest.raises(ValueError):
        e.tracked_hints(1, 2, want=())
    l = np.zeros((2, 1, 8, 8), np.float32)
    m = np.arange(128, dtype=np.float32).reshape(2, 8, 8)
    out = e.track_hints_apply(l, np.zeros((2, 2, 8, 8)), m)
    assert len(out) == 3 and np.array_equal(out[1], m) and e.lib.calls[-1] == ("apply", 2, False)
    out = e.track_hints_apply(l, np.zeros((2, 2, 8, 8)), m, vectors=True)
    assert len(out) == 4 and out[3].shape == (2, 1, 1, 2) and out[3].dtype == np.int8 and e.lib.calls[-1] == ("apply", 2, True)
    for bad in ((l, np.zeros((2, 3, 8, 8)), m), (np.zeros((3, 8, 8)), np.zeros((2, 2, 8, 8)), m), (l, np.zeros((2, 2, 8, 8)), m[:1])):
        with pytest.raises(ValueError):
            e.track_hints_apply(*bad)


@pytest.mark.parametrize("name", TC.GENERATORS)
def test_the_track_key_sets_and_restores_with_the_motion_setting(name):
    on = dict(T.DEFAULT)
    # no tracking asked for: no tracking call reaches the library, whatever the temporal keyword
    for temporal in (None, True, False, dict(R.DEFAULT), dict(motion=True), dict(motion=dict(M.DEFAULT)), dict(motion=dict(search=2, penalty=0.0, track=False))):
        e = _Stub()
        list(TC._generator(e, name, temporal=temporal))
        assert _calls(e, "track") == [] and len(e.seen) == 3, temporal
    # track=True: set behind the motion setting and before the reset and the first batch, every batch sees it, off again behind the last wait
    e = _Stub()
    list(TC._generator(e, name, temporal=dict(motion=dict(track=True))))
    calls = e.lib.calls
    assert calls[:4] == [("set", 1, 0.6, 4.0, 1, 12.0), ("motion", 1, 4, 0.5), ("track", 1, 0, 8.0), ("reset",)] and calls[4][0] == "enqueue"
    assert calls[-3:] == [("track", 0, 0, 8.0), ("motion", 0, 4, 0.5), ("set", 0, 0.6, 4.0, 1, 12.0)] and calls[-4][0] == "wait"
    assert [s[4] for s in e.seen] == [dict(M.DEFAULT)] * 3 and [s[5] for s in e.seen] == [on] * 3
    assert e._temporal is None and e.__dict__.get("_motion") is None and e.__dict__.get("_track") is None
    # a dict of parameters beside the motion's; the previous settings are what comes back
    e = _Stub()
    e.set_temporal_motion(2, 3.0)
    e.set_hint_tracking(life=9, tol=1.0)
    list(TC._generator(e, name, temporal=dict(motion=dict(search=7, penalty=0.0, track=dict(life=2, tol=5.0)))))
    assert [s[4] for s in e.seen] == [dict(search=7, penalty=0.0)] * 3 and [s[5] for s in e.seen] == [dict(life=2, tol=5.0)] * 3
    assert e.__dict__["_motion"] == dict(search=2, penalty=3.0) and e.__dict__["_track"] == dict(life=9, tol=1.0)
    assert _calls(e, "track")[-1] == ("track", 1, 9, 1.0)
    # track=False switches a tracking that is on off for the stream; without the key it stands as it is
    e.seen, e.lib.calls = [], []
    list(TC._generator(e, name, temporal=dict(motion=dict(search=4, penalty=0.5, track=False))))
    assert [s[5] for s in e.seen] == [None] * 3 and e.__dict__["_track"] == dict(life=9, tol=1.0)
    assert _calls(e, "track") == [("track", 0, 9, 1.0), ("track", 1, 9, 1.0)]
    e.seen, e.lib.calls = [], []
    list(TC._generator(e, name, temporal=dict(motion=True)))
    assert [s[5] for s in e.seen] == [dict(life=9, tol=1.0)] * 3 and _calls(e, "track") == []
    # abandoned after the first result, and an exception on the way: restored as well
    e = _Stub()
    g = TC._generator(e, name, temporal=dict(motion=dict(track=True)))
    next(g)
    assert e.__dict__["_track"] == on
    g.close()
    assert e.__dict__["_track"] is None and e.__dict__["_motion"] is None and e._temporal is None
    assert [c[0] for c in e.lib.calls[-3:]] == ["track", "motion", "set"]
    e = _Stub(fail_after=1)
    with pytest.raises(RuntimeError):
        list(TC._generator(e, name, temporal=dict(motion=dict(track=True))))
    assert e.__dict__["_track"] is None and e.__dict__["_motion"] is None and e._temporal is None
    # parameters the engine refuses are refused before anything is enqueued, and the settings come back
    e = _Stub()
    with pytest.raises(TypeError):
        next(TC._generator(e, name, temporal=dict(motion=dict(track=dict(radius=2)))))
    assert e.seen == [] and e._temporal is None and e.__dict__.get("_motion") is None and e.__dict__.get("_track") is None


def test_colorize_video_sends_a_key_frames_hints_to_that_frame_only_when_the_device_carries_them():
    a, b = [(0, 0, 1, 1, 10.0, 20.0)], [(2, 2, 3, 3, -5.0, 5.0)]
    frames = TC._video_frames(["rgb"] * 5 + ["g8"] * 2)

    def stub():
        e = _Stub()
        e.temporal_info = lambda slot, n=None: (np.array([1, 0][:n], np.int32), np.zeros(n))
        e.tracked_hints = lambda slot, n=None, want=None: (None, np.full((n, 8, 8), slot + 1.0 + (want != ("mask",)), np.float32), None)   # the mask alone
        return e
    # tracking asked for, a dict of key frames: each list goes to its own frame, every other frame has none; every frame once, in order
    e = stub()
    results = list(e.colorize_video(iter(frames), hints={1: a, 4: b}, temporal=dict(motion=dict(track=True))))
    assert [int(r[0].flat[0]) for r in results] == [1, 2, 3, 4, 5, 6, 7] and all(len(r) == 2 for r in results)
    assert [(s[0], s[2]) for s in e.seen] == [("images", [1, 2]), ("images", [3, 4]), ("images", [5]), ("gray", [6, 7])]
    assert [s[3] for s in e.seen] == [[None, a], [None, None], [b], [None, None]]
    assert all(s[5] == dict(T.DEFAULT) for s in e.seen) and _calls(e, "track") == [("track", 1, 0, 8.0), ("track", 0, 0, 8.0)]
    # a list still goes to every frame
    e = stub()
    list(e.colorize_video(iter(frames[:3]), hints=a, temporal=dict(motion=dict(track=True))))
    assert [s[3] for s in e.seen] == [[a, a], [a]]
    # without tracking (no key, False, or no motion at all) the key frames hold, as before
    for temporal in (dict(motion=True), dict(motion=dict(search=4, penalty=0.5, track=False)), True):
        e = stub()
        list(e.colorize_video(iter(frames[:5]), hints={1: a, 4: b}, temporal=temporal))
        assert [s[3] for s in e.seen] == [[None, a], [a, a], [b]] and _calls(e, "track") == [], temporal
    # tracked=True: the frame's tracked mask plane behind the other results; zeros where the call ran without tracking
    e = stub()
    results = list(e.colorize_video(iter(frames[:3]), hints={0: a}, temporal=dict(motion=dict(track=True)), tracked=True))
    assert [len(r) for r in results] == [3, 3, 3] and [float(r[2][0, 0]) for r in results] == [1.0, 1.0, 2.0] and results[0][2].shape == (8, 8)
    e = stub()
    e.temporal_vectors = lambda slot, n=None: np.zeros((n, 1, 1, 2), np.int8)
    results = list(e.colorize_video(iter(frames[:3]), temporal=dict(motion=dict(track=True)), vectors=True, tracked=True))
    assert [len(r) for r in results] == [4, 4, 4] and results[0][2].shape == (1, 1, 2) and results[0][3].shape == (8, 8)
    e = stub()
    e.tracked_hints = None
    results = list(e.colorize_video(iter(frames[:3]), temporal=dict(motion=True), tracked=True))
    assert all(r[2].shape == (8, 8) and not r[2].any() for r in results)
