"""The temporal ab filter's rule (include/ideepcolor.h, "frame sequences") restated in plain loops and numpy float64, the inputs of
tests/test_temporal_gpu.py, and the one driver both test files play them through.

``frame`` is the rule for ONE frame from a GIVEN previous state.  That is how the GPU file uses it: every frame of every call is checked against
the restatement of the device's own previous output (the state before the call for frame 0, the device's y of frame f - 1 and the call's own
l plane of frame f - 1 after it), so a rare rounding difference cannot travel down the sequence.

``Sim`` plays a handle: it keeps the sequence state and runs calls of n frames through ``frame``.  With ``mutant`` set it breaks the rule in one
named way; tests/test_temporal_cpu.py shows that ``play`` -- the scenario of the GPU file's first case and its checks -- passes on the rule
and fails on every mutant, so the GPU file would catch a kernel that made the same mistake."""
import numpy as np

DEFAULT = dict(strength=0.6, sigma=4.0, radius=1, cut=12.0)
NETS = [(8, 8), (40, 72), (64, 64)]
MAX_BATCH = 8
BIT_EQUAL_SHARE = 0.999          # of the values of each frame
D_REL = 1e-12
CUT_MARGIN = 1e-6                # every D of the inputs is further than this, relative, from cut^2
MUTANTS = ["replicate", "no_divide", "sigma2", "cut_c", "cut_blends", "lprev_kept_on_cut", "pred_from_state", "raw_prev", "swap_hw"]


# ------------------------------------------------------------------------------------------------ the rule
def window_mean_loops(e, R):
    """m of the rule in plain loops: rows j-R..j+R (outer, ascending), columns i-R..i+R (inner, ascending), clipped; sum / taps inside."""
    H, W = e.shape
    m = np.zeros((H, W), np.float64)
    for j in range(H):
        for i in range(W):
            s, taps = np.float64(0.0), 0
            for jj in range(j - R, j + R + 1):
                if jj < 0 or jj >= H:
                    continue
                for ii in range(i - R, i + R + 1):
                    if ii < 0 or ii >= W:
                        continue
                    s = s + e[jj, ii]
                    taps += 1
            m[j, i] = s / np.float64(taps)
    return m


def window_mean(e, R, mutant=None):
    """``window_mean_loops`` on whole planes: the same additions in the same order per pixel (a tap outside adds nothing: e >= 0, the sum starts
    at +0), bit for bit (test_temporal_cpu.py)."""
    if mutant == "swap_hw":          # the plane read as [W,H]
        return window_mean(e.reshape(e.shape[1], e.shape[0]), R).reshape(e.shape)
    H, W = e.shape
    s = np.zeros((H, W), np.float64)
    taps = np.zeros((H, W), np.float64)
    if mutant == "replicate":        # indices clamped to the plane, (2R+1)^2 taps everywhere
        jj, ii = np.arange(H), np.arange(W)
        for dj in range(-R, R + 1):
            for di in range(-R, R + 1):
                s = s + e[np.clip(jj + dj, 0, H - 1)][:, np.clip(ii + di, 0, W - 1)]
        return s / np.float64((2 * R + 1) ** 2)
    for dj in range(-R, R + 1):
        j0, j1 = max(0, -dj), min(H, H - dj)             # rows j with 0 <= j + dj < H
        for di in range(-R, R + 1):
            i0, i1 = max(0, -di), min(W, W - di)
            if j0 >= j1 or i0 >= i1:
                continue
            s[j0:j1, i0:i1] = s[j0:j1, i0:i1] + e[j0 + dj:j1 + dj, i0 + di:i1 + di]
            taps[j0:j1, i0:i1] += 1.0
    return s if mutant == "no_divide" else s / taps


def frame(x, l, y_prev, l_prev, have, p, mutant=None, exp_shift=0):
    """One frame: x [2,H,W] f32, l [H,W] f32, the previous state -> (y [2,H,W] f32, cut, D, g [H,W] f64 or None)."""
    x = np.asarray(x, np.float32)
    l = np.asarray(l, np.float32)
    if not have:
        return x.copy(), 1, 0.0, None
    s, sigma, R, c = np.float64(p["strength"]), np.float64(p["sigma"]), int(p["radius"]), np.float64(p["cut"])
    d = l.astype(np.float64) - np.asarray(l_prev, np.float32).astype(np.float64)
    e = d * d
    D = float(e.sum() / np.float64(e.size))
    is_cut = bool(c > 0 and D > (c if mutant == "cut_c" else c * c))
    if is_cut and mutant != "cut_blends":
        return x.copy(), 1, D, None
    m = window_mean(e, R, mutant)
    ex = np.exp(-m / ((sigma * sigma) if mutant == "sigma2" else (2.0 * sigma * sigma)))
    if exp_shift:
        ex = np.nextafter(ex, np.inf if exp_shift > 0 else -np.inf)
    g = s * ex
    xd = x.astype(np.float64)
    y = (xd + g[None] * (np.asarray(y_prev).astype(np.float64) - xd)).astype(np.float32)
    return y, int(is_cut), D, g


class Sim(object):
    """A handle's sequence state and its calls, by ``frame``; ``mutant`` breaks it in one way.  The interface ``play`` drives: set / reset /
    apply / state, as HipColorizer's set_temporal_filter / temporal_reset / temporal_apply / temporal_state."""

    def __init__(self, H, W, mutant=None):
        self.H, self.W, self.mutant = H, W, mutant
        self.p = dict(DEFAULT)
        self.reset()

    def set(self, **p):
        self.p = dict(p)

    def reset(self):
        self.y_prev, self.l_prev, self.have = np.zeros((2, self.H, self.W), np.float32), np.zeros((self.H, self.W), np.float32), False

    def state(self):
        return self.y_prev.copy(), self.l_prev.copy(), self.have

    def apply(self, ab, l):
        mu = self.mutant
        n = ab.shape[0]
        y, cut, D = np.empty_like(ab), np.zeros(n, np.int32), np.zeros(n, np.float64)
        yp, lp, have = self.y_prev, self.l_prev, self.have
        l_call = self.l_prev
        for f in range(n):
            if mu == "pred_from_state" and f > 0:
                lp = l_call
            y[f], cut[f], D[f], _ = frame(ab[f], l[f], yp, lp, have, self.p, mu if mu in ("replicate", "no_divide", "sigma2", "cut_c", "cut_blends", "swap_hw") else None)
            if mu == "f64_state" and have and not cut[f]:      # y carried in float64 inside a call, rounded only when it is stored
                g = frame(ab[f], l[f], yp, lp, have, self.p)[3]
                xd = ab[f].astype(np.float64)
                yp = xd + g[None] * (np.asarray(yp, np.float64) - xd)
                y[f] = yp.astype(np.float32)
            else:
                yp = ab[f] if mu == "raw_prev" else y[f]
            if not (mu == "lprev_kept_on_cut" and cut[f] and have):
                lp = l[f]
            have = True
        self.y_prev, self.l_prev, self.have = np.asarray(yp).astype(np.float32), np.asarray(lp, np.float32).copy(), True
        return y, cut, D


# ------------------------------------------------------------------------------------------------ comparisons
def ulp_check(got, want):
    """-> (every value of got is want or one of its two float32 neighbours, share of bit-equal values)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    lo, hi = np.nextafter(want, np.float32(-np.inf)), np.nextafter(want, np.float32(np.inf))
    within = bool(((got >= lo) & (got <= hi)).all())
    return within, float((got.view(np.uint32) == want.view(np.uint32)).mean())


def verify_call(before, ab, l, p, y, cut, D, what=""):
    """One call's results against ``frame`` per frame from the device's own previous output.  ``before`` = (y_prev, l_prev, have) before the
    call.  The bar: within one float32 ulp everywhere, bit-equal on at least BIT_EQUAL_SHARE of each frame, the flags equal, D to D_REL."""
    yp, lp, have = before
    c = float(p["cut"])
    for f in range(ab.shape[0]):
        wy, wc, wD, _ = frame(ab[f], l[f], yp, lp, have, p)
        tag = "%s frame %d" % (what, f)
        if have and c > 0:
            assert abs(wD - c * c) > CUT_MARGIN * c * c, "%s: D %.17g sits on the cut threshold: a bad input" % (tag, wD)
        assert int(cut[f]) == wc, "%s: cut %d, the rule says %d (D %.6g)" % (tag, int(cut[f]), wc, wD)
        assert abs(float(D[f]) - wD) <= D_REL * abs(wD), "%s: D %.17g, the rule says %.17g" % (tag, float(D[f]), wD)
        if wc:
            assert np.array_equal(np.asarray(y[f]).view(np.uint32), np.asarray(ab[f], np.float32).view(np.uint32)), "%s: a passed frame is not x bit for bit" % tag
        within, share = ulp_check(y[f], wy)
        assert within, "%s: a value further than one float32 ulp from the rule (max |diff| %.3g)" % (tag, float(np.abs(y[f].astype(np.float64) - wy).max()))
        assert share >= BIT_EQUAL_SHARE, "%s: only %.5f of the values are bit-equal" % (tag, share)
        yp, lp, have = y[f], l[f], True


# ------------------------------------------------------------------------------------------------ inputs
def _smooth(rs, H, W):
    """A smooth plane in about -40..40: a few low-frequency cosines."""
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.zeros((H, W))
    for _ in range(3):
        fy, fx, ph = rs.uniform(0.02, 0.2), rs.uniform(0.02, 0.2), rs.uniform(0, 6.28)
        out += 13.0 * np.cos(fy * jj + fx * ii + ph)
    return out


def frames(H, W, n, seed, cuts=(), still=None, edge=None):
    """n frames -> (ab [n,2,H,W] f32, l [n,H,W] f32).  A static shot with grain (sd 3: D about 18, between cut and cut^2 of the defaults) and a
    small lit patch that wanders; frame f in ``cuts`` starts a wholly different shot.  ``still``: every l plane is this one.  ``edge`` = (step,
    amplitude): a vertical step edge that moves ``step`` columns a frame over a flat plane, no grain."""
    rs = np.random.RandomState(seed)
    ab = rs.uniform(-80.0, 80.0, (n, 2, H, W)).astype(np.float32)
    l = np.empty((n, H, W), np.float32)
    base = _smooth(rs, H, W)
    for f in range(n):
        if still is not None:
            l[f] = still
            continue
        if edge is not None:
            plane = np.full((H, W), -20.0)
            plane[:, :min(W, (f + 1) * edge[0])] += edge[1]
            l[f] = plane.astype(np.float32)
            continue
        if f in cuts:
            base = rs.uniform(-50.0, 50.0, (H, W))
        plane = base + rs.normal(0.0, 3.0, (H, W))
        y0, x0 = (3 * f) % max(H - 3, 1), (5 * f) % max(W - 3, 1)
        plane[y0:y0 + 3, x0:x0 + 3] += 25.0
        l[f] = plane.astype(np.float32)
    return ab, l


def scenario(H, W, max_batch=MAX_BATCH):
    """The calls of the GPU file's first case on an H x W net, as steps ("reset",) | ("set", params) | ("call", ab, l, check, note); check is
    None, "x" (y is x bit for bit), "still" (D = 0 on every frame) or "edge" (the moving step edge's bound)."""
    seed = 1000 * H + W
    p = dict(DEFAULT)
    steps = [("reset",), ("set", dict(p))]
    ab, l = frames(H, W, 1, seed + 1)
    steps.append(("call", ab, l, "x", "the first frame ever"))
    ab, l = frames(H, W, 1, seed + 2)
    steps.append(("call", ab, l, None, "n = 1: the state is the only predecessor"))
    ab, l = frames(H, W, 5, seed + 3, cuts=(2,))
    steps.append(("call", ab, l, None, "n = 5, a cut in the middle"))
    ab, l = frames(H, W, max_batch, seed + 4, cuts=(0, max_batch - 1))
    steps.append(("call", ab, l, None, "n = max_batch, cuts at frame 0 and at the last frame"))
    for R in range(4):
        steps.append(("set", dict(p, radius=R)))
        ab, l = frames(H, W, 3, seed + 10 + R)
        steps.append(("call", ab, l, None, "radius %d" % R))
    steps.append(("set", dict(p, cut=0.0)))
    ab, l = frames(H, W, 2, seed + 20, cuts=(0, 1))
    steps.append(("call", ab, l, None, "cut = 0 with a huge D"))
    steps.append(("set", dict(p, strength=0.0)))
    ab, l = frames(H, W, 2, seed + 21)
    steps.append(("call", ab, l, "x", "strength 0"))
    steps.append(("set", dict(p)))
    ab, l = frames(H, W, 3, seed + 22, still=l[-1])
    steps.append(("call", ab, l, "still", "identical planes"))
    steps.append(("set", dict(p, cut=0.0, radius=1)))
    ab, l = frames(H, W, 4, seed + 23, edge=(2 if W <= 8 else 8, 60.0))
    steps.append(("call", ab, l, "edge", "a moving step edge"))
    steps.append(("reset",))
    steps.append(("set", dict(p)))
    ab, l = frames(H, W, 2, seed + 24)
    steps.append(("call", ab, l, None, "after a reset: frame 0 passes"))
    return steps


def play(backend, H, W, max_batch=MAX_BATCH):
    """Run ``scenario`` on ``backend`` (a ``Sim``, or the GPU file's adapter of an engine) and check every call; -> the number of frames checked.
    The state before each call is asked of the backend itself."""
    p, checked = dict(DEFAULT), 0
    for step in scenario(H, W, max_batch):
        if step[0] == "reset":
            backend.reset()
            assert not backend.state()[2]
            continue
        if step[0] == "set":
            p = dict(step[1])
            backend.set(**p)
            continue
        _, ab, l, check, note = step
        before = backend.state()
        y, cut, D = backend.apply(ab, l)
        what = "%dx%d, %s:" % (H, W, note)
        verify_call(before, ab, l, p, y, cut, D, what)
        after = backend.state()
        assert after[2] and np.array_equal(after[0].view(np.uint32), y[-1].view(np.uint32)) and np.array_equal(after[1], l[-1]), what + " the state afterwards"
        if check == "x":
            assert np.array_equal(y.view(np.uint32), ab.view(np.uint32)), what + " y is not x bit for bit"
        if check == "still":
            assert (np.asarray(D) == 0).all() and not np.asarray(cut).any(), what + " D or cut"
            yp = before[0]
            for f in range(ab.shape[0]):      # g = s exactly
                xd = ab[f].astype(np.float64)
                want = (xd + np.float64(p["strength"]) * (yp.astype(np.float64) - xd)).astype(np.float32)
                assert np.array_equal(y[f].view(np.uint32), want.view(np.uint32)), what + " g is not s exactly"
                yp = y[f]
        if check == "edge":
            s2 = float(p["sigma"]) ** 2
            lp, yp, hit = before[1], before[0], 0
            for f in range(ab.shape[0]):
                d = l[f].astype(np.float64) - lp.astype(np.float64)
                far = window_mean(d * d, int(p["radius"])) >= 36.0 * s2
                hit += int(far.sum())
                xd = ab[f].astype(np.float64)
                bound = float(p["strength"]) * np.exp(-18.0) * np.abs(yp.astype(np.float64) - xd) + np.spacing(np.abs(ab[f])).astype(np.float64)
                assert (np.abs(y[f].astype(np.float64) - xd)[:, far] <= bound[:, far]).all(), what + " frame %d: motion did not release the colour" % f
                lp, yp = l[f], y[f]
            assert hit > 0, what + " no pixel with m >= 36 sigma^2"
        checked += ab.shape[0]
    return checked


def swing_tolerance(A, B, s, k):
    """The closed form of the flicker claim.  With identical L planes g = s exactly, and x alternating between A and B gives
    y_k = x_k + s (y_{k-1} - x_k): the steady-state difference of consecutive frames is (1 - s) / (1 + s) of |A - B|, approached as s^k.  Each
    stored y is rounded to float32, an error of at most half an ulp of the larger magnitude a frame, which the recursion sums to at most
    (ulp / 2) / (1 - s); the difference of two frames carries twice that.  -> the tolerance on |y_k - y_{k-1}| after k frames, per value."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    mag = np.maximum(np.abs(A), np.abs(B)).astype(np.float32)
    return np.spacing(mag).astype(np.float64) / (1.0 - s) + 2.0 * s ** (k - 1) * np.abs(A - B) + 1e-12
