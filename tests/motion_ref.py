"""The motion compensation of the temporal ab filter (include/ideepcolor.h, "MOTION COMPENSATION") restated in plain loops and in numpy float64,
the inputs of tests/test_motion_gpu.py, and the one driver both test files play them through.

``vectors_loops`` is the rule word for word; ``vectors`` is its whole-plane twin, held bit-equal to it in J (tests/test_motion_cpu.py).
``frame`` is the rule for ONE frame from a GIVEN previous state: the vectors, the warp, then ``temporal_ref.frame`` on the warped state.  The GPU
file checks every frame of every call against the restatement of the device's OWN previous output, as the temporal file does.

``Sim`` plays a handle.  With ``mutant`` set it breaks the rule in one named way; tests/test_motion_cpu.py shows that ``play`` -- the scenario
of the GPU file's first case and its checks -- passes on the rule and fails on every mutant."""
import numpy as np

import temporal_ref as T

B = 8
DEFAULT = dict(search=4, penalty=0.5)
NETS = [(8, 8), (8, 72), (40, 72), (64, 64)]
MAX_BATCH = 8
MARGIN_REL = 1e-6                # where a comparison relies on a non-tie: second-best J - best J >= this, relative to the second-best J
MUTANTS = ["rank_reversed", "le_for_lt", "replicate", "penalty_abs", "warp_minus", "l_not_warped", "D_uncompensated", "apron_centre_vector",
           "previous_vectors", "state_early", "lprev_warped", "swap_hw"]


# ------------------------------------------------------------------------------------------------ the rule
def candidates(S):
    """[(dy, dx)] in rank order: (dy^2 + dx^2, dy, dx) ascending."""
    return sorted(((dy, dx) for dy in range(-S, S + 1) for dx in range(-S, S + 1)), key=lambda v: (v[0] * v[0] + v[1] * v[1], v[0], v[1]))


def valid(by, bx, dy, dx, H, W):
    return 0 <= B * by + dy and B * by + dy + B <= H and 0 <= B * bx + dx and B * bx + dx + B <= W


def vectors_loops(l, l_prev, S, lam):
    """The rule in plain loops -> (v int8 [H/8,W/8,2], J float64 [candidates in rank order, H/8, W/8], the mask of the valid ones)."""
    l, l_prev = np.asarray(l, np.float32), np.asarray(l_prev, np.float32)
    H, W = l.shape
    cands = candidates(S)
    v = np.zeros((H // B, W // B, 2), np.int8)
    J = np.zeros((len(cands), H // B, W // B), np.float64)
    ok = np.zeros((len(cands), H // B, W // B), bool)
    lam = np.float64(lam)
    for by in range(H // B):
        for bx in range(W // B):
            best, best_v = None, (0, 0)
            for k, (dy, dx) in enumerate(cands):
                if not valid(by, bx, dy, dx, H, W):
                    continue
                C = np.float64(0.0)
                for r in range(B):
                    for c in range(B):
                        d = np.float64(l[B * by + r, B * bx + c]) - np.float64(l_prev[B * by + r + dy, B * bx + c + dx])
                        C = C + d * d
                j = C / np.float64(64.0) + lam * np.float64(dy * dy + dx * dx)
                J[k, by, bx], ok[k, by, bx] = j, True
                if k == 0:
                    best = j
                elif j < best:
                    best, best_v = j, (dy, dx)
            v[by, bx] = best_v
    return v, J, ok


def costs(l, l_prev, S, lam, mutant=None):
    """J of every candidate (rank order) and block on whole planes, the additions in the rule's order -> (J [K,H/8,W/8], ok mask, cands)."""
    l, l_prev = np.asarray(l, np.float32).astype(np.float64), np.asarray(l_prev, np.float32).astype(np.float64)
    H, W = l.shape
    nby, nbx = H // B, W // B
    cands = candidates(S)
    J = np.zeros((len(cands), nby, nbx), np.float64)
    ok = np.zeros((len(cands), nby, nbx), bool)
    lam = np.float64(lam)
    jj, ii = np.arange(H), np.arange(W)
    for k, (dy, dx) in enumerate(cands):
        if mutant == "replicate":                    # every candidate valid, the plane's border repeated
            by0, by1, bx0, bx1 = 0, nby, 0, nbx
            shifted = l_prev[np.clip(jj + dy, 0, H - 1)][:, np.clip(ii + dx, 0, W - 1)]
        else:
            by0, by1 = (-dy + B - 1) // B if dy < 0 else 0, min(nby, (H - B - dy) // B + 1)
            bx0, bx1 = (-dx + B - 1) // B if dx < 0 else 0, min(nbx, (W - B - dx) // B + 1)
            if by0 >= by1 or bx0 >= bx1:
                continue
            shifted = np.zeros((H, W), np.float64)
            r0, r1, c0, c1 = B * by0, B * by1, B * bx0, B * bx1
            shifted[r0:r1, c0:c1] = l_prev[r0 + dy:r1 + dy, c0 + dx:c1 + dx]
        d = (l - shifted)[B * by0:B * by1, B * bx0:B * bx1]
        # one accumulator per block, r outer and c inner: cumsum adds strictly in sequence (0 + x is x exactly)
        dd = (d * d).reshape(by1 - by0, B, bx1 - bx0, B).transpose(0, 2, 1, 3).reshape(by1 - by0, bx1 - bx0, B * B)
        C = np.cumsum(dd, axis=-1)[..., -1]
        n2 = np.float64(dy * dy + dx * dx)
        J[k, by0:by1, bx0:bx1] = C / np.float64(64.0) + lam * (np.sqrt(n2) if mutant == "penalty_abs" else n2)
        ok[k, by0:by1, bx0:bx1] = True
    return J, ok, cands


def choose(J, ok, cands, mutant=None):
    """The choice -> v int8 [H/8,W/8,2]: best starts as rank 0, a later valid candidate replaces it iff its J < best strictly."""
    order = list(range(len(cands)))
    if mutant == "rank_reversed":
        order = order[::-1]
    best = np.full(J.shape[1:], np.nan)
    pick = np.full(J.shape[1:], -1, np.int64)
    for k in order:
        with np.errstate(invalid="ignore"):
            better = (J[k] <= best) if mutant == "le_for_lt" else (J[k] < best)
        take = ok[k] & ((pick < 0) | better)
        best = np.where(take, J[k], best)
        pick = np.where(take, k, pick)
    table = np.array(cands, np.int8)
    return table[pick]


def vectors(l, l_prev, S, lam, mutant=None):
    J, ok, cands = costs(l, l_prev, S, lam, mutant)
    return choose(J, ok, cands, mutant)


def margins(l, l_prev, S, lam):
    """Per block: (second-best J - best J) / second-best J over the valid candidates (inf where only one is valid or the second-best is 0)."""
    J, ok, _ = costs(l, l_prev, S, lam)
    Jm = np.where(ok, J, np.inf)
    if Jm.shape[0] < 2:
        return np.full(Jm.shape[1:], np.inf)
    srt = np.sort(Jm, axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = (srt[1] - srt[0]) / srt[1]
    return np.where(np.isfinite(srt[1]) & (srt[1] > 0), rel, np.inf)


def warp(plane, v, sign=1):
    """out[..., p] = plane[..., p + sign * v(block of p)]; indices clamped to the plane (the rule's own vectors never leave it)."""
    H, W = plane.shape[-2:]
    vy = np.repeat(np.repeat(v[..., 0].astype(np.int64), B, 0), B, 1)
    vx = np.repeat(np.repeat(v[..., 1].astype(np.int64), B, 0), B, 1)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return plane[..., np.clip(jj + sign * vy, 0, H - 1), np.clip(ii + sign * vx, 0, W - 1)]


def _blend(x, yw, g):
    xd = np.asarray(x, np.float32).astype(np.float64)
    return (xd + g[None] * (np.asarray(yw, np.float32).astype(np.float64) - xd)).astype(np.float32)


def frame(x, l, y_prev, l_prev, have, p, mp, mutant=None, v_before=None):
    """One frame: x [2,H,W] f32, l [H,W] f32, the previous state, the filter's parameters p and the motion's mp (search, penalty) ->
    (y [2,H,W] f32, cut, D, v int8 [H/8,W/8,2], extras dict: m, g, lw).  ``v_before``: the previous frame's vectors (a mutant's)."""
    x, l = np.asarray(x, np.float32), np.asarray(l, np.float32)
    H, W = l.shape
    if not have:
        return x.copy(), 1, 0.0, np.zeros((H // B, W // B, 2), np.int8), {}
    S, lam = int(mp["search"]), float(mp["penalty"])
    v = vectors(l, l_prev, S, lam, mutant if mutant in ("rank_reversed", "le_for_lt", "replicate", "penalty_abs") else None)
    used = v
    if mutant == "previous_vectors":
        used = v_before if v_before is not None else np.zeros_like(v)
    sign = -1 if mutant == "warp_minus" else 1
    lw, yw = warp(np.asarray(l_prev, np.float32), used, sign), warp(np.asarray(y_prev, np.float32), used, sign)
    if mutant == "l_not_warped":
        lw = np.asarray(l_prev, np.float32)
    if mutant == "state_early":          # the top half of y is in y_prev's place before the bottom half reads it
        y0 = T.frame(x, l, yw, lw, True, p)[0]
        mixed = np.array(y_prev, np.float32)
        mixed[:, :H // 2] = y0[:, :H // 2]
        yw2 = warp(mixed, used, sign)
        yw = np.concatenate([yw[:, :H // 2], yw2[:, H // 2:]], axis=1)
    if mutant in ("D_uncompensated", "apron_centre_vector"):
        s, sigma, R, c = np.float64(p["strength"]), np.float64(p["sigma"]), int(p["radius"]), np.float64(p["cut"])
        d = l.astype(np.float64) - lw.astype(np.float64)
        e = d * d
        if mutant == "D_uncompensated":
            d0 = l.astype(np.float64) - np.asarray(l_prev, np.float32).astype(np.float64)
            D = float((d0 * d0).sum() / np.float64(e.size))
            m = T.window_mean(e, R)
        else:
            D = float(e.sum() / np.float64(e.size))
            m = np.zeros((H, W), np.float64)
            for by in range(H // B):
                for bx in range(W // B):
                    one = np.broadcast_to(used[by, bx], used.shape)
                    db = l.astype(np.float64) - warp(np.asarray(l_prev, np.float32), one, sign).astype(np.float64)
                    m[B * by:B * by + B, B * bx:B * bx + B] = T.window_mean(db * db, R)[B * by:B * by + B, B * bx:B * bx + B]
        is_cut = bool(c > 0 and D > c * c)
        if is_cut:
            return x.copy(), 1, D, v, {}
        g = s * np.exp(-m / (2.0 * sigma * sigma))
        return _blend(x, yw, g), 0, D, v, dict(m=m, g=g, lw=lw)
    y, cut, D, g = T.frame(x, l, yw, lw, True, p)
    extras = {}
    if g is not None:
        d = l.astype(np.float64) - lw.astype(np.float64)
        extras = dict(m=T.window_mean(d * d, int(p["radius"])), g=g, lw=lw)
    return y, cut, D, v, extras


class Sim(object):
    """A handle's sequence state and its calls, by ``frame``; ``mutant`` breaks it in one way.  The interface ``play`` drives: set / motion /
    reset / apply / state, as HipColorizer's set_temporal_filter / set_temporal_motion / temporal_reset / temporal_apply + temporal_vectors(-1) /
    temporal_state."""

    def __init__(self, H, W, mutant=None):
        self.H, self.W, self.mutant = H, W, mutant
        self.p, self.mp = dict(T.DEFAULT), dict(DEFAULT)
        self.reset()

    def set(self, **p):
        self.p = dict(p)

    def motion(self, **mp):
        self.mp = dict(mp)

    def reset(self):
        self.y_prev, self.l_prev, self.have = np.zeros((2, self.H, self.W), np.float32), np.zeros((self.H, self.W), np.float32), False
        self.v_last = None

    def state(self):
        return self.y_prev.copy(), self.l_prev.copy(), self.have

    def apply(self, ab, l):
        mu = self.mutant
        ab, l = np.asarray(ab, np.float32), np.asarray(l, np.float32)
        n = ab.shape[0]
        if mu == "swap_hw":              # every plane read as [W,H]
            t = Sim(self.W, self.H)
            t.p, t.mp = self.p, self.mp
            t.y_prev, t.l_prev, t.have = self.y_prev.reshape(2, self.W, self.H), self.l_prev.reshape(self.W, self.H), self.have
            y, cut, D, v = t.apply(ab.reshape(n, 2, self.W, self.H), l.reshape(n, self.W, self.H))
            self.y_prev, self.l_prev, self.have = t.y_prev.reshape(2, self.H, self.W), t.l_prev.reshape(self.H, self.W), True
            return y.reshape(ab.shape), cut, D, v.reshape(n, self.H // B, self.W // B, 2)
        y, cut, D = np.empty_like(ab), np.zeros(n, np.int32), np.zeros(n, np.float64)
        v = np.zeros((n, self.H // B, self.W // B, 2), np.int8)
        yp, lp, have = self.y_prev, self.l_prev, self.have
        for f in range(n):
            fm = mu
            if mu == "state_early" and n != 1:
                fm = None
            y[f], cut[f], D[f], v[f], ex = frame(ab[f], l[f], yp, lp, have, self.p, self.mp, fm, self.v_last)
            self.v_last = v[f]
            yp = y[f]
            lp = ex["lw"] if (mu == "lprev_warped" and "lw" in ex) else l[f]
            have = True
        self.y_prev, self.l_prev, self.have = np.array(yp, np.float32), np.array(lp, np.float32), True
        return y, cut, D, v


# ------------------------------------------------------------------------------------------------ comparisons
def verify_call(before, ab, l, p, mp, y, cut, D, v, what="", non_tie=None):
    """One call's results against ``frame`` per frame from the device's own previous output.  The vectors EXACTLY (J has the same bits in every
    implementation, so this needs no margin); y, the flags and D at the temporal file's bar.  ``non_tie``: a mask [H/8,W/8] of the blocks on
    which the case goes on to claim a particular vector: there the best candidate must be MARGIN_REL clear of the second."""
    yp, lp, have = before
    c = float(p["cut"])
    for f in range(ab.shape[0]):
        wy, wc, wD, wv, _ = frame(ab[f], l[f], yp, lp, have, p, mp)
        tag = "%s frame %d" % (what, f)
        assert np.array_equal(np.asarray(v[f], np.int8), wv), "%s: %d of %d vectors differ from the rule, e.g. block %s: %s, the rule says %s" % (
            tag, int((np.asarray(v[f]) != wv).any(-1).sum()), wv.shape[0] * wv.shape[1],
            tuple(np.argwhere((np.asarray(v[f]) != wv).any(-1))[0]), np.asarray(v[f])[tuple(np.argwhere((np.asarray(v[f]) != wv).any(-1))[0])].tolist(),
            wv[tuple(np.argwhere((np.asarray(v[f]) != wv).any(-1))[0])].tolist())
        if have and non_tie is not None and non_tie.any():
            worst = float(margins(l[f], lp, int(mp["search"]), float(mp["penalty"]))[non_tie].min())
            assert worst >= MARGIN_REL, "%s: the best candidate is only %.3g (relative) clear of the second: a bad input" % (tag, worst)
        if have and c > 0:
            assert abs(wD - c * c) > T.CUT_MARGIN * c * c, "%s: D %.17g sits on the cut threshold: a bad input" % (tag, wD)
        assert int(cut[f]) == wc, "%s: cut %d, the rule says %d (D %.6g)" % (tag, int(cut[f]), wc, wD)
        assert abs(float(D[f]) - wD) <= T.D_REL * abs(wD), "%s: D %.17g, the rule says %.17g" % (tag, float(D[f]), wD)
        if wc:
            assert np.array_equal(np.asarray(y[f]).view(np.uint32), np.asarray(ab[f], np.float32).view(np.uint32)), "%s: a passed frame is not x bit for bit" % tag
        within, share = T.ulp_check(y[f], wy)
        assert within, "%s: a value further than one float32 ulp from the rule (max |diff| %.3g)" % (tag, float(np.abs(y[f].astype(np.float64) - wy).max()))
        assert share >= T.BIT_EQUAL_SHARE, "%s: only %.5f of the values are bit-equal" % (tag, share)
        yp, lp, have = y[f], l[f], True


# ------------------------------------------------------------------------------------------------ inputs
def texture(rs, H, W):
    """White noise in -50..50: every displacement but the true one costs about 1700, so no two candidates come close."""
    return rs.uniform(-50.0, 50.0, (H, W))


def pan(H, W, n, seed, step):
    """n frames of a window that moves by ``step`` = (my, mx) pixels a frame over one large texture (so the CONTENT moves by -step and the
    rule's vector, which points at where a block came from, is +step) -> (ab, l)."""
    rs = np.random.RandomState(seed)
    my, mx = step
    canvas = texture(rs, H + (n - 1) * abs(my), W + (n - 1) * abs(mx))
    oy, ox = (0 if my >= 0 else (n - 1) * -my), (0 if mx >= 0 else (n - 1) * -mx)
    l = np.stack([canvas[oy + f * my:oy + f * my + H, ox + f * mx:ox + f * mx + W] for f in range(n)]).astype(np.float32)
    ab = rs.uniform(-80.0, 80.0, (n, 2, H, W)).astype(np.float32)
    return ab, l


def moving_object(H, W, n, seed, size, start, step, attached=None):
    """A textured size x size object moving ``step`` pixels a frame from ``start`` over a static textured background -> (ab, l, positions).
    ``attached`` = (A_bg, B_bg, A_obj, B_obj): ab maps that sit on the content and toggle between A (even frames) and B (odd frames);
    None: random ab maps."""
    rs = np.random.RandomState(seed)
    bg, obj = texture(rs, H, W), texture(rs, size, size)
    l = np.empty((n, H, W), np.float32)
    ab = rs.uniform(-80.0, 80.0, (n, 2, H, W)).astype(np.float32)
    pos = []
    for f in range(n):
        y0, x0 = start[0] + f * step[0], start[1] + f * step[1]
        assert 0 <= y0 and y0 + size <= H and 0 <= x0 and x0 + size <= W
        plane = bg.copy()
        plane[y0:y0 + size, x0:x0 + size] = obj
        l[f] = plane.astype(np.float32)
        pos.append((y0, x0))
        if attached is not None:
            a = np.array(attached[f % 2], np.float32)
            a[:, y0:y0 + size, x0:x0 + size] = attached[2 + f % 2]
            ab[f] = a
    return ab, l, pos


def columns(H, W, n, seed, shift, period=None):
    """Planes that vary along x only, the content moving ``shift`` columns a frame: every dy ties.  ``period``: the texture repeats with it."""
    rs = np.random.RandomState(seed)
    width = W + n * abs(shift)
    row = rs.uniform(-50.0, 50.0, period)[np.arange(width) % period] if period else rs.uniform(-50.0, 50.0, width)
    ox = 0 if shift <= 0 else n * shift
    l = np.stack([np.broadcast_to(row[ox - f * shift:ox - f * shift + W], (H, W)) for f in range(n)]).astype(np.float32)
    ab = rs.uniform(-80.0, 80.0, (n, 2, H, W)).astype(np.float32)
    return ab, l


def scenario(H, W, max_batch=MAX_BATCH):
    """The calls of the GPU file's first case on an H x W net, as steps ("reset",) | ("set", filter params) | ("motion", motion params) |
    ("call", ab, l, check, note); check is None, "zeros" (every vector is (0, 0)), "plain" (y is the plain filter's bit for bit), "period4",
    or a (dy, dx) that every block for which that candidate is valid must report (there the non-tie margin is asserted too)."""
    seed = 1000 * H + W
    p, mp = dict(T.DEFAULT), dict(DEFAULT)
    steps = [("reset",), ("set", dict(p)), ("motion", dict(mp))]
    ab, l = T.frames(H, W, 1, seed + 1)
    steps.append(("call", ab, l, "zeros", "the first frame ever"))
    ab, l = T.frames(H, W, 1, seed + 2)
    steps.append(("call", ab, l, None, "grain, n = 1: the state is the only predecessor"))
    ab, l = T.frames(H, W, 5, seed + 3, cuts=(2,))
    steps.append(("call", ab, l, None, "grain, n = 5, a cut in the middle"))
    ab, l = T.frames(H, W, max_batch, seed + 4, cuts=(0, max_batch - 1))
    steps.append(("call", ab, l, None, "grain, n = max_batch, cuts at frame 0 and at the last frame"))
    # whole-plane pans at every search: the corners, the axes, and one step out of range
    steps.append(("set", dict(p, cut=0.0)))
    for S in range(8):
        steps.append(("motion", dict(mp, search=S)))
        dirs = [(S, S), (-S, -S), (S, -S), (-S, S), (0, S), (0, -S), (S, 0), (-S, 0)] if S in (1, 4, 7) else [(S, -S), (0, S)]
        for k, step in enumerate(dirs):
            ab, l = pan(H, W, 2, seed + 100 + 10 * S + k, step)
            steps.append(("reset",))
            steps.append(("call", ab, l, tuple(step) if S else "zeros", "search %d, a pan by %s" % (S, step)))
        ab, l = pan(H, W, 2, seed + 190 + S, (0, S + 1))
        steps.append(("reset",))
        steps.append(("call", ab, l, None, "search %d, a pan by %d columns: out of range" % (S, S + 1)))
    steps.append(("motion", dict(mp)))
    # a moving object (n = 1 calls after the first: the state is read at displaced pixels and must not be written early)
    if H >= 40:
        ab, l, _ = moving_object(H, W, 6, seed + 30, 24, (4, 6), (1, 2))
        steps.append(("reset",))
        steps.append(("call", ab[:3], l[:3], None, "a moving object, n = 3"))
        for f in range(3, 6):
            steps.append(("call", ab[f:f + 1], l[f:f + 1], None, "a moving object, n = 1, frame %d" % f))
    ab, l = pan(H, W, 4, seed + 31, (-1 if H > 8 else 0, -2))
    steps.append(("reset",))
    steps.append(("call", ab[:1], l[:1], "zeros", "a pan frame by frame: frame 0"))
    for f in range(1, 4):
        steps.append(("call", ab[f:f + 1], l[f:f + 1], (-1 if H > 8 else 0, -2), "a pan frame by frame, n = 1, frame %d" % f))
    # the penalty: none, and one no match can pay
    steps.append(("set", dict(p)))
    ab, l = T.frames(H, W, 3, seed + 40)
    steps.append(("motion", dict(mp, penalty=0.0)))
    steps.append(("call", ab, l, None, "grain at penalty 0"))
    ab, l = T.frames(H, W, 3, seed + 41)
    steps.append(("motion", dict(mp, penalty=1e6)))
    steps.append(("call", ab, l, "zeros", "grain at penalty 1e6"))
    steps.append(("motion", dict(mp)))
    ab, l = T.frames(H, W, 3, seed + 42, still=l[-1])
    steps.append(("call", ab, l, "plain", "identical planes"))
    # exact ties
    steps.append(("set", dict(p, cut=0.0)))
    ab, l = T.frames(H, W, 3, seed + 43, still=np.full((H, W), 7.5, np.float32))
    steps.append(("reset",))
    steps.append(("motion", dict(mp, penalty=0.0)))
    steps.append(("call", ab, l, "zeros", "a flat plane at penalty 0: every candidate ties"))
    ab, l = columns(H, W, 3, seed + 44, 2)
    steps.append(("reset",))
    steps.append(("call", ab, l, None, "a column texture moving sideways at penalty 0: every dy ties"))
    ab, l = columns(H, W, 2, seed + 45, 2, period=4)
    steps.append(("reset",))
    steps.append(("call", ab, l, "period4", "a period-4 column texture shifted by 2 at penalty 0"))
    steps.append(("motion", dict(mp)))
    steps.append(("reset",))
    steps.append(("set", dict(p)))
    ab, l = T.frames(H, W, 2, seed + 46)
    steps.append(("call", ab, l, None, "after a reset: frame 0 passes"))
    return steps


def play(backend, H, W, max_batch=MAX_BATCH):
    """Run ``scenario`` on ``backend`` (a ``Sim``, or the GPU file's adapter of an engine) and check every call; -> the number of frames checked."""
    p, mp, checked = dict(T.DEFAULT), dict(DEFAULT), 0
    for step in scenario(H, W, max_batch):
        if step[0] == "reset":
            backend.reset()
            assert not backend.state()[2]
            continue
        if step[0] == "set":
            p = dict(step[1])
            backend.set(**p)
            continue
        if step[0] == "motion":
            mp = dict(step[1])
            backend.motion(**mp)
            continue
        _, ab, l, check, note = step
        before = backend.state()
        y, cut, D, v = backend.apply(ab, l)
        what = "%dx%d, %s:" % (H, W, note)
        mask = None
        if isinstance(check, tuple):
            mask = np.array([[valid(by, bx, check[0], check[1], H, W) for bx in range(W // B)] for by in range(H // B)])
        verify_call(before, ab, l, p, mp, y, cut, D, v, what, non_tie=mask)
        after = backend.state()
        assert after[2] and np.array_equal(after[0].view(np.uint32), y[-1].view(np.uint32)) and np.array_equal(after[1], l[-1]), what + " the state afterwards"
        v = np.asarray(v)
        n = ab.shape[0]
        first = 0 if before[2] else 1            # frames with a predecessor
        if not before[2]:
            assert not v[0].any(), what + " no predecessor: the vectors are reported as zeros"
        if check == "zeros":
            assert not v.any(), what + " a vector that is not (0, 0)"
        if isinstance(check, tuple):
            hit = 0
            for by in range(H // B):
                for bx in range(W // B):
                    if valid(by, bx, check[0], check[1], H, W):
                        assert (v[first:, by, bx] == np.array(check, np.int8)).all(), what + " block (%d, %d) reports %s" % (by, bx, v[first:, by, bx].tolist())
                        hit += 1
            assert hit > 0 or H == 8 or W == 8, what + " no block can see the pan"
        if check == "plain":
            assert not v.any() and (np.asarray(D) == 0).all() and not np.asarray(cut).any(), what + " v, D or cut"
            yp = before[0]
            for f in range(n):
                want = T.frame(ab[f], l[f], yp, l[f], True, p)[0]
                assert np.array_equal(y[f].view(np.uint32), want.view(np.uint32)), what + " y is not the plain filter's"
                yp = y[f]
        if check == "period4":
            S = int(mp["search"])
            for by in range(H // B):
                for bx in range(W // B):
                    want = (0, -2) if valid(by, bx, 0, -2, H, W) else (0, 2) if valid(by, bx, 0, 2, H, W) else None
                    if S >= 2 and want is not None:
                        assert v[first:, by, bx].tolist() == [list(want)] * (n - first), what + " block (%d, %d) reports %s" % (by, bx, v[first:, by, bx].tolist())
        if note.startswith("a column texture"):
            assert not v[..., 0].any(), what + " a dy that is not 0"
            assert W == 8 or v[first:, :, 1:-1, 1].any(), what + " no dx at all"
        checked += n
    return checked


# ------------------------------------------------------------------------------------------------ the claim
CLAIM = dict(H=64, W=64, n=12, size=32, start=(8, 8), step=(1, 2), seed=5, s=0.6)


def claim_inputs():
    """The issue's sequence: a 32 x 32 textured object moving (1, 2) pixels a frame over a static textured background, 12 frames, the colours
    attached to the content and toggled on alternate frames -> (ab, l, positions, (A_bg, B_bg, A_obj, B_obj))."""
    c = CLAIM
    rs = np.random.RandomState(c["seed"] + 1)
    fields = (rs.uniform(-80, 80, (2, c["H"], c["W"])).astype(np.float32), rs.uniform(-80, 80, (2, c["H"], c["W"])).astype(np.float32),
              rs.uniform(-80, 80, (2, c["size"], c["size"])).astype(np.float32), rs.uniform(-80, 80, (2, c["size"], c["size"])).astype(np.float32))
    ab, l, pos = moving_object(c["H"], c["W"], c["n"], c["seed"], c["size"], c["start"], c["step"], attached=fields)
    return ab, l, pos, fields


def claim_set(l, pos, p, mp):
    """The object's pixels, in object coordinates [size,size], whose chain kept the true vector -step and m == 0 in every frame 1 .. n-1."""
    c = CLAIM
    size, true = c["size"], np.array([-c["step"][0], -c["step"][1]], np.int8)
    keep = np.ones((size, size), bool)
    for f in range(1, l.shape[0]):
        v = vectors(l[f], l[f - 1], int(mp["search"]), float(mp["penalty"]))
        d = l[f].astype(np.float64) - warp(l[f - 1], v).astype(np.float64)
        m = T.window_mean(d * d, int(p["radius"]))
        right = np.repeat(np.repeat((v == true).all(-1), B, 0), B, 1)
        y0, x0 = pos[f]
        keep &= (right & (m == 0))[y0:y0 + size, x0:x0 + size]
    return keep
