"""The hint tracking along the motion vectors (include/ideepcolor.h, "HINT TRACKING") restated, the inputs of tests/test_track_gpu.py, and the
conditions and mutants tests/test_track_cpu.py holds them to.

``frame_loops`` is the rule word for word: the RECURSION, one frame from the previous frame's tracked planes, in plain loops.  ``frame`` is its
whole-plane numpy twin, held bit-equal to it on every input (tests/test_track_cpu.py); with ``mutant`` set it breaks the rule in one named way.
``walk`` is the OTHER formulation, the one the kernel uses -- an independent walk back per (frame, pixel) over the raw planes -- kept here only to
show on the host that it is the same function, and to carry the one mutant that exists in that form alone.  The vectors are tests/motion_ref.py's.

``Sim`` plays a handle: the sequence state, ``call`` (a pipelined call), ``apply`` (idc_track_hints_apply: a self-contained sequence)."""
import numpy as np

import motion_ref as M

B = 8
DEFAULT = dict(life=0, tol=8.0)
NETS = M.NETS
MAX_BATCH = M.MAX_BATCH
TOL_MARGIN_REL = 1e-6            # every |dl| the rule compares is EXACTLY tol (float64 of float32 values: the same in every implementation) or this far from it
MUTANTS = ["warp_minus", "tol_uncompensated", "lt_for_le", "life_off_by_one", "age_not_incremented", "carried_over_own", "raw_prev_only",
           "p_block_chain", "state_not_carried", "state_early", "swap_hw"]
FRAME_MUTANTS = MUTANTS[:7] + ["swap_hw"]


class Prev(object):
    """What a frame sees of its predecessor: the tracked planes A [2,H,W], M [H,W] float32, G [H,W] int32, its L plane, and (for one mutant)
    its raw own planes."""

    def __init__(self, A, Mk, G, l, own_ab=None, own_mask=None):
        self.A, self.M, self.G, self.l = np.asarray(A, np.float32), np.asarray(Mk, np.float32), np.asarray(G, np.int32), np.asarray(l, np.float32)
        self.own_ab, self.own_mask = own_ab, own_mask


# ------------------------------------------------------------------------------------------------ the rule
def frame_loops(ab, mask, l, prev, v, life, tol):
    """ONE frame of the recursion in plain loops -> (A [2,H,W] float32, M [H,W] float32, G [H,W] int32).  prev: a ``Prev`` or None."""
    ab, mask, l = np.asarray(ab, np.float32), np.asarray(mask, np.float32), np.asarray(l, np.float32)
    H, W = mask.shape
    A, Mk, G = np.zeros((2, H, W), np.float32), np.zeros((H, W), np.float32), np.zeros((H, W), np.int32)
    own = (mask != 0).tolist()
    if prev is not None:
        pM, pG = (prev.M != 0).tolist(), prev.G.tolist()
        vv = np.asarray(v).tolist()
        lf, lp = l.astype(np.float64).tolist(), prev.l.astype(np.float64).tolist()
    tol = float(tol)
    for y in range(H):
        for x in range(W):
            if own[y][x]:                                # an own hint always wins
                A[:, y, x], Mk[y, x] = ab[:, y, x], mask[y, x]
                continue
            if prev is None:
                continue
            dy, dx = vv[y // B][x // B]
            qy, qx = y + dy, x + dx
            assert 0 <= qy < H and 0 <= qx < W          # a valid vector keeps its whole block inside
            if not pM[qy][qx]:
                continue
            if not (abs(lf[y][x] - lp[qy][qx]) <= tol):  # a NaN carries nothing
                continue
            if not (life == 0 or pG[qy][qx] + 1 <= life):
                continue
            A[:, y, x], Mk[y, x], G[y, x] = prev.A[:, qy, qx], prev.M[qy, qx], pG[qy][qx] + 1
    return A, Mk, G


def _pixel_vectors(v, H, W):
    v = np.asarray(v)
    return np.repeat(np.repeat(v[..., 0].astype(np.int64), B, 0), B, 1), np.repeat(np.repeat(v[..., 1].astype(np.int64), B, 0), B, 1)


def frame(ab, mask, l, prev, v, life, tol, mutant=None):
    """``frame_loops`` on whole planes.  Mutants of FRAME_MUTANTS break it."""
    assert mutant is None or mutant in FRAME_MUTANTS + ["swap_hw_inner"]
    ab, mask, l = np.asarray(ab, np.float32), np.asarray(mask, np.float32), np.asarray(l, np.float32)
    H, W = mask.shape
    if mutant == "swap_hw" and H != W:                   # the rule for a (W, H) net on the same memory
        if prev is not None:
            prev = Prev(prev.A.reshape(2, W, H), prev.M.reshape(W, H), prev.G.reshape(W, H), prev.l.reshape(W, H))
            v = np.asarray(v).reshape(W // B, H // B, 2)
        A, Mk, G = frame(ab.reshape(2, W, H), mask.reshape(W, H), l.reshape(W, H), prev, v, life, tol, "swap_hw_inner")
        return A.reshape(2, H, W), Mk.reshape(H, W), G.reshape(H, W)
    own = mask != 0
    A, Mk, G = np.where(own[None], ab, np.float32(0)), np.where(own, mask, np.float32(0)), np.zeros((H, W), np.int32)
    if prev is None:
        return A, Mk, G
    vy, vx = _pixel_vectors(v, H, W)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sign = -1 if mutant == "warp_minus" else 1
    qy, qx = np.clip(jj + sign * vy, 0, H - 1), np.clip(ii + sign * vx, 0, W - 1)        # (the clamp only ever acts in a mutant)
    pA, pM, pG = prev.A, prev.M, prev.G
    if mutant == "raw_prev_only":                        # carried from the RAW own planes of f - 1: a hint lives one frame
        pA, pM, pG = np.asarray(prev.own_ab, np.float32), np.asarray(prev.own_mask, np.float32), np.zeros((H, W), np.int32)
    lp = prev.l if mutant == "tol_uncompensated" else prev.l[qy, qx]
    with np.errstate(invalid="ignore"):
        d = np.abs(l.astype(np.float64) - lp.astype(np.float64))
        near = (d < np.float64(tol)) if mutant == "lt_for_le" else (d <= np.float64(tol))
    g1 = pG[qy, qx].astype(np.int64) + 1
    alive = np.ones((H, W), bool) if life == 0 else ((g1 - 1 <= life) if mutant == "life_off_by_one" else (g1 <= life))
    carried = (pM[qy, qx] != 0) & near & alive
    take = carried if mutant == "carried_over_own" else carried & ~own
    A = np.where(take[None], pA[:, qy, qx], A)
    Mk = np.where(take, pM[qy, qx], Mk)
    G = np.where(take, g1 - 1 if mutant == "age_not_incremented" else g1, G).astype(np.int32)
    return A.astype(np.float32), Mk.astype(np.float32), G


def walk(ab, mask, l, v, state, life, tol, mutant=None):
    """The kernel's formulation on a whole call: for every (f, p) walk back over the RAW planes ab [n,2,H,W], mask [n,H,W], l [n,H,W] along
    v [n,H/8,W/8,2] until an own hint, a failed test or the call's start, where ``state`` (a ``Prev`` or None; its l is l_prev) is read.
    ``mutant='p_block_chain'``: every step of the chain takes the vector of p's block instead of the block it has reached."""
    assert mutant in (None, "p_block_chain")
    ab, mask, l = np.asarray(ab, np.float32), np.asarray(mask, np.float32), np.asarray(l, np.float32)
    n, H, W = mask.shape
    A, Mk, G = np.zeros((n, 2, H, W), np.float32), np.zeros((n, H, W), np.float32), np.zeros((n, H, W), np.int32)
    have_state = state is not None and state.M is not None
    for f in range(n):
        py, px = [a.ravel() for a in np.meshgrid(np.arange(H), np.arange(W), indexing="ij")]
        qy, qx = py.copy(), px.copy()
        alive = np.ones(H * W, bool)
        steps = 0
        for g in range(f, -1, -1):
            hit = alive & (mask[g, qy, qx] != 0)
            A[f][:, py[hit], px[hit]] = ab[g][:, qy[hit], qx[hit]]
            Mk[f, py[hit], px[hit]] = mask[g, qy[hit], qx[hit]]
            G[f, py[hit], px[hit]] = steps
            alive &= ~hit
            if g == 0 and not have_state:
                break
            by, bx = (py if mutant else qy) // B, (px if mutant else qx) // B
            ny, nx = np.clip(qy + v[g, by, bx, 0], 0, H - 1), np.clip(qx + v[g, by, bx, 1], 0, W - 1)
            lp = l[g - 1] if g > 0 else state.l
            with np.errstate(invalid="ignore"):
                alive &= np.abs(l[g, qy, qx].astype(np.float64) - lp[ny, nx].astype(np.float64)) <= np.float64(tol)
            steps += 1
            if life and steps > life:
                break
            qy, qx = ny, nx
            if g == 0:
                age = state.G[qy, qx].astype(np.int64) + steps
                hit = alive & (state.M[qy, qx] != 0) & ((age <= life) if life else True)
                A[f][:, py[hit], px[hit]] = state.A[:, qy[hit], qx[hit]]
                Mk[f, py[hit], px[hit]] = state.M[qy[hit], qx[hit]]
                G[f, py[hit], px[hit]] = age[hit]
    return A, Mk, G


def call_vectors(l, l_prev, mp):
    """The motion rule's vectors of a call's frames [n,H/8,W/8,2]: zeros for a frame 0 without a predecessor."""
    l = np.asarray(l, np.float32)
    n, H, W = l.shape
    v = np.zeros((n, H // B, W // B, 2), np.int8)
    for f in range(n):
        lp = l[f - 1] if f else l_prev
        if lp is not None:
            v[f] = M.vectors(l[f], lp, int(mp["search"]), float(mp["penalty"]))
    return v


def sequence(l, ab, mask, v, state, life, tol, rule=frame_loops, mutant=None):
    """The recursion over one call from ``state`` (a ``Prev`` whose M may be None: a predecessor without tracked planes; or None) ->
    (A [n,2,H,W], M [n,H,W], G [n,H,W])."""
    n, H, W = np.asarray(mask).shape
    prev = state
    if prev is not None and prev.M is None:
        prev = Prev(np.zeros((2, H, W)), np.zeros((H, W)), np.zeros((H, W)), prev.l, np.zeros((2, H, W)), np.zeros((H, W)))
    out = []
    for f in range(n):
        t = rule(ab[f], mask[f], l[f], prev, v[f], life, tol) if mutant is None else frame(ab[f], mask[f], l[f], prev, v[f], life, tol, mutant)
        out.append(t)
        prev = Prev(t[0], t[1], t[2], l[f], ab[f], mask[f])
    return np.stack([t[0] for t in out]), np.stack([t[1] for t in out]), np.stack([t[2] for t in out])


class _NoTrack(object):
    """A predecessor whose tracked planes were dropped (or never written): l_prev alone."""
    M = None

    def __init__(self, l):
        self.l = np.asarray(l, np.float32)


class Sim(object):
    """A handle: the motion and tracking parameters and the sequence state."""

    def __init__(self, mutant=None, rule=frame):
        assert mutant is None or mutant in MUTANTS
        self.mutant, self.rule = mutant, rule
        self.mp, self.tp = dict(M.DEFAULT), dict(DEFAULT)
        self.state = None

    def motion(self, **mp):
        self.mp = dict(mp)

    def set(self, **tp):
        self.tp = dict(tp)

    def reset(self):
        self.state = None

    def untracked(self, l):
        """A filtered call without tracking (or with motion off): the sequence moves on, the tracked planes are dropped."""
        self.state = _NoTrack(np.asarray(l, np.float32)[-1])

    def call(self, l, ab, mask):
        """A pipelined tracking call -> (A, M, G, v); the state advances."""
        l, ab, mask = np.asarray(l, np.float32), np.asarray(ab, np.float32), np.asarray(mask, np.float32)
        state = self.state
        v = call_vectors(l, None if state is None else state.l, self.mp)
        if state is not None and self.mutant == "state_not_carried":
            state = _NoTrack(state.l)
        if state is not None and state.M is not None and self.mutant == "state_early" and l.shape[0] == 1:
            own = mask[0] != 0                           # the state already holds this call's last frame when frame 0 reads it
            state = Prev(np.where(own[None], ab[0], 0), np.where(own, mask[0], 0), np.zeros(mask[0].shape), state.l, ab[0], mask[0])
        life, tol = int(self.tp["life"]), float(self.tp["tol"])
        if self.mutant == "p_block_chain":
            A, Mk, G = walk(ab, mask, l, v, state, life, tol, "p_block_chain")
        elif self.mutant in FRAME_MUTANTS:
            A, Mk, G = sequence(l, ab, mask, v, state, life, tol, mutant=self.mutant)
        else:
            A, Mk, G = sequence(l, ab, mask, v, state, life, tol, rule=self.rule)
        self.state = Prev(A[-1], Mk[-1], G[-1], l[-1], ab[-1], mask[-1])
        return A, Mk, G, v

    def apply(self, l, ab, mask):
        """idc_track_hints_apply: a self-contained sequence with this handle's parameters; its state is neither read nor written."""
        other = Sim(self.mutant, self.rule)
        other.mp, other.tp = dict(self.mp), dict(self.tp)
        return other.call(l, ab, mask)


# ------------------------------------------------------------------------------------------------ conditions on an input
def tol_margin(l, l_prev, v, tol):
    """The smallest relative distance from ``tol`` of any |dl| the rule can compare in this call (the exact ties apart), and their count."""
    l = np.asarray(l, np.float32)
    worst, ties = np.inf, 0
    for f in range(l.shape[0]):
        lp = l[f - 1] if f else l_prev
        if lp is None:
            continue
        d = np.abs(l[f].astype(np.float64) - M.warp(np.asarray(lp, np.float32), v[f]).astype(np.float64))
        d = d[np.isfinite(d)]
        ties += int((d == tol).sum())
        rest = d[d != tol]
        if rest.size and tol > 0:
            worst = min(worst, float(np.abs(rest - tol).min() / tol))
    return worst, ties


# ------------------------------------------------------------------------------------------------ inputs
def hint_planes(n, H, W, hints):
    """hints: {frame: [(y0, x0, y1, x1, a, b, mask_value)]}, inclusive rectangles clipped to the plane, later over earlier -> (ab, mask)."""
    ab, mask = np.zeros((n, 2, H, W), np.float32), np.zeros((n, H, W), np.float32)
    for f, rects in hints.items():
        for (y0, x0, y1, x1, a, b, m) in rects:
            y0, x0, y1, x1 = max(y0, 0), max(x0, 0), min(y1, H - 1), min(x1, W - 1)
            if y0 > y1 or x0 > x1:
                continue
            ab[f, 0, y0:y1 + 1, x0:x1 + 1], ab[f, 1, y0:y1 + 1, x0:x1 + 1], mask[f, y0:y1 + 1, x0:x1 + 1] = a, b, m
    return ab, mask


def _case(name, l, hints, mp=None, tp=None, **more):
    n, H, W = l.shape
    ab, mask = hint_planes(n, H, W, hints)
    return dict(name=name, l=np.ascontiguousarray(l, np.float32), ab=ab, mask=mask, mp=dict(mp or M.DEFAULT), tp=dict(tp or DEFAULT), **more)


def centre_rect(H, W, a=30.0, b=-20.0, m=1.0):
    """A rectangle of up to 6 x 10 pixels about the plane's centre that straddles blocks."""
    cy, cx = H // 2, W // 2
    return (max(cy - 3, 0), max(cx - 5, 0), min(cy + 2, H - 1), min(cx + 4, W - 1), a, b, m)


def pan_steps():
    """(search, step) of the whole-plane pans: (+-S, +-S), (0, +-S), (+-S, 0) at every search 0..7 (at 0 they are one: no pan)."""
    out = []
    for S in range(8):
        dirs = [(S, S), (-S, -S), (S, -S), (-S, S), (0, S), (0, -S), (S, 0), (-S, 0)] if S else [(0, 0)]
        out += [(S, d) for d in dirs]
    return out


def cases(H, W, max_batch=MAX_BATCH):
    """The inputs of the GPU file's rule-alone case on an H x W net: dicts of name, l, ab, mask, mp (motion), tp (tracking) and, where a closed
    form is asserted beside the bit-for-bit comparison, ``pan`` = (step, rectangle) or ``object`` = (positions, size, rectangle)."""
    seed = 7000 * H + W
    rs = np.random.RandomState(seed)
    out = []
    rect = centre_rect(H, W)
    # hold plus tol: a still texture; from frame 2 on the right half of the plane steps by more than tol and back
    base = M.texture(rs, H, W)
    step = np.zeros((H, W))
    step[:, W // 2:] = 13.0
    l = np.stack([base, base, base + step, base + step, base]).astype(np.float32)
    out.append(_case("a step in L larger than tol under half of a hint", l, {0: [rect]}))
    # the tol test exactly at tol: integer planes, a step of exactly 8
    base = np.round(M.texture(rs, H, W))
    step[:, W // 2:] = 8.0
    step[:, W // 2 + 2:] = 9.0
    l = np.stack([base, base + step, base + step]).astype(np.float32)
    out.append(_case("steps of exactly tol and of tol + 1", l, {0: [rect]}, mp=dict(search=0, penalty=0.5), ties=True))
    # whole-plane pans: the rectangle moves by exactly the pan until it leaves the plane
    for k, (S, d) in enumerate(pan_steps()):
        n = 4 if S in (1, 7) else 3
        l = M.pan(H, W, n, seed + 100 + k, d)[1]
        out.append(_case("search %d, a pan by %s" % (S, d), l, {0: [rect]}, mp=dict(search=S, penalty=0.5), pan=(d, rect)))
    # an own hint over a carried one, another mask_value: the pan brings the first rectangle under the second
    d = (0, 2)
    l = M.pan(H, W, 5, seed + 200, d)[1]
    second = (rect[0] + 1, rect[1] - 2 * d[1] - 3, rect[2] - 1, rect[3] - 2 * d[1] - 3, -40.0, 55.0, 0.5)
    out.append(_case("an own hint over a carried one", l, {0: [rect], 2: [second]}, own_over=(2, second)))
    # life: 1, 3 and n - 1 on a pan of n frames, and none over max_batch frames
    d = (0, -1)
    l = M.pan(H, W, max_batch, seed + 210, d)[1]
    for life in (1, 3, 5):
        out.append(_case("life %d of 6 frames" % life, l[:6], {0: [rect]}, tp=dict(life=life, tol=8.0), life=life))
    out.append(_case("life 0 over max_batch frames", l, {0: [rect]}, life=0))
    # a cut carries nothing; a NaN in L carries nothing
    l = M.pan(H, W, 4, seed + 220, (0, 1))[1]
    l[2:] = M.pan(H, W, 2, seed + 221, (0, 1))[1] + np.float32(150.0)       # another scene, and no pixel of it within tol of any of the first
    out.append(_case("a cut", l, {0: [rect]}, cut=2))
    l = M.pan(H, W, 4, seed + 230, (0, 0))[1]
    l[2, rect[0]:rect[0] + 2, rect[1]:rect[1] + 3] = np.nan
    out.append(_case("a NaN in L", l, {0: [rect]}, mp=dict(search=0, penalty=0.5), nan=True))
    # n = 1
    out.append(_case("n = 1", M.pan(H, W, 1, seed + 240, (0, 0))[1], {0: [rect]}))
    if H >= 40:
        # a textured object moving (1, 2) over a textured background, hinted once inside; a second hint straddles its right edge: blocks
        # with different vectors
        size = 24
        _, l, pos = M.moving_object(H, W, 6, seed + 250, size, (4, 6), (1, 2))
        inside = (4 + 9, 6 + 9, 4 + 14, 6 + 16, 25.0, 35.0, 1.0)
        edge = (4 + 6, 6 + size - 5, 4 + 17, 6 + size + 8, -60.0, 10.0, 1.0)
        out.append(_case("a moving object, hinted once", l, {0: [inside]}, object=(pos, size, inside)))
        out.append(_case("a hint straddling blocks with different vectors", l, {0: [edge]}, straddle=True))
    return out


def _rect_mask(H, W, rect, dy=0, dx=0):
    m = np.zeros((H, W), bool)
    y0, x0, y1, x1 = rect[0] + dy, rect[1] + dx, rect[2] + dy, rect[3] + dx
    if y0 >= 0 and x0 >= 0 and y1 < H and x1 < W:
        m[y0:y1 + 1, x0:x1 + 1] = True
        return m
    return None                                          # it has begun to leave the plane


def _blocks_report(v, where, vec):
    """Every block that holds a pixel of ``where`` reports ``vec``."""
    blocks = where.reshape(where.shape[0] // B, B, where.shape[1] // B, B).any((1, 3))
    return bool((v[blocks] == np.array(vec, np.int8)).all())


def check_case(c, A, Mk, G, v):
    """The closed forms a case names, beside the bit-for-bit comparison -> the number of frames they were asserted on."""
    n, H, W = Mk.shape
    name, checked = c["name"], 0
    rect = next(iter(c_rects(c)), None)
    if "pan" in c or "object" in c:
        # the content moves by -step a frame (a pan: the window moves by step) or by +step (the object): the rectangle with it, for as long as
        # every block it lies in reports the true vector
        if "pan" in c:
            (sy, sx), rect, vec = c["pan"][0], c["pan"][1], c["pan"][0]
            move = (-sy, -sx)
        else:
            rect, move, vec = c["object"][2], (1, 2), (-1, -2)
        for f in range(1, n):
            at = _rect_mask(H, W, rect, f * move[0], f * move[1])
            if at is None or not _blocks_report(v[f], at, vec):
                break
            assert np.array_equal(Mk[f] != 0, at), "%s: frame %d: the hint is not the rectangle moved by %s" % (name, f, (f * move[0], f * move[1]))
            assert (G[f][at] == f).all() and (A[f][0][at] == np.float32(rect[4])).all() and (A[f][1][at] == np.float32(rect[5])).all(), name
            checked += 1
    if "own_over" in c:
        f, second = c["own_over"]
        at = _rect_mask(H, W, second)
        if at is not None:
            assert (Mk[f][at] == np.float32(0.5)).all() and (G[f][at] == 0).all() and (A[f][0][at] == np.float32(second[4])).all(), name
            rest = (Mk[f] != 0) & ~at
            if W >= 40:
                assert rest.any() and (Mk[f][rest] == np.float32(1.0)).all() and (G[f][rest] == f).all(), name + ": the carried hint beside the own one"
                assert (Mk[f + 1] == np.float32(0.5)).any(), name + ": the second call's mask_value does not travel with its hint"
            checked += 1
    if "life" in c and W >= 40 and H >= 40:
        life = c["life"]
        for f in range(n):
            assert (Mk[f] != 0).any() == (life == 0 or f <= life), "%s: frame %d" % (name, f)
        assert G.max() == (n - 1 if life == 0 else life), name
        checked += n
    if "cut" in c:
        assert (Mk[1] != 0).any() or H == 8
        assert not Mk[c["cut"]:].any() and not G[c["cut"]:].any() and not A[c["cut"]:].any(), name + ": a hint crossed the cut"
        checked += n - c["cut"]
    if "nan" in c:
        bad = np.isnan(c["l"][2])
        assert bad.any() and not Mk[2][bad].any() and not Mk[3][bad].any() and (Mk[3] != 0).any(), name
        assert np.array_equal((Mk[2] != 0) | bad, Mk[1] != 0), name
        checked += 2
    if "ties" in c:
        step = (c["l"][1].astype(np.float64) - c["l"][0].astype(np.float64))
        first = c["mask"][0] != 0
        assert np.array_equal(Mk[1] != 0, first & (np.abs(step) <= 8.0)) and (np.abs(step)[first] == 8.0).any() and (np.abs(step)[first] == 9.0).any(), name
        checked += 1
    if name.startswith("a step in L larger") and not v.any():
        first = c["mask"][0] != 0
        left = first.copy()
        left[:, W // 2:] = False
        assert np.array_equal(Mk[1] != 0, first) and np.array_equal(Mk[2] != 0, left) and np.array_equal(Mk[4] != 0, left) and left.any(), name
        assert (G[4][left] == 4).all(), name
        checked += 3
    if name == "n = 1":
        assert np.array_equal(Mk, c["mask"]) and not G.any()
        checked += 1
    return checked


def c_rects(c):
    """The first frame's hinted bounding rectangle of a case, as a one-element list (empty without a hint)."""
    ys, xs = np.nonzero(c["mask"][0])
    return [(int(ys.min()), int(xs.min()), int(ys.max()), int(xs.max()))] if ys.size else []


# ------------------------------------------------------------------------------------------------ the pipelined inputs
RECT_A, RECT_B = (20, 20, 31, 35, 40.0, -30.0), (5, 40, 12, 50, -20.0, 50.0)


def grey_pan_sources(n, H=64, W=64, step=(1, 2), seed=9):
    """n net-sized RGB crops of one image of eight grey levels (16, 48 .. 240), the window moving ``step`` pixels a frame: no resampling, so a pan
    at the net size whose L planes repeat bit for bit along the vectors.  Two L values are equal or a whole level (more than 9 L units) apart:
    no |dl| comes near tol = 8, whatever the last bits of the device's L."""
    rs = np.random.RandomState(seed)
    big = (rs.randint(0, 8, (H + n * step[0], W + n * step[1])) * 32 + 16).astype(np.uint8)
    big = np.repeat(big[..., None], 3, -1)
    return [np.ascontiguousarray(big[f * step[0]:f * step[0] + H, f * step[1]:f * step[1] + W]) for f in range(n)]


def grey_l(srcs):
    """The L planes of grey sources on the host, to about 1e-4: L = 116 cbrt(Y) - 16 of the linearised level (every level here is above the
    linear toe).  The GPU file takes the device's own planes; this serves the conditions and the mutants of tests/test_track_cpu.py."""
    g = np.stack([np.asarray(s)[..., 0] for s in srcs]).astype(np.float64) / 255.0
    lin = np.where(g > 0.04045, ((g + 0.055) / 1.055) ** 2.4, g / 12.92)
    return (116.0 * np.cbrt(lin) - 16.0).astype(np.float32)


def pipeline_inputs(n=7):
    """The split-invariance sequence of the GPU file on the host -> (l, ab, mask): hints at frames 0 and 3 only."""
    l = grey_l(grey_pan_sources(n))
    ab, mask = hint_planes(n, l.shape[1], l.shape[2], {0: [RECT_A + (1.0,)], 3: [RECT_B + (1.0,)]})
    return l, ab, mask


def play_parts(sim, l, ab, mask, parts):
    """The sequence as calls of ``parts`` frames on ``sim`` from a reset -> (A, M, G, v) of all frames."""
    sim.reset()
    out, at = [], 0
    for n in parts:
        out.append(sim.call(l[at:at + n], ab[at:at + n], mask[at:at + n]))
        at += n
    return [np.concatenate([o[k] for o in out]) for k in range(4)]


# ------------------------------------------------------------------------------------------------ the claim
CLAIM = dict(M.CLAIM, rect=(20, 20, 27, 27, 45.0, -35.0, 1.0))


def claim_inputs():
    """motion_ref's moving object (32 x 32, (1, 2) a frame, 12 frames on a 64 x 64 net), hinted at frame 0 only, 12 pixels inside the
    object's corner -> (l, ab, mask, positions)."""
    c = CLAIM
    _, l, pos = M.moving_object(c["H"], c["W"], c["n"], c["seed"], c["size"], c["start"], c["step"])
    ab, mask = hint_planes(c["n"], c["H"], c["W"], {0: [c["rect"]]})
    return l, ab, mask, pos


def claim_counts(Mk, pos):
    """Of the tracked mask [n,H,W]: (interior pixels of the moved rectangle that are hinted at the last frame, their number; pixels of the
    rectangle HELD at p0 that lie on the object at the last frame)."""
    c = CLAIM
    n, (y0, x0, y1, x1) = c["n"], c["rect"][:4]
    dy, dx = (n - 1) * c["step"][0], (n - 1) * c["step"][1]
    inner = Mk[n - 1, y0 + dy + 1:y1 + dy, x0 + dx + 1:x1 + dx]
    oy, ox = pos[n - 1]
    on_object = np.zeros(Mk.shape[1:], bool)
    on_object[oy:oy + c["size"], ox:ox + c["size"]] = True
    return int((inner != 0).sum()), inner.size, int(on_object[y0:y1 + 1, x0:x1 + 1].sum())
