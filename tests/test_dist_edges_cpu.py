"""CPU side of the crafted-head tests (tests/crafted_heads.py, tests/test_dist_edges_gpu.py): the premises of every recipe on the oracle alone,
the constants the GPU file relies on, and a mutation check of its yardsticks -- each documented tie / zero rule of the resident-distribution
kernels restated WRONG once, and shown to give another answer than the float64 restatements on at least one of the GPU file's crafted inputs;
an input that told no mutant apart would be dead weight there.

  premises    oracle/siggraph_torch.forward at 32 x 48 on tests/crafted_heads.py's images and hints: zero bins exactly 0.0 in float32, plateau
              bins bit-equal, one-hot cells exactly 1.0, the mixed recipe's plateau in front in a quarter of the cells at least and behind in a
              quarter at least (measured; the same condition is measured again on the device's distribution)
  mutants     mode decode and peaks taking the HIGHEST index of a tie; rank without its tie term; #{cmf < u}; log(p) without the FLT_MIN floor;
              numpy's NaN entropy on a zero bin; k-means++ seeding that keeps the LAST maximum; a neighbour search that skips an equal d^2
  u == 0      the committed (seed, i) whose draw is exactly 0.0: with leading zero bins it lands on the first bin with p > 0, not on bin 0
  neighbours  dist_score_ref.neighbours(by="d2"), the device's documented order, equals the sort by d wherever no two different d^2 share a root"""
import numpy as np
import pytest

import crafted_heads as C
import dist_batch_ref as D
import dist_maps_ref as M
import dist_score_ref as S
from interactive_deep_colorization_amd import color_bins
from oracle import session, siggraph_torch, weights

H, W, N_IMG = 32, 48, 3
U0_SEED, U0_I = C.U0_SEED, C.U0_I
_DIST = {}


def _base(bins, make_sd):
    if bins == 529:
        return make_sd(0, "he")
    if "sd313" not in _DIST:
        _DIST["sd313"] = weights.add_pred313_head(weights.make_state_dict(2, "he", include_class=False), 2)
    return _DIST["sd313"]


def centres_of(bins):
    return S.grid529() if bins == 529 else np.ascontiguousarray(weights.synthetic_ab_centres(2))


def _dist(bins, recipe, make_sd):
    """(Crafted, p [3,B,Hd,Wd] float32) of the oracle's forward, made once and not written to."""
    key = (bins, recipe)
    if key not in _DIST:
        c = C.craft(_base(bins, make_sd), bins, recipe)
        if "planes" not in _DIST:
            _DIST["planes"] = C.planes(H, W, N_IMG)
        L, ab, mask = _DIST["planes"]
        if bins == 529:
            p = siggraph_torch.forward(c.sd, L, ab, mask, dist=True)[1][:, :, ::4, ::4]
        else:
            p = siggraph_torch.forward(c.sd, L, ab, mask, dist313=True, return_acts=True)[2]["dist_ab_S"]
        p = np.ascontiguousarray(p, np.float32)
        p.setflags(write=False)
        _DIST[key] = (c, p)
    return _DIST[key]


INPUTS = [(bins, recipe) for bins in (529, 313) for recipe in C.RECIPES]


# ------------------------------------------------------------------------------------------------ the helper's own structure
@pytest.mark.parametrize("bins", [529, 313])
def test_the_bin_choices_straddle_the_wave_chunks(bins):
    c = C.chunk(bins)
    assert c == {529: 67, 313: 40}[bins] and 7 * c < bins <= 8 * c
    wave = lambda q: q // c
    top, lower = C.plateau_bins(bins)
    assert top == {529: [66, 67, 528], 313: [39, 40, 312]}[bins]
    assert [wave(q) for q in top] == [0, 1, 7] and len(lower) == 40 and lower[0] == 0 and {wave(q) for q in lower} == {0, 1, 2}
    top_l, lower_l = C.plateau_bins(bins, lead=True)
    assert [wave(q) for q in top_l] == [0, 0, 1, 7] and min(top_l + lower_l) == 10         # bins 0..9 lead with zeros; two top bins share wave 0
    vary, plateau = C.mixed_bins(bins)
    assert 38 <= len(vary) <= 42 and [wave(q) for q in plateau] == [0, 1, 1]
    sd = {C.HEADS[bins] + ".weight": np.ones((bins, 4, 1, 1), np.float32), C.HEADS[bins] + ".bias": np.ones(bins, np.float32), "other": 1}
    for recipe in C.RECIPES:
        k = C.craft(sd, bins, recipe)
        assert k.sd is not sd and k.sd["other"] == 1 and sd[C.HEADS[bins] + ".bias"].min() == 1            # a copy: the base is untouched
        w, b = k.sd[C.HEADS[bins] + ".weight"], k.sd[C.HEADS[bins] + ".bias"]
        assert w.dtype == np.float32 and b.dtype == np.float32 and w.shape == (bins, 4, 1, 1)
        assert (w.reshape(bins, -1) != 0).any(axis=1).tolist() == np.isin(np.arange(bins), k.vary).tolist()
        assert ((b == np.float32(C.NEG)) == k.zero).all() and (recipe != "one_hot" or 0 < k.q0 < bins - 1)
        for pl in k.plateaus:
            assert len(set(b[pl].tolist())) == 1 and not k.zero[pl].any()
            assert not (b[pl].view(np.uint32) & 0xFFFF).any()      # a plateau's bias is a bfloat16 number: the low 16 bits of the float32 are clear
    assert not (np.array([C.MIXED_BIAS[bins], C.LOWER], np.float32).view(np.uint32) & 0xFFFF).any()


# ------------------------------------------------------------------------------------------------ premises, on the oracle alone
@pytest.mark.parametrize("bins,recipe", INPUTS)
def test_premises_hold_on_the_oracle(bins, recipe, make_sd):
    c, p = _dist(bins, recipe, make_sd)
    st_all, st = C.structure(p, c), C.structure(C.interior(bins, p), c)
    print("%d %s: %d cells (%d interior), %d zero bins; zeros exact in %d, plateaus bit-equal in %d, one-hot %d, top plateau in front in %d" %
          (bins, recipe, st_all["cells"], st["cells"], st["zero_bins"], st["zeros"], st_all["ties"], st["one_hot"], st_all["top"]))
    assert st["zeros"] == st["cells"]                              # zero bins exactly 0.0 in float32, and no other bin is
    assert st_all["ties"] == st_all["cells"]                       # plateau bins bit-equal, in every cell (the 313 head's border included)
    assert st["zero_bins"] == {"uniform": 0, "one_hot": bins - 1, "plateau": bins - 43, "plateau_lead": bins - 44, "mixed": bins - 3 - len(c.vary)}[recipe]
    if recipe == "one_hot":
        assert st["one_hot"] == st["cells"] and (C.interior(bins, p)[:, c.q0] == 1.0).all()
    else:
        assert st["one_hot"] == 0
    if recipe == "mixed":
        share = st_all["top"] / float(st_all["cells"])
        assert 0.25 <= share <= 0.75, share                        # the plateau wins a quarter of the cells at least, and loses a quarter at least
        assert len(np.unique(p[:, c.vary[0]])) > st_all["cells"] // 2                                      # the random rows vary from cell to cell
    else:
        assert st_all["top"] == st_all["cells"]
        inner = C.interior(bins, p)
        assert (inner == inner[:1, :, :1, :1]).all()               # a constant recipe: one distribution in every (interior) cell


# ------------------------------------------------------------------------------------------------ the u == 0 draw
def test_the_committed_seed_draws_an_exact_zero_that_lands_on_the_first_live_bin(make_sd):
    x = (U0_I * 0x9E3779B9 + U0_SEED * 0x85EBCA6B + 0x165667B1) & 0xFFFFFFFF
    assert int(session.lowbias32(x)) >> 8 == 0                     # one hash evaluation
    u = session.draws(U0_I + 1, U0_SEED)
    assert u[U0_I] == 0.0 and (u[:U0_I] > 0).all()
    for bins in (529, 313):
        c, p = _dist(bins, "plateau_lead", make_sd)
        pdf = p[1, :, 3, 5]
        assert c.first_live() == 10 and (pdf[:10] == 0).all() and pdf[10] > 0
        one = session.draw_counts(pdf, U0_I + 1, U0_SEED).astype(np.int64) - session.draw_counts(pdf, U0_I, U0_SEED).astype(np.int64)
        assert one.tolist() == np.eye(bins, dtype=np.int64)[10].tolist()                                   # draw U0_I alone: bin 10, not bin 0
        assert _counts_lt(pdf, U0_I + 1, U0_SEED)[0] == 1          # what #{cmf < u} would do
        c, p = _dist(bins, "plateau", make_sd)                     # bin 0 alive: the same draw lands on bin 0
        assert c.first_live() == 0 and session.draw_counts(p[1, :, 3, 5], U0_I + 1, U0_SEED)[0] >= 1


# ------------------------------------------------------------------------------------------------ neighbours ordered by d^2
@pytest.mark.parametrize("bins", [529, 313])
def test_neighbours_by_d2_equal_neighbours_by_d_but_for_shared_roots(bins):
    cc = S.grid529() if bins == 529 else np.ascontiguousarray(np.asarray(color_bins.pts_in_hull(), np.float32))
    rs = np.random.RandomState(bins)
    truth = (rs.rand(2, 40, 60) * 200.0 - 100.0).astype(np.float32)
    truth[:, 0, 0] = (5.0, 0.0)                                    # exact ties in d and in d^2: both orders keep the lower index
    truth[:, 0, 1] = (5.0, 5.0)
    for nn in (1, 2, 16):
        qd, d2d, md, sd_ = S.neighbours(truth, cc, nn)
        q2, d22, m2, s2 = S.neighbours(truth, cc, nn, by="d2")
        assert S.neighbours(truth, cc, nn, by="d")[0].tobytes() == qd.tobytes()                            # the default is today's order
        differ = (qd != q2).any(axis=-1)
        # where the two orders differ, two DIFFERENT d^2 among the first nn + 1 share their float64 root; nowhere else
        full = np.sort(((truth[0].astype(np.float64)[..., None] - cc[:, 0].astype(np.float64)) ** 2 +
                        (truth[1].astype(np.float64)[..., None] - cc[:, 1].astype(np.float64)) ** 2), axis=-1)[..., :nn + 1]
        shared = ((np.diff(full, axis=-1) > 0) & (np.diff(np.sqrt(full), axis=-1) == 0)).any(axis=-1)
        assert not (differ & ~shared).any()
        assert d2d[~differ].tobytes() == d22[~differ].tobytes() and md[~differ].tobytes() == m2[~differ].tobytes()
        assert (np.diff(d22, axis=-1) >= 0).all()                  # by d^2: ascending in d^2 everywhere
        assert q2[0, 0, 0] == qd[0, 0, 0] and q2[0, 1, 0] == qd[0, 1, 0]
    dup = cc.copy()
    i, j = 100, 250
    dup[j] = dup[i]                                                # a duplicated centre: equal d^2, the lower index first, in both orders
    t = np.repeat(dup[i][:, None, None] + np.float32(1.5), 3, axis=2)
    for by in ("d", "d2"):
        q = S.neighbours(t, dup, 2, by=by)[0]
        assert (q[..., 0] == i).all() and (q[..., 1] == j).all()
        assert (S.neighbours(t, dup, 1, by=by)[0] == i).all()


# ------------------------------------------------------------------------------------------------ the mutants
def _decode_mode_highest(p, centres):
    B = p.shape[1]
    return np.moveaxis(np.asarray(centres, np.float32)[B - 1 - np.argmax(p[:, ::-1], axis=1)], -1, 1)


def _peaks_highest(ent, P, radius, s):
    pk, pe = D.peaks(ent[:, ::-1, ::-1], P, radius, s)
    n, Hd, Wd = ent.shape
    out = np.where(pk >= 0, np.array([Hd, Wd]) * s - 1 - pk + (s // 2) * 2 - (s - 1), -1)
    return out.astype(np.int32), pe


def _counts_lt(pdf, N, seed):
    """draw_counts with #{cmf < u} in place of #{cmf <= u}."""
    pdf = np.asarray(pdf, np.float32)
    cmf = np.cumsum(pdf, dtype=np.float32)
    cmf = cmf / cmf[-1]
    idx = np.minimum(np.digitize(session.draws(N, seed), bins=cmf, right=True), len(pdf) - 1)
    return np.bincount(idx, minlength=len(pdf)).astype(np.uint32)


def _xent_no_floor(dist, truth_ab, centres):
    t = S.neighbours(truth_ab, centres, 1, by="d2")[0][..., 0]
    with np.errstate(divide="ignore"):
        return 0.0 - np.log(np.take_along_axis(dist, t[None], axis=0)[0].astype(np.float64))


def _xent_skipping_equal_d2(dist, truth_ab, centres, sigma=5.0):
    """Two neighbours, the second one the nearest centre with a LARGER d^2 than the first: a duplicate of the first is skipped."""
    t = np.asarray(truth_ab, np.float32).astype(np.float64)
    c = np.asarray(centres, np.float32).astype(np.float64)
    da, db = t[0][..., None] - c[:, 0], t[1][..., None] - c[:, 1]
    d2 = da * da + db * db
    order = np.argsort(d2, axis=-1, kind="stable")
    d2s = np.take_along_axis(d2, order, axis=-1)
    nxt = np.argmax(d2s > d2s[..., :1], axis=-1)
    q = np.stack([order[..., 0], np.take_along_axis(order, nxt[..., None], axis=-1)[..., 0]], axis=-1)
    w = S.weights(np.take_along_axis(d2, q, axis=-1), sigma)
    logs = np.log(np.maximum(np.stack([np.take_along_axis(dist, q[..., j][None], axis=0)[0] for j in (0, 1)], axis=-1), np.float32(S.FLT_MIN)).astype(np.float64))
    return 0.0 - (w[..., 0] * logs[..., 0] + w[..., 1] * logs[..., 1])


def _entropy_numpy(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sum(p.astype(np.float64) * np.log(p.astype(np.float64)), axis=1)


def _suggest(pdf, centres, K, N, seed, last):
    """oracle/session.suggest_colors spelt out once more with a switch: ``last`` keeps the LAST maximum of count * D^2 in the seeding pass."""
    cnt = session.draw_counts(pdf, N, seed).astype(np.float64)
    pts = np.asarray(centres, np.float32).astype(np.float64)
    means = np.zeros((K, 2))
    for k in range(K):
        if k == 0:
            d2 = np.ones(len(cnt))
        else:
            d = pts[:, None, :] - means[None, :k, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).min(axis=1)
        v = cnt * d2
        means[k] = pts[int(len(v) - 1 - np.argmax(v[::-1])) if last else int(np.argmax(v))]
    asg, occ = -np.ones(len(cnt), np.int64), np.zeros(K)
    for _ in range(100):
        d = pts[:, None, :] - means[None, :, :]
        new = np.argmin(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1], axis=1)
        changed = bool(np.any((new != asg) & (cnt > 0)))
        asg = new
        for k in range(K):
            sel = (asg == k) & (cnt > 0)
            occ[k] = cnt[sel].sum()
            if occ[k] > 0:
                means[k] = [np.sum(cnt[sel] * pts[sel, 0]) / occ[k], np.sum(cnt[sel] * pts[sel, 1]) / occ[k]]
        if not changed:
            break
    order = sorted(range(K), key=lambda k: (-occ[k], k))
    return means[order], occ[order] / float(N)


def _truths(s):
    key = ("truth", s)
    if key not in _DIST:
        _DIST[key] = np.stack([S.truth(img, H, W, s) for img in C.images(H, W, N_IMG)])
    return _DIST[key]


def _told_apart(bins, recipe, make_sd):
    """name of mutant -> True where its answer on this crafted input differs from the restatement's."""
    c, p = _dist(bins, recipe, make_sd)
    cc = centres_of(bins)
    s = 4 if bins == 529 else 1
    truth = _truths(s)
    out = {}
    out["mode decode: highest bin of a tie"] = _decode_mode_highest(p, cc).tobytes() != M.decode_mode(p, cc)[0].tobytes()
    ent = M.entropy(p).astype(np.float32)
    out["peaks: highest cell of a tie"] = _peaks_highest(ent[:1], 4, 2, s)[0].tobytes() != D.peaks(ent[:1], 4, 2, s)[0].tobytes()
    ref = S.score(p[1], truth[1], cc, 1, 5.0, by="d2")
    out["rank: no tie term"] = S.score(p[1], truth[1], cc, 1, 5.0, tie=False, by="d2")["rank"].tobytes() != ref["rank"].tobytes()
    out["xent: no FLT_MIN floor"] = _xent_no_floor(p[1], truth[1], cc).tobytes() != ref["xent"].tobytes()
    dup, i0, j0, most = C.duplicated_centres(cc, ref["target"], ~c.zero, p[1, :, 0, 0])
    ref2 = S.score(p[1], truth[1], dup, 2, 5.0, by="d2")
    at = ref2["q"][..., 0] == i0
    assert i0 < j0 and at.sum() >= most and (ref2["q"][..., 1][at] == j0).all() and not (ref2["target"] == j0).any()
    skipped = _xent_skipping_equal_d2(p[1], truth[1], dup)
    out["neighbours: equal d^2 skipped"] = bool((np.abs(skipped - ref2["xent"]) > 1e-12 * np.abs(ref2["xent"])).any())       # the GPU file's bar
    out["entropy: NaN on a zero bin"] = bool(np.isnan(_entropy_numpy(p)).any()) and bool(np.isfinite(M.entropy(p)).all())
    pdf = p[1, :, 3, 5]
    out["draws: #{cmf < u}"] = _counts_lt(pdf, 8, U0_SEED).tobytes() != session.draw_counts(pdf, 8, U0_SEED).tobytes()
    want = session.suggest_colors(pdf, cc, K=5, N=25000, seed=7)
    first, last = _suggest(pdf, cc, 5, 25000, 7, False), _suggest(pdf, cc, 5, 25000, 7, True)
    assert first[0].tobytes() == want[0].tobytes() and first[1].tobytes() == want[1].tobytes()            # the switch off: the oracle itself
    out["seeding: last maximum"] = last[0].tobytes() != want[0].tobytes() or last[1].tobytes() != want[1].tobytes()
    return out


def test_every_mutant_is_caught_and_every_crafted_input_catches_one(make_sd):
    table = {inp: _told_apart(inp[0], inp[1], make_sd) for inp in INPUTS}
    names = sorted(next(iter(table.values())))
    for inp in INPUTS:
        print("%d %-13s %s" % (inp[0], inp[1], " ".join("%s=%d" % (n.split(":")[0], table[inp][n]) for n in names)))
    for n in names:
        assert any(table[inp][n] for inp in INPUTS), "no crafted input tells '%s' apart" % n
        for bins in (529, 313):
            assert any(table[(bins, r)][n] for r in C.RECIPES), "no crafted input of the %d head tells '%s' apart" % (bins, n)
    for inp in INPUTS:
        assert any(table[inp].values()), "crafted input %s tells no mutant apart" % (inp,)
    # and the rules on the inputs they were crafted for
    assert table[(529, "uniform")]["rank: no tie term"] and table[(529, "uniform")]["mode decode: highest bin of a tie"]
    assert table[(529, "one_hot")]["seeding: last maximum"] and table[(313, "one_hot")]["xent: no FLT_MIN floor"]
    assert table[(529, "plateau_lead")]["draws: #{cmf < u}"] and not table[(529, "plateau")]["draws: #{cmf < u}"]
    assert not table[(529, "uniform")]["entropy: NaN on a zero bin"] and table[(529, "plateau")]["entropy: NaN on a zero bin"]
    # all probabilities equal: a skipped neighbour cannot show in the cross-entropy of uniform; it does on every other recipe
    assert all(table[inp]["neighbours: equal d^2 skipped"] == (inp[1] != "uniform") for inp in INPUTS)


def test_the_first_maximum_seeds_are_the_oracles_and_show_in_its_result(make_sd):
    """On a one-hot cell the oracle's empty clusters sit on the FIRST maximum's centre (bin
    0), with share [1, 0, ...], for K = 5 and 16 -- where the last maximum would have put them on bin B - 1."""
    for bins in (529, 313):
        c, p = _dist(bins, "one_hot", make_sd)
        cc = centres_of(bins)
        pdf = p[0, :, 2, 7]
        for K in (1, 5, 16):
            cen, conf, cnt = session.suggest_colors(pdf, cc, K=K, N=3, seed=1, return_counts=True)
            assert cnt[c.q0] == 3 and cnt.sum() == 3 and conf.tolist() == [1.0] + [0.0] * (K - 1)
            assert cen[0].tolist() == cc[c.q0].tolist() and (cen[1:] == cc[0]).all()
        assert (_suggest(pdf, cc, 5, 3, 1, True)[0][1:] == cc[bins - 1]).all()
        c, p = _dist(bins, "uniform", make_sd)
        assert len(np.unique(p)) == 1
        c, p = _dist(bins, "plateau", make_sd)                      # 486 / 270 zero bins: no division by zero, no draw in a zero bin
        cen, conf, cnt = session.suggest_colors(p[0, :, 0, 0], cc, K=5, N=25000, seed=U0_SEED, return_counts=True)
        assert np.isfinite(cen).all() and abs(conf.sum() - 1.0) < 1e-12 and not cnt[c.zero].any() and cnt.sum() == 25000
