"""Every grid-capped launcher run PAST its cap at test-sized shapes (csrc/idc_grid.h, option 'grid_cap').

21 launchers clamp their grid and let the kernel walk the rest in a grid-stride loop.  No shape of the suite gives one of them more items than
one pass holds, so the second pass, the stride and the ragged last pass are reached here by LOWERING the cap: every row of ROWS runs the route
its own test file uses, at a shape of that file, with the grid lowered to 1 workgroup and to an odd count, and holds the result against that
file's independent reference at that file's bar -- and bit for bit against the same call at the default grid.

A row (`_drive`):
  1. the call on input X at the default grid -> R0; the stored tensors a reference needs (conv10_2, class_logits, pred_313, the audited
     activations) are read back now, at the default grid; the reference is checked on R0 as well;
  2. for cap in (1, the first of 3, 5, 7 with want > 2 cap and want % cap != 0 for every launch the row records):
       the call on another input Y of the same shape at the default grid (what a capped launch fails to write then holds Y's value),
       the call on X under the cap,
       engine.grid_last(tag) of every recorded launch: blocks == cap, want > 2 cap, want % cap != 0 for the odd cap -- at least three passes,
       a ragged last one,
       the reference at the row's bar, and R0 bit for bit;
  3. Y's default-grid result differs from X's (`_assert_differs`).
The one value not compared bit for bit is global_stats' saturation sum (float64 atomics: the order of the additions is free); it is held at
the bar of tests/test_caffe_branches_gpu.py, its counts are integers and equal.

How far Y differs.  "In every element" cannot be asserted of these outputs: two uint8 colours, two fp32 probabilities out of millions, a
ReLU's zeros and a histogram's empty bins coincide by chance.  What a fault in a grid-stride loop loses is a whole iteration of a workgroup
(256 consecutive items, or the last, ragged one), so `_assert_differs` asks: at least 99 % of the units (a pixel's three bytes, one float)
differ (95 % of the 313 head's decoded pred_ab, which collapses to a bin centre where one bin holds all the mass), no aligned run of 64 units
is equal throughout, and the last unit differs.  Outputs behind a ReLU (the exact-lattice op rows) and
the audit's per-layer maxima are exempt from the last two and ask 40 % / 95 %; the 313-bin histogram (mostly empty bins, counts added to
zeroed memory) only has to differ.

Bars: none is stated here -- every row names the bar of its source file (heads_ref.*_BAR, ingest's 1e-9 / bit equality / one uint8 level on
2e-4 of the values, exact integer SSE, the audit's census, exact_lattice.compare, the global statistics' 4 / 4096 and 1e-5).

Wall time of this file on an MI355X: 13.8 s for its 33 cases (eleven handles, the largest 256 x 256 without weights); the slowest case takes 1.7 s
(batch_203x187: three 203 x 187 images through scipy's zoom and the oracle's lab2rgb on the host), a case without host-side colour references
a few tenths of a second at most.  At cap 1 the longest launch is one workgroup walking 2880 passes of a layout converter.
"""
import numpy as np
import pytest

import eval_ref as E
import exact_lattice as xl
import heads_ref as hr
import ingest_ref
import ragged_ref as R
from interactive_deep_colorization_amd import engine, workloads
from oracle import colorspace as ocs
from oracle import display, weights
from test_batch_rgb_gpu import FRAC, HINTS_AB, _batch, _hint_lists, _pipelined
from test_eval_gpu import _eval
from test_ingest_gpu import HINTS, LAB_TOL
from test_ops_exact_gpu import CASES, run_case
from test_ragged_batch_gpu import _run as _ragged_run

pytestmark = pytest.mark.gpu

_OPTION_DEFAULTS = {"grid_cap": 0, "pcie_kernel": 1, "op_policy_batch": 0, "winograd": 1, "ds_mfma16": 1, "kwave": 1, "click": -1, "v2p": 1,
                    "fp16_fast": 1, "split_ds_fuse": 1, "op_out_f32": 0, "op_resid_f32": 0}
_E = {}
_SD = {}


@pytest.fixture(autouse=True)
def _reset_grid_cap_and_policies():
    yield
    for name, value in _OPTION_DEFAULTS.items():
        engine.set_option(name, value)
    engine.set_tile_policy("auto")
    engine.set_splitk_policy("auto")


def _heads_sd():
    """The state dict of tests/test_heads_gpu.py: he-style trunk, Global-Hints branch, 313 head."""
    if "heads" not in _SD:
        from conftest import state_dict_for
        sd = dict(state_dict_for(hr.WEIGHT_SEED, hr.WEIGHT_STYLE))
        weights.add_global_branch(sd, hr.GLOB_SEED)
        weights.add_pred313_head(sd, hr.PRED_SEED)
        _SD["heads"] = sd
    return _SD["heads"]


def _engine(key, H, W, sd=None, **kw):
    """One handle per key for the whole file (conftest closes them when the module is done)."""
    if key not in _E:
        e = engine.HipColorizer(H, W, **kw)
        if sd is not None:
            e.load_state_dict(sd)
        e.key = key
        _E[key] = e
    return _E[key]


def _rec(res, *tags):
    """Note what the last launch of each tag asked for and got."""
    for t in tags:
        res.setdefault("_grid", []).append((t,) + engine.grid_last(t))


def _check_u8(got, want, what):
    mx, frac = ingest_ref.close_u8(got, want)
    print("%s: max level difference %d on %.3g of %d values" % (what, mx, frac, want.size))
    assert got.shape == want.shape and got.dtype == np.uint8
    assert mx <= 1 and frac <= FRAC, (what, mx, frac)


def _assert_differs(a, b, what, unit=1, min_frac=0.99, runs=True):
    """Y's default-grid result differs from X's wherever a lost iteration of a grid-stride loop would have to show (the file's docstring)."""
    a, b = np.asarray(a).reshape(-1, unit), np.asarray(b).reshape(-1, unit)
    d = (a != b).any(axis=1)
    print("%s: Y differs from X in %.4f of %d units" % (what, d.mean(), d.size))
    assert d.mean() >= min_frac, (what, float(d.mean()))
    if runs:
        assert d[-1], "%s: the last unit of Y equals X's" % what
        full = d[:d.size // 64 * 64].reshape(-1, 64)
        assert full.any(axis=1).all(), "%s: a run of 64 units of Y equals X's" % what


def _odd_cap(wants):
    for cap in (3, 5, 7):
        if all(w > 2 * cap and w % cap != 0 for w in wants):
            return cap
    raise AssertionError("no cap of 3, 5, 7 gives three passes with a ragged last one for wants %s: take a larger shape" % (wants,))


class Row:
    """tags: the launch sites the row records.  inputs() -> (X, Y); run(inp, stored) -> dict of results ('_...' keys: stored tensors and the
    grid records, not compared); check(res, r0): the independent reference at the source file's bar (r0 carries the stored tensors);
    differs(r0, ry); same(res, r0): bit equality of every key not starting with '_' unless a row says otherwise."""
    tags = ()

    def same(self, res, r0):
        for k in r0:
            if not k.startswith("_"):
                np.testing.assert_array_equal(res[k], r0[k], err_msg="%s under a lowered grid against the default grid" % k)


def _drive(row):
    X, Y = row.inputs()
    r0 = row.run(X, True)
    ry = row.run(Y, False)
    row.differs(r0, ry)
    row.check(r0, r0)
    seen = sorted(set(g[0] for g in r0["_grid"]))
    assert seen == sorted(row.tags), (seen, row.tags)
    wants = [g[1] for g in r0["_grid"]]
    for tag, want, blocks in r0["_grid"]:
        assert blocks == want, "%s: the default grid of this shape (%d of %d) is capped already" % (tag, blocks, want)
    for cap in (1, _odd_cap(wants)):
        row.run(Y, False)
        engine.set_option("grid_cap", cap)
        try:
            res = row.run(X, False)
        finally:
            engine.set_option("grid_cap", 0)
        assert [g[0] for g in res["_grid"]] == [g[0] for g in r0["_grid"]]
        for tag, want, blocks in res["_grid"]:
            print("cap %d: %s want %d blocks %d = %d passes" % (cap, tag, want, blocks, -(-want // blocks)))
            assert blocks == cap and want > 2 * cap, (tag, want, blocks, cap)
            assert cap == 1 or want % cap != 0, (tag, want, cap)
        row.check(res, r0)
        row.same(res, r0)


# ---- head, softmax_nchw, dist313: float64 from the stored input (tests/test_heads_gpu.py) ---------------------------------------------------
class HeadsRow(Row):
    def __init__(self, shape, precision):
        self.shape, self.precision = shape, precision
        H, W, n = hr.SHAPES[shape]
        flags = dict(dist=True, dist313=True) if precision == "fp32" else {}
        self.e = _engine(("heads", shape, precision), H, W, _heads_sd(), max_batch=hr.MAX_BATCH, precision=precision, **flags)
        self.n = n
        self.ref = None

    def inputs(self):
        H, W, n = hr.SHAPES[self.shape]
        return hr.images(self.shape), workloads.random_batch(n, H, W, seed=29, max_points=4, max_p=2)

    def differs(self, r0, ry):
        for k in r0:
            if not k.startswith("_"):
                # pred_ab is a mean over the 313 centres at temperature 2.6: where one bin holds all the mass, X and Y both give that centre
                _assert_differs(r0[k], ry[k], "%s %s %s" % (self.tags[0], self.shape, k), min_frac=0.95 if k == "pred" else 0.99)


class HeadRow(HeadsRow):
    tags = ("head",)

    def run(self, inp, stored):
        e = self.e
        if self.precision == "bf16":
            engine.set_tile_policy("small")            # conv10_2 on the small tile: stored, the head is a launch of its own (bf16 form)
        res = {"out": e.forward(*inp, 0.0).copy()}
        _rec(res, "head")
        if stored:
            rows = {r["name"]: r for r in e.layer_table()}
            assert rows["head"]["kernel"] == "head_kernel" and "+head" not in rows["conv10_2"]["kernel"], rows["conv10_2"]
            res["_x"] = e.activation("conv10_2", self.n)
        return res

    def check(self, res, r0):
        sd = _heads_sd()
        if self.ref is None:
            self.ref = hr.head(r0["_x"], sd["model_out.0.weight"], sd["model_out.0.bias"], 110.0)
            assert float((np.abs(self.ref) < 99.0).mean()) >= 0.5                   # a saturated tanh hides a wrong sum
        err = float(np.abs(res["out"] - self.ref).max())
        print("head %s %s: abs err %.3e (bar %.3e)" % (self.shape, self.precision, err, hr.HEAD_BAR))
        assert err <= hr.HEAD_BAR


class SoftmaxRow(HeadsRow):
    tags = ("softmax_nchw",)

    def run(self, inp, stored):
        res = {"dq": self.e.forward_dist(*inp, 0.0)[1].copy()}
        _rec(res, "softmax_nchw")
        if stored:
            res["_l"] = self.e.activation("class_logits", self.n)
        return res

    def check(self, res, r0):
        if self.ref is None:
            self.ref = hr.softmax529(r0["_l"])
        rel = float((np.abs(res["dq"] - self.ref) / (self.ref + 1e-12)).max())
        print("softmax529 %s: p rel %.3e (bar %.3e)" % (self.shape, rel, hr.P529_REL_BAR))
        assert res["dq"].shape == self.ref.shape and rel <= hr.P529_REL_BAR


class Dist313Row(HeadsRow):
    tags = ("dist313",)

    def __init__(self, shape, want_dist):
        HeadsRow.__init__(self, shape, "fp32")
        self.want_dist = want_dist

    def run(self, inp, stored):
        e = self.e
        e.set_dist_temperature(hr.S_DEFAULT)
        _, pred, dist = e.forward_dist313(*inp, 0.0, want_dist=self.want_dist)
        res = {"pred": pred.copy()}
        _rec(res, "dist313")
        if self.want_dist:
            res["dist"] = dist.copy()
        else:
            assert dist is None
        if stored:
            res["_l"] = e.activation("pred_313", self.n)
        return res

    def check(self, res, r0):
        sd = _heads_sd()
        if self.ref is None:
            self.ref = hr.dist313(r0["_l"], hr.S_DEFAULT, sd["pred.pred_ab.weight"][:, :, 0, 0].T, sd["pred.pred_ab.bias"])
        ref_d, ref_p = self.ref
        err = float(np.abs(res["pred"] - ref_p).max())
        print("dist313 %s want_dist=%s: pred_ab abs %.3e (bar %.3e)" % (self.shape, self.want_dist, err, hr.PRED_AB_BAR))
        assert err <= hr.PRED_AB_BAR
        if self.want_dist:
            rel = float((np.abs(res["dist"] - ref_d) / (ref_d + 1e-12)).max())
            print("dist313 %s: p rel %.3e (bar %.3e)" % (self.shape, rel, hr.P313_REL_BAR))
            assert res["dist"].shape == ref_d.shape and rel <= hr.P313_REL_BAR


# ---- ingest_rgb (tests/test_ingest_gpu.py): bit-identical resize, Lab to 1e-9 -----------------------------------------------------------------
class IngestRow(Row):
    tags = ("ingest_rgb",)
    SIZES = [(5, 7), (130, 97), (1, 257), (203, 187)]

    def __init__(self, H, W):
        self.H, self.W = H, W
        self.e = _engine(("ingest", H, W), H, W, max_batch=4, precision="bf16")          # no weights: ingestion runs no layer
        self.ref = {}

    def inputs(self):
        # X: the seeds of tests/test_ingest_gpu.py (crops of the photograph and noise); Y: odd seeds, noise throughout
        return [[np.stack([ingest_ref.source_image(sh, sw, seed + 10 * k + step * j) for j in range(3)]) for k, (sh, sw) in enumerate(self.SIZES)]
                for seed, step in ((0, 1), (501, 2))]

    def run(self, inp, stored):
        res = {}
        for (sh, sw), batch in zip(self.SIZES, inp):
            rgb, lab = self.e.set_image_rgb(batch, img=1)
            res["rgb %dx%d" % (sh, sw)], res["lab %dx%d" % (sh, sw)] = rgb.copy(), lab.copy()
            _rec(res, "ingest_rgb")
        if stored:
            res["_src"] = inp
        return res

    def check(self, res, r0):
        for (sh, sw), batch in zip(self.SIZES, r0["_src"]):
            if (sh, sw) not in self.ref:
                want_rgb = np.stack([ingest_ref.net_rgb(s, self.H, self.W) for s in batch])
                self.ref[(sh, sw)] = (want_rgb, np.stack([ingest_ref.net_lab(r) for r in want_rgb]))
            want_rgb, want_lab = self.ref[(sh, sw)]
            np.testing.assert_array_equal(res["rgb %dx%d" % (sh, sw)], want_rgb, err_msg="rgb_net of a %dx%d source" % (sh, sw))
            err = float(np.abs(res["lab %dx%d" % (sh, sw)] - want_lab).max())
            print("source %dx%d -> %dx%d: lab_net max abs error %.3e" % (sh, sw, self.H, self.W, err))
            assert err <= LAB_TOL, (sh, sw, err)

    def differs(self, r0, ry):
        for sh, sw in self.SIZES:
            _assert_differs(r0["rgb %dx%d" % (sh, sw)], ry["rgb %dx%d" % (sh, sw)], "ingest rgb %dx%d" % (sh, sw), unit=3)
            lab0, laby = r0["lab %dx%d" % (sh, sw)], ry["lab %dx%d" % (sh, sw)]
            _assert_differs(lab0.transpose(0, 2, 3, 1), laby.transpose(0, 2, 3, 1), "ingest lab %dx%d" % (sh, sw), unit=3)


# ---- fullres_rgb (tests/test_ingest_gpu.py) and upsample_lab2rgb (tests/test_round2_gpu.py): one uint8 level on 2e-4 of the values --------------
def _net64():
    from conftest import state_dict_for
    return _engine("net64", 64, 64, state_dict_for(0, "he"), max_batch=1, precision="bf16")


class FullresRow(Row):
    tags = ("fullres_rgb",)

    def __init__(self, sh, sw, source, interp, l_mode):
        self.size, self.args = (sh, sw), (source, interp, l_mode)
        self.e = _net64()
        self.ref = None

    def inputs(self):
        sh, sw = self.size
        x = ingest_ref.source_image(sh, sw, 2 * (sh + sw))
        return (x, HINTS), (ingest_ref.source_image(sh, sw, 2 * (sh + sw) + 7), [(2, 3, 60, 50, -45.0, 20.0), (40, 30, 63, 63, 35.0, 35.0)])

    def run(self, inp, stored):
        e = self.e
        src, hints = inp
        e.set_image_rgb(src, keep_source=True, want_rgb=False, want_lab=False)
        e.set_hints(hints, mode="ab")
        _, _, lab_q = e.forward_resident(1)
        res = {}
        if stored:
            in_ab, in_mask = e.hint_planes(0)
            res.update(_src=src, _out_ab=lab_q[0, 1:].copy(), _in_ab=in_ab.copy(), _in_mask=in_mask.copy())
        res["full"] = e.fullres_rgb(*self.args).copy()
        _rec(res, "fullres_rgb")
        return res

    def check(self, res, r0):
        source, interp, l_mode = self.args
        if self.ref is None:
            ab = r0["_out_ab"] if source == "output_ab" else r0["_in_ab"]
            self.ref = ingest_ref.fullres(r0["_src"], ab, {"linear": 1, "nearest": 0}[interp], mask=r0["_in_mask"] if l_mode == "mask50" else None)
        _check_u8(res["full"], self.ref, "fullres %s %s" % (self.size, self.args))

    def differs(self, r0, ry):
        _assert_differs(r0["full"], ry["full"], "fullres %s %s" % (self.size, self.args), unit=3)


class UpsampleRow(Row):
    tags = ("upsample_lab2rgb",)

    def __init__(self, oh, ow, source, interp):
        self.size, self.source, self.interp = (oh, ow), source, interp
        self.e = _net64()
        self.ref = None

    def inputs(self):
        oh, ow = self.size
        return [workloads.random_batch(1, 64, seed=s) + (np.random.RandomState(s).uniform(0, 100, (oh, ow)),) for s in (5, 6)]

    def run(self, inp, stored):
        L, ab, m, l_win = inp
        out, _, labq = self.e.forward_rgb(L, ab, m, 0.0)
        res = {}
        if stored:
            res.update(_l_win=l_win, _planes=(labq[0, 1:] if self.source == "output_ab" else out[0].astype(np.float64)).copy())
        res["up"] = self.e.upsample_lab2rgb(l_win, self.source, self.interp).copy()
        _rec(res, "upsample_lab2rgb")
        return res

    def check(self, res, r0):
        from scipy.ndimage import zoom
        oh, ow = self.size
        if self.ref is None:
            if self.interp == "cubic":
                self.ref = display.display_rgb(r0["_planes"], r0["_l_win"])
            else:
                z = zoom(r0["_planes"], (1, 1. * oh / 64, 1. * ow / 64), order=1 if self.interp == "linear" else 0)
                self.ref = ocs.lab2rgb_transpose(r0["_l_win"][None], z)
        _check_u8(res["up"], self.ref, "upsample %s %s %s" % (self.size, self.source, self.interp))

    def differs(self, r0, ry):
        _assert_differs(r0["up"], ry["up"], "upsample %s %s %s" % (self.size, self.source, self.interp), unit=3)


# ---- global_stats (tests/test_caffe_branches_gpu.py: 64 x 64 holds 256 blocks = one workgroup, so its 256 x 256, n = 2 shape) -------------------
class GlobalStatsRow(Row):
    tags = ("global_stats",)

    def __init__(self):
        self.e = _engine("stats256", 256, 256, max_batch=2, precision="bf16")
        self.centres = weights.synthetic_ab_centres(0)
        self.ref = None

    def inputs(self):
        rgb = ingest_ref.mortar()
        noise = [np.random.RandomState(s).randint(0, 256, (256, 256, 3)).astype(np.uint8) for s in (1, 2)]
        return np.stack([rgb, noise[0]]), np.stack([noise[1], np.ascontiguousarray(rgb[::-1, ::-1])])

    def run(self, inp, stored):
        hist, sat = self.e.global_histogram(inp, self.centres)
        res = {"hist": hist.copy(), "sat": sat.copy()}
        _rec(res, "global_stats")
        if stored:
            res["_src"] = inp
        return res

    def check(self, res, r0):
        if self.ref is None:
            self.ref = [ocs.global_stats(img, self.centres) for img in r0["_src"]]
        for i, (rh, rsat) in enumerate(self.ref):
            assert abs(res["hist"][i].sum() - 1.0) < 1e-6
            assert np.abs(res["hist"][i] - rh).sum() <= 4.0 / 4096 + 1e-7, np.abs(res["hist"][i] - rh).sum()
            assert abs(res["sat"][i] - rsat) < 1e-5

    def differs(self, r0, ry):
        # (counts are added to zeroed memory with atomics: nothing stale can stand in for a count; most of the 313 bins are empty in both)
        assert (r0["hist"] != ry["hist"]).any(axis=1).all() and (r0["sat"] != ry["sat"]).all()

    def same(self, res, r0):
        np.testing.assert_array_equal(res["hist"], r0["hist"])                      # integer counts: exact in any order
        assert np.abs(res["sat"].astype(np.float64) - r0["sat"]).max() < 1e-5       # float64 atomics: the order is free, the file's bar


# ---- batch_prologue, batch_fullres_rgb, lab_post (tests/test_batch_rgb_gpu.py) and the ragged forms (tests/test_ragged_batch_gpu.py) -----------
def _oracle_colours(images, r0, H, W):
    """The references of test_batch_matches_the_oracle_colour_conversions, from the sources and the default-grid call's ab map and net-size image
    (read back at the default grid, like a stored activation; a lowered grid has to give the same bits): [(net-size rgb, source-size rgb)]."""
    refs = []
    for i, img in enumerate(images):
        lab = ingest_ref.net_lab(ingest_ref.net_rgb(img, H, W))
        L = np.float32(lab[0] - 50).astype(np.float64) + 50                         # the slot's fp32 L plane, + l_cent
        refs.append((ocs.lab2rgb_transpose(L[None], r0["ab"][i].astype(np.float64)), ingest_ref.fullres(img, ingest_ref.net_lab(r0["net"][i])[1:], 1)))
    return refs


def _oracle_colour_check(refs, net, full, what):
    for i, (want_net, want_full) in enumerate(refs):
        _check_u8(net[i], want_net, "%s net-size image %d" % (what, i))
        _check_u8(full[i], want_full, "%s source-size image %d of %dx%d" % (what, i, want_full.shape[0], want_full.shape[1]))


def _flat_pixels(images):
    return np.concatenate([np.asarray(a).reshape(-1, 3) for a in images])


class BatchRow(Row):
    tags = ("batch_prologue", "batch_fullres_rgb", "lab_post")

    def __init__(self, sh, sw):
        from conftest import state_dict_for
        self.size = (sh, sw)
        self.e = _engine("batch64", 64, 64, state_dict_for(0, "he"), max_batch=4, precision="bf16")
        self.ref = None

    def inputs(self):
        sh, sw = self.size
        return (_batch(3, sh, sw, 30), _hint_lists(3, "ab", 0)), (_batch(3, sh, sw, 731), _hint_lists(3, "ab", 1))

    def run(self, inp, stored):
        batch, hints = inp
        res = {}
        net, ab = _pipelined(self.e, batch, hints, "ab", 1.0, "net")
        _rec(res, "batch_prologue", "lab_post")
        full, ab2 = _pipelined(self.e, batch, hints, "ab", 1.0, "source", slot=1)
        _rec(res, "batch_prologue", "lab_post", "batch_fullres_rgb")
        res.update(net=net.copy(), full=full.copy(), ab=np.array(ab), ab2=np.array(ab2))
        if stored:
            res["_src"] = batch
        return res

    def check(self, res, r0):
        assert np.isfinite(res["ab"]).all() and np.abs(res["ab"]).max() > 0
        np.testing.assert_array_equal(res["ab2"], res["ab"])
        if self.ref is None:
            self.ref = _oracle_colours(list(r0["_src"]), r0, 64, 64)
        _oracle_colour_check(self.ref, res["net"], res["full"], "batch %s" % (self.size,))

    def differs(self, r0, ry):
        _assert_differs(r0["ab"], ry["ab"], "batch out_ab")
        _assert_differs(r0["net"], ry["net"], "batch net-size rgb", unit=3)
        _assert_differs(r0["full"], ry["full"], "batch source-size rgb", unit=3)


def _mixed_engine():
    from conftest import state_dict_for
    return _engine("mixed64", 64, 64, state_dict_for(0, "he"), max_batch=8, precision="bf16")


def _mixed_images(seed):
    return [R.image(sh, sw, seed + j) for j, (sh, sw) in enumerate(R.sizes(R.MIXED, 64, 64))]


class RaggedRow(Row):
    tags = ("ragged_prologue", "ragged_fullres_rgb", "lab_post")

    def __init__(self):
        self.e = _mixed_engine()
        self.ref = None

    def inputs(self):
        return (_mixed_images(400), [HINTS_AB[i % 4] for i in range(7)]), (_mixed_images(901), [HINTS_AB[(i + 1) % 4] for i in range(7)])

    def run(self, inp, stored):
        images, hints = inp
        res = {}
        net, ab = _ragged_run(self.e, images, hints, "ab", 1.0, "net", slot=0)
        _rec(res, "ragged_prologue", "lab_post")
        full, ab2 = _ragged_run(self.e, images, hints, "ab", 1.0, "source", slot=1)
        _rec(res, "ragged_prologue", "lab_post", "ragged_fullres_rgb")
        res.update(net=np.stack(net), full=_flat_pixels(full), ab=np.array(ab), ab2=np.array(ab2), _full=[f.copy() for f in full])
        if stored:
            res["_src"] = images
        return res

    def check(self, res, r0):
        assert np.isfinite(res["ab"]).all() and np.abs(res["ab"]).max() > 0
        np.testing.assert_array_equal(res["ab2"], res["ab"])
        if self.ref is None:
            self.ref = _oracle_colours(r0["_src"], r0, 64, 64)
        _oracle_colour_check(self.ref, res["net"], res["_full"], "mixed batch")

    def differs(self, r0, ry):
        _assert_differs(r0["ab"], ry["ab"], "mixed batch out_ab")
        _assert_differs(r0["net"], ry["net"], "mixed batch net-size rgb", unit=3)
        _assert_differs(r0["full"], ry["full"], "mixed batch source-size rgb", unit=3)


# ---- ragged_net_truth, eval_sse (tests/test_eval_gpu.py): the exact integer score -------------------------------------------------------------------
class EvalRow(Row):
    """The net-size score reads ragged_net_truth's pixels; its eval_sse launch holds 5 workgroups' worth (4096 pixels an image), so the
    eval_sse record is taken from the source-size score, whose largest image (203 x 187) makes 38."""
    tags = ("ragged_net_truth", "eval_sse")

    def __init__(self):
        self.e = _mixed_engine()

    def inputs(self):
        return (_mixed_images(400), [E.LISTS[i % 4] for i in range(7)]), (_mixed_images(901), [E.LISTS[(i + 1) % 4] for i in range(7)])

    def run(self, inp, stored):
        images, hints = inp
        res = {}
        sse_n, _, net, _ = _eval(self.e, images, hints, out="net", slot=0)
        _rec(res, "ragged_net_truth")
        sse_s, _, full, _ = _eval(self.e, images, hints, out="source", slot=1)
        _rec(res, "eval_sse")
        res.update(sse_n=sse_n, sse_s=sse_s, net=np.stack(net), full=_flat_pixels(full), _full=[f.copy() for f in full])
        if stored:
            res["_src"] = images
        return res

    def check(self, res, r0):
        assert res["sse_n"].shape == (7, 3) and res["sse_n"].dtype == np.uint64
        for i, img in enumerate(r0["_src"]):
            assert res["sse_n"][i].tolist() == E.sse(res["net"][i], ingest_ref.net_rgb(img, 64, 64)), "net-size score of image %d %s" % (i, img.shape)
            assert res["sse_s"][i].tolist() == E.sse(res["_full"][i], img), "source-size score of image %d %s" % (i, img.shape)
        assert int(res["sse_s"][5].sum()) > 0

    def differs(self, r0, ry):
        assert (r0["sse_n"] != ry["sse_n"]).all() and (r0["sse_s"] != ry["sse_s"])[2:6].all()     # (images 0, 1, 6 have 1, 35 and 6 pixels)
        _assert_differs(r0["net"], ry["net"], "eval net-size rgb", unit=3)
        _assert_differs(r0["full"], ry["full"], "eval source-size rgb", unit=3)


# ---- range_audit (tests/test_range_audit_gpu.py): the numpy census of the stored activations ---------------------------------------------------------
class AuditRow(Row):
    tags = ("range_audit",)

    def __init__(self, precision):
        from conftest import state_dict_for
        self.precision = precision
        self.e = _engine(("audit", precision), 64, 64, state_dict_for(1, "he"), max_batch=2, precision=precision)

    def inputs(self):
        return [workloads.random_batch(2, 64, 64, seed=s, max_points=5, max_p=3) for s in (11, 12)]

    def run(self, inp, stored):
        e = self.e
        e.range_reset()
        e.set_range_audit(True)
        try:
            e.forward(*inp, 0.5)
            res = {}
            _rec(res, "range_audit")
            rep = e.range_report()
        finally:
            e.set_range_audit(False)
        live = [r for r in rep if r["n_values"]]
        res.update(max_abs=np.array([r["max_abs"] for r in live], np.float64), n_tiny=np.array([r["n_tiny"] for r in live], np.int64),
                   n_values=np.array([r["n_values"] for r in live], np.int64), _rep=live)
        if stored:
            res["_acts"] = {r["name"]: e.activation(r["name"], 2) for r in live}
        return res

    def check(self, res, r0):
        assert len(res["_rep"]) >= 25 and [r["name"] for r in res["_rep"]] == list(r0["_acts"])
        for r in res["_rep"]:
            got = r0["_acts"][r["name"]]
            mx = float(np.abs(got).max())
            assert r["n_saturated"] == 0 and r["n_nonfinite"] == 0 and r["n_values"] == got.size, r
            if r["storage"].endswith("x3"):
                assert abs(r["max_abs"] - mx) <= 2.0 ** -22 * mx, r
            else:
                assert r["max_abs"] == mx, (r, mx)
            assert r["n_tiny"] == int(np.count_nonzero((got != 0) & (np.abs(got) < 2.0 ** -14))), r
        want = {"fp32": "fp32", "fp16x3": "fp16x2"}[self.precision]
        assert {r["name"]: r["storage"] for r in res["_rep"]}["conv6_1"] == want

    def differs(self, r0, ry):
        _assert_differs(r0["max_abs"], ry["max_abs"], "audit max_abs %s" % self.precision, min_frac=0.95, runs=False)


# ---- splitk_epilogue and the four layout converters: exact-lattice cases of tests/test_ops_exact_gpu.py, bit for bit ------------------------------
class OpRow(Row):
    def __init__(self, case_id, tags):
        self.c = [c for c in CASES if c.id == case_id][0]
        self.tags = tags
        self.ref = None

    def inputs(self):
        return xl.draw(self.c), xl.draw(self.c._replace(id=self.c.id + "/y"))

    def run(self, inp, stored):
        got, label = run_case(self.c, inp)
        assert label == self.c.label, "%s ran %r, the table expects %r" % (self.c.id, label, self.c.label)
        res = {"y": got.copy()}
        _rec(res, *self.tags)
        if stored:
            res["_d"] = inp
        return res

    def check(self, res, r0):
        if self.ref is None:
            self.ref = xl.expected(self.c, r0["_d"])
        xl.compare(res["y"], self.ref, "%s [%s]" % (self.c.id, self.c.label))

    def differs(self, r0, ry):
        relu = self.c.act == 1
        _assert_differs(r0["y"], ry["y"], self.c.id, min_frac=0.4 if relu else 0.99, runs=not relu)


SPLITK_TAGS = ("splitk_epilogue", "nchw_to_nhwc", "nhwc_to_nchw")
SPLIT_TAGS = ("nchw_to_split", "split_to_nchw")


# ---- pcie_copy: a click whose transfers run as the copy kernel equals the same click through the copy engines -----------------------------------------
class PcieRow(Row):
    tags = ("pcie_copy",)

    def __init__(self):
        from conftest import state_dict_for
        self.e = _engine("click64", 64, 64, state_dict_for(0, "he"), max_batch=1, precision="bf16")
        self.ref = None

    def inputs(self):
        return workloads.random_batch(1, 64, seed=3), workloads.random_batch(1, 64, seed=4)

    def run(self, inp, stored):
        engine.set_option("pcie_kernel", 1)
        res = {"out": self.e.forward(*inp, 0.0).copy()}
        _rec(res, "pcie_copy")
        if stored:
            res["_inp"] = inp
        return res

    def check(self, res, r0):
        if self.ref is None:
            engine.set_option("pcie_kernel", 0)
            try:
                self.ref = self.e.forward(*r0["_inp"], 0.0).copy()
            finally:
                engine.set_option("pcie_kernel", 1)
            assert np.isfinite(self.ref).all() and np.abs(self.ref).max() > 0
        np.testing.assert_array_equal(res["out"], self.ref)

    def differs(self, r0, ry):
        _assert_differs(r0["out"], ry["out"], "click out_ab")


# id: (tags the row records, how to make it)
ROWS = {
    "head_A_fp32": (("head",), lambda: HeadRow("A", "fp32")),
    "head_B_fp32": (("head",), lambda: HeadRow("B", "fp32")),
    "head_A_bf16": (("head",), lambda: HeadRow("A", "bf16")),
    "head_B_bf16": (("head",), lambda: HeadRow("B", "bf16")),
    "softmax_A": (("softmax_nchw",), lambda: SoftmaxRow("A", "fp32")),
    "softmax_B": (("softmax_nchw",), lambda: SoftmaxRow("B", "fp32")),
    "dist313_A": (("dist313",), lambda: Dist313Row("A", True)),
    "dist313_B": (("dist313",), lambda: Dist313Row("B", True)),
    "dist313_A_pred_only": (("dist313",), lambda: Dist313Row("A", False)),
    "dist313_B_pred_only": (("dist313",), lambda: Dist313Row("B", False)),
    "ingest_64x64": (IngestRow.tags, lambda: IngestRow(64, 64)),
    "ingest_40x72": (IngestRow.tags, lambda: IngestRow(40, 72)),
    "fullres_203x187_f64_linear": (FullresRow.tags, lambda: FullresRow(203, 187, "output_ab", "linear", "image")),
    "fullres_180x200_f32_nearest": (FullresRow.tags, lambda: FullresRow(180, 200, "input_ab", "nearest", "image")),
    "fullres_203x187_f32_linear": (FullresRow.tags, lambda: FullresRow(203, 187, "input_ab", "linear", "image")),
    "upsample_180x200_f64_cubic": (UpsampleRow.tags, lambda: UpsampleRow(180, 200, "output_ab", "cubic")),
    "upsample_203x187_f32_nearest": (UpsampleRow.tags, lambda: UpsampleRow(203, 187, "output_ab_raw", "nearest")),
    "upsample_203x187_f64_linear": (UpsampleRow.tags, lambda: UpsampleRow(203, 187, "output_ab", "linear")),
    "global_stats_256": (GlobalStatsRow.tags, GlobalStatsRow),
    "batch_130x97": (BatchRow.tags, lambda: BatchRow(130, 97)),
    "batch_203x187": (BatchRow.tags, lambda: BatchRow(203, 187)),
    "ragged_mixed": (RaggedRow.tags, RaggedRow),
    "eval_mixed": (EvalRow.tags, EvalRow),
    "range_audit_fp32": (AuditRow.tags, lambda: AuditRow("fp32")),
    "range_audit_fp16x3": (AuditRow.tags, lambda: AuditRow("fp16x3")),
    "op_f32_igemm_stride2_splitk": (SPLITK_TAGS, lambda: OpRow("f32_igemm_stride2_splitk", SPLITK_TAGS)),
    "op_bf16_igemm_splitk": (SPLITK_TAGS, lambda: OpRow("bf16_igemm_splitk", SPLITK_TAGS)),
    "op_bf16_f32out_splitk_1x1_529": (SPLITK_TAGS, lambda: OpRow("bf16_f32out_splitk_1x1_529", SPLITK_TAGS)),
    "op_f32_click_d2": (SPLITK_TAGS, lambda: OpRow("f32_click_d2", SPLITK_TAGS)),
    "op_bf16x3_v2ps_22_split_small": (SPLIT_TAGS, lambda: OpRow("bf16x3_v2ps_22_split_small", SPLIT_TAGS)),
    "op_fp16x3_v2psh_22_rule22": (SPLIT_TAGS, lambda: OpRow("fp16x3_v2psh_22_rule22", SPLIT_TAGS)),
    "pcie_click": (PcieRow.tags, PcieRow),
}


def test_every_tag_has_a_row():
    tags = engine.grid_tags()
    assert len(tags) == 21 and len(set(tags)) == 21
    covered = set(t for row_tags, _ in ROWS.values() for t in row_tags)
    assert not set(tags) - covered, "capped launch sites without a row: %s" % sorted(set(tags) - covered)
    assert not covered - set(tags), sorted(covered - set(tags))
    for t in tags:
        want, blocks = engine.grid_last(t)
        assert want >= 0 and blocks >= 0
    with pytest.raises(Exception):
        engine.grid_last("no_such_tag")
    with pytest.raises(Exception):
        engine.set_option("grid_cap", -1)


@pytest.mark.parametrize("row", sorted(ROWS))
def test_lowered_grid(row):
    tags, make = ROWS[row]
    r = make()
    assert tuple(r.tags) == tuple(tags)
    _drive(r)
