"""Antialiased ingestion without a device: the rule (tests/resample_ref.py, plain numpy float64) against torch's antialiased bilinear and
PIL's resize, ``colorspace.resize_antialias`` against the rule, the condition the GPU inputs have to meet, six mutants the exact
comparison catches, csrc/idc_resample.h and the batch plan through two stand-alone programs (plain and under ASan + UBSan: host programs,
nothing is loaded into Python), the ABI symbol, and the Python plumbing on stub engines.  Section 5: the cases on nets of their own
(resample_ref.NET_CASES) -- the tiling of csrc/idc_resample.h restated in Python and held equal to what ``resample_selftest in out channels``
prints, the path each case is named for asserted from it (chunks > 1, 1 < tw < 64, a ragged last tile, span == chunk), the tie condition,
idc_create's and the planner's answer for the narrow nets, and four mutants of the walk (H and W swapped, the sum restarted at a chunk, the
last chunk dropped, every tile given the first tile's windows) caught on every case they concern and invisible on the 64 x 64 cases."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import resample_ref as R
from conftest import REPO
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import api, colorspace, engine
from test_plan_cpu import plan_dump  # noqa: F401  (the module-scoped fixture that compiles tools/plan_dump.cpp)

CSRC = os.path.join(REPO, "interactive_deep_colorization_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MUTANTS = ["replicate", "unnormalised", "half_support", "centre", "float32", "round_first"]


# ------------------------------------------------------------------------------------------------ 1. the rule
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_the_restatement_is_torchs_antialiased_bilinear(name):
    import torch
    import torch.nn.functional as F
    src, v, _ = R.case(name)
    x = torch.from_numpy(np.ascontiguousarray(src.astype(np.float64).reshape(src.shape[0], src.shape[1], -1).transpose(2, 0, 1)))[None]
    y = F.interpolate(x, size=(R.H, R.W), mode="bilinear", antialias=True, align_corners=False)[0].numpy().transpose(1, 2, 0)
    err = float(np.abs(y - v.reshape(R.H, R.W, -1)).max())
    print("%s: restatement - torch %.3e" % (name, err))
    assert err <= 1e-10


@pytest.mark.parametrize("name", sorted(k for k, c in R.CASES.items() if c[3] == np.uint8))
def test_pil_is_within_one_level(name):
    from PIL import Image
    src, _, out = R.case(name)
    got = np.asarray(Image.fromarray(src).resize((R.W, R.H), Image.BILINEAR))
    d = np.abs(got.astype(np.int32) - out.astype(np.int32))
    print("%s: PIL differs on %.1f %% of the samples, by at most %d" % (name, 100.0 * (d > 0).mean(), d.max()))
    assert d.max() <= 1


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_the_host_twin_is_the_rule_exactly(name):
    src, _, out = R.case(name)
    got = colorspace.resize_antialias(src, R.H, R.W)
    assert got.dtype == src.dtype and got.shape == out.shape
    np.testing.assert_array_equal(got, out)
    if name in R.SAME:                              # not down-scaled: today's resize, bit for bit
        np.testing.assert_array_equal(got, colorspace.resize_bilinear_u8(src, R.H, R.W))
        np.testing.assert_array_equal(colorspace.resize_antialias(src[:, :, 1], R.H, R.W), colorspace.resize_bilinear_u8(src[:, :, 1], R.H, R.W))


def test_the_host_twin_takes_planes_and_refuses_other_types():
    src, _, out = R.case("rgb_211x83")
    np.testing.assert_array_equal(colorspace.resize_antialias(src[:, :, 2], R.H, R.W), out[:, :, 2])
    g16 = (src[:23, :31, 0].astype(np.uint16) * 257)    # a uint16 plane that is not down-scaled: the bilinear rule on the 16-bit lattice
    np.testing.assert_array_equal(colorspace.resize_antialias(g16, R.H, R.W), R.resample(g16)[1])
    other = colorspace.resize_antialias(src, 48, 80)    # down on one axis, up on the other, not square
    np.testing.assert_array_equal(other, R.resample(src, 48, 80)[1])
    for bad in (src.astype(np.float32), src.astype(np.int32), src[0, 0]):
        with pytest.raises(ValueError):
            colorspace.resize_antialias(bad, 8, 8)


@pytest.mark.parametrize("name", sorted(R.DOWN))
def test_gpu_inputs_keep_clear_of_rounding_ties(name):
    src, v, out = R.case(name)
    h, w, ch, dtype = R.CASES[name]
    assert src.dtype == dtype and src.shape == ((h, w, 3) if ch == 3 else (h, w))
    d = R.tie_distance(v if v.ndim == 3 else v[:, :, None])
    exempt = R.exempt_from_edge(name)
    print("%s: nearest value to a tie %.3e (%d samples decided by exact arithmetic)" % (name, d[~exempt].min(), int(exempt.sum()) * ch))
    assert R.meets_condition(name, v) and (d[~exempt] > R.EDGE).all()
    if name == "rgb_128x128":                       # the exempt samples: exact multiples of 1/64, ties among them
        inner = v[1:-1, 1:-1] * 64
        assert (inner == np.floor(inner)).all() and (d[1:-1, 1:-1] == 0).any()
    assert len(np.unique(out)) > 16                 # no constant image


def test_the_stripe_claim():
    g = R.stripes()
    b = colorspace.resize_bilinear_u8(g, R.H, R.W)
    a = R.resample(g)[1]
    print("stripes: bilinear %d..%d, tent %d..%d" % (b.min(), b.max(), a.min(), a.max()))
    assert b.min() == 16 and b.max() == 239
    assert a.min() >= 123 and a.max() <= 132
    np.testing.assert_array_equal(colorspace.resize_antialias(g, R.H, R.W), a)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_the_exact_comparison_catches_the_mutant(mutant):
    caught = {}
    for name in sorted(R.DOWN):
        src, _, out = R.case(name)
        caught[name] = int((R.resample(src, mutant=mutant)[1] != out).sum())
    print("%s: differing samples per input %s" % (mutant, caught))
    # The set of inputs has to catch each mutant.  float32 sums are off by ~1e-7 of the value times the root of the tap count: 1e-5..1e-4 levels
    # on uint8, which flips a sample only when it lies that close to a tie (about one sample in 1e4), but 1e-3..1e-2 on uint16: the 16-bit
    # planes are the inputs that have to show it.  The five mutants of the geometry move values by whole levels wherever their windows differ
    # from the rule's: replicated windows only at the border of an axis that is down-scaled by more than a tap, the others everywhere.
    assert sum(caught.values()) > 0, caught
    if mutant == "float32":
        assert caught["gray16_211x83"] and caught["gray16_700x300"], caught
    elif mutant == "round_first":               # (no mutant at all where the second pass is the identity or reads one column)
        assert sorted(k for k, v in caught.items() if not v) == ["rgb_1000x1", "rgb_1x1000", "rgb_65x64"], caught
    elif mutant == "replicate":                 # (65 -> 64: the window at the border is already inside the image)
        assert sorted(k for k, v in caught.items() if not v) == ["rgb_65x64"], caught
    else:
        assert all(caught.values()), caught


# ------------------------------------------------------------------------------------------------ 2. the header and the plan
def _make(target, out, san):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc (%s): tools/%s.cpp cannot be compiled" % (HIPCC, target))
    cmd = ["make", "-C", CSRC, target, "BINDIR=" + out, "HIPCC=" + HIPCC] + (["SAN=1"] if san else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return os.path.join(out, target)


@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan_ubsan"])
def test_window_and_tiling_arithmetic(tmp_path, san):
    run = subprocess.run([_make("resample_selftest", str(tmp_path), san)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("resample_selftest: ok ("), run.stdout + run.stderr


def test_the_header_is_plain_cpp():
    text = open(os.path.join(CSRC, "idc_resample.h")).read()
    # tools/resample_selftest.cpp includes it alone: no header of its own, no runtime call, no kernel
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", text) == [] and "__global__" not in text and not re.search(r"\bhip[A-Z]\w+\(", text)


@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan_ubsan"])
def test_the_plan_off_is_todays_and_on_has_the_ingestion_view(tmp_path, san):
    run = subprocess.run([_make("resample_plan_selftest", str(tmp_path), san)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert lines[-1] == "resample_plan_selftest: ok (12 calls)", run.stdout + run.stderr
    golden = open(os.path.join(REPO, "tests", "golden", "resample_plan_off.txt")).read().splitlines()
    assert lines[:-1] == golden


def test_no_grid_tag_was_added():
    text = open(os.path.join(CSRC, "idc_resample.hip")).read()
    assert "grid_blocks" not in text and "gridDim" not in text           # an exact grid: no cap, no grid-stride loop
    assert len(re.findall(r"hipLaunchKernelGGL\(", text)) == 3 and text.count("resample_kernel<") == 3


# ------------------------------------------------------------------------------------------------ 3. the ABI
def test_abi_symbol_and_statuses():
    header = open(os.path.join(REPO, "include", "ideepcolor.h")).read()
    assert re.search(r"\bint\s+idc_set_ingest_filter\s*\(\s*idc_handle\s+h\s*,\s*int\s+filter\s*\)\s*;", header)
    assert re.search(r"enum\s*\{\s*IDC_FILTER_BILINEAR\s*=\s*0\s*,\s*IDC_FILTER_ANTIALIAS\s*=\s*1\s*\}", header)
    assert "idc_set_ingest_filter" in N.EXPORTED_SYMBOLS and (N.IDC_FILTER_BILINEAR, N.IDC_FILTER_ANTIALIAS) == (0, 1)
    lib = N.load()
    assert hasattr(lib, "idc_set_ingest_filter")
    assert lib.idc_set_ingest_filter(None, N.IDC_FILTER_ANTIALIAS) == -1      # a null handle, without a device
    for line in ("c = (i + 0.5) * s", "lo = max(0, (int)(c - s + 0.5))", "hi = min(in, (int)(c + s + 0.5))", "r_k = max(0, 1 - |k + 0.5 - c| / s)",
                 "tot = sum of r_k in ascending k", "weight_k = r_k / tot"):
        assert line in header, line


# ------------------------------------------------------------------------------------------------ 4. the Python plumbing
class _Lib(object):
    def __init__(self):
        self.calls = []

    def idc_set_ingest_filter(self, h, f):
        self.calls.append(f)
        return 0


class _Pool(object):
    def take(self, shape, dtype):
        return np.zeros(shape, dtype)


class _Stub(engine.HipColorizer):
    """The streaming generators over an engine that launches nothing: every enqueue records the two settings in force."""

    def __init__(self, fail_after=None):
        self.H, self.W, self.max_batch = 8, 8, 2
        self._batch_upsample, self._ingest_filter = "linear", "bilinear"
        self._pool, self.lib, self._h = _Pool(), _Lib(), None
        self.seen, self.fail_after = [], fail_after

    def __del__(self):
        pass

    def _chk(self, rc):
        assert rc == 0

    def set_batch_upsample(self, interp="linear"):
        if interp not in ("linear", "joint"):
            raise ValueError(interp)
        self._batch_upsample = interp

    def _pinned_slices(self, shapes):
        return [np.zeros(s, np.uint8) for s in shapes]

    def wait(self, slot):
        pass

    def dist_bins(self):
        return 313

    def _enqueue(self):
        if self.fail_after is not None and len(self.seen) >= self.fail_after:
            raise RuntimeError("enqueue refused")
        self.seen.append((self._ingest_filter, self._batch_upsample))

    def forward_async_rgb(self, slot, rgb, hints, out_rgb, **kw):
        self._enqueue()

    def forward_async_images(self, slot, images, hints, **kw):
        self._enqueue()
        return [np.zeros(a.shape, np.uint8) for a in images]

    def forward_async_gray(self, slot, images, hints, **kw):
        self._enqueue()
        if kw.get("peaks") is not None or kw.get("bin_centres") is not None:
            return self._dist(images)
        return [np.zeros(a.shape + (3,), np.uint8) for a in images]

    def forward_async_eval(self, slot, images, hints, **kw):
        self._enqueue()
        return np.zeros((len(images), 3), np.uint64), None, None

    def _dist(self, images):
        n, res = len(images), engine.DistBatch()
        res.out_rgb = [np.zeros(a.shape[:2] + (3,), np.uint8) for a in images]
        res.peaks, res.sugg_centres, res.sugg_conf = np.zeros((n, 2, 2), np.int32), np.zeros((n * 2, 3, 2)), np.zeros((n * 2, 3))
        res.peak_ent = np.zeros((n, 2), np.float32)
        res.sse, res.score = np.zeros((n, 3), np.uint64), engine.DistScore()
        res.score.xent, res.score.hits, res.score.cells = np.zeros(n), np.zeros((n, 2), np.uint32), 4
        return res

    def forward_async_dist(self, slot, images, hints, **kw):
        self._enqueue()
        return self._dist(images)


GENERATORS = ["colorize_stream", "colorize_images", "evaluate_images", "suggest_images", "score_images", "colorize_gray", "suggest_gray"]


def _generator(e, name, ingest, upsample=None):
    img, g = np.zeros((5, 7, 3), np.uint8), np.zeros((5, 7), np.uint8)
    items, c = [img] * 5, np.zeros((313, 2), np.float32)         # three batches of at most two
    return {
        "colorize_stream": lambda: e.colorize_stream([(img[None], None)] * 3, out="source", ingest=ingest, upsample=upsample),
        "colorize_images": lambda: e.colorize_images(items, ingest=ingest, upsample=upsample),
        "evaluate_images": lambda: e.evaluate_images(items, out="source", ingest=ingest, upsample=upsample),
        "suggest_images": lambda: e.suggest_images(items, c, peaks=2, K=3, ingest=ingest, upsample=upsample),
        "score_images": lambda: e.score_images(items, c, ingest=ingest, upsample=upsample),
        "colorize_gray": lambda: e.colorize_gray([g] * 5, ingest=ingest, upsample=upsample),
        "suggest_gray": lambda: e.suggest_gray([g] * 5, c, peaks=2, K=3, ingest=ingest, upsample=upsample),
    }[name]()


def test_set_ingest_filter_reaches_the_library():
    e = _Stub()
    e.set_ingest_filter("antialias")
    e.set_ingest_filter("bilinear")
    e.set_ingest_filter()
    assert e.lib.calls == [1, 0, 0] and e._ingest_filter == "bilinear"
    with pytest.raises(ValueError):
        e.set_ingest_filter("cubic")
    assert e.lib.calls == [1, 0, 0]


@pytest.mark.parametrize("name", GENERATORS)
def test_the_ingest_keyword_sets_and_restores_the_state(name):
    # run to the end: set before the first batch, every batch sees it, the previous setting is back afterwards
    e = _Stub()
    results = list(_generator(e, name, "antialias"))
    assert len(results) in (3, 5) and e.seen == [("antialias", "linear")] * 3 and e.lib.calls == [1, 0] and e._ingest_filter == "bilinear"
    # a previous 'antialias' is what comes back, and None touches nothing
    e = _Stub()
    e.set_ingest_filter("antialias")
    list(_generator(e, name, "bilinear"))
    assert e.lib.calls == [1, 0, 1] and set(e.seen) == {("bilinear", "linear")}
    e.lib.calls, e.seen = [], []
    list(_generator(e, name, None))
    assert e.lib.calls == [] and set(e.seen) == {("antialias", "linear")}
    # together with upsample=: both are set, both come back
    e = _Stub()
    list(_generator(e, name, "antialias", "joint"))
    assert set(e.seen) == {("antialias", "joint")} and (e._ingest_filter, e._batch_upsample) == ("bilinear", "linear")
    # abandoned after the first result: restored when the generator is closed
    e = _Stub()
    g = _generator(e, name, "antialias")
    assert e.lib.calls == []                                # nothing happens before the first next()
    next(g)
    assert e._ingest_filter == "antialias"
    g.close()
    assert e.lib.calls == [1, 0] and e._ingest_filter == "bilinear"
    # an exception on the way: restored as well
    e = _Stub(fail_after=1)
    with pytest.raises(RuntimeError):
        list(_generator(e, name, "antialias", "joint"))
    assert e.seen == [("antialias", "joint")] and (e._ingest_filter, e._batch_upsample) == ("bilinear", "linear")
    # a value that is neither is refused before anything is enqueued, and a set upsample goes back
    e = _Stub()
    with pytest.raises(ValueError):
        next(_generator(e, name, "cubic", "joint"))
    assert e.seen == [] and (e._ingest_filter, e._batch_upsample) == ("bilinear", "linear")


class _Net(object):
    """What ColorizeImageBase's device ingestion needs of an engine, on the host: records the filter in force at each call."""

    def __init__(self):
        self._ingest_filter, self.seen, self.l_serial = "bilinear", [], 0

    def set_ingest_filter(self, name):
        self._ingest_filter = name

    def set_image_rgb(self, rgb, img=0, l_cent=50.0, keep_source=False):
        self.seen.append(("rgb", self._ingest_filter))
        resize = colorspace.resize_antialias if self._ingest_filter == "antialias" else colorspace.resize_bilinear_u8
        net = resize(rgb, 16, 16)
        return net[None], colorspace.rgb2lab(net).transpose((2, 0, 1))[None]

    def set_image_gray(self, gray, img=0, l_cent=50.0, keep_source=False):
        self.seen.append(("gray", self._ingest_filter))
        net = colorspace.resize_antialias(gray, 16, 16)
        return net[None], np.zeros((1, 16, 16))


def test_the_wrapper_passes_the_filter_on(tmp_path):
    from PIL import Image
    model = api.ColorizeImageTorch(Xd=16)
    model.Xfullres_max = 100
    with pytest.raises(ValueError):
        model.set_ingest_filter("cubic")
    model.set_ingest_filter("antialias")                    # before there is an engine: remembered
    model.net, model.net_set = _Net(), True
    src = R.case("rgb_40x100")[0]
    model.set_image_device(src)
    assert model.net.seen == [("rgb", "antialias")]
    np.testing.assert_array_equal(model.img_rgb, colorspace.resize_antialias(src, 16, 16))
    model.set_image_device(src[:, :, 0].copy())
    assert model.net.seen[-1] == ("gray", "antialias")
    # the host route of a source beyond Xfullres_max follows the filter; load_image, the reference's own method, does not
    big = R.case("rgb_211x83")[0]
    path = str(tmp_path / "big.png")
    Image.fromarray(big).save(path)
    model.load_image_device(path)
    assert len(model.net.seen) == 2
    np.testing.assert_array_equal(model.img_rgb, colorspace.resize_antialias(big, 16, 16))
    model.load_image(path)
    np.testing.assert_array_equal(model.img_rgb, colorspace.resize_bilinear_u8(big, 16, 16))
    model.set_ingest_filter("bilinear")
    assert model.net._ingest_filter == "bilinear"
    model.load_image_device(path)
    np.testing.assert_array_equal(model.img_rgb, colorspace.resize_bilinear_u8(big, 16, 16))
    model.set_image_device(src)
    assert model.net.seen[-1] == ("rgb", "bilinear")


# ------------------------------------------------------------------------------------------------ 5. nets of their own, and the rare tilings
NET = sorted(R.NET_CASES)
NARROW_NETS = [(16, 8), (8, 24), (24, 16), (40, 72), (72, 40)]
NET_MUTANTS = ["transposed_net"] + R.TILE_MUTANTS


def _tiles(name):
    (_, net_w), _, w, ch, _ = R.spec(name)
    return R.tiles_of(w, net_w, ch)


@pytest.mark.parametrize("name", NET)
def test_net_cases_are_torchs_antialiased_bilinear_and_the_host_twin(name):
    import torch
    import torch.nn.functional as F
    (net_h, net_w), h, w, ch, dtype = R.spec(name)
    src, v, out = R.case(name)
    assert src.dtype == dtype and src.shape == ((h, w, 3) if ch == 3 else (h, w)) and out.shape[:2] == (net_h, net_w)
    x = torch.from_numpy(np.ascontiguousarray(src.astype(np.float64).reshape(h, w, -1).transpose(2, 0, 1)))[None]
    y = F.interpolate(x, size=(net_h, net_w), mode="bilinear", antialias=True, align_corners=False)[0].numpy().transpose(1, 2, 0)
    err = float(np.abs(y - v.reshape(net_h, net_w, -1)).max())
    print("%s: restatement - torch %.3e" % (name, err))
    assert err <= 1e-10 * (257 if dtype == np.uint16 else 1)       # (the existing bar, which is for 8-bit magnitudes, scaled to 65535)
    np.testing.assert_array_equal(colorspace.resize_antialias(src, net_h, net_w), out)


@pytest.mark.parametrize("name", NET)
def test_net_cases_keep_clear_of_rounding_ties(name):
    src, v, out = R.case(name)
    d = R.tie_distance(v)
    print("%s: nearest value to a tie %.3e, %d levels" % (name, d.min(), len(np.unique(out))))
    assert not R.exempt_from_edge(name).any() and R.meets_condition(name, v) and (d > R.EDGE).all()
    assert len(np.unique(out)) > 16                 # no constant image


@pytest.mark.parametrize("name", NET)
def test_net_cases_take_the_path_they_are_named_for(name):
    (_, net_w), _, w, ch, _ = R.spec(name)
    want = R.PATHS[name]
    tw, tiles = _tiles(name)
    cols = R.chunk_cols(ch)
    got = dict(tw=tw, tiles=len(tiles), spans=sorted({t[3] - t[2] for t in tiles}), chunks=sorted({len(t[4]) for t in tiles}),
               last=sorted({t[4][-1][1] - t[4][-1][0] for t in tiles}), last_tile=tiles[-1][1] - tiles[-1][0])
    print("%s: %s" % (name, got))
    assert {k: got[k] for k in want} == want
    assert R.tiling(w, net_w, ch) == (tw, len(tiles), max(got["chunks"]))
    if "chunks" in want:                            # a one-column tile whose window alone is the span
        assert tw == 1 and all(t[1] - t[0] == 1 for t in tiles)
        if ch == 3:
            assert max(got["chunks"]) > 1 and cols == 1365 and all(sum(c1 - c0 for c0, c1 in t[4]) == t[3] - t[2] for t in tiles)
        else:                                       # one channel: the largest span IS the chunk, and no span is chunked
            assert got["chunks"] == [1] and max(got["spans"]) == cols == R.CHUNK_ELEMS
    else:
        assert got["chunks"] == [1]
        if net_w == 64 or len(tiles) > 1:           # several column tiles of three channels: i0 > 0 and a reduced tile width, or a net past 64
            assert len(tiles) > 1 and (1 < tw < 64 or net_w > 64) and (ch == 3 or net_w > 64)
    ragged = [n for n in NET if R.PATHS[n].get("last_tile", 99) < R.PATHS[n]["tw"]]
    assert "n64x64_rgb_5x4099" in ragged and "n64x64_rgb_2x1400" in ragged and "n40x72_rgb_211x83" in ragged
    if name in R.LEAN:                              # the sample that leans on the one-column chunk: dropping that column flips it
        y, x, c = R.lean_on_the_last_column(name, np.array(R.case(name)[0]))
        src, v, out = R.case(name)
        ks, ws = R.taps(x, w, net_w)
        adds = ws[-1] * float(src[0, ks[-1], c])
        assert len(tiles[x][4]) == 2 and tiles[x][4][1] == (ks[-1], ks[-1] + 1)
        assert np.floor(v[y, x, c] + 0.5) == np.floor(v[y, x, c] - adds + 0.5) + 1 and R.tie_distance(v)[y, x, c] > 10 * R.EDGE


def test_the_chunked_path_needs_three_channels_and_a_net_at_most_24_wide():
    # sources end at 16384 a side: a window of more than 1365 columns needs s > 682, which 16384 / W gives for W <= 24 only; one channel's
    # chunk is 4096 columns, which the widest window of the narrowest net (16384 -> 8: s = 2048) fills exactly and does not pass
    for net_w in (8, 16, 24, 32, 64, 72):
        assert (R.tiling(16384, net_w, 3)[2] > 1) == (net_w <= 24), net_w
        assert R.tiling(16384, net_w, 1)[2] == 1
    assert max(c1 - c0 for _, _, c0, c1, _ in R.tiles_of(16384, 8, 1)[1]) == R.chunk_cols(1)
    assert R.tiling(16384, 4, 1)[2] == 2            # (no net: the header's "s > 2047 with one" needs a width idc_create refuses)


def test_the_tiling_restatement_is_the_headers(tmp_path):
    triples = sorted({(w, net[1], ch) for net, _, w, ch, _ in R.NET_CASES.values()} | {(w, R.W, ch) for _, w, ch, _ in R.CASES.values()} |
                     {(16384, 1, 3), (16384, 1, 1), (16384, 24, 3), (16384, 32, 3), (16383, 8, 3), (6000, 8, 1)})
    args = [str(v) for t in triples for v in t]
    run = subprocess.run([_make("resample_selftest", str(tmp_path), False)] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    got = [tuple(int(v) for v in line.split()) for line in run.stdout.splitlines()]
    assert got == [R.tiling(*t) for t in triples], [(t, g, R.tiling(*t)) for t, g in zip(triples, got) if g != R.tiling(*t)]
    bad = subprocess.run([os.path.join(str(tmp_path), "resample_selftest"), "16385", "8", "3"], capture_output=True, text=True)
    assert bad.returncode == 2 and bad.stdout == ""


def test_the_plan_takes_the_narrow_nets(plan_dump):
    """include/ideepcolor.h promises any positive multiples of 8: idc_create gets past its checks of the geometry for the nets of NET_CASES
    (a device index that does not exist is then IDC_ERR_NO_DEVICE on any machine), and the planner plans a forward for each."""
    import ctypes
    lib = N.load()
    h = ctypes.c_void_p()
    for net_h, net_w in NARROW_NETS + [(16, 24)]:
        assert lib.idc_create(-1, net_h, net_w, 4, N.IDC_BF16, 0, ctypes.byref(h)) == -2 and not h, (net_h, net_w, lib.idc_last_error(None))
        run = subprocess.run([plan_dump, "bf16", "0", str(net_h), str(net_w), "4", "1"], capture_output=True, text=True)
        assert run.returncode == 0 and "\nconv10_2\t" in run.stdout, (net_h, net_w, run.stderr)
    assert lib.idc_create(-1, 16, 12, 4, N.IDC_BF16, 0, ctypes.byref(h)) == -1
    assert {R.spec(n)[0] for n in NET} == set(NARROW_NETS) | {(16, 24), (64, 64)}


def _concerns(mutant, name):
    (net_h, net_w), _, w, ch, _ = R.spec(name)
    tw, tiles = _tiles(name)
    if mutant == "transposed_net":
        return net_h != net_w
    if mutant == "first_tile_only":
        return len(tiles) > 1
    return max(len(t[4]) for t in tiles) > 1


@pytest.mark.parametrize("mutant", NET_MUTANTS)
def test_the_net_cases_catch_the_mutant(mutant):
    caught = {}
    for name in NET:
        if _concerns(mutant, name):
            src, _, out = R.case(name)
            net_h, net_w = R.spec(name)[0]
            caught[name] = int((R.resample(src, net_h, net_w, mutant=mutant)[1] != out).sum())
    print("%s: differing samples per input %s" % (mutant, caught))
    assert len(caught) >= 4 and all(caught.values()), caught
    # ... and the 64 x 64 net cannot see a swap of H and W, nor can one chunk and one tile see theirs: that is what the cases are for
    blind = sorted(R.DOWN) if mutant == "transposed_net" else ["rgb_211x83", "rgb_1x1000", "gray16_211x83"]
    for name in blind:
        src, _, out = R.case(name)
        assert not _concerns(mutant, name)
        np.testing.assert_array_equal(R.resample(src, mutant=mutant)[1], out)
