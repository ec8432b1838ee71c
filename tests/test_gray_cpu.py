"""Greyscale sources, the parts that need no GPU: the C-ABI symbols against the header, tests/gray_ref.py against code that exists (the
wrapper's resize, its rgb2lab and the oracle's), the identity (I16) in float64, the conditions the GPU file's inputs have to meet, the
mutants of gray_ref that the GPU file's comparisons have to catch, the plan of a greyscale batch (tools/gray_plan_selftest.cpp, plain and
under the address and undefined-behaviour sanitizers), and the marshalling of HipColorizer.set_image_gray / fullres_rgb(depth=) /
forward_async_gray and the generators colorize_gray / suggest_gray on an engine that calls no library.  The inputs of the 40 x 72 net
(gray_ref.NET) are held to the same rounding condition, and a swap of H and W is shown to be caught on each of them and on none of the 64 x 64
net's."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import gray_ref as G
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import colorspace, engine
from oracle import colorspace as ocs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "interactive_deep_colorization_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW = ("idc_set_image_gray", "idc_fullres_rgb16", "idc_forward_async_gray")


# ------------------------------------------------------------------------------------------------ 1. ABI
def test_the_symbols_match_the_header():
    header = open(os.path.join(REPO, "include", "ideepcolor.h")).read()
    declared = set(re.findall(r"\b(idc_[a-z0-9_]+)\s*\(", header))
    lib = N.load()
    for sym in NEW:
        assert sym in declared and sym in N.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    assert lib.idc_version() == 2
    m = re.search(r"int\s+idc_set_image_gray\s*\(([^;]*)\);", header)
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert len(args.split(",")) == len(lib.idc_set_image_gray.argtypes) == 11
    assert len(lib.idc_fullres_rgb16.argtypes) == 5
    m = re.search(r"int\s+idc_forward_async_gray\s*\(([^;]*)\);", header)
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert len(args.split(",")) == len(lib.idc_forward_async_gray.argtypes) == 16
    assert re.search(r"enum\s*\{\s*IDC_BATCH_OUT_RGB16\s*=\s*2\s*\}", header) and N.IDC_BATCH_OUT_RGB16 == 2 and N.IDC_BATCH_OUT_SOURCE == 1
    # typedef struct idc_gray_image { const void* pix; int32_t h, w; }: a pointer and two int32, 16 bytes
    assert re.search(r"typedef struct idc_gray_image \{ const void\* pix; int32_t h, w; \} idc_gray_image;", header)
    assert ctypes.sizeof(N.GrayImage) == 16 and [f[0] for f in N.GrayImage._fields_] == ["pix", "h", "w"]
    assert (N.GrayImage.pix.offset, N.GrayImage.h.offset, N.GrayImage.w.offset) == (0, 8, 12)
    for phrase in ("v / 255.0 or v / 65535.0", "(uint16)(s * 65535.0)", "fl(257 g / 65535) == fl(g / 255)", "no colour to reveal or to score against"):
        assert phrase in header, phrase


def test_null_handle_statuses():
    lib = N.load()
    buf = np.zeros(6, np.uint16)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.idc_set_image_gray(None, 0, 1, 1, 1, 16, p, 50.0, 0, None, None) == -1
    assert lib.idc_fullres_rgb16(None, 0, 0, 1, p) == -1
    assert lib.idc_forward_async_gray(None, 0, 1, 16, None, None, None, 0, 1.0, 0.0, 50.0, 0, None, None, None, None) == -1


# ------------------------------------------------------------------------------------------------ 1b. the plan
@pytest.fixture(scope="module", params=["plain", "san"])
def gray_plan_selftest(request, tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc (%s): tools/gray_plan_selftest.cpp cannot be compiled" % HIPCC)
    out = str(tmp_path_factory.mktemp("gray_plan_selftest_" + request.param))
    cmd = ["make", "-C", CSRC, "gray_plan_selftest", "BINDIR=" + out, "HIPCC=" + HIPCC] + (["SAN=1"] if request.param == "san" else [])
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return os.path.join(out, "gray_plan_selftest")


def test_gray_plan_layouts_refusals_copy_runs_and_table(gray_plan_selftest):
    run = subprocess.run([gray_plan_selftest], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("gray_plan_selftest: ok"), run.stdout + run.stderr


# ------------------------------------------------------------------------------------------------ 2. the reference against existing code
@pytest.mark.parametrize("size", G.SIZES + [(300, 17)])
def test_the_8_bit_resize_is_the_wrappers(size):
    g = G.gray8(*size) if max(size) <= 256 else np.random.RandomState(3).randint(0, 256, size).astype(np.uint8)
    want = colorspace.resize_bilinear_u8(np.repeat(g[..., None], 3, 2), G.H, G.W)
    got = G.resize(g)
    assert got.dtype == np.uint8
    for c in range(3):
        np.testing.assert_array_equal(got, want[..., c])


def test_the_lightness_is_rgb2labs():
    # bar: L is 116 f(y) - 16 with y a three-term sum of products below 1; the two sides may add the terms in another order, which moves y by
    # at most 2 ulp (4.4e-16 relative) and L by 116 / 3 of that: 1e-12 leaves more than a decade
    g = np.arange(256, dtype=np.uint8).reshape(16, 16)
    rep = np.repeat(g[..., None], 3, 2)
    for want in (colorspace.rgb2lab(rep)[..., 0], ocs.rgb2lab(rep)[..., 0]):
        assert float(np.abs(G.lightness(g) - want).max()) <= 1e-12
    # and the way back: the reference's Lab -> sRGB against the oracle's
    ab = np.stack([np.linspace(-60, 60, 256).reshape(16, 16), np.linspace(40, -40, 256).reshape(16, 16)])
    L = G.lightness(g)
    want = ocs.lab2rgb(np.concatenate([L[None], ab]).transpose((1, 2, 0)))
    assert float(np.abs(G.lab_to_srgb(L, ab) - want).max()) <= 1e-12
    np.testing.assert_array_equal(G.image(g, ab, 8), ocs.lab2rgb_transpose(L[None], ab))


def test_identity_i16_for_all_256_values():
    g = np.arange(256, dtype=np.uint8)
    g16 = (257 * g.astype(np.uint32)).astype(np.uint16)
    np.testing.assert_array_equal(g16.astype(np.float64) / 65535.0, g.astype(np.float64) / 255.0)
    np.testing.assert_array_equal(G.lightness(g16[None]), G.lightness(g[None]))
    assert g16[255] == 65535 and np.array_equal(g16 >> 8, g)


# ------------------------------------------------------------------------------------------------ 3. the GPU file's inputs
@pytest.mark.parametrize("size", G.SIZES)
def test_gpu_inputs_stay_away_from_rounding_boundaries(size):
    for g in (G.gray16(*size), G.gray8(*size)):
        v = G.resize_unrounded(g, G.H, G.W) + 0.5
        assert float(np.abs(v - np.round(v)).min()) > 1e-6, (size, g.dtype)


def test_gpu_inputs_use_the_low_byte_and_every_residue():
    for size in G.SIZES:
        g = G.gray16(*size)
        assert (g % 257 != 0).any() or size == (1, 1), size
    assert (G.gray16(211, 83) & 255).std() > 50
    assert len({(sh * sw) % 4 for sh, sw in G.SIZES}) == 4          # the tail of the flat run: 0..3 pixels through narrow accesses
    assert sorted(G.BATCH) == sorted(G.SIZES)
    assert sorted(set(s % 4 for s in G.starts(G.BATCH))) == [0, 1, 2, 3]       # image starts in the packed run, the same in both widths
    assert sum(h * w for h, w in G.BATCH) % 4 == 1                  # ... and the run itself ends on a narrow tail
    r = G.ramp16()
    assert r.shape == (211, 83) and len(np.unique(r)) == 300 and int(r.max()) - int(r.min()) == 299
    assert len(np.unique(r >> 8)) <= 2


@pytest.mark.parametrize("size", G.NET_SIZES)
def test_the_40x72_net_inputs_stay_away_from_rounding_boundaries_and_show_a_swap(size):
    H, W = G.NET
    for g in (G.gray16(*size, net=G.NET), G.gray8(*size, net=G.NET)):
        assert g.shape == size
        v = G.resize_unrounded(g, H, W) + 0.5
        assert float(np.abs(v - np.round(v)).min()) > 1e-6, (size, g.dtype)
        net = G.resize(g, H, W)
        assert net.shape == (H, W) and net.dtype == g.dtype
        if size == G.NET:
            np.testing.assert_array_equal(net, g)                               # the net's own size: the identity
        # 'transposed_net' is caught by the exact comparison of the net plane and by l_net, on every entry ...
        swapped = G.resize(g, H, W, variant="transposed_net")
        assert swapped.shape == net.shape and not G.same(swapped, net)[0]
        assert not G.close(G.lightness(swapped), G.lightness(net), G.L_TOL)[0]
    assert (G.gray16(*size, net=G.NET) % 257 != 0).any()
    # ... and by no comparison on the 64 x 64 net, whatever the plane
    for s in G.SIZES:
        np.testing.assert_array_equal(G.resize(G.gray16(*s), variant="transposed_net"), G.resize(G.gray16(*s)))
    assert all(0 <= r[0] <= r[2] < H and 0 <= r[1] <= r[3] < W for r in G.NET_HINTS)
    np.testing.assert_array_equal(G.gray16(23, 31), G.gray16(23, 31, net=None))     # today's draws are as they were
    assert not np.array_equal(G.gray16(23, 31), G.gray16(23, 31, net=G.NET))


# ------------------------------------------------------------------------------------------------ 4. mutants
def _ab(size):
    rs = np.random.RandomState(5)
    return rs.uniform(-60, 60, (2,) + size)


@pytest.mark.parametrize("variant", ["drop8", "scale65536", "round_out", "resize8"])
def test_the_comparisons_catch_the_mutant(variant):
    """Each comparison of the GPU file is run with the unmutated reference in the device's place and the mutant as the reference."""
    caught = []
    for size in [(23, 31), (211, 83)]:
        g = G.gray16(*size)
        ab = _ab(size)
        net, net_m = G.resize(g), G.resize(g, variant=variant)
        checks = {
            "gray_net": G.same(net, net_m)[0],
            "l_net": G.close(G.lightness(net), G.lightness(net_m, variant), G.L_TOL)[0],
            "image16": G.image16_matches(G.image(g, ab, 16), g, ab, variant)[0],
        }
        caught += [k for k, ok in checks.items() if not ok]
        assert G.image16_matches(G.image(g, ab, 16), g, ab)[0]                  # (and the comparison passes what it should)
    print("%s: caught by %s" % (variant, sorted(set(caught))))
    assert caught, variant
    expected = {"drop8": "l_net", "scale65536": "l_net", "round_out": "image16", "resize8": "gray_net"}[variant]
    assert expected in caught, (variant, caught)


# ------------------------------------------------------------------------------------------------ 5. marshalling
class _Pool(object):
    def take(self, shape, dtype):
        return np.zeros(shape, dtype)


class _Lib(object):
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name,) + args)
            return 0
        return call


class _Stub(engine.HipColorizer):
    def __init__(self):
        self.H, self.W, self.max_batch = 8, 8, 2
        self._pool, self.lib, self._h = _Pool(), _Lib(), None
        self._src_shape, self.l_serial = {}, 0

    def __del__(self):
        pass

    def _chk(self, status):
        assert status == 0


def test_set_image_gray_refuses_dtypes_and_shapes_before_the_library():
    e = _Stub()
    for bad in (np.zeros((4, 4), np.float32), np.zeros((4, 4), np.int16), np.zeros((4, 4), np.uint32), np.zeros((4, 4, 3), np.uint8)[..., None],
                np.zeros(4, np.uint8)):
        with pytest.raises(ValueError):
            e.set_image_gray(bad)
    assert e.lib.calls == []
    with pytest.raises(ValueError):
        e.fullres_rgb(depth=12)
    with pytest.raises(ValueError):
        e.fullres_rgb(l_mode="mask50", depth=16)
    assert e.lib.calls == []


def test_set_image_gray_passes_the_dtype_as_the_format():
    e = _Stub()
    for dtype, bits in ((np.uint8, 8), (np.uint16, 16)):
        e.lib.calls = []
        net, l_net = e.set_image_gray(np.zeros((2, 5, 7), dtype), img=0, keep_source=True)
        name, _h, img, n, sh, sw, b = e.lib.calls[0][:7]
        assert (name, img, n, sh, sw, b) == ("idc_set_image_gray", 0, 2, 5, 7, bits)
        assert net.dtype == dtype and net.shape == (2, 8, 8) and l_net.shape == (2, 8, 8) and l_net.dtype == np.float64
        assert e._src_shape == {0: (5, 7), 1: (5, 7)}
    # a view that is not contiguous (every other column of uint16: odd strides for the library) is packed first
    g = np.arange(40, dtype=np.uint16).reshape(4, 10)[:, ::2]
    e.lib.calls = []
    e.set_image_gray(g, want_net=False, want_l=False)
    assert e.lib.calls[0][4:6] == (4, 5) and e.lib.calls[0][7].value % 2 == 0 and e._src_shape.get(0) is None
    # depth: the 16-bit getter is its own call and returns uint16
    e.set_image_gray(np.zeros((5, 7), np.uint16), keep_source=True)
    e.lib.calls = []
    out = e.fullres_rgb("no_ab", "linear", depth=16)
    assert e.lib.calls[0][0] == "idc_fullres_rgb16" and out.dtype == np.uint16 and out.shape == (5, 7, 3)
    out = e.fullres_rgb("no_ab", "linear")
    assert e.lib.calls[1][0] == "idc_fullres_rgb" and out.dtype == np.uint8


# ------------------------------------------------------------------------------------------------ 6. the pipelined call and the generators
class _Stream(engine.HipColorizer):
    """The streaming generators over an engine that launches nothing: every enqueue records its slot, dtypes and the upsampling in force."""

    def __init__(self):
        self.H, self.W, self.max_batch = 8, 8, 3
        self._batch_upsample = "linear"
        self._pool, self.lib, self._h = _Pool(), _Lib(), None
        self._in_flight = {}
        self.calls, self.seen, self.busy = [], [], set()

    def __del__(self):
        pass

    def _chk(self, status):
        assert status == 0

    def set_batch_upsample(self, interp="linear"):
        if interp not in ("linear", "joint"):
            raise ValueError(interp)
        self.calls.append(interp)
        self._batch_upsample = interp

    def _pinned_slices(self, shapes):
        return [np.zeros(s, np.uint8) for s in shapes]

    def wait(self, slot):
        self.busy.discard(slot)

    def dist_bins(self):
        return 313

    def forward_async_gray(self, slot, images, hints, **kw):
        assert slot not in self.busy                      # a slot is waited for before it is used again
        self.busy.add(slot)
        for a in images:
            assert a.ctypes.data % a.dtype.itemsize == 0 and a.flags.c_contiguous
        self.seen.append((slot, [a.dtype.name for a in images], [a.shape for a in images], self._batch_upsample, kw.get("depth", 8)))
        odt = np.uint16 if kw.get("depth", 8) == 16 else np.uint8
        outs = [np.full(a.shape + (3,), len(self.seen), odt) for a in images]
        if not kw.get("peaks"):
            return outs
        res, n, P = engine.DistBatch(), len(images), kw["peaks"]
        res.out_rgb = outs
        res.peaks, res.sugg_centres, res.sugg_conf = np.zeros((n, P, 2), np.int32), np.zeros((n * P, kw["K"], 2)), np.zeros((n * P, kw["K"]))
        return res


def _items():
    a, b = np.zeros((5, 7), np.uint8), np.zeros((3, 3), np.uint16)
    return [a, a, (b, None), b, b, b, a]                   # groups of at most three: [a a] [b b b] [b] [a]


def test_the_generators_group_by_dtype_alternate_slots_and_keep_the_order():
    e = _Stream()
    res = list(e.colorize_gray(_items()))
    assert [(s[0], s[1]) for s in e.seen] == [(0, ["uint8"] * 2), (1, ["uint16"] * 3), (0, ["uint16"]), (1, ["uint8"])]
    assert [r.shape for r in res] == [(5, 7, 3)] * 2 + [(3, 3, 3)] * 4 + [(5, 7, 3)]
    assert [int(r[0, 0, 0]) for r in res] == [1, 1, 2, 2, 2, 3, 4]                 # each result from its own batch, in input order
    assert not e.busy and e.calls == []
    e = _Stream()
    c = np.zeros((313, 2), np.float32)
    res = list(e.suggest_gray(_items(), c, peaks=2, K=3))
    assert [(s[0], s[1]) for s in e.seen] == [(0, ["uint8"] * 2), (1, ["uint16"] * 3), (0, ["uint16"]), (1, ["uint8"])]
    assert len(res) == 7 and res[0][1].shape == (2, 2) and res[0][2].shape == (2, 3, 2) and res[0][3].shape == (2, 3)


@pytest.mark.parametrize("name", ["colorize_gray", "suggest_gray"])
def test_the_upsample_keyword_sets_and_restores_the_state(name):
    c = np.zeros((313, 2), np.float32)

    def gen(e, upsample):
        if name == "colorize_gray":
            return e.colorize_gray(_items(), upsample=upsample)
        return e.suggest_gray(_items(), c, peaks=2, K=3, upsample=upsample)

    e = _Stream()
    assert len(list(gen(e, "joint"))) == 7
    assert [s[3] for s in e.seen] == ["joint"] * 4 and e.calls == ["joint", "linear"] and e._batch_upsample == "linear"
    e = _Stream()
    g = gen(e, "joint")
    assert e.calls == []
    next(g)
    assert e._batch_upsample == "joint"
    g.close()                                              # abandoned after the first result: both slots waited for, the setting back
    assert e.calls == ["joint", "linear"] and not e.busy
    e = _Stream()
    list(gen(e, None))
    assert e.calls == []
    with pytest.raises(ValueError):
        next(gen(_Stream(), "cubic"))


def test_depth_16_and_wrong_items_are_refused_before_anything_is_enqueued():
    a, b = np.zeros((5, 7), np.uint8), np.zeros((3, 3), np.uint16)
    e = _Stream()
    with pytest.raises(ValueError):
        list(e.colorize_gray([b, a], depth=16))           # an 8-bit item cannot give 16 bits ...
    assert e.seen == []                                    # ... and the group it would have closed was not sent
    with pytest.raises(ValueError):
        next(e.colorize_gray([b], depth=16, out="net"))
    with pytest.raises(ValueError):
        next(e.colorize_gray([b], depth=12))
    for bad in (np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.float32), np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError):
            next(e.colorize_gray([bad]))
    assert e.seen == []
    assert [r.dtype for r in e.colorize_gray([b, b], depth=16)] == [np.uint16] * 2 and [s[4] for s in e.seen] == [16]
    # the existing generators and calls keep refusing planes
    for gen in (e.colorize_images, e.evaluate_images):
        with pytest.raises(ValueError):
            next(gen([a]))
    with pytest.raises(ValueError):
        engine.HipColorizer.forward_async_images(e, 0, [a], None)


def test_forward_async_gray_marshals_one_format_and_even_addresses():
    e = _Stub()
    e._in_flight = {}
    a, b = np.zeros((5, 7), np.uint8), np.zeros((3, 3), np.uint16)
    call = lambda *args, **kw: engine.HipColorizer.forward_async_gray(e, *args, **kw)
    for images, kw in (([a, b], {}), ([np.zeros((3, 3, 3), np.uint8)], {}), ([np.zeros((4, 6), np.uint16)[:, ::2]], {}), ([a], dict(depth=16, out="source")),
                       ([b], dict(depth=16)), ([b], dict(depth=12)), ([b], dict(out_rgb=[np.zeros((3, 3, 3), np.uint8)], depth=16, out="source")),
                       ([b], dict(mode="reveal"))):
        with pytest.raises((ValueError, KeyError)):
            call(0, images, None, **kw)
    assert e.lib.calls == []
    outs = call(1, [b, b[:2]], [None, [(0, 0, 1, 1, 5.0, 6.0)]], out="source", depth=16)
    name, _h, slot, n, bits, table = e.lib.calls[0][:6]
    assert (name, slot, n, bits) == ("idc_forward_async_gray", 1, 2, 16) and e.lib.calls[0][12] == (N.IDC_BATCH_OUT_SOURCE | N.IDC_BATCH_OUT_RGB16)
    assert (table[0].h, table[0].w, table[1].h, table[1].w) == (3, 3, 2, 3) and table[1].pix == b.ctypes.data
    assert [o.dtype for o in outs] == [np.uint16] * 2 and [o.shape for o in outs] == [(3, 3, 3), (2, 3, 3)]
    assert all(o.ctypes.data % 2 == 0 for o in outs) and e.lib.calls[0][-1] is None
    outs = call(0, [a], None)
    assert e.lib.calls[1][4] == 8 and e.lib.calls[1][12] == 0 and outs[0].shape == (8, 8, 3) and outs[0].dtype == np.uint8
