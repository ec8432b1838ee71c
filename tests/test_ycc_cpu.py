"""CPU checks of the YCbCr 4:2:0 output planes (idc_set_batch_output / idc_fullres_ycc / idc_rgb_to_ycc420): the matrices and ranges of the
rule, tests/ycc_ref.py against PIL, the host twins in colorspace.py against tests/ycc_ref.py, eight mutants of the rule that the GPU file's exact
comparison catches on the GPU file's inputs, tools/ycc_selftest.cpp plain and under ASan + UBSan, and the ABI and Python plumbing on a stub
engine.  Nothing here needs a device."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ycc_ref as R
from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import colorspace, engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "interactive_deep_colorization_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


# ------------------------------------------------------------------------------------------------ 1. the matrices
def _cube(matrix):
    """(Y, Cb, Cr) int64 [2^24] of every colour at k = 1, vectorised."""
    my, mcb, mcr, yoff = R.MATRICES[matrix]
    v = np.arange(256, dtype=np.int64)
    r, g, b = v[:, None, None], v[None, :, None], v[None, None, :]
    y = ((my[0] * r + my[1] * g + my[2] * b + 32768) >> 16) + yoff
    cb = mcb[0] * r + mcb[1] * g + mcb[2] * b + R.BIAS
    cr = mcr[0] * r + mcr[1] * g + mcr[2] * b + R.BIAS
    assert cb.min() >= 0 and cr.min() >= 0                  # the numerator is never negative: the shift is a floor
    return y, cb >> 16, cr >> 16


@pytest.mark.parametrize("matrix,sum_y,ry,rcb,rcr", [("jfif", 65536, (0, 255), (0, 255), (0, 255)), ("bt709", 56284, (16, 235), (16, 240), (16, 240))])
def test_matrices_greys_and_ranges_over_the_whole_cube(matrix, sum_y, ry, rcb, rcr):
    my, mcb, mcr, yoff = R.MATRICES[matrix]
    assert sum(my) == sum_y and sum(mcb) == 0 and sum(mcr) == 0
    for g in range(256):
        assert R.pixel(g, g, g, matrix)[1:] == (128, 128)
    y, cb, cr = _cube(matrix)
    assert (int(y.min()), int(y.max())) == ry and (int(cb.min()), int(cb.max())) == rcb and (int(cr.min()), int(cr.max())) == rcr
    assert R.MATRICES == colorspace.YCC_MATRICES


def test_the_rule_at_k1_is_within_one_level_of_pil():
    from PIL import Image
    rs = np.random.RandomState(7)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    cols = np.concatenate([rs.randint(0, 256, (200000, 3)).astype(np.uint8), corners])
    pil = np.asarray(Image.fromarray(cols[None], "RGB").convert("YCbCr"))[0].astype(np.int64)
    my, mcb, mcr, yoff = R.MATRICES["jfif"]
    c = cols.astype(np.int64)
    ours = np.stack([((c @ np.array(my) + 32768) >> 16) + yoff, (c @ np.array(mcb) + R.BIAS) >> 16, (c @ np.array(mcr) + R.BIAS) >> 16], axis=1)
    for k in range(0, len(cols), 997):                      # the vectorised restatement is ycc_ref's pixel()
        assert tuple(ours[k]) == R.pixel(*[int(v) for v in cols[k]], "jfif")
    diff = np.abs(ours - pil).max(axis=0)
    print("max |ycc_ref - PIL| per channel:", diff)
    assert diff.max() <= 1


# ------------------------------------------------------------------------------------------------ 2. the host twins
@pytest.mark.parametrize("matrix", sorted(R.MATRICES))
def test_the_host_twin_is_the_rule_on_the_gpu_inputs(matrix):
    for name, rgb in R.inputs():
        for fmt in R.FORMATS:
            got = colorspace.rgb_to_ycc420(rgb, fmt, matrix)
            assert got.dtype == np.uint8 and got.size == R.nbytes(*rgb.shape[:2])
            np.testing.assert_array_equal(got, R.block(rgb, fmt, matrix), err_msg="%s %s %s" % (name, fmt, matrix))


@pytest.mark.parametrize("matrix", sorted(R.MATRICES))
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_a_flat_image_comes_back_within_two_levels(fmt, matrix):
    rs = np.random.RandomState(3)
    for colour in [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 0, 255), (12, 200, 77)] + [tuple(c) for c in rs.randint(0, 256, (40, 3))]:
        flat = np.tile(np.array(colour, np.uint8), (5, 7, 1))
        back = colorspace.ycc420_to_rgb(colorspace.rgb_to_ycc420(flat, fmt, matrix), 5, 7, fmt, matrix)
        assert back.shape == (5, 7, 3) and np.abs(back.astype(int) - flat).max() <= 2, colour


def test_the_host_twin_refuses_other_types():
    with pytest.raises(ValueError):
        colorspace.rgb_to_ycc420(np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError):
        colorspace.rgb_to_ycc420(np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError):
        colorspace.rgb_to_ycc420(np.zeros((4, 4, 3), np.uint8), "yuy2")
    with pytest.raises(KeyError):
        colorspace.rgb_to_ycc420(np.zeros((4, 4, 3), np.uint8), "i420", "bt2020")


# ------------------------------------------------------------------------------------------------ 3. the inputs and the mutants
def test_gpu_inputs_meet_their_conditions():
    ins = R.inputs()
    sizes = [a.shape[:2] for _, a in ins]
    for s in R.SIZES:
        assert s in sizes
    assert any(h % 2 and w % 2 for h, w in sizes) and any(h % 2 and not w % 2 for h, w in sizes) and any(w % 2 and not h % 2 for h, w in sizes)
    assert R.start_residues() == {0, 1, 2, 3}               # image starts of the packed RGB run on every residue mod 4
    assert any((a == 0).all() for _, a in ins) and any((a == 255).all() for _, a in ins)
    blue = red = edge = 0
    for _, a in ins:
        h, w = a.shape[:2]
        for j in range(h // 2):
            for i in range(min(w // 2, 64)):
                blk = a[2 * j:2 * j + 2, 2 * i:2 * i + 2].reshape(4, 3)
                blue += (blk == (0, 0, 255)).all()
                red += (blk == (255, 0, 0)).all()
                prim = [tuple(p) in R.PRIMARIES for p in blk]
                edge += all(prim) and len(set(map(tuple, blk))) > 1
    print("saturated blue blocks %d, red %d, blocks that straddle an edge between two primaries %d" % (blue, red, edge))
    assert blue >= 4 and red >= 4 and edge >= 4


def _mutant(rgb, fmt, matrix, mutant):
    """The rule in numpy with one mistake."""
    my, mcb, mcr, yoff = R.MATRICES[matrix]
    if mutant == "luma601_under_709" and matrix == "bt709":
        my = tuple(int(round(v * 219 / 255)) for v in R.MATRICES["jfif"][0])
    h, w = rgb.shape[:2]
    ch, cw = ((h + 1) // 2, w // 2) if mutant == "cw_floor" else ((h + 1) // 2, (w + 1) // 2)
    p = rgb.astype(np.int64)
    if mutant == "replicate":                               # edge blocks replicated to 2 x 2 in place of clipped
        p = np.pad(p, ((0, h % 2), (0, w % 2), (0, 0)), mode="edge")
    if mutant == "zero_pad":                                # edge blocks filled up to 2 x 2 with neutral chroma: the k pixels' sum over 4
        p = np.pad(p, ((0, h % 2), (0, w % 2), (0, 0)), mode="constant")
    y = ((rgb.astype(np.int64) @ np.array(my) + 32768) >> 16) + yoff
    hh, ww = p.shape[:2]
    ones = np.zeros((2 * ch, 2 * ((ww + 1) // 2)), np.int64)
    ones[:hh, :ww] = 1
    k = ones.reshape(ch, 2, -1, 2).sum(axis=(1, 3))
    lg = (k == 2) + 2 * (k == 4)
    planes = []
    for m in (mcb, mcr):
        t = p @ np.array(m)
        if mutant == "round_each_pixel":                    # each pixel's chroma rounded to 8 bits before the mean
            t = ((t + R.BIAS) >> 16 << 16) - R.BIAS + 32767
        s = np.zeros(ones.shape, np.int64)
        s[:hh, :ww] = t
        s = s.reshape(ch, 2, -1, 2).sum(axis=(1, 3))
        if mutant == "truncating_division":                 # the signed sum divided towards zero, then the offset
            q = np.abs(s + k * 32767) // (65536 * k) * np.sign(s + k * 32767) + 128
        elif mutant == "bias_32768":
            q = (s + k * ((128 << 16) + 32768)) >> (16 + lg)
        else:
            q = (s + k * R.BIAS) >> (16 + lg)
        planes.append(q[:, :cw])
    if mutant == "swap_cb_cr":
        planes = planes[::-1]
    if fmt == "nv12":
        c = np.stack(planes[::-1] if mutant == "nv12_order" else planes, axis=-1)
    else:
        c = np.stack(planes, axis=0)
    return np.concatenate([y.reshape(-1), c.reshape(-1)]).astype(np.uint8)


MUTANTS = ["truncating_division", "bias_32768", "round_each_pixel", "zero_pad", "cw_floor", "swap_cb_cr", "nv12_order", "luma601_under_709"]


def test_the_restatement_without_a_mistake_is_the_rule():
    for name, rgb in R.inputs()[:10]:
        for fmt in R.FORMATS:
            for matrix in R.MATRICES:
                np.testing.assert_array_equal(_mutant(rgb, fmt, matrix, None), R.block(rgb, fmt, matrix), err_msg=name)


def test_replicating_the_edge_is_the_clipped_mean_exactly():
    """Replicating an edge block's pixels to 2 x 2 is no mistake the comparison could catch: it is the clipped mean, bit for bit.  A block of
    k = 2 pixels with sum S becomes 4 pixels with sum 2S, and floor((2S + 4B) / 2^18) == floor((S + 2B) / 2^17); k = 1 alike with 4S.  So no
    input tells the two apart, and the edge mutant of the list above is the nearest mistake that is one: the missing pixels taken as neutral
    (``zero_pad``), which odd sizes catch."""
    odd = 0
    for name, rgb in R.inputs():
        odd += rgb.shape[0] % 2 or rgb.shape[1] % 2
        for fmt in R.FORMATS:
            for matrix in sorted(R.MATRICES):
                np.testing.assert_array_equal(_mutant(rgb, fmt, matrix, "replicate"), R.block(rgb, fmt, matrix), err_msg=name)
    assert odd >= 10


@pytest.mark.parametrize("mutant", MUTANTS)
def test_the_exact_comparison_catches_the_mutant(mutant):
    caught = 0
    for name, rgb in R.inputs():
        for fmt in R.FORMATS:
            for matrix in sorted(R.MATRICES):
                got, want = _mutant(rgb, fmt, matrix, mutant), R.block(rgb, fmt, matrix)
                caught += got.size != want.size or bool((got != want).any())
    print("%s: caught on %d (image, format, matrix) combinations" % (mutant, caught))
    assert caught >= 1


# ------------------------------------------------------------------------------------------------ 4. the header and the plan
def _make(target, out, san):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc (%s): tools/%s.cpp cannot be compiled" % (HIPCC, target))
    cmd = ["make", "-C", CSRC, target, "BINDIR=" + out, "HIPCC=" + HIPCC] + (["SAN=1"] if san else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return os.path.join(out, target)


@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan_ubsan"])
def test_sizes_offsets_workgroups_and_plan(tmp_path, san):
    run = subprocess.run([_make("ycc_selftest", str(tmp_path), san)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert re.match(r"ycc_selftest: ok \(\d+ sizes, 11 calls\)", run.stdout.splitlines()[-1]), run.stdout + run.stderr


def test_the_header_is_plain_cpp_and_the_kernel_keeps_to_its_brief():
    text = open(os.path.join(CSRC, "idc_ycc.h")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", text) == ["stddef.h"] and "__global__" not in text and not re.search(r"\bhip[A-Z]\w+\(", text)
    tool = open(os.path.join(REPO, "tools", "ycc_selftest.cpp")).read()
    assert [i for i in re.findall(r"#include\s*\"([^\"]+)", tool)] == ["idc_ycc.h", "idc_batch.h"]
    kern = open(os.path.join(CSRC, "idc_ycc.hip")).read()
    assert "grid_blocks" not in kern and "GridTag" not in kern and "gridDim" not in kern            # an exact grid: no cap, no tag, no grid-stride loop
    assert len(re.findall(r"hipLaunchKernelGGL\(", kern)) == 1 and len(re.findall(r"__global__", kern)) == 1      # NV12 is a layout switch, not a kernel
    assert "double" not in kern.split("#include <hip/hip_runtime.h>")[1] and "float" not in kern.split("#include <hip/hip_runtime.h>")[1]
    for coeff in ("19595, 38470, 7471", "-11059, -21709, 32768", "32768, -27439, -5329", "11966, 40254, 4064", "-6596, -22189, 28785", "28784, -26145, -2639"):
        assert coeff in text and coeff in open(os.path.join(REPO, "include", "ideepcolor.h")).read()


# ------------------------------------------------------------------------------------------------ 5. the ABI
def test_abi_symbols_prototypes_and_null_statuses():
    header = open(os.path.join(REPO, "include", "ideepcolor.h")).read()
    assert re.search(r"enum\s*\{\s*IDC_OUT_RGB\s*=\s*0\s*,\s*IDC_OUT_I420\s*=\s*1\s*,\s*IDC_OUT_NV12\s*=\s*2\s*\}", header)
    assert re.search(r"enum\s*\{\s*IDC_YCC_JFIF\s*=\s*0\s*,\s*IDC_YCC_BT709_VIDEO\s*=\s*1\s*\}", header)
    assert re.search(r"\bsize_t\s+idc_ycc420_bytes\s*\(\s*int\s+h\s*,\s*int\s+w\s*\)\s*;", header)
    assert re.search(r"\bint\s+idc_set_batch_output\s*\(\s*idc_handle\s+h\s*,\s*int\s+format\s*,\s*int\s+matrix\s*\)\s*;", header)
    assert re.search(r"\bint\s+idc_fullres_ycc\s*\(\s*idc_handle\s+h\s*,\s*int\s+img\s*,\s*int\s+source\s*,\s*int\s+interp\s*,\s*int\s+l_mode\s*,"
                     r"\s*int\s+format\s*,\s*int\s+matrix\s*,\s*uint8_t\s*\*\s*out\s*\)\s*;", header)
    assert re.search(r"\bint\s+idc_rgb_to_ycc420\s*\(\s*idc_handle\s+h\s*,\s*int\s+n\s*,\s*const\s+idc_ref_image\s*\*\s*images\s*,\s*int\s+format\s*,"
                     r"\s*int\s+matrix\s*,\s*uint8_t\s*\*\s*const\s*\*\s*out\s*\)\s*;", header)
    for s in ("idc_ycc420_bytes", "idc_set_batch_output", "idc_fullres_ycc", "idc_rgb_to_ycc420"):
        assert s in N.EXPORTED_SYMBOLS
    assert (N.IDC_OUT_RGB, N.IDC_OUT_I420, N.IDC_OUT_NV12, N.IDC_YCC_JFIF, N.IDC_YCC_BT709_VIDEO) == (0, 1, 2, 0, 1)
    lib = N.load()
    for h, w in [(1, 1), (3, 3), (64, 64), (211, 83), (65, 16384), (16384, 16384)]:
        assert lib.idc_ycc420_bytes(h, w) == R.nbytes(h, w) == engine.ycc420_bytes(h, w)
    for h, w in [(0, 1), (1, 0), (16385, 4), (4, 16385), (-3, 5)]:
        assert lib.idc_ycc420_bytes(h, w) == 0
    assert lib.idc_set_batch_output(None, N.IDC_OUT_I420, N.IDC_YCC_JFIF) == -1         # a null handle, without a device
    assert lib.idc_rgb_to_ycc420(None, 1, None, N.IDC_OUT_I420, N.IDC_YCC_JFIF, None) == -1


def test_views_of_a_block():
    buf = np.arange(R.nbytes(5, 7), dtype=np.uint8)
    v = engine.ycc420_views(buf, 5, 7, "i420")
    assert v._fields == ("y", "cb", "cr", "buf") and v.y.shape == (5, 7) and v.cb.shape == v.cr.shape == (3, 4)
    assert v.y[0, 0] == 0 and v.cb[0, 0] == 35 and v.cr[0, 0] == 47 and v.cr[-1, -1] == 58 and np.shares_memory(v.buf, buf)
    assert np.shares_memory(v.y, buf) and np.shares_memory(v.cr, buf)
    v = engine.ycc420_views(buf, 5, 7, "nv12")
    assert v._fields == ("y", "cbcr", "buf") and v.cbcr.shape == (3, 4, 2) and v.cbcr[0, 0, 0] == 35 and v.cbcr[0, 0, 1] == 36
    with pytest.raises(ValueError):
        engine.ycc420_views(buf[:-1], 5, 7)
    with pytest.raises(ValueError):
        engine.ycc420_views(buf, 5, 7, "rgb")


# ------------------------------------------------------------------------------------------------ 6. the Python plumbing
class _Lib(object):
    def __init__(self):
        self.calls, self.seen = [], []

    def idc_set_batch_output(self, h, f, m):
        self.calls.append((f, m))
        return 0

    def idc_set_ingest_filter(self, h, f):
        return 0

    def idc_rgb_to_ycc420(self, h, n, table, f, m, outs):
        self.seen.append((n, f, m, [(table[i].h, table[i].w) for i in range(n)]))
        return 0


class _Pool(object):
    def take(self, shape, dtype):
        return np.zeros(shape, dtype)


class _Stub(engine.HipColorizer):
    """The streaming generators over an engine that launches nothing: every enqueue records the output setting in force and returns buffers of
    the shapes the real calls would."""

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
        self.seen.append((self._out_format, self._out_matrix, self._batch_upsample))

    def _outs(self, images):
        return [np.zeros(s, np.uint8) for s in self._out_shapes([a.shape[:2] + (3,) for a in images])]

    def forward_async_rgb(self, slot, rgb, hints, out_rgb, **kw):
        self._enqueue()
        assert out_rgb.shape == ((rgb.shape[0], R.nbytes(*rgb.shape[1:3])) if self._out_format != "rgb" else rgb.shape)

    def forward_async_images(self, slot, images, hints, **kw):
        self._enqueue()
        return self._outs(images)

    def forward_async_layers(self, slot, images, layers, hints, **kw):
        self._enqueue()
        return self._outs(images), np.zeros(len(images), np.int32)

    def forward_async_gray(self, slot, images, hints, **kw):
        self._enqueue()
        if kw.get("peaks") is not None or kw.get("bin_centres") is not None:
            return self._dist(images)
        return self._outs(images)

    def forward_async_eval(self, slot, images, hints, **kw):
        self._enqueue()
        return np.zeros((len(images), 3), np.uint64), None, None

    def _dist(self, images):
        n, res = len(images), engine.DistBatch()
        res.out_rgb = self._outs(images)
        res.peaks, res.sugg_centres, res.sugg_conf = np.zeros((n, 2, 2), np.int32), np.zeros((n * 2, 3, 2)), np.zeros((n * 2, 3))
        res.peak_ent = np.zeros((n, 2), np.float32)
        res.sse, res.score = np.zeros((n, 3), np.uint64), engine.DistScore()
        res.score.xent, res.score.hits, res.score.cells = np.zeros(n), np.zeros((n, 2), np.uint32), 4
        return res

    def forward_async_dist(self, slot, images, hints, **kw):
        self._enqueue()
        return self._dist(images)


GENERATORS = ["colorize_stream", "colorize_images", "colorize_gray", "colorize_layers", "evaluate_images", "suggest_images", "suggest_gray", "score_images"]
WITH_IMAGES = {"colorize_stream": None, "colorize_images": None, "colorize_gray": None, "colorize_layers": 0, "suggest_images": 0, "suggest_gray": 0}


def _generator(e, name, **kw):
    img, g = np.zeros((5, 7, 3), np.uint8), np.zeros((5, 7), np.uint8)
    items, c = [img] * 5, np.zeros((313, 2), np.float32)         # three batches of at most two
    return {
        "colorize_stream": lambda: e.colorize_stream([(np.stack([img, img]), None)] * 3, out="source", **kw),
        "colorize_images": lambda: e.colorize_images(items, **kw),
        "colorize_gray": lambda: e.colorize_gray([g] * 5, **kw),
        "colorize_layers": lambda: e.colorize_layers([(img, None, None)] * 5, **kw),
        "evaluate_images": lambda: e.evaluate_images(items, out="source", **kw),
        "suggest_images": lambda: e.suggest_images(items, c, peaks=2, K=3, **kw),
        "suggest_gray": lambda: e.suggest_gray([g] * 5, c, peaks=2, K=3, **kw),
        "score_images": lambda: e.score_images(items, c, **kw),
    }[name]()


def test_set_batch_output_reaches_the_library():
    e = _Stub()
    e.set_batch_output("i420")
    e.set_batch_output("nv12", "bt709")
    e.set_batch_output()
    assert e.lib.calls == [(1, 0), (2, 1), (0, 0)] and (e._out_format, e._out_matrix) == ("rgb", "jfif")
    for bad in (("yuy2", "jfif"), ("i420", "bt2020")):
        with pytest.raises(ValueError):
            e.set_batch_output(*bad)
    assert len(e.lib.calls) == 3 and (e._out_format, e._out_matrix) == ("rgb", "jfif")


@pytest.mark.parametrize("name", GENERATORS)
def test_the_out_format_keyword_sets_and_restores_the_state(name):
    # run to the end: set before the first batch, every batch sees it, the previous setting is back afterwards
    e = _Stub()
    results = list(_generator(e, name, out_format="nv12", out_matrix="bt709"))
    assert len(results) in (3, 5) and e.seen == [("nv12", "bt709", "linear")] * 3
    assert e.lib.calls == [(2, 1), (0, 0)] and (e._out_format, e._out_matrix) == ("rgb", "jfif")
    if name in WITH_IMAGES:                                 # one tuple of plane views per image
        first = results[0] if WITH_IMAGES[name] is None else results[0][WITH_IMAGES[name]]
        if name == "colorize_stream":
            assert len(first) == 2
            first = first[0]
        assert isinstance(first, engine.NV12) and first.y.shape == (5, 7) and first.cbcr.shape == (3, 4, 2) and first.buf.size == R.nbytes(5, 7)
    # only one of the two given: the other stays; a previous setting is what comes back; None touches nothing
    e = _Stub()
    e.set_batch_output("nv12", "bt709")
    results = list(_generator(e, name, out_format="i420"))
    assert set(e.seen) == {("i420", "bt709", "linear")} and e.lib.calls == [(2, 1), (1, 1), (2, 1)]
    if name in WITH_IMAGES and name != "colorize_stream":
        first = results[0] if WITH_IMAGES[name] is None else results[0][WITH_IMAGES[name]]
        assert isinstance(first, engine.YCC420) and first.cb.shape == first.cr.shape == (3, 4)
    e.lib.calls, e.seen = [], []
    list(_generator(e, name))
    assert e.lib.calls == [] and set(e.seen) == {("nv12", "bt709", "linear")}
    # with the format off the generators yield what they always did
    e = _Stub()
    results = list(_generator(e, name))
    if name in WITH_IMAGES:
        first = results[0] if WITH_IMAGES[name] is None else results[0][WITH_IMAGES[name]]
        assert isinstance(first, np.ndarray) and first.shape[-3:] == (5, 7, 3)
    # together with upsample=: both are set, both come back
    e = _Stub()
    list(_generator(e, name, out_format="i420", upsample="joint"))
    assert set(e.seen) == {("i420", "jfif", "joint")} and (e._out_format, e._batch_upsample) == ("rgb", "linear")
    # abandoned after the first result: restored when the generator is closed
    e = _Stub()
    g = _generator(e, name, out_format="i420")
    assert e.lib.calls == []                                # nothing happens before the first next()
    next(g)
    assert e._out_format == "i420"
    g.close()
    assert e.lib.calls == [(1, 0), (0, 0)] and e._out_format == "rgb"
    # an exception on the way: restored as well
    e = _Stub(fail_after=1)
    with pytest.raises(RuntimeError):
        list(_generator(e, name, out_format="nv12", upsample="joint", ingest="antialias"))
    assert e.seen == [("nv12", "jfif", "joint")] and (e._out_format, e._batch_upsample, e._ingest_filter) == ("rgb", "linear", "bilinear")
    # a value that is neither is refused before anything is enqueued, and what was already set goes back
    e = _Stub()
    with pytest.raises(ValueError):
        next(_generator(e, name, out_format="yuy2", upsample="joint", ingest="antialias"))
    assert e.seen == [] and (e._out_format, e._batch_upsample, e._ingest_filter) == ("rgb", "linear", "bilinear")


def test_rgb_to_ycc420_marshals_its_arguments():
    e = _Stub()
    a, b = np.zeros((5, 7, 3), np.uint8), np.zeros((2, 3, 3), np.uint8)
    one = e.rgb_to_ycc420(a)
    assert isinstance(one, engine.YCC420) and one.y.shape == (5, 7)
    two = e.rgb_to_ycc420([a, b[:, ::-1]], format="nv12", matrix="bt709")        # a non-contiguous view is copied, not refused
    assert [type(t) for t in two] == [engine.NV12, engine.NV12] and two[1].cbcr.shape == (1, 2, 2)
    assert e.lib.seen == [(1, 1, 0, [(5, 7)]), (2, 2, 1, [(5, 7), (2, 3)])]
    for bad in (dict(format="rgb"), dict(matrix="bt601")):
        with pytest.raises(ValueError):
            e.rgb_to_ycc420(a, **bad)
    with pytest.raises(ValueError):
        e.rgb_to_ycc420([np.zeros((4, 4), np.uint8)])


def test_the_enqueue_calls_ask_for_flat_blocks_under_a_ycbcr_format():
    e = _Stub()
    shapes = [(5, 7, 3), (8, 8, 3)]
    assert e._out_shapes(shapes) == shapes
    e.set_batch_output("i420")
    assert e._out_shapes(shapes) == [(R.nbytes(5, 7),), (R.nbytes(8, 8),)]
    assert e._out_shapes(shapes, 16) == shapes              # 16-bit RGB: the shapes stay and the library refuses the call
