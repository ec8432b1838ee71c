"""Plans of geometries where ONE image passes the per-image 32-bit bound of some layer, from tools/plan_dump (the planner without a device).

Several kernel families address one source image of a launch with 32-bit offsets and are kept off larger images by host predicates.  For every row
of every plan below, the bytes one image of the row's source holds (tests/large_ref.py: Hs * si * Ws * si * nkc * parts * kRowBytes in Python
integers) are held against the bound of the family the row's label names -- FAMILY_BOUND, one line per family, each read from the predicate
named beside it.  A family with 64-bit addressing carries None.

What this found: conv_igemm and conv_click (hoff[], 32-bit) had no guard at all, and conv_igemm_v2m's body (also the operand-split conv_igemm_v2s
forms) added a 32-bit offset to the image's base although the planner hands it exactly the images that conv_igemm_v2p's guard turns away.  Now
conv_igemm_v2m's body addresses from the halo tile's own 64-bit base (any image; v2m_rows_fit bounds the tile's rows), both small-tile launchers
carry conv_igemm_offsets_fit, and a layer that ends on the small tile with a source image beyond 2^31 bytes is refused by plan_forward with
IDC_ERR_INVALID_ARG -- by idc_create before it asks for a device (include/ideepcolor.h).  Which geometries that refuses, and why no other
family could take the launch:
  bf16  8192 x 8192   conv10_1: a deconv whose shortcut conv could not be fused (conv_ds_m_fits) sums a shortcut tensor, which only the small
                      tile does on the bf16 path; its source conv9_2 is 4096 x 4096 x 256 B = 2^32
  fp32  2896 x 2896   conv10_2: the fp32 path has the Winograd form (wino_offsets_fit) and the small tile; conv10_1 is 2896^2 x 512 B = 4.29e9
  fp32  4096, 8192    conv1_2 already: conv1_1 is 4096^2 x 256 B = 2^32
fp16x3 plans every size (every layer but conv1_1 on conv_igemm_v2sh / v2psh / the fused deconv forms), bf16 up to 4096 x 4096.
At 2048 x 2048 every plan is the parent commit's, label for label (tests/golden/large_plan_2048.json): no guard fires early."""
import ctypes
import json
import os
import re
import subprocess

import pytest

import large_ref as lr
from conftest import GOLDEN
from test_plan_cpu import plan_dump  # noqa: F401  (the module-scoped fixture that compiles tools/plan_dump.cpp)

BELOW = 0x7fffffff - 1            # "bytes < 0x7fffffffLL": the largest byte count such a predicate admits
FAMILY_BOUND = {                  # family -> largest admissible bytes of one source image, or None (64-bit addressing / no stored source)
    "conv_igemm": 1 << 31,                    # conv_igemm_offsets_fit (inclusive: the largest offset formed is 16 bytes short of the image's size)
    "conv_click": 1 << 31,                    # conv_igemm_offsets_fit
    "conv_wino_f32": BELOW,                   # wino_offsets_fit (conv_wino_applies)
    "conv_wino_deconv_f32": BELOW,            # wino_offsets_fit
    "conv_kwave_bf16": BELOW,                 # wino_offsets_fit (conv_kwave_applies, set_geometry)
    "conv_kwave_deconv_bf16": BELOW,          # wino_offsets_fit
    "conv_igemm_v2+m16p": BELOW,              # conv_v2p_applies: buffer loads, 32-bit offsets into one image
    "conv_igemm_v2ph": BELOW,                 # conv_v2p_applies
    "conv_igemm_v2ps": BELOW,                 # conv_v2ps_applies (nkc * in_parts)
    "conv_igemm_v2psh": BELOW,                # conv_v2ps_applies
    "conv_igemm_v2+m16": None,                # conv_igemm_v2m: 64-bit tile base (v2m_rows_fit bounds the tile's rows: ROWS_FIT below)
    "conv_igemm_v2s": None,                   # conv_igemm_v2m's body
    "conv_igemm_v2sh": None,                  # conv_igemm_v2m's body
    "conv_ds_fused_m": BELOW,                 # conv_ds_m_fits: 4 * Hs * Ws * max(nkc, nkc2) chunks, which covers both of its sources
    "conv_ds_fused_mh": BELOW,                # conv_ds_m_fits
    "conv_ds_fused_ms": BELOW,                # conv_ds_m_fits (nkc * in_parts)
    "conv_ds_fused_msh": BELOW,               # conv_ds_m_fits
    "conv1_2_split_kernel": BELOW,            # conv1_2_split_applies
    "conv1_block_fused": None,                # reads the caller's planes (64-bit pixel index); its conv1_2 half reads LDS
    "conv1_1_bf16_kernel": None,              # the caller's planes
    "conv1_1_split_kernel": None,             # the caller's planes
}
ROWS_FIT = ("conv_igemm_v2+m16", "conv_igemm_v2s", "conv_igemm_v2sh")      # v2m_rows_fit: 20 * si source rows of one tile below 2^31 - 1 bytes

SIZES, BATCHES, PRECISIONS, FLAGS = (2896, 4096, 8192), (1, 32), ("bf16", "fp16x3", "fp32"), (0, lr.FLAG_DIST313)
REFUSED = {("bf16", 8192): ("conv10_1", "conv9_2"), ("fp32", 2896): ("conv10_2", "conv10_1"), ("fp32", 4096): ("conv1_2", "conv1_1"),
           ("fp32", 8192): ("conv1_2", "conv1_1")}


def family(label):
    label = re.sub(r" splitK\d+$", "", label)
    m = re.match(r"(conv_igemm_v2(?:psh|ps|ph|sh|s)?)<\d,\d>(?:x\d)?(\+m16p|\+m16)?", label)
    if m:
        return m.group(1) + (m.group(2) or "")
    return re.match(r"[a-z0-9_]+", label).group(0)


def test_family_names():
    assert family("conv_igemm<bf16,2,2> splitK4") == "conv_igemm" and family("conv_igemm_v2<2,2>+m16p+head") == "conv_igemm_v2+m16p"
    assert family("conv_igemm_v2<2,2>+m16+head") == "conv_igemm_v2+m16" and family("conv_igemm_v2psh<4,2>x3") == "conv_igemm_v2psh"
    assert family("conv_igemm_v2sh<2,2>x3+head") == "conv_igemm_v2sh" and family("conv_ds_fused_msh+shortcut x3") == "conv_ds_fused_msh"
    assert family("conv1_2_split_kernel x3") == "conv1_2_split_kernel" and family("conv_igemm_v2<4,2>") == "conv_igemm_v2"      # (a partner build's: not in the table)


def _run(plan_dump, precision, flags, size, max_batch):
    return subprocess.run([plan_dump, precision, str(flags), str(size), str(size), str(max_batch), "1"], capture_output=True, text=True)


def _rows(stdout):
    return [line.split("\t")[:2] for line in stdout.splitlines()]


def check_rows(rows, precision, size, flags):
    """Every conv row's source image inside the bound of the family its label names; returns how many rows were held against a bound."""
    layers = {l[0]: l for l in lr.LAYERS}
    label = dict(rows)
    held = 0
    for name, kernel in rows:
        if name not in layers:                 # glob_branch / head / dist_softmax: not conv launches
            continue
        src_bytes = lr.source_bytes(name, precision, size, size, flags)
        host = kernel[len("fused into "):] if kernel.startswith("fused into ") else name
        fam = family(label[host])
        assert fam in FAMILY_BOUND, "%s runs %s: a family this table does not know" % (name, label[host])
        bound = FAMILY_BOUND[fam]
        if src_bytes is None or bound is None or (host != name and fam == "conv1_block_fused"):
            pass
        else:
            assert src_bytes <= bound, "%s (%s, %d x %d): one source image holds %d bytes, %s addresses %d" % (name, precision, size, size, src_bytes, fam, bound)
            held += 1
        _, kind, _, _, si, src, _, _, level, _ = layers[name]
        t = lr.tensors(precision, size, size, flags).get(src)
        if fam.startswith("conv_ds_fused") and host == name:     # the predicate's own, conservative quantity
            short = [n for n, k in rows if k == "fused into " + name]
            assert len(short) == 1, (name, short)
            ts = lr.tensors(precision, size, size, flags)[layers[short[0]][5]]
            chunks = max(t["pixel_bytes"], ts["pixel_bytes"]) // lr.ROW_BYTES
            assert 4 * t["h"] * t["w"] * chunks * lr.ROW_BYTES <= BELOW, (name, fam)
        if fam in ROWS_FIT and src_bytes is not None:
            si = 1 if kind == "dc" else si
            ws = t["w"] if kind == "dc" else size // level
            assert 20 * si * ws * si * t["pixel_bytes"] <= BELOW, (name, fam)
    return held


@pytest.mark.parametrize("flags", FLAGS, ids=["plain", "dist313"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("max_batch", BATCHES)
@pytest.mark.parametrize("size", SIZES)
def test_every_planned_row_is_addressable_or_the_geometry_is_refused(plan_dump, size, max_batch, precision, flags):
    r = _run(plan_dump, precision, flags, size, max_batch)
    if (precision, size) in REFUSED:
        layer, src = REFUSED[(precision, size)]
        nbytes = lr.source_bytes(layer, precision, size, size, flags)
        assert nbytes > FAMILY_BOUND["conv_igemm"]
        assert r.returncode == 1 and r.stdout == "", (r.returncode, r.stdout[:200])
        for word in ("%d x %d is too large" % (size, size), "one image of %s," % src, "layer %s" % layer, "%d bytes" % nbytes, "2^31"):
            assert word in r.stderr, (word, r.stderr)
        return
    assert r.returncode == 0, r.stderr
    rows = _rows(r.stdout)
    assert [n for n, _ in rows if not n.startswith(("glob_", "head", "dist_"))] == [l[0] for l in lr.active_layers(flags)]
    check_rows(rows, precision, size, flags)
    # one image of SOME layer's source is past the bound of the guarded families here: that is what these sizes are for.  (bf16 at 2896 x 2896 is the
    # largest square every guard still admits: conv10_1 holds 2896^2 x 256 B, 458 752 bytes short of 2^31.)
    largest = max(t["image_bytes"] for t in lr.tensors(precision, size, size, flags).values())
    assert largest > BELOW or ((precision, size) == ("bf16", 2896) and largest == (1 << 31) - 458752)


with open(os.path.join(GOLDEN, "large_plan_2048.json")) as _f:
    BELOW_THE_BOUNDARY = json.load(_f)["configs"]


@pytest.mark.parametrize("cfg", BELOW_THE_BOUNDARY, ids=lambda c: "%s mb%d flags%d" % (c["precision"], c["max_batch"], c["flags"]))
def test_2048_plans_as_before(plan_dump, cfg):
    r = _run(plan_dump, cfg["precision"], cfg["flags"], cfg["size"], cfg["max_batch"])
    assert r.returncode == 0, r.stderr
    rows = _rows(r.stdout)
    assert rows == cfg["rows"], [(w, g) for w, g in zip(cfg["rows"], rows) if w != g]
    assert check_rows(rows, cfg["precision"], cfg["size"], cfg["flags"]) >= 20


@pytest.mark.parametrize("precision,last,first", [("bf16", 5792, 5800), ("fp32", 2048, 2056)])
def test_the_limit_include_ideepcolor_h_states(plan_dump, precision, last, first):
    """The largest square image each precision plans, and the next multiple of 8, refused (the figures in idc_create's comment)."""
    for flags in FLAGS:
        r = _run(plan_dump, precision, flags, last, 1)
        assert r.returncode == 0, r.stderr
        check_rows(_rows(r.stdout), precision, last, flags)
        r = _run(plan_dump, precision, flags, first, 1)
        assert r.returncode == 1 and "%d x %d is too large" % (first, first) in r.stderr, r.stderr


def test_golden_holds_the_twelve_plans():
    assert sorted((c["precision"], c["max_batch"], c["flags"], c["size"]) for c in BELOW_THE_BOUNDARY) == \
        sorted((p, b, f, 2048) for p in PRECISIONS for b in BATCHES for f in FLAGS)


def test_a_wrong_plan_would_be_seen():
    """The checker against plans it must refuse: a guarded family on an image past its bound, and a label outside the table."""
    rows = _rows("conv1_1\tconv1_block_fused\nconv1_2\tfused into conv1_1\nconv2_1\tconv_igemm_v2<2,2>+m16p\n")
    with pytest.raises(AssertionError, match="conv2_1 .*one source image holds 2147483648 bytes"):      # conv1_2 at 4096 x 4096: 2^31 bytes
        check_rows(rows, "bf16", 4096, 0)
    assert check_rows(rows, "bf16", 2896, 0) == 1
    rows[2][1] = "conv_igemm_v2<2,2>+m16"
    assert check_rows(rows, "bf16", 4096, 0) == 0
    rows[2][1] = "conv_igemm_v2<2,2>"
    with pytest.raises(AssertionError, match="does not know"):
        check_rows(rows, "bf16", 2896, 0)
    rows[2][1] = "conv_igemm<bf16,2,2>"
    assert check_rows(rows, "bf16", 4096, 0) == 1                                                        # 2^31 inclusive
    with pytest.raises(AssertionError, match="conv_igemm addresses"):
        check_rows(rows, "bf16", 4104, 0)


def test_idc_create_refuses_before_it_asks_for_a_device():
    """IDC_ERR_INVALID_ARG with the reason, whether or not the machine has a GPU; an addressable geometry gets past the check (and, without a
    device, to IDC_ERR_NO_DEVICE)."""
    from interactive_deep_colorization_amd import _native as N
    lib = N.load()
    h = ctypes.c_void_p()
    for precision, size in ((N.IDC_BF16, 8192), (N.IDC_FP32, 2896)):
        assert lib.idc_create(0, size, size, 1, precision, 0, ctypes.byref(h)) == -1 and not h
        msg = lib.idc_last_error(None).decode()
        assert "%d x %d is too large for this precision" % (size, size) in msg and "2^31 bytes" in msg, msg
    if lib.idc_device_count() == 0:
        assert lib.idc_create(0, 4096, 4096, 1, N.IDC_BF16, 0, ctypes.byref(h)) == -2
        assert lib.idc_create(0, 8192, 8192, 1, N.IDC_FP16X3, 0, ctypes.byref(h)) == -2
