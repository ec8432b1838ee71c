"""model1's kernels, bit for bit, through a forward: conv1_block_fused_t<4,3,true> / <4,2,true> and their fp16 twins conv1_block_fused_th,
conv1_1_split_kernel + conv1_2_split_kernel (bf16x3, bf16x6, fp16x3 and the one-part fp16 form), conv_igemm reading the fused input pack
(fp32 and bf16, with the conv1_2 launch that follows it), and conv1_1_bf16_kernel in a -DIDC_AB_PARTNERS build.

These kernels have no single-operator entry: their input is the three planes a forward is handed.  tests/model1_ref.py puts the integer
lattice of tests/exact_lattice.py there -- planes that pack to the integers -2..2, lattice model1 weights, a BN whose fold is a power of two
and an integer -- so activation("conv1_2") (and activation("conv1_1") where it is its own launch) is ONE float64 computation plus the storage
rounding of the path, compared with exact_lattice.compare.  No tolerance appears in this file.  That sees what the older tolerance tests
(tests/test_net_gpu.py::test_conv1_1_throughput_kernel, tests/test_round6_gpu.py: the split kernels and the fp16 twin against a sibling
kernel or the oracle at 2e-4 .. 4e-3 * (1 + max|ref|)) cannot: one tap-channel product of conv1_2 (1/576 of a sum) lost at a 32 x 12 tile
corner, a halo pixel taken from the next image, a conv1_1 halo site not zeroed outside the image, a truncating 16-bit store
(tests/test_model1_exact_cpu.py holds each of these faults against the same data).

One handle per row at 40 x 72 -- 12+12+12+4 rows for the 32 x 12 tile, five 8-row tiles, 16+16+8 for the split conv1_1 tile, 32+8 for the
32 x 32 form; 32+32+8 columns -- with the max_batch that selects the row's variant (model1_ref.ROWS has the arithmetic) and THREE images per
forward, each its own draw (the two max_batch = 1 handles take them one call each; max_batch 3 plans the same kernels and carries them together).  Every row first asserts the layer_table() labels of conv1_1 and conv1_2, then compares, then forwards image 1
alone and requires the same bits.  The rest of the network runs on its seeded weights; only model1's tensors are read.

test_shipped_model1_kernels_are_all_in_the_rows builds the shipped 256 x 256 configurations and (32, "fp16"), and fails when their conv1_1 /
conv1_2 rows name a kernel no row here asserted.

Wall time of this file on an MI355X: 7.7 s for its 20 cases (15 handles at 40 x 72, five 256 x 256 census handles); the slowest case takes
0.8 s (the fp32 handles: their Winograd weight images), every other 0.2 - 0.65 s.
"""
import re

import numpy as np
import pytest

import exact_lattice as xl
import model1_ref as m1
from interactive_deep_colorization_amd import engine, workloads

pytestmark = pytest.mark.gpu

_OPTION_DEFAULTS = {"op_policy_batch": 0, "winograd": 1, "ds_mfma16": 1, "kwave": 1, "click": -1, "v2p": 1, "fp16_fast": 1, "split_ds_fuse": 1,
                    "fuse_conv1": 1, "conv1_1_split": 1, "conv1_2_split": 1}
SHIPPED = [(32, "bf16"), (32, "fp16x3"), (1, "bf16"), (1, "fp32"), (32, "fp16")]          # 256 x 256: (max_batch, precision)


@pytest.fixture(autouse=True)
def _reset_policies():
    yield
    engine.set_tile_policy("auto")
    engine.set_splitk_policy("auto")
    for name, value in _OPTION_DEFAULTS.items():
        engine.set_option(name, value)


def normalise(label):
    """A label without its split-K slice count (as tests/test_ops_exact_gpu.py::normalise)."""
    return re.sub(r" splitK\d+$", "", label)


def _labels(e):
    return {r["name"]: (r["kernel"], r["launches"]) for r in e.layer_table() if r["name"] in ("conv1_1", "conv1_2")}


@pytest.mark.parametrize("row", [r.id for r in m1.ROWS])
def test_model1_exact(make_sd, row):
    r = m1.BY_ID[row]
    if r.partner:
        from conftest import has_ab_partners
        if not has_ab_partners():
            pytest.skip("partner kernel: -DIDC_AB_PARTNERS build only")
    exp = m1.expected(r)                         # asserts the lattice, the BN fold, the bounds and the storage fit before anything runs on the GPU
    L, ab, mask, maskcent = m1.planes(r)
    for name, value in r.opts:
        engine.set_option(name, value)
    e = engine.HipColorizer(m1.H, m1.W, max_batch=r.max_batch, precision=r.precision)
    try:
        e.load_state_dict(m1.state_dict(r, make_sd(0, "he")))
        if r.max_batch >= m1.N:
            e.forward(L, ab, mask, maskcent)
            labels = _labels(e)
            got = {name: e.activation(name, m1.N) for name in r.read}
        else:                                    # a max_batch = 1 handle: the three images one call each
            parts = {name: [] for name in r.read}
            for i in range(m1.N):
                e.forward(L[i:i + 1], ab[i:i + 1], mask[i:i + 1], maskcent)
                labels = _labels(e)
                for name in r.read:
                    parts[name].append(e.activation(name, 1))
            got = {name: np.concatenate(parts[name]) for name in r.read}
        e.forward(L[1:2], ab[1:2], mask[1:2], maskcent)
        labels_1 = _labels(e)
        alone = {name: e.activation(name, 1) for name in r.read}
    finally:
        e.close()
    want = {"conv1_1": (r.conv1_1, 1), "conv1_2": (r.conv1_2, 0 if r.conv1_2.startswith("fused") else 1)}
    assert labels == want and labels_1 == want, "%s ran %r (one image: %r), the row expects %r" % (row, labels, labels_1, want)
    for name in r.read:
        xl.compare(got[name], exp[name], "%s %s [%s]" % (row, name, labels[name][0]))
    for name in r.read:
        xl.compare(alone[name], got[name][1:2], "%s %s: image 1 alone against image 1 of three" % (row, name))


@pytest.mark.parametrize("max_batch,precision", SHIPPED)
def test_shipped_model1_kernels_are_all_in_the_rows(make_sd, max_batch, precision):
    """What the shipped configurations launch for conv1_1 and conv1_2 is what a row above asserted (template arguments included; the
    layer table is filled by a forward's planning pass, so each handle runs ONE single-image forward)."""
    asserted = set(("conv1_1", normalise(r.conv1_1)) for r in m1.ROWS if not r.partner) | set(("conv1_2", normalise(r.conv1_2)) for r in m1.ROWS if not r.partner)
    e = engine.HipColorizer(256, 256, max_batch=max_batch, precision=precision)
    try:
        e.load_state_dict(make_sd(0, "he"))
        L, ab, m = workloads.random_batch(1, 256, seed=3)
        e.forward(L, ab, m, 0.0)
        labels = _labels(e)
    finally:
        e.close()
    assert set(labels) == {"conv1_1", "conv1_2"}
    missing = [(name, k) for name, (k, _) in sorted(labels.items()) if (name, normalise(k)) not in asserted]
    assert not missing, "shipped model1 kernels no row reaches (max_batch %d, %s): %s" % (max_batch, precision, missing)
