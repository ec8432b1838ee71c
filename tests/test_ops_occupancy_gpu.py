"""Exact conv tests on grids that fill the chip: replicated lattice batches, bit for bit, with the kernel that ran asserted.

tests/test_ops_exact_gpu.py holds every conv template to bit equality at a quarter of the network's spatial size with two or three images: 4 to
about 40 workgroups on 256 CUs.  Here the same rows (imported, with run_case's mechanics) run where a synchronisation fault has room to show:
two workgroups of a kernel on one CU, a second wave of workgroups that starts while the first drains, block indices in the thousands through
xcd_remap and the bid -> (tile, parity, n, cout group) walk, batch indices in the hundreds.  The batch is a few DISTINCT lattice images in a
seeded order with no two neighbours equal (tests/occupancy_lattice.py); on the lattice every summation order gives the same bits, so the
expected output is exp[order] of one float64 computation of the distinct images and EVERY image of the batch is compared.  A failure names
the image, its place in the order, the tile, and whether the other copies of that distinct image agree among themselves.

  throughput rows   n_big = the smallest batch with workgroups >= 2 * 256 * residency(label) and >= 1024 (asserted on the CPU for every row:
                    tests/test_ops_occupancy_cpu.py); the policy batch stays the exact table's
  half-form pair    conv_ds_fused_m / _mh "half" at the largest batch with blocks < CUs and the 8-wave form one image later: either side of the
                    only grid-dependent kernel choice (conv_ds_m_half); the CU count is read from the device
  batch-1 rows      conv_kwave_bf16 / _deconv, conv_click, conv_wino_f32 / _deconv at the level sizes of ONE 256 x 256 image, two distinct images
  whole network     32 images = 4 distinct x 8 copies through the max_batch = 32 handles (bf16, fp16x3), 264 = 4 x 66 through a 64 x 64 bf16
                    handle: every copy bit for bit its first copy, the four first copies equal to the image sent alone.  The only route to
                    conv1_block_fused, the split model1 pair and the fused tanh head at a chip-filling grid.

Grids as traced on an MI355X (256 CUs), one `rocprofv3 --kernel-trace` run of this file, against occupancy_lattice.workgroups:
every launch of every row has the grid workgroups() states, none differs (workgroups x threads; residency as restated):
  conv_igemm_v2p<4,2,1> 1024 x 512 (1)   v2p<4,2,2> 1024 x 512 (1)   v2p<2,2,1> 1026 x 256 (2), plain and stride 2
  conv_igemm_v2m<2,4,1> 1024 x 512 (1)   v2m<4,2,1> 1024 x 512 (1)   v2m<2,2,2> 1024 x 256 (1)   v2m<2,4,0> 1025 x 512 (1)
  conv_ds_fused_m<2> 1024 x 512 (1)      conv_igemm<bf16,2,2,1> 1032 x 256 (2)                    conv_igemm<f32,2,2,1> 1044 x 256 (2)
  conv_igemm_v2ph<4,2,1> 1024 x 512 (1)  v2ph<2,2,1> 1026 x 256 (2)  v2sh<2,4,1> 1024 x 512 (1)  conv_ds_fused_mh<2> 1024 x 512 (1)
  conv_igemm_v2ps<4,2,1> 1024 x 512 (1), x3 and x6   v2psh<4,2,2> 1024 x 512 (1)   v2s<2,4,1> 1024 x 512 (1)   v2s<4,2,1> 1024 x 512 (1)
  conv_ds_fused_ms 1030 and 1024 x 512 (1)   conv_ds_fused_msh 1026 x 512 (1)
  half-form pair: conv_ds_fused_m<1> / _mh<1> 500 x 256 at 25 images, conv_ds_fused_m<2> / _mh<2> 260 x 512 at 26
  batch-1: conv_kwave_bf16<8,1,8> 512 x 512 (d = 1 and 2)   <4,2,8> 512 x 512   <2,2,4> 1024 x 256   conv_kwave_deconv_bf16<8> 512 x 512   <4> 1024 x 512
           conv_click<bf16,4,1> 512 x 256   conv_click<bf16,2,2> 384 x 128   conv_click<f32,4,2> 1024 x 256   conv_wino_f32<1,2> 512 x 512 (d = 1 and 2)
           conv_wino_deconv_f32<1> 512 x 768
  network, 32 x 256 x 256: conv1_block_fused_t 5632, conv_igemm_v2p<2,2,1> 2048 / 1024 / 8192 (+head), v2p<4,2,1> 512 and 256, v2p<4,2,2> 256,
           conv_ds_fused_m<2> 512 / 1024 / 4096; fp16x3: conv1_1_split_kernel 4096, conv1_2_split_kernel 5632, v2psh and conv_ds_fused_msh as bf16's;
           264 x 64 x 64: conv1_block_fused_t 3168, v2p<2,2,1> 1056 / 4224, v2p<4,2,*> 528, conv_ds_fused_m<2> 1056 / 2112
The trace reports static LDS only (0 for every kernel here: all of it is dynamic), so the LDS term of residency() stays a restatement of the
launchers; it reports at most 140 vector registers for any of these kernels, which does not lower a residency of 2 (512 per SIMD lane).

Wall time of this file on an MI355X, as measured there: 6.8 s for its 40 tests (pytest's own figure, under the trace); the slowest are the two
max_batch = 32 handles at 0.5 s, every op case is below 0.35 s.
"""
import time

import numpy as np
import pytest
import torch

import exact_lattice as xl
import large_ref as lr
import occupancy_lattice as ol
from interactive_deep_colorization_amd import engine, workloads
from test_ops_exact_gpu import SHIPPED, _reset_policies, run_case  # noqa: F401  (_reset_policies: the autouse fixture that restores the options)

pytestmark = pytest.mark.gpu

HEADROOM = 1.25                            # tests/test_large_batch_gpu.py's free-memory condition


def _run(c, d, exp, order, n):
    t0 = time.time()
    got, label = run_case(c, d)
    dt = time.time() - t0
    assert label == c.label, "%s ran %r, the table expects %r" % (c.id, label, c.label)
    assert got.shape[0] == n == len(order)
    ol.compare_replicated(got, exp, order, c, label, "%s [%s, %d images, %d workgroups]" % (c.id, label, n, ol.workgroups(c, n, label)))
    print("%s: %s, n = %d, %d workgroups, residency %d, op call %.2f s" % (c.id, label, n, ol.workgroups(c, n, label), ol.residency(label, c), dt))


@pytest.mark.parametrize("c", ol.ROWS, ids=[c.id for c in ol.ROWS])
def test_throughput_family_on_a_full_chip(c):
    n_big = ol.smallest_batch(c)
    d, exp, order = ol.replicate(c, n_big)
    _run(c, d, exp, order, n_big)


@pytest.mark.parametrize("pair", ol.HALF_PAIRS, ids=[p[0].id for p in ol.HALF_PAIRS])
def test_ds_half_form_on_either_side_of_its_switch(pair):
    c_half, c_past = pair
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    batches = ol.half_pair_batches(c_half, cus)
    if batches is None:
        pytest.skip("%s: %d workgroups per image cannot straddle %d CUs with %d distinct images" % (
            c_half.id, ol.workgroups(c_half, 1, c_past.label), cus, c_half.n))
    n_half, n_past = batches
    assert ol.workgroups(c_half, n_half, c_half.label) == 2 * ol.workgroups(c_half, n_half, c_past.label) < 2 * cus
    for c, n in ((c_half, n_half), (c_past, n_past)):
        d, exp, order = ol.replicate(c, n)
        _run(c, d, exp, order, n)


@pytest.mark.parametrize("c", ol.BATCH1_ROWS, ids=[c.id for c in ol.BATCH1_ROWS])
def test_batch1_family_at_the_network_level_sizes(c):
    d = xl.draw(c)
    exp = xl.expected(c, d)
    _run(c, d, exp, np.arange(c.n), c.n)


# ---- whole network, replicated ---------------------------------------------------------------------------------------------------------
DISTINCT = 4
NETWORK = [dict(id="%s-256x256x%d" % (p, mb), precision=p, size=256, max_batch=mb, seed=50) for mb, p in SHIPPED if mb >= 16]
NETWORK.append(dict(id="bf16-64x64x264", precision="bf16", size=64, max_batch=264, seed=51))


def _first_difference(a, b):
    bad = np.argwhere(a != b)
    ch, y, x = (int(v) for v in bad[0])
    return "%d of %d values differ, first at (channel %d, y %d, x %d): %r against %r; rows %d..%d, columns %d..%d" % (
        len(bad), a.size, ch, y, x, float(a[ch, y, x]), float(b[ch, y, x]), bad[:, 1].min(), bad[:, 1].max(), bad[:, 2].min(), bad[:, 2].max())


@pytest.mark.parametrize("c", NETWORK, ids=[c["id"] for c in NETWORK])
def test_every_copy_of_a_replicated_batch_equals_the_image_alone(make_sd, c):
    precision, size, nb = c["precision"], c["size"], c["max_batch"]
    assert (32, "bf16") in SHIPPED and (32, "fp16x3") in SHIPPED and nb % DISTINCT == 0
    need = lr.device_bytes(precision, size, size, nb)
    free, total = torch.cuda.mem_get_info(0)
    if free < HEADROOM * need:
        pytest.skip("%s needs %.2f GiB on the device x %.2f headroom; %.2f of %.2f GiB are free" % (
            c["id"], need / 2.0 ** 30, HEADROOM, free / 2.0 ** 30, total / 2.0 ** 30))
    order = ol.balanced_order(c["seed"], DISTINCT, nb // DISTINCT)
    assert (order[1:] != order[:-1]).all() and (np.bincount(order) == nb // DISTINCT).all()
    L4, ab4, m4 = workloads.random_batch(DISTINCT, size, seed=c["seed"])
    e = engine.HipColorizer(size, size, max_batch=nb, precision=precision)
    try:
        e.load_state_dict(make_sd(0, "he"))                    # full tanh range: the images differ everywhere
        t0 = time.time()
        full = e.forward(L4[order], ab4[order], m4[order], 0.0)
        dt = time.time() - t0
        assert full.shape == (nb, 2, size, size) and np.isfinite(full).all()
        first = [int(np.flatnonzero(order == k)[0]) for k in range(DISTINCT)]
        for a in range(DISTINCT):
            for b in range(a + 1, DISTINCT):
                assert not np.array_equal(full[first[a]], full[first[b]]), "distinct images %d and %d give the same output" % (a, b)
        wrong = [(i, int(order[i])) for i in range(nb) if not np.array_equal(full[i], full[first[order[i]]])]
        if wrong:
            i, k = wrong[0]
            copies = [int(j) for j in np.flatnonzero(order == k)]
            raise AssertionError("%s: %d of %d images differ from the first copy of their distinct image: %s; image %d (copy %d of %d of distinct image %d, "
                                 "first copy at %d): %s" % (c["id"], len(wrong), nb, wrong[:8], i, copies.index(i) + 1, len(copies), k, first[k],
                                                            _first_difference(full[i], full[first[k]])))
        for k in range(DISTINCT):
            alone = e.forward(L4[k:k + 1], ab4[k:k + 1], m4[k:k + 1], 0.0)
            assert np.array_equal(full[first[k]], alone[0]), "%s: image %d (first copy of distinct image %d) differs from the image sent alone: %s" % (
                c["id"], first[k], k, _first_difference(full[first[k]], alone[0]))
        kernels = sorted(set(r["kernel"] for r in e.layer_table() if r["launches"] > 0))
    finally:
        e.close()
    print("%s: forward of %d images %.3f s; kernels %s" % (c["id"], nb, dt, kernels))
