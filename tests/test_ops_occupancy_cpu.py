"""CPU side of the occupancy tests (tests/test_ops_occupancy_gpu.py): replicate()'s properties, the grid and size conditions of every GPU row,
the CU straddle of the half-form pair, workgroups() against a brute-force count of (tile, parity, image, cout-group) tuples, and a mutation
check of the replicated comparison.  None of it touches the library.

The mutation check applies three faults of ONE workgroup to one tile of one copy of a materialised expected batch (512 -> 512, 7 x 33, the trunk's
8-wave tile): the tile holds another copy's values, one tap of one 32-channel chunk is missing from its sums, the tile of image k was written
into image k - 1.  compare_replicated must catch each and name image and tile.  The same faults on Gaussian operands of the same shape, under
test_ops_gpu.py's bound 2.5e-2 * (1 + max|ref|), are printed, not asserted; what came out (pytest -s):
    tile of another copy              exact: caught   Gaussian bound: caught   (max|err| 4.5, bound 0.14)
    one tap of one 32-channel chunk   exact: caught   Gaussian bound: caught   (max|err| 0.46, bound 0.14)
    tile of image k in image k - 1    exact: caught   Gaussian bound: caught   (max|err| 4.5, bound 0.14)
So at this shape the Gaussian bound would have seen all three, the dropped tap included: 32 missing products of a K = 4608 sum have a spread
of 0.083, the bound is 1.7 of that, and a whole tile (7 x 32 pixels x 512 couts) holds 114 688 draws of it.  The bound lets a dropped tap
through only where a few dozen outputs carry it (tests/test_ops_exact_cpu.py: one product, a truncating store).  What the exact rows add to the
Gaussian ones at these grids is therefore those smaller faults, the localisation (image, copy, tile, whether the other copies agree), no bound
to tune, and every image of the batch compared.
"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_lattice as xl
import occupancy_lattice as ol

BF16_TOL = 2.5e-2            # tests/test_ops_gpu.py: |err| <= 2.5e-2 * (1 + max|ref|) on the bf16 path


# ---- replicate ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_big,distinct", [(3, 3), (4, 3), (25, 3), (26, 3), (29, 3), (171, 3), (512, 3), (2, 2), (9, 2), (32, 4), (264, 4)])
def test_order_has_no_equal_neighbours_and_meets_the_counts(n_big, distinct):
    for seed in (0, 1, 12345):
        order = ol.make_order(seed, n_big, distinct)
        assert order.shape == (n_big,) and order.min() >= 0 and order.max() < distinct
        assert (order[1:] != order[:-1]).all()
        assert np.bincount(order, minlength=distinct).min() >= n_big // (distinct + 1)
        np.testing.assert_array_equal(order, ol.make_order(seed, n_big, distinct))          # seeded


@pytest.mark.parametrize("distinct,copies", [(4, 8), (4, 66), (2, 5), (3, 7)])
def test_balanced_order_has_exact_counts(distinct, copies):
    order = ol.balanced_order(50, distinct, copies)
    assert (order[1:] != order[:-1]).all() and (np.bincount(order, minlength=distinct) == copies).all()


SMALL = [ol.occupancy_row("bf16_v2p_22_half_tiles"), ol.occupancy_row("bf16_ds_8wave_256")]


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.id)
def test_expected_of_the_order_is_expected_of_the_materialised_batch(c):
    """exp[order] is what exact_lattice.expected gives for the batch as the device sees it."""
    n_big = 11
    d, exp, order = ol.replicate(c, n_big)
    assert d["x"].shape[0] == n_big and all(d[k].shape[0] == n_big for k in ("resid", "x2") if k in d)
    small = xl.draw(c)
    for k in ("x", "resid", "x2"):
        if k in d:
            np.testing.assert_array_equal(d[k], small[k][order])
    for k in ("w", "b", "w2", "b2", "bn_s", "bn_t"):
        if k in d:
            np.testing.assert_array_equal(d[k], small[k])
    np.testing.assert_array_equal(exp[order], xl.expected(c._replace(n=n_big), d))
    assert not exp.flags.writeable
    for a, b in itertools.combinations(range(c.n), 2):
        assert not np.array_equal(exp[a], exp[b])                                          # the distinct images are distinct in the output too


# ---- the conditions of every GPU row ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ol.ROWS, ids=lambda c: c.id)
def test_throughput_row_fills_the_chip_within_the_host_cap(c):
    res = ol.residency(c.label, c)
    n_big = ol.smallest_batch(c)
    wgs = ol.workgroups(c, n_big, c.label)
    print("%s: %s  n_big %d  workgroups %d  residency %d  host %.0f MiB" % (c.id, c.label, n_big, wgs, res, ol.host_bytes(c, n_big) / 2.0 ** 20))
    assert 1 <= res <= ol.residency(c.label)
    assert wgs >= 2 * ol.CUS * res, "no second wave of co-resident workgroups"
    assert wgs >= ol.MIN_GRID
    too_few = ol.workgroups(c, n_big - 1, c.label)
    assert too_few < 2 * ol.CUS * res or too_few < ol.MIN_GRID, "n_big is not the smallest such batch"
    assert ol.host_bytes(c, n_big) < ol.HOST_CAP
    assert n_big > 2 and (c.h, c.w) in ((7, 33), (5, 9), (10, 18), (20, 36), (40, 72), (8, 16))      # batch index beyond 2; the table's ragged sizes
    assert c.policy >= 16 or c.tile == "large"
    d, exp, order = ol.replicate(c, min(n_big, 8))                                             # the lattice bounds hold under the row's own draw
    assert exp.shape[0] == c.n == 3


def test_rows_cover_the_families_the_issue_names():
    labels = [c.label for c in ol.ROWS]
    for want in ("conv_igemm_v2<4,2>+m16p", "conv_igemm_v2<2,2>+m16p", "conv_igemm_v2<2,4>+m16", "conv_igemm_v2<4,2>+m16", "conv_igemm_v2<2,2>+m16",
                 "conv_ds_fused_m+shortcut 8-wave", "conv_igemm<bf16,2,2>", "conv_igemm<f32,2,2>", "conv_igemm_v2ph<4,2>", "conv_igemm_v2ph<2,2>",
                 "conv_igemm_v2sh<2,4>x1", "conv_ds_fused_mh+shortcut 8-wave", "conv_igemm_v2ps<4,2>x3", "conv_igemm_v2ps<4,2>x6", "conv_igemm_v2psh<4,2>x3",
                 "conv_igemm_v2s<2,4>x3", "conv_igemm_v2s<4,2>x6", "conv_ds_fused_ms+shortcut x3", "conv_ds_fused_ms+shortcut x6", "conv_ds_fused_msh+shortcut x3"):
        assert want in labels, want
    assert labels.count("conv_igemm_v2<4,2>+m16p") == 2 and {c.dilation for c in ol.ROWS if c.label == "conv_igemm_v2<4,2>+m16p"} == {1, 2}
    assert {c.in_stride for c in ol.ROWS if c.label == "conv_igemm_v2<2,2>+m16p"} == {1, 2}
    assert any(c.ksize == 1 and c.cout == 529 for c in ol.ROWS) and any(c.out_f32 for c in ol.ROWS if c.label == "conv_igemm<bf16,2,2>")
    b1 = [(c.label.split(" ")[0], c.cin, c.h, c.w, c.dilation) for c in ol.BATCH1_ROWS]
    for want in (("conv_kwave_bf16", 512, 32, 32, 1), ("conv_kwave_bf16", 512, 32, 32, 2), ("conv_kwave_bf16", 256, 64, 64, 1), ("conv_kwave_bf16", 128, 128, 128, 1),
                 ("conv_kwave_deconv_bf16", 512, 32, 32, 1), ("conv_kwave_deconv_bf16", 256, 64, 64, 1), ("conv_click<bf16,1,4>", 256, 64, 64, 1),
                 ("conv_click<bf16,1,2>", 512, 7, 33, 2), ("conv_click<f32,1,4>", 512, 32, 32, 2), ("conv_wino_f32", 512, 32, 32, 1),
                 ("conv_wino_f32", 512, 32, 32, 2), ("conv_wino_deconv_f32", 512, 32, 32, 1)):
        assert want in b1, want
    assert all(c.n == 2 and (c.policy == 1 or c.precision == "fp32") for c in ol.BATCH1_ROWS)


@pytest.mark.parametrize("c", ol.BATCH1_ROWS, ids=lambda c: c.id)
def test_batch1_row_is_about_one_workgroup_per_cu_and_image(c):
    """The batch-1 families ship at a grid of about one workgroup per CU: each image of the row brings 192 .. 512 workgroups."""
    per_image = ol.workgroups(c, 1, c.label)
    print("%s: %s  %d workgroups per image, residency %d" % (c.id, c.label, per_image, ol.residency(c.label, c)))
    assert ol.workgroups(c, 2, c.label) == 2 * per_image and 192 <= per_image <= 512
    assert ol.host_bytes(c, c.n) < ol.HOST_CAP
    xl.assert_bounds(c, xl.draw(c))


@pytest.mark.parametrize("pair", ol.HALF_PAIRS, ids=lambda p: p[0].id)
def test_half_form_pair_straddles_256_cus(pair):
    c_half, c_past = pair
    assert c_half.label.endswith(" half") and c_past.label == c_half.label.replace(" half", " 8-wave") and c_half.cin2 == 64      # one shortcut chunk
    assert c_half._replace(id="", label="") == c_past._replace(id="", label="")
    n_half, n_past = ol.half_pair_batches(c_half, 256)
    assert (n_half, n_past) == (25, 26)
    blocks_half, blocks_past = ol.workgroups(c_half, n_half, c_past.label), ol.workgroups(c_past, n_past, c_past.label)
    assert blocks_half == 250 < 256 <= blocks_past == 260                        # blocks = CUs - 6: ten 128-cout workgroups per image
    assert ol.workgroups(c_half, n_half, c_half.label) == 500                    # two 64-cout workgroups per block
    assert ol.half_pair_batches(c_half, 20) is None and ol.half_pair_batches(c_half, 31) == (3, 4)
    assert ol.residency(c_half.label, c_half) == ol.residency(c_past.label, c_past) == 1          # 160 KiB of LDS per workgroup


# ---- workgroups against a brute-force count ----------------------------------------------------------------------------------------------------
def _tuples(c, n, label):
    """Count the (tile, parity, image, cout group, K slice) tuples of a launch by walking the output: every output pixel of every (image, cout group)
    is assigned to its workgroup, the workgroups are counted as a set."""
    g = ol.geometry(c)
    rows, cols = ol.launch(c, n, label)[4]
    ho, wo = xl.out_hw(c)
    d = g["d"] if label in ("conv_kwave_bf16", "conv_wino_f32") else 1
    seen = set()
    for y in range(ho):
        for x in range(wo):
            if g["so"] == 2 and not label.startswith(("conv_ds", "conv_kwave_deconv", "conv_wino_deconv")):
                # a deconv on a conv tile: one workgroup per output parity over a tile of INPUT sites
                seen.add((y // 2 // (rows // 2), x // 2 // (cols // 2), y % 2, x % 2))
            elif d > 1:
                # dilated sub-grids: a workgroup owns a block of ONE of the d x d sub-grids; every sub-grid gets the blocks of the largest one
                if y % d == 0 and x % d == 0:
                    seen.update(((y // d) // (rows // d), (x // d) // (cols // d), py, px) for py in range(d) for px in range(d))
            else:
                seen.add((y // rows, x // cols, 0, 0))
    return len(seen)


def _cout_groups_and_slices(c, label):
    """Workgroups along the cout axis and the K axis, from the label's template arguments."""
    cpad = ol.cout_pad(c.cout)
    m = ol._V2.match(label) or ol._IGEMM.match(label)
    if m:
        wm = int(m.group(2))
        ks = int(m.group(4) or 1) if ol._IGEMM.match(label) else 1
        return cpad // (64 * wm), ks
    m = ol._CLICK.match(label)
    if m:
        return cpad // 64, int(m.group(3) or 1)
    if ol._DS.match(label):
        return cpad // (64 if label.endswith(" half") else 128), 1
    if label == "conv_kwave_bf16":
        return cpad // 32, 1
    if label == "conv_wino_f32":
        return cpad // (16 * ol._wino_form(c, ol.geometry(c), c.n)[1]), 1
    return cpad // 16, 1                                            # conv_kwave_deconv_bf16, conv_wino_deconv_f32: 16 couts per workgroup


BRUTE = [(c._replace(h=h, w=w), n) for c in ol.ALL_ROWS if not c.id.endswith("past_half")
         for (h, w), n in zip(((c.h, c.w), (c.h + 6, c.w + 31), (2 * c.h, 2 * c.w + 2)), (c.n, 5, 7))]


@pytest.mark.parametrize("c,n", BRUTE, ids=["%s-%dx%dx%d" % (c.id, c.h, c.w, n) for c, n in BRUTE])
def test_workgroups_equal_a_brute_force_count(c, n):
    if c.in_stride == 2:
        c = c._replace(h=c.h + c.h % 2, w=c.w + c.w % 2)
    tiles = _tuples(c, n, c.label)
    groups, slices = _cout_groups_and_slices(c, c.label)
    assert ol.workgroups(c._replace(n=n), n, c.label) == tiles * n * groups * slices, (tiles, n, groups, slices)


# ---- mutation check ----------------------------------------------------------------------------------------------------------------------
MUT = ol.occupancy_row("bf16_v2p_42_halo1")
N_MUT, IMG, TILE = 9, 5, (0, 0)                                    # the mutated copy and its tile: rows 0..6, columns 0..31 of the 7 x 33 image


def _tile_slice(c, label, tile):
    rows, cols = ol.launch(c, c.n, label)[4]
    return slice(tile[0] * rows, (tile[0] + 1) * rows), slice(tile[1] * cols, (tile[1] + 1) * cols)


def _mutants(full, dropped, order):
    """The three faults on a materialised batch `full` (dropped: the batch with one tap of one 32-channel chunk missing from every sum)."""
    ys, xs = _tile_slice(MUT, MUT.label, TILE)
    other = int(np.flatnonzero(order != order[IMG])[0])
    out = {}
    m = full.copy(); m[IMG, :, ys, xs] = full[other, :, ys, xs]; out["tile of another copy"] = (m, IMG)
    m = full.copy(); m[IMG, :, ys, xs] = dropped[IMG, :, ys, xs]; out["one tap of one 32-channel chunk"] = (m, IMG)
    m = full.copy(); m[IMG - 1, :, ys, xs] = full[IMG, :, ys, xs]; out["tile of image k in image k - 1"] = (m, IMG - 1)
    return out


def test_the_replicated_comparison_catches_one_workgroups_faults():
    c = MUT
    d, exp, order = ol.replicate(c, N_MUT)
    assert order[IMG] != order[IMG - 1]
    full = exp[order]
    ol.compare_replicated(full, exp, order, c, c.label, "unmutated")
    small = xl.draw(c)
    w2 = small["w"].copy()
    w2[:, 64:96, 0, 2] = 0                                          # tap (ky 0, kx 2) of channels 64..95
    assert np.abs(small["w"][:, 64:96, 0, 2]).max() > 0
    dropped = xl.expected(c, dict(small, w=w2))[order]

    # the same shape on Gaussian operands (tests/test_ops_gpu.py's: x ~ N(0, 1), w ~ N(0, 1) / sqrt(9 cin)), float64 reference, bf16-stored result
    rs = np.random.RandomState(7)
    gx = rs.standard_normal((c.n, c.cin, c.h, c.w)).astype(np.float32)
    gw = (rs.standard_normal((c.cout, c.cin, 3, 3)) / np.sqrt(c.cin * 9)).astype(np.float32)
    gw2 = gw.copy(); gw2[:, 64:96, 0, 2] = 0
    conv = lambda w: np.maximum(F.conv2d(torch.from_numpy(gx).double(), torch.from_numpy(w).double(), padding=1).numpy(), 0.0)
    gref = conv(gw)[order]
    gfull, gdropped = xl.bf16_rne(gref.astype(np.float32)), xl.bf16_rne(conv(gw2)[order].astype(np.float32))
    bound = BF16_TOL * (1 + np.abs(gref).max())
    assert np.abs(gfull - gref).max() <= bound

    gauss = _mutants(gfull, gdropped, order)
    for name, (mutant, image) in _mutants(full, dropped, order).items():
        assert not np.array_equal(mutant, full), name
        with pytest.raises(AssertionError) as info:
            ol.compare_replicated(mutant, exp, order, c, c.label, name)
        msg = str(info.value)
        copies = np.flatnonzero(order == order[image])
        assert "first at (n=%d," % image in msg and "image %d is copy %d of %d of distinct image %d" % (
            image, int(np.searchsorted(copies, image)) + 1, len(copies), order[image]) in msg, msg
        assert "tile (row %d, column %d)" % TILE in msg and "1 (image, tile) pairs differ: [(%d, %d, %d)]" % ((image,) + TILE) in msg, msg
        assert "agree among themselves, %d of them equal the expectation" % (len(copies) - 1) in msg, msg
        gerr = np.abs(gauss[name][0] - gref).max()
        print("%-32s exact: caught   Gaussian bound: %s   (max|err| %.2g, bound %.2g)" % (name, "caught" if gerr > bound else "PASSES", gerr, bound))


def test_copies_that_disagree_are_reported():
    c = MUT
    d, exp, order = ol.replicate(c, N_MUT)
    bad = exp[order].copy()
    k = int(order[IMG])
    copies = np.flatnonzero(order == k)
    bad[copies[0], 3, 2, 32] += 1
    bad[copies[-1], 9, 6, 1] += 1
    with pytest.raises(AssertionError) as info:
        ol.compare_replicated(bad, exp, order, c, c.label, "two copies")
    assert "2 (image, tile) pairs differ" in str(info.value)
    assert len(copies) > 2
    assert "DISAGREE among themselves, %d of them equal the expectation" % (len(copies) - 2) in str(info.value)
