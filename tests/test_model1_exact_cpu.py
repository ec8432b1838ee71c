"""tests/model1_ref.py without a GPU: the reference's own assertions hold for every row's draw, it agrees with torch's float64 convolutions,
and exact_lattice.compare sees, on that drawn data, each fault tests/test_model1_exact_gpu.py is there for:
  one tap-channel term dropped at a tile-corner pixel (conv1_2 and conv1_1), a conv1_1 halo site outside the image left non-zero,
  the next image's border pixel used as halo (conv1_2's halo tile and the planes of the pack), a truncating 16-bit store, BN before the ReLU.
A fault counts as seen when compare raises on a tensor the row READS (the block's rows read conv1_2 only)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_lattice as xl
import model1_ref as m1

ROW_IDS = [r.id for r in m1.ROWS]
ROWS_READING_CONV1_2 = [r.id for r in m1.ROWS if "conv1_2" in r.read]


def _seen(r, fault, site=None):
    """Does compare fail on a tensor the row reads?  -> the names of those tensors."""
    good, bad = m1.expected(r), m1.expected(r, fault=fault, site=site)
    seen = []
    for name in r.read:
        try:
            xl.compare(bad[name], good[name], "%s %s %s" % (r.id, fault, site))
        except AssertionError:
            seen.append(name)
    return seen


@pytest.mark.parametrize("row", ROW_IDS)
def test_the_reference_asserts_hold_and_the_draw_is_a_test(row):
    r = m1.BY_ID[row]
    exp = m1.expected(r)                             # lattice, BN fold, bf16-exact conv1_1, bounds below 2^24, storage fit
    c1max, acc_bound, wino_bound, pre_bound = m1._stages(r)["bounds"]
    print("%s: max conv1_1 %d, bounds: K loop %.0f, Winograd (quarters) %.0f, before the store %.0f; conv1_2 within +-%.1f, %d significant bits" %
          (row, c1max, acc_bound, wino_bound, pre_bound, np.abs(exp["conv1_2"]).max(), xl.significant_bits(m1.expected(r)["conv1_2"])))
    c1, c2 = exp["conv1_1"], exp["conv1_2"]
    assert c1.shape == c2.shape == (m1.N, 64, m1.H, m1.W) and c1.dtype == c2.dtype == np.float32
    assert 0.2 <= (c1 > 0).mean() <= 0.8 and c1max >= 16             # the ReLU is live on both sides, the values use the range
    assert all(np.abs(c2[i] - c2[j]).max() > 0 for i in range(m1.N) for j in range(i))
    raw = m1._stages(r)["acc"]
    assert 0.3 <= (raw[:, :32] > 0).mean() <= 0.7 and (raw[:, 32:] > 256).mean() >= 0.3          # the zero-mean couts; the large ones, beyond bf16's exact integers
    if xl.STORAGE[r.precision] in ("bf16", "fp16"):                  # the 16-bit store rounds thousands of values UP: a truncating store shows
        assert (np.abs(c2) > np.abs(m1.expected(r, fault="truncating_store")["conv1_2"])).sum() >= 10000


@pytest.mark.parametrize("row", ["bf16_block_32x12", "fp32_batch1"])
def test_the_reference_is_torchs_float64_model1(row):
    r = m1.BY_ID[row]
    t = m1.model1_tensors(r)
    L, ab, mask, maskcent = m1.planes(r)
    x = torch.cat([torch.from_numpy(L).double() / 100.0, torch.from_numpy(ab).double() / 110.0, torch.from_numpy(mask).double() - maskcent], dim=1)
    c1 = F.relu(F.conv2d(x, torch.from_numpy(t["model1.0.weight"]).double(), torch.from_numpy(t["model1.0.bias"]).double(), padding=1))
    y = F.relu(F.conv2d(c1, torch.from_numpy(t["model1.2.weight"]).double(), torch.from_numpy(t["model1.2.bias"]).double(), padding=1))
    y = F.batch_norm(y, torch.zeros(64).double(), torch.from_numpy(t["model1.4.running_var"]).double(), torch.from_numpy(t["model1.4.weight"]).double(),
                     torch.from_numpy(t["model1.4.bias"]).double(), training=False, eps=1e-5)
    np.testing.assert_array_equal(m1._stages(r)["c1"], c1.numpy())
    st = m1._stages(r)
    mine = np.maximum(st["acc"], 0) * st["scale"][None, :, None, None].astype(np.float64) + st["shift"][None, :, None, None]
    assert np.abs(mine - y.numpy()).max() <= 1e-7 * np.abs(mine).max()          # torch's BN divides by sqrt(var + eps) that is 1 + 5e-9, not 1


def test_the_planes_are_the_lattice_and_touch_every_edge():
    for r in m1.ROWS:
        L, ab, mask, maskcent = m1.planes(r)
        assert maskcent == 0.0 and L.shape == (m1.N, 1, m1.H, m1.W) and ab.shape == (m1.N, 2, m1.H, m1.W) and mask.shape == L.shape
        x = m1.pack(L, ab, mask, maskcent)
        assert set(np.unique(x[:, :3])) == {-2.0, -1.0, 0.0, 1.0, 2.0} and set(np.unique(x[:, 3])) == {0.0, 1.0}
        for ys in ([0, m1.H - 1] + list(m1.TILE_EDGES_Y)):
            assert (x[:, :, ys, :] != 0).all()
        for xs in ([0, m1.W - 1] + list(m1.TILE_EDGES_X)):
            assert (x[:, :, :, xs] != 0).all()


def test_the_bn_fold_refuses_what_is_not_a_power_of_two():
    t = m1.model1_tensors(m1.ROWS[0])
    m1.bn_fold(t)
    t["model1.4.running_var"] = np.ones(64, np.float32)              # 1 / sqrt(1 + 1e-5) is not 1 in fp32
    with pytest.raises(AssertionError):
        m1.bn_fold(t)


# ---- mutants ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS_READING_CONV1_2)
def test_a_dropped_conv1_2_term_at_a_tile_corner_is_seen(row):
    r = m1.BY_ID[row]
    for site in m1.CORNERS:
        assert _seen(r, "drop_product", site) == ["conv1_2"], site


@pytest.mark.parametrize("row", ROW_IDS)
def test_a_dropped_conv1_1_term_at_a_tile_corner_is_seen(row):
    r = m1.BY_ID[row]
    for site in m1.CORNERS:
        assert _seen(r, "drop_product_conv1_1", site), site


@pytest.mark.parametrize("row", ROWS_READING_CONV1_2)
def test_a_halo_site_outside_the_image_left_non_zero_is_seen(row):
    r = m1.BY_ID[row]
    for site in m1.OUTSIDE:
        assert _seen(r, "halo_not_zeroed", site) == ["conv1_2"], site


@pytest.mark.parametrize("row", ROW_IDS)
def test_the_next_images_border_pixel_as_halo_is_seen(row):
    r = m1.BY_ID[row]
    for xs in m1.BELOW:
        assert _seen(r, "pack_next_image", (m1.H, xs)), xs
        if "conv1_2" in r.read:
            assert _seen(r, "next_image_halo", (m1.H, xs)) == ["conv1_2"], xs


@pytest.mark.parametrize("row", [r.id for r in m1.ROWS if xl.STORAGE[r.precision] in ("bf16", "fp16") and "conv1_2" in r.read])
def test_a_truncating_store_is_seen(row):
    assert _seen(m1.BY_ID[row], "truncating_store") == ["conv1_2"]


@pytest.mark.parametrize("row", ROWS_READING_CONV1_2)
def test_bn_before_the_relu_is_seen(row):
    assert _seen(m1.BY_ID[row], "bn_before_relu") == ["conv1_2"]


def test_the_rows_cover_the_variants():
    labels = set((r.conv1_1, r.conv1_2) for r in m1.ROWS)
    assert ("conv1_block_fused", "fused into conv1_1") in labels and ("conv1_1_split_kernel", "conv1_2_split_kernel x6") in labels
    assert sorted(set(r.precision for r in m1.ROWS)) == ["bf16", "bf16x3", "bf16x6", "fp16", "fp16x3", "fp32"]
    assert set(r.w_max for r in m1.ROWS) == {1, 2}
