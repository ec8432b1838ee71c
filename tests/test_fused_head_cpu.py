"""tests/fused_head_ref.py without a GPU: the restatement against torch, the quantised weights, the non-saturation condition on the oracle's
own forward, and proof that the 1e-3 cap of tests/test_fused_head_gpu.py's bar can see the faults it is there for: each deliberately wrong
restatement, applied to a synthetic non-negative bf16-valued conv10_1 of the GPU cases' shapes, moves the output by more than the cap
(the bar itself, 4 x the measured error, is below the cap)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_lattice as xl
import fused_head_ref as fh

FAULTS = ["drop_product", "edge_replication", "plain_relu", "no_head_bias", "swap_channels", "bf16_conv10_2"]


def _weights(make_sd):
    sd = fh.state_dict(make_sd(fh.WEIGHT_SEED, fh.WEIGHT_STYLE))
    return sd["model10.1.weight"], sd["model10.1.bias"], sd["model_out.0.weight"], sd["model_out.0.bias"]


def _x(shape):
    """A stand-in for the stored conv10_1 (a ReLU output in bf16 storage): half zeros, O(1) values, bf16-exact, different per image."""
    H, W, n = fh.SHAPES[shape]
    rs = np.random.RandomState(11)
    return xl.bf16_rne(np.maximum(rs.standard_normal((n, 128, H, W)) * 1.2, 0).astype(np.float32))


def test_bar_and_cap():
    assert fh.FUSED_HEAD_CAP == 1e-3 and fh.FUSED_HEAD_BAR == 4 * fh.FUSED_HEAD_MEASURED and 0 < fh.FUSED_HEAD_BAR <= fh.FUSED_HEAD_CAP


def test_quantised_weights_are_exact_in_every_operand_format(make_sd):
    w = make_sd(fh.WEIGHT_SEED, fh.WEIGHT_STYLE)["model10.1.weight"]
    q = fh.quantise_weights(w)
    assert np.array_equal(xl.bf16_rne(q), q)                                             # bf16, and the hi part of a bf16 split: the lo parts are zero
    assert np.array_equal(q.astype(np.float16).astype(np.float32), q)                    # fp16: 8 significant bits, normal numbers
    assert (np.abs(q[q != 0]) >= fh.W_FLOOR).all() and xl.significant_bits(q) <= 8
    assert (q != 0).mean() >= 0.99 and np.abs(q - w).max() <= 2.0 ** -9 * np.abs(w).max() + fh.W_FLOOR
    s = np.float32(2.0 ** (13 - np.floor(np.log2(np.abs(q).max()))))                     # fp16x3's pre-scale: max|w| into [8192, 16384) (idc_pack.hip)
    assert 8192 <= np.abs(q).max() * s < 16384
    assert np.array_equal((q * s).astype(np.float16).astype(np.float32), q * s)          # ... keeps every weight exact, the lo part zero


@pytest.mark.parametrize("shape", ["A", "B"])
def test_the_restatement_is_torchs_float64_head(make_sd, shape):
    w, b, wo, bo = _weights(make_sd)
    x = _x(shape)
    y = F.leaky_relu(F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=1), 0.2)
    pre = F.conv2d(y, torch.from_numpy(wo).double(), torch.from_numpy(bo).double())
    out, mine_pre = fh.fused_head(x, w, b, wo, bo)
    assert out.shape == (x.shape[0], 2) + x.shape[2:]
    assert np.abs(mine_pre - pre.numpy()).max() <= 1e-12 and np.abs(out - 110.0 * torch.tanh(pre).numpy()).max() <= 1e-10


@pytest.mark.parametrize("shape", ["A", "B"])
def test_the_oracles_pre_tanh_sums_are_inside_the_live_range(make_sd, shape):
    """The seed of the GPU cases: in the oracle's float64 forward at least 90 % of the pre-tanh sums lie inside +-2, the images and the two
    planes differ."""
    from oracle import siggraph_torch
    import heads_ref as hr
    sd = fh.state_dict(make_sd(fh.WEIGHT_SEED, fh.WEIGHT_STYLE))
    L, ab, m = hr.images(shape)
    out, _, acts = siggraph_torch.forward(sd, L, ab, m, 0.0, dtype=torch.float64, return_acts=True)
    ref, pre = fh.fused_head(acts["conv10_1"], sd["model10.1.weight"], sd["model10.1.bias"], sd["model_out.0.weight"], sd["model_out.0.bias"])
    assert np.abs(ref - out).max() <= 1e-9                    # the restatement from the oracle's conv10_1 is the oracle's output
    assert (np.abs(pre) < fh.LIVE_RANGE).mean() >= fh.LIVE_SHARE
    assert np.abs(ref[0] - ref[1]).max() > 1.0 and np.abs(ref[:, 0] - ref[:, 1]).max() > 1.0


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("shape", ["A", "B"])
def test_mutants_move_the_output_beyond_the_cap(make_sd, shape, fault):
    w, b, wo, bo = _weights(make_sd)
    x = _x(shape)
    H, W, n = fh.SHAPES[shape]
    ref, pre = fh.fused_head(x, w, b, wo, bo)
    assert (np.abs(pre) < fh.LIVE_RANGE).mean() >= fh.LIVE_SHARE
    sites = [(n - 1, H - 1, W - 1), (1, 0, 0), (0, min(7, H - 1), min(31, W - 1))] if fault == "drop_product" else [None]
    for site in sites:
        bad, _ = fh.fused_head(x, w, b, wo, bo, fault=fault, site=site)
        moved = float(np.abs(bad - ref).max())
        print("fused head mutant %s %s %s: moves the output by %.3e (cap %.1e)" % (shape, fault, site, moved, fh.FUSED_HEAD_CAP))
        assert moved > fh.FUSED_HEAD_CAP
