"""The float64 restatements of tests/heads_ref.py against torch, and proof that the bars of tests/test_heads_gpu.py (heads_ref.*_BAR) can see the
faults they are there for: each deliberately wrong restatement, applied to synthetic inputs of the GPU cases' shapes, misses the right one
by at least 10 x the bar of its comparison."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import heads_ref as hr
from oracle import siggraph_torch, weights

GRIDS = {"A": (3, 10, 18), "B": (2, 4, 6)}               # n and the quarter grid of heads_ref.SHAPES


def _logits(shape, bins, seed=0):
    n, h, w = GRIDS[shape]
    return (np.random.RandomState(seed).standard_normal((n, bins, h, w)) * 4.0).astype(np.float32)


# ---- the restatements -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["A", "B"])
def test_bilinear_rule_is_the_two_grouped_deconvs(shape):
    l = _logits(shape, 7).astype(np.float64)
    k = torch.tensor(siggraph_torch.BILINEAR_US, dtype=torch.float64)[None, None].repeat(7, 1, 1, 1)
    up = F.conv_transpose2d(torch.from_numpy(l), k, None, stride=2, padding=1, groups=7)
    up = F.conv_transpose2d(up, k, None, stride=2, padding=1, groups=7).numpy()
    mine = hr.upsample4(l)
    assert mine.shape == up.shape
    assert np.abs(mine - up).max() <= 1e-12


def test_dist313_is_the_oracles_head():
    l = _logits("A", 313, 1)
    centres = weights.synthetic_ab_centres(0)
    bias = np.array([0.3, -0.7])
    t = torch.from_numpy(l.astype(np.float64))
    k = torch.tensor(siggraph_torch.BILINEAR_US, dtype=torch.float64)[None, None].repeat(313, 1, 1, 1)
    up = F.conv_transpose2d(F.conv_transpose2d(t, k, None, stride=2, padding=1, groups=313), k, None, stride=2, padding=1, groups=313)
    for S in (0.2, 1.0):
        dist, pred = hr.dist313(l, S, centres, bias)
        assert np.abs(dist - torch.softmax(up * S, dim=1).numpy()).max() <= 1e-12
        ref_p = F.conv2d(torch.softmax(up * 2.6, dim=1), torch.from_numpy(centres.T.astype(np.float64))[:, :, None, None], torch.from_numpy(bias))
        assert np.abs(pred - ref_p.numpy()).max() <= 1e-10


def test_softmax_and_head_against_torch():
    l = _logits("A", 529, 2)
    assert np.abs(hr.softmax529(l) - torch.softmax(torch.from_numpy(l.astype(np.float64)) * 0.2, dim=1).numpy()).max() <= 1e-14
    rs = np.random.RandomState(3)
    x = rs.standard_normal((2, 128, 8, 16))
    w, b = rs.standard_normal((2, 128, 1, 1)) * 0.05, rs.uniform(-0.1, 0.1, 2)
    ref = 110.0 * torch.tanh(F.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b))).numpy()
    assert np.abs(hr.head(x, w, b) - ref).max() <= 1e-11


def test_branch_restatement_against_the_oracle(golden):
    g = golden("glob64_he_s3")
    sd = weights.add_global_branch({}, int(g["weight_seed"]))
    ref = siggraph_torch.global_branch(sd, g["glob"], g["sat"], torch.float64).numpy()[:, :, 0, 0]
    mine = hr.glob_branch(sd, g["glob"], g["sat"])
    assert mine.shape == ref.shape == (g["glob"].shape[0], 512)
    assert np.abs(mine - ref).max() <= 1e-10 * (1 + np.abs(ref).max())
    glob, sat = hr.hint_rows()
    ref = siggraph_torch.global_branch(sd, glob, sat, torch.float64).numpy()[:, :, 0, 0]
    assert np.abs(hr.glob_branch(sd, glob, sat) - ref).max() <= 1e-10 * (1 + np.abs(ref).max())
    assert np.abs(hr.shift_difference(sd, glob, sat)[1]).max() <= 1e-12                      # the all-zero row IS the cleared input


def test_storage_ulp():
    assert hr.storage_ulp(1.0, "bf16") == 2.0 ** -7 and hr.storage_ulp(1.99, "bf16") == 2.0 ** -7 and hr.storage_ulp(-2.0, "bf16") == 2.0 ** -6
    assert hr.storage_ulp(1.0, "fp16") == 2.0 ** -10 and hr.storage_ulp(1e-9, "fp16") == 2.0 ** -24
    x = torch.tensor([0.3, 1.7, 93.2, 1e-3], dtype=torch.float32)
    for dt, p in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
        stored = x.to(dt).to(torch.float64).numpy()
        assert (np.abs(stored - x.numpy().astype(np.float64)) <= 0.5 * hr.storage_ulp(stored, p)).all()
        hi = x.to(dt).to(torch.float32)                      # a two-part split: the low part's ulp is below the figure of the table
        lo = (x - hi).to(dt).to(torch.float64).numpy()
        assert (hr.storage_ulp(lo, p) <= hr.storage_ulp(stored, {"bf16": "bf16x3", "fp16": "fp16x3"}[p])).all()


# ---- the hint rows separate the images, and the head is not saturated --------------------------------------------------------------------
_ORACLE = {}


def _oracle_sd(make_sd):
    if "sd" not in _ORACLE:
        sd = dict(make_sd(hr.WEIGHT_SEED, hr.WEIGHT_STYLE))
        weights.add_global_branch(sd, hr.GLOB_SEED)
        _ORACLE["sd"] = sd
    return _ORACLE["sd"]


def test_hint_rows_separate_the_images(make_sd):
    """In the reference the shift vectors of any two images differ by more than 100 x the bar on at least half of the channels, in every
    precision.  The bar of a 16-bit row is elementwise (ulps of the two stored values), so it is evaluated where the values are: on the
    oracle's own conv4_3 of shape A's images, with the hint rows and without, and a channel's bar is the median over its pixels."""
    sd = _oracle_sd(make_sd)
    glob, sat = hr.hint_rows()
    g = hr.glob_branch(sd, glob, sat)
    L, ab, m = hr.images("A")
    acts = siggraph_torch.forward(sd, L, ab, m, 0.0, return_acts=True)[2]
    v = acts["conv4_3"].astype(np.float64)                                                     # before any shift, (3,512,5,9)
    g0 = hr.glob_branch(sd, np.zeros((1, 314)))
    cleared = v + g0[:, :, None, None]
    fp32_bar = hr.SHIFT_REL_BAR * (1.0 + np.abs(g).max())
    for precision in hr.PRECISIONS:
        bar = [np.median(hr.shift_bar(v + g[k][None, :, None, None], cleared, precision, fp32_bar).transpose(1, 0, 2, 3).reshape(512, -1), axis=1)
               for k in range(3)]
        for i, j in ((0, 1), (0, 2), (1, 2)):
            frac = (np.abs(g[i] - g[j]) > 100.0 * np.maximum(bar[i], bar[j])).mean()
            assert frac >= 0.5, (precision, i, j, frac)


@pytest.mark.parametrize("shape", ["A", "B"])
def test_the_oracles_head_is_not_saturated(make_sd, shape):
    """The weight style and seed of the GPU cases: the oracle's output has |out| < 0.9 out_mul on at least half of the pixels (a saturated
    tanh hides a wrong sum), and the images and the two planes differ."""
    L, ab, m = hr.images(shape)
    out = siggraph_torch.forward(_oracle_sd(make_sd), L, ab, m, 0.0)
    assert (np.abs(out) < 0.9 * 110.0).mean() >= 0.5
    assert min((np.abs(o) < 0.9 * 110.0).mean() for o in out) >= 0.5
    assert np.abs(out[0] - out[1]).max() > 1.0 and np.abs(out[:, 0] - out[:, 1]).max() > 1.0


# ---- mutants: every listed fault is at least 10 x over the bar of its comparison --------------------------------------------------------
def _rel(p, ref):
    return float((np.abs(p - ref) / (ref + 1e-12)).max())


@pytest.mark.parametrize("fault", ["image0", "clamp", "swap_jyjx", "drop_group"])
@pytest.mark.parametrize("S", [0.2, 1.0])
@pytest.mark.parametrize("shape", ["A", "B"])
def test_mutants_of_dist313(shape, S, fault):
    l = _logits(shape, 313, 4)
    centres, bias = weights.synthetic_ab_centres(hr.PRED_SEED), np.array([0.5, -0.5])
    ref_d, ref_p = hr.dist313(l, S, centres, bias)
    bad_d, bad_p = hr.dist313(l, S, centres, bias, fault=fault)
    assert _rel(bad_d, ref_d) >= 10 * hr.P313_REL_BAR
    assert np.abs(bad_p - ref_p).max() >= 10 * hr.PRED_AB_BAR


@pytest.mark.parametrize("fault", ["image0", "drop_group"])
@pytest.mark.parametrize("shape", ["A", "B"])
def test_mutants_of_softmax529(shape, fault):
    l = _logits(shape, 529, 5)
    assert _rel(hr.softmax529(l, fault=fault), hr.softmax529(l)) >= 10 * hr.P529_REL_BAR


@pytest.mark.parametrize("fault", ["image0", "swap_planes", "drop_group"])
@pytest.mark.parametrize("shape", ["A", "B"])
def test_mutants_of_the_head(shape, fault):
    H, W, n = hr.SHAPES[shape]
    rs = np.random.RandomState(6)
    x = rs.standard_normal((n, 128, H, W))
    w, b = rs.standard_normal((2, 128)) * 0.6 / np.sqrt(128), rs.uniform(-0.1, 0.1, 2)
    ref = hr.head(x, w, b)
    assert (np.abs(ref) < 99.0).mean() >= 0.5
    assert np.abs(hr.head(x, w, b, fault=fault) - ref).max() >= 10 * hr.HEAD_BAR


@pytest.mark.parametrize("fault", ["image0", "bn_scaled", "skipped", "channel_block"])
@pytest.mark.parametrize("precision", hr.PRECISIONS)
@pytest.mark.parametrize("shape", ["A", "B"])
def test_mutants_of_the_shift(shape, precision, fault):
    H, W, n = hr.SHAPES[shape]
    sd = weights.add_global_branch({}, hr.GLOB_SEED)
    glob, sat = hr.hint_rows()
    glob, sat = glob[:n], sat[:n]
    rs = np.random.RandomState(7)
    v = np.abs(rs.standard_normal((n, 512, H // 8, W // 8))) * 1.5                                 # conv4_3 before the shift
    bn_scale = rs.uniform(0.8, 1.2, 512) / np.sqrt(rs.uniform(0.25, 0.6, 512))
    g = hr.glob_branch(sd, glob, sat)
    g0 = hr.glob_branch(sd, np.zeros((1, 314)))
    ref = hr.shift_difference(sd, glob, sat)
    bad = hr.shift_difference(sd, glob, sat, fault=fault, bn_scale=bn_scale)
    cleared = v + g0[:, :, None, None]
    with_hints = cleared + bad[:, :, None, None]
    bar = hr.shift_bar(with_hints, cleared, precision, hr.SHIFT_REL_BAR * (1.0 + np.abs(g).max()))
    err = np.abs(bad - ref)[:, :, None, None]
    assert (err / bar).max() >= 10.0
