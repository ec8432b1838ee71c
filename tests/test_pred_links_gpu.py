"""Each launch of the distribution heads' conv branch against float64, from the device's OWN stored inputs of the same forward: the 313
head's hyper-column chain conv3_pred .. conv345678_pred, pred_313, and class_logits of the 529-bin head (tests/pred_links_ref.py has the
graph and the restatement).  This is the method of tests/test_heads_gpu.py one layer earlier: that file starts from the stored pred_313 /
class_logits, this one ends there.  A link's inputs -- its source tensor and the previous partial sum -- are read back with activation(),
the link is restated in float64 with bf16-rounded weights and the fp32 bias, and the result is compared with what the launch stored.  Seven
of the eight links store fp32, so what is measured is ONE launch's fp32 accumulation error, whatever the trunk before it did at bf16
precision; conv345678_pred stores bf16 and gets one bf16 ulp of the expected value on top.  What the end-to-end checks of this branch
(0.04 (1 + max|ref|) on the logits, tests/test_caffe_branches_gpu.py) cannot see shows here: a shortcut sum read from the wrong link, a
missing bias or ReLU, one product lost at a tile corner (tests/test_pred_links_cpu.py holds these four mutants against the bar's cap).

Two bf16 handles at 40 x 72 with dist and dist313, three different images: max_batch 3 plans the batch-1 families (conv_kwave_bf16,
conv_kwave_deconv_bf16, conv_click + split-K, conv_igemm + split-K), max_batch 32 the small tile on the deconvs and pred_313 and
conv_igemm<bf16,2,2> on class_logits.  The labels are asserted first (pred_links_ref.LABELS).

Bar: max |got - ref| / (1 + max|ref|) <= LINK_REL_BAR = 4 x the largest figure measured on an MI355X over both handles and all links -- two
binades for the summation orders of other ROCm versions, as in tests/test_heads_gpu.py -- and never above 1e-4, 1/400 of the end-to-end
bound.  Every test prints its figure before it asserts.  Measured (max_batch 3 / max_batch 32):
  conv3_pred       1.331e-7 / 1.375e-7  (conv_kwave_bf16 on both)
  conv34_pred      9.382e-8 / 3.321e-7  (conv_kwave_deconv_bf16 / conv_igemm<bf16,2,1>)      <- the largest: LINK_REL_BAR = 1.328e-6
  conv345_pred     7.145e-8 / 2.668e-7
  conv3456_pred    5.980e-8 / 2.204e-7
  conv34567_pred   7.066e-8 / 2.542e-7
  conv345678_pred  nothing beyond the bf16 ulp on either handle (conv_click<bf16,1,4> splitK4 / splitK2); worst |err| / ulp = 0.500: the
                   store rounds to nearest
  pred_313         1.313e-7 / 2.179e-7  (conv_igemm<bf16,2,1> splitK3 / unsplit; 1 + max|ref| = 25.6)
  class_logits     1.201e-7 / 2.967e-7  (conv_igemm<bf16,2,1> splitK2 / conv_igemm<bf16,2,2>; 1 + max|ref| = 20.9)
In absolute terms 3e-7 .. 6.2e-6: fp32 sums of 2048 - 2304 products (384 and 256 on the 1x1 links).  K split over the waves of a workgroup
(the kwave kernels, four to eight partial sums) and split-K err less than one workgroup walking the whole K loop, as pairwise summation does.
Exact: image 0 of the batch equals the same image run alone, bit for bit, on every link and every tensor a link reads.

Wall time of this file on an MI355X: 1.9 s for its 20 tests (pytest's own figure); the slowest is the first of each handle (0.8 s and 0.2 s:
handle, weights, two forwards, the read-backs), every link after that 0.04 s.
"""
import numpy as np
import pytest

import pred_links_ref as pr
from interactive_deep_colorization_amd import engine

pytestmark = pytest.mark.gpu

_STATE = {}
TENSORS = sorted(set(l.name for l in pr.LINKS) | set(l.src for l in pr.LINKS))


def state_dict():
    if "sd" not in _STATE:
        import heads_ref as hr
        from conftest import state_dict_for
        from oracle import weights
        sd = dict(state_dict_for(hr.WEIGHT_SEED, hr.WEIGHT_STYLE))
        weights.add_pred313_head(sd, hr.PRED_SEED)
        _STATE["sd"] = sd
    return _STATE["sd"]


def images():
    from interactive_deep_colorization_amd import workloads
    return workloads.random_batch(pr.N, pr.H, pr.W, seed=17, max_points=4, max_p=2)


def run(max_batch):
    """One forward of the three images and one of image 0 alone on a handle of this max_batch -> (labels, stored tensors of the batch,
    stored tensors of image 0 alone).  Run once per handle; the arrays are shared by the tests and left unchanged."""
    if max_batch not in _STATE:
        L, ab, m = images()
        e = engine.HipColorizer(pr.H, pr.W, max_batch=max_batch, precision="bf16", dist=True, dist313=True)
        try:
            e.load_state_dict(state_dict())
            e.forward_dist313(L, ab, m, 0.0, want_dist=False)
            labels = {r["name"]: (r["kernel"], r["launches"]) for r in e.layer_table()}
            batch = {t: e.activation(t, pr.N) for t in TENSORS}
            e.forward_dist313(L[:1], ab[:1], m[:1], 0.0, want_dist=False)
            alone = {t: e.activation(t, 1) for t in TENSORS}
        finally:
            e.close()
        for d in (batch, alone):
            for a in d.values():
                a.setflags(write=False)
        _STATE[max_batch] = (labels, batch, alone)
    return _STATE[max_batch]


@pytest.mark.parametrize("max_batch", pr.MAX_BATCHES)
def test_labels(max_batch):
    labels, batch, _ = run(max_batch)
    got = {name: labels[name][0] for name in pr.BY_NAME}
    assert got == pr.LABELS[max_batch], "\n".join("%-16s %-32s | %s" % (k, pr.LABELS[max_batch][k], got[k]) for k in got if got[k] != pr.LABELS[max_batch][k])
    assert all(labels[name][1] == 1 for name in pr.BY_NAME)
    for t in TENSORS:                                          # the images differ: a wrong image base shows
        assert np.abs(batch[t][0] - batch[t][1]).max() > 0.1 and np.abs(batch[t][1] - batch[t][2]).max() > 0.1, t


@pytest.mark.parametrize("name", [l.name for l in pr.LINKS])
@pytest.mark.parametrize("max_batch", pr.MAX_BATCHES)
def test_link(max_batch, name):
    labels, batch, _ = run(max_batch)
    sd = state_dict()
    l = pr.BY_NAME[name]
    x = batch[l.src]
    prev = batch[l.prev] if l.prev else None
    got = batch[name].astype(np.float64)
    ref = pr.link(l, x, sd[l.wkey + ".weight"], sd[l.wkey + ".bias"], prev)
    assert got.shape == ref.shape == (pr.N, pr.COUT.get(name, 384), pr.H // 4, pr.W // 4)
    err = np.abs(got - ref)
    bar = pr.bar(l, ref)
    print("link %-16s max_batch %2d [%s]: max err %.3e, rel %.3e of 1 + max|ref| = %.2f; worst err / bar %.3f%s" %
          (name, max_batch, labels[name][0], err.max(), pr.rel_error(l, got, ref), 1 + np.abs(ref).max(), (err / bar).max(),
           "" if l.out_f32 else " (bf16 store: one ulp of the expected value allowed besides; %.0f %% zeros of the ReLU)" % (100 * (ref == 0).mean())))
    assert pr.LINK_REL_BAR <= pr.MUTANT_BAR
    assert np.abs(ref).max() > 1.0 and (l.relu or (ref < 0).any())
    if prev is not None:      # the partial sum matters: a link that dropped it, or read another, is far outside the bar
        assert np.abs(prev).max() > 0.5
    assert (err <= bar).all(), "worst err / bar %.3f at %s" % ((err / bar).max(), np.unravel_index(np.argmax(err / bar), err.shape))


@pytest.mark.parametrize("max_batch", pr.MAX_BATCHES)
def test_image0_of_the_batch_equals_the_image_alone(max_batch):
    _, batch, alone = run(max_batch)
    for t in TENSORS:
        assert alone[t].shape == batch[t][:1].shape
        np.testing.assert_array_equal(alone[t][0], batch[t][0], err_msg=t)
