"""CPU side of tests/test_pred_links_gpu.py: the float64 restatement of each link (tests/pred_links_ref.py) on seeded stand-in inputs, held
against a plain loop at a few pixels, and four deliberately wrong variants of it that the GPU file's bar must not let through -- each moves a
link by more than MUTANT_BAR (1 + max|ref|), the cap the recorded bar may never exceed.  Nothing here touches the library."""
import numpy as np
import pytest

import pred_links_ref as pr
from exact_lattice import bf16_rne

_CACHE = {}


def _case(name):
    """Stand-in inputs and the reference of a link, computed once and left unchanged."""
    if name not in _CACHE:
        l = pr.BY_NAME[name]
        x, w, b, prev = pr.standin_inputs(l)
        ref = pr.link(l, x, w, b, prev)
        for a in (x, w, b, prev, ref):
            if a is not None:
                a.setflags(write=False)
        _CACHE[name] = (l, x, w, b, prev, ref)
    return _CACHE[name]


def _exceeds(l, mutant, ref):
    """Does the mutant leave the bar of the GPU file at its cap?  (On the bf16-stored link: after the storage rounding, the bf16 ulp allowed.)"""
    return bool((np.abs(pr.stored(l, mutant) - ref) > pr.bar(l, ref, pr.MUTANT_BAR)).any())


def test_the_bar_is_under_its_cap_and_the_table_is_the_network():
    assert 0 < pr.LINK_REL_BAR <= pr.MUTANT_BAR == 1e-4
    assert [l.name for l in pr.LINKS] == ["conv3_pred", "conv34_pred", "conv345_pred", "conv3456_pred", "conv34567_pred", "conv345678_pred",
                                          "pred_313", "class_logits"]
    for a, b in zip(pr.LINKS[1:6], pr.LINKS[:5]):
        assert a.prev == b.name                               # the chain: every partial sum feeds the next launch
    assert [l.name for l in pr.LINKS if l.relu] == ["conv345678_pred"] == [l.name for l in pr.LINKS if not l.out_f32]
    assert pr.BY_NAME["pred_313"].src == "conv345678_pred" and pr.BY_NAME["class_logits"].src == "conv8_3"
    for mb in pr.MAX_BATCHES:
        assert set(pr.LABELS[mb]) == set(pr.BY_NAME)


@pytest.mark.parametrize("name", [l.name for l in pr.LINKS])
def test_restatement_equals_a_plain_loop(name):
    """A few output values of each link summed term by term from the definition (corner, border, interior; another image)."""
    l, x, w, b, prev, ref = _case(name)
    wq = bf16_rne(w).astype(np.float64)
    xd = x.astype(np.float64)
    n_, _, hi, wi = x.shape
    assert ref.shape == (pr.N, pr.COUT.get(name, 384), pr.H // 4, pr.W // 4)
    for (n, co, oy, ox) in ((0, 0, 0, 0), (1, 7, 0, 5), (2, ref.shape[1] - 1, ref.shape[2] - 1, ref.shape[3] - 1), (1, 100, 4, 9)):
        s = float(b[co])
        if l.kind == "conv3x3":
            for ky in range(3):
                for kx in range(3):
                    iy, ix = oy + ky - 1, ox + kx - 1
                    if 0 <= iy < hi and 0 <= ix < wi:
                        s += float((xd[n, :, iy, ix] * wq[co, :, ky, kx]).sum())
        elif l.kind == "deconv":
            for ky in range(4):
                for kx in range(4):
                    ty, tx = oy + 1 - ky, ox + 1 - kx          # oy = 2 iy - 1 + ky
                    if ty % 2 == 0 and tx % 2 == 0 and 0 <= ty // 2 < hi and 0 <= tx // 2 < wi:
                        s += float((xd[n, :, ty // 2, tx // 2] * wq[:, co, ky, kx]).sum())
        else:
            s += float((xd[n, :, oy, ox] * wq[co, :, 0, 0]).sum())
        if prev is not None:
            s += float(prev[n, co, oy, ox])
        if l.relu:
            s = max(s, 0.0)
        assert abs(s - ref[n, co, oy, ox]) <= 1e-12 * (1 + abs(s)), (name, n, co, oy, ox)
    assert not _exceeds(l, ref, ref)
    # the reference rounded as the link stores it stays inside the recorded bar: fp32's own rounding is 6e-8 of a value
    got = ref.astype(np.float32).astype(np.float64) if l.out_f32 else pr.stored(l, ref)
    assert (np.abs(got - ref) <= pr.bar(l, ref)).all()


@pytest.mark.parametrize("name", [l.name for l in pr.LINKS])
def test_missing_bias_is_seen(name):
    l, x, w, b, prev, ref = _case(name)
    mutant = pr.link(l, x, w, b, prev, fault="no_bias")
    assert np.abs(mutant - ref).max() > pr.MUTANT_BAR * (1 + np.abs(ref).max())
    assert _exceeds(l, mutant, ref)


@pytest.mark.parametrize("name", [l.name for l in pr.LINKS])
def test_a_product_dropped_on_the_border_row_is_seen(name):
    l, x, w, b, prev, ref = _case(name)
    prod = pr.dropped_product(l, x, w)
    mutant = pr.link(l, x, w, b, prev, fault="drop_product")
    diff = np.abs(mutant - ref)
    assert prod != 0 and int((diff > 0).sum()) == 1 and diff[1, 7, 0, 5] == diff.max()
    assert abs(diff.max() - abs(prod)) <= 1e-12
    assert diff.max() > pr.MUTANT_BAR * (1 + np.abs(ref).max()), "%s: product %.3e against %.3e" % (name, prod, pr.MUTANT_BAR * (1 + np.abs(ref).max()))
    if l.out_f32:             # (the bf16-stored link hides what is below its storage ulp: the fp32-stored links are where one product shows)
        assert _exceeds(l, mutant, ref)


@pytest.mark.parametrize("name", [l.name for l in pr.LINKS if l.prev is not None])
def test_shortcut_from_two_links_back_is_seen(name):
    """The launch reads the partial sum before the previous one (conv34_pred: there is none before conv3_pred, it reads nothing)."""
    l, x, w, b, prev, ref = _case(name)
    two_back = pr.BY_NAME[l.prev].prev
    older = np.zeros_like(prev) if two_back is None else pr.standin_inputs(pr.BY_NAME[l.prev])[3]      # (what the previous link read)
    assert older.shape == prev.shape and np.abs(older - prev).max() > 1.0
    mutant = pr.link(l, x, w, b, older)
    assert np.abs(mutant - ref).max() > pr.MUTANT_BAR * (1 + np.abs(ref).max())
    assert _exceeds(l, mutant, ref)


def test_missing_relu_of_the_last_link_is_seen():
    l, x, w, b, prev, ref = _case("conv345678_pred")
    mutant = pr.link(l, x, w, b, prev, fault="no_relu")
    assert (ref >= 0).all() and (mutant < -1.0).any() and float((ref == 0).mean()) > 0.1
    assert np.abs(mutant - ref).max() > pr.MUTANT_BAR * (1 + np.abs(ref).max())
    assert _exceeds(l, mutant, ref)
    for name in (n.name for n in pr.LINKS if not n.relu):     # ... and no other link has one: the partial sums keep their sign
        assert (_case(name)[5] < 0).any()
