"""Census of the small and lopsided nets, from the planner alone (tests/small_nets.py declares the grid): every configuration of
small_nets.GRID is planned with tools/plan_dump, and every conv label a plan launches must be reached by a row of an exact table --
test_ops_exact_gpu.CASES, model1_ref.ROWS or fused_head_ref.ROWS -- on its family with its template arguments.  Taken without the rows this
census asked for (small_nets.NEW_ROW_IDS), it reports exactly the kernels no test had reached: the census can fail."""
import pytest

import small_nets as sn
from test_ops_exact_gpu import CASES
from test_plan_cpu import plan_dump  # noqa: F401  (the module-scoped fixture that compiles tools/plan_dump.cpp: same skip, same assertion on the built library)


@pytest.fixture(scope="module")
def plans(plan_dump):      # noqa: F811
    return [(cfg, sn.plan_rows(plan_dump, cfg)) for cfg in sn.GRID]


def test_the_grid_holds_what_it_must():
    g = sn.GRID
    assert 150 <= len(g) <= 250, len(g)                                   # about 200 plan_dump runs
    assert {(c.H, c.W) for c in g} == set(sn.NETS) | {sn.WIDE_NET} and set(sn.NETS) >= {(8, 8), (8, 16), (16, 8), (24, 24), (8, 136), (136, 8)}
    assert {c.precision for c in g} == set(sn.PRECISIONS) and len(sn.PRECISIONS) == 6
    assert {c.max_batch for c in g} == {1, 32}
    assert {c.flags for c in g} == {(), ("dist",), ("dist313",)}
    assert {c.options for c in g} == {(), (("winograd", 0),), (("kwave", 0),)}
    for H, W in sn.NETS:                                                  # every net under every precision, batch, flag and option set
        here = [c for c in g if (c.H, c.W) == (H, W)]
        assert {(c.precision, c.max_batch) for c in here} == {(p, mb) for p in sn.PRECISIONS for mb in (1, 32)}
        assert {c.flags for c in here} == {(), ("dist",), ("dist313",)} and {c.options for c in here} == {(), (("winograd", 0),), (("kwave", 0),)}
    assert all(H % 8 == 0 and W % 8 == 0 for H, W in sn.NETS + (sn.WIDE_NET,))


def test_every_small_net_kernel_is_reached_by_an_exact_row(plans):
    assert len(plans) == len(sn.GRID) and all(sum(1 for _ in sn.conv_rows(rows)) >= 20 for _, rows in plans)
    missing = sn.census(plans, sn.covered())
    assert not missing, "conv labels no exact row reaches: " + "; ".join(
        "%s (planned by %s for %s)" % (label, where, layer) for label, (where, layer) in missing.items())


def test_without_the_new_rows_the_census_reports_what_was_unreached(plans):
    """The helper itself: with the rows of NEW_ROW_IDS out of the covered set the census names exactly the labels that had no test, each with
    a configuration and a layer that plans it."""
    ids = set(c.id for c in CASES)
    assert set(sn.NEW_ROW_IDS) <= ids, set(sn.NEW_ROW_IDS) - ids
    missing = sn.census(plans, sn.covered(without=sn.NEW_ROW_IDS))
    assert set(missing) == sn.UNREACHED_BEFORE, sorted(set(missing) ^ sn.UNREACHED_BEFORE)
    by_cfg = {sn.describe(cfg): rows for cfg, rows in plans}
    for label, (where, layer) in missing.items():
        assert any(r["name"] == layer and sn.family(r["kernel"]) == label for r in by_cfg[where]), (label, where, layer)
    # the new rows are what closes it: every unreached family is the family of one of them
    assert sn.UNREACHED_BEFORE == set(sn.family(c.label) for c in CASES if c.id in sn.NEW_ROW_IDS)


def test_the_one_wave_click_form_is_on_a_default_path(plans):
    """conv345678_pred of a dist313 handle on any net 8 pixels tall plans as conv_click<T,1,1> under the default options."""
    for cfg, rows in plans:
        if cfg.flags == ("dist313",) and cfg.H == 8 and cfg.max_batch == 1 and cfg.precision in ("fp32", "bf16"):
            k = [r["kernel"] for r in rows if r["name"] == "conv345678_pred"][0]
            t = "f32" if cfg.precision == "fp32" else "bf16"
            assert cfg.options == () and sn.family(k) == "conv_click<%s,1,1>" % t, (sn.describe(cfg), k)


def test_family_and_the_list_of_what_is_no_conv():
    assert sn.family("conv_click<f32,1,1> splitK16") == "conv_click<f32,1,1>"
    assert sn.family("conv_ds_fused_m+shortcut 8-wave") == sn.family("conv_ds_fused_m+shortcut half") == "conv_ds_fused_m+shortcut"
    assert sn.family("conv_igemm_v2ps<1,4>x3") != sn.family("conv_igemm_v2ps<1,4>x6") != sn.family("conv_igemm_v2ps<2,2>x6")
    rows = [dict(name="glob_branch", kernel="(input pack fused into conv1_1)", launches=0), dict(name="head", kernel="head_kernel", launches=1),
            dict(name="dist_softmax", kernel="softmax_nchw_kernel", launches=0), dict(name="conv1_2", kernel="fused into conv1_1", launches=0),
            dict(name="conv5_1", kernel="conv_click<bf16,1,1> splitK8", launches=1), dict(name="conv10_2", kernel="conv_igemm_v2<2,2>+m16p+head", launches=1)]
    assert [r["name"] for r in sn.conv_rows(rows)] == ["conv5_1", "conv10_2"]
    cfg = sn.Config("bf16", (), 8, 8, 1, (("kwave", 0),))
    assert sn.census([(cfg, rows)], {"conv_igemm_v2<2,2>+m16p"}) == {"conv_click<bf16,1,1>": ("8 x 8 bf16 max_batch 1 kwave=0", "conv5_1"),
                                                                       "conv_igemm_v2<2,2>+m16p+head": ("8 x 8 bf16 max_batch 1 kwave=0", "conv10_2")}
    with pytest.raises(AssertionError):                                   # a row of a new kind must be put on one of the two lists
        list(sn.conv_rows([dict(name="x", kernel="chained into conv4_2", launches=0)]))
