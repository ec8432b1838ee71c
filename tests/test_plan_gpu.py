"""A forward's plan is a function of its inputs (precision, flags, shape, max_batch, n, the options), not of what earlier forwards of the
handle were planned as: after forwards at another batch and under other options, a forward plans -- and computes -- what a fresh handle's
first forward does.  64 x 64 at max_batch 2: the operand-split handle fuses its three deconv + shortcut pairs and un-fuses them under
split_ds_fuse = 0; the bf16 handle runs the batch-1 kernels and the trunk chain, whose rows a forward at another batch rewrites."""
import numpy as np
import pytest

from interactive_deep_colorization_amd import engine, workloads

pytestmark = pytest.mark.gpu

_OPTIONS = {"fuse_conv1": 1, "split_ds_fuse": 1}


def _table(e):
    return [(r["name"], r["kernel"], r["launches"]) for r in e.layer_table()]


@pytest.mark.parametrize("precision", ["bf16", "fp16x3"])
def test_plan_is_a_function_of_its_inputs(make_sd, precision):
    sd = make_sd(1, "torch")
    L, ab, m = workloads.random_batch(2, 64, seed=2, max_points=5, max_p=3)
    fresh = engine.HipColorizer(64, 64, max_batch=2, precision=precision)
    used = engine.HipColorizer(64, 64, max_batch=2, precision=precision)
    try:
        fresh.load_state_dict(sd)
        used.load_state_dict(sd)
        want_ab = np.array(fresh.forward(L, ab, m, 0.5))
        want_table = _table(fresh)
        used.forward(L, ab, m, 0.5)
        used.forward(L[:1], ab[:1], m[:1], 0.5)
        try:
            for name in _OPTIONS:
                engine.set_option(name, 0)
            used.forward(L, ab, m, 0.5)
        finally:
            for name, value in _OPTIONS.items():
                engine.set_option(name, value)
        got_ab = np.array(used.forward(L, ab, m, 0.5))
        got_table = _table(used)
        assert got_table == want_table, [(w, g) for w, g in zip(want_table, got_table) if w != g]
        assert np.array_equal(got_ab, want_ab)
    finally:
        fresh.close()
        used.close()
