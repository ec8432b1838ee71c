"""CPU checks of the pipelined uint8 batches (idc_forward_async_rgb / HipColorizer.forward_async_rgb / colorize_stream): the symbol is
declared, bound and exported, hint lists are flattened to the offsets the C call reads, and colorize_stream drives the two slots in the
right order -- with a stub engine that records the calls, so that no device is needed."""
import numpy as np
import pytest

from interactive_deep_colorization_amd import _native as N
from interactive_deep_colorization_amd import engine


def test_the_symbol_is_bound_and_exported():
    assert "idc_forward_async_rgb" in N.EXPORTED_SYMBOLS
    lib = N.load()
    assert hasattr(lib, "idc_forward_async_rgb")
    assert len(lib.idc_forward_async_rgb.argtypes) == 15
    assert N.IDC_BATCH_OUT_SOURCE == 1 and N.IDC_BATCH_MAX_SOURCE_BYTES == 1 << 30 and N.IDC_BATCH_MAX_HINTS == 1 << 20


def test_hint_lists_are_flattened_to_offsets():
    assert engine.flatten_hints(None, 3) == (None, None)
    a = [(1, 2, 3, 4, 5.0, 6.0), (7, 8, 9, 10, 11.0, 12.0, 13.0)]
    b = [(20, 21, 22, 23, -1.5, 2.5)]
    offsets, arr = engine.flatten_hints([a, [], None, b], 4)
    assert offsets.dtype == np.int32 and offsets.tolist() == [0, 2, 2, 2, 3]
    rows = [(h.y0, h.x0, h.y1, h.x1, h.c0, h.c1, h.c2) for h in arr]
    assert rows == [(1, 2, 3, 4, 5.0, 6.0, 0.0), (7, 8, 9, 10, 11.0, 12.0, 13.0), (20, 21, 22, 23, -1.5, 2.5, 0.0)]
    offsets, arr = engine.flatten_hints([[], None], 2)                         # all empty: explicit zero offsets, a non-empty dummy array
    assert offsets.tolist() == [0, 0, 0] and len(arr) == 1
    offsets, arr = engine.flatten_hints(iter([b, a]), 2)                        # any iterable of lists
    assert offsets.tolist() == [0, 1, 3] and arr[0].y0 == 20 and arr[2].c2 == 13.0
    with pytest.raises(ValueError):
        engine.flatten_hints([a], 2)


class _Pool(object):
    def take(self, shape, dtype):
        return np.empty(shape, dtype)


class _StubEngine(engine.HipColorizer):
    """colorize_stream over recorded calls: 'the device' writes batch[0,0,0,0] + 1 into the whole result when the slot is waited for."""

    def __init__(self, H, W):
        self.H, self.W = H, W
        self._pool = _Pool()
        self.calls = []
        self.busy = {}

    def close(self):
        pass

    def forward_async_rgb(self, slot, rgb, hints, out_rgb, out_ab=None, **kw):
        assert slot not in self.busy, "slot %d reused before its wait" % slot
        self.calls.append(("run", slot, tuple(rgb.shape), hints, tuple(out_rgb.shape), dict(kw)))
        self.busy[slot] = (int(rgb[0, 0, 0, 0]) + 1, out_rgb)

    def wait(self, slot):
        self.calls.append(("wait", slot))
        if slot in self.busy:
            v, dst = self.busy.pop(slot)
            dst[...] = v


@pytest.mark.parametrize("count", [1, 2, 5])
@pytest.mark.parametrize("out", ["net", "source"])
def test_colorize_stream_alternates_slots_and_keeps_the_order(count, out):
    e = _StubEngine(8, 16)
    sizes = [(2, 5, 7), (3, 9, 4), (1, 8, 16), (4, 3, 3), (2, 6, 6)][:count]
    items = []
    for k, (n, h, w) in enumerate(sizes):
        items.append((np.full((n, h, w, 3), 10 * k, np.uint8), None if k % 2 else [[(0, 0, 1, 1, 1.0, 2.0)]] * n))
    seen = []
    for k, res in enumerate(e.colorize_stream(iter(items), out=out, mode="ab", mask_value=110.0)):
        n, h, w = sizes[k]
        assert res.shape == ((n, h, w, 3) if out == "source" else (n, 8, 16, 3)) and res.dtype == np.uint8
        assert (res == 10 * k + 1).all(), "result %d is not batch %d's" % (k, k)
        seen.append(res)
    assert len(seen) == count and not e.busy
    runs = [c for c in e.calls if c[0] == "run"]
    assert [c[1] for c in runs] == [k & 1 for k in range(count)]                # slot alternation
    for k, c in enumerate(runs):
        assert c[2] == items[k][0].shape and c[3] is items[k][1] and c[5] == {"out": out, "mode": "ab", "mask_value": 110.0}
    # a wait before each reuse of a slot (the stub asserts it too), and exactly one wait per batch
    assert [c[1] for c in e.calls if c[0] == "wait"] == [k & 1 for k in range(count)]
    for k in range(2, count):
        i_run = e.calls.index(runs[k])
        assert ("wait", k & 1) in e.calls[e.calls.index(runs[k - 2]) + 1:i_run]
    for a, b in zip(seen, seen[1:]):                                            # results are the caller's own arrays
        assert not np.shares_memory(a, b)


def test_colorize_stream_waits_for_what_is_in_flight_when_the_consumer_stops():
    e = _StubEngine(8, 8)
    gen = e.colorize_stream((np.zeros((1, 4, 4, 3), np.uint8), None) for _ in range(4))
    next(gen)
    assert e.busy
    gen.close()
    assert not e.busy


def test_forward_async_rgb_refuses_malformed_arrays_before_the_library_sees_them():
    e = _StubEngine(8, 8)
    call = engine.HipColorizer.forward_async_rgb
    good = np.zeros((2, 5, 6, 3), np.uint8)
    with pytest.raises(ValueError):
        call(e, 0, good.astype(np.float32), None, np.zeros((2, 8, 8, 3), np.uint8))
    with pytest.raises(ValueError):
        call(e, 0, good[:, :, ::2], None, np.zeros((2, 8, 8, 3), np.uint8))                # not contiguous
    with pytest.raises(ValueError):
        call(e, 0, good, None, np.zeros((2, 5, 6, 3), np.uint8))                            # out='net' wants (n,H,W,3)
    with pytest.raises(ValueError):
        call(e, 0, good, None, np.zeros((2, 8, 8, 3), np.uint8), out="source")              # out='source' wants the source's shape
    with pytest.raises(ValueError):
        call(e, 0, good, None, np.zeros((2, 8, 8, 3), np.uint8), out_ab=np.zeros((2, 2, 8, 8), np.float64))
