"""Batches whose activation tensors pass 2^31 and 2^32 bytes inside one handle.

Property: offset independence.  Image k of a batch that fills the handle equals, bit for bit, the same image sent alone (n = 1: offset 0 of every
tensor) through the SAME handle -- the same kernels, since the variant follows max_batch.  test_net_gpu.py::test_batching_is_exactly_per_image
holds that at 5 x 64 x 64; here it is held for the images around every 2^31- and 2^32-byte mark of every tensor size class, for image 0 and for the
last one.  An index narrowed to 32 bits would read or write image k - D (D = the images one mark spans): out[k] != out[k - D] is asserted too, so
the comparison cannot pass by aliasing.  The big handle's layer table names the kernels of a max_batch = 32, 256 x 256 handle of its precision:
the shipped throughput families ran.

Bytes per image and tensor follow build_layers (tests/large_ref.py: H/level * W/level * Cpad * bytes * parts).  Marks, as image indices:

  bf16, 256 x 256, max_batch 264 (4.125 GiB in each of conv10_1, conv10_2, conv1_2_short)
      16 MiB per image   conv10_1 conv10_2 conv1_2_short      2^31 at image 128, 2^32 at image 256        D = 128, 256
       8 MiB             conv1_1 conv1_2                      2^31 at image 256                           D = 256
       4 MiB and less    every other tensor                   below 2^31 (1.03 GiB at most)
      images compared: 0 127 128 129 255 256 257 263 -- by forward, forward_rgb (lab_post_kernel over all 264: RGB and refreshed Lab of the image
      alone) and forward_async on slot 0 (slot-owned planes, copy-out list)
  fp16x3 and fp32, 64 x 64, max_batch 2057 = the smallest batch that puts the largest tensor past 2^32 bytes (2049), plus 8.  (fp16x3 stores TWO
  fp16 planes per tensor, not three: 128 channels x 2 B x 2 planes = fp32's 512 bytes per pixel, so both precisions get there at the same batch,
  137 at 256 x 256.)  The arena of 256 x 256 x 137 within 7 %, with the float64 oracle affordable: 2 s for the eight images, computed once.
       2 MiB per image   conv10_1 conv10_2 conv1_2_short (fp16x3: the shortcut branch is stored in fp32)
                                                              2^31 at image 1024, 2^32 at image 2048      D = 1024, 2048
       1 MiB             conv1_1 conv1_2                      2^31 at image 2048                          D = 2048
       512 KiB and less  every other tensor                   below 2^31 (1.004 GiB at most)
      images compared: 0 1023 1024 1025 2047 2048 2049 2056, and against oracle.siggraph_torch in float64 at tests/bounds.py's FP32_TOL (he-style
      weights: 3e-3, the bound test_parity_record_gpu.py holds fp16x3 and fp32 to)
      Both plans name the kernels of the max_batch = 32, 256 x 256 handle, so 64 x 64 is the only size: no 256 x 256 twin is needed.
  2^31 fp32 ELEMENTS (8 GiB in one tensor) is not reached: at 2 MiB per image that is max_batch 4097, an arena twice this one (55 GiB of
  tensors), for an index the kernels never form -- they address bytes from a 64-bit per-image base, and bytes pass 2^31 and 2^32 here.

Before a handle is created the device's free memory is compared with 1.25 x its computed size (tests/large_ref.py: the arena alloc_graph makes plus
the handle's planes); the case is skipped, with the figures, if it does not fit.  A 288 GB card takes all three, one after another.

Measured on an MI355X (no case skipped; wall time of the whole case, the max_batch = 32 handle and the oracle included):
  case                 arena bytes (GiB)        one forward of the batch   case     worst image against the float64 oracle
  bf16   256^2 x 264   30 452 744 192 (28.36)   0.055 s                    2.2 s    --
  fp16x3 64^2 x 2057   29 693 575 168 (27.65)   0.109 s                    2.7 s    6.5e-4 (bound 3e-3)
  fp32   64^2 x 2057   29 693 575 168 (27.65)   0.271 s                    2.2 s    3.5e-4 (bound 3e-3)
  (a second run, inside the whole suite: 2.0 / 2.8 / 3.2 s)
The inputs take 0.09 s (264 x 256^2) and 0.24 s (2057 x 64^2) to draw: workloads.random_batch as it is.
"""
import time

import numpy as np
import pytest
import torch

import large_ref as lr
from bounds import FP32_TOL
from interactive_deep_colorization_amd import engine, workloads
from oracle import siggraph_torch

pytestmark = pytest.mark.gpu

SEED_WEIGHTS, STYLE = 0, "he"             # full tanh range: images differ everywhere
HEADROOM = 1.25


def _max_batch_past(precision, size, mark=1 << 32, extra=8):
    largest = max(lr.size_classes(precision, size, size))
    return mark // largest + 1 + extra


CASES = [
    dict(id="bf16-256x256x264", precision="bf16", size=256, max_batch=264, seed=40, oracle=False, routes=True,
         images=[0, 127, 128, 129, 255, 256, 257, 263], distances=[128, 256]),
    dict(id="fp16x3-64x64x2057", precision="fp16x3", size=64, max_batch=_max_batch_past("fp16x3", 64), seed=41, oracle=True, routes=False,
         images=[0, 1023, 1024, 1025, 2047, 2048, 2049, 2056], distances=[1024, 2048]),
    dict(id="fp32-64x64x2057", precision="fp32", size=64, max_batch=_max_batch_past("fp32", 64), seed=41, oracle=True, routes=False,
         images=[0, 1023, 1024, 1025, 2047, 2048, 2049, 2056], distances=[1024, 2048]),
]

_INPUTS, _ORACLE, _TABLE32 = {}, {}, {}


def _inputs(c):
    key = (c["max_batch"], c["size"], c["seed"])
    if key not in _INPUTS:
        _INPUTS.clear()                                      # one batch at a time: 280 MB each
        _INPUTS[key] = workloads.random_batch(c["max_batch"], c["size"], seed=c["seed"])
    return _INPUTS[key]


def _oracle(c, sd, idx):
    """float64 reference of the compared images: computed once, shared by the cases that draw the same batch, never written to."""
    key = (c["max_batch"], c["size"], c["seed"], tuple(idx))
    if key not in _ORACLE:
        L, ab, m = _inputs(c)
        ref = siggraph_torch.forward(sd, L[idx], ab[idx], m[idx], 0.0, dtype=torch.float64)
        ref.setflags(write=False)
        _ORACLE[key] = ref
    return _ORACLE[key]


def _kernels(table):
    return [(r["name"], r["kernel"]) for r in table]


def _table_of_a_batch32_handle(precision, sd):
    if precision not in _TABLE32:
        L, ab, m = workloads.random_batch(1, 256, seed=3)
        e = engine.HipColorizer(256, 256, max_batch=32, precision=precision)
        e.load_state_dict(sd)
        e.forward(L, ab, m, 0.0)
        _TABLE32[precision] = _kernels(e.layer_table())
        e.close()
    return _TABLE32[precision]


def marks_of(c):
    """The images to compare and the aliasing distances, worked out from the tensor sizes: what the case's lists state."""
    marks = lr.boundary_images(c["precision"], c["size"], c["size"], c["max_batch"])
    images = {0, c["max_batch"] - 1}
    for _, _, k, _ in marks:
        images.update(i for i in (k - 1, k, k + 1) if 0 <= i < c["max_batch"])
    return marks, sorted(images), sorted(set(d for _, _, _, d in marks if d))


def _same_image(got, want, k, what):
    assert np.array_equal(got, want), "%s of image %d differs from the image sent alone: %d values, max %.3e" % (
        what, k, int((got != want).sum()), float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()))


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_image_k_of_a_full_handle_equals_the_image_alone(make_sd, c):
    t_start = time.time()
    precision, size, nb = c["precision"], c["size"], c["max_batch"]
    marks, images, distances = marks_of(c)
    assert images == c["images"] and distances == c["distances"], (images, distances)
    assert any(mark == 1 << 32 for _, mark, _, _ in marks) and nb * max(lr.size_classes(precision, size, size)) > 1 << 32
    if precision != "bf16":
        assert nb == 2057

    sd = make_sd(SEED_WEIGHTS, STYLE)
    table32 = _table_of_a_batch32_handle(precision, sd)
    arena = lr.arena_bytes(precision, size, size, nb)
    need = lr.device_bytes(precision, size, size, nb, post=c["routes"], pipeline=c["routes"])
    free, total = torch.cuda.mem_get_info(0)
    if free < HEADROOM * need:
        pytest.skip("%s needs %.2f GiB on the device (arena %.2f GiB) x %.2f headroom; %.2f of %.2f GiB are free" % (
            c["id"], need / 2.0 ** 30, arena / 2.0 ** 30, HEADROOM, free / 2.0 ** 30, total / 2.0 ** 30))

    t0 = time.time()
    L, ab, m = _inputs(c)
    t_inputs = time.time() - t0
    e = engine.HipColorizer(size, size, max_batch=nb, precision=precision)
    try:
        e.load_state_dict(sd)
        t0 = time.time()
        full = e.forward(L, ab, m, 0.0)
        t_forward = time.time() - t0
        assert full.shape == (nb, 2, size, size) and np.isfinite(full).all() and np.abs(full).max() <= 110.0
        assert _kernels(e.layer_table()) == table32, [(a, b) for a, b in zip(_kernels(e.layer_table()), table32) if a != b]

        # an offset narrowed by one mark would land D images short: those images are not what image k holds
        for d in distances:
            for k in images:
                if k >= d:
                    assert not np.array_equal(full[k], full[k - d]) and not np.array_equal(L[k], L[k - d]), (k, d)
        for k in images:
            alone = e.forward(L[k:k + 1], ab[k:k + 1], m[k:k + 1], 0.0)
            _same_image(full[k], alone[0], k, "forward: ab")
        np.testing.assert_array_equal(e.forward(L, ab, m, 0.0), full)             # the n = 1 runs left nothing behind

        if c["oracle"]:
            ref = _oracle(c, sd, images)
            err = np.abs(full[images].astype(np.float64) - ref).max(axis=(1, 2, 3))
            print("%s: max-abs error of images %s against the float64 oracle: %s (bound %.1e)" % (c["id"], images, ["%.2e" % v for v in err], FP32_TOL[STYLE]))
            assert err.max() <= FP32_TOL[STYLE], (images, err)

        if c["routes"]:
            # forward_rgb: the forward plus lab_post_kernel over all images
            out2, rgb, labq = e.forward_rgb(L, ab, m, 0.0)
            np.testing.assert_array_equal(out2, full)
            for d in distances:
                for k in images:
                    if k >= d:
                        assert not np.array_equal(rgb[k], rgb[k - d]), (k, d)
            for k in images:
                o1, r1, q1 = e.forward_rgb(L[k:k + 1], ab[k:k + 1], m[k:k + 1], 0.0)
                _same_image(full[k], o1[0], k, "forward_rgb: ab")
                _same_image(rgb[k], r1[0], k, "forward_rgb: RGB")
                _same_image(labq[k], q1[0], k, "forward_rgb: refreshed Lab")
            del out2, rgb, labq
            # forward_async on one slot: the slot's own planes in, the copy-out list out
            out3 = np.empty((nb, 2, size, size), np.float32)
            e.forward_async(0, L, ab, m, out3, 0.0)
            e.wait(0)
            np.testing.assert_array_equal(out3, full)
            one = np.empty((1, 2, size, size), np.float32)
            for k in images:
                e.forward_async(0, L[k:k + 1], ab[k:k + 1], m[k:k + 1], one, 0.0)
                e.wait(0)
                _same_image(full[k], one[0], k, "forward_async: ab")
    finally:
        e.close()
    print("%s: arena %d bytes (%.2f GiB), device %.2f GiB; inputs %.2f s, full forward %.3f s, case %.2f s" % (
        c["id"], arena, arena / 2.0 ** 30, need / 2.0 ** 30, t_inputs, t_forward, time.time() - t_start))
