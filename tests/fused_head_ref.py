"""float64 numpy restatement of the head fused into conv10_2's epilogue ('+head' labels: conv10_2 = model10.1, 3x3 128 -> 128, LeakyReLU(0.2);
model_out 1x1 128 -> 2; tanh; x out_mul -- models/pytorch/model.py:101-109,175), for tests/test_fused_head_cpu.py and
tests/test_fused_head_gpu.py.  The method of tests/heads_ref.py one layer earlier: conv10_2 is never stored under the fused head, its INPUT
conv10_1 is, so the reference starts from the device's own stored conv10_1 of the same forward.

Weights.  model10.1.weight is replaced by bf16_rne of itself with entries below 2^-12 in magnitude set to 0: exact in bf16, in fp16 (normal
numbers, 8 significant bits) and in every part of a split precision (the lower parts are zero; fp16x3's power-of-two pre-scale keeps that).
The stored conv10_1 is exact in its own storage, so every MFMA product is exact and the kernel's only error is the fp32 accumulation order,
the fp32 LeakyReLU, the fp32 128 -> 2 dot product and tanhf.  model_out keeps its fp32 weights: the kernel reads them as fp32.

The keyword ``fault`` produces the deliberately wrong variants of test_fused_head_cpu.py; no other caller passes it.
A helper, not a conftest: nothing here touches the library or a GPU."""
import collections

import numpy as np

import exact_lattice as xl
import heads_ref as hr

SHAPES = hr.SHAPES                        # A = 40 x 72, n = 3; B = 16 x 24, n = 2 -- at FULL resolution here: B is smaller than one 32-wide tile
WEIGHT_SEED, WEIGHT_STYLE = hr.WEIGHT_SEED, hr.WEIGHT_STYLE
W_FLOOR = 2.0 ** -12
LIVE_RANGE, LIVE_SHARE = 2.0, 0.9         # at least 90 % of the pre-tanh sums inside +-2: the tanh cannot hide a wrong sum

# ---- the bar of tests/test_fused_head_gpu.py: absolute on the +-110 scale, the maximum over all rows.  heads_ref's convention: 4 x the largest
# error measured on an MI355X against this float64 reference (two binades for other ROCm versions' tanhf and summation orders); the cap the
# stand-alone head got is 1e-3.  Measured per row: the docstring of tests/test_fused_head_gpu.py.
FUSED_HEAD_MEASURED = 4.845e-5            # A_fp16_v2sh; every row lies in 2.17e-5 .. 4.85e-5
FUSED_HEAD_CAP = 1e-3
FUSED_HEAD_BAR = 4 * FUSED_HEAD_MEASURED  # 1.938e-4

# One row of tests/test_fused_head_gpu.py: the handle (shape, precision, max_batch), the tile policy and idc_set_option pairs of the forward,
# and the label conv10_2 must show.
Row = collections.namedtuple("Row", "id shape precision max_batch tile opts label")


def _row(id, shape, precision, max_batch, label, tile="auto", opts=()):
    return Row(id, shape, precision, max_batch, tile, tuple(opts), label)


# bf16 / fp16: the large tile needs 128 workgroups (max_batch 32 at A: 3 x 5 tiles of 32 x 8 x 32 images); B is one tile per image, so the bf16
# forward keeps the batch-1 kernels there unless the tile policy says "large" (fp16 is the split machinery: the large tile everywhere).
# Split precisions: the large tile whatever the grid, max_batch = heads_ref.MAX_BATCH.
ROWS = [
    _row("A_bf16_v2p", "A", "bf16", 32, "conv_igemm_v2<2,2>+m16p+head", opts=(("v2p", 1),)),
    _row("A_bf16_v2m", "A", "bf16", 32, "conv_igemm_v2<2,2>+m16+head", opts=(("v2p", 0),)),
    _row("B_bf16_v2m_24", "B", "bf16", 32, "conv_igemm_v2<2,4>+m16+head", tile="large", opts=(("v2p", 1),)),
    _row("A_fp16_v2ph", "A", "fp16", 32, "conv_igemm_v2ph<2,2>+head", opts=(("v2p", 1),)),
    _row("A_fp16_v2sh", "A", "fp16", 32, "conv_igemm_v2sh<2,2>x1+head", opts=(("v2p", 0),)),
    _row("B_fp16_v2ph", "B", "fp16", 32, "conv_igemm_v2ph<2,2>+head", opts=(("v2p", 1),)),
    _row("B_fp16_v2sh", "B", "fp16", 32, "conv_igemm_v2sh<2,2>x1+head", opts=(("v2p", 0),)),
]
for _p, _ps, _s in (("bf16x3", "conv_igemm_v2ps<2,2>x3", "conv_igemm_v2s<2,2>x3"), ("bf16x6", "conv_igemm_v2ps<2,2>x6", "conv_igemm_v2s<2,2>x6"),
                    ("fp16x3", "conv_igemm_v2psh<2,2>x3", "conv_igemm_v2sh<2,2>x3")):
    for _shape in ("A", "B"):
        ROWS.append(_row("%s_%s_v2ps" % (_shape, _p), _shape, _p, hr.MAX_BATCH, _ps + "+head", opts=(("v2p", 1),)))
        ROWS.append(_row("%s_%s_v2s" % (_shape, _p), _shape, _p, hr.MAX_BATCH, _s + "+head", opts=(("v2p", 0),)))
assert len(set(r.id for r in ROWS)) == len(ROWS)
BY_ID = {r.id: r for r in ROWS}


def quantise_weights(w):
    """bf16_rne(w) with entries below 2^-12 in magnitude set to 0."""
    q = xl.bf16_rne(np.asarray(w, np.float32))
    q = np.where(np.abs(q) < W_FLOOR, np.float32(0), q).astype(np.float32)
    assert np.array_equal(xl.bf16_rne(q), q) and np.array_equal(q.astype(np.float16).astype(np.float32), q)
    return q


def state_dict(base):
    """`base` (a whole seeded state dict, left unchanged) with model10.1.weight quantised as above."""
    sd = dict(base)
    sd["model10.1.weight"] = quantise_weights(base["model10.1.weight"])
    return sd


def _conv3x3(xp, w):
    """xp (n, cin, h + 2, w + 2), already padded; w (cout, cin, 3, 3) -> (n, cout, h, w), float64."""
    n, _, hp, wp = xp.shape
    h, ww = hp - 2, wp - 2
    out = np.zeros((n, w.shape[0], h, ww), np.float64)
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("oc,nchw->nohw", w[:, :, ky, kx], xp[:, :, ky:ky + h, kx:kx + ww], optimize=True)
    return out


def fused_head(x, w, b, wo, bo, out_mul=110.0, fault=None, site=None):
    """conv10_1 (n,128,H,W) as activation() returns it -> (out (n,2,H,W) = out_mul * tanh(model_out(LeakyReLU(conv3x3(x) + b))), the
    pre-tanh sums); w (128,128,3,3), b (128,), wo (2,128) or (2,128,1,1), bo (2,).  site (image, y, x) for the fault that strikes one pixel."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    wo = np.asarray(wo, np.float64).reshape(2, 128)
    bo = np.asarray(bo, np.float64)
    pad = ((0, 0), (0, 0), (1, 1), (1, 1))
    xp = np.pad(x, pad, mode="edge") if fault == "edge_replication" else np.pad(x, pad)
    y = _conv3x3(xp, w) + np.asarray(b, np.float64)[None, :, None, None]
    if fault == "drop_product":             # ONE product (one cout, one cin, one tap) missing at one pixel
        n0, y0, x0 = site
        terms = w[:, :, 1, 1] * x[n0, :, y0, x0][None, :]                  # the centre tap's products (cout, cin) at that pixel
        live = np.argwhere(terms != 0)
        order = np.argsort(np.abs(terms[terms != 0]), kind="stable")
        co, ci = (int(i) for i in live[order[len(order) // 2]])           # a typical one: the median magnitude of those that are not zero
        y[n0, co, y0, x0] -= terms[co, ci]
    y = np.where(y < 0, (0.0 if fault == "plain_relu" else 0.2) * y, y)
    if fault == "bf16_conv10_2":            # conv10_2 rounded to bf16 before the head, as the stand-alone head of the bf16 forward reads it
        y = xl.bf16_rne(y.astype(np.float32)).astype(np.float64)
    pre = np.einsum("nkyx,ck->ncyx", y, wo, optimize=True)
    if fault != "no_head_bias":
        pre = pre + bo.reshape(1, 2, 1, 1)
    out = out_mul * np.tanh(pre)
    if fault == "swap_channels":
        out = out[:, ::-1].copy()
    return out, pre
