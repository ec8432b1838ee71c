"""float64 numpy restatements of what follows the conv stack (csrc/idc_heads.hip) and of the Global-Hints shift, for
tests/test_heads_cpu.py and tests/test_heads_gpu.py.  Plain and slow on purpose; nothing here reads a file.

Every function takes the tensor the kernel read (as idc_get_activation returns it, NCHW) and returns what the kernel should have written.
The keyword arguments named ``fault`` produce the deliberately wrong variants of test_heads_cpu.py's mutation checks; no other caller passes them."""
import numpy as np

BN_EPS = 1e-5
T_PRED = 2.6          # the 313 head's decode temperature (deploy_nopred.prototxt scale_T)
S_DEFAULT = 0.2       # ... and the default of the distribution's (scale_S; idc_set_dist_temperature)
T_529 = 0.2           # model.py:160 softmax(model_class(conv8_3) * .2)


# ---- the cases both test files share: shapes, seeds, inputs (numpy only: test_heads_cpu.py must not import the GPU file) ----------------
SHAPES = {"A": (40, 72, 3), "B": (16, 24, 2)}             # H, W, n
MAX_BATCH = 3
PRECISIONS = ("fp32", "bf16", "fp16", "bf16x3", "bf16x6", "fp16x3")
WEIGHT_SEED, WEIGHT_STYLE, GLOB_SEED, PRED_SEED = 0, "he", 3, 2

# ---- the bars of tests/test_heads_gpu.py: 4 x the largest error measured on an MI355X over all cases of the comparison (that file's
# docstring has the figures); test_heads_cpu.py holds the mutants against them
P313_REL_BAR = 4 * 3.711e-6       # 313 probabilities, |p - ref| / (ref + 1e-12)
PRED_AB_BAR = 4 * 2.490e-4        # pred_ab, absolute on the +-110 scale
P529_REL_BAR = 4 * 5.598e-7       # 529 probabilities, relative
HEAD_BAR = 4 * 2.030e-5           # head output, absolute at out_mul = 110 (scaled with out_mul)
SHIFT_REL_BAR = 4 * 1.334e-6      # the shift identity on fp32 storage, absolute / (1 + max|g|)


def images(shape):
    from interactive_deep_colorization_amd import workloads
    H, W, n = SHAPES[shape]
    return workloads.random_batch(n, H, W, seed=17, max_points=4, max_p=2)


def hint_rows():
    """Three hint rows: an unnormalised histogram with a saturation, the all-zero input, a signed 'histogram' with another saturation.
    (The branch is four GEMVs: nothing in it needs a physical histogram, and rows this far apart give shift vectors that differ by tens
    to hundreds of units, test_heads_cpu.py::test_hint_rows_separate_the_images.)"""
    rs = np.random.RandomState(0)
    glob = np.zeros((3, 314), np.float32)
    sat = np.zeros((3, 2), np.float32)
    glob[0, :313] = rs.uniform(0, 1, 313); glob[0, 313] = 1.0; sat[0] = (0.7, 1.0)
    glob[2, :313] = 3.0 * rs.standard_normal(313); glob[2, 313] = 1.0; sat[2] = (-0.4, 1.0)
    return glob, sat


def softmax(x, axis=1):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def _up4_axis(a, axis, clamp=False):
    """The two grouped bilinear x2 deconvs (kernel (.25 .5 .25 0) (x) same, stride 2, pad 1) composed, along one axis:
    out[4m + j] = ((4 - j) a[m] + j a[m + 1]) / 4, with a[M] = 0 beyond the far border."""
    a = np.moveaxis(np.asarray(a, np.float64), axis, -1)
    far = a[..., -1:] if clamp else np.zeros_like(a[..., :1])
    nxt = np.concatenate([a[..., 1:], far], axis=-1)
    out = np.empty(a.shape[:-1] + (a.shape[-1], 4), np.float64)
    for j in range(4):
        out[..., j] = ((4 - j) * a + j * nxt) / 4.0
    return np.moveaxis(out.reshape(a.shape[:-1] + (4 * a.shape[-1],)), -1, axis)


def upsample4(l, fault=None):
    """(n,C,h,w) -> (n,C,4h,4w)."""
    up = _up4_axis(_up4_axis(l, 2, clamp=fault == "clamp"), 3, clamp=fault == "clamp")
    if fault == "swap_jyjx":            # the sub-pixel offsets of a 4 x 4 block exchanged
        n, c, H, W = up.shape
        up = up.reshape(n, c, H // 4, 4, W // 4, 4).transpose(0, 1, 2, 5, 4, 3).reshape(n, c, H, W)
    return up


def dist313(l, S, centres, bias, fault=None):
    """pred_313 logits (n,313,h,w) -> (dist (n,313,4h,4w) = softmax(S up), pred_ab (n,2,4h,4w) = centres . softmax(2.6 up) + bias);
    centres (313,2), bias (2,)."""
    l = np.asarray(l, np.float64)
    if fault == "image0":               # the per-image base ignored
        l = np.broadcast_to(l[:1], l.shape)
    up = upsample4(l, fault)
    dist = softmax(S * up)
    pt = softmax(T_PRED * up)
    if fault == "drop_group":           # lanes' second 64-bin group left out of both sums
        keep = np.ones(up.shape[1], bool); keep[64:128] = False
        e = np.exp(S * (up - up.max(axis=1, keepdims=True))) * keep[None, :, None, None]
        dist = e / e.sum(axis=1, keepdims=True)
        e = np.exp(T_PRED * (up - up.max(axis=1, keepdims=True))) * keep[None, :, None, None]
        pt = e / e.sum(axis=1, keepdims=True)
    pred = np.einsum("nqyx,qc->ncyx", pt, np.asarray(centres, np.float64)) + np.asarray(bias, np.float64).reshape(1, 2, 1, 1)
    return dist, pred


def softmax529(l, fault=None):
    """class_logits (n,529,h,w) -> softmax(0.2 l) over the channels."""
    l = np.asarray(l, np.float64)
    if fault == "image0":
        l = np.broadcast_to(l[:1], l.shape)
    if fault == "drop_group":           # 529 = 8 * 64 + 17: the partial last group left out of the sum
        e = np.exp(T_529 * (l - l.max(axis=1, keepdims=True)))
        return e / e[:, :512].sum(axis=1, keepdims=True)
    return softmax(T_529 * l)


def head(x, w, b, out_mul=110.0, fault=None):
    """conv10_2 (n,128,H,W) -> out_mul * tanh(W x + b); w (2,128) or (2,128,1,1), b (2,)."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64).reshape(2, 128)
    if fault == "drop_group":           # one lane's 8 channels left out of the sum
        w = w.copy(); w[:, 40:48] = 0.0
    out = out_mul * np.tanh(np.einsum("nkyx,ck->ncyx", x, w) + np.asarray(b, np.float64).reshape(1, 2, 1, 1))
    if fault == "swap_planes":          # n*2 + c taken as c*2 + n-ish: the two planes of every image but the first exchanged
        out = out.copy(); out[1:] = out[1:, ::-1]
    if fault == "image0":
        out = np.broadcast_to(out[:1], out.shape).copy()
    return out


def _bn(sd, key):
    s = np.asarray(sd[key + ".weight"], np.float64) / np.sqrt(np.asarray(sd[key + ".running_var"], np.float64) + BN_EPS)
    return s, np.asarray(sd[key + ".bias"], np.float64) - np.asarray(sd[key + ".running_mean"], np.float64) * s


def glob_branch(sd, glob, sat=None):
    """The Global-Hints branch (deploy_nodist.prototxt:37-172): glob (n,314), sat (n,2) or None (zeros) -> (n,512).
    relu(glob_conv1 g + s_conv1 s) -> BN1, then three 1x1 conv -> ReLU -> BN stages."""
    g = np.atleast_2d(np.asarray(glob, np.float64))
    s = np.zeros((g.shape[0], 2)) if sat is None else np.atleast_2d(np.asarray(sat, np.float64))

    def fc(x, key):
        return x @ np.asarray(sd[key + ".weight"], np.float64).reshape(512, -1).T + np.asarray(sd[key + ".bias"], np.float64)
    y = np.maximum(fc(g, "glob.glob_conv1") + fc(s, "glob.s_conv1"), 0.0)
    sc, sh = _bn(sd, "glob.bn1")
    y = y * sc + sh
    for i in (2, 3, 4):
        sc, sh = _bn(sd, "glob.bn%d" % i)
        y = np.maximum(fc(y, "glob.glob_conv%d" % i), 0.0) * sc + sh
    return y


def shift_difference(sd, glob, sat=None, fault=None, bn_scale=None):
    """What conv4_3 with hints minus conv4_3 after clear_global_hints() must be: (n,512) = g(hints[n]) - g(0), the same at every pixel
    (the shift is added after the ReLU and the BN affine).  bn_scale (512,): conv4_3's own folded BN scale, for the fault that applies
    the shift before it."""
    g = glob_branch(sd, glob, sat)
    g0 = glob_branch(sd, np.zeros((1, 314)), np.zeros((1, 2)))
    d = g - g0
    if fault == "image0":
        d = np.broadcast_to(d[:1], d.shape).copy()
    if fault == "bn_scaled":
        d = d * np.asarray(bn_scale, np.float64)[None]
    if fault == "skipped":
        d = np.zeros_like(d)
    if fault == "channel_block":        # the 64-channel block index taken from the neighbouring block
        d = np.roll(d, 64, axis=1)
    return d


# ---- storage: what one unit in the last place of a stored value is --------------------------------------------------------------------
# bits below the leading one of a value in [2^e, 2^(e+1)) that the storage keeps: bf16 7, fp16 10.  A split tensor is hi = rne(v),
# next = rne(v - hi), ... (idc_common.hip.h): a remainder is at most half an ulp of the part above, so each further bf16 part starts
# 8 bits lower (two planes: the low part is below 2^(e-7), its ulp at most 2^(e-15); three: 2^(e-23)) and the fp16 pair's low part
# 11 bits lower (ulp at most 2^(e-21)).
_FRAC_BITS = {"bf16": 7, "fp16": 10, "bf16x3": 15, "bf16x6": 23, "fp16x3": 21, "fp32": 23}
_MIN_ULP = {"fp16": 2.0 ** -24, "fp16x3": 2.0 ** -24}     # fp16's subnormal spacing


def storage_ulp(x, precision):
    """Elementwise: the spacing of the storage format of `precision` around the stored value x."""
    ax = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(ax, 2.0 ** -126)))
    return np.maximum(2.0 ** (e - _FRAC_BITS[precision]), _MIN_ULP.get(precision, 2.0 ** -149))


def shift_bar(with_hints, cleared, precision, fp32_bar):
    """Elementwise bar of the identity with - cleared == g(hints) - g(0): the fp32 bar (two fp32 roundings of the stored values plus the
    branch's own error: SHIFT_REL_BAR (1 + max|g|), measured on fp32 storage) and, on 16-bit storage, one storage ulp of each of the two
    stored values.  The fp32 term is below the storage ulps of every format but the three-plane bf16x6, whose lowest part is fp32's ulp."""
    if precision == "fp32":
        return np.full(np.shape(with_hints), float(fp32_bar))
    return fp32_bar + storage_ulp(with_hints, precision) + storage_ulp(cleared, precision)
