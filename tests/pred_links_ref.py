"""float64 restatements of the launches of the distribution heads' conv branch on a bf16 handle, one link at a time, for
tests/test_pred_links_cpu.py and tests/test_pred_links_gpu.py: the 313 head's hyper-column chain (deploy_nopred.prototxt:650-775)

    conv3_pred      = conv3x3(conv3_3)
    conv34_pred     = deconv4x4s2(conv4_3) + conv3_pred          ... conv345_pred (conv5_3), conv3456_pred (conv6_3), conv34567_pred (conv7_3)
    conv345678_pred = relu(conv3x3(conv8_3) + conv34567_pred)    (stored as bf16: the only 16-bit tensor of the chain)
    pred_313        = conv1x1(conv345678_pred)

and class_logits = conv1x1(conv8_3) of the 529-bin head.  A link takes what its launch read -- the source tensor and the previous partial
sum, as idc_get_activation returns them (NCHW; a bf16 tensor's values are exact in float32) -- and returns what the launch should have
stored before the storage rounding: weights rounded to bf16 (round to nearest even, as the blob packer stores them), bias in fp32, every
product and sum in float64.  Against it an fp32-stored link shows one launch's fp32 accumulation error and nothing else.

The keyword argument ``fault`` produces the deliberately wrong variants of test_pred_links_cpu.py's mutation checks; no other caller passes it.
Plain and slow on purpose; nothing here reads a file or touches the library."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

from exact_lattice import bf16_rne
from heads_ref import storage_ulp

Link = collections.namedtuple("Link", "name wkey kind src prev relu out_f32")
LINKS = (
    Link("conv3_pred", "pred.conv3_pred", "conv3x3", "conv3_3", None, False, True),
    Link("conv34_pred", "pred.conv4_pred", "deconv", "conv4_3", "conv3_pred", False, True),
    Link("conv345_pred", "pred.conv5_pred", "deconv", "conv5_3", "conv34_pred", False, True),
    Link("conv3456_pred", "pred.conv6_pred", "deconv", "conv6_3", "conv345_pred", False, True),
    Link("conv34567_pred", "pred.conv7_pred", "deconv", "conv7_3", "conv3456_pred", False, True),
    Link("conv345678_pred", "pred.conv8_pred", "conv3x3", "conv8_3", "conv34567_pred", True, False),
    Link("pred_313", "pred.pred_313", "conv1x1", "conv345678_pred", None, False, True),
    Link("class_logits", "model_class.0", "conv1x1", "conv8_3", None, False, True),
)
BY_NAME = {l.name: l for l in LINKS}
CIN = {"conv3_3": 256, "conv4_3": 512, "conv5_3": 512, "conv6_3": 512, "conv7_3": 512, "conv8_3": 256, "conv345678_pred": 384}
COUT = {"pred_313": 313, "class_logits": 529}

# ---- the case both test files share (numpy only: the CPU file must not import the GPU file)
H, W, N = 40, 72, 3                   # quarter grid 10 x 18 (not square, 180 pixels: no multiple of a wave), trunk 5 x 9
MAX_BATCHES = (3, 32)
# The labels the planner gives the links on a bf16 handle with dist and dist313 at 40 x 72 (tools/plan_dump): max_batch 3 takes the batch-1
# families, max_batch 32 the small tile on the deconvs and pred_313 and its 128-pixel form on class_logits.
LABELS = {
    3: {"conv3_pred": "conv_kwave_bf16", "conv34_pred": "conv_kwave_deconv_bf16", "conv345_pred": "conv_kwave_deconv_bf16",
        "conv3456_pred": "conv_kwave_deconv_bf16", "conv34567_pred": "conv_kwave_deconv_bf16", "conv345678_pred": "conv_click<bf16,1,4> splitK4",
        "pred_313": "conv_igemm<bf16,2,1> splitK3", "class_logits": "conv_igemm<bf16,2,1> splitK2"},
    32: {"conv3_pred": "conv_kwave_bf16", "conv34_pred": "conv_igemm<bf16,2,1>", "conv345_pred": "conv_igemm<bf16,2,1>",
         "conv3456_pred": "conv_igemm<bf16,2,1>", "conv34567_pred": "conv_igemm<bf16,2,1>", "conv345678_pred": "conv_click<bf16,1,4> splitK2",
         "pred_313": "conv_igemm<bf16,2,1>", "class_logits": "conv_igemm<bf16,2,2>"},
}

# ---- the bar of tests/test_pred_links_gpu.py: max |got - ref| / (1 + max|ref|) per link, 4 x the largest figure measured on an MI355X over both
# handles and all eight links (that file's docstring has the figures); the mutants of test_pred_links_cpu.py are held against MUTANT_BAR, the
# cap the bar may never exceed
LINK_REL_BAR = 4 * 3.321e-7
MUTANT_BAR = 1e-4


def link(l, x, w, b, prev=None, fault=None):
    """What link `l` holds before it stores: x (n, cin, h, w) its source tensor, w / b the state dict's fp32 weight and bias, prev the previous
    partial sum (n, 384, 2h, 2w for a deconv link) or None."""
    assert (prev is None) == (l.prev is None), l.name
    xt = torch.from_numpy(np.asarray(x, np.float64))
    wt = torch.from_numpy(bf16_rne(np.asarray(w, np.float32)).astype(np.float64))
    bt = torch.from_numpy(np.asarray(b, np.float32).astype(np.float64))
    if fault == "no_bias":
        bt = torch.zeros_like(bt)
    if l.kind == "conv3x3":
        y = F.conv2d(xt, wt, bt, padding=1)
    elif l.kind == "deconv":
        y = F.conv_transpose2d(xt, wt, bt, stride=2, padding=1)
    else:
        y = F.conv2d(xt, wt.reshape(wt.shape[0], -1, 1, 1), bt)
    y = y.numpy()
    if fault == "drop_product":         # one (tap, cin) product lost on the border row: output (image 1, cout 7, y 0, x 5)
        y = y.copy()
        y[1, 7, 0, 5] -= dropped_product(l, x, w)
    if prev is not None:
        y = y + np.asarray(prev, np.float64)
    if l.relu and fault != "no_relu":
        y = np.maximum(y, 0.0)
    return y


def dropped_product(l, x, w):
    """The product the 'drop_product' fault loses at output (n 1, cout 7, y 0, x 5): input channel 3 under the kernel's centre-most tap there."""
    x = np.asarray(x, np.float64)
    wq = bf16_rne(np.asarray(w, np.float32)).astype(np.float64)
    if l.kind == "conv3x3":
        return x[1, 3, 0, 5] * wq[7, 3, 1, 1]
    if l.kind == "deconv":              # out[co, 2m, 2n + 1] takes in[m, n] through W[ci, co, 1, 2]  (oy = 2 iy - 1 + ky, ox = 2 ix - 1 + kx)
        return x[1, 3, 0, 2] * wq[3, 7, 1, 2]
    return x[1, 3, 0, 5] * wq[7, 3, 0, 0]


def stored(l, ref):
    """The reference as the link stores it: fp32 links as they are (to fp32's own rounding), conv345678_pred rounded to bf16."""
    return np.asarray(ref, np.float64) if l.out_f32 else bf16_rne(np.asarray(ref, np.float32)).astype(np.float64)


def bar(l, ref, rel_bar=LINK_REL_BAR):
    """Elementwise bar on |stored - ref|: rel_bar (1 + max|ref|), and on conv345678_pred one bf16 ulp of the expected value as well (the
    storage rounding of a sum that may sit on either side of a rounding boundary), as heads_ref.shift_bar does."""
    ref = np.asarray(ref, np.float64)
    base = np.full(ref.shape, rel_bar * (1.0 + np.abs(ref).max()))
    return base if l.out_f32 else base + storage_ulp(ref, "bf16")


def rel_error(l, got, ref):
    """max over the tensor of (|got - ref| - the storage ulp of a 16-bit link) / (1 + max|ref|): the figure the bar is 4 x of."""
    ref = np.asarray(ref, np.float64)
    err = np.abs(np.asarray(got, np.float64) - ref)
    if not l.out_f32:
        err = np.maximum(err - storage_ulp(ref, "bf16"), 0.0)
    return float(err.max() / (1.0 + np.abs(ref).max()))


def standin_inputs(l, seed=0):
    """Seeded stand-ins for what a link reads on the device, at the shapes of the 40 x 72 case: a non-negative bf16-valued source (the
    trunk's tensors follow a ReLU; its BN shift is left out), an fp32 partial sum of a few units, he-style weights and a small bias."""
    rs = np.random.RandomState(1000 + seed + [k.name for k in LINKS].index(l.name))
    h, w = (H // 8, W // 8) if l.kind == "deconv" else (H // 4, W // 4)
    cin = CIN[l.src]
    cout = COUT.get(l.name, 384)
    x = np.maximum(rs.standard_normal((N, cin, h, w)), 0).astype(np.float32)
    x[1, 3, 0] += 1.0                   # (the product the 'drop_product' fault loses is not a zero of the ReLU)
    x = bf16_rne(x)
    taps = {"conv3x3": 9, "deconv": 4, "conv1x1": 1}[l.kind]
    shape = {"conv3x3": (cout, cin, 3, 3), "deconv": (cin, cout, 4, 4), "conv1x1": (cout, cin, 1, 1)}[l.kind]
    wt = (rs.standard_normal(shape) * np.sqrt(2.0 / (cin * taps))).astype(np.float32)
    b = rs.uniform(-0.5, 0.5, cout).astype(np.float32)
    prev = None if l.prev is None else (2.0 * rs.standard_normal((N, cout, H // 4, W // 4))).astype(np.float32)
    if prev is not None:
        prev[1, 7, 0, 5] = 8.0          # (... and the sum it is lost from is not cut off by the last link's ReLU)
    return x, wt, b, prev
