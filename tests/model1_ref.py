"""model1 (the input pack, conv1_1 + ReLU, conv1_2 + ReLU + eval-BN; models/pytorch/model.py:13-17,139-148) on the integer lattice, for
tests/test_model1_exact_gpu.py and tests/test_model1_exact_cpu.py.

model1's kernels (csrc/idc_conv1.hip, and conv_igemm / conv_click reading the fused input pack) have no single-operator entry: their input
is the three planes a forward is handed.  So the lattice of tests/exact_lattice.py is put where a forward can carry it:
  planes    L_mc = 100 k, ab = 110 k, mask in {0, 1}, maskcent = 0: the pack L / 100, ab / 110, mask * 1 - 0 (true fp32 division) gives the
            integers k in [-2, 2], different per image, non-zero on the image border and on both sides of every tile edge
  weights   model1.0 / model1.2: integers in [-w_max, w_max] (1 or 2 per row), small integer biases; half of conv1_2's couts lean positive so
            that their sums reach thousands (16-bit stores round, on exact ties too), the other half stay zero-mean (the ReLU is live)
  model1.4  running_mean 0, bias an integer in [-8, 8], weight one of 0.5 / 1 / 2, running_var float32(1 - 1e-5): the packer's float64 fold
            gamma / sqrt(var + 1e-5), rounded to fp32, is that power of two exactly (bn_fold asserts it)
Every conv1_1 value is then an integer of at most 256: exact in bf16 and in fp16, and held by the hi part of a split tensor ALONE -- on this lattice
the lo and mid parts of conv1_1 and of every weight are zero, so the split pair's lo / mid segments multiply zeros here; the rows of
tests/test_model1_carry_gpu.py (keyword `carry`) give conv1_1 values and conv1_2 weights that need the other parts.  Every partial sum of
conv1_2's K = 576 loop stays below 2^24, and the expected tensors are ONE float64 computation plus the storage rounding of the path,
compared bit for bit (exact_lattice.compare).  The rest of the network keeps its seeded weights; only model1's tensors are read.

The keyword ``fault`` produces the deliberately wrong variants of test_model1_exact_cpu.py; no other caller passes it.
A helper, not a conftest: nothing here touches the library or a GPU."""
import collections

import numpy as np

import exact_lattice as xl

H, W, N = 40, 72, 3               # 40 rows: 12+12+12+4 (32 x 12 tile), five 8-row tiles, 16+16+8 (split conv1_1), 32+8; 72 columns: 32+32+8
K_MAX = 2                         # packed inputs: integers in [-2, 2]
B1_MAX, B2_MAX = 4, xl.B_MAX
BN_SCALES = (0.5, 1.0, 2.0)
BN_EPS = 1e-5
C1_LIMIT = 256                    # integers up to 2^8 are exact in bf16
TILE_EDGES_X, TILE_EDGES_Y = (31, 32, 63, 64), (7, 8, 11, 12)

# One row of tests/test_model1_exact_gpu.py: the handle (precision, max_batch, idc_set_option pairs), the tensors read back, the labels
# layer_table() must give for conv1_1 and conv1_2, the weight range of the row's draw.  partner: a -DIDC_AB_PARTNERS build only.
Row = collections.namedtuple("Row", "id precision max_batch opts read conv1_1 conv1_2 w_max partner")


def row(id, precision, max_batch, read, conv1_1, conv1_2, w_max, opts=(), partner=False):
    return Row(id, precision, max_batch, tuple(opts), tuple(read), conv1_1, conv1_2, w_max, partner)


# max_batch follows from plan_forward / choose_kernel (csrc/idc_plan.hip) at 40 x 72, three 32-wide tile columns:
#   conv1_block_fused, 32 x 12 tile   t32 = 3 * 2 * max_batch >= 128                     -> 32 (192)
#   conv1_block_fused, 32 x 8 tile    t32 < 128 and t8 = 3 * 5 * max_batch >= 128        -> 16 (96, 240)
#   conv1_1_split_kernel              3 * max_batch * 3 (16-row tiles) >= 128            -> 32 (288)
#   conv1_2_split_kernel              3 * max_batch * 4 (12-row tiles) >= 256            -> 32 (384)
#   conv1_1_bf16_kernel               3 * max_batch * 2 (32-row tiles) >= 128            -> 32 (192)
#   max_batch 1: neither block tile reaches 128 workgroups, conv1_1 is its own launch on the small tile.  A max_batch = 1 handle takes the three
#   images one call each; max_batch 3 plans the same kernels and carries them in one call
# The layer table does not name the block's tile or its fp16 twin (conv1_block_fused_th): both follow from max_batch and the precision.
# Every label below is what the planner gives for the row's configuration (tools/plan_dump prints it without a device).
ROWS = [
    row("bf16_block_32x12", "bf16", 32, ("conv1_2",), "conv1_block_fused", "fused into conv1_1", 2),
    row("bf16_block_32x8", "bf16", 16, ("conv1_2",), "conv1_block_fused", "fused into conv1_1", 1),
    row("fp16_block_32x12", "fp16", 32, ("conv1_2",), "conv1_block_fused", "fused into conv1_1", 2, opts=(("fp16_fast", 1),)),
    row("fp16_block_32x8", "fp16", 16, ("conv1_2",), "conv1_block_fused", "fused into conv1_1", 2, opts=(("fp16_fast", 1),)),
    row("bf16x3_split_pair", "bf16x3", 32, ("conv1_1", "conv1_2"), "conv1_1_split_kernel", "conv1_2_split_kernel x3", 2),
    row("bf16x6_split_pair", "bf16x6", 32, ("conv1_1", "conv1_2"), "conv1_1_split_kernel", "conv1_2_split_kernel x6", 1),
    row("fp16x3_split_pair", "fp16x3", 32, ("conv1_1", "conv1_2"), "conv1_1_split_kernel", "conv1_2_split_kernel x3", 2),
    row("fp16_split_pair", "fp16", 32, ("conv1_1", "conv1_2"), "conv1_1_split_kernel", "conv1_2_split_kernel x1", 2, opts=(("fp16_fast", 0),)),
    # conv1_1 as its own launch outside model1's kernels: conv_igemm reading the fused input pack (K = 36 im2col); the labels are what the plan gives
    row("fp32_batch1", "fp32", 1, ("conv1_1", "conv1_2"), "conv_igemm<f32,1,1> splitK2", "conv_wino_f32", 2),
    row("fp32_batch3", "fp32", 3, ("conv1_1", "conv1_2"), "conv_igemm<f32,1,1> splitK2", "conv_wino_f32", 1),             # batch 1's kernels, three images in one call
    row("fp32_batch24", "fp32", 24, ("conv1_1", "conv1_2"), "conv_igemm<f32,1,2>", "conv_wino_f32", 1),       # the tile the 256 x 256 batch-1 forward takes
    row("bf16_batch1", "bf16", 1, ("conv1_1", "conv1_2"), "conv_igemm<bf16,1,1>", "conv_kwave_bf16", 2),
    row("bf16_batch3", "bf16", 3, ("conv1_1", "conv1_2"), "conv_igemm<bf16,1,1>", "conv_kwave_bf16", 1),
    row("bf16_unfused", "bf16", 32, ("conv1_1", "conv1_2"), "conv_igemm<bf16,1,2>", "conv_igemm<bf16,1,2>", 1, opts=(("fuse_conv1", 0),)),
    row("bf16_conv1_1_partner", "bf16", 32, ("conv1_1",), "conv1_1_bf16_kernel", "conv_igemm<bf16,1,2>", 1, opts=(("fuse_conv1", 0),), partner=True),
]
assert len(set(r.id for r in ROWS)) == len(ROWS)
BY_ID = {r.id: r for r in ROWS}


def _seed(r, salt):
    return (sum(ord(ch) * (i + 1) for i, ch in enumerate(r.id)) * 7 + salt) % (2 ** 31)


def _ints(rs, lo, hi, shape):
    return rs.randint(lo, hi + 1, size=shape).astype(np.float32)


def model1_tensors(r, w1_max=None, w2_m=0, w2_mag=1, bn_scales=BN_SCALES):
    """The state-dict entries of model1 for a row's draw: lattice weights, integer biases, the BN of the module docstring.
    The keywords are those of the carry rows (tests/test_model1_carry_gpu.py; the defaults leave every draw as it was): conv1_1 weights in
    [-w1_max, w1_max], conv1_2 weights exactly w2_m entries of +-[ceil(w2_mag / 2), w2_mag] per cout, BN scales drawn from bn_scales."""
    rs = np.random.RandomState(_seed(r, 1))
    w1 = _ints(rs, -(w1_max or r.w_max), w1_max or r.w_max, (64, 4, 3, 3))
    b1 = _ints(rs, -B1_MAX, B1_MAX, (64,))
    w2 = _ints(rs, -r.w_max, r.w_max, (64, 64, 3, 3))
    # couts 32..63 of conv1_2: half of the negative weights turned positive, so that their sums reach thousands -- beyond fp16's 11 bits as
    # odd integers and halves, deep into bf16's rounding -- while couts 0..31 stay zero-mean and keep conv1_2's ReLU live on both sides
    flip = rs.randint(0, 2, size=(32, 64, 3, 3)) > 0
    w2[32:] = np.where(flip, np.abs(w2[32:]), w2[32:])
    if w2_m:
        pos = np.argsort(rs.rand(64, 576), axis=1)[:, :w2_m]
        val = _ints(rs, (w2_mag + 1) // 2, w2_mag, (64, w2_m)) * np.where(rs.randint(0, 2, size=(64, w2_m)) > 0, 1.0, -1.0).astype(np.float32)
        w2 = np.zeros((64, 576), np.float32)
        w2[np.arange(64)[:, None], pos] = val
        w2 = w2.reshape(64, 64, 3, 3)
    return {
        "model1.0.weight": w1,
        "model1.0.bias": b1,
        "model1.2.weight": w2,
        "model1.2.bias": _ints(rs, -B2_MAX, B2_MAX, (64,)),
        "model1.4.weight": rs.choice(np.asarray(bn_scales, np.float32), 64).astype(np.float32),
        "model1.4.bias": _ints(rs, -xl.BN_SHIFT_MAX, xl.BN_SHIFT_MAX, (64,)),
        "model1.4.running_mean": np.zeros(64, np.float32),
        "model1.4.running_var": np.full(64, np.float32(1.0 - BN_EPS), np.float32),
        "model1.4.num_batches_tracked": np.array(1, dtype=np.int64),
    }


def state_dict(r, base, **draw):
    """`base` (a whole seeded state dict, left unchanged) with model1's tensors replaced by the row's draw."""
    sd = dict(base)
    sd.update(model1_tensors(r, **draw))
    return sd


def planes(r):
    """(L_mc (N,1,H,W), ab (N,2,H,W), mask (N,1,H,W), maskcent): the integers k times 100 / 110, the mask in {0, 1}; every image its own
    draw; no zero on the outermost rows and columns nor on either side of a tile edge."""
    rs = np.random.RandomState(_seed(r, 2))
    k = _ints(rs, -K_MAX, K_MAX, (N, 4, H, W))
    k[:, 3] = _ints(rs, 0, 1, (N, H, W))
    sign = np.where(rs.randint(0, 2, size=(N, 3, H, W)) > 0, 1.0, -1.0).astype(np.float32)
    edge = np.zeros((H, W), bool)
    edge[[0, H - 1], :] = True
    edge[:, [0, W - 1]] = True
    edge[list(TILE_EDGES_Y), :] = True
    edge[:, list(TILE_EDGES_X)] = True
    k[:, :3] = np.where(edge[None, None] & (k[:, :3] == 0), sign, k[:, :3])
    k[:, 3] = np.where(edge[None], 1.0, k[:, 3])
    L = (np.float32(100.0) * k[:, 0:1]).astype(np.float32)
    ab = (np.float32(110.0) * k[:, 1:3]).astype(np.float32)
    mask = np.ascontiguousarray(k[:, 3:4], np.float32)
    assert all(np.abs(L[i] - L[j]).max() > 0 and np.abs(ab[i] - ab[j]).max() > 0 and np.abs(mask[i] - mask[j]).max() > 0
               for i in range(N) for j in range(i))
    return np.ascontiguousarray(L), np.ascontiguousarray(ab), mask, 0.0


def pack(L, ab, mask, maskcent=0.0, l_div=100.0, ab_div=110.0, mask_mul=1.0):
    """The input pack as the kernels compute it -- fp32 division, fp32 multiply and subtract -- asserted to be the integer lattice."""
    x = np.concatenate([L.astype(np.float32) / np.float32(l_div), ab.astype(np.float32) / np.float32(ab_div),
                        mask.astype(np.float32) * np.float32(mask_mul) - np.float32(maskcent)], axis=1)
    assert x.dtype == np.float32 and np.array_equal(x, np.round(x)) and np.abs(x).max() <= K_MAX, "the packed planes left the integer lattice"
    return x.astype(np.float64)


def bn_fold(t):
    """The packer's fold of model1.4 (csrc/idc_pack.hip: float64 gamma / sqrt(var + 1e-5) and beta - mean * that, rounded to fp32), asserted
    to be exactly the power of two and the integer the draw intended."""
    s64 = t["model1.4.weight"].astype(np.float64) / np.sqrt(t["model1.4.running_var"].astype(np.float64) + BN_EPS)
    scale = s64.astype(np.float32)
    shift = (t["model1.4.bias"].astype(np.float64) - t["model1.4.running_mean"].astype(np.float64) * s64).astype(np.float32)
    assert np.array_equal(scale, t["model1.4.weight"]) and np.isin(scale, BN_SCALES).all(), "the folded BN scale is not the power of two"
    assert np.array_equal(shift, t["model1.4.bias"]) and np.array_equal(shift, np.round(shift)), "the folded BN shift is not the integer"
    return scale, shift


def _conv3x3(xp, w):
    """xp (n, cin, h + 2, w + 2), already padded; w (cout, cin, 3, 3) -> (n, cout, h, w), float64."""
    n, _, hp, wp = xp.shape
    h, ww = hp - 2, wp - 2
    out = np.zeros((n, w.shape[0], h, ww), np.float64)
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("oc,nchw->nohw", w[:, :, ky, kx], xp[:, :, ky:ky + h, kx:kx + ww], optimize=True)
    return out


def _pad(x, p=1):
    return np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)))


# where the faults strike: image 1 of 3, pixels at tile corners (32 x 12, 32 x 8, 32 x 16, 32 x 32 tiles, the image's own corners) ...
CORNERS = [(11, 31), (12, 32), (7, 31), (8, 32), (15, 63), (16, 64), (31, 31), (32, 32), (0, 0), (H - 1, W - 1)]
# ... conv1_1 halo sites OUTSIDE the image (y, x), next to a tile corner or the image's ...
OUTSIDE = [(-1, -1), (-1, 31), (-1, 32), (H, 63), (H, W), (7, -1), (12, W)]
# ... and columns of the row below image 0's last one (the next image's first row in memory)
BELOW = [0, 31, 32, W - 1]
_STAGES = {}


def _stages(r, carry=None):
    """The fault-free computation of a row, once: operands, conv1_1, conv1_2's sums -- and the assertions of expected()'s docstring.
    carry: the draw keywords of a carry row and "c1_limit", the largest conv1_1 value its split storage holds with zero residue."""
    key = r.id if carry is None else (r.id,) + tuple(sorted(carry.items()))
    if key in _STAGES:
        return _STAGES[key]
    draw = {k: v for k, v in (carry or {}).items() if k != "c1_limit"}
    c1_limit = (carry or {}).get("c1_limit", C1_LIMIT)
    t = model1_tensors(r, **draw)
    L, ab, mask, maskcent = planes(r)
    x = pack(L, ab, mask, maskcent)
    scale, shift = bn_fold(t)
    w1, b1 = t["model1.0.weight"].astype(np.float64), t["model1.0.bias"].astype(np.float64)
    w2, b2 = t["model1.2.weight"].astype(np.float64), t["model1.2.bias"].astype(np.float64)
    for a in (w1, b1, w2, b2):
        assert np.array_equal(a, np.round(a)), "%s: a model1 tensor is not on the integer lattice" % r.id
    assert 36 * np.abs(x).max() * np.abs(w1).max() + np.abs(b1).max() <= c1_limit, "%s: conv1_1's worst case leaves bf16's exact integers" % r.id
    pre1 = _conv3x3(_pad(x), w1) + b1[None, :, None, None]
    c1 = np.maximum(pre1, 0.0)
    assert np.array_equal(c1, np.round(c1)) and c1.max() <= c1_limit, "%s: a conv1_1 value is not a bf16-exact integer" % r.id
    c1max = float(c1.max())
    acc_bound = 576 * c1max * np.abs(w2).max() + np.abs(b2).max()
    if carry is not None:
        # a carry row: at most w2_m terms meet in an output, each the sum over the kept segments of the parts' maxima (carry_lattice); the parts hold
        # conv1_1 and conv1_2's weights with zero residue, and one of the two fits ONE part, so that no dropped segment multiplies two non-zeros
        import carry_lattice as cl
        acc_bound = carry["w2_m"] * cl.segment_sum(r.precision, c1max, float(np.abs(w2).max())) + np.abs(b2).max()
        p1, p2 = cl.parts(c1.astype(np.float32), r.precision), cl.parts(w2.astype(np.float32), r.precision)
        assert np.array_equal(sum(p.astype(np.float64) for p in p1), c1) and np.array_equal(sum(p.astype(np.float64) for p in p2), w2), r.id
        assert not p1[1].any() or not p2[1].any(), "%s: both conv1_2 operands carry" % r.id
    # the fp32 forward may run conv1_2 as Winograd F(2x2,3x3): U = G g G^T holds quarters (|U| <= 9/4 max|w|), the input transform sums four
    # pixels, the output transform 3 x 3 products' sums -- exact in fp32 while the bound, counted in quarters, stays below 2^24
    wino_bound = 4 * (64 * (4 * c1max) * (9 * np.abs(w2).max() / 4) * 9) if carry is None else 0.0      # (carry rows are split-precision rows: no Winograd)
    pre_bound = acc_bound * max(BN_SCALES) + xl.BN_SHIFT_MAX
    assert max(acc_bound, wino_bound, pre_bound) < xl.EXACT_LIMIT, "%s: a partial sum can leave the exact fp32 range (%.0f, %.0f, %.0f)" % (
        r.id, acc_bound, wino_bound, pre_bound)
    acc = _conv3x3(_pad(c1), w2) + b2[None, :, None, None]
    _STAGES[key] = dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, scale=scale, shift=shift, pre1=pre1, c1=c1, acc=acc,
                         bounds=(c1max, acc_bound, wino_bound, pre_bound))
    return _STAGES[key]


def _change_site(acc, w, n, sy, sx, delta):
    """acc += the 3x3 conv's response to adding `delta` (cin,) to its zero-padded input at site (sy, sx) of image n (-1 and H / W: the padding)."""
    hh, ww = acc.shape[2], acc.shape[3]
    for ky in range(3):
        for kx in range(3):
            oy, ox = sy + 1 - ky, sx + 1 - kx
            if 0 <= oy < hh and 0 <= ox < ww:
                acc[n, :, oy, ox] += w[:, :, ky, kx] @ delta


def expected(r, fault=None, site=None, carry=None):
    """{"conv1_1": ..., "conv1_2": ...} as float32 arrays (N, 64, H, W): what activation() must return, bit for bit (shared: leave them as
    they are).  Asserts, before anything runs on a GPU: the packed planes and the BN fold are on the lattice, every conv1_1 value is a
    bf16-exact integer, every partial-sum bound is below 2^24, every expected conv1_2 value fits the storage of a split precision."""
    st = _stages(r, carry)
    x, w1, b1, w2 = st["x"], st["w1"], st["b1"], st["w2"]
    c1, acc = st["c1"], st["acc"]
    if fault in ("drop_product_conv1_1", "pack_next_image"):
        pre1 = st["pre1"].copy()
        if fault == "drop_product_conv1_1":     # one tap-channel term of conv1_1 missing at one pixel of image 1, for every cout
            y0, x0 = site
            xp = _pad(x)
            ch, ky, kx = [(ch, ky, kx) for ky in range(3) for kx in range(3) for ch in range(4) if xp[1, ch, y0 + ky, x0 + kx] != 0][0]
            pre1[1, :, y0, x0] -= w1[:, ch, ky, kx] * xp[1, ch, y0 + ky, x0 + kx]
        else:                                   # the plane read below image 0's last row runs into image 1's first row
            _change_site(pre1, w1, 0, H, site[1], x[1, :, 0, site[1]])
        c1_new = np.maximum(pre1, 0.0)
        acc = acc.copy()
        for n, y, xx in np.argwhere((c1_new != c1).any(axis=1)):          # conv1_2 sees the few changed conv1_1 sites
            _change_site(acc, w2, n, y, xx, c1_new[n, :, y, xx] - c1[n, :, y, xx])
        c1 = c1_new
    if fault == "halo_not_zeroed":              # a conv1_1 halo site outside image 1 holds ReLU(bias + its partial window), not conv1_2's zero padding
        hy, hx = site
        assert not (0 <= hy < H and 0 <= hx < W)
        ext = np.maximum(_conv3x3(_pad(x[1:2], 2), w1) + b1[None, :, None, None], 0.0)     # conv1_1 on the (H + 2) x (W + 2) sites of the halo
        assert ext[0, :, hy + 1, hx + 1].max() > 0
        acc = acc.copy()
        _change_site(acc, w2, 1, hy, hx, ext[0, :, hy + 1, hx + 1])
    if fault == "next_image_halo":              # the halo row below image 0 taken from image 1's first row
        assert c1[1, :, 0, site[1]].max() > 0
        acc = acc.copy()
        _change_site(acc, w2, 0, H, site[1], c1[1, :, 0, site[1]])
    if fault == "drop_product":                 # ONE tap-channel term missing at one pixel of image 1 (for every cout: a lost element of the B fragment)
        y0, x0 = site
        c1p = _pad(c1[1:2])
        ci, ky, kx = [(ci, ky, kx) for ky in range(3) for kx in range(3) for ci in range(64) if c1p[0, ci, y0 + ky, x0 + kx] != 0][0]
        assert np.abs(w2[:, ci, ky, kx]).max() > 0
        acc = acc.copy()
        acc[1, :, y0, x0] -= w2[:, ci, ky, kx] * c1p[0, ci, y0 + ky, x0 + kx]
    assert np.array_equal(acc, np.round(acc)) and np.abs(acc).max() < xl.EXACT_LIMIT, r.id
    v = acc.astype(np.float32)                  # exact: integers below 2^24
    s, sh = st["scale"][None, :, None, None], st["shift"][None, :, None, None]
    if fault == "bn_before_relu":
        v = np.maximum((v * s).astype(np.float32) + sh, np.float32(0))
    else:
        v = (np.maximum(v, np.float32(0)) * s).astype(np.float32) + sh         # a power of two times an integer, plus an integer: exact
    v = np.ascontiguousarray(v, np.float32)
    c1f = np.ascontiguousarray(c1, np.float32)
    if fault == "truncating_store":
        return {"conv1_1": c1f, "conv1_2": store_truncating(r, v)}
    if fault is not None:                       # (the storage-fit assertion is about the right values, made once below)
        return {"conv1_1": c1f, "conv1_2": v if xl.STORAGE[r.precision] == "split" else xl.store(r, v)}
    if "expected" not in st:
        st["expected"] = {"conv1_1": xl.store(r, c1f), "conv1_2": xl.store(r, v)}
    return st["expected"]


def store_truncating(r, v):
    """A 16-bit store that drops the low bits instead of rounding to nearest even (split storage keeps every bit of a fitting value:
    there is nothing to truncate)."""
    kind = xl.STORAGE[r.precision]
    if kind == "bf16":
        return xl.bf16_trunc(v)
    if kind == "fp16":
        assert np.abs(v).max() < 65504 and (np.abs(v[v != 0]) >= 2.0 ** -14).all()
        u = np.ascontiguousarray(v, np.float32).view(np.uint32) & np.uint32(0xffffe000)      # fp16 keeps 10 of fp32's 23 fraction bits
        return u.view(np.float32).reshape(v.shape)
    return xl.store(r, v)
