"""Replicated lattice batches and launch-grid arithmetic for the occupancy tests (tests/test_ops_occupancy_gpu.py, tests/test_ops_occupancy_cpu.py).

On the integer lattice of tests/exact_lattice.py every summation order gives the same bits, so a batch made of a few DISTINCT lattice images
repeated many times has an exact expected output that costs one float64 computation of the distinct images: replicate() tiles the operands
in a seeded order in which no two neighbours are the same image, the expected output is exp[order].  That lets an exact case fill the chip
(a thousand workgroups and more) for the price of three images.

workgroups() and residency() restate, from the source, the grid each launcher makes and the workgroups of that kernel one CU holds; the file
and line of every restated expression stands beside it (interactive_deep_colorization_amd/csrc/, lines as of this file's commit).  The rows
of the GPU file live here (ROWS, HALF_PAIRS, BATCH1_ROWS) so that the CPU file can hold every row's grid, residency and host size to the
conditions without a device.

residency = min(launch bound, floor(160 KiB / LDS bytes of the launch), 32 waves / waves per workgroup).  It is an UPPER bound of what the
hardware does: a kernel's register count can lower it further, and the conditions below only ask for grids large enough, so the bound errs
on the side of a larger batch.

A helper, not a conftest and not a test module: nothing here touches the library or a GPU.
"""
import re

import numpy as np

import exact_lattice as xl
from test_ops_exact_gpu import CASES as EXACT_CASES

CUS = 256                                 # MI355X
LDS_PER_CU = 160 * 1024
WAVES_PER_CU = 32
HOST_CAP = 512 << 20                      # host arrays of one case: operands, output and expected output, fp32
MIN_GRID = 1024

# idc_layout.h:20-24
K_ROW_BYTES, K_SLOT_BYTES, K_SLOTS, K_COUT_GROUP = 128, 16, 8, 64
K_WBLOCK_BYTES = K_COUT_GROUP * K_ROW_BYTES


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------- a case's launch geometry
def cout_pad(cout):
    return 64 if cout <= 64 else _cdiv(cout, 128) * 128                  # idc_net.h:79


def geometry(c):
    """What run_single_op (idc_diag.hip:261-281) and fill_taps (idc_plan.hip:73-108) make of a case: the site grid Hs x Ws the tiles cover (a
    deconv's INPUT, a conv's output), cout groups, cin chunks, phases, halo, dilation."""
    deconv = c.op in ("deconv", "fused")
    kc = 32 if c.precision == "fp32" else 64                               # idc_layout.h:69  channels per 128-byte chunk
    return dict(Hs=c.h if deconv else c.h // c.in_stride, Ws=c.w if deconv else c.w // c.in_stride, ncg=cout_pad(c.cout) // K_COUT_GROUP,
                nkc=c.cin // kc, nphase=4 if deconv else 1, halo=1 if deconv else (c.dilation if c.ksize == 3 else 0), d=c.dilation,
                so=2 if deconv else 1)


_V2 = re.compile(r"^conv_igemm_v2(ph|psh|ps|sh|s)?<(\d),(\d)>(x\d)?(\+m16p?)?$")
_IGEMM = re.compile(r"^conv_igemm<(f32|bf16),(\d),(\d)>(?: splitK(\d+))?$")
_CLICK = re.compile(r"^conv_click<(f32|bf16),1,(\d)>(?: splitK(\d+))?$")
_DS = re.compile(r"^conv_ds_fused_m(h|sh|s)?\+shortcut(?: x\d)?(?: (half|8-wave))?$")


def _wino_form(c, g, n):
    """<TB,CB> of conv_wino_f32: option 'winograd' = 12 / 21 / 22 forces it, else by the grid of the launch (idc_wino.hip:751-755)."""
    forced = dict(c.opts).get("winograd", 0)
    if forced in (12, 21, 22):
        return forced // 10, forced % 10
    t2 = _cdiv(_cdiv(g["Ws"], g["d"]), 16) * _cdiv(_cdiv(g["Hs"], g["d"]), 8) * g["d"] ** 2 * n
    return (2, 2) if t2 * g["ncg"] * 2 >= 256 else (1, 2)


def _kw_form(nkc):
    """<NKC,TWB,NW> of conv_kwave_bf16 by cin chunks (idc_kw.hip:726-729)."""
    return {8: (8, 1, 8), 4: (4, 2, 8), 2: (2, 2, 4), 1: (1, 2, 4)}[nkc]


def launch(c, n, label):
    """(workgroups, waves per workgroup, launch bound or None, dynamic LDS bytes, output rows and columns one workgroup owns) of the launch
    `label` makes for case c at batch n."""
    g = geometry(c)
    Hs, Ws, ncg, nkc, nphase, halo, d, so = (g[k] for k in ("Hs", "Ws", "ncg", "nkc", "nphase", "halo", "d", "so"))
    m = _V2.match(label)
    if m:
        wm, wp = int(m.group(2)), int(m.group(3))
        # grid: idc_v2m.hip:765 (v2p / v2ph), :789 (v2m), :807 (v2s / v2sh), :826 (v2ps / v2psh): tiles_x * tiles_y * N * (ncg / wm) [* nphase],
        # tiles of 32 x 4*wp sites (idc_plan.hip:138,155); the 3x3 forms have one phase
        blocks = _cdiv(Ws, 32) * _cdiv(Hs, 4 * wp) * n * (ncg // wm) * nphase
        # LDS: TileKernel::lds_bytes, idc_v2m.hip:730-735; launch bounds (WCO*WPX*64, 2): idc_v2m.hip:363-367, 717-723
        nt = wm * wp * 64
        items = _cdiv((32 + 2 * halo) * (4 * wp + 2 * halo) * K_SLOTS, nt)
        lds = items * nt * K_SLOT_BYTES + 2 * (64 * wm) * K_ROW_BYTES
        return blocks, wm * wp, 2, lds, (4 * wp * so, 32 * so)
    m = _IGEMM.match(label)
    if m:
        wm, wp, ks = int(m.group(2)), int(m.group(3)), int(m.group(4) or 1)
        # grid: idc_igemm.hip:662, tiles of 16 x 4*wp sites (idc_plan.hip:207-208)
        blocks = _cdiv(Ws, 16) * _cdiv(Hs, 4 * wp) * n * (ncg // wm) * nphase * ks
        # LDS: conv_lds_bytes_c, idc_igemm.hip:649-655; __launch_bounds__(WM*WP*64), no second figure: idc_igemm.hip:33
        nt = wm * wp * 64
        items = _cdiv((16 + 2 * halo) * (4 * wp + 2 * halo) * K_SLOTS, nt)
        lds = items * nt * K_SLOT_BYTES + 2 * (64 * wm) * K_ROW_BYTES + (18 * (4 * wp + 2) * 16 if halo == 0 else 0)
        return blocks, wm * wp, None, lds, (4 * wp * so, 16 * so)
    m = _CLICK.match(label)
    if m:
        wp, ks = int(m.group(2)), int(m.group(3) or 1)
        # grid: idc_igemm.hip:611; LDS: click_lds_bytes, idc_igemm.hip:591-600 (two halo buffers when a workgroup walks more than one chunk);
        # __launch_bounds__(WP*64, 2): idc_igemm.hip:311
        blocks = _cdiv(Ws, 16) * _cdiv(Hs, 4 * wp) * n * ncg * nphase * ks
        kc_per = _cdiv(nkc, ks)
        nt = wp * 64
        halo_bytes = _cdiv((16 + 2 * halo) * (4 * wp + 2 * halo) * K_SLOTS, nt) * nt * K_SLOT_BYTES
        lds = max((2 if kc_per > 1 else 1) * halo_bytes + 4 * K_WBLOCK_BYTES, wp * 4096)
        return blocks, wp, 2, lds, (4 * wp * so, 16 * so)
    m = _DS.match(label)
    if m:
        # grid: idc_dsm.hip:500 (8-wave: blocks, half: 2 * blocks, :504-509), :523 (ms / msh); tiles of 32 x 4 sites = 64 x 8 output pixels
        # (idc_dsm.hip:67); LDS: 160 KiB on every form (:504-509, :525-526); launch bounds (NCW*256, 2): idc_dsm.hip:467-472
        blocks = _cdiv(Ws, 32) * _cdiv(Hs, 4) * n * (ncg // 2)
        half = m.group(2) == "half"
        return (2 * blocks if half else blocks), (4 if half else 8), 2, 160 * 1024, (8, 64)
    if label == "conv_kwave_bf16":
        NKC, TWB, NW = _kw_form(nkc)
        # grid: idc_kw.hip:704-706; LDS: kw_lds_bytes, idc_kw.hip:48-54; __launch_bounds__(NW*64, 2): idc_kw.hip:63
        blocks = _cdiv(_cdiv(Ws, d), 8 * TWB) * _cdiv(_cdiv(Hs, d), 8) * d * d * n * (ncg * 2)
        nt = NW * 64
        halo_bytes = _cdiv(NKC * 10 * (8 * TWB + 2) * 8, nt) * nt * K_SLOT_BYTES
        return blocks, NW, 2, max(halo_bytes, NW * 8192) + 256, (8 * d, 8 * TWB * d)
    if label == "conv_kwave_deconv_bf16":
        # grid: idc_kw.hip:716-718; LDS: kwd_lds_bytes, idc_kw.hip:56-60; __launch_bounds__(512, NKC == 8 ? 2 : 4): idc_kw.hip:260
        blocks = _cdiv(Ws, 8) * _cdiv(Hs, 8) * n * (ncg * 4)
        halo_bytes = _cdiv(nkc * 800, 512) * 512 * K_SLOT_BYTES
        return blocks, 8, (2 if nkc == 8 else 4), max(halo_bytes, 8 * (4 // (8 // nkc)) * 4096) + 256, (16, 16)
    if label == "conv_wino_f32":
        TB, CB = _wino_form(c, g, n)
        # grid: idc_wino.hip:734-736; LDS: wino_lds, idc_wino.hip:39-45; __launch_bounds__(512, 2): idc_wino.hip:52
        blocks = _cdiv(_cdiv(Ws, d), 8 * TB) * _cdiv(_cdiv(Hs, d), 8) * d * d * n * (ncg * 4 // CB)
        v_bytes = 16 * 16 * TB * K_ROW_BYTES
        p_bytes = _cdiv(10 * (8 * TB + 2) * 8, 512) * 512 * K_SLOT_BYTES
        return blocks, 8, 2, (2 if TB == 1 else 1) * v_bytes + 2 * p_bytes, (8 * d, 8 * TB * d)
    if label == "conv_wino_deconv_f32":
        # grid: idc_wino.hip:716-721; LDS: kWinoDLds, idc_wino.hip:505-508; __launch_bounds__(768, 3): idc_wino.hip:511
        blocks = _cdiv(Ws, 8) * _cdiv(Hs, 8) * n * (ncg * 4)
        return blocks, 12, 3, 36 * 16 * K_ROW_BYTES + 2 * (2 * 1024 * K_SLOT_BYTES), (16, 16)
    raise KeyError("no launcher restated for label %r" % label)


def workgroups(c, n, label):
    """The grid the launcher of `label` makes for case c at batch n."""
    return launch(c, n, label)[0]


_HALOS = {"conv": (0, 1, 2), "deconv": (1,), "fused": (1,)}


def residency(label, c=None):
    """Workgroups of the kernel of `label` one CU holds: min(launch bound, floor(160 KiB / LDS of the launch), 32 / waves per workgroup).
    With the case: of that launch.  Without: the largest figure over the halos and chunk counts the label launches with (the grid
    conditions then ask for the larger batch)."""
    if c is not None:
        _, waves, bound, lds, _ = launch(c, c.n, label)
        return min(x for x in (bound, LDS_PER_CU // lds, WAVES_PER_CU // waves) if x is not None)
    best = 0
    for op, ksize, dil, cin in ((op, k, dd, cin) for op in ("conv", "deconv", "fused") for k in (1, 3) for dd in (1, 2) for cin in (64, 128, 256, 512)):
        if (op != "conv" and (ksize != 3 or dil != 1)) or (ksize == 1 and dil != 1):
            continue
        precision = "fp32" if "f32" in label else "bf16"
        probe = xl.case("probe", op, precision, 1, cin, 128, 8, 32, label, ksize=ksize, dilation=dil, cin2=64 if op == "fused" else 0)
        try:
            best = max(best, residency(label, probe))
        except (KeyError, ZeroDivisionError):
            continue
    assert best > 0, label
    return best


def tile_of(c, label, y, x):
    """(tile row, tile column) of output pixel (y, x) in the tiling `label` gives case c, and the tile's (rows, columns) in output pixels."""
    rows, cols = launch(c, c.n, label)[4]
    return (y // rows, x // cols), (rows, cols)


# ---------------------------------------------------------------------------------------------------------------- replicated batches
def make_order(seed, n_big, distinct):
    """order[i] in range(distinct), seeded; no two neighbours equal, every distinct image at least n_big // (distinct + 1) times."""
    assert distinct >= 2 and n_big >= distinct
    need = n_big // (distinct + 1)
    for attempt in range(1000):
        rs = np.random.RandomState((seed + 7919 * attempt) % (2 ** 31))
        order = np.empty(n_big, np.int64)
        order[0] = rs.randint(distinct)
        steps = rs.randint(1, distinct, size=n_big)                        # a step of 1 .. distinct-1 never lands on the same image
        for i in range(1, n_big):
            order[i] = (order[i - 1] + steps[i]) % distinct
        if np.bincount(order, minlength=distinct).min() >= need:
            return order
    raise AssertionError("no order of %d images over %d distinct ones met the counts" % (n_big, distinct))


def balanced_order(seed, distinct, copies):
    """An order of distinct * copies images with every distinct image EXACTLY `copies` times and no two neighbours equal: `copies` seeded
    permutations of range(distinct) in a row, a permutation drawn again while it would begin with the image the one before ended on."""
    assert distinct >= 2
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(copies):
        p = rs.permutation(distinct)
        while out and p[0] == out[-1]:
            p = rs.permutation(distinct)
        out.extend(int(v) for v in p)
    return np.asarray(out, np.int64)


def _seed(c):
    return sum(ord(ch) * (i + 3) for i, ch in enumerate(c.id)) % (2 ** 31)


def replicate(c, n_big, distinct=3):
    """-> (operands of the n_big-image batch, expected output of the DISTINCT images, order).  The batch's expected output is exp[order]."""
    assert c.n == distinct, "%s: the case carries n = %d, %d distinct images asked" % (c.id, c.n, distinct)
    d = xl.draw(c)
    exp = xl.expected(c, d)                                                # asserts the lattice bounds and the storage fit
    exp.setflags(write=False)
    order = make_order(_seed(c), n_big, distinct)
    big = dict(d)
    for k in ("x", "resid", "x2"):
        if k in d:
            big[k] = np.ascontiguousarray(d[k][order])
    return big, exp, order


def host_bytes(c, n_big):
    """fp32 bytes of the host arrays of one replicated case: x (+ resid, x2), the output and the materialised expected output."""
    ho, wo = xl.out_hw(c)
    per_image = c.cin * c.h * c.w + 2 * c.cout * ho * wo + (c.cout * ho * wo if c.resid else 0) + (c.cin2 * ho * wo if c.op == "fused" else 0)
    return 4 * n_big * per_image


def compare_replicated(got, exp, order, c, label, what=""):
    """exact_lattice.compare(got, exp[order]); a failure also names the image, its place in `order`, the tile, and whether the other copies
    of the same distinct image agree among themselves (a fault of one workgroup against a fault of the kernel)."""
    got = np.asarray(got)
    try:
        xl.compare(got, exp[order], what)
        return
    except AssertionError as e:
        first = str(e)
    bad = np.argwhere(~(got == exp[order]))
    i, _, y, x = (int(v) for v in bad[0])
    k = int(order[i])
    copies = np.flatnonzero(order == k)
    others = [int(j) for j in copies if j != i]
    agree = all(np.array_equal(got[others[0]], got[j]) for j in others[1:]) if others else True
    others_right = sum(1 for j in others if np.array_equal(got[j], exp[k]))
    (ty, tx), (rows, cols) = tile_of(c, label, y, x)
    tiles = [tuple(int(v) for v in t) for t in np.unique(np.stack([bad[:, 0], bad[:, 2] // rows, bad[:, 3] // cols], axis=1), axis=0)]
    raise AssertionError("%s\n  image %d is copy %d of %d of distinct image %d (order[%d] = %d); first mismatch in tile (row %d, column %d) of the %d x %d-pixel "
                         "tiles; %d (image, tile) pairs differ: %s%s; the other %d copies of distinct image %d %s among themselves, %d of them equal the expectation"
                         % (first, i, int(np.searchsorted(copies, i)) + 1, len(copies), k, i, k, ty, tx, rows, cols, len(tiles), tiles[:6],
                            " ..." if len(tiles) > 6 else "", len(others), k, "agree" if agree else "DISAGREE", others_right))


# ---------------------------------------------------------------------------------------------------------------- the rows of the GPU file
def _exact(case_id):
    return [c for c in EXACT_CASES if c.id == case_id][0]


def occupancy_row(case_id, distinct=3, **changes):
    """A row of the exact table under a name of its own (its own draw), carrying `distinct` images."""
    return _exact(case_id)._replace(id="occ_" + case_id, n=distinct, **changes)


def smallest_batch(c):
    """The smallest batch at which the launch of c.label has workgroups >= 2 * CUS * residency (co-residency and a second wave) and >= 1024."""
    want = max(MIN_GRID, 2 * CUS * residency(c.label, c))
    per_image = workgroups(c, 1, c.label)
    n = _cdiv(want, per_image)
    assert workgroups(c, n, c.label) >= want > workgroups(c, n - 1, c.label)
    return n


# throughput families: one row per label of the exact table that a policy batch of 16 or more (or tile="large") reaches, at the table's own
# ragged sizes (7 x 33, 5 x 9, 10 x 18, 20 x 36, 40 x 72); the policy batch stays the table's, the launch carries n_big = smallest_batch(row)
ROWS = [occupancy_row(i) for i in (
    "bf16_v2p_42_halo1", "bf16_v2p_42_halo2", "bf16_v2p_22_half_tiles", "bf16_v2p_22_stride2",
    "bf16_v2m_24_deconv", "bf16_v2m_42_deconv", "bf16_v2m_22_halo2", "bf16_v2m_24_1x1_529",
    "bf16_ds_8wave",
    "bf16_f32out_22_384", "f32_igemm_22_deconv_resid",
    "fp16_v2ph_42", "fp16_v2ph_22", "fp16_v2sh_24_deconv", "fp16_ds_8wave",
    "bf16x3_v2ps_42", "bf16x6_v2ps_42_leaky", "fp16x3_v2psh_42_halo2", "bf16x3_v2s_24_deconv", "bf16x6_v2s_42_deconv",
    "bf16x3_ds_ms", "bf16x6_ds_ms", "fp16x3_ds_msh",
)]

# the half form of conv_ds_fused_m / _mh exists only while blocks < CUs (conv_ds_m_half, idc_dsm.hip:491-496: blocks counts 128-cout
# workgroups of the LAUNCHED batch): (half row, the 8-wave row of the same shape)
HALF_PAIRS = [
    (occupancy_row("bf16_ds_half"), occupancy_row("bf16_ds_half", label="conv_ds_fused_m+shortcut 8-wave")._replace(id="occ_bf16_ds_past_half")),
    (occupancy_row("fp16_ds_half"), occupancy_row("fp16_ds_half", label="conv_ds_fused_mh+shortcut 8-wave")._replace(id="occ_fp16_ds_past_half")),
]


def half_pair_batches(c_half, cus):
    """(largest batch that still takes the half form, first batch past the switch) on a device of `cus` CUs; None where the shape cannot
    straddle the CU count with at least as many images as the row has distinct ones."""
    per_image = workgroups(c_half, 1, c_half.label.replace(" half", " 8-wave"))      # 128-cout workgroups per image
    n_half = (cus - 1) // per_image
    if n_half < c_half.n:
        return None
    assert per_image * n_half < cus <= per_image * (n_half + 1)
    return n_half, n_half + 1


# batch-1 families at the network's own level sizes for one 256 x 256 image (32 x 32 x 512, 64 x 64 x 256, 128 x 128 x 128), two distinct
# images, nothing replicated: the variant is chosen for policy batch 1, as the table's rows choose it.
#   conv_wino_f32: the form follows the LAUNCHED grid (idc_wino.hip:751-755) and two images of 32 x 32 x 512 reach <2,2>; the shipped batch-1
#   launch is <1,2>, so the rows force it (option winograd = 12), 256 workgroups per image as shipped.
#   conv_click<bf16,1,2>: rows-of-4 per workgroup drop to 2 only below 8 site rows (idc_plan.hip:186), which no level of a 256 x 256 image has:
#   that row runs at 7 x 33.  (Below 4 site rows they drop to 1: the conv_click<T,1,1> rows `*_click11_*` of tests/test_ops_exact_gpu.py, which
#   the nets of tests/small_nets.py plan and tests/test_small_nets_gpu.py runs through whole forwards.)
BATCH1_ROWS = [
    occupancy_row("bf16_kwave_8chunks", 2, h=32, w=32),
    occupancy_row("bf16_kwave_8chunks_d2", 2, h=32, w=32),
    occupancy_row("bf16_kwave_4chunks_leaky", 2, h=64, w=64),
    occupancy_row("bf16_kwave_2chunks", 2, h=128, w=128),
    occupancy_row("bf16_kwave_deconv_8chunks", 2, h=32, w=32),
    occupancy_row("bf16_kwave_deconv_4chunks", 2, h=64, w=64),
    occupancy_row("bf16_click_leaky_resid", 2, h=64, w=64),
    occupancy_row("bf16_click_d2_resid", 2, h=7, w=33),
    occupancy_row("f32_click_d2", 2, h=32, w=32, label="conv_click<f32,1,4> splitK16"),
    occupancy_row("f32_wino12", 2, h=32, w=32),
    occupancy_row("f32_wino21_d2", 2, h=32, w=32, opts=(("winograd", 12),)),
    occupancy_row("f32_wino_deconv", 2, h=32, w=32),
]

ALL_ROWS = ROWS + [c for pair in HALF_PAIRS for c in pair] + BATCH1_ROWS
assert len(set(c.id for c in ALL_ROWS)) == len(ALL_ROWS)
