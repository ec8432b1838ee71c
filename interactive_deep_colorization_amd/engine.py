"""HipColorizer -- thin Python owner of one ``idc_handle`` (one GPU, one stream).

Stands where ``SIGGRAPHGenerator`` (``models/pytorch/model.py:5-175``) stands in
the reference: ``forward(L_mc, ab, mask, maskcent)`` returns the raw ab map the
reference returns at ``data/colorize_image.py:263``.  All arithmetic happens in
the HIP library behind the C ABI (``include/ideepcolor.h``); this file only
marshals numpy arrays and weight dictionaries.
"""
import collections
import ctypes
import threading

import numpy as np

from . import _native as N

_PREC = {"fp32": N.IDC_FP32, "f32": N.IDC_FP32, "float32": N.IDC_FP32, 0: N.IDC_FP32,
         "bf16": N.IDC_BF16, "bfloat16": N.IDC_BF16, 1: N.IDC_BF16,
         # operand-split precisions (round 6): fp32 values carried as 2 / 3 bf16 parts, 3 / 6 bf16 MFMA products per fp32 product
         "bf16x3": N.IDC_BF16X3, 2: N.IDC_BF16X3, "bf16x6": N.IDC_BF16X6, 3: N.IDC_BF16X6,
         "fp16x3": N.IDC_FP16X3, 4: N.IDC_FP16X3, "fp16": N.IDC_FP16, 5: N.IDC_FP16}


_INTERP = {"cubic": N.IDC_INTERP_CUBIC, "linear": N.IDC_INTERP_LINEAR, "nearest": N.IDC_INTERP_NEAREST, "joint": N.IDC_INTERP_JOINT}
_INGEST_FILTER = {"bilinear": N.IDC_FILTER_BILINEAR, "antialias": N.IDC_FILTER_ANTIALIAS}
_OUT_FORMAT = {"rgb": N.IDC_OUT_RGB, "i420": N.IDC_OUT_I420, "nv12": N.IDC_OUT_NV12}
_YCC_MATRIX = {"jfif": N.IDC_YCC_JFIF, "bt709": N.IDC_YCC_BT709_VIDEO}
YCC420 = collections.namedtuple("YCC420", "y cb cr buf")       # I420: views [h,w], [ch,cw], [ch,cw] into ``buf``, one uint8 block
NV12 = collections.namedtuple("NV12", "y cbcr buf")            # NV12: views [h,w], [ch,cw,2] into ``buf``


def ycc420_bytes(h, w):
    """Bytes of one image's 4:2:0 plane block (``idc_ycc420_bytes``): h*w + 2*((h+1)//2)*((w+1)//2); 0 for a side outside 1..16384."""
    return int(N.load().idc_ycc420_bytes(int(h), int(w)))


def ycc420_views(buf, h, w, format="i420"):
    """The planes of one image's block as numpy views into ``buf`` (uint8, at least ``ycc420_bytes(h, w)`` long): a ``YCC420``
    ``(y, cb, cr, buf)`` for 'i420', an ``NV12`` ``(y, cbcr, buf)`` for 'nv12'."""
    h, w = int(h), int(w)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    buf = np.asarray(buf).reshape(-1)
    if buf.dtype != np.uint8 or buf.size < h * w + 2 * ch * cw:
        raise ValueError("ycc420_views needs a uint8 buffer of %d bytes" % (h * w + 2 * ch * cw))
    y = buf[:h * w].reshape(h, w)
    if format == "nv12":
        return NV12(y, buf[h * w:h * w + 2 * ch * cw].reshape(ch, cw, 2), buf)
    if format != "i420":
        raise ValueError("format is 'i420' or 'nv12', got %r" % (format,))
    return YCC420(y, buf[h * w:h * w + ch * cw].reshape(ch, cw), buf[h * w + ch * cw:h * w + 2 * ch * cw].reshape(ch, cw), buf)


def _fptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _f32c(a, shape=None):
    """float32, C-contiguous view/copy (bool masks and f64 GUI arrays accepted)."""
    out = np.ascontiguousarray(np.asarray(a), dtype=np.float32)
    if shape is not None and tuple(out.shape) != tuple(shape):
        raise ValueError("expected shape %s, got %s" % (tuple(shape), out.shape))
    return out


def state_dict_to_numpy(sd):
    """Accept a torch ``state_dict`` (tensors) or a dict of arrays; return {name: f32 ndarray}."""
    out = {}
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            continue
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        out[k] = np.ascontiguousarray(np.asarray(v), dtype=np.float32)
    return out


def _tensor_descs(sd):
    sd = state_dict_to_numpy(sd)
    names = sorted(sd)
    arr = (N.TensorDesc * len(names))()
    keep = []
    for i, k in enumerate(names):
        a = sd[k]
        if a.ndim > 4:
            raise ValueError("tensor %s has %d dims" % (k, a.ndim))
        kb = k.encode()
        keep.append((kb, a))
        arr[i].name = kb
        arr[i].data = _fptr(a)
        arr[i].ndim = a.ndim
        for d in range(a.ndim):
            arr[i].dims[d] = a.shape[d]
    return arr, len(names), keep


TILE_POLICIES = {"auto": 0, "small": 1, "large": 2}


def set_tile_policy(policy="auto"):
    """Process-wide tile-shape policy of the conv kernels (speed only; same results): "auto",
    "small" (conv_igemm only) or "large" (conv_igemm_v2 wherever it applies, bf16)."""
    N.check(N.load().idc_set_tile_policy(TILE_POLICIES[policy] if isinstance(policy, str) else int(policy)))


def _flags(dist=False, global_hints=False, dist313=False, throughput_blob=False):
    return ((N.IDC_FLAG_DIST_HEAD if dist else 0) | (N.IDC_FLAG_GLOBAL_HINTS if global_hints else 0) |
            (N.IDC_FLAG_DIST313 if dist313 else 0) | (N.IDC_FLAG_THROUGHPUT_BLOB if throughput_blob else 0))


SPLITK_POLICIES = {"auto": 0, "never": 1, "always": 2}


def set_option(name, value):
    """Process-wide switches (``idc_set_option``; speed / kernel choice only -- every setting computes the same function).  Names and values are
    documented in ``include/ideepcolor.h``: 'fuse_conv1', 'click', 'winograd', 'mfma16', 'v2p', 'ds_mfma16', 'kwave', 'kwave_chain', and since
    round 6 'split_ds_fuse', 'conv1_1_split', 'conv1_2_split', 'spin_sync', 'pcie_kernel' (former environment switches) and the test hooks 'kw_force_abort' and 'grid_cap' (grid_tags() / grid_last()).  'mfma16' = 0 / 'ds_mfma16' = 0 select the
    32x32x16-MFMA partner kernels, which exist only in a ``make EXTRA=-DIDC_AB_PARTNERS`` build: the default library raises IdcError (UNSUPPORTED)."""
    N.check(N.load().idc_set_option(name.encode(), int(value)))


def set_splitk_policy(policy="auto"):
    """Process-wide split-K policy of the small-tile kernels (speed only): "auto", "never" or "always"."""
    N.check(N.load().idc_set_splitk_policy(SPLITK_POLICIES[policy] if isinstance(policy, str) else int(policy)))


# The conv layers in the order of the engine's layer table (csrc/idc_net.h; HipColorizer.layer_table() on a handle): row 0 is the global-hints
# branch, the conv layers follow, then the head and the 529-bin softmax.  Activation exponents are indexed by that table.
_CONV_LAYERS = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3",
                "conv5_1", "conv5_2", "conv5_3", "conv6_1", "conv6_2", "conv6_3", "conv7_1", "conv7_2", "conv7_3",
                "conv3_3_short", "conv8_1", "conv8_2", "conv8_3", "class_logits", "conv2_2_short", "conv9_1", "conv9_2",
                "conv1_2_short", "conv10_1", "conv10_2")
_PRED_LAYERS = ("conv3_pred", "conv34_pred", "conv345_pred", "conv3456_pred", "conv34567_pred", "conv345678_pred", "pred_313")


def layer_table_names(dist=False, dist313=False):
    """Row names of the layer table a handle with these flags has (no handle, no GPU needed)."""
    rows = [n for n in _CONV_LAYERS if dist or n != "class_logits"] + (list(_PRED_LAYERS) if dist313 else [])
    return ["glob_branch"] + rows + ["head", "dist_softmax"]


def _act_exp_array(act_exp, dist=False, dist313=False):
    """``act_exp`` as the C int array of the ``_ex`` entry points: None -> (None, 0); a dict {layer name: exponent} is laid out over the layer
    table of these flags (unnamed layers 0); a sequence is passed on as it is (its length is checked by the library)."""
    if act_exp is None:
        return None, 0
    if isinstance(act_exp, dict):
        names = layer_table_names(dist, dist313)
        unknown = sorted(set(act_exp) - set(names))
        if unknown:
            raise KeyError("no layer named %s" % ", ".join(unknown))
        act_exp = [int(act_exp.get(nm, 0)) for nm in names]
    vals = [int(v) for v in act_exp]
    return (ctypes.c_int * max(len(vals), 1))(*vals), len(vals)


def pack_weights(sd, precision="bf16", dist=False, global_hints=False, dist313=False, throughput_blob=False, act_exp=None):
    """Host-only: reference ``state_dict`` -> packed device-ready blob (uint8 ndarray).
    Needs no GPU (used by rank 0 before the RCCL broadcast).  ``throughput_blob``: without the Winograd images of the
    batch-1 / fp32 kernels (IDC_FLAG_THROUGHPUT_BLOB: fp32 136 MB instead of 384 MB; a bf16 blob is 68 MB either way) -- must match the handle's.
    ``act_exp`` (fp16x3 only; ``calibrate_activation_exponents``): per-layer activation exponents, a sequence over the layer table or a dict
    {layer name: exponent}; None or all zeros = the plain blob, byte for byte."""
    lib = N.load()
    prec = _PREC[precision]
    flags = _flags(dist, global_hints, dist313, throughput_blob)
    nbytes = lib.idc_weights_blob_bytes(prec, flags)
    blob = np.zeros(nbytes, dtype=np.uint8)
    arr, n, keep = _tensor_descs(sd)
    ae, n_layers = _act_exp_array(act_exp, dist, dist313)
    if ae is None:
        N.check(lib.idc_pack_weights(prec, flags, arr, n, blob.ctypes.data_as(ctypes.c_void_p), nbytes))
    else:
        N.check(lib.idc_pack_weights_ex(prec, flags, arr, n, ae, n_layers, blob.ctypes.data_as(ctypes.c_void_p), nbytes))
    del keep
    return blob


# Calibration target: the largest value a calibration image produced in a tensor lands in (2^(TARGET_EXP-1), 2^TARGET_EXP] = (2048, 4096].
# fp16 saturates at 65504 ~ 2^16, so images the calibration did not see have 16x headroom; and the lo part of a stored value v 2^a is a normal
# fp16 number while |v 2^a| >= 2^-14 * 2^11 = 2^-3, i.e. values down to 2^-15 of the tensor's maximum keep all 22 bits of hi + lo.
TARGET_EXP = 12
ACT_EXP_RANGE = (-24, 24)       # what the packer accepts (csrc/idc_net.h kActExpMax); exponents beyond are clipped to it


def exponents_from_report(report, target_exp=TARGET_EXP, clip=ACT_EXP_RANGE):
    """Range-audit report (``HipColorizer.range_report()``) -> activation exponents over the same layer table:
    a = target_exp - ceil(log2(max_abs)), clipped; 0 where the layer stored nothing (n_values == 0) or stored only zeros."""
    out = []
    for row in report:
        mx = float(row["max_abs"])
        if row["n_values"] == 0 or not (mx > 0.0) or not np.isfinite(mx):
            out.append(0)
            continue
        m, e = np.frexp(mx)                                  # mx = m 2^e, m in [0.5, 1): ceil(log2(mx)) = e, or e - 1 for an exact power of two
        ceil_log2 = int(e) - 1 if m == 0.5 else int(e)
        a = int(target_exp) - ceil_log2 + int(row.get("act_exp", 0))      # (a report of scaled tensors: max_abs is of value * 2^act_exp)
        out.append(int(min(max(a, clip[0]), clip[1])))
    return out


def calibrate_activation_exponents(sd, L_mc, ab, mask, maskcent=0.0, device=0, dist=False, throughput_blob=False, io_scales=None,
                                   target_exp=TARGET_EXP, engine_factory=None):
    """Activation exponents for ``precision='fp16x3'`` from calibration images: a temporary ``bf16x6`` engine (fp16x3's layer table and
    kernels, fp32's exponent range) runs the batch with the range audit on; each layer's exponent brings the largest value seen to
    ``2^target_exp`` (``exponents_from_report``).  Returns a list over the layer table, for ``load_state_dict(sd, act_exp=...)`` /
    ``pack_weights(..., act_exp=...)``.  ``io_scales``: keyword arguments of ``set_io_scales`` (the Caffe twin's)."""
    L_mc = np.asarray(L_mc)
    if L_mc.ndim == 3:
        L_mc, ab, mask = L_mc[None], np.asarray(ab)[None], np.asarray(mask)[None]
    n, H, W = L_mc.shape[0], L_mc.shape[2], L_mc.shape[3]
    make = engine_factory or HipColorizer
    e = make(H, W, max_batch=n, precision="bf16x6", device=device, dist=dist, throughput_blob=throughput_blob)
    try:
        if io_scales:
            e.set_io_scales(**io_scales)
        e.load_state_dict(sd)
        e.set_range_audit(True)
        e.forward(L_mc, ab, mask, maskcent)
        report = e.range_report()
    finally:
        e.close()
    return exponents_from_report(report, target_exp)


class _PinnedBuffer(object):
    """Owner of one idc_alloc_host allocation.  numpy arrays made from it (``np.asarray`` through the array interface)
    hold it as their base, so the pinned memory is returned to the driver only when the last view is collected."""

    def __init__(self, lib, nbytes):
        self._lib = lib
        self.nbytes = max(int(nbytes), 1)
        self.ptr = lib.idc_alloc_host(self.nbytes)
        if not self.ptr:
            raise MemoryError("idc_alloc_host(%d) failed" % self.nbytes)

    @property
    def __array_interface__(self):
        return {"shape": (self.nbytes,), "typestr": "|u1", "data": (int(self.ptr), False), "version": 3}

    def __del__(self):
        try:
            if self.ptr:
                self._lib.idc_free_host(ctypes.c_void_p(self.ptr))
                self.ptr = None
        except Exception:
            pass


class _PinnedPool(object):
    """Recycled pinned result buffers of the blocking calls.  ``take`` returns a fresh numpy array over pinned memory (the
    library then copies device -> caller in place, no staging memcpy); when the last view of it is collected the memory goes
    back on the free list instead of to the driver (hipHostMalloc / hipHostFree cost more than the copy they save).  An array
    is never handed out while another array still views the same memory, so results keep the value semantics of ``np.empty``
    outputs.  Bounded on both sides: buffers above ``MAX_ONE`` or beyond ``MAX_TOTAL`` retained (free-list) bytes are plain
    numpy / freed, and at most ``MAX_LIVE`` bytes of pinned memory are in callers' hands at any time -- a caller that keeps
    many results alive gets pageable ``np.empty`` arrays beyond that (the library stages those through its own pinned
    buffer), so kept outputs cannot pin unbounded host RAM.  Counters are guarded by a lock (results may be
    dropped on any thread)."""
    MAX_ONE = 32 << 20
    MAX_TOTAL = 256 << 20
    MAX_LIVE = 512 << 20

    def __init__(self, lib):
        self.lib = lib
        self.free = {}                      # nbytes -> [ptr]
        self.retained = 0                   # bytes on the free lists
        self.live = 0                       # pinned bytes currently viewed by arrays handed out
        # re-entrant: give() runs from __del__, and a cyclic-GC pass triggered by an allocation INSIDE a locked region can finalise
        # another pooled buffer on the same thread (a plain Lock would deadlock there); the counters tolerate the nesting
        self._lock = threading.RLock()

    def take(self, shape, dtype):
        shape = tuple(int(x) for x in shape)
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if nbytes == 0 or nbytes > self.MAX_ONE:
            return np.empty(shape, dtype)
        with self._lock:
            if self.live + nbytes > self.MAX_LIVE:
                return np.empty(shape, dtype)
            lst = self.free.get(nbytes)
            ptr = lst.pop() if lst else None
            if ptr is not None:
                self.retained -= nbytes
            self.live += nbytes
        try:
            owner = _PooledPinned(self, nbytes, ptr)
        except MemoryError:
            with self._lock:
                self.live -= nbytes
            return np.empty(shape, dtype)
        return np.asarray(owner)[:nbytes].view(dtype).reshape(shape)

    def give(self, ptr, nbytes):
        with self._lock:
            self.live -= nbytes
            keep = self.retained + nbytes <= self.MAX_TOTAL
            if keep:
                self.free.setdefault(nbytes, []).append(ptr)
                self.retained += nbytes
        if not keep:
            self.lib.idc_free_host(ctypes.c_void_p(ptr))

    def drain(self):
        with self._lock:
            ptrs = [p for lst in self.free.values() for p in lst]
            self.free = {}
            self.retained = 0
        for p in ptrs:
            self.lib.idc_free_host(ctypes.c_void_p(p))


class _PooledPinned(_PinnedBuffer):
    def __init__(self, pool, nbytes, ptr=None):
        self._pool = pool
        if ptr:
            self._lib, self.nbytes, self.ptr = pool.lib, nbytes, ptr
        else:
            _PinnedBuffer.__init__(self, pool.lib, nbytes)

    def __del__(self):
        try:
            if self.ptr:
                self._pool.give(self.ptr, self.nbytes)
                self.ptr = None
        except Exception:
            pass


_POOLS = {}


def _result_pool(lib):
    pool = _POOLS.get(id(lib))
    if pool is None:
        pool = _POOLS[id(lib)] = _PinnedPool(lib)
    return pool


def trim_pinned_pool():
    """Return the recycled pinned result buffers nobody views any more to the driver (at most ``_PinnedPool.MAX_TOTAL`` bytes
    are ever retained; buffers still viewed by a live array are untouched)."""
    for pool in _POOLS.values():
        pool.drain()


def flatten_hints(hints, n):
    """Per-image hint lists -> what ``idc_forward_async_rgb`` reads: (offsets (n+1,) int32, ``N.Hint`` array).  ``hints``: ``None`` (no image
    has hints: (None, None)) or n entries, each ``None`` / a list of rows (y0, x0, y1, x1, c0, c1[, c2]) as in ``set_hints``; image i's rows
    are ``[offsets[i], offsets[i+1])`` of the array."""
    if hints is None:
        return None, None
    lists = [[] if h is None else [tuple(r) for r in h] for h in hints]
    if len(lists) != n:
        raise ValueError("%d hint lists for %d images" % (len(lists), n))
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum([len(l) for l in lists])
    arr = (N.Hint * max(int(offsets[-1]), 1))()
    k = 0
    for rows in lists:
        for r in rows:
            arr[k].y0, arr[k].x0, arr[k].y1, arr[k].x1 = int(r[0]), int(r[1]), int(r[2]), int(r[3])
            arr[k].c0, arr[k].c1, arr[k].c2 = float(r[4]), float(r[5]), float(r[6]) if len(r) > 6 else 0.0
            k += 1
    return offsets, arr


def dist_queries(queries, seed=0):
    """Suggestion queries -> the ``N.DistQuery`` array ``idc_suggest_colors_batch`` / ``idc_forward_async_dist`` read, or ``None`` for none.
    Rows are (img, y, x[, seed]); a row without a seed takes ``seed`` + its index.  (y, x) == (-1, -1) is the empty query."""
    rows = [] if queries is None else [tuple(int(v) for v in r) for r in queries]
    if not rows:
        return None
    arr = (N.DistQuery * len(rows))()
    for q, r in enumerate(rows):
        arr[q].img, arr[q].y, arr[q].x = r[0], r[1], r[2]
        arr[q].seed = (r[3] if len(r) > 3 else int(seed) + q) & 0xFFFFFFFF
    return arr


class DistBatch(object):
    """What ``forward_async_dist`` returns: the arrays a distribution batch fills, valid after the slot's ``wait``; ``None`` where not asked for."""
    sse = hint_colours = out_rgb = out_ab = peaks = peak_ent = entropy = sugg_centres = sugg_conf = score = None


class DistScore(object):
    """What ``dist_score`` returns and ``forward_async_dist(score=...)`` fills (``DistBatch.score``): ``xent`` (n,) float64 = the SUM of the
    cells' cross-entropies per image (``mean()`` divides by the cell count), ``hits`` (n, len(ranks)) uint32 = cells whose true bin is among the
    head's ranks[j] most probable, and with the maps asked for ``xent_map`` (n,Hd,Wd) float64, ``rank_map`` / ``target`` (n,Hd,Wd) int32 and
    ``truth_ab`` (n,2,Hd,Wd) float32; ``None`` otherwise."""
    xent = hits = xent_map = rank_map = target = truth_ab = None
    cells = 0

    def mean(self):
        """Mean cross-entropy per image, (n,) float64."""
        return np.asarray(self.xent, np.float64) / float(self.cells)

    def rates(self):
        """Top-k rates per image, (n, len(ranks)) float64."""
        return np.asarray(self.hits, np.float64) / float(self.cells)


def score_spec(nn=1, sigma=5.0, ranks=(1, 5)):
    """``N.DistScoreSpec`` of a distribution score: ``nn`` neighbours and ``sigma`` of the soft encoding, up to 8 top-k thresholds."""
    ranks = [int(r) for r in ranks]
    if len(ranks) > N.IDC_SCORE_MAX_RANKS:
        raise ValueError("%d rank thresholds, more than %d" % (len(ranks), N.IDC_SCORE_MAX_RANKS))
    spec = N.DistScoreSpec()
    spec.nn, spec.sigma, spec.n_ranks = int(nn), float(sigma), len(ranks)
    for j, r in enumerate(ranks):
        spec.ranks[j] = r
    return spec


def score_buffers(n, grid, n_ranks, want_maps, take):
    """(``DistScore`` with its arrays allocated by ``take(shape, dtype)``, the ``N.DistScoreOut`` that points into them)."""
    res, out = DistScore(), N.DistScoreOut()
    res.cells = int(grid[0]) * int(grid[1])
    res.xent = take((n,), np.float64)
    out.xent = res.xent.ctypes.data
    res.hits = take((n, n_ranks), np.uint32)
    if n_ranks:
        out.hits = res.hits.ctypes.data
    if want_maps:
        res.xent_map, res.rank_map = take((n,) + tuple(grid), np.float64), take((n,) + tuple(grid), np.int32)
        res.target, res.truth_ab = take((n,) + tuple(grid), np.int32), take((n, 2) + tuple(grid), np.float32)
        out.xent_map, out.rank_map = res.xent_map.ctypes.data, res.rank_map.ctypes.data
        out.target, out.truth_ab = res.target.ctypes.data, res.truth_ab.ctypes.data
    return res, out


def ref_images(refs):
    """Reference photographs -> what the ``idc_*_ref*`` calls read: (``N.RefImage`` array, the uint8 C-contiguous arrays it points into).  Each
    entry is an (h,w,3) uint8 array of its own size; the library copies the pixels before the call returns, the arrays only have to live until then."""
    keep = []
    for r in refs:
        a = np.ascontiguousarray(np.asarray(r), dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError("a reference must be an (h,w,3) uint8 image, got %s" % (a.shape,))
        keep.append(a)
    arr = (N.RefImage * max(len(keep), 1))()
    for k, a in enumerate(keep):
        arr[k].rgb, arr[k].h, arr[k].w = a.ctypes.data, a.shape[0], a.shape[1]
    return arr, keep


def dedupe_refs(refs, n):
    """Per-image references (n entries, each ``None`` or an array) -> (the distinct arrays in order of first use, ref_index (n,) int32 with -1
    for ``None``).  Distinct means object identity: the same array object given for several images is uploaded once."""
    refs = list(refs)
    if len(refs) != n:
        raise ValueError("%d references for %d images" % (len(refs), n))
    uniq, where, index = [], {}, np.full(n, -1, np.int32)
    for i, r in enumerate(refs):
        if r is None:
            continue
        if id(r) not in where:
            where[id(r)] = len(uniq)
            uniq.append(r)
        index[i] = where[id(r)]
    return uniq, index


def _ref_index(ref_index, n):
    if ref_index is None:
        return None
    idx = np.ascontiguousarray(np.asarray(ref_index), dtype=np.int32)
    if idx.shape != (n,):
        raise ValueError("ref_index must have %d entries, got %s" % (n, idx.shape))
    return idx


def _ref_args(refs, ref_index, centres, hist_flag, saturation, n):
    """The reference arguments of a pipelined call, checked: (m, ``N.RefImage`` array or None, ref_index (n,) int32 or None, centres (313,2)
    float32 or None, hist_flag, flags) and the arrays the table points into.  All of it has to live until the call has returned: it copies."""
    if isinstance(refs, np.ndarray) and refs.ndim == 3:
        refs = [refs]
    rarr, keep = ref_images(refs)
    idx = _ref_index(ref_index, n)
    c = _f32c(centres, (313, 2)) if centres is not None else None
    return (len(keep), rarr if keep else None, idx, c, float(hist_flag), N.IDC_REF_SATURATION if saturation else 0), keep


def _image_item(who, item, with_ref):
    """One item of ``who``'s image stream -- ``rgb``, ``(rgb, hints)`` or, ``with_ref``, ``(rgb, hints, ref)`` -- as (rgb, hints) or
    (rgb, hints, ref, whether the item had a reference field)."""
    item = (item,) if isinstance(item, np.ndarray) else tuple(item)
    rgb = np.asarray(item[0])
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.size == 0:
        raise ValueError("%s needs uint8 (h,w,3) images, got %s %s" % (who, rgb.dtype, rgb.shape))
    hints = item[1] if len(item) > 1 else None
    return (rgb, hints, item[2] if len(item) > 2 else None, len(item) > 2) if with_ref else (rgb, hints)


def _layer_array(who, layer):
    """A painted hint layer as the library reads it: (lh,lw,4) uint8 RGBA, C-contiguous."""
    a = np.asarray(layer)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4 or a.size == 0:
        raise ValueError("%s needs uint8 (h,w,4) RGBA layers, got %s %s" % (who, a.dtype, a.shape))
    return np.ascontiguousarray(a)


def _gray_item(who, item, with_ref):
    """``_image_item`` for greyscale planes: ``gray`` (h,w) uint8 or uint16, its dtype kept."""
    item = (item,) if isinstance(item, np.ndarray) else tuple(item)
    gray = np.asarray(item[0])
    if gray.dtype not in (np.uint8, np.uint16) or gray.ndim != 2 or gray.size == 0:
        raise ValueError("%s needs uint8 or uint16 (h,w) planes, got %s %s" % (who, gray.dtype, gray.shape))
    hints = item[1] if len(item) > 1 else None
    return (gray, hints, item[2] if len(item) > 2 else None, len(item) > 2) if with_ref else (gray, hints)


class HipColorizer(object):
    _out_format, _out_matrix = "rgb", "jfif"    # what set_batch_output last set (class defaults: an engine that never called it)
    _temporal = None                            # what set_temporal_filter last set: None = off, else the dict of its four parameters

    def __init__(self, H=256, W=None, max_batch=1, precision="bf16", device=0, dist=False, global_hints=False, dist313=False,
                 throughput_blob=False):
        self.lib = N.load()
        self.H, self.W = int(H), int(H if W is None else W)
        self.max_batch = int(max_batch)
        self.precision = precision
        self._prec = _PREC[precision]
        self.dist = bool(dist)
        self.device = int(device)
        self.global_hints = bool(global_hints)
        self.dist313 = bool(dist313)
        self.throughput_blob = bool(throughput_blob)
        self._flags = _flags(dist, global_hints, dist313, throughput_blob)
        self._h = ctypes.c_void_p()
        N.check(self.lib.idc_create(self.device, self.H, self.W, self.max_batch, self._prec, self._flags,
                                    ctypes.byref(self._h)))
        self._blob_keepalive = None
        self._pool = _result_pool(self.lib)
        # pipeline slot -> the arrays forward_async_rgb handed to the library, held until wait(slot).  A blocking call drains the slots inside the
        # library, so an entry can outlive its batch until that slot's next wait or forward_async_rgb: it only keeps the arrays alive longer
        self._in_flight = {}
        self.forward_serial = 0             # bumped by every call that replaces the handle's resident results (api.py's lazy output attributes)
        self.l_serial = 0                   # bumped by every call that may write image slot 0's L plane (set_image_l and every forward): api.py's resident L
        self._src_shape = {}                # image slot -> (h, w) of the source set_image_rgb(keep_source=True) left on the device
        self.before_overwrite = None        # callable run ONCE right before the next such call: whoever still wants the resident results fetches them
        self._batch_upsample = "linear"     # what set_batch_upsample last set: the source-size upsampling of the pipelined calls
        self._ingest_filter = "bilinear"    # what set_ingest_filter last set: how every source is brought to the net size

    # ---- lifetime -------------------------------------------------------------------------
    def close(self):
        """Destroy the handle (idc_destroy drains its streams first).  Pinned buffers handed out by ``pinned_empty``
        are NOT freed here: each is released when the last numpy view of it is garbage-collected, so an array that
        outlives the engine stays valid memory."""
        if getattr(self, "_h", None) is not None and self._h:
            cb, self.before_overwrite = getattr(self, "before_overwrite", None), None
            if cb is not None:                        # somebody still wants the resident results (api.py's lazy output attributes): last chance
                try:
                    cb()
                except Exception:
                    pass
            for slot in (0, 1):                       # batches still in flight own caller buffers: finish them first
                try:
                    self.lib.idc_wait(self._h, slot)
                except Exception:
                    pass
            self.lib.idc_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, status):
        return N.check(status, self._h)

    # ---- weights --------------------------------------------------------------------------
    def load_state_dict(self, sd, act_exp=None):
        """``act_exp`` (fp16x3 only): per-layer activation exponents as ``pack_weights`` takes them; None = the plain load."""
        arr, n, keep = _tensor_descs(sd)
        ae, n_layers = _act_exp_array(act_exp, self.dist, self.dist313)
        if ae is None:
            self._chk(self.lib.idc_load_weights(self._h, arr, n))
        else:
            self._chk(self.lib.idc_load_weights_ex(self._h, arr, n, ae, n_layers))
        del keep

    # ---- range audit ----------------------------------------------------------------------
    def set_range_audit(self, on=True):
        """While on, every forward folds each layer's STORED output into a sticky per-layer record (``range_report``); results do not change."""
        self._chk(self.lib.idc_set_range_audit(self._h, 1 if on else 0))

    def range_reset(self):
        self._chk(self.lib.idc_range_reset(self._h))

    def range_report(self):
        """One dict per row of ``layer_table()``: {index, name, storage, act_exp, max_abs, n_values, n_saturated, n_tiny, n_nonfinite}.
        ``storage``: 'fp32', 'bf16', 'fp16', 'bf16x2' / 'bf16x3' / 'fp16x2' (planes whose sum is the value), or None where the layer
        stored nothing of its own (n_values == 0).  The figures are of the stored values, i.e. value * 2^act_exp."""
        rows = []
        kinds = {N.IDC_STORE_F32: "fp32", N.IDC_STORE_BF16: "bf16", N.IDC_STORE_F16: "fp16"}
        for i in range(self.lib.idc_num_layers(self._h)):
            r = N.RangeInfo()
            self._chk(self.lib.idc_range_report(self._h, i, ctypes.byref(r)))
            kind = kinds.get(r.storage)
            storage = None if kind is None else (kind if r.parts <= 1 else "%sx%d" % (kind, r.parts))
            rows.append(dict(index=i, name=r.name.decode(), storage=storage, act_exp=int(r.act_exp), max_abs=float(r.max_abs),
                             n_values=int(r.n_values), n_saturated=int(r.n_saturated), n_tiny=int(r.n_tiny),
                             n_nonfinite=int(r.n_nonfinite)))
        return rows

    def blob_bytes(self):
        return int(self.lib.idc_weights_blob_bytes(self._prec, self._flags))

    def set_weights_blob(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        self._chk(self.lib.idc_set_weights_host(self._h, blob.ctypes.data_as(ctypes.c_void_p), blob.size))

    def set_weights_device(self, dev_ptr, nbytes, copy=False, keepalive=None):
        """Adopt (or copy) a packed blob already in device memory, e.g. the torch uint8 tensor that
        received the RCCL broadcast; ``keepalive`` is held so the memory outlives the handle."""
        self._chk(self.lib.idc_set_weights_device(self._h, ctypes.c_void_p(int(dev_ptr)), int(nbytes), 1 if copy else 0))
        self._blob_keepalive = None if copy else keepalive

    def set_io_scales(self, l_div=100., ab_div=110., mask_mul=1., out_mul=110.):
        self._chk(self.lib.idc_set_io_scales(self._h, l_div, ab_div, mask_mul, out_mul))

    # ---- global hints (models/global_model/deploy_nodist.prototxt inputs) ------------------
    def set_global_hints(self, glob_ab_313_mask, s_avg_mask=None):
        """(n,314) histogram+flag rows and optional (n,2) saturation+flag rows; in effect until cleared."""
        g = _f32c(np.atleast_2d(glob_ab_313_mask))
        if g.shape[1] != 314:
            raise ValueError("glob_ab_313_mask must be (n, 314), got %s" % (g.shape,))
        sat = None if s_avg_mask is None else _f32c(np.atleast_2d(s_avg_mask), (g.shape[0], 2))
        self._chk(self.lib.idc_set_global_hints(self._h, g.shape[0], _fptr(g), _fptr(sat) if sat is not None else None))

    def clear_global_hints(self):
        self._chk(self.lib.idc_clear_global_hints(self._h))

    # ---- forward --------------------------------------------------------------------------
    def _results_will_be_replaced(self):
        cb, self.before_overwrite = self.before_overwrite, None
        if cb is not None:
            cb()
        self.forward_serial += 1
        self.l_serial += 1

    def _prep(self, L_mc, ab, mask):
        L_mc = np.asarray(L_mc)
        if L_mc.ndim == 3:                      # reference call shape: (1,X,X),(2,X,X),(1,X,X)
            L_mc, ab, mask = L_mc[None], np.asarray(ab)[None], np.asarray(mask)[None]
        n = L_mc.shape[0]
        L = self._f32in(L_mc, (n, 1, self.H, self.W))
        A = self._f32in(ab, (n, 2, self.H, self.W))
        M = self._f32in(mask, (n, 1, self.H, self.W))
        return n, L, A, M

    def _f32in(self, a, shape):
        """float32 C-contiguous view of an input.  An array that needs converting anyway (the GUI's float64 hint planes) is
        converted straight into a pooled pinned buffer, which the library then uploads in place."""
        a = np.asarray(a)
        if a.dtype == np.float32 and a.flags.c_contiguous:
            return _f32c(a, shape)
        if tuple(a.shape) != tuple(shape):
            return _f32c(a, shape)              # raises the shape error
        dst = self._pool.take(shape, np.float32)
        np.copyto(dst, a, casting="unsafe")
        return dst

    def forward(self, L_mc, ab, mask, maskcent=0.0):
        """(N,1,H,W),(N,2,H,W),(N,1,H,W) -> (N,2,H,W) float32 ab.  3-D inputs = one image."""
        n, L, A, M = self._prep(L_mc, ab, mask)
        out = self._pool.take((n, 2, self.H, self.W), np.float32)
        self._results_will_be_replaced()
        self._chk(self.lib.idc_forward(self._h, n, _fptr(L), _fptr(A), _fptr(M), float(maskcent), _fptr(out)))
        return out

    def forward_dist(self, L_mc, ab, mask, maskcent=0.0, want_dist=True):
        """Also returns the 529-bin distribution at quarter resolution (N,529,H/4,W/4); ``want_dist=False`` leaves it
        on the device (``dist_at`` / ``suggest_colors`` / ``get_dist``) and returns None in its place."""
        n, L, A, M = self._prep(L_mc, ab, mask)
        out = np.empty((n, 2, self.H, self.W), np.float32)
        dq = np.empty((n, 529, self.H // 4, self.W // 4), np.float32) if want_dist else None
        self._results_will_be_replaced()
        self._chk(self.lib.idc_forward_dist(self._h, n, _fptr(L), _fptr(A), _fptr(M), float(maskcent),
                                            _fptr(out), _fptr(dq) if want_dist else None))
        return out, dq

    # ---- click session: resident L plane + device-side hint rasterisation ------------
    def set_image_l(self, L_mc, img=0):
        """Upload L-50 of one image slot ((H,W) or (1,H,W)); stays resident for ``forward_resident``."""
        L = _f32c(np.asarray(L_mc).reshape(self.H, self.W))
        self.l_serial += 1
        self._chk(self.lib.idc_set_image_l(self._h, int(img), _fptr(L)))

    def set_image_rgb(self, rgb, img=0, l_cent=50., keep_source=False, want_rgb=True, want_lab=True):
        """Ingest uint8 RGB image(s) on the device (``idc_set_image_rgb``): rgb (h,w,3) or (n,h,w,3), any size up to 16384 a side, go to
        slots img..img+n-1 -- bilinear resize to the net size (``colorspace.resize_bilinear_u8``'s rule; none at the net size; with
        ``set_ingest_filter('antialias')`` a source larger than the net on an axis takes ``colorspace.resize_antialias``'s), rgb2lab,
        and the slot's resident plane becomes L - l_cent, as after ``set_image_l``.  Returns (rgb_net (n,H,W,3) uint8 | None,
        lab_net (n,3,H,W) float64 | None).  ``keep_source``: the source stays on the device for ``fullres_rgb``."""
        rgb = np.ascontiguousarray(np.asarray(rgb), dtype=np.uint8)
        if rgb.ndim == 3:
            rgb = rgb[None]
        if rgb.ndim != 4 or rgb.shape[3] != 3:
            raise ValueError("rgb must be (h,w,3) or (n,h,w,3) uint8, got %s" % (rgb.shape,))
        n, sh, sw = rgb.shape[:3]
        net = self._pool.take((n, self.H, self.W, 3), np.uint8) if want_rgb else None
        lab = self._pool.take((n, 3, self.H, self.W), np.float64) if want_lab else None
        vp = ctypes.c_void_p
        self.l_serial += 1
        try:
            self._chk(self.lib.idc_set_image_rgb(self._h, int(img), n, sh, sw, rgb.ctypes.data_as(vp), float(l_cent),
                                                 N.IDC_INGEST_KEEP_SOURCE if keep_source else 0,
                                                 net.ctypes.data_as(vp) if want_rgb else None, lab.ctypes.data_as(vp) if want_lab else None))
        except N.IdcError as ex:
            if ex.status not in (-1, -6):           # (a call refused for its arguments changed nothing; after any other failure the slots' sources are gone)
                for i in range(n):
                    self._src_shape.pop(int(img) + i, None)
            raise
        for i in range(n):
            if keep_source:
                self._src_shape[int(img) + i] = (sh, sw)
            else:
                self._src_shape.pop(int(img) + i, None)
        return net, lab

    def set_image_gray(self, gray, img=0, l_cent=50., keep_source=False, want_net=True, want_l=True):
        """``set_image_rgb`` for single-channel image(s) (``idc_set_image_gray``): gray (h,w) or (n,h,w), uint8 or uint16 -- the dtype is
        the format, nothing is converted -- whose sRGB value v / 255 or v / 65535 stands on all three channels.  Returns (gray_net (n,H,W) of
        the same dtype | None, l_net (n,H,W) float64 | None).  ``keep_source``: the plane stays on the device for ``fullres_rgb`` (a uint16
        plane also serves ``depth=16``) and ``fullres_ab``."""
        gray = np.asarray(gray)
        if gray.dtype not in (np.uint8, np.uint16):
            raise ValueError("gray must be uint8 or uint16, got %s" % gray.dtype)
        if gray.ndim == 2:
            gray = gray[None]
        if gray.ndim != 3:
            raise ValueError("gray must be (h,w) or (n,h,w), got %s" % (gray.shape,))
        gray = np.ascontiguousarray(gray)
        n, sh, sw = gray.shape
        net = self._pool.take((n, self.H, self.W), gray.dtype) if want_net else None
        l_net = self._pool.take((n, self.H, self.W), np.float64) if want_l else None
        vp = ctypes.c_void_p
        self.l_serial += 1
        try:
            self._chk(self.lib.idc_set_image_gray(self._h, int(img), n, sh, sw, 8 * gray.dtype.itemsize, gray.ctypes.data_as(vp), float(l_cent),
                                                  N.IDC_INGEST_KEEP_SOURCE if keep_source else 0,
                                                  net.ctypes.data_as(vp) if want_net else None, l_net.ctypes.data_as(vp) if want_l else None))
        except N.IdcError as ex:
            if ex.status not in (-1, -6):
                for i in range(n):
                    self._src_shape.pop(int(img) + i, None)
            raise
        for i in range(n):
            if keep_source:
                self._src_shape[int(img) + i] = (sh, sw)
            else:
                self._src_shape.pop(int(img) + i, None)
        return net, l_net

    def fullres_rgb(self, source="output_ab", interp="linear", l_mode="image", img=0, depth=8):
        """The full-resolution getters from the resident source of slot ``img`` (``idc_fullres_rgb``) -> (src_h, src_w, 3) uint8.
        ``depth=16`` (``idc_fullres_rgb16``): uint16, from a kept uint16 greyscale source only, l_mode 'image'.
        source: 'output_ab', 'output_ab_raw', 'input_ab' as in ``upsample_lab2rgb``, or 'no_ab' (a = b = 0); interp: 'cubic', 'linear',
        'nearest', or 'joint' (the joint bilateral upsampling of ``set_joint_upsample``, guided by the source's own L; needs l_mode 'image');
        l_mode: 'image' (L of the source pixel) or 'mask50' (50 x the nearest-upsampled hint mask).  IdcError (UNSUPPORTED)
        when the slot has no resident source: ``set_image_rgb(keep_source=True)`` first, and nothing else may have written its L plane."""
        src = {"output_ab": N.IDC_SRC_OUTPUT_AB, "output_ab_raw": N.IDC_SRC_OUTPUT_AB_RAW, "input_ab": N.IDC_SRC_INPUT_AB,
               "no_ab": N.IDC_SRC_NO_AB}[source]
        itp = _INTERP[interp]
        lm = {"image": N.IDC_L_IMAGE, "mask50": N.IDC_L_MASK50}[l_mode]
        if depth not in (8, 16):
            raise ValueError("depth must be 8 or 16, got %r" % (depth,))
        if depth == 16 and l_mode != "image":
            raise ValueError("depth=16 carries the L of the source samples: it needs l_mode 'image'")
        if depth == 16:
            call = lambda p: self.lib.idc_fullres_rgb16(self._h, int(img), src, itp, p)
        else:
            call = lambda p: self.lib.idc_fullres_rgb(self._h, int(img), src, itp, lm, p)
        shape = self._src_shape.get(int(img))
        self.l_serial += 1
        if shape is None:       # no source was kept through this object: the library says so (without a result pointer it cannot write anything)
            self._chk(call(None))
            raise N.IdcError(-7, "the source of image slot %d was not ingested through this object" % img)
        rgb = self._pool.take(shape + (3,), np.uint16 if depth == 16 else np.uint8)
        try:
            self._chk(call(rgb.ctypes.data_as(ctypes.c_void_p)))
        except N.IdcError as ex:
            if ex.status == -7 and "resident source" in str(ex):
                self._src_shape.pop(int(img), None)
            raise
        return rgb

    def fullres_ab(self, source="output_ab", interp="joint", img=0):
        """The ab map ``fullres_rgb`` hands to Lab -> RGB (``idc_fullres_ab``): the planes ``source`` names resized to the resident source's
        size by ``interp`` ('cubic', 'linear', 'nearest', 'joint') -> (2, src_h, src_w) float64.  Residency and errors as in ``fullres_rgb``."""
        src = {"output_ab": N.IDC_SRC_OUTPUT_AB, "output_ab_raw": N.IDC_SRC_OUTPUT_AB_RAW, "input_ab": N.IDC_SRC_INPUT_AB,
               "no_ab": N.IDC_SRC_NO_AB}[source]
        itp = _INTERP[interp]
        shape = self._src_shape.get(int(img))
        if shape is None:
            self._chk(self.lib.idc_fullres_ab(self._h, int(img), src, itp, None))
            raise N.IdcError(-7, "the source of image slot %d was not ingested through this object" % img)
        ab = self._pool.take((2,) + shape, np.float64)
        try:
            self._chk(self.lib.idc_fullres_ab(self._h, int(img), src, itp, ab.ctypes.data_as(ctypes.c_void_p)))
        except N.IdcError as ex:
            if ex.status == -7 and "resident source" in str(ex):
                self._src_shape.pop(int(img), None)
            raise
        return ab

    def set_joint_upsample(self, radius=2, sigma_s=1.0, sigma_r=8.0):
        """Parameters of the joint bilateral upsampling (``idc_set_joint_upsample``): taps within ``radius`` (1..4) net-size pixels, spatial
        sigma ``sigma_s`` in net-size pixels (0.25..8), range sigma ``sigma_r`` in L units (0.5..100).  The defaults are plausible values from
        the literature; nobody has measured them on trained weights.  A pipelined call keeps the values it was enqueued with."""
        self._chk(self.lib.idc_set_joint_upsample(self._h, int(radius), float(sigma_s), float(sigma_r)))

    def set_batch_upsample(self, interp="linear"):
        """How the pipelined calls bring ab to the source size with out='source' (``idc_set_batch_upsample``): 'linear' (default, the
        reference's zoom) or 'joint'.  Handle state; a batch in flight keeps what it was enqueued with."""
        if interp not in ("linear", "joint"):
            raise ValueError("set_batch_upsample takes 'linear' or 'joint', got %r" % (interp,))
        self._chk(self.lib.idc_set_batch_upsample(self._h, _INTERP[interp]))
        self._batch_upsample = interp

    def _upsample_scope(self, upsample):
        """The ``upsample=`` keyword of the streaming generators: set the state now, return what to restore (None: leave it alone)."""
        if upsample is None:
            return None
        prev = self._batch_upsample
        self.set_batch_upsample(upsample)
        return prev

    def set_ingest_filter(self, name="bilinear"):
        """How every entry point brings a source to the net size (``idc_set_ingest_filter``): 'bilinear' (default: the reference's
        point-sampled 4-tap rule) or 'antialias' (a tent filter stretched by the scale, for sources larger than the net on an axis; the host
        twin is ``colorspace.resize_antialias``).  Handle state; a batch in flight keeps what it was enqueued with."""
        if name not in _INGEST_FILTER:
            raise ValueError("set_ingest_filter takes 'bilinear' or 'antialias', got %r" % (name,))
        self._chk(self.lib.idc_set_ingest_filter(self._h, _INGEST_FILTER[name]))
        self._ingest_filter = name

    def _ingest_scope(self, ingest):
        """The ``ingest=`` keyword of the streaming generators: set the state now, return what to restore (None: leave it alone)."""
        if ingest is None:
            return None
        prev = self._ingest_filter
        self.set_ingest_filter(ingest)
        return prev

    def set_batch_output(self, format="rgb", matrix="jfif"):
        """What the pipelined calls return as images (``idc_set_batch_output``): 'rgb' (default: interleaved uint8 RGB), or the YCbCr 4:2:0
        plane block of every image, 'i420' (Y, Cb, Cr) or 'nv12' (Y, interleaved CbCr), by ``matrix`` 'jfif' (BT.601 full range, what a JPEG
        encoder takes) or 'bt709' (BT.709 limited range, video); the rule stands in ``include/ideepcolor.h`` and ``colorspace.rgb_to_ycc420``
        is its host twin.  While it is not 'rgb' every ``out_rgb`` of the ``forward_async_*`` calls is a flat uint8 array of
        ``ycc420_bytes(h, w)`` per image ((n, bytes) for ``forward_async_rgb``); ``ycc420_views`` gives the planes.  Handle state; a batch in
        flight keeps what it was enqueued with."""
        if format not in _OUT_FORMAT:
            raise ValueError("set_batch_output takes 'rgb', 'i420' or 'nv12', got %r" % (format,))
        if matrix not in _YCC_MATRIX:
            raise ValueError("set_batch_output takes the matrix 'jfif' or 'bt709', got %r" % (matrix,))
        self._chk(self.lib.idc_set_batch_output(self._h, _OUT_FORMAT[format], _YCC_MATRIX[matrix]))
        self._out_format, self._out_matrix = format, matrix

    def _output_scope(self, out_format, out_matrix):
        """The ``out_format=`` / ``out_matrix=`` keywords of the streaming generators: set the state now, return what to restore (None: leave
        it alone)."""
        if out_format is None and out_matrix is None:
            return None
        prev = (self._out_format, self._out_matrix)
        self.set_batch_output(prev[0] if out_format is None else out_format, prev[1] if out_matrix is None else out_matrix)
        return prev

    # ---- frame sequences: the temporal ab filter ---------------------------------------------
    def set_temporal_filter(self, strength=0.6, sigma=4.0, radius=1, cut=12.0):
        """The motion-adaptive recursive filter on the net-size ab map of the pipelined calls (``idc_set_temporal_filter``; the rule stands in
        ``include/ideepcolor.h``): consecutive images of the ``forward_async_rgb`` / ``_images`` / ``_eval`` / ``_dist`` / ``_gray`` /
        ``_layers`` calls are frames of one sequence, in enqueue order.  Each pixel's colour is pulled towards its filtered value in the
        previous frame with weight ``strength`` (0..0.95) where L did not change, falling off as exp(-m / 2 sigma^2) with the mean squared L
        difference m over a (2 radius + 1)^2 window (``sigma`` 0.5..100 L units, ``radius`` 0..3); a frame whose mean squared L difference
        exceeds ``cut``^2 (0 < cut <= 100; 0 = never) is a scene cut and passes unfiltered.  ``set_temporal_filter(None)`` switches it off (the
        default).  The defaults are plausible values; nobody has measured them on trained weights.  Handle state; a batch in flight keeps
        what it was enqueued with.  ``forward_async`` and the blocking calls are no sequences."""
        if strength is None or strength is False:
            prev = self._temporal or dict(strength=0.6, sigma=4.0, radius=1, cut=12.0)
            self._chk(self.lib.idc_set_temporal_filter(self._h, 0, float(prev["strength"]), float(prev["sigma"]), int(prev["radius"]),
                                                       float(prev["cut"])))
            self._temporal = None
            return
        self._chk(self.lib.idc_set_temporal_filter(self._h, 1, float(strength), float(sigma), int(radius), float(cut)))
        self._temporal = dict(strength=float(strength), sigma=float(sigma), radius=int(radius), cut=float(cut))

    def set_temporal_motion(self, search=4, penalty=0.5):
        """Block-matched motion compensation inside the temporal filter (``idc_set_temporal_motion``; the rule stands in
        ``include/ideepcolor.h``): the previous state is warped along one integer vector per 8 x 8 block of the net-size L plane before the
        filter compares and blends, so a moving surface is held against itself.  ``search`` 0..7 pixels either way, ``penalty`` 0..1e6 L^2 per
        squared pixel of displacement.  ``set_temporal_motion(None)`` switches it off (the default).  The defaults are plausible values;
        nobody has measured them on trained weights.  Handle state like the filter's; it acts only where the filter is on, and in
        ``temporal_apply``."""
        if search is None or search is False:
            prev = self.__dict__.get("_motion") or dict(search=4, penalty=0.5)
            self._chk(self.lib.idc_set_temporal_motion(self._h, 0, int(prev["search"]), float(prev["penalty"])))
            self.__dict__["_motion"] = None
            return
        self._chk(self.lib.idc_set_temporal_motion(self._h, 1, int(search), float(penalty)))
        self.__dict__["_motion"] = dict(search=int(search), penalty=float(penalty))

    def temporal_vectors(self, slot, n=None):
        """The block vectors int8 (n, H/8, W/8, 2) as (dy, dx) of the slot's last completed call, or with ``slot=-1`` of the last
        ``temporal_apply`` (``idc_temporal_vectors``).  ``n``: the call's frame count (default: the one this engine enqueued on the slot, or
        gave ``temporal_apply``).  IdcError for a slot in flight or a call that ran with the filter or motion off."""
        slot = int(slot)
        if n is None:
            n = self.__dict__.get("_apply_n") if slot < 0 else self.__dict__.get("_slot_n", {}).get(slot)
            if n is None:
                raise ValueError("temporal_vectors: this engine ran nothing on slot %d: give the call's frame count" % slot)
        v = np.zeros((self.max_batch, self.H // 8, self.W // 8, 2), np.int8)
        self._chk(self.lib.idc_temporal_vectors(self._h, slot, v.ctypes.data_as(ctypes.c_void_p)))
        return v[:int(n)].copy()

    def set_hint_tracking(self, on=True, life=0, tol=8.0):
        """Hints that follow the motion vectors (``idc_set_hint_tracking``; the rule stands in ``include/ideepcolor.h``): in the pipelined
        calls enqueued with the filter and motion on, the search runs in front of the network and every frame's hint planes are its own
        hints plus the previous frame's tracked ones, carried along the block vectors where L agrees within ``tol`` (0..100 L units) and,
        with ``life`` > 0 (up to 65535), for at most ``life`` frames.  ``set_hint_tracking(None)`` (or False) switches it off (the default).
        The defaults are plausible values; nobody has measured them on trained weights.  Handle state like the motion setting's."""
        if on is None or on is False:
            prev = self.__dict__.get("_track") or dict(life=0, tol=8.0)
            self._chk(self.lib.idc_set_hint_tracking(self._h, 0, int(prev["life"]), float(prev["tol"])))
            self.__dict__["_track"] = None
            return
        self._chk(self.lib.idc_set_hint_tracking(self._h, 1, int(life), float(tol)))
        self.__dict__["_track"] = dict(life=int(life), tol=float(tol))

    def tracked_hints(self, slot, n=None, want=("ab", "mask", "age")):
        """``(ab (n,2,H,W) float32, mask (n,H,W) float32, age (n,H,W) int32)``: the tracked hint planes the network saw in the slot's last
        completed call (``idc_tracked_hints``), copied from the device on request.  ``n``: the call's frame count (default: the one this
        engine enqueued on the slot).  ``want``: which of the three to copy; the others come back as ``None`` and cost nothing.  IdcError for
        a slot in flight or a call that ran without the filter or without tracking."""
        slot = int(slot)
        if n is None:
            n = self.__dict__.get("_slot_n", {}).get(slot)
            if n is None:
                raise ValueError("tracked_hints: this engine ran nothing on slot %d: give the call's frame count" % slot)
        want = set(want)
        if not want or not want <= {"ab", "mask", "age"}:
            raise ValueError("tracked_hints: want is a non-empty subset of ('ab', 'mask', 'age')")
        # room for max_batch frames whatever n says (the library writes ITS frame count, packed: frame f starts f planes in); untouched
        # pages of an np.empty block cost nothing, and a plane that is not wanted is neither allocated nor copied
        hw, n = self.H * self.W, int(n)
        bufs = [np.empty(self.max_batch * per * hw, dtype) if name in want else None
                for name, per, dtype in (("ab", 2, np.float32), ("mask", 1, np.float32), ("age", 1, np.int32))]
        vp = ctypes.c_void_p
        self._chk(self.lib.idc_tracked_hints(self._h, slot, *[None if b is None else b.ctypes.data_as(vp) for b in bufs]))
        shapes = ((n, 2, self.H, self.W), (n, self.H, self.W), (n, self.H, self.W))
        return tuple(None if b is None else b[:int(np.prod(shp))].reshape(shp) for b, shp in zip(bufs, shapes))

    def track_hints_apply(self, l, ab, mask, vectors=False):
        """The tracking rule alone on host arrays (``idc_track_hints_apply``): l (n,H,W) float32 the frames' L planes, ab (n,2,H,W) and mask
        (n,H,W) float32 their own hint planes, as one self-contained sequence with the engine's current motion and tracking parameters; the
        engine's sequence state is neither read nor written.  Returns ``(ab, mask, age)``, with ``vectors=True`` also the block vectors
        int8 (n,H/8,W/8,2).  Blocks; needs no weights."""
        l = np.ascontiguousarray(l, np.float32)
        ab = np.ascontiguousarray(ab, np.float32)
        mask = np.ascontiguousarray(mask, np.float32)
        if ab.ndim != 4 or tuple(ab.shape[1:]) != (2, self.H, self.W):
            raise ValueError("track_hints_apply needs ab of shape (n,2,%d,%d), got %s" % (self.H, self.W, ab.shape))
        n = ab.shape[0]
        if tuple(l.shape) == (n, 1, self.H, self.W):
            l = l.reshape(n, self.H, self.W)
        if tuple(mask.shape) == (n, 1, self.H, self.W):
            mask = mask.reshape(n, self.H, self.W)
        if tuple(l.shape) != (n, self.H, self.W) or tuple(mask.shape) != (n, self.H, self.W):
            raise ValueError("track_hints_apply needs l and mask of shape (%d,%d,%d), got %s and %s" % (n, self.H, self.W, l.shape, mask.shape))
        ab_out = np.zeros_like(ab)
        mask_out = np.zeros_like(mask)
        age = np.zeros((n, self.H, self.W), np.int32)
        v = np.zeros((max(n, 1), self.H // 8, self.W // 8, 2), np.int8) if vectors else None
        vp = ctypes.c_void_p
        self._chk(self.lib.idc_track_hints_apply(self._h, int(n), l.ctypes.data_as(vp), ab.ctypes.data_as(vp), mask.ctypes.data_as(vp),
                                                 ab_out.ctypes.data_as(vp), mask_out.ctypes.data_as(vp), age.ctypes.data_as(vp),
                                                 v.ctypes.data_as(vp) if vectors else None))
        return (ab_out, mask_out, age, v[:n]) if vectors else (ab_out, mask_out, age)

    def temporal_reset(self):
        """The next frame enqueued starts a sequence (``idc_temporal_reset``): ordered behind the batches in flight, does not block."""
        self._chk(self.lib.idc_temporal_reset(self._h))

    def temporal_info(self, slot, n=None):
        """``(cut, D)`` of the slot's last completed call (``idc_temporal_info``): per frame whether it passed unfiltered (the first frame of a
        sequence, or a scene cut) and its mean squared L difference to its predecessor.  ``n``: the call's frame count (default: the one this
        engine enqueued on the slot).  IdcError for a slot in flight or whose last call ran with the filter off."""
        if n is None:
            n = self.__dict__.get("_slot_n", {}).get(int(slot))
            if n is None:
                raise ValueError("temporal_info: this engine enqueued nothing on slot %d: give the call's frame count" % int(slot))
        cut = np.zeros(self.max_batch, np.int32)
        D = np.zeros(self.max_batch, np.float64)
        vp = ctypes.c_void_p
        self._chk(self.lib.idc_temporal_info(self._h, int(slot), cut.ctypes.data_as(vp), D.ctypes.data_as(vp)))
        return cut[:int(n)].copy(), D[:int(n)].copy()

    def temporal_apply(self, ab, l):
        """The rule alone on host arrays (``idc_temporal_apply``): ab (n,2,H,W) float32 the raw maps, l (n,H,W) float32 the frames' L planes
        (L - l_cent); reads and advances the engine's sequence state with its current parameters, whether the filter is on or not, and with
        the current ``set_temporal_motion`` setting (``temporal_vectors(-1)`` then has its vectors).  Returns ``(y, cut, D)``.  Blocks; needs
        no weights."""
        ab = np.ascontiguousarray(ab, np.float32)
        l = np.ascontiguousarray(l, np.float32)
        if ab.ndim != 4 or tuple(ab.shape[1:]) != (2, self.H, self.W):
            raise ValueError("temporal_apply needs ab of shape (n,2,%d,%d), got %s" % (self.H, self.W, ab.shape))
        n = ab.shape[0]
        if tuple(l.shape) == (n, 1, self.H, self.W):
            l = l.reshape(n, self.H, self.W)
        if tuple(l.shape) != (n, self.H, self.W):
            raise ValueError("temporal_apply needs l of shape (%d,%d,%d), got %s" % (n, self.H, self.W, l.shape))
        y = np.empty_like(ab)
        cut = np.zeros(max(n, 1), np.int32)
        D = np.zeros(max(n, 1), np.float64)
        vp = ctypes.c_void_p
        self._chk(self.lib.idc_temporal_apply(self._h, int(n), ab.ctypes.data_as(vp), l.ctypes.data_as(vp), y.ctypes.data_as(vp),
                                              cut.ctypes.data_as(vp), D.ctypes.data_as(vp)))
        self.__dict__["_apply_n"] = int(n)
        return y, cut[:n], D[:n]

    def temporal_state(self):
        """``(y_prev (2,H,W) float32, l_prev (H,W) float32, have)``: the sequence state behind everything enqueued
        (``idc_temporal_state``).  Blocks."""
        y = np.zeros((2, self.H, self.W), np.float32)
        l = np.zeros((self.H, self.W), np.float32)
        have = ctypes.c_int32(0)
        vp = ctypes.c_void_p
        self._chk(self.lib.idc_temporal_state(self._h, y.ctypes.data_as(vp), l.ctypes.data_as(vp), ctypes.cast(ctypes.byref(have), vp)))
        return y, l, bool(have.value)

    def _hold(self, slot, n, arrays):
        """What every pipelined enqueue leaves behind: the arrays the library reads / writes until the slot's wait, and the call's image
        count (``temporal_info``'s default)."""
        self._in_flight[int(slot)] = arrays
        self.__dict__.setdefault("_slot_n", {})[int(slot)] = int(n)

    def _temporal_stream(self, temporal, gen):
        """The ``temporal=`` keyword of the streaming generators around the generator ``gen``: None leaves the setting alone; True (the
        defaults), a dict of ``set_temporal_filter``'s parameters or False (off) is set, and the sequence reset, before the first batch; the
        previous setting comes back when the generator ends or its consumer walks away, behind the waits of the slots.  A dict may carry a
        key ``motion``: True (the defaults), a dict of ``set_temporal_motion``'s parameters or False (off), set and restored with the filter;
        without the key the motion setting stands as it is.  The ``motion`` dict may in turn carry a key ``track``: True (the defaults), a
        dict of ``set_hint_tracking``'s parameters or False (off), set and restored with the motion setting; without the key no
        tracking call is made."""
        if temporal is None:
            yield from gen
            return
        prev = self._temporal
        motion, prev_motion, motion_set = None, self.__dict__.get("_motion"), False
        track, prev_track, track_set = None, self.__dict__.get("_track"), False
        if temporal is True:
            self.set_temporal_filter()
        elif temporal is False:
            self.set_temporal_filter(None)
        else:
            temporal = dict(temporal)
            motion = temporal.pop("motion", None)
            self.set_temporal_filter(**temporal)
        try:
            if motion is not None and not (motion is False and prev_motion is None):       # (off and to stay off: no call)
                motion_set = True
                if motion is True:
                    self.set_temporal_motion()
                elif motion is False:
                    self.set_temporal_motion(None)
                else:
                    motion = dict(motion)
                    track = motion.pop("track", None)
                    self.set_temporal_motion(**motion)
            if track is not None and not (track is False and prev_track is None):          # (off and to stay off: no call)
                track_set = True
                if track is True:
                    self.set_hint_tracking()
                elif track is False:
                    self.set_hint_tracking(None)
                else:
                    self.set_hint_tracking(**dict(track))
            self.temporal_reset()
            yield from gen
        finally:
            try:
                gen.close()
            finally:
                try:
                    try:
                        if track_set:
                            if prev_track is None:
                                self.set_hint_tracking(None)
                            else:
                                self.set_hint_tracking(**prev_track)
                    finally:
                        if motion_set:
                            if prev_motion is None:
                                self.set_temporal_motion(None)
                            else:
                                self.set_temporal_motion(**prev_motion)
                finally:
                    if prev is None:
                        self.set_temporal_filter(None)
                    else:
                        self.set_temporal_filter(**prev)

    def _out_shapes(self, shapes, depth=8):
        """The shapes of a pipelined call's image outputs under the output format in effect: (h,w,3) each, or flat plane blocks."""
        if self._out_format == "rgb" or depth != 8:     # (16-bit RGB with a YCbCr format: the library refuses the call)
            return shapes
        return [(ycc420_bytes(s[0], s[1]),) for s in shapes]

    def _own_image(self, r, hw):
        """A generator's copy of one image result: the (h,w,3) array, or the planes of its block (``YCC420`` / ``NV12``) over one copy."""
        if r.ndim != 1:
            return np.array(r)
        return ycc420_views(np.array(r), hw[0], hw[1], self._out_format)

    def ycc420_bytes(self, h, w):
        return ycc420_bytes(h, w)

    def fullres_ycc(self, source="output_ab", interp="linear", l_mode="image", img=0, format="i420", matrix="jfif"):
        """``fullres_rgb`` whose image arrives as its YCbCr 4:2:0 plane block (``idc_fullres_ycc``): a ``YCC420`` / ``NV12`` tuple of views
        into one uint8 buffer, at the kept source's size.  Every source, interp ('joint' included) and l_mode of ``fullres_rgb``; RGB and grey
        kept sources."""
        if format not in ("i420", "nv12") or matrix not in _YCC_MATRIX:
            raise ValueError("fullres_ycc takes format 'i420' | 'nv12' and matrix 'jfif' | 'bt709'")
        shape = self._src_shape.get(int(img))
        if shape is None:
            raise N.IdcError(-7, "the source of image slot %d was not ingested through this object" % img)
        buf = np.empty(ycc420_bytes(shape[0], shape[1]), np.uint8)
        src = {"output_ab": N.IDC_SRC_OUTPUT_AB, "output_ab_raw": N.IDC_SRC_OUTPUT_AB_RAW, "input_ab": N.IDC_SRC_INPUT_AB,
               "no_ab": N.IDC_SRC_NO_AB}[source]
        lm = {"image": N.IDC_L_IMAGE, "mask50": N.IDC_L_MASK50}[l_mode]
        self.l_serial += 1
        self._chk(self.lib.idc_fullres_ycc(self._h, int(img), src, _INTERP[interp], lm, _OUT_FORMAT[format], _YCC_MATRIX[matrix],
                                           buf.ctypes.data_as(ctypes.c_void_p)))
        return ycc420_views(buf, shape[0], shape[1], format)

    def rgb_to_ycc420(self, images, format="i420", matrix="jfif"):
        """The conversion alone on the device (``idc_rgb_to_ycc420``): ``images`` is one (h,w,3) uint8 array or a list of them, each of its
        own size; a ``YCC420`` / ``NV12`` tuple per image comes back (one tuple for one array).  Blocking; needs no weights."""
        if format not in ("i420", "nv12") or matrix not in _YCC_MATRIX:
            raise ValueError("rgb_to_ycc420 takes format 'i420' | 'nv12' and matrix 'jfif' | 'bt709'")
        single = isinstance(images, np.ndarray) and images.ndim == 3
        arrs = [np.ascontiguousarray(a, np.uint8) for a in ([images] if single else images)]
        for a in arrs:
            if a.ndim != 3 or a.shape[2] != 3 or a.size == 0:
                raise ValueError("rgb_to_ycc420 needs (h,w,3) uint8 arrays")
        n = len(arrs)
        table = (N.RefImage * max(n, 1))()
        outs = (ctypes.c_void_p * max(n, 1))()
        bufs = [np.empty(ycc420_bytes(a.shape[0], a.shape[1]), np.uint8) for a in arrs]
        for i, (a, b) in enumerate(zip(arrs, bufs)):
            table[i].rgb, table[i].h, table[i].w = a.ctypes.data, a.shape[0], a.shape[1]
            outs[i] = b.ctypes.data
        self._chk(self.lib.idc_rgb_to_ycc420(self._h, n, table, _OUT_FORMAT[format], _YCC_MATRIX[matrix], outs))
        res = [ycc420_views(b, a.shape[0], a.shape[1], format) for a, b in zip(arrs, bufs)]
        return res[0] if single else res

    # ---- colour picker (data/lab_gamut.py): no weights needed, nothing resident is read or written ---------
    def gamut_map(self, L, gamut_size=110, D=1, want_pts=False):
        """``abGrid(gamut_size, D).update_gamut(L[k])`` for every L in one launch (``idc_gamut_map``).  L: a scalar or n values.
        Returns (masked_rgb (n,A,B,3) uint8, mask (n,A,B) bool[, pts_rgb (n,A,B,3) uint8]) with A = B = ceil(2 gamut_size / D) + 1;
        row i is a = -gamut_size + i D, column j is b."""
        L = np.ascontiguousarray(np.atleast_1d(np.asarray(L, np.float64)).reshape(-1))
        n, g, d = int(L.shape[0]), int(gamut_size), int(D)
        A = -(-2 * g // d) + 1 if g >= 1 and 1 <= d <= g else 1     # (the library refuses such arguments before it writes anything)
        masked = np.empty((n, A, A, 3), np.uint8)
        mask = np.empty((n, A, A), np.uint8)
        pts = np.empty((n, A, A, 3), np.uint8) if want_pts else None
        vp = ctypes.c_void_p
        self._chk(self.lib.idc_gamut_map(self._h, n, L.ctypes.data_as(vp), g, d, pts.ctypes.data_as(vp) if want_pts else None,
                                         masked.ctypes.data_as(vp), mask.ctypes.data_as(vp)))
        return (masked, mask.view(np.bool_), pts) if want_pts else (masked, mask.view(np.bool_))

    def snap_colors(self, L, rgb, want_lab=False, want_iters=False):
        """``snap_ab(L[k], rgb[k])`` for n colours in one launch (``idc_snap_colors``).  L: a scalar or (n,); rgb: (3,) or (n,3) uint8.
        Returns rgb_out (n,3) uint8 [return_type 'rgb'], then lab_out (n,3) float64 [return_type 'lab'] and iters (n,) int32 (loop
        rounds run, 1..20) when asked for."""
        L = np.ascontiguousarray(np.atleast_1d(np.asarray(L, np.float64)).reshape(-1))
        rgb = np.ascontiguousarray(np.asarray(rgb), dtype=np.uint8).reshape(-1, 3)
        n = int(L.shape[0])
        if rgb.shape[0] != n:
            raise ValueError("%d L values for %d colours" % (n, rgb.shape[0]))
        out = np.empty((n, 3), np.uint8)
        lab = np.empty((n, 3), np.float64) if want_lab else None
        its = np.empty((n,), np.int32) if want_iters else None
        vp = ctypes.c_void_p
        self._chk(self.lib.idc_snap_colors(self._h, n, L.ctypes.data_as(vp), rgb.ctypes.data_as(vp), out.ctypes.data_as(vp),
                                           lab.ctypes.data_as(vp) if want_lab else None, its.ctypes.data_as(vp) if want_iters else None))
        ret = (out,) + ((lab,) if want_lab else ()) + ((its,) if want_iters else ())
        return ret[0] if len(ret) == 1 else ret

    def set_hints(self, hints, mode="ab", img=0, mask_value=1.0):
        """Rasterise a hint list on the device.  hints: rows (y0, x0, y1, x1, c0, c1[, c2]) -- inclusive rectangle and
        its (a, b) [mode 'ab', the notebook's put_point] or uint8 (r, g, b) [mode 'rgb', UIControl.get_input +
        rgb2lab]; later rows paint over earlier ones."""
        rows = [tuple(r) for r in hints]
        arr = (N.Hint * max(len(rows), 1))()
        for i, r in enumerate(rows):
            arr[i].y0, arr[i].x0, arr[i].y1, arr[i].x1 = int(r[0]), int(r[1]), int(r[2]), int(r[3])
            arr[i].c0, arr[i].c1, arr[i].c2 = float(r[4]), float(r[5]), float(r[6]) if len(r) > 6 else 0.0
        self._chk(self.lib.idc_set_hints(self._h, int(img), len(rows), arr, {"ab": N.IDC_HINT_AB, "rgb": N.IDC_HINT_RGB}[mode],
                                         float(mask_value)))

    def set_hint_layer(self, rgba, hints=(), mode="rgb", img=0, mask_value=1.0, alpha_min=128, cover=0):
        """``set_hints`` with a painted layer under the rectangles (``idc_set_hints_layer``): ``rgba`` (lh,lw,4) uint8, straight alpha, of any
        size -- it is stretched over the image.  A layer pixel is painted iff A >= ``alpha_min``; a net cell no rectangle covers is hinted
        iff its footprint holds a painted pixel and 255 * painted >= ``cover`` * pixels, with the mean Lab colour of the painted ones.
        Returns the number of cells the layer hinted.  ``rgba=None``: ``set_hints`` exactly (returns 0)."""
        rows = [tuple(r) for r in hints]
        arr = (N.Hint * max(len(rows), 1))()
        for i, r in enumerate(rows):
            arr[i].y0, arr[i].x0, arr[i].y1, arr[i].x1 = int(r[0]), int(r[1]), int(r[2]), int(r[3])
            arr[i].c0, arr[i].c1, arr[i].c2 = float(r[4]), float(r[5]), float(r[6]) if len(r) > 6 else 0.0
        layer, a = None, None
        if rgba is not None:
            a = _layer_array("set_hint_layer", rgba)
            layer = N.HintLayer(a.ctypes.data, a.shape[0], a.shape[1])
        cells = ctypes.c_int32(0)
        self._chk(self.lib.idc_set_hints_layer(self._h, int(img), len(rows), arr, {"ab": N.IDC_HINT_AB, "rgb": N.IDC_HINT_RGB}[mode],
                                               float(mask_value), ctypes.byref(layer) if layer is not None else None, int(alpha_min), int(cover),
                                               ctypes.cast(ctypes.byref(cells), ctypes.c_void_p)))
        return int(cells.value)

    def reveal_hints(self, rects, img=0, mask_value=1.0):
        """``set_hints`` in 'ab' mode with every colour revealed on the device (``idc_reveal_hints``): rects are rows (y0, x0, y1, x1[, ...]),
        and a rectangle's colour is the mean ground-truth ab of slot ``img``'s kept source (``set_image_rgb(keep_source=True)``) under it -- the
        paper's simulated user.  Returns the revealed colours (k,2) float32, (0, 0) for a rectangle wholly outside the image."""
        rows = [tuple(r) for r in rects]
        arr = (N.Hint * max(len(rows), 1))()
        for i, r in enumerate(rows):
            arr[i].y0, arr[i].x0, arr[i].y1, arr[i].x1 = int(r[0]), int(r[1]), int(r[2]), int(r[3])
        colours = np.zeros((len(rows), 2), np.float32)
        self._chk(self.lib.idc_reveal_hints(self._h, int(img), len(rows), arr, float(mask_value), _fptr(colours)))
        return colours

    def hint_planes(self, img=0):
        """(ab (2,H,W), mask (1,H,W)) float32 copies of the resident hint planes of one slot."""
        ab = np.empty((2, self.H, self.W), np.float32)
        mask = np.empty((1, self.H, self.W), np.float32)
        self._chk(self.lib.idc_get_hint_planes(self._h, int(img), _fptr(ab), _fptr(mask)))
        return ab, mask

    def forward_resident(self, n=1, maskcent=0.0, l_cent=50.0, want_ab=True, want_rgb=True, want_lab=True):
        """Forward of slots 0..n-1 from the resident planes -> (out_ab | None, rgb | None, lab_q | None)."""
        out = np.empty((n, 2, self.H, self.W), np.float32) if want_ab else None
        rgb = np.empty((n, self.H, self.W, 3), np.uint8) if want_rgb else None
        labq = np.empty((n, 3, self.H, self.W), np.float64) if (want_rgb and want_lab) else None
        self._results_will_be_replaced()
        self._chk(self.lib.idc_forward_resident(self._h, int(n), float(maskcent), float(l_cent), _fptr(out) if want_ab else None,
                                                rgb.ctypes.data_as(ctypes.c_void_p) if want_rgb else None,
                                                labq.ctypes.data_as(ctypes.c_void_p) if labq is not None else None))
        return out, rgb, labq

    # ---- colour suggestions on the resident distribution ---------------------------
    def dist_bins(self):
        return int(self.lib.idc_dist_bins(self._h))

    def keep_dist(self, on=True):
        self._chk(self.lib.idc_keep_dist(self._h, 1 if on else 0))

    def dist_at(self, y, x, img=0):
        """The predicted distribution (529 or 313 probabilities, float32) of pixel (y, x) from the last forward."""
        pdf = np.empty(self.dist_bins(), np.float32)
        self._chk(self.lib.idc_dist_at(self._h, int(img), int(y), int(x), _fptr(pdf)))
        return pdf

    def get_dist(self, n=1):
        """The whole resident distribution: (n,529,H/4,W/4) or (n,313,H,W) float32."""
        shape = (n, 313, self.H, self.W) if self.dist_bins() == 313 else (n, 529, self.H // 4, self.W // 4)
        d = np.empty(shape, np.float32)
        self._chk(self.lib.idc_get_dist(self._h, int(n), _fptr(d)))
        return d

    def suggest_colors(self, y, x, centres, K=5, N_draws=25000, seed=0, img=0, want_counts=False):
        """``get_ab_reccs`` on the device: (centres (K,2) f64, conf (K,) f64[, counts (B,) uint32]) ordered by occupancy."""
        B = self.dist_bins()
        c = _f32c(centres, (B, 2))
        oc, of = np.empty((K, 2), np.float64), np.empty(K, np.float64)
        cnt = np.empty(B, np.uint32) if want_counts else None
        vp = ctypes.c_void_p
        self._chk(self.lib.idc_suggest_colors(self._h, int(img), int(y), int(x), int(K), int(N_draws), int(seed) & 0xFFFFFFFF, _fptr(c),
                                              oc.ctypes.data_as(vp), of.ctypes.data_as(vp),
                                              cnt.ctypes.data_as(vp) if want_counts else None))
        return (oc, of, cnt) if want_counts else (oc, of)

    def _dist_grid(self):
        return (self.H, self.W) if self.dist_bins() == 313 else (self.H // 4, self.W // 4)

    def dist_peaks(self, n=1, P=8, radius=2, skip_hints=False):
        """Where the model is least sure (``idc_dist_peaks``): per image of the resident distribution the P cells of smallest ``dist_entropy``
        (MINUS the entropy), chosen greedily -- ties to the lowest cell index, every cell closer than ``radius`` (Chebyshev, in cells) to a
        chosen one leaves -- as net coordinates of the cell centres.  ``skip_hints``: cells under a non-zero pixel of the resident hint mask
        (``hint_planes``) are not candidates.  Returns (peaks (n,P,2) int32 rows (y, x), peak_ent (n,P) float32); once the candidates run out
        the rows are (-1, -1) and 0."""
        peaks = np.empty((n, P, 2), np.int32)
        pent = np.empty((n, P), np.float32)
        vp = ctypes.c_void_p
        self._chk(self.lib.idc_dist_peaks(self._h, int(n), int(P), int(radius), N.IDC_PEAKS_SKIP_HINTS if skip_hints else 0,
                                          peaks.ctypes.data_as(vp), pent.ctypes.data_as(vp)))
        return peaks, pent

    def suggest_colors_batch(self, queries, centres, K=5, N_draws=25000):
        """``suggest_colors`` for many pixels in one launch (``idc_suggest_colors_batch``): ``queries`` rows (img, y, x, seed) -> (centres
        (nq,K,2) f64, conf (nq,K) f64), row q bit for bit ``suggest_colors(y, x, centres, K, N_draws, seed, img)``.  A row with
        (y, x) == (-1, -1) is empty and gives zeros."""
        arr = dist_queries(queries)
        nq = len(arr) if arr is not None else 0
        c = _f32c(centres, (self.dist_bins(), 2))
        oc, of = np.empty((nq, K, 2), np.float64), np.empty((nq, K), np.float64)
        vp = ctypes.c_void_p
        self._chk(self.lib.idc_suggest_colors_batch(self._h, nq, arr, int(K), int(N_draws), _fptr(c), oc.ctypes.data_as(vp), of.ctypes.data_as(vp)))
        return oc, of

    def dist_entropy(self, n=1):
        """``sum_q p log p`` (the reference's ``compute_entropy``: MINUS the entropy) of the resident distribution of images
        0..n-1, on the device: (n,Hd,Wd) float32, Hd x Wd = H/4 x W/4 (529 head) or H x W (313 head).  p == 0 bins add 0."""
        ent = np.empty((n,) + self._dist_grid(), np.float32)
        self._chk(self.lib.idc_dist_entropy(self._h, int(n), _fptr(ent)))
        return ent

    def dist_decode(self, centres, n=1, mode='mode', gamma=1.0, want_conf=False):
        """A colour map of the resident distribution, on the device: ab (n,2,Hd,Wd) float32 [, conf (n,Hd,Wd) = p_max].
        ``mode='mode'``: the centre of the most probable bin; ``mode='mean'``: the mean of ``centres`` (B,2) under weights
        ``(p / p_max) ** gamma`` (1 = plain mean; 2.6 / S = the 313 net's ``pred_ab`` without its bias)."""
        hd, wd = self._dist_grid()
        c = _f32c(centres, (self.dist_bins(), 2))
        ab = np.empty((n, 2, hd, wd), np.float32)
        conf = np.empty((n, hd, wd), np.float32) if want_conf else None
        self._chk(self.lib.idc_dist_decode(self._h, int(n), {"mode": N.IDC_DECODE_MODE, "mean": N.IDC_DECODE_MEAN}[mode], float(gamma),
                                           _fptr(c), _fptr(ab), _fptr(conf) if want_conf else None))
        return (ab, conf) if want_conf else ab

    def dist_score(self, centres, n=1, nn=1, sigma=5.0, ranks=(1, 5), want_maps=False):
        """How much probability the head put on the colours the pixels really have (``idc_dist_score``): the resident distribution of images
        0..n-1 against the ground-truth images ``set_image_rgb(..., keep_source=True)`` left in slots 0..n-1, on the device.  Per cell the
        truth is the mean ab under it (``reveal_hints``' colour), soft-encoded over its ``nn`` nearest ``centres`` (B,2) with a Gaussian of
        ``sigma`` (the training layers' NNEncode; nn = 1: the nearest bin alone), scored by cross-entropy and by the rank of the nearest bin.
        Returns a ``DistScore``: ``xent`` sums, ``hits`` per threshold of ``ranks``, and the per-cell maps with ``want_maps``."""
        c = _f32c(centres, (self.dist_bins(), 2))
        spec = score_spec(nn, sigma, ranks)
        res, out = score_buffers(int(n), self._dist_grid(), spec.n_ranks, want_maps, lambda shape, dtype: np.empty(shape, dtype))
        self._chk(self.lib.idc_dist_score(self._h, int(n), ctypes.byref(spec), _fptr(c), ctypes.byref(out)))
        return res

    def global_histogram(self, rgb, centres, want_sat=True):
        """Global statistics of reference image(s) (the reference's global_stats.prototxt): rgb (n,H,W,3) or (H,W,3)
        uint8, centres (313,2) -> (hist (n,313) float32 summing to 1, s_avg (n,) mean HSV saturation or None)."""
        rgb = np.ascontiguousarray(np.asarray(rgb), dtype=np.uint8)
        if rgb.ndim == 3:
            rgb = rgb[None]
        n = rgb.shape[0]
        if rgb.shape != (n, self.H, self.W, 3):
            raise ValueError("rgb must be (n,%d,%d,3), got %s" % (self.H, self.W, rgb.shape))
        c = _f32c(centres, (313, 2))
        hist = np.empty((n, 313), np.float32)
        sat = np.empty(n, np.float32) if want_sat else None
        self._chk(self.lib.idc_global_histogram(self._h, n, rgb.ctypes.data_as(ctypes.c_void_p), _fptr(c), _fptr(hist),
                                                _fptr(sat) if want_sat else None))
        return hist, sat

    def global_stats_rgb(self, refs, centres, want_sat=True):
        """``global_histogram`` for reference photographs as they come (``idc_global_stats_rgb``): refs is a list of (h,w,3) uint8 arrays of
        individual sizes (or one array), each resized on the device by ``set_image_rgb``'s rule; centres (313,2) -> (hist (m,313) float32
        summing to 1, s_avg (m,) or None).  A reference's figures do not depend on the others in the call."""
        if isinstance(refs, np.ndarray) and refs.ndim == 3:
            refs = [refs]
        arr, keep = ref_images(refs)
        m = len(keep)
        c = _f32c(centres, (313, 2))
        hist = np.empty((max(m, 1), 313), np.float32)
        sat = np.empty(max(m, 1), np.float32) if want_sat else None
        self._chk(self.lib.idc_global_stats_rgb(self._h, m, arr, _fptr(c), _fptr(hist), _fptr(sat) if want_sat else None))
        return hist[:m], (sat[:m] if want_sat else None)

    def set_global_refs(self, refs, centres, ref_index=None, img=0, hist_flag=1.0, saturation=False):
        """Install references as the global hints of image slots img .. img+n-1 on the device (``idc_set_global_refs``): the rows
        ``set_global_hints`` would be given -- histogram, ``hist_flag`` and, with ``saturation``, (mean saturation, 1) -- without the histogram
        visiting the host.  ``ref_index`` (n,): which of ``refs`` each image takes, -1 = none (a zero row); None = one reference per image in
        order.  Other slots keep their rows; in effect until replaced or cleared."""
        if isinstance(refs, np.ndarray) and refs.ndim == 3:
            refs = [refs]
        arr, keep = ref_images(refs)
        m = len(keep)
        n = m if ref_index is None else len(ref_index)
        idx = _ref_index(ref_index, n)
        c = _f32c(centres, (313, 2))
        self._chk(self.lib.idc_set_global_refs(self._h, int(img), int(n), m, arr, idx.ctypes.data_as(ctypes.c_void_p) if idx is not None else None,
                                               _fptr(c), float(hist_flag), N.IDC_REF_SATURATION if saturation else 0))

    def lab2rgb(self, L, ab, want_lab=True):
        """Device colour step: L (n,1,H,W) in [0,100], ab (n,2,H,W) -> (rgb (n,H,W,3) uint8, lab_q (n,3,H,W) f64 or None)
        = ``lab2rgb_transpose`` + the rgb->Lab refresh of the reference (colorize_image.py:20-36,196-198)."""
        L = np.asarray(L)
        if L.ndim == 3:
            L, ab = L[None], np.asarray(ab)[None]
        n = L.shape[0]
        Lc, Ac = _f32c(L, (n, 1, self.H, self.W)), _f32c(ab, (n, 2, self.H, self.W))
        rgb = np.empty((n, self.H, self.W, 3), np.uint8)
        labq = np.empty((n, 3, self.H, self.W), np.float64) if want_lab else None
        self._results_will_be_replaced()
        self._chk(self.lib.idc_lab2rgb(self._h, n, _fptr(Lc), _fptr(Ac), rgb.ctypes.data_as(ctypes.c_void_p),
                                       labq.ctypes.data_as(ctypes.c_void_p) if want_lab else None))
        return rgb, labq

    def forward_rgb(self, L_mc, ab, mask, maskcent=0.0, l_cent=50.0, want_lab=True):
        """forward + the colour step on the device: (out_ab (n,2,H,W) f32, rgb (n,H,W,3) u8, lab_q (n,3,H,W) f64 | None)."""
        n, L, A, M = self._prep(L_mc, ab, mask)
        out = self._pool.take((n, 2, self.H, self.W), np.float32)       # pinned: the library copies device -> result in place
        rgb = self._pool.take((n, self.H, self.W, 3), np.uint8)
        labq = self._pool.take((n, 3, self.H, self.W), np.float64) if want_lab else None
        self._results_will_be_replaced()
        self._chk(self.lib.idc_forward_rgb(self._h, n, _fptr(L), _fptr(A), _fptr(M), float(maskcent), float(l_cent), _fptr(out),
                                           rgb.ctypes.data_as(ctypes.c_void_p),
                                           labq.ctypes.data_as(ctypes.c_void_p) if want_lab else None))
        return out, rgb, labq

    def forward_rgb_lazy(self, L_mc, ab, mask, maskcent=0.0, l_cent=50.0):
        """forward + the colour step on the device, only the uint8 image copied back: rgb (n,H,W,3).  The ab map and the refreshed Lab
        stay resident; ``fetch_outputs`` brings them over when somebody reads them (2.0 of the 2.2 MB a 256x256 click sends back).
        ``L_mc=None``: the L plane ``set_image_l`` left in the handle (one image; it is constant between the clicks on that image)."""
        if L_mc is None:
            A = np.asarray(ab)
            A = self._f32in(A[None] if A.ndim == 3 else A, (1, 2, self.H, self.W))
            M = np.asarray(mask)
            M = self._f32in(M[None] if M.ndim == 3 else M, (1, 1, self.H, self.W))
            n, Lp = 1, None
        else:
            n, L, A, M = self._prep(L_mc, ab, mask)
            Lp = _fptr(L)
        rgb = self._pool.take((n, self.H, self.W, 3), np.uint8)
        self._results_will_be_replaced()
        self._chk(self.lib.idc_forward_rgb_lazy(self._h, n, Lp, _fptr(A), _fptr(M), float(maskcent), float(l_cent),
                                                rgb.ctypes.data_as(ctypes.c_void_p)))
        return rgb

    def fetch_outputs(self, n=1, want_ab=True, want_lab=True):
        """(out_ab (n,2,H,W) f32 | None, lab_q (n,3,H,W) f64 | None) of the last forward, from the device."""
        out = self._pool.take((n, 2, self.H, self.W), np.float32) if want_ab else None
        labq = self._pool.take((n, 3, self.H, self.W), np.float64) if want_lab else None
        self._chk(self.lib.idc_fetch_outputs(self._h, int(n), _fptr(out) if want_ab else None,
                                             labq.ctypes.data_as(ctypes.c_void_p) if want_lab else None))
        return out, labq

    def forward_dist313(self, L_mc, ab, mask, maskcent=0.0, want_dist=True):
        """313-bin head of the Caffe distribution net: returns (out_ab regression, pred_ab soft-decode (N,2,H,W),
        dist_S (N,313,H,W) full-resolution softmax(S*logits) or None)."""
        n, L, A, M = self._prep(L_mc, ab, mask)
        out = np.empty((n, 2, self.H, self.W), np.float32)
        pred = np.empty((n, 2, self.H, self.W), np.float32)
        dist = np.empty((n, 313, self.H, self.W), np.float32) if want_dist else None
        self._results_will_be_replaced()
        self._chk(self.lib.idc_forward_dist313(self._h, n, _fptr(L), _fptr(A), _fptr(M), float(maskcent), _fptr(out),
                                               _fptr(pred), _fptr(dist) if want_dist else None))
        return out, pred, dist

    def set_dist_temperature(self, S):
        self._chk(self.lib.idc_set_dist_temperature(self._h, float(S)))

    def forward_device(self, n, d_L, d_ab, d_mask, d_out, maskcent=0.0, sync=False):
        """Device-pointer form (ints / objects with ``data_ptr()`` / numpy arrays over PINNED host memory from
        ``pinned_empty``, which the device reads and writes in place); enqueued on the handle stream."""
        def p(x):
            if hasattr(x, "data_ptr"):
                return ctypes.c_void_p(int(x.data_ptr()))
            if isinstance(x, np.ndarray):               # pinned host memory (pinned_empty): zero-copy, see idc_pipeline_times' note
                return ctypes.c_void_p(int(x.ctypes.data))
            return ctypes.c_void_p(int(x))
        self._results_will_be_replaced()
        self._chk(self.lib.idc_forward_device(self._h, int(n), p(d_L), p(d_ab), p(d_mask), float(maskcent),
                                              p(d_out), 1 if sync else 0))

    def sync(self):
        self._chk(self.lib.idc_sync(self._h))

    # ---- stream ordering against a caller stream (e.g. torch.cuda.current_stream().cuda_stream) --------------
    def stream_wait(self, caller_stream):
        """Work enqueued on this handle after the call waits for everything already enqueued on ``caller_stream``."""
        self._chk(self.lib.idc_stream_wait(self._h, ctypes.c_void_p(int(caller_stream))))

    def stream_signal(self, caller_stream):
        """Work enqueued on ``caller_stream`` after the call waits for everything this handle has enqueued."""
        self._chk(self.lib.idc_stream_signal(self._h, ctypes.c_void_p(int(caller_stream))))

    # ---- overlapped host transfers: two slots ----------------------------------------------
    def pinned_empty(self, shape, dtype=np.float32):
        """numpy array over pinned host memory (``idc_alloc_host``): ``forward_async`` transfers it in place and
        ``forward_device`` may be given it directly (zero-copy: the memory is mapped into the device's address space).
        The memory lives as long as any array that views it (the base buffer frees it when collected), not as long as
        this engine."""
        shape = tuple(int(x) for x in shape)
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        raw = np.asarray(_PinnedBuffer(self.lib, nbytes))           # uint8 view; .base keeps the owner alive
        return raw[:nbytes].view(dtype).reshape(shape)

    def forward_async(self, slot, L_mc, ab, mask, out, maskcent=0.0):
        """Enqueue one batch on pipeline slot 0/1 (float32 C-contiguous arrays, used in place -- keep them alive and
        untouched until ``wait(slot)``); ``out`` (n,2,H,W) float32 receives the result."""
        n = L_mc.shape[0]
        for a, shp in ((L_mc, (n, 1, self.H, self.W)), (ab, (n, 2, self.H, self.W)), (mask, (n, 1, self.H, self.W)), (out, (n, 2, self.H, self.W))):
            if a.dtype != np.float32 or not a.flags.c_contiguous or tuple(a.shape) != shp:
                raise ValueError("forward_async needs float32 C-contiguous arrays of shape %s" % (shp,))
        self._results_will_be_replaced()
        self._chk(self.lib.idc_forward_async(self._h, int(slot), int(n), _fptr(L_mc), _fptr(ab), _fptr(mask), float(maskcent), _fptr(out)))

    def forward_async_rgb(self, slot, rgb, hints, out_rgb, out_ab=None, mode="ab", mask_value=1.0, maskcent=0.0, l_cent=50.0, out="net",
                          refs=None, ref_index=None, centres=None, hist_flag=1.0, saturation=False):
        """Enqueue one batch of uint8 images on pipeline slot 0/1 (``idc_forward_async_rgb``): rgb (n,h,w,3) uint8 C-contiguous, any size up
        to 16384 a side, is ingested as by ``set_image_rgb``; ``hints`` is a list of n per-image hint lists (rows as in ``set_hints``, ``None``
        or [] for an image without) or ``None``.  ``out_rgb`` uint8 receives the colourised images: (n,H,W,3) with out='net' (what
        ``forward_rgb`` returns), (n,h,w,3) with out='source' (``fullres_rgb('output_ab', 'linear', 'image')`` of every image); ``out_ab``
        (n,2,H,W) float32 or None the network's ab map.  The arrays are used in place: leave them untouched until ``wait(slot)`` (the engine
        holds a reference to each until then, so a caller that drops its own cannot have the result written into freed memory).
        ``refs`` (a ``global_hints`` engine): a list of m reference photographs, (h,w,3) uint8 each of its own size, whose statistics become
        the batch's global hints on the device (``idc_forward_async_rgb_ref``; an empty list: no image has one); ``ref_index`` (n,) names
        each image's reference, -1 = none, None = one per image in order; ``centres`` (313,2), ``hist_flag`` and ``saturation`` as in
        ``set_global_refs``.  The slot keeps these global inputs to itself: ``set_global_hints`` / ``set_global_refs`` are neither read nor
        changed.  ``refs=None``: the plain call, which reads the handle's global hints."""
        if not isinstance(rgb, np.ndarray) or rgb.dtype != np.uint8 or rgb.ndim != 4 or rgb.shape[3] != 3 or not rgb.flags.c_contiguous:
            raise ValueError("forward_async_rgb needs a uint8 C-contiguous (n,h,w,3) array")
        n, sh, sw = rgb.shape[:3]
        flags = {"net": 0, "source": N.IDC_BATCH_OUT_SOURCE}[out]
        shp = (n, sh, sw, 3) if flags else (n, self.H, self.W, 3)
        if self._out_format != "rgb":            # the plane blocks back to back (set_batch_output)
            shp = (n, ycc420_bytes(shp[1], shp[2]))
        if not isinstance(out_rgb, np.ndarray) or out_rgb.dtype != np.uint8 or not out_rgb.flags.c_contiguous or tuple(out_rgb.shape) != shp:
            raise ValueError("forward_async_rgb needs a uint8 C-contiguous out_rgb of shape %s" % (shp,))
        if out_ab is not None and (out_ab.dtype != np.float32 or not out_ab.flags.c_contiguous or tuple(out_ab.shape) != (n, 2, self.H, self.W)):
            raise ValueError("forward_async_rgb needs a float32 C-contiguous out_ab of shape %s" % ((n, 2, self.H, self.W),))
        offsets, arr = flatten_hints(hints, n)
        vp = ctypes.c_void_p
        head = (self._h, int(slot), int(n), int(sh), int(sw), rgb.ctypes.data_as(vp),
                offsets.ctypes.data_as(vp) if offsets is not None else None, ctypes.cast(arr, vp) if arr is not None else None,
                {"ab": N.IDC_HINT_AB, "rgb": N.IDC_HINT_RGB}[mode], float(mask_value), float(maskcent), float(l_cent), flags)
        tail = (out_rgb.ctypes.data_as(vp), out_ab.ctypes.data_as(vp) if out_ab is not None else None)
        if refs is None:
            self._chk(self.lib.idc_forward_async_rgb(*(head + tail)))
        else:
            (m, rarr, idx, c, hist_flag, rflags), keep = _ref_args(refs, ref_index, centres, hist_flag, saturation, n)
            self._chk(self.lib.idc_forward_async_rgb_ref(*(head + (m, rarr, idx.ctypes.data_as(vp) if idx is not None else None,
                                                                   _fptr(c) if c is not None else None, hist_flag, rflags) + tail)))
        self._hold(slot, n, (rgb, out_rgb, out_ab))      # the library reads / writes them until the slot's wait

    def colorize_stream(self, batches, out="net", upsample=None, ingest=None, out_format=None, out_matrix=None, temporal=None, **kw):
        """Generator: colourise a stream of uint8 batches with both pipeline slots busy.  ``batches`` yields (rgb (n,h,w,3) uint8, hints) items
        (``hints`` as in ``forward_async_rgb``; n and the source size may change from item to item); each item's (n,H,W,3) [out='net'] or
        (n,h,w,3) [out='source'] uint8 result is yielded in input order, as an array of the caller's own (copied out of the pinned buffer the
        device wrote).  Item k runs on slot k % 2 while item k - 1 computes; its buffers come from the pinned pool.  ``kw``: mode, mask_value,
        maskcent, l_cent of ``forward_async_rgb``.
        An item may be (rgb, hints, refs) on a ``global_hints`` engine: ``refs`` is a list of n entries, each ``None`` or an (h,w,3) uint8
        reference photograph for that image.  The same array OBJECT given for several images of an item is uploaded once (``dedupe_refs``);
        ``kw`` then also carries centres (needed), hist_flag and saturation.  A two-entry item makes the plain call.
        ``upsample``: 'linear' or 'joint' -- ``set_batch_upsample`` before the first batch, the previous setting back when the generator
        ends or is abandoned; None (default) leaves the setting alone.
        ``ingest``: 'bilinear' or 'antialias' -- ``set_ingest_filter`` with the same scope.
        ``out_format`` / ``out_matrix``: 'rgb' | 'i420' | 'nv12' and 'jfif' | 'bt709' -- ``set_batch_output`` with the same scope.  With a
        YCbCr format an item's result is a list of n ``YCC420`` / ``NV12`` tuples, one per image (``ycc420_views``), not one array.
        ``temporal``: True (the defaults), a dict of ``set_temporal_filter``'s parameters, or False -- the images of the stream are the frames
        of ONE sequence: the filter is set and the sequence reset before the first batch, the previous setting back with the same scope."""
        def submit(slot, group, first):
            item = group[0]
            rgb, hints = item[0], item[1]
            rgb = np.asarray(rgb)
            if rgb.dtype != np.uint8 or rgb.ndim != 4 or rgb.shape[3] != 3:
                raise ValueError("colorize_stream needs uint8 (n,h,w,3) batches, got %s %s" % (rgb.dtype, rgb.shape))
            src = self._pool.take(rgb.shape, np.uint8)
            np.copyto(src, rgb)
            dims = rgb.shape[1:3] if out == "source" else (self.H, self.W)
            dst = self._pool.take((rgb.shape[0],) + ((dims[0], dims[1], 3) if self._out_format == "rgb" else (ycc420_bytes(*dims),)), np.uint8)
            if len(item) > 2:
                uniq, index = dedupe_refs(item[2], rgb.shape[0])
                self.forward_async_rgb(slot, src, hints, dst, out=out, refs=uniq, ref_index=index, **kw)
            else:
                self.forward_async_rgb(slot, src, hints, dst, out=out, **kw)
            return dst, src, dims

        def finish(state):
            if state[0].ndim != 2:
                return [np.array(state[0])]
            return [[self._own_image(r, state[2]) for r in state[0]]]

        # a group of one: the items are whole batches, checked in submit, behind the yield of the slot's older result
        yield from self._temporal_stream(temporal, self._two_slot_stream(batches, 1, upsample, lambda item: item, submit, finish, ingest=ingest,
                                                                         output=(out_format, out_matrix)))

    def _two_slot_stream(self, items, batch, upsample, parse, submit, finish, key=None, ingest=None, output=(None, None)):
        """The generator behind ``colorize_stream``, ``colorize_images`` and their relatives: ``parse(item)`` every item as it arrives, group
        ``batch`` of them (default ``max_batch``; the last group may be shorter), ``submit(slot, group, first_index)`` group k on slot k % 2
        once that slot's older batch is finished -- ``first_index`` is the stream index of the group's first item; what it returns (results
        and whatever must stay alive: pinned pool memory) is kept until ``wait(slot)`` has returned -- and yield everything in
        ``finish(state)`` of each batch in input order.  ``upsample`` and ``ingest`` as in ``colorize_stream``.  A consumer that stops early: both slots are
        waited for, so nothing stays in flight on buffers about to be recycled, then the upsample and ingest settings go back.
        ``output``: the generator's (out_format, out_matrix), ``set_batch_output`` with the same scope.
        ``key`` (of a parsed item): an item whose key differs from its group's closes that group, as a full batch does."""
        batch = self._group_size(batch)
        pending = [None, None]                      # per slot: submit's state of the batch in flight

        def groups():
            group = []
            for item in items:
                parsed = parse(item)
                if key is not None and group and key(parsed) != key(group[0]):
                    yield group
                    group = []
                group.append(parsed)
                if len(group) == batch:
                    yield group
                    group = []
            if group:
                yield group

        def drain(slot):
            self.wait(slot)
            state, pending[slot] = pending[slot], None
            return finish(state)

        k, first = 0, 0
        restore = self._upsample_scope(upsample)
        try:
            restore_ingest = self._ingest_scope(ingest)
        except Exception:
            if restore is not None:
                self.set_batch_upsample(restore)
            raise
        try:
            restore_output = self._output_scope(*output)
        except Exception:
            try:
                if restore is not None:
                    self.set_batch_upsample(restore)
            finally:
                if restore_ingest is not None:
                    self.set_ingest_filter(restore_ingest)
            raise
        try:
            for group in groups():
                if pending[k & 1] is not None:
                    yield from drain(k & 1)
                pending[k & 1] = submit(k & 1, group, first)
                k, first = k + 1, first + len(group)
            for slot in (k & 1, (k + 1) & 1):       # the older batch first
                if pending[slot] is not None:
                    yield from drain(slot)
        finally:
            try:
                for slot in (0, 1):
                    if pending[slot] is not None:
                        pending[slot] = None
                        self.wait(slot)
            finally:
                try:
                    if restore is not None:
                        self.set_batch_upsample(restore)
                finally:
                    try:
                        if restore_ingest is not None:
                            self.set_ingest_filter(restore_ingest)
                    finally:
                        if restore_output is not None:
                            self.set_batch_output(*restore_output)

    def _group_size(self, batch):
        batch = self.max_batch if batch is None else int(batch)
        if batch != 1 and not 1 <= batch <= self.max_batch:       # (one image fits every engine)
            raise ValueError("batch %d outside 1..%d" % (batch, self.max_batch))
        return batch

    def _pinned_sources(self, group):
        """The images of a parsed group (``_image_item``), copied into one pinned pool block."""
        srcs = self._pinned_slices([g[0].shape for g in group])
        for s, g in zip(srcs, group):
            np.copyto(s, g[0])
        return srcs


    def _pinned_slices(self, shapes):
        """One pinned pool block (a multiple of 64 KiB, so that blocks of ragged batches recycle) sliced into uint8 arrays of ``shapes``."""
        sizes = [int(np.prod(s)) for s in shapes]
        block = self._pool.take((-(-max(sum(sizes), 1) // 65536) * 65536,), np.uint8)
        ends = np.cumsum(sizes)
        return [block[e - z:e].reshape(s) for e, z, s in zip(ends, sizes, shapes)]

    def forward_async_images(self, slot, images, hints, out_rgb=None, out_ab=None, mode="ab", mask_value=1.0, maskcent=0.0, l_cent=50.0,
                             out="net", refs=None, ref_index=None, centres=None, hist_flag=1.0, saturation=False):
        """``forward_async_rgb`` for images of individual sizes (``idc_forward_async_images``): ``images`` is a list of n C-contiguous (h,w,3)
        uint8 arrays, each of its own size; ``out_rgb`` a list of n uint8 arrays, (H,W,3) each with out='net', images[i].shape with
        out='source', or ``None``: they are taken from the pinned pool.  Returns the list of outputs, valid after ``wait(slot)``.  Image i's
        result is bit for bit what ``forward_async_rgb`` gives for it alone.  Every other argument as in ``forward_async_rgb``; pinned and
        pageable arrays may be mixed within a call, and the engine holds a reference to each until ``wait(slot)``."""
        return self._enqueue_images("forward_async_images", slot, images, hints, out_rgb, out_ab, mode, mask_value, maskcent, l_cent, out,
                                    refs, ref_index, centres, hist_flag, saturation)

    def forward_async_eval(self, slot, images, hints, out_rgb=None, out_ab=None, mode="reveal", mask_value=1.0, maskcent=0.0, l_cent=50.0,
                           out="net", refs=None, ref_index=None, centres=None, hist_flag=1.0, saturation=False, want_rgb=False):
        """``forward_async_images`` that also scores the batch on the device (``idc_forward_async_eval``): returns ``(sse, hint_colours,
        out_rgb)``, valid after ``wait(slot)``.  ``sse`` (n,3) uint64 is the exact sum of squared uint8 differences per image and channel
        between the result and the ground truth -- the images themselves at the net size (out='net') or at their own (out='source').  mode
        'reveal' (default): ``hints`` holds per-image lists of rectangles (y0, x0, y1, x1[, ...]) whose colours the device takes from the
        image (the mean ab under the rectangle), and ``hint_colours`` (all rectangles, 2) float32 reports them; modes 'ab' / 'rgb' score a
        given hint list and ``hint_colours`` is None.  No image leaves the device unless ``want_rgb`` or ``out_rgb`` asks for it (``out_rgb``
        is then the list ``forward_async_images`` returns, else None).  Array validation and every other argument as there."""
        return self._enqueue_images("forward_async_eval", slot, images, hints, out_rgb, out_ab, mode, mask_value, maskcent, l_cent, out,
                                    refs, ref_index, centres, hist_flag, saturation, evaluate=True, want_rgb=want_rgb or out_rgb is not None)

    def forward_async_dist(self, slot, images, hints, out_rgb=None, out_ab=None, mode="ab", mask_value=1.0, maskcent=0.0, l_cent=50.0,
                           out="net", refs=None, ref_index=None, ref_centres=None, hist_flag=1.0, saturation=False, want_rgb=False,
                           want_sse=False, peaks=8, radius=2, skip_hints=False, queries=None, K=5, N_draws=25000, seed=0, centres=None,
                           want_entropy=False, score=None):
        """``forward_async_eval`` on an engine with a distribution head that also runs the head and reads it on the device
        (``idc_forward_async_dist``).  Images, hints (mode 'ab', 'rgb' or 'reveal'), outputs and reference arguments as there
        (``ref_centres``: the (313,2) centres of the reference statistics); ``want_sse`` asks for the score.  Behind the network the slot
        computes the entropy map (``want_entropy``), ``peaks`` uncertainty peaks per image (``dist_peaks``; ``skip_hints`` reads this batch's
        own hint masks; 0: none) and colour suggestions (``suggest_colors_batch``) for ``queries``: rows (img, y, x[, seed]) with img the index
        in this batch and seed defaulting to ``seed`` + row, or ``"peaks"``: at every peak, straight from the device buffer, peak (i, k) with
        seed ``seed + i * peaks + k``.  ``centres`` (B,2): the bin centres, needed with queries.  Returns a ``DistBatch`` whose arrays
        (sse, hint_colours, out_rgb, peaks (n,P,2), peak_ent (n,P), entropy (n,Hd,Wd), sugg_centres (Q,K,2), sugg_conf (Q,K); ``None`` where not
        asked for) are valid after ``wait(slot)``.  Afterwards the resident distribution (``get_dist``, ``dist_at`` ...) is this batch's.
        ``score``: ``None``, or a dict of ``dist_score``'s arguments (centres, nn, sigma, ranks, want_maps) -- the batch's distribution is then
        also scored against the batch's own images behind the other taps (``idc_forward_async_dist_score``) and ``DistBatch.score`` is the
        ``DistScore``; with peaks=0, no queries and no entropy map only the score runs."""
        taps = dict(peaks=int(peaks), radius=int(radius), skip_hints=bool(skip_hints), queries=queries, K=int(K), N=int(N_draws), seed=int(seed),
                    centres=centres, want_entropy=bool(want_entropy), want_sse=bool(want_sse))
        if score is not None:
            taps["score"] = dict(score)
        return self._enqueue_images("forward_async_dist", slot, images, hints, out_rgb, out_ab, mode, mask_value, maskcent, l_cent, out,
                                    refs, ref_index, ref_centres, hist_flag, saturation, evaluate=True, want_rgb=want_rgb or out_rgb is not None,
                                    taps=taps)

    def _enqueue_images(self, who, slot, images, hints, out_rgb, out_ab, mode, mask_value, maskcent, l_cent, out, refs, ref_index, centres,
                        hist_flag, saturation, evaluate=False, want_rgb=True, taps=None):
        images = list(images)
        n = len(images)
        for a in images:
            if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or not a.flags.c_contiguous or a.size == 0:
                raise ValueError("%s needs uint8 C-contiguous (h,w,3) arrays" % who)
        flags = {"net": 0, "source": N.IDC_BATCH_OUT_SOURCE}[out]
        shapes = self._out_shapes([tuple(a.shape) if flags else (self.H, self.W, 3) for a in images])
        if want_rgb:
            if out_rgb is None:
                out_rgb = self._pinned_slices(shapes)
            out_rgb = list(out_rgb)
            if len(out_rgb) != n:
                raise ValueError("%s needs %d outputs, got %d" % (who, n, len(out_rgb)))
            for o, shp in zip(out_rgb, shapes):
                if not isinstance(o, np.ndarray) or o.dtype != np.uint8 or not o.flags.c_contiguous or tuple(o.shape) != shp:
                    raise ValueError("%s needs a uint8 C-contiguous out_rgb of shape %s" % (who, shp))
        if out_ab is not None and (out_ab.dtype != np.float32 or not out_ab.flags.c_contiguous or tuple(out_ab.shape) != (n, 2, self.H, self.W)):
            raise ValueError("%s needs a float32 C-contiguous out_ab of shape %s" % (who, (n, 2, self.H, self.W)))
        modes = {"ab": N.IDC_HINT_AB, "rgb": N.IDC_HINT_RGB}
        if evaluate:
            modes["reveal"] = N.IDC_HINT_REVEAL
            if mode == "reveal" and hints is not None:     # rectangles only: the colours are the device's to find
                hints = [None if h is None else [tuple(r[:4]) + (0.0, 0.0) for r in h] for h in hints]
        offsets, arr = flatten_hints(hints, n)
        vp = ctypes.c_void_p
        table = (N.RefImage * max(n, 1))()
        outs = (vp * max(n, 1))() if want_rgb else None
        for i, a in enumerate(images):
            table[i].rgb, table[i].h, table[i].w = a.ctypes.data, a.shape[0], a.shape[1]
            if want_rgb:
                outs[i] = out_rgb[i].ctypes.data
        block = None
        if refs is not None:
            (m, rarr, idx, c, hist_flag, rflags), keep = _ref_args(refs, ref_index, centres, hist_flag, saturation, n)
            block = N.BatchRefs(m, rarr, idx.ctypes.data if idx is not None else None, c.ctypes.data if c is not None else None, hist_flag, rflags)
        args = (self._h, int(slot), int(n), table, offsets.ctypes.data_as(vp) if offsets is not None else None,
                ctypes.cast(arr, vp) if arr is not None else None, modes[mode], float(mask_value),
                float(maskcent), float(l_cent), flags, ctypes.byref(block) if block is not None else None, outs,
                out_ab.ctypes.data_as(vp) if out_ab is not None else None)
        if not evaluate:
            self._chk(self.lib.idc_forward_async_images(*args))
            self._hold(slot, len(images), (images, out_rgb, out_ab))    # the library reads / writes them until the slot's wait
            return out_rgb
        sse = self._pool.take((n, 3), np.uint64) if taps is None or taps["want_sse"] else None
        colours = None
        if mode == "reveal":
            colours = self._pool.take((int(offsets[-1]) if offsets is not None else 0, 2), np.float32)
        args = args + (sse.ctypes.data_as(vp) if sse is not None else None, colours.ctypes.data_as(vp) if colours is not None and colours.size else None)
        if taps is None:
            self._chk(self.lib.idc_forward_async_eval(*args))
            self._hold(slot, len(images), (images, out_rgb, out_ab, sse, colours))
            return sse, colours, (out_rgb if want_rgb else None)
        # the distribution taps: every result in pinned pool memory, written in place by the copy-out stream
        P, hd_wd = taps["peaks"], self._dist_grid()
        res = DistBatch()
        res.sse, res.hint_colours, res.out_rgb, res.out_ab = sse, colours, (out_rgb if want_rgb else None), out_ab
        t = N.DistTaps()
        t.n_peaks, t.radius = P, taps["radius"]
        t.flags = (N.IDC_PEAKS_SKIP_HINTS if taps["skip_hints"] else 0) | (N.IDC_TAPS_SUGGEST_AT_PEAKS if isinstance(taps["queries"], str) else 0)
        if isinstance(taps["queries"], str) and taps["queries"] != "peaks":
            raise ValueError("queries is a list of rows, None or 'peaks'")
        if P > 0:
            res.peaks, res.peak_ent = self._pool.take((n, P, 2), np.int32), self._pool.take((n, P), np.float32)
            t.peaks, t.peak_ent = res.peaks.ctypes.data, res.peak_ent.ctypes.data
        if taps["want_entropy"]:
            res.entropy = self._pool.take((n,) + hd_wd, np.float32)
            t.entropy = res.entropy.ctypes.data
        qarr = None if isinstance(taps["queries"], str) else dist_queries(taps["queries"], taps["seed"])
        Q = n * P if isinstance(taps["queries"], str) else (len(qarr) if qarr is not None else 0)
        c = None
        if Q > 0:
            t.n_queries = 0 if qarr is None else len(qarr)
            if qarr is not None:
                t.queries = qarr
            t.K, t.N, t.seed = taps["K"], taps["N"], taps["seed"] & 0xFFFFFFFF
            c = _f32c(taps["centres"], (self.dist_bins(), 2)) if taps["centres"] is not None else None
            t.centres = c.ctypes.data if c is not None else None
            res.sugg_centres, res.sugg_conf = self._pool.take((Q, t.K, 2), np.float64), self._pool.take((Q, t.K), np.float64)
            t.sugg_centres, t.sugg_conf = res.sugg_centres.ctypes.data, res.sugg_conf.ctypes.data
        sc = taps.get("score")
        if sc is None:
            self._chk(self.lib.idc_forward_async_dist(*(args + (ctypes.byref(t),))))
        else:
            unknown = set(sc) - {"centres", "nn", "sigma", "ranks", "want_maps"}
            if unknown or "centres" not in sc:
                raise ValueError("score is a dict of centres[, nn, sigma, ranks, want_maps]; got %s" % sorted(sc))
            sc_c = _f32c(sc["centres"], (self.dist_bins(), 2))
            spec = score_spec(sc.get("nn", 1), sc.get("sigma", 5.0), sc.get("ranks", (1, 5)))
            res.score, sout = score_buffers(n, hd_wd, spec.n_ranks, bool(sc.get("want_maps", False)), self._pool.take)
            only_score = P == 0 and Q == 0 and not taps["want_entropy"]
            self._chk(self.lib.idc_forward_async_dist_score(*(args + (None if only_score else ctypes.byref(t), ctypes.byref(spec), _fptr(sc_c),
                                                                      ctypes.byref(sout)))))
        self._hold(slot, len(images), (images, out_rgb, out_ab, res))
        return res

    def forward_async_gray(self, slot, images, hints, out_rgb=None, out_ab=None, mode="ab", mask_value=1.0, maskcent=0.0, l_cent=50.0,
                           out="net", depth=8, refs=None, ref_index=None, centres=None, hist_flag=1.0, saturation=False, want_rgb=True,
                           peaks=0, radius=2, skip_hints=False, queries=None, K=5, N_draws=25000, seed=0, bin_centres=None):
        """``forward_async_images`` for greyscale planes (``idc_forward_async_gray``): ``images`` is a list of n C-contiguous (h,w) arrays, all
        uint8 or all uint16 (the dtype is the format; one format per call), each of its own size.  ``out_rgb``: a list of n arrays, (H,W,3)
        uint8 with out='net', images[i].shape + (3,) with out='source' -- uint8, or uint16 with ``depth=16`` (uint16 planes and out='source'
        only) -- or ``None``: taken from the pinned pool.  Without taps it returns the list of outputs.  ``peaks`` > 0 or ``queries`` (an
        engine with a distribution head): ``forward_async_dist``'s peaks and suggestions (``bin_centres`` (B,2): the bin centres) without its
        score and revealed colours; it then returns a ``DistBatch``, and ``want_rgb=False`` colourises nothing for the caller.  Everything is
        valid after ``wait(slot)``.  Hints, references and the other arguments as in ``forward_async_images``; mode 'reveal' does not exist
        here: a grey source has no colour to reveal."""
        images = list(images)
        n = len(images)
        dtypes = set(a.dtype for a in images if isinstance(a, np.ndarray))
        if len(dtypes) != 1 or not dtypes <= {np.dtype(np.uint8), np.dtype(np.uint16)}:
            raise ValueError("forward_async_gray needs (h,w) arrays that are all uint8 or all uint16")
        for a in images:
            if not isinstance(a, np.ndarray) or a.ndim != 2 or not a.flags.c_contiguous or a.size == 0:
                raise ValueError("forward_async_gray needs C-contiguous (h,w) arrays")
        bits = 8 * images[0].dtype.itemsize
        if depth not in (8, 16):
            raise ValueError("depth must be 8 or 16, got %r" % (depth,))
        if depth == 16 and (bits != 16 or out != "source"):
            raise ValueError("depth=16 needs uint16 planes and out='source'")
        flags = {"net": 0, "source": N.IDC_BATCH_OUT_SOURCE}[out] | (N.IDC_BATCH_OUT_RGB16 if depth == 16 else 0)
        odt = np.uint16 if depth == 16 else np.uint8
        shapes = self._out_shapes([tuple(a.shape) + (3,) if flags else (self.H, self.W, 3) for a in images], depth)
        if want_rgb:
            if out_rgb is None:
                nbytes = [int(np.prod(s)) * (depth // 8) for s in shapes]           # (each output starts on an even byte of the block)
                out_rgb = [o[:b].view(odt).reshape(s) for o, b, s in zip(self._pinned_slices([(b + 1) // 2 * 2 for b in nbytes]), nbytes, shapes)]
            out_rgb = list(out_rgb)
            if len(out_rgb) != n:
                raise ValueError("forward_async_gray needs %d outputs, got %d" % (n, len(out_rgb)))
            for o, shp in zip(out_rgb, shapes):
                if not isinstance(o, np.ndarray) or o.dtype != odt or not o.flags.c_contiguous or tuple(o.shape) != shp:
                    raise ValueError("forward_async_gray needs a %s C-contiguous out_rgb of shape %s" % (np.dtype(odt).name, shp))
        else:
            out_rgb = None
        if out_ab is not None and (out_ab.dtype != np.float32 or not out_ab.flags.c_contiguous or tuple(out_ab.shape) != (n, 2, self.H, self.W)):
            raise ValueError("forward_async_gray needs a float32 C-contiguous out_ab of shape %s" % ((n, 2, self.H, self.W),))
        offsets, arr = flatten_hints(hints, n)
        vp = ctypes.c_void_p
        table = (N.GrayImage * max(n, 1))()
        outs = (vp * max(n, 1))() if want_rgb else None
        for i, a in enumerate(images):
            table[i].pix, table[i].h, table[i].w = a.ctypes.data, a.shape[0], a.shape[1]
            if want_rgb:
                outs[i] = out_rgb[i].ctypes.data
        block, keep = None, None
        if refs is not None:
            (m, rarr, idx, c, hist_flag, rflags), keep = _ref_args(refs, ref_index, centres, hist_flag, saturation, n)
            block = N.BatchRefs(m, rarr, idx.ctypes.data if idx is not None else None, c.ctypes.data if c is not None else None, hist_flag, rflags)
        res, t, held = None, None, None
        P = int(peaks)
        if P > 0 or queries is not None:
            if isinstance(queries, str) and queries != "peaks":
                raise ValueError("queries is a list of rows, None or 'peaks'")
            at_peaks = isinstance(queries, str)
            res, t = DistBatch(), N.DistTaps()
            res.out_rgb, res.out_ab = out_rgb, out_ab
            t.n_peaks, t.radius = P, int(radius)
            t.flags = (N.IDC_PEAKS_SKIP_HINTS if skip_hints else 0) | (N.IDC_TAPS_SUGGEST_AT_PEAKS if at_peaks else 0)
            if P > 0:
                res.peaks, res.peak_ent = self._pool.take((n, P, 2), np.int32), self._pool.take((n, P), np.float32)
                t.peaks, t.peak_ent = res.peaks.ctypes.data, res.peak_ent.ctypes.data
            qarr = None if at_peaks else dist_queries(queries, int(seed))
            Q = n * P if at_peaks else (len(qarr) if qarr is not None else 0)
            if Q > 0:
                t.n_queries = 0 if qarr is None else len(qarr)
                if qarr is not None:
                    t.queries = qarr
                t.K, t.N, t.seed = int(K), int(N_draws), int(seed) & 0xFFFFFFFF
                held = _f32c(bin_centres, (self.dist_bins(), 2)) if bin_centres is not None else None
                t.centres = held.ctypes.data if held is not None else None
                res.sugg_centres, res.sugg_conf = self._pool.take((Q, t.K, 2), np.float64), self._pool.take((Q, t.K), np.float64)
                t.sugg_centres, t.sugg_conf = res.sugg_centres.ctypes.data, res.sugg_conf.ctypes.data
        self._chk(self.lib.idc_forward_async_gray(self._h, int(slot), int(n), bits, table, offsets.ctypes.data_as(vp) if offsets is not None else None,
                                                  ctypes.cast(arr, vp) if arr is not None else None, {"ab": N.IDC_HINT_AB, "rgb": N.IDC_HINT_RGB}[mode],
                                                  float(mask_value), float(maskcent), float(l_cent), flags,
                                                  ctypes.byref(block) if block is not None else None, outs,
                                                  out_ab.ctypes.data_as(vp) if out_ab is not None else None, ctypes.byref(t) if t is not None else None))
        self._hold(slot, len(images), (images, out_rgb, out_ab, res, held, keep))      # the library reads / writes them until the slot's wait
        return res if res is not None else out_rgb

    def forward_async_layers(self, slot, images, layers, hints, out_rgb=None, out_ab=None, mode="rgb", mask_value=1.0, maskcent=0.0,
                             l_cent=50.0, out="net", depth=8, alpha_min=128, cover=0, refs=None, ref_index=None, centres=None, hist_flag=1.0,
                             saturation=False):
        """``forward_async_images`` / ``forward_async_gray`` with a painted hint layer per image (``idc_forward_async_layers``).  ``images``:
        n C-contiguous arrays, all (h,w,3) uint8 RGB, or all (h,w) uint8 or all (h,w) uint16 planes -- ``ndim`` and dtype tell which.
        ``layers``: n entries, each ``None`` or an (lh,lw,4) uint8 RGBA array of any size (``set_hint_layer``'s rule, one ``alpha_min`` and
        ``cover`` per call), or ``None``: the call is the layer-free one.  Returns ``(out_rgb, cells)``, valid after ``wait(slot)``: the list
        of outputs as those calls give it (``depth=16``: uint16, for uint16 planes with out='source') and the (n,) int32 counts of the cells
        each layer hinted (``None`` without ``layers``).  Hints (note the default mode 'rgb'), references and the rest as in those calls."""
        who = "forward_async_layers"
        images = list(images)
        n = len(images)
        kinds = set((a.ndim, a.dtype) for a in images if isinstance(a, np.ndarray))
        if len(kinds) != 1 or len(images) == 0 or not all(isinstance(a, np.ndarray) for a in images):
            raise ValueError("%s needs arrays of one kind: (h,w,3) uint8, (h,w) uint8 or (h,w) uint16" % who)
        ndim, dt = next(iter(kinds))
        if (ndim, dt) == (3, np.dtype(np.uint8)):
            bits = 0
        elif ndim == 2 and dt in (np.dtype(np.uint8), np.dtype(np.uint16)):
            bits = 8 * dt.itemsize
        else:
            raise ValueError("%s needs arrays of one kind: (h,w,3) uint8, (h,w) uint8 or (h,w) uint16" % who)
        for a in images:
            if not a.flags.c_contiguous or a.size == 0 or (bits == 0 and a.shape[2] != 3):
                raise ValueError("%s needs C-contiguous, non-empty (h,w,3) or (h,w) arrays" % who)
        if depth not in (8, 16):
            raise ValueError("depth must be 8 or 16, got %r" % (depth,))
        if depth == 16 and (bits != 16 or out != "source"):
            raise ValueError("depth=16 needs uint16 planes and out='source'")
        flags = {"net": 0, "source": N.IDC_BATCH_OUT_SOURCE}[out] | (N.IDC_BATCH_OUT_RGB16 if depth == 16 else 0)
        odt = np.uint16 if depth == 16 else np.uint8
        shapes = self._out_shapes([tuple(a.shape[:2]) + (3,) if flags else (self.H, self.W, 3) for a in images], depth)
        if out_rgb is None:
            nbytes = [int(np.prod(s)) * (depth // 8) for s in shapes]           # (each output starts on an even byte of the block)
            out_rgb = [o[:b].view(odt).reshape(s) for o, b, s in zip(self._pinned_slices([(b + 1) // 2 * 2 for b in nbytes]), nbytes, shapes)]
        out_rgb = list(out_rgb)
        if len(out_rgb) != n:
            raise ValueError("%s needs %d outputs, got %d" % (who, n, len(out_rgb)))
        for o, shp in zip(out_rgb, shapes):
            if not isinstance(o, np.ndarray) or o.dtype != odt or not o.flags.c_contiguous or tuple(o.shape) != shp:
                raise ValueError("%s needs a %s C-contiguous out_rgb of shape %s" % (who, np.dtype(odt).name, shp))
        if out_ab is not None and (out_ab.dtype != np.float32 or not out_ab.flags.c_contiguous or tuple(out_ab.shape) != (n, 2, self.H, self.W)):
            raise ValueError("%s needs a float32 C-contiguous out_ab of shape %s" % (who, (n, 2, self.H, self.W)))
        offsets, arr = flatten_hints(hints, n)
        vp = ctypes.c_void_p
        table = (N.GrayImage * n)() if bits else (N.RefImage * n)()
        outs = (vp * n)()
        for i, a in enumerate(images):
            if bits:
                table[i].pix = a.ctypes.data
            else:
                table[i].rgb = a.ctypes.data
            table[i].h, table[i].w = a.shape[0], a.shape[1]
            outs[i] = out_rgb[i].ctypes.data
        lblock, ltab, larrs, cells = None, None, None, None
        if layers is not None:
            layers = list(layers)
            if len(layers) != n:
                raise ValueError("%s: %d layers for %d images" % (who, len(layers), n))
            larrs = [None if l is None else _layer_array(who, l) for l in layers]
            ltab = (N.HintLayer * n)()
            for i, l in enumerate(larrs):
                if l is not None:
                    ltab[i].rgba, ltab[i].h, ltab[i].w = l.ctypes.data, l.shape[0], l.shape[1]
            cells = self._pool.take((n,), np.int32)
            lblock = N.BatchLayers(ltab, int(alpha_min), int(cover), cells.ctypes.data)
        block, keep = None, None
        if refs is not None:
            (m, rarr, idx, c, hist_flag, rflags), keep = _ref_args(refs, ref_index, centres, hist_flag, saturation, n)
            block = N.BatchRefs(m, rarr, idx.ctypes.data if idx is not None else None, c.ctypes.data if c is not None else None, hist_flag, rflags)
        self._chk(self.lib.idc_forward_async_layers(self._h, int(slot), int(n), bits, ctypes.cast(table, vp),
                                                    ctypes.byref(lblock) if lblock is not None else None,
                                                    offsets.ctypes.data_as(vp) if offsets is not None else None,
                                                    ctypes.cast(arr, vp) if arr is not None else None, {"ab": N.IDC_HINT_AB, "rgb": N.IDC_HINT_RGB}[mode],
                                                    float(mask_value), float(maskcent), float(l_cent), flags,
                                                    ctypes.byref(block) if block is not None else None, outs,
                                                    out_ab.ctypes.data_as(vp) if out_ab is not None else None))
        self._hold(slot, len(images), (images, larrs, out_rgb, out_ab, cells, keep))   # the library reads / writes them until the slot's wait
        return out_rgb, cells

    def colorize_layers(self, items, batch=None, out="source", depth=8, upsample=None, ingest=None, out_format=None, out_matrix=None, temporal=None,
                        **kw):
        """Generator: ``colorize_images`` / ``colorize_gray`` for images with painted hint layers (``forward_async_layers``).  An item is
        ``(image, layer_or_None, hints)``: image (h,w,3) uint8, or (h,w) uint8 or uint16; layer (lh,lw,4) uint8 RGBA of any size or ``None``;
        hints that image's rectangle list or ``None``.  Grouping, slot alternation and order as in ``colorize_images``; a change of image kind
        closes the group as a full batch does.  ``(rgb, cells)`` is yielded per image: the colourised image as those generators yield it and
        the number of cells its layer hinted (0 without a layer).  ``kw``: mode, mask_value, alpha_min, cover, maskcent, l_cent, ...;
        ``upsample``, ``ingest``, ``out_format`` and ``out_matrix`` as in ``colorize_stream``: with a YCbCr format the image is a ``YCC420`` /
        ``NV12`` tuple.  ``temporal``: as in ``colorize_stream``."""
        if depth not in (8, 16) or (depth == 16 and out != "source"):
            raise ValueError("depth must be 8, or 16 with out='source'")

        def parse(item):
            item = tuple(item)
            if len(item) != 3:
                raise ValueError("colorize_layers needs items (image, layer_or_None, hints)")
            img = np.asarray(item[0])
            if img.ndim == 3:
                img = _image_item("colorize_layers", (img,), False)[0]
            else:
                img = _gray_item("colorize_layers", (img,), False)[0]
            if depth == 16 and img.dtype != np.uint16:
                raise ValueError("colorize_layers: depth=16 needs uint16 items, got %s" % img.dtype)
            return img, (None if item[1] is None else _layer_array("colorize_layers", item[1])), item[2]

        def submit(slot, group, first):
            srcs = self._pinned_planes(group) if group[0][0].ndim == 2 else self._pinned_sources(group)
            lays = [g[1] for g in group]
            held = self._pinned_slices([l.shape for l in lays if l is not None])
            pinned = []
            for l in lays:
                if l is None:
                    pinned.append(None)
                else:
                    pinned.append(held[sum(1 for q in pinned if q is not None)])
                    np.copyto(pinned[-1], l)
            res = self.forward_async_layers(slot, srcs, pinned, [g[2] for g in group], out=out, depth=depth, **kw)
            return res, srcs, pinned

        def finish(state):
            (rgbs, cells), srcs, _ = state
            return [(self._own_image(r, self._out_dims(s, out)), int(c)) for r, s, c in zip(rgbs, srcs, cells)]

        yield from self._temporal_stream(temporal, self._two_slot_stream(items, batch, upsample, parse, submit, finish,
                                                                         key=lambda g: (g[0].ndim, g[0].dtype), ingest=ingest,
                                                                         output=(out_format, out_matrix)))

    def _out_dims(self, src, out):
        """(h, w) of the result of the image whose source array is ``src``."""
        return tuple(src.shape[:2]) if out == "source" else (self.H, self.W)

    def _pinned_planes(self, group):
        """The planes of a parsed group (``_gray_item``), copied into one pinned pool block; each starts on an even byte."""
        planes = [g[0] for g in group]
        blocks = self._pinned_slices([(p.nbytes + 1) // 2 * 2 for p in planes])
        srcs = [b[:p.nbytes].view(p.dtype).reshape(p.shape) for b, p in zip(blocks, planes)]
        for s, p in zip(srcs, planes):
            np.copyto(s, p)
        return srcs

    def colorize_gray(self, items, batch=None, out="source", depth=8, upsample=None, ingest=None, out_format=None, out_matrix=None, temporal=None,
                      **kw):
        """Generator: ``colorize_images`` for greyscale planes (``forward_async_gray``).  An item is ``gray``, ``(gray, hints)`` or
        ``(gray, hints, ref)``: gray (h,w) uint8 or uint16.  Grouping, slot alternation and order as in ``colorize_images``, and a change of
        dtype closes the group as a full batch does: a call carries one format.  One array per image is yielded: (h,w,3) [out='source'] or
        (H,W,3) [out='net'], uint8, or uint16 with ``depth=16`` (uint16 items and out='source' only).  ``upsample``, ``out_format`` and ``out_matrix``: as in ``colorize_stream`` (a YCbCr format yields a ``YCC420`` /
        ``NV12`` tuple per image and needs depth 8).  ``temporal``: as in ``colorize_stream``."""
        if depth not in (8, 16) or (depth == 16 and out != "source"):
            raise ValueError("depth must be 8, or 16 with out='source'")

        def parse(item):
            g = _gray_item("colorize_gray", item, True)
            if depth == 16 and g[0].dtype != np.uint16:
                raise ValueError("colorize_gray: depth=16 needs uint16 items, got %s" % g[0].dtype)
            return g

        def submit(slot, group, first):
            srcs = self._pinned_planes(group)
            more = dict(kw)
            if any(g[3] for g in group):
                more["refs"], more["ref_index"] = dedupe_refs([g[2] for g in group], len(group))
            return self.forward_async_gray(slot, srcs, [g[1] for g in group], out=out, depth=depth, **more), srcs

        yield from self._temporal_stream(temporal, self._two_slot_stream(
            items, batch, upsample, parse, submit, lambda state: [self._own_image(r, self._out_dims(s, out)) for r, s in zip(state[0], state[1])],
            key=lambda g: g[0].dtype, ingest=ingest, output=(out_format, out_matrix)))

    def suggest_gray(self, items, centres, batch=None, out="source", depth=8, peaks=8, radius=2, skip_hints=True, K=5, N_draws=25000, seed=0,
                     upsample=None, ingest=None, out_format=None, out_matrix=None, **kw):
        """Generator: ``suggest_images`` for greyscale planes -- where to put the next hints on a folder of black-and-white photographs, and
        in which colours.  An item is ``gray`` or ``(gray, hints)``; it yields ``(rgb, peaks, colours, conf)`` per image as ``suggest_images``
        does, grouped as ``colorize_gray`` groups."""
        P = int(peaks)
        if depth not in (8, 16) or (depth == 16 and out != "source"):
            raise ValueError("depth must be 8, or 16 with out='source'")

        def parse(item):
            g = _gray_item("suggest_gray", item, False)
            if depth == 16 and g[0].dtype != np.uint16:
                raise ValueError("suggest_gray: depth=16 needs uint16 items, got %s" % g[0].dtype)
            return g

        def submit(slot, group, first):
            srcs = self._pinned_planes(group)
            res = self.forward_async_gray(slot, srcs, [g[1] for g in group], out=out, depth=depth, peaks=P, radius=radius, skip_hints=skip_hints,
                                          queries="peaks", K=K, N_draws=N_draws, seed=int(seed) + first * P, bin_centres=centres, **kw)
            return res, srcs

        def finish(state):
            res, srcs = state
            K_ = res.sugg_centres.shape[1]
            sc, sf = np.array(res.sugg_centres).reshape(len(srcs), P, K_, 2), np.array(res.sugg_conf).reshape(len(srcs), P, K_)
            pk = np.array(res.peaks)
            return [(self._own_image(r, self._out_dims(srcs[i], out)), pk[i], sc[i], sf[i]) for i, r in enumerate(res.out_rgb)]

        batch = self._group_size(batch)
        if P < 1:
            raise ValueError("suggest_gray needs at least one peak per image")
        yield from self._two_slot_stream(items, batch, upsample, parse, submit, finish, key=lambda g: g[0].dtype, ingest=ingest,
                                         output=(out_format, out_matrix))

    def colorize_images(self, items, batch=None, out="source", upsample=None, ingest=None, out_format=None, out_matrix=None, temporal=None, **kw):
        """Generator: colourise a stream of single images of any sizes with both pipeline slots busy.  An item is ``rgb``, ``(rgb, hints)`` or
        ``(rgb, hints, ref)``: rgb (h,w,3) uint8, ``hints`` that image's hint list (rows as in ``set_hints``) or ``None``, ``ref`` ``None`` or an
        (h,w,3) uint8 reference photograph (a ``global_hints`` engine; ``kw`` then carries centres).  Consecutive items are grouped into
        batches of ``batch`` images (default ``max_batch``; the last may be shorter), batch k runs on slot k % 2 while batch k - 1 computes
        (``forward_async_images``), and one array per image is yielded in input order: (h,w,3) [out='source'] or (H,W,3) [out='net'], the
        caller's own copy.  Sources travel through one pinned pool block per batch; the same reference OBJECT given for several images of a
        batch is uploaded once (``dedupe_refs``).  ``kw``: mode, mask_value, maskcent, l_cent, centres, hist_flag, saturation.
        ``upsample``: as in ``colorize_stream`` ('joint': the edge-aware source-size output).  ``out_format`` / ``out_matrix``: as there; with
        'i420' or 'nv12' a ``YCC420`` / ``NV12`` tuple of plane views into one uint8 buffer is yielded per image.  ``temporal``: as in
        ``colorize_stream``."""
        def submit(slot, group, first):
            srcs = self._pinned_sources(group)
            more = dict(kw)
            if any(g[3] for g in group):
                more["refs"], more["ref_index"] = dedupe_refs([g[2] for g in group], len(group))
            return self.forward_async_images(slot, srcs, [g[1] for g in group], out=out, **more), srcs

        yield from self._temporal_stream(temporal, self._two_slot_stream(
            items, batch, upsample, lambda item: _image_item("colorize_images", item, True), submit,
            lambda state: [self._own_image(r, self._out_dims(s, out)) for r, s in zip(state[0], state[1])], ingest=ingest,
            output=(out_format, out_matrix)))

    def colorize_video(self, frames, hints=None, batch=None, out="source", depth=8, temporal=True, upsample=None, ingest=None, out_format=None,
                       out_matrix=None, vectors=False, tracked=False, **kw):
        """Generator: colourise the frames of one video sequence with the temporal ab filter (``set_temporal_filter``) and both pipeline slots
        busy.  ``frames`` is an iterable of (h,w,3) uint8 RGB images, or of (h,w) uint8 / uint16 planes (``forward_async_images`` /
        ``forward_async_gray``; a change of kind or dtype closes the batch, the sequence goes on).  ``hints``: None, a hint list held for every
        frame, or a dict frame index -> hint list: a key frame's hints hold until the next key (frames before the first key have none).
        ``(image, cut)`` is yielded per frame, in order: the image as ``colorize_images`` / ``colorize_gray`` yield it, and whether the
        frame passed unfiltered (the first frame, or a scene cut); with ``temporal=False`` every cut is False.  ``temporal``: True (the
        defaults), a dict of parameters (``motion=True`` or a dict of ``set_temporal_motion``'s adds motion compensation), False, or None (the
        engine's setting as it stands, the sequence not reset).  ``vectors=True``: ``(image, cut, v)`` is yielded, v int8 (H/8, W/8, 2) the
        frame's block vectors (dy, dx), zeros where the call ran without the filter or without motion.  With hint tracking in force
        (``temporal=dict(motion=dict(track=True))`` or a dict of ``set_hint_tracking``'s parameters there) and ``hints`` a dict, a key
        frame's list goes to THAT frame only and the device carries it along the vectors; a list ``hints`` still goes to every frame.
        ``tracked=True`` appends the frame's tracked mask plane (H,W) float32 to each yielded tuple (zeros where the call ran without
        tracking).  ``upsample``,
        ``ingest``, ``out_format`` and ``out_matrix`` as in ``colorize_stream``; ``kw``: mode, mask_value, maskcent, l_cent."""
        if depth not in (8, 16) or (depth == 16 and out != "source"):
            raise ValueError("depth must be 8, or 16 with out='source'")
        if hints is not None and not isinstance(hints, (list, tuple, dict)):
            raise ValueError("colorize_video: hints is None, a list or a dict frame index -> list")
        held = [None]

        def indexed():
            # (pulled behind ``_temporal_stream``'s settings: tracking is in force iff the filter, motion and tracking are all on)
            carried = self._temporal is not None and self.__dict__.get("_motion") is not None and self.__dict__.get("_track") is not None
            for k, frame in enumerate(frames):
                if isinstance(hints, dict):
                    if carried:                          # the device carries a key frame's hints: they go to that frame alone
                        yield frame, hints.get(k)
                        continue
                    if k in hints:
                        held[0] = hints[k]
                    yield frame, held[0]
                else:
                    yield frame, hints

        def parse(item):
            img = np.asarray(item[0])
            if img.ndim == 3:
                return _image_item("colorize_video", (img, item[1]), False)
            g = _gray_item("colorize_video", (img, item[1]), False)
            if depth == 16 and g[0].dtype != np.uint16:
                raise ValueError("colorize_video: depth=16 needs uint16 planes, got %s" % g[0].dtype)
            return g

        def submit(slot, group, first):
            if group[0][0].ndim == 2:
                srcs = self._pinned_planes(group)
                res = self.forward_async_gray(slot, srcs, [g[1] for g in group], out=out, depth=depth, **kw)
            else:
                if depth == 16:
                    raise ValueError("colorize_video: depth=16 needs uint16 planes, got RGB frames")
                srcs = self._pinned_sources(group)
                res = self.forward_async_images(slot, srcs, [g[1] for g in group], out=out, **kw)
            filtered = self._temporal is not None
            moving = filtered and self.__dict__.get("_motion") is not None
            return res, srcs, slot, filtered, moving, moving and self.__dict__.get("_track") is not None

        def finish(state):
            res, srcs, slot, filtered, moving, tracking = state
            cuts = self.temporal_info(slot, len(srcs))[0] if filtered else np.zeros(len(srcs), np.int32)
            rows = [(self._own_image(r, self._out_dims(s, out)), bool(c)) for r, s, c in zip(res, srcs, cuts)]
            if vectors:
                v = self.temporal_vectors(slot, len(srcs)) if moving else np.zeros((len(srcs), self.H // 8, self.W // 8, 2), np.int8)
                rows = [row + (v[k],) for k, row in enumerate(rows)]
            if tracked:
                m = self.tracked_hints(slot, len(srcs), want=("mask",))[1] if tracking else np.zeros((len(srcs), self.H, self.W), np.float32)
                rows = [row + (m[k],) for k, row in enumerate(rows)]
            return rows

        yield from self._temporal_stream(temporal, self._two_slot_stream(indexed(), batch, upsample, parse, submit, finish,
                                                                         key=lambda g: (g[0].ndim, g[0].dtype), ingest=ingest,
                                                                         output=(out_format, out_matrix)))

    def evaluate_images(self, items, batch=None, out="net", mode="reveal", upsample=None, ingest=None, out_format=None, out_matrix=None,
                        temporal=None, **kw):
        """Generator: score a stream of ground-truth colour images with both pipeline slots busy -- ``colorize_images`` whose every image is
        compared with itself on the device (``forward_async_eval``).  An item is ``rgb``, ``(rgb, rects)`` or ``(rgb, rects, ref)``; with
        mode='reveal' (default) ``rects`` are rows (y0, x0, y1, x1) whose colours the device reveals from the image, with 'ab' / 'rgb' they
        are hint rows as in ``set_hints``.  Grouping, slot alternation and order as in ``colorize_images``; one ``(psnr, sse)`` per image is
        yielded: ``sse`` (3,) uint64, ``psnr`` = ``evaluate.psnr_from_sse`` of it over the image's net size (out='net') or its own
        (out='source'), ``inf`` for an exact match.  24 bytes per image come back; no image does.  ``upsample``: as in ``colorize_stream``;
        with out='source' the score is then that of the joint image.  ``temporal``: as in ``colorize_stream``; the score is then that of
        the filtered image."""
        from .evaluate import psnr_from_sse

        def submit(slot, group, first):
            srcs = self._pinned_sources(group)
            more = dict(kw)
            if any(g[3] for g in group):
                more["refs"], more["ref_index"] = dedupe_refs([g[2] for g in group], len(group))
            sse = self.forward_async_eval(slot, srcs, [g[1] for g in group], out=out, mode=mode, want_rgb=False, **more)[0]
            return sse, [g[0].shape[:2] if out == "source" else (self.H, self.W) for g in group], srcs

        def finish(state):
            sse = np.array(state[0])
            return [(psnr_from_sse(sse[i], h, w), sse[i]) for i, (h, w) in enumerate(state[1])]

        yield from self._temporal_stream(temporal, self._two_slot_stream(
            items, batch, upsample, lambda item: _image_item("evaluate_images", item, True), submit, finish, ingest=ingest,
            output=(out_format, out_matrix)))      # (output scope only: no image comes back, the score reads the RGB)

    def suggest_images(self, items, centres, batch=None, out="source", peaks=8, radius=2, skip_hints=True, K=5, N_draws=25000, seed=0,
                       upsample=None, ingest=None, out_format=None, out_matrix=None, **kw):
        """Generator: ``colorize_images`` on an engine with a distribution head that also proposes where to put the next hints and in which
        colours (``forward_async_dist`` with the suggestions at the peaks).  An item is ``rgb`` or ``(rgb, hints)``; grouping, slot alternation
        and order as in ``colorize_images``.  Per image it yields ``(rgb, peaks (P,2) int32, colours (P,K,2) float64, conf (P,K) float64)``:
        the colourised image, its ``peaks`` uncertainty peaks as net coordinates (y, x) -- (-1, -1) once the image ran out of cells -- and
        the K suggested colours of each with their shares.  Peak k of the g-th image of the stream draws with seed ``seed + g * peaks + k``,
        whatever the batch size.  ``centres`` (B,2): the bin centres; ``kw``: mode, mask_value, maskcent, l_cent.  ``upsample``: as in
        ``colorize_stream``."""
        P = int(peaks)

        def submit(slot, group, first):
            srcs = self._pinned_sources(group)
            res = self.forward_async_dist(slot, srcs, [g[1] for g in group], out=out, want_rgb=True, peaks=P, radius=radius, skip_hints=skip_hints,
                                          queries="peaks", K=K, N_draws=N_draws, seed=int(seed) + first * P, centres=centres, **kw)
            return res, srcs

        def finish(state):
            res, srcs = state
            K_ = res.sugg_centres.shape[1]
            sc, sf = np.array(res.sugg_centres).reshape(len(srcs), P, K_, 2), np.array(res.sugg_conf).reshape(len(srcs), P, K_)
            pk = np.array(res.peaks)
            return [(self._own_image(r, self._out_dims(srcs[i], out)), pk[i], sc[i], sf[i]) for i, r in enumerate(res.out_rgb)]

        batch = self._group_size(batch)
        if P < 1:
            raise ValueError("suggest_images needs at least one peak per image")
        yield from self._two_slot_stream(items, batch, upsample, lambda item: _image_item("suggest_images", item, False), submit, finish, ingest=ingest,
                                         output=(out_format, out_matrix))

    def score_images(self, items, centres, batch=None, nn=1, sigma=5.0, ranks=(1, 5), mode="reveal", want_psnr=False, upsample=None, ingest=None,
                     out_format=None, out_matrix=None, **kw):
        """Generator: score the distribution head on a stream of ground-truth colour images with both pipeline slots busy --
        ``evaluate_images`` for the distribution (``forward_async_dist`` with ``score`` and no other tap).  An item is ``rgb`` or
        ``(rgb, rects)``, hints as in ``evaluate_images`` (mode 'reveal': the colours come from the image).  Per image it yields
        ``(xent_mean, hits, psnr)``: the mean cross-entropy of its cells against the (soft-)encoded truth, ``hits`` (len(ranks),) uint32 =
        cells whose true bin is among the ranks[j] most probable, and with ``want_psnr`` the net-size PSNR of the regression head
        (``None`` otherwise).  A few dozen bytes per image come back; no image and no distribution does.  ``kw``: mask_value, maskcent, l_cent.
        ``upsample``: as in ``colorize_stream``."""
        from .evaluate import psnr_from_sse
        score = dict(centres=centres, nn=nn, sigma=sigma, ranks=tuple(ranks))

        def submit(slot, group, first):
            srcs = self._pinned_sources(group)
            return self.forward_async_dist(slot, srcs, [g[1] for g in group], mode=mode, want_sse=bool(want_psnr), peaks=0, score=score, **kw), srcs

        def finish(state):
            res = state[0]
            mean, hits = res.score.mean(), np.array(res.score.hits)
            sse = np.array(res.sse) if want_psnr else None
            return [(float(mean[i]), hits[i], psnr_from_sse(sse[i], self.H, self.W) if want_psnr else None) for i in range(len(mean))]

        yield from self._two_slot_stream(items, batch, upsample, lambda item: _image_item("score_images", item, False), submit, finish, ingest=ingest,
                                         output=(out_format, out_matrix))

    def wait(self, slot):
        self._chk(self.lib.idc_wait(self._h, int(slot)))
        self._in_flight.pop(int(slot), None)

    def pipeline_times(self, slot):
        """ms since the pipeline's first use of (H2D start, H2D end, compute start, compute end, D2H start, D2H end) of the
        slot's last completed batch (after ``wait(slot)``)."""
        ms = np.zeros(6, np.float32)
        self._chk(self.lib.idc_pipeline_times(self._h, int(slot), _fptr(ms)))
        return ms

    # ---- RCCL weight broadcast through the C ABI (one call per rank) -------------------------------------------
    def comm_unique_id(self):
        buf = (ctypes.c_char * N.IDC_UNIQUE_ID_BYTES)()
        N.check(self.lib.idc_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p)))
        return bytes(buf)

    def broadcast_weights(self, unique_id, rank, world, root=0):
        if len(unique_id) != N.IDC_UNIQUE_ID_BYTES:
            raise ValueError("unique id must be %d bytes" % N.IDC_UNIQUE_ID_BYTES)
        buf = ctypes.create_string_buffer(bytes(unique_id), N.IDC_UNIQUE_ID_BYTES)
        self._chk(self.lib.idc_broadcast_weights(self._h, ctypes.cast(buf, ctypes.c_void_p), int(rank), int(world), int(root)))

    # ---- display / full-resolution step on the device (ui/gui_draw.py:280-283, colorize_image.py:123-158) ------
    def upsample_lab2rgb(self, L_out, source="output_ab", interp="cubic", img=0):
        """ab planes of slot ``img`` resized to ``L_out.shape`` and combined with that L plane -> (oh, ow, 3) uint8.
        source: 'output_ab' (refreshed, float64), 'output_ab_raw', 'input_ab'; interp: 'cubic' (cv2 INTER_CUBIC),
        'linear' / 'nearest' (scipy.ndimage.zoom order 1 / 0)."""
        Ld = np.ascontiguousarray(np.asarray(L_out, dtype=np.float64))
        if Ld.ndim == 3 and Ld.shape[0] == 1:
            Ld = Ld[0]
        oh, ow = Ld.shape
        rgb = np.empty((oh, ow, 3), np.uint8)
        src = {"output_ab": N.IDC_SRC_OUTPUT_AB, "output_ab_raw": N.IDC_SRC_OUTPUT_AB_RAW, "input_ab": N.IDC_SRC_INPUT_AB}[source]
        itp = {"cubic": N.IDC_INTERP_CUBIC, "linear": N.IDC_INTERP_LINEAR, "nearest": N.IDC_INTERP_NEAREST}[interp]
        self._chk(self.lib.idc_upsample_lab2rgb(self._h, int(img), src, itp, int(oh), int(ow), Ld.ctypes.data_as(ctypes.c_void_p),
                                                rgb.ctypes.data_as(ctypes.c_void_p)))
        return rgb

    @property
    def stream(self):
        return self.lib.idc_stream(self._h)

    # ---- introspection ----------------------------------------------------------------------
    def layer_table(self):
        rows = []
        for i in range(self.lib.idc_num_layers(self._h)):
            info = N.LayerInfo()
            self._chk(self.lib.idc_layer_info_get(self._h, i, ctypes.byref(info)))
            rows.append(dict(index=i, name=info.name.decode(), kernel=info.kernel.decode(), flops=info.flops,
                             min_bytes=info.min_bytes, launches=info.launches))
        return rows

    def set_profiling(self, on):
        self._chk(self.lib.idc_set_profiling(self._h, 2 if on == "forward" else (1 if on else 0)))

    def layer_times_ms(self):
        n = self.lib.idc_num_layers(self._h)
        ms = np.zeros(n, np.float32)
        self._chk(self.lib.idc_layer_times_ms(self._h, _fptr(ms), n))
        return ms

    def layer_times_stats(self):
        """(min, median, max) per layer over the forwards recorded since profiling was switched on (at most the last 32)."""
        n = self.lib.idc_num_layers(self._h)
        lo, med, hi = (np.zeros(n, np.float32) for _ in range(3))
        self._chk(self.lib.idc_layer_times_stats(self._h, _fptr(lo), _fptr(med), _fptr(hi), n))
        return lo, med, hi

    def activation(self, name, n=1):
        """NCHW fp32 copy of an intermediate tensor of the last forward (parity tests)."""
        cap = int(n) * 640 * self.H * self.W
        buf = np.empty(cap, np.float32)
        C, H, W = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._chk(self.lib.idc_get_activation(self._h, name.encode(), int(n), _fptr(buf), cap,
                                              ctypes.byref(C), ctypes.byref(H), ctypes.byref(W)))
        return buf[: n * C.value * H.value * W.value].reshape(n, C.value, H.value, W.value).copy()


# ---- single operators through the same kernels (used by the parity tests) ---------------------
# policy_batch: the batch the kernel variant is chosen for, as a handle's max_batch is (option 'op_policy_batch'); None leaves the option as it
# is, 0 = the call's own batch.  The launch carries the call's batch either way; op_last_kernel() names what ran.
def _set_policy_batch(policy_batch):
    if policy_batch is not None:
        set_option("op_policy_batch", int(policy_batch))


# out_f32 / resid_f32: the op's output tensor / the shortcut sum of a bf16 op stored in fp32, as the network stores its class / 313 logits and the
# hyper-column partial sums (options 'op_out_f32', 'op_resid_f32').  Set on EVERY call, so that one call's storage never reaches the next.
def _set_op_storage(out_f32, resid_f32):
    set_option("op_out_f32", 1 if out_f32 else 0)
    set_option("op_resid_f32", 1 if resid_f32 else 0)


def op_last_kernel():
    """Label of the kernel the last op_* call of this thread launched, as layer_table() names kernels (``idc_op_last_kernel``)."""
    buf = ctypes.create_string_buffer(96)
    N.check(N.load().idc_op_last_kernel(buf, len(buf)))
    return buf.value.decode()


def op_conv2d(x, weight, bias, dilation=1, in_stride=1, act=0, bn_scale=None, bn_shift=None, resid=None,
              precision="fp32", device=0, policy_batch=None, out_f32=False, resid_f32=False):
    lib = N.load()
    _set_policy_batch(policy_batch)
    _set_op_storage(out_f32, resid_f32)
    x = _f32c(x); weight = _f32c(weight); bias = _f32c(bias)
    n, cin, h, w = x.shape
    cout, ksize = weight.shape[0], weight.shape[2]
    y = np.empty((n, cout, h // in_stride, w // in_stride), np.float32)
    keep = [_f32c(a) if a is not None else None for a in (bn_scale, bn_shift, resid)]
    ptr = [_fptr(a) if a is not None else None for a in keep]
    N.check(lib.idc_op_conv2d(device, _PREC[precision], n, cin, h, w, _fptr(x), cout, ksize, dilation, in_stride,
                              _fptr(weight), _fptr(bias), act, ptr[0], ptr[1], ptr[2], _fptr(y)))
    return y


def op_deconv4x4s2(x, weight, bias, act=0, resid=None, precision="fp32", device=0, policy_batch=None, out_f32=False, resid_f32=False):
    lib = N.load()
    _set_policy_batch(policy_batch)
    _set_op_storage(out_f32, resid_f32)
    x = _f32c(x); weight = _f32c(weight); bias = _f32c(bias)
    n, cin, h, w = x.shape
    cout = weight.shape[1]
    y = np.empty((n, cout, 2 * h, 2 * w), np.float32)
    r = _f32c(resid) if resid is not None else None
    N.check(lib.idc_op_deconv4x4s2(device, _PREC[precision], n, cin, h, w, _fptr(x), cout, _fptr(weight),
                                   _fptr(bias), act, _fptr(r) if r is not None else None, _fptr(y)))
    return y


def op_deconv_shortcut(x, w_deconv, b_deconv, x_short, w_short, b_short, act=0, precision="bf16", policy_batch=None, device=0):
    """act(deconv4x4s2(x) + conv3x3(x_short) + b_deconv + b_short) as the ONE launch the network makes of a decoder level's ConvTranspose and
    the shortcut conv summed into it (``idc_op_deconv_shortcut``); raises IdcError (UNSUPPORTED) where the network would launch the two apart."""
    lib = N.load()
    _set_policy_batch(policy_batch)
    _set_op_storage(False, False)                # (the fused launch stores 16-bit outputs and never reads a stored shortcut sum)
    x = _f32c(x); w_deconv = _f32c(w_deconv); b_deconv = _f32c(b_deconv)
    x_short = _f32c(x_short); w_short = _f32c(w_short); b_short = _f32c(b_short)
    n, cin, h, w = x.shape
    cout, cin_short = w_deconv.shape[1], w_short.shape[1]
    if x_short.shape != (n, cin_short, 2 * h, 2 * w) or w_short.shape != (cout, cin_short, 3, 3) or w_deconv.shape != (cin, cout, 4, 4):
        raise ValueError("op_deconv_shortcut: shapes %s %s %s %s do not fit" % (x.shape, w_deconv.shape, x_short.shape, w_short.shape))
    y = np.empty((n, cout, 2 * h, 2 * w), np.float32)
    N.check(lib.idc_op_deconv_shortcut(device, _PREC[precision], n, cin, h, w, _fptr(x), cout, _fptr(w_deconv), _fptr(b_deconv),
                                       cin_short, _fptr(x_short), _fptr(w_short), _fptr(b_short), act, _fptr(y)))
    return y


def grid_tags():
    """Names of the capped grid-stride launch sites (``idc_grid_tag``): what option 'grid_cap' lowers and grid_last() reports."""
    lib = N.load()
    tags, i = [], 0
    while True:
        t = lib.idc_grid_tag(i)
        if t is None:
            return tags
        tags.append(t.decode())
        i += 1


def grid_last(tag):
    """(want, blocks) of the last launch of capped launch site ``tag`` in this process (``idc_grid_last``): the workgroups that would cover its
    items in one pass and the grid it got; (0, 0) before its first launch."""
    want, blocks = ctypes.c_longlong(0), ctypes.c_int(0)
    N.check(N.load().idc_grid_last(tag.encode(), ctypes.byref(want), ctypes.byref(blocks)))
    return int(want.value), int(blocks.value)
