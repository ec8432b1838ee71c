"""The sizes of a handle's activation tensors, restated in Python integers from the rules of build_layers / alloc_graph (csrc/idc_plan.hip) and
the layer list of csrc/idc_net.h -- for the tests that work out where a tensor passes 2^31 and 2^32 bytes (tests/test_large_batch_gpu.py) and how
many bytes of its source one image of a layer holds (tests/test_large_plan_cpu.py).  Nothing here touches the library."""
from collections import OrderedDict

ROW_BYTES = 128                   # kRowBytes: one 128-byte chunk of a pixel's channels
ARENA_ALIGN = 2 << 20             # alloc_graph: every tensor starts on a 2 MiB boundary of the one arena
FLAG_DIST, FLAG_DIST313 = 0x1, 0x8
PARTS = {"fp32": 1, "bf16": 1, "bf16x3": 2, "bf16x6": 3, "fp16x3": 2, "fp16": 1}      # split_parts
SPLIT = ("bf16x3", "bf16x6", "fp16x3", "fp16")                                       # is_split

# (name, kind, cin, cout, in_stride, src, resid, out_f32, level, dist_only): layer_specs(), the columns the sizes depend on
LAYERS = [
    ("conv1_1", "im2col", 4, 64, 1, "data_l_ab_mask", None, 0, 1, 0),
    ("conv1_2", "c3", 64, 64, 1, "conv1_1", None, 0, 1, 0),
    ("conv2_1", "c3", 64, 128, 2, "conv1_2", None, 0, 2, 0),
    ("conv2_2", "c3", 128, 128, 1, "conv2_1", None, 0, 2, 0),
    ("conv3_1", "c3", 128, 256, 2, "conv2_2", None, 0, 4, 0),
    ("conv3_2", "c3", 256, 256, 1, "conv3_1", None, 0, 4, 0),
    ("conv3_3", "c3", 256, 256, 1, "conv3_2", None, 0, 4, 0),
    ("conv4_1", "c3", 256, 512, 2, "conv3_3", None, 0, 8, 0),
    ("conv4_2", "c3", 512, 512, 1, "conv4_1", None, 0, 8, 0),
    ("conv4_3", "c3", 512, 512, 1, "conv4_2", None, 0, 8, 0),
    ("conv5_1", "c3", 512, 512, 1, "conv4_3", None, 0, 8, 0),
    ("conv5_2", "c3", 512, 512, 1, "conv5_1", None, 0, 8, 0),
    ("conv5_3", "c3", 512, 512, 1, "conv5_2", None, 0, 8, 0),
    ("conv6_1", "c3", 512, 512, 1, "conv5_3", None, 0, 8, 0),
    ("conv6_2", "c3", 512, 512, 1, "conv6_1", None, 0, 8, 0),
    ("conv6_3", "c3", 512, 512, 1, "conv6_2", None, 0, 8, 0),
    ("conv7_1", "c3", 512, 512, 1, "conv6_3", None, 0, 8, 0),
    ("conv7_2", "c3", 512, 512, 1, "conv7_1", None, 0, 8, 0),
    ("conv7_3", "c3", 512, 512, 1, "conv7_2", None, 0, 8, 0),
    ("conv3_3_short", "c3", 256, 256, 1, "conv3_3", None, 0, 4, 0),
    ("conv8_1", "dc", 512, 256, 1, "conv7_3", "conv3_3_short", 0, 4, 0),
    ("conv8_2", "c3", 256, 256, 1, "conv8_1", None, 0, 4, 0),
    ("conv8_3", "c3", 256, 256, 1, "conv8_2", None, 0, 4, 0),
    ("class_logits", "c1", 256, 529, 1, "conv8_3", None, 1, 4, 1),
    ("conv2_2_short", "c3", 128, 128, 1, "conv2_2", None, 0, 2, 0),
    ("conv9_1", "dc", 256, 128, 1, "conv8_3", "conv2_2_short", 0, 2, 0),
    ("conv9_2", "c3", 128, 128, 1, "conv9_1", None, 0, 2, 0),
    ("conv1_2_short", "c3", 64, 128, 1, "conv1_2", None, 0, 1, 0),
    ("conv10_1", "dc", 128, 128, 1, "conv9_2", "conv1_2_short", 0, 1, 0),
    ("conv10_2", "c3", 128, 128, 1, "conv10_1", None, 0, 1, 0),
    ("conv3_pred", "c3", 256, 384, 1, "conv3_3", None, 1, 4, 2),
    ("conv34_pred", "dc", 512, 384, 1, "conv4_3", "conv3_pred", 1, 4, 2),
    ("conv345_pred", "dc", 512, 384, 1, "conv5_3", "conv34_pred", 1, 4, 2),
    ("conv3456_pred", "dc", 512, 384, 1, "conv6_3", "conv345_pred", 1, 4, 2),
    ("conv34567_pred", "dc", 512, 384, 1, "conv7_3", "conv3456_pred", 1, 4, 2),
    ("conv345678_pred", "c3", 256, 384, 1, "conv8_3", "conv34567_pred", 0, 4, 2),
    ("pred_313", "c1", 384, 313, 1, "conv345678_pred", None, 1, 4, 2),
]


def cout_pad(cout):
    return 64 if cout <= 64 else (cout + 127) // 128 * 128


def active_layers(flags=0):
    return [l for l in LAYERS if l[9] == 0 or (l[9] == 1 and flags & FLAG_DIST) or (l[9] == 2 and flags & FLAG_DIST313)]


def tensors(precision, H, W, flags=0):
    """name -> dict(cpad, h, w, f32, parts, pixel_bytes, image_bytes) of every activation tensor a handle stores, in build_layers' order.
    Storage: fp32 on the fp32 path, for LayerSpec.out_f32, and on the operand-split path for every shortcut branch; else 2-byte elements in
    `parts` planes.  (conv1_1 of a split handle is written as split planes: conv1_2 reads it.)"""
    act = active_layers(flags)
    split, eb = precision in SPLIT, 4 if precision == "fp32" else 2
    shortcuts = set(l[6] for l in act if l[6])
    out = OrderedDict()
    for name, kind, cin, cout, si, src, resid, out_f32, level, _ in act:
        f32 = precision == "fp32" or bool(out_f32) or (split and name in shortcuts)
        if split and kind == "im2col":
            f32 = False
        parts = PARTS[precision] if (split and not f32) else 1
        cpad = cout_pad(cout)
        pixel_bytes = cpad * (4 if f32 else eb * parts)
        out[name] = dict(cpad=cpad, h=H // level, w=W // level, f32=f32, parts=parts, pixel_bytes=pixel_bytes,
                         image_bytes=(H // level) * (W // level) * pixel_bytes)
    return out


def _align(v, a):
    return (v + a - 1) // a * a


def arena_bytes(precision, H, W, max_batch, flags=0):
    """alloc_graph's one arena: every tensor (max_batch images each) on a 2 MiB boundary, the never-materialised input tensor's 256 bytes first."""
    return _align(256, ARENA_ALIGN) + sum(_align(max_batch * t["image_bytes"], ARENA_ALIGN) for t in tensors(precision, H, W, flags).values())


def device_bytes(precision, H, W, max_batch, flags=0, post=False, pipeline=False):
    """The arena plus the handle's planes: L, ab, mask, ab output (24 bytes per pixel); the colour step's RGB, float64 Lab and input (39); the two pipeline
    slots' planes (48).  What a test compares with the device's free memory before it creates the handle."""
    px = max_batch * H * W
    return arena_bytes(precision, H, W, max_batch, flags) + px * (24 + (39 if post else 0) + (48 if pipeline else 0))


def size_classes(precision, H, W, flags=0):
    """image_bytes -> names of the tensors with that many bytes per image, largest first."""
    by = {}
    for name, t in tensors(precision, H, W, flags).items():
        by.setdefault(t["image_bytes"], []).append(name)
    return OrderedDict(sorted(by.items(), reverse=True))


def boundary_images(precision, H, W, max_batch, flags=0, marks=(1 << 31, 1 << 32)):
    """[(image_bytes, mark, k, D)] for every size class whose tensor passes a mark inside the handle: image k = mark // image_bytes holds the tensor's
    byte `mark` (it starts exactly there when image_bytes divides the mark: then D = k is the distance, in images, that an offset narrowed by
    `mark` bytes lands short; else D is None).  Images k - 1 and k + 1 lie wholly below and above the mark."""
    out = []
    for ib in size_classes(precision, H, W, flags):
        for mark in marks:
            if max_batch * ib > mark:
                k = mark // ib
                out.append((ib, mark, k, k if mark % ib == 0 else None))
    return out


def source_bytes(layer, precision, H, W, flags=0):
    """Bytes of ONE image of the tensor `layer` reads as its K-loop source -- Hs * si * Ws * si * nkc * parts * kRowBytes of its launch -- or None for
    conv1_1, whose source is the caller's planes (its input tensor is never stored)."""
    name, kind, cin, cout, si, src, resid, out_f32, level, _ = [l for l in LAYERS if l[0] == layer][0]
    if kind == "im2col":
        return None
    t = tensors(precision, H, W, flags)[src]
    hs, ws = (t["h"], t["w"]) if kind == "dc" else (H // level, W // level)          # a deconv's sites are its source's pixels
    si = 1 if kind == "dc" else si
    nkc = t["cpad"] * (4 if t["f32"] else 2) // ROW_BYTES
    got = hs * si * ws * si * nkc * t["parts"] * ROW_BYTES
    assert got == t["image_bytes"], (layer, got, t)
    return got
