"""The YCbCr 4:2:0 output rule of include/ideepcolor.h in plain Python integers, and the inputs the GPU file converts.  The rule loops over the
chroma blocks and divides the non-negative numerators with ``//``; it shares no code with the engine or with colorspace.py.  tests/test_ycc_cpu.py
shows that the exact comparison against it catches eight mutants of the rule on these inputs."""
import numpy as np

import ragged_ref

H = W = 64                                   # the net of the GPU file

# 16.16 fixed point: (luma, Cb, Cr, Yoff)
MATRICES = {
    "jfif": ((19595, 38470, 7471), (-11059, -21709, 32768), (32768, -27439, -5329), 0),
    "bt709": ((11966, 40254, 4064), (-6596, -22189, 28785), (28784, -26145, -2639), 16),
}
FORMATS = ("i420", "nv12")
BIAS = (128 << 16) + 32767


def nbytes(h, w):
    return h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)


def pixel(r, g, b, matrix):
    """(Y, Cb, Cr) of one colour: the rule at k = 1."""
    my, mcb, mcr, yoff = MATRICES[matrix]
    return (((my[0] * r + my[1] * g + my[2] * b + 32768) >> 16) + yoff,
            (mcb[0] * r + mcb[1] * g + mcb[2] * b + BIAS) // 65536,
            (mcr[0] * r + mcr[1] * g + mcr[2] * b + BIAS) // 65536)


_PLANES = {}


def planes(rgb, matrix):
    """(Y [h,w], Cb [ch,cw], Cr [ch,cw]) uint8 of an (h,w,3) uint8 image.  Cached per (array object, matrix): the inputs below are made once and
    never written to."""
    key = (id(rgb), matrix)
    if key in _PLANES and _PLANES[key][0] is rgb:
        return _PLANES[key][1]
    my, mcb, mcr, yoff = MATRICES[matrix]
    h, w = rgb.shape[:2]
    ch, cw = (h + 1) // 2, (w + 1) // 2
    rows = [bytes(rgb[y].tobytes()) for y in range(h)]
    Y, Cb, Cr = bytearray(), bytearray(), bytearray()
    for j in range(ch):
        ys = range(2 * j, min(2 * j + 2, h))                 # clipped at the image's edge, not replicated
        tcb, tcr = [], []
        for y in ys:
            px = list(zip(rows[y][0::3], rows[y][1::3], rows[y][2::3]))
            for r, g, b in px:
                v = ((my[0] * r + my[1] * g + my[2] * b + 32768) >> 16) + yoff
                assert 0 <= v <= 255
                Y.append(v)
            tcb.append([mcb[0] * r + mcb[1] * g + mcb[2] * b for r, g, b in px])
            tcr.append([mcr[0] * r + mcr[1] * g + mcr[2] * b for r, g, b in px])
        for i in range(cw):
            xs = range(2 * i, min(2 * i + 2, w))
            k = len(ys) * len(xs)
            for terms, plane in ((tcb, Cb), (tcr, Cr)):
                num = sum(t[x] for t in terms for x in xs) + k * BIAS
                assert num >= 0 and k in (1, 2, 4)
                v = num // (65536 * k)
                assert 0 <= v <= 255
                plane.append(v)
    out = (np.frombuffer(bytes(Y), np.uint8).reshape(h, w), np.frombuffer(bytes(Cb), np.uint8).reshape(ch, cw),
           np.frombuffer(bytes(Cr), np.uint8).reshape(ch, cw))
    _PLANES[key] = (rgb, out)
    return out


def block(rgb, fmt, matrix):
    """The image's plane block: Y, then Cb and Cr ('i420') or the interleaved pairs ('nv12'), one flat uint8 array."""
    y, cb, cr = planes(rgb, matrix)
    if fmt == "i420":
        return np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)])
    assert fmt == "nv12"
    return np.concatenate([y.reshape(-1), np.stack([cb, cr], axis=-1).reshape(-1)])


# ---- the inputs of the GPU file's conversion case: ONE call holds them all -----------------------------------------------------------------
SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (1, 1000), (1000, 1), (64, 64), (48, 80), (211, 83), (65, 16384)]
PRIMARIES = [(255, 0, 0), (0, 0, 255), (0, 255, 0), (255, 255, 0), (255, 0, 255), (0, 255, 255), (0, 0, 0), (255, 255, 255)]


def painted(h, w, seed):
    """Seeded noise under PIL-drawn rectangles of saturated primaries whose hard edges lie at odd coordinates: blocks that are one saturated
    colour, and blocks that straddle an edge between two."""
    from PIL import Image, ImageDraw
    rs = np.random.RandomState(seed)
    im = Image.fromarray(rs.randint(0, 256, (h, w, 3)).astype(np.uint8))
    draw = ImageDraw.Draw(im)
    for k, colour in enumerate(PRIMARIES):
        y0, x0 = 1 + 2 * rs.randint(0, max(1, h // 2)), 1 + 2 * rs.randint(0, max(1, w // 2))
        draw.rectangle([x0, y0, x0 + 2 * rs.randint(1, 8 + w // 8), y0 + 2 * rs.randint(1, 8 + h // 8)], fill=colour)
    if h >= 8 and w >= 8:                                    # two fixed ones, so that what the CPU file asserts about the inputs holds for every seed
        draw.rectangle([1, 1, 6, 6], fill=(0, 0, 255))      # pure blue blocks at (1..2, 1..2) and blue / noise edges through blocks 0 and 3
        draw.rectangle([7, 1, 12, 6], fill=(255, 0, 0))     # red against blue inside block column 3
    a = np.array(im)
    return a


_INPUTS = []


def inputs():
    """[(name, (h,w,3) uint8 read-only)]: the sizes above with painted content (tiny ones: noise), the size lists of tests/ragged_ref.py (a
    packed run whose image starts cover every residue mod 4) with noise, and flat 0 and 255 at odd sizes."""
    if _INPUTS:
        return _INPUTS
    out = []
    for k, (h, w) in enumerate(SIZES):
        if min(h, w) >= 3:
            out.append(("%dx%d painted" % (h, w), painted(h, w, 100 + k)))
        else:
            out.append(("%dx%d noise" % (h, w), np.random.RandomState(100 + k).randint(0, 256, (h, w, 3)).astype(np.uint8)))
    for li, lst in enumerate([ragged_ref.MIXED] + ragged_ref.SPANS):
        for k, (h, w) in enumerate(ragged_ref.sizes(lst, H, W)):
            out.append(("ragged%d.%d %dx%d" % (li, k, h, w), np.random.RandomState(1000 + 50 * li + k).randint(0, 256, (h, w, 3)).astype(np.uint8)))
    out.append(("5x7 flat 0", np.zeros((5, 7, 3), np.uint8)))
    out.append(("7x5 flat 255", np.full((7, 5, 3), 255, np.uint8)))
    out.append(("3x9 blue", np.tile(np.array([0, 0, 255], np.uint8), (3, 9, 1))))
    out.append(("9x3 red", np.tile(np.array([255, 0, 0], np.uint8), (9, 3, 1))))
    for _, a in out:
        a.setflags(write=False)
    _INPUTS.extend(out)
    return _INPUTS


def start_residues():
    """The residues mod 4 of the byte at which each input's RGB starts in a packed run."""
    at, seen = 0, set()
    for _, a in inputs():
        seen.add(at % 4)
        at += a.size
    return seen
