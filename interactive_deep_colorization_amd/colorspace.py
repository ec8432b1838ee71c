"""Host-side colour maths and image IO for the drop-in API (vectorised numpy).

The reference does this with scikit-image / OpenCV / scipy
(``data/colorize_image.py:20-36,52-66,123-158``); neither skimage nor cv2 exists
in this image, so the formulas are restated.  This is
host plumbing around the HIP path, not part of it; it runs once per image load
(RGB->Lab) and once per ``net_forward`` (Lab->RGB of the 256x256 result).

sRGB, D65 white, 2-degree observer -- the constants skimage uses.
"""
import numpy as np

_XYZ_FROM_RGB = np.array([[0.412453, 0.357580, 0.180423],
                          [0.212671, 0.715160, 0.072169],
                          [0.019334, 0.119193, 0.950227]], dtype=np.float64)
_RGB_FROM_XYZ = np.linalg.inv(_XYZ_FROM_RGB)
_WHITE = np.array([0.95047, 1.0, 1.08883], dtype=np.float64)


def _as_float_rgb(rgb):
    arr = np.asarray(rgb)
    if arr.dtype == np.uint8:
        return arr.astype(np.float64) / 255.0
    return arr.astype(np.float64)


def rgb2lab(rgb):
    """``skimage.color.rgb2lab``: (...,3) uint8 or float[0,1] -> (...,3) float64 Lab."""
    arr = _as_float_rgb(rgb)
    lin = np.where(arr > 0.04045, np.power((arr + 0.055) / 1.055, 2.4), arr / 12.92)
    xyz = lin @ _XYZ_FROM_RGB.T
    xyz = xyz / _WHITE
    f = np.where(xyz > 0.008856, np.cbrt(xyz), 7.787 * xyz + 16.0 / 116.0)
    fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
    return np.stack((116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)), axis=-1)


def lab2rgb(lab):
    """``skimage.color.lab2rgb``: (...,3) Lab -> (...,3) float64 sRGB clipped to [0,1]."""
    lab = np.asarray(lab, dtype=np.float64)
    fy = (lab[..., 0] + 16.0) / 116.0
    fx = lab[..., 1] / 500.0 + fy
    fz = np.maximum(fy - lab[..., 2] / 200.0, 0.0)          # skimage zeroes negative z
    f = np.stack((fx, fy, fz), axis=-1)
    xyz = np.where(f > 0.2068966, f ** 3, (f - 16.0 / 116.0) / 7.787) * _WHITE
    lin = xyz @ _RGB_FROM_XYZ.T
    srgb = np.where(lin > 0.0031308, 1.055 * np.power(np.maximum(lin, 0.0), 1.0 / 2.4) - 0.055, 12.92 * lin)
    return np.clip(srgb, 0.0, 1.0)


def lab2rgb_transpose(img_l, img_ab):
    """``data/colorize_image.py:20-28``: (1,X,X) L + (2,X,X) ab -> (X,X,3) uint8."""
    pred_lab = np.concatenate((img_l, img_ab), axis=0).transpose((1, 2, 0))
    return (np.clip(lab2rgb(pred_lab), 0, 1) * 255).astype("uint8")


def rgb2lab_transpose(img_rgb):
    """``data/colorize_image.py:31-36``: (X,X,3) -> (3,X,X)."""
    return rgb2lab(img_rgb).transpose((2, 0, 1))


def resize_bilinear_u8(img, out_h, out_w):
    """Bilinear resize with half-pixel centres and edge clamp, no antialiasing --
    the sampling rule of ``cv2.resize(im, (Xd, Xd))`` (INTER_LINEAR) used at
    ``data/colorize_image.py:58``.  Float arithmetic, round-half-up; OpenCV's
    11-bit fixed-point path can differ by one grey level."""
    img = np.asarray(img)
    in_h, in_w = img.shape[:2]
    ys = (np.arange(out_h) + 0.5) * (in_h / float(out_h)) - 0.5
    xs = (np.arange(out_w) + 0.5) * (in_w / float(out_w)) - 0.5
    y0 = np.floor(ys).astype(np.int64); x0 = np.floor(xs).astype(np.int64)
    wy = (ys - y0)[:, None, None]; wx = (xs - x0)[None, :, None]
    y0c = np.clip(y0, 0, in_h - 1); y1c = np.clip(y0 + 1, 0, in_h - 1)
    x0c = np.clip(x0, 0, in_w - 1); x1c = np.clip(x0 + 1, 0, in_w - 1)
    f = img.astype(np.float64)
    if f.ndim == 2:
        f = f[:, :, None]
    top = f[y0c][:, x0c] * (1 - wx) + f[y0c][:, x1c] * wx
    bot = f[y1c][:, x0c] * (1 - wx) + f[y1c][:, x1c] * wx
    out = top * (1 - wy) + bot * wy
    out = np.floor(out + 0.5).clip(0, 255).astype(np.uint8)
    return out if img.ndim == 3 else out[:, :, 0]


def _antialias_axis(n_in, n_out):
    """Taps and weights of one axis of ``resize_antialias``: (idx, wt), both (n_out, K); a row's taps ascend, and the padding at the end of
    a row shorter than K has weight 0 (adding 0.0 last changes no sum)."""
    i = np.arange(n_out, dtype=np.float64)
    s = n_in / float(n_out)
    if n_in <= n_out:                                   # the two clamped taps of resize_bilinear_u8
        src = (i + 0.5) * s - 0.5
        i0 = np.floor(src)
        w = src - i0
        i0 = i0.astype(np.int64)
        idx = np.stack([np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1)], axis=1)
        return idx, np.stack([1.0 - w, w], axis=1)
    c = (i + 0.5) * s
    lo = np.maximum(0, np.trunc(c - s + 0.5).astype(np.int64))
    hi = np.minimum(n_in, np.trunc(c + s + 0.5).astype(np.int64))
    k = lo[:, None] + np.arange(int((hi - lo).max()), dtype=np.int64)[None, :]
    r = np.maximum(0.0, 1.0 - np.abs((k.astype(np.float64) + 0.5) - c[:, None]) / s) * (k < hi[:, None])
    tot = np.zeros(n_out)
    for j in range(r.shape[1]):                         # ascending k, one term at a time: numpy's own sum is pairwise
        tot = tot + r[:, j]
    return np.minimum(k, n_in - 1), r / tot[:, None]


def resize_antialias(img, out_h, out_w):
    """The host twin of the device's antialiased ingestion (``HipColorizer.set_ingest_filter('antialias')``; the rule:
    include/ideepcolor.h): a source larger than the target on an axis is filtered with the tent stretched by the scale -- the window
    clipped to the image and renormalised, the rule of PIL's BILINEAR and of torch's ``interpolate(mode='bilinear', antialias=True)`` -- in
    float64, the vertical sums first, each in ascending order, then floor(v + .5) clamped to the lattice of the source's dtype.  uint8 or
    uint16, (h,w) or (h,w,c).  A source that is not down-scaled on either axis takes ``resize_bilinear_u8``'s expressions (on the 16-bit
    lattice for uint16) and is bit-identical to it."""
    img = np.asarray(img)
    if img.dtype not in (np.uint8, np.uint16) or img.ndim not in (2, 3):
        raise ValueError("resize_antialias needs a uint8 or uint16 (h,w) or (h,w,c) image, got %s %s" % (img.dtype, img.shape))
    full = 255 if img.dtype == np.uint8 else 65535
    in_h, in_w = img.shape[:2]
    f = img if img.ndim == 3 else img[:, :, None]
    if in_h <= out_h and in_w <= out_w:
        if img.dtype == np.uint8:
            return resize_bilinear_u8(img, out_h, out_w)
        (iy, wy), (ix, wx) = _antialias_axis(in_h, out_h), _antialias_axis(in_w, out_w)
        g = f.astype(np.float64)
        wxe, wye = wx[None, :, 1, None], wy[:, 1, None, None]
        top = g[iy[:, 0]][:, ix[:, 0]] * (1 - wxe) + g[iy[:, 0]][:, ix[:, 1]] * wxe
        bot = g[iy[:, 1]][:, ix[:, 0]] * (1 - wxe) + g[iy[:, 1]][:, ix[:, 1]] * wxe
        out = np.floor(top * (1 - wye) + bot * wye + 0.5).clip(0, full).astype(img.dtype)
        return out if img.ndim == 3 else out[:, :, 0]
    (iy, wy), (ix, wx) = _antialias_axis(in_h, out_h), _antialias_axis(in_w, out_w)
    t = np.zeros((out_h, in_w, f.shape[2]))
    for j in range(iy.shape[1]):                        # t[x] = sum_y wy * f[y][x], ascending y
        t = t + wy[:, j, None, None] * f[iy[:, j]].astype(np.float64)
    v = np.zeros((out_h, out_w, f.shape[2]))
    for j in range(ix.shape[1]):                        # v = sum_x wx * t[x], ascending x
        v = v + wx[None, :, j, None] * t[:, ix[:, j]]
    out = np.floor(v + 0.5).clip(0, full).astype(img.dtype)
    return out if img.ndim == 3 else out[:, :, 0]


# 16.16 fixed point: (luma, Cb, Cr, Yoff) of the two matrices of include/ideepcolor.h's YCbCr rule
YCC_MATRICES = {
    "jfif": ((19595, 38470, 7471), (-11059, -21709, 32768), (32768, -27439, -5329), 0),        # BT.601 full range, libjpeg's jccolor.c
    "bt709": ((11966, 40254, 4064), (-6596, -22189, 28785), (28784, -26145, -2639), 16),       # BT.709 limited range
}


def rgb_to_ycc420(rgb, format="i420", matrix="jfif"):
    """The host twin of the device's YCbCr 4:2:0 output (``HipColorizer.set_batch_output``; the rule: include/ideepcolor.h): rgb (h,w,3) uint8
    -> one uint8 block of h*w + 2*ch*cw bytes, ch = (h+1)//2, cw = (w+1)//2: Y [h,w], then Cb [ch,cw] and Cr [ch,cw] ('i420') or
    [ch,cw,2] interleaved ('nv12').  Integers only: Y = ((y.(R,G,B) + 32768) >> 16) + Yoff per pixel; a chroma block is the 2 x 2 pixels
    clipped at the image's edge (k = 1, 2 or 4), C = (sum of c.(R,G,B) + k * ((128 << 16) + 32767)) >> (16 + log2 k)."""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.size == 0:
        raise ValueError("rgb_to_ycc420 needs a uint8 (h,w,3) image, got %s %s" % (rgb.dtype, rgb.shape))
    if format not in ("i420", "nv12"):
        raise ValueError("format is 'i420' or 'nv12', got %r" % (format,))
    my, mcb, mcr, yoff = YCC_MATRICES[matrix]
    h, w = rgb.shape[:2]
    ch, cw = (h + 1) // 2, (w + 1) // 2
    p = rgb.astype(np.int64)
    y = ((p @ np.array(my, np.int64) + 32768) >> 16) + yoff
    ones = np.zeros((2 * ch, 2 * cw), np.int64)
    ones[:h, :w] = 1
    k = ones.reshape(ch, 2, cw, 2).sum(axis=(1, 3))
    shift = 16 + (k == 2) + 2 * (k == 4)
    planes = []
    for m in (mcb, mcr):
        s = np.zeros((2 * ch, 2 * cw), np.int64)
        s[:h, :w] = p @ np.array(m, np.int64)
        planes.append((s.reshape(ch, 2, cw, 2).sum(axis=(1, 3)) + k * ((128 << 16) + 32767)) >> shift)
    chroma = np.stack(planes, axis=-1) if format == "nv12" else np.stack(planes, axis=0)
    return np.concatenate([y.reshape(-1), chroma.reshape(-1)]).astype(np.uint8)


def ycc420_to_rgb(buf, h, w, format="i420", matrix="jfif"):
    """The inverse of ``rgb_to_ycc420`` for display: every chroma sample is repeated over its block (nearest), the matrix is inverted in
    float64 and the result rounded and clamped to uint8 -> (h,w,3).  Not bit-exact: 4:2:0 discards chroma resolution."""
    h, w = int(h), int(w)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    buf = np.asarray(buf, np.uint8).reshape(-1)
    if buf.size < h * w + 2 * ch * cw:
        raise ValueError("ycc420_to_rgb needs %d bytes, got %d" % (h * w + 2 * ch * cw, buf.size))
    my, mcb, mcr, yoff = YCC_MATRICES[matrix]
    y = buf[:h * w].reshape(h, w).astype(np.float64) - yoff
    c = buf[h * w:h * w + 2 * ch * cw]
    if format == "nv12":
        cb, cr = c.reshape(ch, cw, 2)[..., 0], c.reshape(ch, cw, 2)[..., 1]
    elif format == "i420":
        cb, cr = c[:ch * cw].reshape(ch, cw), c[ch * cw:].reshape(ch, cw)
    else:
        raise ValueError("format is 'i420' or 'nv12', got %r" % (format,))
    up = lambda a: np.repeat(np.repeat(a.astype(np.float64) - 128.0, 2, axis=0), 2, axis=1)[:h, :w]
    ycc = np.stack([y, up(cb), up(cr)], axis=-1)
    inv = np.linalg.inv(np.array([my, mcb, mcr], np.float64) / 65536.0)
    return np.clip(np.floor(ycc @ inv.T + 0.5), 0, 255).astype(np.uint8)


def imread_rgb(path):
    """``cv2.cvtColor(cv2.imread(path, 1), cv2.COLOR_BGR2RGB)`` -> (H,W,3) uint8 RGB."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB")).copy()


def imread_gray_or_rgb(path):
    """``imread_rgb`` that keeps a single-channel file single-channel: PIL modes L -> (H,W) uint8, I;16 (either byte order) -> (H,W)
    uint16 in native order; every other mode -> (H,W,3) uint8 RGB."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode == "L":
            return np.asarray(im).copy()
        if im.mode.startswith("I;16"):
            return np.asarray(im).astype(np.uint16)
        return np.asarray(im.convert("RGB")).copy()
