"""The reference for image ingestion on the device (idc_set_image_rgb / idc_fullres_rgb), made of code that is not under test:
``colorspace.resize_bilinear_u8`` (the wrapper's own host resize, the rule the kernel has to reproduce bit for bit), the oracle's
``rgb2lab`` / ``lab2rgb_transpose`` (pinned to skimage golden vectors by tests/test_colorspace.py) and ``scipy.ndimage.zoom``."""
import os

import numpy as np
from scipy.ndimage import zoom

from interactive_deep_colorization_amd import colorspace
from oracle import colorspace as ocs

HERE = os.path.dirname(os.path.abspath(__file__))


def mortar():
    return np.load(os.path.join(HERE, "golden", "mortar_pestle_256_rgb.npy"))


def source_image(h, w, seed):
    """(h, w, 3) uint8: a crop of the golden photograph where it fits (smooth content: real interpolation weights), seeded noise otherwise."""
    rs = np.random.RandomState(seed)
    if h <= 256 and w <= 256 and seed % 2 == 0:
        y, x = rs.randint(0, 256 - h + 1), rs.randint(0, 256 - w + 1)
        return mortar()[y:y + h, x:x + w].copy()
    return rs.randint(0, 256, (h, w, 3)).astype(np.uint8)


def net_rgb(src, H, W):
    """[H,W,3] uint8: what load_image feeds the net (colorize_image.py:58 through the wrapper's restatement of cv2.resize)."""
    return colorspace.resize_bilinear_u8(src, H, W)


def net_lab(rgb_net):
    """[3,H,W] float64 Lab of a net-size image."""
    return ocs.rgb2lab(rgb_net).transpose((2, 0, 1))


def zoom_to(planes, sh, sw, order):
    """[C,H,W] -> [C,sh,sw] as the full-resolution getters do it (colorize_image.py:123-158)."""
    planes = np.asarray(planes, np.float64)
    out = zoom(planes, (1, 1. * sh / planes.shape[1], 1. * sw / planes.shape[2]), order=order)
    assert out.shape == (planes.shape[0], sh, sw), out.shape
    return out


def fullres(src, ab=None, order=1, mask=None, mask_value=1.0):
    """[sh,sw,3] uint8: Lab -> RGB of L = rgb2lab(src)[..., 0] (mask None) or 50 * zoom(mask / mask_value, order 0), with ab [2,H,W]
    zoomed to the source size by ``order`` (None: zeros)."""
    sh, sw = src.shape[:2]
    if mask is None:
        L = ocs.rgb2lab(src)[..., 0][None]
    else:
        L = 50 * zoom_to(np.asarray(mask, np.float64) / mask_value, sh, sw, 0)
    ab_full = np.zeros((2, sh, sw)) if ab is None else zoom_to(ab, sh, sw, order)
    return ocs.lab2rgb_transpose(L, ab_full)


def close_u8(got, want, frac=2e-4):
    """The bound of test_upsample_lab2rgb_display_and_fullres: at most one uint8 level on at most ``frac`` of the values.  Returns the figures."""
    d = np.abs(np.asarray(got).astype(np.int32) - np.asarray(want).astype(np.int32))
    return int(d.max()), float((d > 0).mean())
