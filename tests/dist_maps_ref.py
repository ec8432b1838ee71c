"""float64 numpy restatement of the two device read-outs of the resident colour distribution (include/ideepcolor.h:
idc_dist_entropy, idc_dist_decode), applied to a given float32 tensor p of shape (n, B, Hd, Wd).  Not a test module."""
import numpy as np


def _p64(p):
    p = np.asarray(p)
    assert p.dtype == np.float32 and p.ndim == 4
    return p.astype(np.float64)


def entropy(p):
    """sum_q p log p over the bin axis (the reference's sign), bins with p == 0 contributing 0: (n, Hd, Wd) float64."""
    p = _p64(p)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(p > 0, p * np.log(p), 0.0).sum(axis=1)


def decode_mode(p, centres):
    """Centre of the arg-max bin (first maximum): ab (n, 2, Hd, Wd) float32 and conf = p_max (n, Hd, Wd) float32."""
    p = np.asarray(p)
    assert p.dtype == np.float32
    centres = np.asarray(centres, np.float32)
    return np.moveaxis(centres[np.argmax(p, axis=1)], -1, 1), p.max(axis=1)


def decode_mean(p, centres, gamma):
    """ab = sum_q w_q c_q / sum_q w_q with w_q = exp(gamma (log p_q - log p_max)), w_q = 0 where p_q == 0: (n, 2, Hd, Wd)
    float64.  gamma is taken as the float32 the C ABI receives."""
    p = _p64(p)
    g = float(np.float32(gamma))
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(p > 0, np.exp(g * (np.log(p) - np.log(p.max(axis=1, keepdims=True)))), 0.0)
    c = np.asarray(centres, np.float32).astype(np.float64)
    return np.einsum("nbhw,bc->nchw", w, c) / w.sum(axis=1)[:, None]
