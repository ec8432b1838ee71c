"""The colour picker's gamut maths: the surface of the reference's ``data/lab_gamut.py`` without scikit-image.

``ui/gui_draw.py:11`` and ``ui/gui_gamut.py:4`` import ``lab_gamut`` for ``abGrid`` (the ab plane at one lightness, masked
to the colours sRGB can show) and ``snap_ab`` (an arbitrary colour pulled into the gamut at a given lightness).  Same
names, argument names and defaults as the reference module; the code is this package's own, on this package's colour
functions (``colorspace.rgb2lab`` / ``lab2rgb``).

Two routes.  With no engine bound -- the default, nothing binds one implicitly -- everything runs on the host in numpy:
a working ``lab_gamut`` on any machine.  After ``set_engine(engine)`` (an ``engine.HipColorizer``, e.g. ``colorModel.net``)
``abGrid.update_gamut``, ``snap_ab`` and ``snap_ab_many`` run on the device through ``idc_gamut_map`` /
``idc_snap_colors``; ``set_engine(None)`` goes back to the host.  A grid whose ``gamut_size`` or ``D`` is not an integer,
or lies outside the library's limits (1..512, 1..gamut_size), takes the host route either way.

Extras, not in the reference: ``set_engine`` / ``get_engine`` and ``snap_ab_many`` (n colours in one call).

DEVIATIONS.  The reference calls ``warnings.filterwarnings("ignore")`` inside its functions, which silences every warning
of the whole process from then on; this module leaves the warning filters alone.  Integer colours of any dtype are read as
0..255 levels (the GUI passes uint8).

PARITY UNPINNED against scikit-image itself, which is not installable beside this package: the colour functions follow
the published sRGB / D65 formulas skimage uses; the tests compare both routes with
``tests/gamut_ref.py``, a float64 restatement on ``oracle/colorspace.py``.
"""
import numpy as np

from . import colorspace

_ENGINE = None
_MAX_GAMUT_SIZE, _MAX_COLORS = 512, 65536      # idc_gamut_map / idc_snap_colors limits (include/ideepcolor.h)
_SNAP_ROUNDS = 20


def set_engine(engine):
    """Bind the engine (``engine.HipColorizer``) whose device runs ``update_gamut`` / ``snap_ab`` / ``snap_ab_many``; None = the host."""
    global _ENGINE
    _ENGINE = engine


def get_engine():
    return _ENGINE


def _levels(rgb):
    """A colour as the reference's callers pass it: integer dtypes are 0..255 levels, floats are [0, 1] (skimage's rule)."""
    arr = np.asarray(rgb)
    return arr.astype(np.uint8) if arr.dtype.kind in 'iub' else arr


def qcolor2lab_1d(qc):
    """A QColor -> its (3,) Lab value."""
    return rgb2lab_1d(np.array((qc.red(), qc.green(), qc.blue()), dtype=np.uint8))


def rgb2lab_1d(in_rgb):
    """(3,) uint8 (or float in [0, 1]) -> (3,) float64 Lab."""
    return colorspace.rgb2lab(np.asarray(in_rgb).reshape(1, 1, 3)).reshape(3)


def lab2rgb_1d(in_lab, clip=True, dtype='uint8'):
    """(3,) Lab -> (3,) sRGB: uint8 levels rounded half to even, or floats in [0, 1] for any other ``dtype``.  (``colorspace.lab2rgb``
    clips to [0, 1] itself, as skimage's does, so ``clip`` changes nothing; it is kept for the signature.)"""
    srgb = colorspace.lab2rgb(np.asarray(in_lab, np.float64).reshape(1, 1, 3)).reshape(3)
    if clip:
        srgb = np.clip(srgb, 0, 1)
    return np.round(srgb * 255).astype('uint8') if dtype == 'uint8' else srgb


def _snap_host(input_l, input_rgb):
    """The loop of ``snap_ab``: the colour's (a, b) at lightness input_l, sent through Lab -> clipped sRGB -> Lab until it stops moving
    (sum |delta| < 1) or 20 rounds have run.  L is replaced by input_l only at the start of a round, so the Lab that leaves the loop
    carries the round-tripped L (as in the reference)."""
    lab = rgb2lab_1d(_levels(input_rgb))
    for _ in range(_SNAP_ROUNDS):
        start = np.array((input_l, lab[1], lab[2]), np.float64)
        lab = colorspace.rgb2lab(colorspace.lab2rgb(start))
        if np.sum(np.abs(lab - start)) < 1:
            break
    return lab2rgb_1d(lab)


def snap_ab(input_l, input_rgb, return_type='rgb'):
    """Given a lightness and an RGB colour, snap the colour to where (input_l, a, b) is in gamut: (3,) uint8 for return_type 'rgb',
    its (3,) float64 Lab for 'lab', None for anything else."""
    if return_type not in ('rgb', 'lab'):
        return None
    out = snap_ab_many([input_l], np.asarray(_levels(input_rgb)).reshape(1, 3), return_type)
    return out[0]


def snap_ab_many(ls, rgbs, return_type='rgb'):
    """``snap_ab`` for n colours: ls (n,), rgbs (n,3) -> (n,3) uint8 ('rgb') or (n,3) float64 Lab ('lab'); one device call when an
    engine is bound (in pieces of 65536)."""
    if return_type not in ('rgb', 'lab'):
        return None
    ls = np.asarray(ls, np.float64).reshape(-1)
    rgbs = np.asarray(_levels(rgbs)).reshape(-1, 3)
    if ls.shape[0] != rgbs.shape[0]:
        raise ValueError("%d lightness values for %d colours" % (ls.shape[0], rgbs.shape[0]))
    want_lab = return_type == 'lab'
    n = ls.shape[0]
    if _ENGINE is not None and n > 0 and rgbs.dtype == np.uint8:
        parts = []
        for i in range(0, n, _MAX_COLORS):
            r = _ENGINE.snap_colors(ls[i:i + _MAX_COLORS], rgbs[i:i + _MAX_COLORS], want_lab=want_lab)
            parts.append(r[1] if want_lab else r)
        return parts[0] if len(parts) == 1 else np.concatenate(parts)
    out = np.empty((n, 3), np.float64 if want_lab else np.uint8)
    for k in range(n):
        rgb = _snap_host(ls[k], rgbs[k])
        out[k] = rgb2lab_1d(rgb) if want_lab else rgb
    return out


class abGrid():
    """The (a, b) plane on a regular grid: ``pts_full_grid[i, j] = (a_i, b_j)``, rows are a, columns are b."""

    def __init__(self, gamut_size=110, D=1):
        axis = np.arange(-gamut_size, gamut_size + D, D)
        self.vals_a, self.vals_b = np.meshgrid(axis, axis, indexing='ij')
        self.pts_full_grid = np.stack((self.vals_a, self.vals_b), axis=2)
        self.A, self.B = self.pts_full_grid.shape[:2]
        self.AB = self.A * self.B
        self.gamut_size = gamut_size
        self.D = D

    def _on_device(self):
        g, d = self.gamut_size, self.D
        return (_ENGINE is not None and isinstance(g, (int, np.integer)) and isinstance(d, (int, np.integer))
                and 1 <= g <= _MAX_GAMUT_SIZE and 1 <= d <= g)

    def update_gamut(self, l_in):
        """The grid's colours at lightness l_in: ``pts_rgb`` (A,B,3) uint8 (truncated), ``mask`` (A,B) bool = the uint8 colour lies
        within 1.0 of the grid point in Lab, ``masked_rgb`` = pts_rgb with everything outside the mask white.  Returns (masked_rgb, mask)."""
        if self._on_device() and np.ndim(l_in) == 0 and np.isfinite(l_in):
            masked, mask, pts = _ENGINE.gamut_map(float(l_in), int(self.gamut_size), int(self.D), want_pts=True)
            self.pts_rgb, self.mask, self.masked_rgb = pts[0], mask[0], masked[0]
            return self.masked_rgb, self.mask
        lab = np.empty((self.A, self.B, 3), np.float64)
        lab[..., 0] = l_in
        lab[..., 1:] = self.pts_full_grid
        self.pts_rgb = (255 * colorspace.lab2rgb(lab)).astype('uint8')            # truncation; lab2rgb clips to [0, 1]
        self.mask = np.linalg.norm(lab - colorspace.rgb2lab(self.pts_rgb), axis=2) < 1.0
        self.masked_rgb = np.where(self.mask[..., None], self.pts_rgb, np.uint8(255))
        return self.masked_rgb, self.mask

    def ab2xy(self, a, b):
        """Grid coordinates (x = column, y = row) of the colour (a, b), in units of one ab step from the corner."""
        return self.gamut_size + b, self.gamut_size + a

    def xy2ab(self, x, y):
        return y - self.gamut_size, x - self.gamut_size
