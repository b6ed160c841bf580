"""The reference's C-grid group restated in numpy, OPERATOR FOR OPERATOR -- what the kernels of
csrc/momlevel_vort.hip must reproduce bit for bit: ``calc_rel_vort`` (src/momlevel/derived.py:
232-239), ``calc_pv`` (:538-556), ``calc_coriolis`` (:177) and ``calc_rossby_rd`` (:588), with
xgcm's ``grid.diff`` / ``grid.interp(boundary="fill")`` written out (xgcm is not installed):

* non-symmetric grid (``center -> right``): ``out[k] = f[k+1] - f[k]`` with ONE padded element, the
  literal 0.0, past the end; ``interp`` is ``0.5 * (f[k] + f[k+1])`` on the same padded array;
* symmetric grid (``center -> outer``): ``out[k] = f[k] - f[k-1]`` for k = 0..n, both
  out-of-range elements 0.0; ``interp`` is ``0.5 * (f[k-1] + f[k])`` on the same padded array.

Every function takes and returns plain numpy arrays whose last two axes are (y, x); dtypes are
left to numpy's promotion -- that IS the specification of the kernels' arithmetic.  ``periodic``
pads by wrapping instead: NOT the reference (its ``cm`` pin is 584073.76, wrapping gives
851037.06); tests/test_vort_host.py uses it to guard the reading."""

import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def goldens():
    with open(os.path.join(GOLDEN, "vort_goldens.json")) as f:
        return json.load(f)


def _padded(f, axis, symmetric, periodic=False):
    """``f`` with the padding ``boundary="fill"`` (fill value 0.0) gives it along ``axis``"""
    width = [(0, 0)] * f.ndim
    width[axis] = (1, 1) if symmetric else (0, 1)
    return np.pad(f, width, mode="wrap" if periodic else "constant")


def _pair(f, axis, symmetric, periodic=False):
    """(f[k], f[k+1]) of the padded array: the two neighbours of every output point"""
    p = _padded(f, axis, symmetric, periodic)
    n = p.shape[axis]
    lo = np.take(p, np.arange(0, n - 1), axis=axis)
    hi = np.take(p, np.arange(1, n), axis=axis)
    return lo, hi


def diff(f, axis, symmetric=False, periodic=False):
    lo, hi = _pair(f, axis, symmetric, periodic)
    return hi - lo


def interp(f, axis, symmetric=False, periodic=False):
    lo, hi = _pair(f, axis, symmetric, periodic)
    return 0.5 * (lo + hi)


def rel_vort(u, v, dx, dy, area, symmetric=False, periodic=False):
    """(-diff_Y(u * dx) + diff_X(v * dy)) / area                                 derived.py:232-239"""
    return (-diff(u * dx, -2, symmetric, periodic) + diff(v * dy, -1, symmetric, periodic)) / area


def interp_n2(n2, symmetric=False, periodic=False):
    """grid.interp(n2, axis=["X", "Y"], boundary="fill"): along X first, then along Y"""
    return interp(interp(n2, -1, symmetric, periodic), -2, symmetric, periodic)


def pv(zeta, coriolis, n2, gravity=9.8, symmetric=False, units="m", interp=True, periodic=False):
    """derived.py:538-563; ``gravity`` a python float (weak: it takes n2's dtype)"""
    if interp:
        n2 = interp_n2(n2, symmetric, periodic)
    out = (zeta + coriolis) * (n2 / gravity)
    if units == "cm":
        out = np.abs(((out / 100) * 1.0e14))
    elif units != "m":
        raise ValueError(f"unknown units option `{units}`")
    return out


def coriolis(lat):
    return 2.0 * (2.0 * np.pi / (60.0 * 60.0 * 24.0)) * np.sin(lat * np.pi / 180.0)


def rossby_rd(wave_speed, f):
    """``f`` already shaped to broadcast against ``wave_speed``"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return wave_speed / np.abs(f)
