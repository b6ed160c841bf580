"""spatial - horizontal smoothing of a ``(..., yh, xh)`` record on the GPU: area-weighted,
land-aware box and Gaussian filters, a fixed length scale on a converging grid, and the high-pass
residual.

EXTENSION: momlevel has no such functions.  They are the one step of a sea-level analysis that is
left between a device-resident record and a figure: the mesoscale against the large scale
(``highpass``: eta - smooth(eta)), a trend or EOF map smoothed before it is looked at, a local
steric field coarse-grained to the scale of a tide-gauge or altimetry comparison.  In xarray this is
``gcm-filters``, or a ``rolling`` over two dims weighted by ``areacello`` with the land masked out;
neither is importable where the tests run, so parity with them is UNPINNED: the specification is
the numpy restatement tests/smooth_numpy.py, which the kernels (csrc/momlevel_smooth.hip,
``core.plane_smooth``) are gated against bit for bit.

All of it is ONE operator (include/momlevel_smooth.h states the contract): a separable, normalised
convolution over the two trailing dims,

    smooth[j, i] = sum_l wy[l] sum_k wx[r, k] area[r, c] v[r, c]
                   / sum_l wy[l] sum_k wx[r, k] area[r, c],     r = j - lead_y + l, c = i - lead_x + k

over the VALID cells of the window -- neither value nor area NaN, area positive -- with x periodic
or closed and the y edges closed, in float64 with k and l ascending.  ``wx`` is one row of weights,
or a table with one row per source row: that is how a fixed length scale becomes a wider index
window at high latitude (``length_scale_weights``).  The weights are made here, on the host.

Records are independent: a device record gives a device result, a large host or lazy record goes
up and comes back in groups of whole leading rows, and the grouping cannot show in the result.

NOT BUILT: the tripolar north fold (the north and south edges are closed) and tiles spread over
several ranks, which need a halo exchange.
"""

import numpy as np
import torch

from . import core, derived, engine, hostio
from .adapters import accepts_xarray
from .labeled import DataArray, Dataset, check_field_dtype

__all__ = ["smooth", "highpass", "boxcar_weights", "gaussian_weights", "length_scale_weights"]


# ---------------------------------------------------------------------------------------
# the weights: functions of the window alone, made on the host
# ---------------------------------------------------------------------------------------
def _width(width):
    if int(width) != width or int(width) < 1:
        raise ValueError(f"a window is a whole number of cells >= 1, got {width}")
    return int(width)


def boxcar_weights(width):
    """``width`` equal weights that sum to 1 (float64)."""
    width = _width(width)
    return np.full(width, 1.0 / width, dtype=np.float64)


def gaussian_weights(sigma_cells, truncate=3.0):
    """Gaussian weights ``exp(-k^2 / (2 sigma^2))``, k = -m .. m with ``m = max(1, round(truncate *
    sigma_cells))``, divided by their sum: ``2m + 1`` symmetric float64 weights."""
    sigma, truncate = float(sigma_cells), float(truncate)
    if not (np.isfinite(sigma) and sigma > 0.0):
        raise ValueError(f"sigma_cells must be a positive number of cells, got {sigma_cells}")
    if not (np.isfinite(truncate) and truncate > 0.0):
        raise ValueError(f"truncate must be positive, got {truncate}")
    m = max(1, int(truncate * sigma + 0.5))
    k = np.arange(-m, m + 1, dtype=np.float64)
    w = np.exp(-0.5 * (k / sigma) ** 2)
    return w / np.sum(w)


def length_scale_weights(scale, dx_rows, kind="gaussian"):
    """The ``(ny, Wx)`` table of x weights for a length ``scale`` in the units of ``dx_rows``, the
    nominal x spacing of every row: row r holds ``gaussian_weights(scale / dx_rows[r])`` or
    ``boxcar_weights`` of the odd width nearest ``scale / dx_rows[r]``, zero-padded symmetrically
    to the widest window of the table -- where the grid converges the same length is more cells."""
    if kind not in ("gaussian", "boxcar"):
        raise ValueError(f"kind must be 'gaussian' or 'boxcar', got '{kind}'")
    scale = float(scale)
    dx = np.asarray(dx_rows, dtype=np.float64)
    if dx.ndim != 1 or dx.size < 1:
        raise ValueError("dx_rows must hold one spacing per row of the plane")
    if not (np.isfinite(scale) and scale > 0.0):
        raise ValueError(f"scale must be a positive length, got {scale}")
    if not (np.all(np.isfinite(dx)) and np.all(dx > 0.0)):
        raise ValueError("dx_rows must be positive and finite")
    if kind == "gaussian":
        rows = [gaussian_weights(scale / d) for d in dx]
    else:
        rows = [boxcar_weights(2 * int(scale / d / 2.0) + 1) for d in dx]
    W = max(r.size for r in rows)
    table = np.zeros((dx.size, W), dtype=np.float64)
    for r, w in enumerate(rows):
        pad = (W - w.size) // 2
        table[r, pad:pad + w.size] = w
    return table


# ---------------------------------------------------------------------------------------
# one call's plan: checked on the host before any upload
# ---------------------------------------------------------------------------------------
class _Plan:
    def __init__(self, areacello, weights_x, weights_y, periodic_x, min_count, fill, center):
        self.named = isinstance(areacello, DataArray)  # (else the plane is the record's last two dims)
        if not self.named:
            areacello = DataArray(areacello, ("yh", "xh") if len(np.shape(areacello)) == 2 else None)
        if areacello.ndim != 2:
            raise ValueError(f"areacello has dims {areacello.dims}: a 2-D (ydim, xdim) field is "
                             "expected")
        self.src = areacello
        self.dims = tuple(areacello.dims)
        self.shape = tuple(int(n) for n in areacello.shape)
        name = derived.float_name(areacello, "areacello", allow_other=True)
        # (a device-resident map is small: downloaded for the check)
        self.area = np.ascontiguousarray(areacello.values,
                                         dtype=np.float32 if name == "float32" else np.float64)
        if np.any(self.area < 0):  # (NaN compares False: it carries no weight)
            raise ValueError("areacello holds negative areas")
        if np.any(np.isinf(self.area)):
            raise ValueError("areacello holds infinite areas")
        ny, nx = self.shape
        wx = np.asarray(weights_x, dtype=np.float64)
        if weights_y is None:
            if wx.ndim != 1:
                raise ValueError("a table of x weights needs weights_y: one row cannot serve both")
            weights_y = wx
        self.wx, self.wy = core.smooth_weights(wx, weights_y, ny, nx)
        Wx, Wy = self.wx.shape[-1], self.wy.shape[0]
        if center:
            if Wx % 2 == 0 or Wy % 2 == 0:
                raise ValueError(f"a centred window is odd each way, got {Wy} x {Wx}: pass "
                                 "center=False for a window that ends at its cell")
            self.lead_x, self.lead_y = Wx // 2, Wy // 2
        else:
            self.lead_x, self.lead_y = Wx - 1, Wy - 1
        if int(min_count) != min_count or not 1 <= int(min_count) <= Wx * Wy:
            raise ValueError(f"min_count must lie in [1, {Wx * Wy}], got {min_count}")
        self.min_count = int(min_count)
        self.periodic_x, self.fill = bool(periodic_x), bool(fill)
        self._on = {}

    def on(self, dev):
        """(area, wx, wy) on ``dev``: uploaded once per device"""
        key = str(dev)
        if key not in self._on:
            f64 = lambda a: hostio.to_device(a, dev, torch.float64).contiguous()  # noqa: E731
            self._on[key] = (engine.to_device(self.area, dev).contiguous(), f64(self.wx), f64(self.wy))
        return self._on[key]

    def launch(self, v, dev, residual):
        area, wx, wy = self.on(dev)
        return core.plane_smooth(v, area, wx, wy, self.lead_x, self.lead_y, self.periodic_x,
                                 self.min_count, fill=self.fill, residual=residual)


def _records(da, plan, residual):
    """one DataArray through ``core.plane_smooth`` -> the raw result, of the input's shape and of
    the record's dtype (integers as float64): on the device for a device record, on the host
    otherwise"""
    ydim, xdim = plan.dims if plan.named or da.ndim < 2 else da.dims[-2:]
    derived.check_trailing(da, ydim, xdim, da.name or "the record")
    if tuple(int(n) for n in da.shape[-2:]) != plan.shape:
        raise ValueError(f"the record's plane {tuple(da.shape[-2:])} is not areacello's {plan.shape}")
    name = check_field_dtype(da.dtype, "records")
    tdt = torch.float32 if name == "float32" else torch.float64  # (integers compute as float64)
    ndt = np.float32 if name == "float32" else np.float64
    lead = tuple(int(n) for n in da.shape[:-2])
    nrec = int(np.prod(lead, dtype=np.int64))
    ny, nx = plan.shape
    dev = engine.device_of(da.data, plan.src.data)

    if not da.is_device and len(lead) >= 1 and hostio.wants_pipeline(lead[0], nrec * ny * nx):
        # a large host / lazy record: groups of whole leading rows; a lazy record is never
        # materialised whole.  A record's result depends on that record alone.
        inner = nrec // lead[0]
        source = da.data if da.is_lazy else da.values

        def kernel(tensors, i0, i1):
            v = tensors[0].to(tdt).reshape((i1 - i0) * inner, ny, nx)
            return plan.launch(v, dev, residual).reshape((i1 - i0,) + lead[1:] + (ny, nx))

        return hostio.pipeline_rows(hostio.row_bounds(lead[0], inner * ny * nx), dev,
                                    hostio.leading_slices([source]), kernel,
                                    np.empty(lead + (ny, nx), dtype=ndt))

    # (a device record is read where it lives; only a host record goes through hostio)
    v = da.data.to(tdt) if da.is_device else engine.to_device(da.values, dev, tdt)
    res = plan.launch(v.reshape(nrec, ny, nx).contiguous(), dev, residual).reshape(lead + (ny, nx))
    return res if da.is_device else hostio.to_host(res)


def _labelled(da, plan, residual):
    out = DataArray(_records(da, plan, residual), da.dims, dict(da.coords), dict(da.attrs), da.name)
    out.encoding = dict(da.encoding)
    return out


def _apply(xobj, plan, residual):
    if isinstance(xobj, DataArray):
        return _labelled(xobj, plan, residual)
    if isinstance(xobj, Dataset):
        out = Dataset(attrs=xobj.attrs)
        for name, c in xobj.coords.items():
            out._set(name, c, is_coord=True)
        for name, var in xobj.data_vars.items():
            plane = all(d in var.dims for d in plan.dims) and var.dtype.kind in "fiub"
            out[name] = _labelled(var, plan, residual) if plane else var
        return out
    if isinstance(xobj, (np.ndarray, torch.Tensor)):
        if xobj.ndim < 2:
            raise ValueError("a record has at least the two dims of the plane")
        dims = tuple(f"dim_{i}" for i in range(xobj.ndim - 2)) + plan.dims
        return _labelled(DataArray(xobj, dims), plan, residual).data
    raise TypeError("Input must be a DataArray, a Dataset, a numpy array or a device tensor")


# ---------------------------------------------------------------------------------------
# public functions
# ---------------------------------------------------------------------------------------
@accepts_xarray
def smooth(xobj, areacello, weights_x, weights_y=None, periodic_x=True, min_count=1, fill=False,
           center=True):
    """Area-weighted, land-aware smoothing over the horizontal plane (EXTENSION: not in momlevel;
    parity with gcm-filters / a weighted 2-D ``rolling`` is unpinned -- the specification is the
    module docstring and tests/smooth_numpy.py).

    ``areacello`` is the 2-D ``(ydim, xdim)`` cell area (float32 / float64; NaN or 0 = land, no
    weight; negative or infinite values a ``ValueError``).  ``xobj``: a DataArray whose LAST two
    dims are those, with any leading dims (each leading index is a record of its own); a Dataset
    (every numeric variable with the two dims is smoothed, the others pass through); or a numpy
    array / device tensor ``(..., ny, nx)``, answered in kind.  The result has the record's dims,
    coords, attrs and dtype (float32 is the float64 result rounded once; integers give float64).

    ``weights_x``: the x weights, ``(Wx,)`` -- ``boxcar_weights``, ``gaussian_weights``, any finite
    numbers -- or a ``(ny, Wx)`` table with one row per row of the plane
    (``length_scale_weights``).  ``weights_y``: ``(Wy,)``, default ``weights_x`` (a table needs it
    spelled out).  ``center=True`` wants odd windows and centres them; ``center=False`` ends the
    window at its cell.  ``periodic_x`` wraps x (the window may not be wider than the plane); the
    north and south edges are closed: the tripolar fold is not built.

    A cell is valid when its value is not NaN and its area is positive.  Invalid cells are left out
    and the weights present renormalised; fewer than ``min_count`` valid cells in the window give
    NaN.  A cell that is not valid itself stays NaN unless ``fill``."""
    plan = _Plan(areacello, weights_x, weights_y, periodic_x, min_count, fill, center)
    return _apply(xobj, plan, False)


@accepts_xarray
def highpass(xobj, areacello, weights_x, weights_y=None, periodic_x=True, min_count=1, fill=False,
             center=True):
    """``xobj - smooth(xobj, ...)`` (EXTENSION, see ``smooth``): the small scales, formed in the
    same pass -- one float64 subtraction per cell, so for a float64 record ``smooth + highpass`` is
    the record again wherever both are defined.  NaN at every cell that is not valid, with or
    without ``fill``."""
    plan = _Plan(areacello, weights_x, weights_y, periodic_x, min_count, fill, center)
    return _apply(xobj, plan, True)
