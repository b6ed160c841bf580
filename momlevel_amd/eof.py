"""eof.py -- the leading modes of variability of a ``(time, yh, xh)`` record on the MI355X: the time
covariance matrix, the EOFs with their principal components, and the projection of another record
onto them.

AN EXTENSION, in the sense of ``regional``: momlevel has no such function.  It is the step after
the trends, climatologies, filters and regional means -- the one that couples all cells: the ENSO
pattern of steric height, the share of variance in the first mode.  In the xarray world this is
the ``eofs`` package; it is not importable where the tests run, so parity with it is UNPINNED: the
specification is the numpy restatement tests/eof_numpy.py, which the kernel
(csrc/momlevel_eof.hip) and this module are gated against.

The method is the time-covariance ("snapshot") one: with ``a`` the anomaly of every cell from its
own time mean, ``nt`` steps and ``N = nt - ddof``::

    G[s, t]   = sum_c area[c] * a[s, c] * a[t, c]          one contraction over the cells
    C         = G / N                                      (time, time)
    C u_k     = lambda_k u_k                               numpy.linalg.eigh on the host: nt x nt
    pc_k      = u_k * sqrt(N)                              unit variance; sign: largest |.| positive
    E_k[c]    = sum_t pc_k[t] * a[t, c] / N                the covariance map, the record's units
    a[t, c]  ~= sum_k pc_k[t] * E_k[c]

``G`` is ``core.time_gram`` -- the float64 matrix cores, the anomalies formed while the rows are
staged (no second buffer the size of the record), a fixed order of summation; the maps are
``core.time_project``.  A cell with a missing step (NaN) or without a positive area carries no
weight and its maps are NaN.  A record that lives on the device stays there: what crosses the host
link is the ``nt x nt`` matrix, for the eigen-decomposition.  A host record is uploaded whole.
"""

import numpy as np
import torch

from . import _lib, core, engine, hostio
from .adapters import accepts_xarray
from .labeled import DataArray, Dataset, check_field_dtype

__all__ = ["calc_eofs", "project_field", "time_covariance"]

MODES_PER_PASS = _lib.TREND_MAX_TERMS  # the columns one core.time_project pass takes


# ---------------------------------------------------------------------------------------
# host rules: pure functions of small arrays
# ---------------------------------------------------------------------------------------
def fix_signs(pcs):
    """``pcs`` (time, mode) with every column's element of largest magnitude positive -- the lowest
    index on ties"""
    pcs = np.array(pcs, dtype=np.float64)
    for k in range(pcs.shape[1]):
        if pcs[np.argmax(np.abs(pcs[:, k])), k] < 0:
            pcs[:, k] = -pcs[:, k]
    return pcs


def north_error(eigenvalues, nt):
    """North et al. (1982): the sampling error of an eigenvalue, ``lambda * sqrt(2 / nt)``"""
    return np.asarray(eigenvalues, dtype=np.float64) * np.sqrt(2.0 / nt)


def decompose(cov, neofs, ddof=1):
    """``(eigenvalues, variance_fraction, eigenvalue_error, pcs)`` of a (time, time) covariance
    matrix: the ``neofs`` leading modes, eigenvalues descending, pcs (time, mode) of unit variance
    with the sign rule of ``fix_signs``"""
    cov = np.asarray(cov, dtype=np.float64)
    nt = cov.shape[0]
    lam, vec = np.linalg.eigh(cov)
    lam, vec = lam[::-1][:neofs].copy(), vec[:, ::-1][:, :neofs]
    pcs = fix_signs(vec * np.sqrt(nt - ddof))
    return lam, lam / np.trace(cov), north_error(lam, nt), pcs


def area_scale(areacello, shape):
    """``sqrt(area)`` as a flat float64 host array for a record whose cells have ``shape``: NaN
    where the area is NaN or not positive (the cell carries no weight); None for no area"""
    if areacello is None:
        return None
    if isinstance(areacello, DataArray):
        areacello = areacello.values
    elif isinstance(areacello, torch.Tensor):
        areacello = areacello.detach().cpu().numpy()
    area = np.asarray(areacello, dtype=np.float64)
    if tuple(area.shape) != tuple(shape):
        raise ValueError(f"areacello {tuple(area.shape)} does not cover the record's cells "
                         f"{tuple(shape)}")
    with np.errstate(invalid="ignore"):
        pos = area > 0
        return np.where(pos, np.sqrt(np.where(pos, area, 1.0)), np.nan).reshape(-1)


def _check_counts(nt, neofs, ddof):
    if ddof not in (0, 1):
        raise ValueError(f"ddof must be 0 or 1, got {ddof!r}")
    if nt - ddof < 1:
        raise ValueError(f"a record of {nt} step(s) has no covariance with ddof={ddof}")
    if neofs is not None and not 1 <= int(neofs) <= nt - 1:
        raise ValueError(f"neofs must be 1 .. nt - 1 = {nt - 1}, got {neofs}: the anomalies of "
                         f"{nt} steps span at most nt - 1 modes")


def _as_record(xobj, tcoord, what="the record"):
    """``xobj`` as a DataArray whose LEADING dim is ``tcoord``; a bare array's leading axis is
    taken to be time"""
    if isinstance(xobj, Dataset):
        raise TypeError(f"{what} must be a DataArray or an array, not a Dataset")
    if not isinstance(xobj, DataArray):
        if not isinstance(xobj, (np.ndarray, torch.Tensor)):
            raise TypeError(f"{what} must be a DataArray, a numpy array or a device tensor")
        xobj = DataArray(xobj, (tcoord,) + tuple(f"dim_{i}" for i in range(1, len(xobj.shape))))
    if xobj.ndim < 2:
        raise ValueError(f"{what} has dims {xobj.dims}: it needs '{tcoord}' and at least one cell dim")
    if tcoord not in xobj.dims:
        raise ValueError(f"{what} has dims {xobj.dims}: no '{tcoord}'")
    if xobj.dims[0] != tcoord:
        raise ValueError(f"{what} has dims {xobj.dims}: '{tcoord}' must be the leading dim")
    return xobj


# ---------------------------------------------------------------------------------------
# the device pass
# ---------------------------------------------------------------------------------------
class _Prepared:
    """a record on the device as the kernels read it, with its per-cell maps"""

    def __init__(self, da, areacello, center=None):
        name = check_field_dtype(da.dtype, "records")
        tdt = torch.float32 if name == "float32" else torch.float64  # (integers: float64)
        self.nt = int(da.shape[0])
        self.cells = tuple(int(k) for k in da.shape[1:])
        self.n = int(np.prod(self.cells, dtype=np.int64))
        if self.n < 1:
            raise ValueError("the record holds no cells")
        scale = area_scale(areacello, self.cells)  # (refusals come before any upload)
        if center is not None:
            if isinstance(center, DataArray):
                center = center.data
            if not isinstance(center, torch.Tensor):
                center = np.asarray(center, dtype=np.float64)
            if tuple(center.shape) != self.cells:
                raise ValueError(f"center {tuple(center.shape)} does not cover the record's cells "
                                 f"{self.cells}")
        self.on_device = da.is_device
        self.dev = engine.device_of(da.data)
        y = da.data.to(tdt) if self.on_device else engine.to_device(da.values, self.dev, tdt)
        self.y = y.reshape(self.nt, self.n).contiguous()
        self.scale = None if scale is None else core._f64(scale, self.dev)
        if center is None:
            center = time_mean(self.y)
        self.center = core._f64(center, self.dev).reshape(-1)

    def out(self, t):
        """a result where the record lives"""
        if self.on_device:
            return t if isinstance(t, torch.Tensor) else core._f64(t, self.dev).reshape(t.shape)
        return hostio.to_host(t) if isinstance(t, torch.Tensor) else t


def time_mean(y):
    """the per-cell time mean of a (time, cells) device record, NaN where any step is missing:
    ``core.time_project`` with a column of ``1 / nt``"""
    nt = int(y.shape[0])
    return core.time_project(y, np.full((nt, 1), 1.0 / nt))[0]


def _covariance(prep, ddof):
    """the (time, time) covariance matrix on the host"""
    G = core.time_gram(prep.y, None, prep.center, None, prep.scale)
    return hostio.to_host(G) / (prep.nt - ddof)


def _maps(prep, pcs, ddof):
    """E_k = sum_t pc_k[t] a[t, c] / N as a (mode, cells) device tensor: ``core.time_project`` on
    the RAW record, at most MODES_PER_PASS modes a pass, with the columns of P re-centred on the
    host"""
    P = pcs / (prep.nt - ddof)
    P = P - P.mean(axis=0, keepdims=True)
    out = torch.empty((P.shape[1], prep.n), dtype=torch.float64, device=prep.dev)
    for k0 in range(0, P.shape[1], MODES_PER_PASS):
        part = np.ascontiguousarray(P[:, k0:k0 + MODES_PER_PASS])
        out[k0:k0 + part.shape[1]] = core.time_project(prep.y, part)
    return out


def _time_coords(da, tcoord):
    return {k: c for k, c in da.coords.items() if tuple(c.dims) == (tcoord,)}


def _cell_coords(da, tcoord):
    return {k: c for k, c in da.coords.items() if tcoord not in c.dims}


def _mode_coord(nmode):
    return DataArray(np.arange(1, nmode + 1, dtype=np.int64), ("mode",), None, None, "mode")


# ---------------------------------------------------------------------------------------
# public functions
# ---------------------------------------------------------------------------------------
@accepts_xarray
def time_covariance(xobj, areacello=None, tcoord="time", ddof=1):
    """The area-weighted covariance between the time steps of a ``(time, ...)`` record (EXTENSION:
    not in momlevel; parity with the ``eofs`` package unpinned -- the specification is
    tests/eof_numpy.py): ``C[s, t] = sum_c area[c] a[s, c] a[t, c] / (nt - ddof)``, ``a`` the anomaly
    from each cell's time mean.  Returns a ``(time, time_2)`` float64 DataArray.

    ``xobj``: a DataArray whose LEADING dim is ``tcoord`` (anything else is a ``ValueError``), a
    numpy array or a device tensor (leading axis = time); float32 / float64 are read as they are,
    integers as float64.  ``areacello``: the cells' area, shaped as the record without ``tcoord``;
    NaN or non-positive area gives the cell no weight; None weighs every cell 1.  A cell with a
    missing step (NaN) is left out.  A device record gives a device result."""
    da = _as_record(xobj, tcoord)
    _check_counts(int(da.shape[0]), None, ddof)
    prep = _Prepared(da, areacello)
    cov = prep.out(_covariance(prep, ddof))
    coords = _time_coords(da, tcoord)
    if tcoord in coords:
        c = coords[tcoord]
        coords[tcoord + "_2"] = DataArray(c.data, (tcoord + "_2",), None, c.attrs, tcoord + "_2")
    return DataArray(cov, (tcoord, tcoord + "_2"), coords, {"long_name": "Time covariance"},
                     da.name)


@accepts_xarray
def calc_eofs(xobj, areacello=None, neofs=4, tcoord="time", ddof=1):
    """The ``neofs`` leading EOFs of a ``(time, ...)`` record and their principal components
    (EXTENSION, see time_covariance).  Returns a Dataset:

    - ``eigenvalues`` (mode): of the time covariance matrix, descending
      (``numpy.linalg.eigh`` on the host: an nt x nt problem)
    - ``variance_fraction`` (mode): each eigenvalue over the trace
    - ``eigenvalue_error`` (mode): North's rule of thumb, ``lambda * sqrt(2 / nt)``
    - ``pcs`` (time, mode): unit variance (``ddof``); the sign makes each PC's element of largest
      magnitude positive, the lowest index on ties
    - ``eofs`` (mode, ...): the covariance maps ``E_k = sum_t pc_k[t] a[t, c] / (nt - ddof)``, in the
      record's units, so that ``a ~= sum_k pc_k E_k``

    The maps are taken from the RAW record by ``core.time_project``, with the columns of the
    projector re-centred on the host; what remains of the cell's mean ``m`` in a map is the rounding
    of that centring, at most ``|m[c]| * nt * 2**-53 * max|P|`` with ``P = pcs / (nt - ddof)``.

    Cells with a missing step are NaN in ``eofs`` (and carry no weight); ``areacello`` as in
    time_covariance.  ``neofs > nt - 1`` is a ``ValueError``: the anomalies span no more modes.  A
    device record gives device results."""
    da = _as_record(xobj, tcoord)
    nt = int(da.shape[0])
    _check_counts(nt, neofs, ddof)
    neofs = int(neofs)
    prep = _Prepared(da, areacello)
    lam, frac, err, pcs = decompose(_covariance(prep, ddof), neofs, ddof)
    eofs = _maps(prep, pcs, ddof).reshape((neofs,) + prep.cells)

    mode = _mode_coord(neofs)
    out = Dataset(attrs=dict(da.attrs))
    for name, c in {**_cell_coords(da, tcoord), **_time_coords(da, tcoord)}.items():
        out._set(name, c, is_coord=True)
    out._set("mode", mode, is_coord=True)
    units = da.attrs.get("units")
    out["eigenvalues"] = DataArray(prep.out(lam), ("mode",), None,
                                   {"long_name": "Eigenvalues of the time covariance matrix"})
    out["variance_fraction"] = DataArray(prep.out(frac), ("mode",), None,
                                         {"long_name": "Fraction of the variance", "units": "1"})
    out["eigenvalue_error"] = DataArray(prep.out(err), ("mode",), None,
                                        {"long_name": "Sampling error of the eigenvalues (North)"})
    out["pcs"] = DataArray(prep.out(pcs), (tcoord, "mode"), None,
                           {"long_name": "Principal components (unit variance)", "units": "1"})
    out["eofs"] = DataArray(prep.out(eofs), ("mode",) + tuple(da.dims[1:]), None,
                            {"long_name": "EOFs as covariance maps",
                             **({"units": units} if units is not None else {})})
    return out


@accepts_xarray
def project_field(xobj, eofs, areacello=None, center=None, tcoord="time"):
    """Pseudo-PCs ``(time, mode)`` of a record projected onto ``eofs`` (mode, ...), the ``eofs``
    variable of calc_eofs (EXTENSION, see time_covariance)::

        ppc_k[t] = sum_c area[c] (x[t, c] - center[c]) E_k[c]  /  sum_c area[c] E_k[c]**2

    over the cells where the maps, the area and the center are valid -- the cross form of
    ``core.time_gram`` over the symmetric one's diagonal.  ``center``: the per-cell mean to
    subtract, shaped as the cells (the climatology the EOFs were computed against, for a record
    from another period); None is the record's own time mean.  Projecting the record the EOFs came
    from returns its ``pcs``.  A device record gives a device result."""
    da = _as_record(xobj, tcoord)
    if isinstance(eofs, Dataset):
        eofs = eofs["eofs"]
    maps = eofs if isinstance(eofs, DataArray) else DataArray(eofs)
    if maps.ndim < 2 or tuple(maps.shape[1:]) != tuple(da.shape[1:]):
        raise ValueError(f"eofs {tuple(maps.shape)} must be (mode,) + the record's cells "
                         f"{tuple(da.shape[1:])}")
    prep = _Prepared(da, areacello, center)
    nmode = int(maps.shape[0])
    E = core._f64(maps.data if maps.is_device else maps.values, prep.dev).reshape(nmode, prep.n)
    # 0 where every map (and the center) is valid, NaN elsewhere: a center that excludes the cell
    land = core.time_project(E, np.zeros((nmode, 1)))[0]
    both = core.time_project(torch.cat([E, prep.center.reshape(1, -1)]), np.zeros((nmode + 1, 1)))[0]
    num = hostio.to_host(core.time_gram(prep.y, E, prep.center, land, prep.scale))
    den = hostio.to_host(core.time_gram(E, None, both, None, prep.scale))
    with np.errstate(invalid="ignore", divide="ignore"):
        ppc = num / np.diag(den)[None, :]
    coords = _time_coords(da, tcoord)
    coords["mode"] = _mode_coord(nmode)
    return DataArray(prep.out(ppc), (tcoord, "mode"), coords,
                     {"long_name": "Pseudo principal components", "units": "1"}, da.name)
