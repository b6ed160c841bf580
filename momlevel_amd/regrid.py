"""regrid - a ``(..., yh, xh)`` record moved to another grid on the GPU: sparse remapping of the
horizontal plane through a weight table, with the land-aware renormalisation of the weights.

EXTENSION: momlevel has no such functions.  They are what stands between a device-resident record
and a comparison on another grid: the model's eta against altimetry on a regular 1 or 0.25 degree
grid, a 0.25 degree run against a 1 degree run, a coarsened field for a plot or an EOF.  In xarray
this is ``xesmf`` or ``.coarsen()``; neither is importable where the tests run, so parity with them
is UNPINNED: the specification is the numpy restatement tests/regrid_numpy.py, which the kernel
(csrc/momlevel_regrid.hip, ``core.regrid_apply``) is gated against bit for bit.

All of it is ONE operator (include/momlevel_regrid.h states the contract): for every destination
``d`` and record, over the entries ``k`` of row ``d`` in ascending order of the source index,

    out[d] = sum_k S[k] v[col[k]] / sum_k S[k]        over the sources that are not NaN

in float64; a destination without a valid source, or whose valid weight is below ``min_frac`` of
its whole weight, is NaN.  ``skipna=False`` lets any NaN source make the destination NaN,
``renorm=False`` keeps the plain weighted sum.  What differs is the table, made here on the host:

  ``coarsen_weights``       conservative block coarsening of any grid (the tripolar grid as it is),
  ``conservative_weights``  first-order conservative remapping between rectilinear lat/lon grids,
  ``nearest_weights``       the nearest wet source point (the search of ``tidegauge.locate``),
  ``from_triplets``         any weights at all, as ESMF_RegridWeightGen or xesmf write them.

A ``Plan`` holds a table; ``apply`` runs a record through it, ``coarsen`` is the one-call form.
Records are independent and device tensors stay on the device.

One lane owns one destination, so a row as long as the source plane (a global mean) is correct but
slow: that is ``regional.area_mean``'s job.

NOT BUILT: bilinear weights and a conservative generator for curvilinear grids -- ``from_triplets``
takes both from the tools that make them; the tripolar north fold in ``coarsen_weights``' periodic
option (only x wraps); tables spread over several ranks.
"""

import numpy as np
import torch

from . import core, engine, hostio
from .adapters import accepts_xarray
from .labeled import DataArray, Dataset, check_field_dtype

__all__ = ["Plan", "from_triplets", "coarsen_weights", "conservative_weights", "nearest_weights",
           "apply", "coarsen"]

_NEAREST_BLOCK = 1 << 16  # destinations of one search: far inside mlx_gauge_nearest's range


# ---------------------------------------------------------------------------------------
# the table: rows on the host, and the sliced layout the kernel reads
# ---------------------------------------------------------------------------------------
def pack_rows(indptr, col, S, slice_rows):
    """Rows (indptr, col, S) -> ``(slice_ptr, len, col, S)`` in slices of ``slice_rows``
    destinations: entry k of destination d = s * slice_rows + lane at
    ``slice_ptr[s] + k * slice_rows + lane``, every slice padded to its longest row with
    col = -1, S = 0 (include/momlevel_regrid.h)."""
    L = int(slice_rows)
    indptr = np.asarray(indptr, dtype=np.int64)
    ndst = indptr.size - 1
    length = np.diff(indptr)
    if length.size and length.max() >= 2 ** 31:
        raise ValueError("a row holds 2^31 entries or more")
    nslices = -(-ndst // L)
    padded = np.zeros(nslices * L, dtype=np.int64)
    padded[:ndst] = length
    slice_ptr = np.zeros(nslices + 1, dtype=np.int64)
    np.cumsum(padded.reshape(nslices, L).max(axis=1) * L, out=slice_ptr[1:])
    nentries = int(slice_ptr[-1])
    d = np.repeat(np.arange(ndst, dtype=np.int64), length)
    k = np.arange(d.size, dtype=np.int64) - indptr[d]
    pos = slice_ptr[d // L] + k * L + d % L
    pcol = np.full(nentries, -1, dtype=np.int32)
    pS = np.zeros(nentries, dtype=np.float64)
    pcol[pos] = col
    pS[pos] = S
    return slice_ptr, length.astype(np.int32), pcol, pS


class Plan:
    """A weight table between two grids.

    ``src_shape`` / ``dst_shape``: the two planes; ``nsrc`` / ``ndst`` their cell counts;
    ``dst_dims`` and ``dst_coords`` label the result; ``indptr`` (ndst + 1) int64, ``col`` int32
    and ``S`` float64 are the rows on the host, a row's entries in ascending order of ``col``;
    ``packed`` is ``(slice_ptr, len, col, S)`` as the kernel reads them (``pack_rows``), made once;
    ``on(device)`` their upload, made once per device."""

    def __init__(self, indptr, col, S, src_shape, dst_shape, dst_dims=("lat", "lon"),
                 dst_coords=None):
        self.src_shape = tuple(int(n) for n in src_shape)
        self.dst_shape = tuple(int(n) for n in dst_shape)
        if len(self.src_shape) != 2 or len(self.dst_shape) != 2:
            raise ValueError("src_shape and dst_shape are (ny, nx) planes")
        if min(self.src_shape + self.dst_shape) < 0:
            raise ValueError("shapes must not be negative")
        self.nsrc = self.src_shape[0] * self.src_shape[1]
        self.ndst = self.dst_shape[0] * self.dst_shape[1]
        if self.nsrc >= 2 ** 31:
            raise ValueError("the source plane must hold fewer than 2^31 cells")
        self.dst_dims = tuple(dst_dims)
        if len(self.dst_dims) != 2 or self.dst_dims[0] == self.dst_dims[1]:
            raise ValueError("dst_dims names the two dims of the destination plane")
        self.dst_coords = dict(dst_coords) if dst_coords else {}
        for name, c in self.dst_coords.items():
            dims = c.dims if isinstance(c, DataArray) else None
            shape = tuple(np.shape(c.data if isinstance(c, DataArray) else c))
            sizes = dict(zip(self.dst_dims, self.dst_shape))
            if dims is None:
                dims = (name,) if len(shape) == 1 and name in sizes else self.dst_dims
                self.dst_coords[name] = DataArray(np.asarray(c), dims, None, None, name)
            if len(dims) != len(shape) or any(sizes.get(d) != n for d, n in zip(dims, shape)):
                raise ValueError(f"coordinate '{name}' {shape} does not lie on the destination "
                                 f"plane {sizes}")
        self.indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.S = np.ascontiguousarray(S, dtype=np.float64)
        if self.indptr.shape != (self.ndst + 1,) or self.col.shape != self.S.shape \
                or self.col.ndim != 1 or int(self.indptr[-1]) != self.col.size:
            raise ValueError("indptr, col and S are not the rows of one table")
        self._packed = None
        self._on = {}

    @property
    def nnz(self):
        return int(self.col.size)

    @property
    def packed(self):
        if self._packed is None:
            self._packed = pack_rows(self.indptr, self.col, self.S, core.regrid_slice())
        return self._packed

    def on(self, device):
        """``(slice_ptr, len, col, S)`` on ``device``: uploaded once per device"""
        key = str(device)
        if key not in self._on:
            self._on[key] = tuple(torch.from_numpy(a).to(device) for a in self.packed)
        return self._on[key]


def from_triplets(row, col, S, src_shape, dst_shape, one_based=False, dst_dims=("lat", "lon"),
                  dst_coords=None):
    """A ``Plan`` from ESMF-style weights: ``out[row[e]] += S[e] * src[col[e]]`` with ``row`` /
    ``col`` flat C-order indices into the destination / source plane (``one_based``: as
    ESMF_RegridWeightGen's ``row`` / ``col`` variables are).  Entries are sorted by (row, col); two
    entries for one (row, col) pair, a weight that is not finite and an index outside its plane
    are a ``ValueError``.  Touches no device."""
    row = np.asarray(row)
    col = np.asarray(col)
    S = np.asarray(S, dtype=np.float64)
    if row.ndim != 1 or row.shape != col.shape or row.shape != S.shape:
        raise ValueError("row, col and S must be 1-D arrays of one length")
    if row.size and (row.dtype.kind not in "iu" or col.dtype.kind not in "iu"):
        raise ValueError("row and col must be integers")
    row, col = row.astype(np.int64), col.astype(np.int64)
    if one_based:
        row, col = row - 1, col - 1
    src_shape = tuple(int(n) for n in src_shape)
    dst_shape = tuple(int(n) for n in dst_shape)
    if len(src_shape) != 2 or len(dst_shape) != 2:
        raise ValueError("src_shape and dst_shape are (ny, nx) planes")
    nsrc, ndst = src_shape[0] * src_shape[1], dst_shape[0] * dst_shape[1]
    if row.size and (row.min() < 0 or row.max() >= ndst):
        raise ValueError(f"row holds indices outside the destination plane of {ndst} cells")
    if col.size and (col.min() < 0 or col.max() >= nsrc):
        raise ValueError(f"col holds indices outside the source plane of {nsrc} cells")
    if not np.isfinite(S).all():
        raise ValueError("weights must be finite")
    order = np.lexsort((col, row))
    row, col, S = row[order], col[order], S[order]
    if row.size > 1 and np.any((row[1:] == row[:-1]) & (col[1:] == col[:-1])):
        raise ValueError("two weights for one (row, col) pair: sum them first")
    indptr = np.zeros(ndst + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=ndst), out=indptr[1:])
    return Plan(indptr, col, S, src_shape, dst_shape, dst_dims, dst_coords)


def _plane_of(areacello):
    """(values float64 (ny, nx), dims or None) of a 2-D area / mask"""
    dims = tuple(areacello.dims) if isinstance(areacello, DataArray) else None
    a = areacello.values if isinstance(areacello, DataArray) else areacello
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()  # (a small map: downloaded for the table)
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError(f"a 2-D (ydim, xdim) field is expected, got shape {a.shape}")
    if a.dtype.kind not in "fiub":
        raise TypeError(f"a numeric field is expected, got {a.dtype}")
    return a.astype(np.float64), dims


def _factor(f, what):
    if int(f) != f or int(f) < 1:
        raise ValueError(f"{what} is a whole number of cells >= 1, got {f}")
    return int(f)


def coarsen_weights(areacello, fy, fx, periodic_x=False):
    """Conservative block coarsening: destination ``(J, I)`` of the ``ceil(ny / fy)`` x
    ``ceil(nx / fx)`` plane is the area-weighted mean of source rows ``J*fy .. J*fy + fy - 1`` and
    columns ``I*fx .. I*fx + fx - 1``, the weights the source areas.  A NaN or non-positive area
    carries no entry (land); an infinite area is a ``ValueError``.  Blocks at the north and east
    edge are cut at the edge; with ``periodic_x`` the last block of a row is completed from the
    row's first columns instead (the tripolar fold is not built: only x wraps).  Index arithmetic
    only, so it works on the tripolar grid as it is.  Touches no device."""
    area, dims = _plane_of(areacello)
    fy, fx = _factor(fy, "fy"), _factor(fx, "fx")
    if np.isinf(area).any():
        raise ValueError("areacello holds infinite areas")
    ny, nx = area.shape
    my, mx = -(-ny // fy), -(-nx // fx)
    jj = np.arange(ny, dtype=np.int64)
    ii = np.arange(mx * fx if periodic_x else nx, dtype=np.int64)
    src = jj[:, None] * nx + (ii % max(nx, 1))[None, :]
    dst = (jj // fy)[:, None] * mx + (ii // fx)[None, :]
    w = area.reshape(-1)[src] if area.size else np.zeros(src.shape)
    with np.errstate(invalid="ignore"):
        keep = w > 0.0  # (NaN compares False)
    return from_triplets(dst[keep], src[keep], w[keep], (ny, nx), (my, mx),
                         dst_dims=dims or ("yh", "xh"))


def _bounds(b, what, lat):
    b = np.asarray(b, dtype=np.float64)
    if b.ndim != 1 or b.size < 2 or not np.isfinite(b).all():
        raise ValueError(f"{what} must hold the n + 1 finite 1-D bounds of n cells")
    step = np.diff(b)
    if not (np.all(step > 0) or np.all(step < 0)):
        raise ValueError(f"{what} must be strictly monotonic")
    if lat and (b.min() < -90.0 or b.max() > 90.0):
        raise ValueError(f"{what} must lie in [-90, 90]")
    if not lat and abs(b[-1] - b[0]) > 360.0:
        raise ValueError(f"{what} spans more than 360 degrees")
    return np.minimum(b[:-1], b[1:]), np.maximum(b[:-1], b[1:])


def _lat_overlap(slo, shi, dlo, dhi):
    """(nd, ns): sin(top) - sin(bottom) of the part of source band s inside destination band d"""
    lo = np.maximum(dlo[:, None], slo[None, :])
    hi = np.minimum(dhi[:, None], shi[None, :])
    w = np.sin(np.deg2rad(hi)) - np.sin(np.deg2rad(lo))
    return np.where(hi > lo, w, 0.0)


def _lon_overlap(slo, shi, dlo, dhi):
    """(nd, ns): radians of longitude source cell s shares with destination cell d, the source
    cell taken at the two positions modulo 360 degrees that can reach the destination cell"""
    turns = np.floor((dlo[:, None] - slo[None, :]) / 360.0)
    deg = np.zeros((dlo.size, slo.size))
    for n in (turns, turns + 1.0):
        lo = np.maximum(dlo[:, None], slo[None, :] + 360.0 * n)
        hi = np.minimum(dhi[:, None], shi[None, :] + 360.0 * n)
        deg += np.where(hi > lo, hi - lo, 0.0)
    return np.deg2rad(deg)


def conservative_weights(src_lat_b, src_lon_b, dst_lat_b, dst_lon_b, src_mask=None):
    """First-order conservative remapping between two rectilinear latitude/longitude grids given
    by their 1-D cell bounds in degrees (``n + 1`` strictly monotonic bounds for ``n`` cells).  The
    weight of a source cell in a destination cell is the exact area of their intersection on the
    unit sphere, ``(sin phi2 - sin phi1) * dlambda`` of the intersection box, with longitudes
    matched modulo 360 degrees.  It is separable: the table is the outer product of the two 1-D
    overlap tables and is never formed as a dense (ndst, nsrc) array.  ``src_mask`` (ny, nx):
    source cells where it is 0, False or NaN carry no entry.  The result's dims are
    ``("lat", "lon")``, its coords the destination cell centres.  Curvilinear grids are not built:
    bring their weights through ``from_triplets``.  Touches no device."""
    sy = _bounds(src_lat_b, "src_lat_b", True)
    sx = _bounds(src_lon_b, "src_lon_b", False)
    dy = _bounds(dst_lat_b, "dst_lat_b", True)
    dx = _bounds(dst_lon_b, "dst_lon_b", False)
    nys, nxs, nyd, nxd = sy[0].size, sx[0].size, dy[0].size, dx[0].size
    # a descending axis: cell i lies between bounds i and i + 1 whichever is the lower
    wy = _lat_overlap(*sy, *dy)
    wx = _lon_overlap(*sx, *dx)
    jd, js = np.nonzero(wy > 0.0)
    i_d, i_s = np.nonzero(wx > 0.0)
    row = (jd[:, None] * nxd + i_d[None, :]).reshape(-1)
    col = (js[:, None] * nxs + i_s[None, :]).reshape(-1)
    S = (wy[jd, js][:, None] * wx[i_d, i_s][None, :]).reshape(-1)
    if src_mask is not None:
        m, _ = _plane_of(src_mask)
        if m.shape != (nys, nxs):
            raise ValueError(f"src_mask must be ({nys}, {nxs}), got {m.shape}")
        with np.errstate(invalid="ignore"):
            wet = (m != 0.0) & ~np.isnan(m)
        keep = wet.reshape(-1)[col]
        row, col, S = row[keep], col[keep], S[keep]
    dlat = np.asarray(dst_lat_b, dtype=np.float64)
    dlon = np.asarray(dst_lon_b, dtype=np.float64)
    coords = {"lat": 0.5 * (dlat[:-1] + dlat[1:]), "lon": 0.5 * (dlon[:-1] + dlon[1:])}
    return from_triplets(row, col, S, (nys, nxs), (nyd, nxd), dst_coords=coords)


def _grid(lat, lon, what):
    """(lat2d, lon2d): two 1-D axes span a rectilinear grid, two arrays of one shape are the grid"""
    dev = [isinstance(a, torch.Tensor) and a.is_cuda for a in (lat, lon)]
    if any(dev):
        if not all(dev) or tuple(lat.shape) != tuple(lon.shape) or lat.dim() != 2:
            raise ValueError(f"device {what}_lat and {what}_lon must be 2-D tensors of one shape")
        return lat, lon
    lat = np.asarray(lat.values if isinstance(lat, DataArray) else lat, dtype=np.float64)
    lon = np.asarray(lon.values if isinstance(lon, DataArray) else lon, dtype=np.float64)
    if lat.ndim == 1 and lon.ndim == 1:
        lat, lon = np.broadcast_to(lat[:, None], (lat.size, lon.size)), \
            np.broadcast_to(lon[None, :], (lat.size, lon.size))
    if lat.ndim != 2 or lat.shape != lon.shape:
        raise ValueError(f"{what}_lat and {what}_lon must be two 1-D axes or 2-D arrays of one shape")
    return np.ascontiguousarray(lat), np.ascontiguousarray(lon)


def nearest_weights(src_lat, src_lon, dst_lat, dst_lon, mask=None, threshold=None):
    """One entry of weight 1 per destination: the nearest wet source point by great-circle
    distance.  Coordinates in degrees, as two 1-D axes (a rectilinear grid) or two 2-D arrays of
    one shape (numpy, or device tensors for the source).  The search is ``tidegauge.locate``'s --
    a source point takes part iff its ``mask`` value is 1.0 exactly and its coordinates are
    finite, ties go to the lowest flat index -- run on the GPU in blocks of destinations that stay
    inside that kernel's range.  A destination farther than ``threshold`` km from every wet point
    (or without one) gets no entry, so its result is NaN."""
    from . import tidegauge

    slat, slon = _grid(src_lat, src_lon, "src")
    dlat, dlon = _grid(dst_lat, dst_lon, "dst")
    if isinstance(dlat, torch.Tensor):
        dlat, dlon = dlat.detach().cpu().numpy(), dlon.detach().cpu().numpy()
    src_shape, dst_shape = tuple(int(n) for n in slat.shape), tuple(int(n) for n in dlat.shape)
    ndst = dst_shape[0] * dst_shape[1]
    flat_lat, flat_lon = dlat.reshape(-1), dlon.reshape(-1)
    index = np.full(ndst, -1, dtype=np.int64)
    for i0 in range(0, ndst, _NEAREST_BLOCK):
        i1 = min(i0 + _NEAREST_BLOCK, ndst)
        found = tidegauge.locate(slat, slon, flat_lat[i0:i1], flat_lon[i0:i1], mask=mask,
                                 threshold=threshold)
        index[i0 + found.which] = found.flat_index
    row = np.nonzero(index >= 0)[0]
    coords = {}
    axes = np.ndim(dst_lat) == 1 and np.ndim(dst_lon) == 1
    if axes:
        coords = {"lat": np.asarray(dst_lat, dtype=np.float64),
                  "lon": np.asarray(dst_lon, dtype=np.float64)}
    return from_triplets(row, index[row], np.ones(row.size), src_shape, dst_shape,
                         dst_coords=coords)


# ---------------------------------------------------------------------------------------
# a record through a plan
# ---------------------------------------------------------------------------------------
def _check(plan, min_frac, skipna, renorm):
    if not isinstance(plan, Plan):
        raise TypeError("plan must be a regrid.Plan (from_triplets, coarsen_weights, "
                        "conservative_weights, nearest_weights)")
    try:
        min_frac = float(min_frac)
    except (TypeError, ValueError):
        raise ValueError(f"min_frac must be a number in [0, 1], got {min_frac!r}") from None
    if not 0.0 <= min_frac <= 1.0:  # (a NaN compares false)
        raise ValueError(f"min_frac must lie in [0, 1], got {min_frac}")
    return min_frac, bool(skipna), bool(renorm)


def _records(da, plan, min_frac, skipna, renorm):
    """one DataArray through ``core.regrid_apply`` -> the raw result ``lead + plan.dst_shape`` of
    the record's dtype (integers as float64): on the device for a device record, on the host
    otherwise"""
    if da.ndim < 2:
        raise ValueError("a record has at least the two dims of the plane")
    if tuple(int(n) for n in da.shape[-2:]) != plan.src_shape:
        raise ValueError(f"the record's plane {tuple(da.shape[-2:])} is not the plan's source "
                         f"plane {plan.src_shape}")
    name = check_field_dtype(da.dtype, "records")
    tdt = torch.float32 if name == "float32" else torch.float64  # (integers compute as float64)
    ndt = np.float32 if name == "float32" else np.float64
    lead = tuple(int(n) for n in da.shape[:-2])
    nrec = int(np.prod(lead, dtype=np.int64))
    dev = engine.device_of(da.data)

    def launch(v):
        return core.regrid_apply(v, plan.on(dev), plan.nsrc, plan.ndst, min_frac,
                                 propagate=not skipna, renorm=renorm)

    if not da.is_device and len(lead) >= 1 and hostio.wants_pipeline(lead[0], nrec * plan.nsrc):
        # a large host / lazy record: groups of whole leading rows; a lazy record is never
        # materialised whole.  A record's result depends on that record alone.
        inner = nrec // lead[0]
        source = da.data if da.is_lazy else da.values

        def kernel(tensors, i0, i1):
            v = tensors[0].to(tdt).reshape((i1 - i0) * inner, plan.nsrc)
            return launch(v).reshape((i1 - i0,) + lead[1:] + plan.dst_shape)

        return hostio.pipeline_rows(hostio.row_bounds(lead[0], inner * plan.nsrc), dev,
                                    hostio.leading_slices([source]), kernel,
                                    np.empty(lead + plan.dst_shape, dtype=ndt))

    v = da.data.to(tdt) if da.is_device else engine.to_device(da.values, dev, tdt)
    res = launch(v.reshape(nrec, plan.nsrc).contiguous()).reshape(lead + plan.dst_shape)
    return res if da.is_device else hostio.to_host(res)


def _labelled(da, plan, *args):
    drop = set(da.dims[-2:])
    coords = {n: c for n, c in da.coords.items()
              if not (isinstance(c, DataArray) and drop & set(c.dims)) and n not in drop}
    coords.update(plan.dst_coords)
    out = DataArray(_records(da, plan, *args), tuple(da.dims[:-2]) + plan.dst_dims, coords,
                    dict(da.attrs), da.name)
    out.encoding = dict(da.encoding)
    return out


def _apply(xobj, plan, *args):
    if isinstance(xobj, DataArray):
        return _labelled(xobj, plan, *args)
    if isinstance(xobj, Dataset):
        out = Dataset(attrs=xobj.attrs)
        planes = {tuple(v.dims[-2:]) for v in xobj.data_vars.values()
                  if v.ndim >= 2 and tuple(v.shape[-2:]) == plan.src_shape and v.dtype.kind in "fiub"}
        if len(planes) != 1:
            raise ValueError(f"the Dataset must hold variables on one source plane "
                             f"{plan.src_shape}, found {sorted(planes)}")
        plane = planes.pop()
        for name, var in xobj.data_vars.items():
            on_plane = var.ndim >= 2 and tuple(var.dims[-2:]) == plane and var.dtype.kind in "fiub"
            if on_plane:
                out[name] = _labelled(var, plan, *args)
            elif not set(plane) & set(var.dims):
                out[name] = var  # (a variable that does not lie on the plane passes through)
        return out
    if isinstance(xobj, (np.ndarray, torch.Tensor)):
        if xobj.ndim < 2:
            raise ValueError("a record has at least the two dims of the plane")
        dims = tuple(f"dim_{i}" for i in range(xobj.ndim - 2)) + ("src_y", "src_x")
        return _labelled(DataArray(xobj, dims), plan, *args).data
    raise TypeError("Input must be a DataArray, a Dataset, a numpy array or a device tensor")


@accepts_xarray
def apply(xobj, plan, min_frac=0.0, skipna=True, renorm=True):
    """A record on the plan's source grid moved to its destination grid (EXTENSION: not in
    momlevel; parity with xesmf / ``.coarsen()`` is unpinned -- the specification is the module
    docstring and tests/regrid_numpy.py).

    ``xobj``: a DataArray whose LAST two dims are the plan's source plane, with any leading dims
    (each leading index is a record of its own); a Dataset (every numeric variable on the plane is
    remapped, variables that do not touch it pass through, the others are dropped); or a numpy
    array / device tensor ``(..., ny, nx)``, answered in kind.  The result has the record's leading
    dims, their coords, its attrs and dtype (float32 is the float64 result rounded once; integers
    give float64) and the plan's ``dst_dims`` and ``dst_coords`` in place of the plane's.

    NaN sources are left out and the weights present renormalised; a destination whose valid
    weight is below ``min_frac`` (in [0, 1]) of its whole weight, or without a valid source, is
    NaN.  ``skipna=False``: any NaN source makes the destination NaN and the plain weighted sum is
    returned.  ``renorm=False``: NaN sources are left out but the sum is not divided by the weight
    present.  A row as long as the plane is correct but slow: see ``regional.area_mean``."""
    return _apply(xobj, plan, *_check(plan, min_frac, skipna, renorm))


@accepts_xarray
def coarsen(xobj, areacello, fy, fx, periodic_x=False, min_frac=0.0, skipna=True, renorm=True):
    """``apply(xobj, coarsen_weights(areacello, fy, fx, periodic_x), ...)`` (EXTENSION, see
    ``apply``): the area-weighted mean over blocks of ``fy`` x ``fx`` cells, land left out."""
    return apply(xobj, coarsen_weights(areacello, fy, fx, periodic_x), min_frac=min_frac,
                 skipna=skipna, renorm=renorm)
