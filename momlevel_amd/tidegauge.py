"""tidegauge - tide gauges on the model grid: the nearest wet grid point of every gauge and the
gauges' series out of a ``(..., yh, xh)`` record, on the GPU.

Same name, signature and result as the reference's ``momlevel.tidegauge.extract_tidegauge``
(src/momlevel/tidegauge.py:40-152), on ``labeled.DataArray`` and, through ``accepts_xarray``, on
xarray objects; ``locate`` is the array-level function behind it and behind
``util.geolocate_points``.

The reference maps the gauges with a scikit-learn BallTree on pandas frames (util.py:252-367) and
pulls the series out with one ``arr.sel`` per gauge.  Here the search is a brute-force argmin over
all valid grid points (csrc/momlevel_gauge.hip: unit vectors once per point, squared chords in the
inner loop, the haversine angle once for the winner) and the extraction is ONE gather launch for
all gauges, each series a contiguous row of its result.

Contract of the search: a grid point takes part iff its mask value equals 1.0 exactly (a NaN mask
is land) and its coordinates are finite; ties go to the lowest flat index (numpy's ``argmin``;
BallTree leaves ties unspecified); the result does not depend on the launch geometry.

Placement: a device record in gives device series out and nothing crosses the host link; a host (or
lazily read) record goes up a block of rows at a time through ``hostio`` and the series come back
as numpy arrays.  The record is laid out by ``record.layout``, as for the fits and the grouped
statistics.
"""

import csv as _csv
import os
import warnings

import numpy as np

from . import util
from .adapters import accepts_xarray
from .labeled import DataArray, Dataset

__all__ = ["extract_tidegauge", "locate", "read_gauge_table"]

RAD_EARTH = 6.378e03  # km, the reference's (util.py:257)
_BUNDLED = ("us", "global")


class Located:
    """What ``locate`` found: numpy arrays with one entry per KEPT gauge, in input order.

    ``which`` the gauge's position in the table; ``distance`` in km; ``flat_index`` and
    ``iy`` / ``ix`` the grid position; ``mod_index`` the rank of the point among the valid points in
    C order (the reference's row in its masked frame); ``model_coords`` = ``(lat, lon)`` arrays of
    the grid point.  ``all_index`` / ``all_distance`` hold every gauge of the table (-1 / NaN where
    no valid point exists): what the warnings about dropped gauges are made from."""

    def __init__(self, which, distance, flat_index, shape, mod_index, model_coords, all_index,
                 all_distance):
        self.which, self.distance, self.flat_index = which, distance, flat_index
        self.shape, self.mod_index, self.model_coords = tuple(shape), mod_index, model_coords
        self.all_index, self.all_distance = all_index, all_distance
        grid = self.shape if len(self.shape) == 2 else (1, int(np.prod(self.shape, dtype=np.int64)))
        self.iy, self.ix = (a.astype(np.int64) for a in np.unravel_index(flat_index, grid))

    def __len__(self):
        return len(self.which)


def _shape(x):
    return tuple(x.shape) if hasattr(x, "shape") else tuple(np.asarray(x).shape)


def locate(lat2d, lon2d, gauge_lat, gauge_lon, mask=None, threshold=None, rad_earth=RAD_EARTH):
    """Nearest valid grid point of every gauge by great-circle distance -> ``Located``.

    ``lat2d`` / ``lon2d`` (degrees, one shape; numpy arrays or device tensors) are the grid,
    ``gauge_lat`` / ``gauge_lon`` the gauges; ``mask`` (the grid's shape) marks valid points with
    1.0 exactly.  A gauge is kept iff a valid point exists and (``threshold is None`` or
    ``distance <= threshold``), the distance being the haversine angle times ``rad_earth``
    (util.py:343, :356).  Three HIP passes: ``core.gauge_prepare`` for grid and gauges,
    ``core.gauge_nearest``; the grid point's own coordinates come back through
    ``core.gauge_gather``."""
    from . import core, hostio

    shape = _shape(lat2d)
    if _shape(lon2d) != shape or (mask is not None and _shape(mask) != shape):
        raise ValueError("lat2d, lon2d and mask must have one shape")
    glat = np.asarray(gauge_lat, dtype=np.float64).reshape(-1)
    glon = np.asarray(gauge_lon, dtype=np.float64).reshape(-1)
    if glat.size != glon.size:
        raise ValueError("one latitude and one longitude per gauge")
    n, ng = int(np.prod(shape, dtype=np.int64)), glat.size
    if n == 0 or ng == 0:
        empty_i, empty_f = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float64)
        return Located(empty_i, empty_f, empty_i, shape, empty_i, (empty_f, empty_f),
                       np.full(ng, -1, dtype=np.int64), np.full(ng, np.nan))

    core.require_device()
    from . import engine

    device = engine.device_of(lat2d, lon2d, mask)
    lat = core._gauge_operand(lat2d, device, "lat2d")
    lon = core._gauge_operand(lon2d, device, "lon2d")
    points, valid = core.gauge_prepare(lat, lon, mask, device=device)
    gauges, _ = core.gauge_prepare(glat, glon, device=device)
    index, angle = core.gauge_nearest(points, gauges)
    all_index = index.cpu().numpy()
    all_distance = angle.cpu().numpy() * rad_earth
    keep = all_index >= 0
    if threshold is not None:
        with np.errstate(invalid="ignore"):
            keep &= all_distance <= threshold
    which = np.nonzero(keep)[0].astype(np.int64)
    flat = all_index[which]
    rank = np.cumsum(valid.cpu().numpy(), dtype=np.int64) - 1  # position among the valid points
    if len(which):
        mlat = hostio.to_host(core.gauge_gather(lat.reshape(1, n), flat)).reshape(-1)
        mlon = hostio.to_host(core.gauge_gather(lon.reshape(1, n), flat)).reshape(-1)
    else:
        mlat = mlon = np.zeros(0, dtype=np.float64)
    return Located(which, all_distance[which], flat, shape, rank[flat],
                   (mlat.astype(np.float64), mlon.astype(np.float64)), all_index, all_distance)


def torch_index(host_indices, device):
    """a host index list as an int64 tensor on ``device``"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(host_indices, dtype=np.int64)).to(device)


def warn_unmapped(names, located, threshold):
    """the reference's warning (util.py:345-353), one per gauge at or beyond the threshold"""
    with np.errstate(invalid="ignore"):
        missing = np.nonzero(located.all_distance >= threshold)[0]
    for i in missing:
        warnings.warn(
            f"Unable to map site name: {names[i]} "
            + f"with distance {located.all_distance[i]} greater "
            + f"than threshold of {threshold}"
        )


# ---------------------------------------------------------------------------------------
# the gauge table
# ---------------------------------------------------------------------------------------
def _column(values):
    """a CSV column as numbers where every entry is one (int, else float), else as it is"""
    for kind in (int, float):
        try:
            return [kind(v) for v in values]
        except (TypeError, ValueError):
            continue
    return list(values)


def read_gauge_table(csv):
    """The gauge table as ``{column: list}`` with ``PSMSL_site`` renamed to ``name``
    (tidegauge.py:132-133): from a path to a CSV file (the standard library's ``csv`` module), a
    mapping of column -> sequence, or a pandas DataFrame.  ``name``, ``lat`` and ``lon`` are
    required (``KeyError``).  The reference's bundled tables "us" and "global" are its data and are
    not shipped: those two names raise ``FileNotFoundError``."""
    if isinstance(csv, str) and csv in _BUNDLED:
        raise FileNotFoundError(
            f"the reference's bundled table '{csv}' is not shipped with momlevel_amd: pass the path "
            f"of a CSV file with the columns name (or PSMSL_site), lat, lon -- momlevel's "
            f"resources/{csv}_tide_gauges.csv is one -- or an in-memory table")
    if hasattr(csv, "columns") and hasattr(csv, "__getitem__") and not isinstance(csv, dict):
        table = {str(c): list(csv[c]) for c in csv.columns}  # a pandas DataFrame
    elif hasattr(csv, "keys"):
        table = {str(k): list(csv[k]) for k in csv.keys()}
    else:
        path = os.fspath(csv)
        assert os.path.exists(path)  # (tidegauge.py:130)
        with open(path, newline="") as f:
            rows = list(_csv.reader(f))
        header, body = [h.strip() for h in rows[0]], [r for r in rows[1:] if r]
        table = {h: _column([r[i].strip() for r in body]) for i, h in enumerate(header)}
    if "PSMSL_site" in table:
        table = {("name" if k == "PSMSL_site" else k): v for k, v in table.items()}
    missing = [c for c in ("name", "lat", "lon") if c not in table]
    if missing:
        raise KeyError(f"the gauge table lacks the columns {missing} (it has {sorted(table)})")
    if len({len(v) for v in table.values()}) > 1:
        raise ValueError("the columns of the gauge table differ in length")
    return table


# ---------------------------------------------------------------------------------------
# extraction
# ---------------------------------------------------------------------------------------
def _grid_values(da):
    """the coordinate's data as ``locate`` takes it: the device tensor, or numpy"""
    return da.data if da.is_device else da.values


def _gather_series(arr, ydim, xdim, flat_index):
    """``(series (ng, nrest), rest_dims, rest_shape, on_device)``: the record with the horizontal
    dims last, flattened to (nrest, ny * nx) and gathered at ``flat_index`` in one launch (device
    record) or one launch per uploaded block of rows (host record)."""
    from . import core, engine, hostio, record

    rest_dims = tuple(d for d in arr.dims if d not in (ydim, xdim))
    moved = arr.transpose(*rest_dims, ydim, xdim)
    n = arr.sizes[ydim] * arr.sizes[xdim]
    rest_shape = tuple(arr.sizes[d] for d in rest_dims)
    nrest = int(np.prod(rest_shape, dtype=np.int64))
    # (contiguous, float32 kept, anything else float64)
    y = record.layout(moved, moved.dims[0]).reshape(nrest, n)
    if moved.is_device:
        return core.gauge_gather(y, flat_index), rest_dims, rest_shape, True
    device = engine.device_of()
    index = torch_index(flat_index, device)
    out = np.empty((len(flat_index), nrest), dtype=y.dtype)
    block = engine.chunk_steps(nrest, n * y.dtype.itemsize, device)
    for r0 in range(0, nrest, block):
        r1 = min(r0 + block, nrest)
        got = core.gauge_gather(hostio.to_device(np.ascontiguousarray(y[r0:r1]), device), index)
        out[:, r0:r1] = hostio.to_host(got)
    return out, rest_dims, rest_shape, False


def _python(v):
    return v.item() if isinstance(v, np.generic) else v


@accepts_xarray
def extract_tidegauge(arr, xcoord="geolon", ycoord="geolat", csv="us", mask=None, threshold=None,
                      disable_warning=True):
    """Extract tide-gauge locations from a DataArray (tidegauge.py:40-152): a Dataset with one
    variable per gauge that could be mapped, named by the table's ``name`` column.

    ``xcoord`` / ``ycoord``: names of coordinates of ``arr`` or DataArrays, 2-D (``geolon`` /
    ``geolat``) or 1-D -- 1-D coordinates are tiled, with the reference's warning
    (``util.tile_nominal_coords``).  ``csv``: the path of a CSV file, a mapping column -> sequence
    or a pandas DataFrame with the columns ``name`` (or ``PSMSL_site``), ``lat``, ``lon``; the
    reference's bundled "us" / "global" tables are not shipped and raise ``FileNotFoundError`` --
    pass a path.  ``mask``: wet mask on the grid (1 = ocean; NaN counts as land).  ``threshold``:
    gauges farther than this many km from their grid point are dropped.  ``disable_warning=False``
    warns once per gauge at or beyond the threshold.

    Each variable has ``arr``'s dims without the two horizontal ones and the attrs
    ``{**arr.attrs, **row}``: the gauge's table row plus ``distance`` (km), ``mod_index`` (rank of
    the grid point among the wet points), ``model_coords``, ``dim_vals``, ``real_coords`` and
    ``dims``, as in the reference.  A device record gives device series, each a contiguous row of
    one gather's result (``core.gauge_gather``); a host record gives numpy series.

    Two deviations.  The reference selects by coordinate LABEL (``arr.sel(**dim_vals)``), this
    selects by POSITION: the same series whenever the horizontal dimension coordinates are free of
    duplicates.  With ``threshold=None`` and ``disable_warning=False`` nothing is warned; the
    reference raises a ``TypeError`` there (util.py:346)."""
    util.validate_tidegauge_data(arr, xcoord, ycoord, mask)
    _xcoord = arr[xcoord] if isinstance(xcoord, str) else xcoord
    _ycoord = arr[ycoord] if isinstance(ycoord, str) else ycoord
    assert len(_xcoord.shape) == len(_ycoord.shape), "x and y coordinates must have the same shape"
    if len(_xcoord.shape) == 1:
        _xcoord, _ycoord = util.tile_nominal_coords(_xcoord, _ycoord)
    _xdims = tuple(_xcoord.dims)
    assert len(_xdims) == 2 and set(_ycoord.dims) == set(_xdims), (
        "x and y coordinates must share two dimensions")
    assert all(d in arr.dims for d in _xdims), (
        f"the coordinates' dimensions {_xdims} are not dimensions of the input array")
    ydim, xdim = _xdims
    _ycoord = _ycoord.transpose(ydim, xdim)
    if mask is not None:
        assert set(mask.dims) == set(_xdims), "mask must have the coordinates' dimensions"
        mask = mask.transpose(ydim, xdim)

    table = read_gauge_table(csv)
    loc = locate(_grid_values(_ycoord), _grid_values(_xcoord), table["lat"], table["lon"],
                 mask=None if mask is None else _grid_values(mask), threshold=threshold)
    if not disable_warning and threshold is not None:
        warn_unmapped(table["name"], loc, threshold)

    results = Dataset()
    if len(loc) == 0:
        return results
    series, rest_dims, rest_shape, _ = _gather_series(arr, ydim, xdim, loc.flat_index)
    coords = {d: arr.coords[d] for d in rest_dims if d in arr.coords}
    labels = [np.asarray(arr.coords[d].values) if d in arr.coords else None for d in _xdims]
    for j, g in enumerate(loc.which):
        row = {k: _python(v[g]) for k, v in table.items() if k not in ("lat", "lon")}
        pos = (int(loc.iy[j]), int(loc.ix[j]))
        row["distance"] = float(loc.distance[j])
        row["mod_index"] = int(loc.mod_index[j])
        row["model_coords"] = (float(loc.model_coords[0][j]), float(loc.model_coords[1][j]))
        row["dim_vals"] = tuple(_python(lab[p]) if lab is not None else p
                                for lab, p in zip(labels, pos))
        row["real_coords"] = (float(table["lat"][g]), float(table["lon"][g]))
        row["dims"] = _xdims
        name = row["name"]
        results[name] = DataArray(series[j].reshape(rest_shape), rest_dims, coords,
                                  {**arr.attrs, **row}, name)
    return results
