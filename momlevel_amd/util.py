"""Host-side helpers of the steric path: the reference's ``momlevel.util`` hot subset.

Same names, argument meaning and error behaviour as src/momlevel/util.py
(default_coords :199-224, eos_func_from_str :227-249, validate_areacello
:669-694, validate_dataset :697-814, annual_average :49-119).  No device work
except the area sum of device-resident ``areacello`` (mlx_nansum).
"""

import inspect
import warnings

import numpy as np

from . import eos
from .adapters import accepts_xarray
from .labeled import DataArray, Dataset

__all__ = [
    "annual_average",
    "annual_cycle",
    "default_coords",
    "eos_func_from_str",
    "geolocate_points",
    "linear_detrend",
    "monthly_average",
    "tile_nominal_coords",
    "validate_areacello",
    "validate_dataset",
    "validate_tidegauge_data",
]


_COORD_DEFAULTS = (("t", "time"), ("z", "z_l"), ("zbounds", "z_i"))


def default_coords(coord_names=None):
    """``(tcoord, zcoord, zbounds)``: MOM6's ``("time", "z_l", "z_i")`` unless the mapping
    overrides them under the keys ``"t"``, ``"z"``, ``"zbounds"`` (behaviour of util.py:199-224;
    a non-dict mapping is an ``AssertionError`` there, and here)."""
    mapping = coord_names if coord_names is not None else {}
    if not isinstance(mapping, dict):
        raise AssertionError("Coordinate mapping must be a dictionary.")
    return tuple(mapping.get(key, fallback) for key, fallback in _COORD_DEFAULTS)


def eos_func_from_str(eos_str, func_name="density"):
    """The function ``func_name`` of the equation-of-state module named ``eos_str`` (any case):
    ``"Wright"`` -> ``momlevel_amd.eos.wright.density``.  Unknown equation of state ->
    ``ValueError("Unknown equation of state: ...")`` as util.py:227-249; a function the module does
    not provide (the linear EOS has no alpha / beta here) is a ``ValueError`` too, not the bare
    ``KeyError`` of the reference's ``__dict__`` lookup."""
    if not isinstance(eos_str, str):
        raise AssertionError("Expecting string for equation of state")
    name = eos_str.lower()
    module = None if name.startswith("_") else getattr(eos, name, None)
    if not inspect.ismodule(module):
        raise ValueError(f"Unknown equation of state: {name}")
    func = getattr(module, func_name, None)
    if not callable(func):
        raise ValueError(
            f"Equation of state '{name}' does not provide `{func_name}` in momlevel_amd"
        )
    return func


def _area_sum(areacello):
    """skipna sum of areacello; on the device (mlx_nansum) when the data lives there."""
    if isinstance(areacello, DataArray) and areacello.is_device:
        from . import core

        return float(core.nansum(areacello.data).item())
    return float(np.nansum(np.asarray(areacello)))


def validate_areacello(areacello, reference=3.6111092e14, tolerance=0.02, total=None):
    """Does ``areacello`` sum to the real ocean's surface (3.6111092e14 m2) within a relative
    ``tolerance``?  Catches an unmasked field, e.g. the whole globe's area (util.py:669-694).
    ``total`` (not in momlevel): the sum over ALL horizontal tiles when ``areacello`` is one rank's
    tile of a multi-GPU run (momlevel_amd.parallel) -- the check is about the whole ocean."""
    area = _area_sum(areacello) if total is None else float(total)
    relative_error = (area - reference) / reference
    return bool(abs(relative_error) < tolerance)


_FIELDS_4D = ("thetao", "so", "volcello")
_FIELDS_2D = ("areacello", "deptho")
_REFERENCE_SCALARS = ("masso", "volo", "rhoga")
_REQUIRED = ("thetao", "so", "volcello", "areacello")
_REQUIRED_IN_REFERENCE = ("rho", "volo", "masso", "rhoga")


def _dataset_findings(dset, reference, additional_vars, area_total=None):
    """Yield ``(severity, message)`` for every requirement ``dset`` does not meet, in the order
    util.py:697-814 reports them.  severity "area" marks the one finding ``strict=False`` turns
    into a warning."""
    present = set(dset.variables)
    extra = [] if additional_vars is None else (
        list(additional_vars) if isinstance(additional_vars, list) else [additional_vars])
    wanted = list(_REQUIRED) + extra + (list(_REQUIRED_IN_REFERENCE) if reference else [])
    missing = [name for name in dict.fromkeys(wanted) if name not in present]
    if missing:
        yield "error", f"Reference dataset is missing variables: {missing}"

    # (a reference dataset "cannot contain a time coordinate": the reference's test compares names
    #  with unbound ``str.lower`` methods and can never fire, util.py:728-733 -- nothing to report)

    nd, layout = (3, "(z,y,x)") if reference else (4, "t,z,y,x")
    rank_rules = [(name, nd, f"Variable {name} must have exactly {nd} dimensions {layout}")
                  for name in _FIELDS_4D]
    rank_rules += [(name, 2, f"Variable {name} must have exactly 2 dimensions (y,x)")
                   for name in _FIELDS_2D]
    for name, rank, message in rank_rules:
        if name in present and len(dset[name].dims) != rank:
            yield "error", message

    if "areacello" in present and not validate_areacello(dset["areacello"], total=area_total):
        yield "area", "Variable `areacello` field is out of range. It may not be masked."

    if reference:
        # the reference words the `rho` finding with the name `areacello` (util.py:800);
        # the text is what a user of either package sees, so it is kept
        if "rho" in present and len(dset["rho"].dims) != 3:
            yield "error", "Variable areacello must have exactly 3 dimensions (z,y,x)"
        for name in _REFERENCE_SCALARS:
            if name in present and len(dset[name].dims) != 0:
                yield "error", f"Variable {name} must be a scalar"


def local_findings(dset, reference=False, additional_vars=None):
    """The fatal findings that do not depend on the areacello range check -- what ONE RANK of a
    tiled run can establish about its own tile before the first collective (steric.all_ranks_ok)."""
    # area_total=reference value: the range finding cannot fire here; it is judged on the global sum
    return [msg for severity, msg in _dataset_findings(dset, reference, additional_vars,
                                                       area_total=3.6111092e14)
            if severity != "area"]


def validate_dataset(dset, reference=False, strict=True, additional_vars=None, area_total=None):
    """Is ``dset`` a usable input (or, ``reference=True``, reference-state) dataset?

    Same observable behaviour as util.py:697-814: required variables present, fields of the right
    rank, ``areacello`` summing to the real ocean's area.  All findings are printed, then ONE
    ``ValueError("Errors found in dataset.")`` is raised; ``strict=False`` downgrades only the
    areacello range finding to a ``UserWarning``.  Returns None.  ``area_total``: see
    validate_areacello (tiled multi-GPU runs only).
    """
    fatal = []
    for severity, message in _dataset_findings(dset, reference, additional_vars, area_total):
        if severity == "area" and not strict:
            warnings.warn(message)
        else:
            fatal.append(message)
    if fatal:
        print("\n".join(fatal))
        raise ValueError("Errors found in dataset.")


# ---------------------------------------------------------------------------------------
# annual_average (util.py:49-119).  The time coordinate must hold calendar-aware
# objects exposing .year, .month, .calendar and .daysinmonth -- cftime.datetime does;
# momlevel_amd.cftime_lite.DatetimeLite is the stand-in when cftime is not installed.
# ---------------------------------------------------------------------------------------
def _annual_weights(time_values):
    years = np.array([t.year for t in time_values])
    weights = np.array([float(t.daysinmonth) for t in time_values])
    return years, weights


def _annual_mean_array(values, years, weights):
    """Per-year weighted mean over axis 0 (xarray ``weighted(w).mean``: NaNs carry no weight)."""
    out = []
    for yr in sorted(set(years.tolist())):
        sel = np.nonzero(years == yr)[0]
        assert len(sel) == 12
        x = values[sel]
        w = weights[sel].reshape((12,) + (1,) * (x.ndim - 1))
        num = np.sum(np.where(np.isnan(x), 0.0, x) * w, axis=0)
        den = np.sum(np.where(np.isnan(x), 0.0, 1.0) * w, axis=0)
        out.append(num / np.where(den != 0, den, np.nan))
    return np.stack(out, axis=0)


def _np_dtype(var):
    """numpy dtype of a labelled variable WITHOUT copying device data to the host."""
    from .labeled import np_dtype

    return np_dtype(var.data.dtype)


class AnnualPlan:
    """Calendar bookkeeping of annual_average for one time coordinate."""

    def __init__(self, time_da, tcoord):
        from .cftime_lite import year_midpoint

        time_values = list(time_da.values)
        calendar = time_values[0].calendar
        self.years, self.weights = _annual_weights(time_values)
        self.year_list = sorted(set(self.years.tolist()))
        for yr in self.year_list:
            assert int(np.sum(self.years == yr)) == 12  # util.py:85
        new_time = [year_midpoint(int(y), calendar) for y in self.year_list]
        self.time = DataArray(np.array(new_time, dtype=object), (tcoord,), None, time_da.attrs,
                              tcoord)
        # whole years stored back to back in ascending order: the device kernel's layout
        self.contiguous = bool(np.array_equal(self.years, np.repeat(self.year_list, 12)))


def annual_average(xobj, tcoord="time"):
    """Days-in-month weighted annual means (util.py:49-119).

    Accepts a labelled Dataset or DataArray; asserts 12 steps per year; the new
    time axis holds the mid-points of the years.
    """
    plan = AnnualPlan(xobj[tcoord], tcoord)
    years, weights, time_da = plan.years, plan.weights, plan.time

    def avg(da):
        if tcoord not in da.dims:
            return da
        moved = da.transpose(tcoord, ...)
        if moved.is_device and plan.contiguous:  # device-resident data: mlx_group_weighted_mean
            from . import core

            res = core.group_weighted_mean(moved.data.contiguous(), weights, 12)
        else:
            res = _annual_mean_array(moved.values.astype(np.float64), years, weights)
        coords = {k: v for k, v in moved.coords.items() if tcoord not in v.dims}
        coords[tcoord] = time_da
        out = DataArray(res, moved.dims, coords, da.attrs, da.name)
        out.encoding = dict(da.encoding)
        return out

    if isinstance(xobj, Dataset):
        result = Dataset(attrs=xobj.attrs)
        for name, c in xobj.coords.items():
            if tcoord not in c.dims:
                result._set(name, c, is_coord=True)
        result._set(tcoord, time_da, is_coord=True)
        for name, var in xobj.data_vars.items():
            if np.dtype(_np_dtype(var)).kind not in "fiu":
                continue  # non-numeric variables are skipped (util.py:79-84)
            result[name] = avg(var)
        return result
    return avg(xobj)


@accepts_xarray
def monthly_average(xobj, tcoord="time"):
    """Monthly means of daily (or any sub-monthly) data (util.py:454-511): one step per calendar
    month of every year present, the new time axis holding the months' mid-points; the result has
    ``tcoord`` leading.  It is what makes a daily record acceptable to ``annual_cycle`` and
    ``annual_average``.

    Accepts a labelled Dataset or DataArray (xarray objects through the adapter) whose time
    coordinate holds calendar objects.  One HIP pass (mlx_clim_group_stat) averages every month of
    every cell, NaNs skipped: float64 results are bit-identical to numpy's nanmean over the month's
    rows; float32 keeps its dtype (accumulated in float64, rounded once); integers and booleans give
    float64; float16 / long double are refused.  Device data stays on the device.  Dataset:
    non-numeric variables are skipped, variables without ``tcoord`` are left out, coordinates not
    on ``tcoord`` and the variables' attrs and encoding are kept.  A year that lacks a calendar
    month is a ``ValueError``.  Parity with real xarray objects is unpinned: xarray is not
    importable where the tests run."""
    from . import climatology

    return climatology.grouped_stat(xobj, tcoord, climatology.monthly_plan(xobj[tcoord], tcoord),
                                    "mean")


@accepts_xarray
def annual_cycle(xobj, tcoord="time", func="mean", time_axis_year=None):
    """Annual-cycle climatology of a monthly record (util.py:122-196): ``func`` ("mean", "std",
    "min" or "max") over all steps of each calendar month -- 12 time points, the month mid-points
    of ``time_axis_year`` or, without it, of the year in the middle of the record.  An unknown
    ``func`` is a ``ValueError``, as is a record that lacks a calendar month.

    One HIP pass (mlx_clim_group_stat; two reads of the record for "std") over every cell, NaNs
    skipped: float64 results are bit-identical to numpy's nanmean / nanstd (ddof = 0) / nanmin /
    nanmax.  Dtypes, placement and Dataset handling as ``monthly_average``; integer records give
    float64 for every ``func`` (xarray keeps integers for min / max).  Parity with real xarray
    objects is unpinned: xarray is not importable where the tests run."""
    from . import climatology

    if func not in climatology.STATS:
        raise ValueError(f"Unknown argument 'func={func}' to annual cycle")
    plan = climatology.annual_cycle_plan(xobj[tcoord], tcoord, time_axis_year)
    return climatology.grouped_stat(xobj, tcoord, plan, func)


# ---------------------------------------------------------------------------------------
# tide gauges: what tidegauge.extract_tidegauge leans on (util.py:252-367, :620-666, :817-860)
# ---------------------------------------------------------------------------------------
@accepts_xarray
def tile_nominal_coords(xcoord, ycoord, warn=True):
    """1-D x and y coordinates -> 2-D ``(geolon, geolat)`` with dims ``(ycoord.name, xcoord.name)``
    (util.py:620-666).  Right for regular lat-lon grids, wrong for the nominal coordinates of an
    irregular ocean grid -- hence the reference's warning, issued unless ``warn`` is False."""
    assert isinstance(xcoord, DataArray), "xcoord must be xarray.DataArray"
    assert isinstance(ycoord, DataArray), "ycoord must be xarray.DataArray"
    if warn:
        warnings.warn(
            "Constructing coordinates from 1-D vectors. "
            + "Make sure this is the intended behavior. "
            + "Do not use `xh`/`yh` when `geolon`/`geolat` are available"
        )
    xgrp, ygrp = np.meshgrid(xcoord.values, ycoord.values)
    dims = (ycoord.name, xcoord.name)

    def label(c):
        return DataArray(c.values, (c.name,), None, c.attrs, c.name)

    coords = {ycoord.name: label(ycoord), xcoord.name: label(xcoord)}
    return (DataArray(xgrp, dims, coords, None, "geolon"),
            DataArray(ygrp, dims, coords, None, "geolat"))


@accepts_xarray
def validate_tidegauge_data(arr, xcoord, ycoord, mask):
    """The argument checks of ``tidegauge.extract_tidegauge`` (util.py:817-860): ``arr`` a
    DataArray; ``xcoord`` / ``ycoord`` either the name of a coordinate of ``arr`` or a DataArray;
    ``mask`` a DataArray or None.  ``AssertionError`` otherwise, as in the reference."""
    assert isinstance(arr, DataArray), "Input array must be `xarray.DataArray` instance"
    _coords = list(arr.coords)
    if isinstance(xcoord, str):
        assert xcoord in _coords, f"`{xcoord}` not found in input array."
    else:
        assert isinstance(xcoord, DataArray), (
            "xcoord must either be a DataArray object or a "
            + "string that references an existing coordinate"
        )
    if isinstance(ycoord, str):
        assert ycoord in _coords, f"`{ycoord}` not found in input array."
    else:
        assert isinstance(ycoord, DataArray), (
            "ycoord must either be a DataArray object or a "
            + "string that references an existing coordinate"
        )
    if mask is not None:
        assert isinstance(mask, DataArray), "mask be a DataArray object"


def geolocate_points(df_model, df_locs, threshold=None, model_coords=("geolat", "geolon"),
                     rad_earth=6.378e03, loc_coords=("lat", "lon"), apply_mask=True,
                     disable_warning=True):
    """Map real-world locations to their nearest model grid points (util.py:252-367): pandas
    frames in, a frame out -- ``df_locs`` without its ``lat`` / ``lon`` columns and with
    ``distance`` (km), ``mod_index`` (the row of the point in the masked model frame),
    ``model_coords``, ``dim_vals`` (the point's label in the index of ``df_model``) and
    ``real_coords``.  Rows of ``df_model`` whose ``mask`` is not 1.0 are left out unless
    ``apply_mask`` is False.

    The reference queries a scikit-learn BallTree; this is ``tidegauge.locate`` -- a brute-force
    search on the GPU, ties to the lowest row -- and needs pandas only.  With ``threshold=None``
    nothing is filtered and nothing warned (the reference raises a ``TypeError`` when warnings are
    enabled without a threshold)."""
    from . import tidegauge  # (pandas itself is never imported: the frames bring their methods)

    ycoord1, xcoord1 = model_coords
    ycoord2, xcoord2 = loc_coords
    df1 = df_model.loc[:, ~df_model.columns.duplicated()]
    mask = df1["mask"].to_numpy() if (apply_mask and "mask" in df1.columns) else None
    loc = tidegauge.locate(df1[ycoord1].to_numpy(), df1[xcoord1].to_numpy(),
                           df_locs[ycoord2].to_numpy(), df_locs[xcoord2].to_numpy(), mask=mask,
                           threshold=threshold, rad_earth=rad_earth)
    if not disable_warning and threshold is not None:
        tidegauge.warn_unmapped(df_locs["name"].tolist(), loc, threshold)
    df2 = df_locs.iloc[loc.which].copy()
    df2["distance"] = loc.distance
    df2["mod_index"] = loc.mod_index
    df2["model_coords"] = list(zip(*loc.model_coords))
    df2["dim_vals"] = [df1.index[i] for i in loc.flat_index]
    df2["real_coords"] = list(zip(df2["lat"].values, df2["lon"].values))
    return df2.drop(["lat", "lon"], axis=1)


def linear_detrend(*args, **kwargs):
    """Deprecated shim of util.py:863-870: use ``momlevel_amd.trend.linear_detrend``."""
    from . import trend

    warnings.warn(
        "`util.linear_trend()` will be removed. "
        + "Please use version in the new `momlevel.trend` module",
        DeprecationWarning,
        stacklevel=2,
    )
    return trend.linear_detrend(*args, **kwargs)
