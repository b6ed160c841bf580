"""trend - linear trends, detrending and seasonal-model fits of a (time, ...) record on the GPU.

Same names, signatures and results as the reference's ``momlevel.trend``
(src/momlevel/trend.py): ``calc_linear_trend`` (:214-290), ``linear_detrend`` (:293-357),
``broadcast_trend`` (:20-112), ``time_conversion_factor`` (:115-164), ``seasonal_model``
(:360-461) and ``deseason`` (:683-856), on ``labeled.DataArray`` / ``Dataset`` and, through
``accepts_xarray``, on xarray objects.

The reference fits through ``xarray.polyfit`` (numpy's lstsq, one CPU thread) and a dask map of
``pinv`` / ``dot`` over single time series.  Here every pass over the record is a HIP kernel
(csrc/momlevel_trend.hip): the fit dimension is moved to the front on the device and each cell
(every other axis, flattened) is fitted independently in one streaming pass.  The host only
builds what depends on the time axis alone: its numeric values (``cftime_lite.axis_to_numeric``:
what xarray's ``get_clean_interp_index`` yields), the 6-row model matrix and its pseudo-inverse.

Placement is the record module's (``record.Record``): device in, device out; host arrays in blocks
of cells.  Each cell's fit is independent, so the split never changes a bit of the result.

One documented deviation: a cell with fewer than 2 valid steps gets NaN for slope and intercept
(numpy's lstsq returns a minimum-norm answer and a RankWarning there).
"""

import warnings

import numpy as np

from . import cftime_lite
from .adapters import accepts_xarray
from .labeled import DataArray, Dataset
from .record import Record, axis_values, rest_coords, slope_units, to_end

__all__ = [
    "broadcast_trend",
    "calc_linear_trend",
    "linear_detrend",
    "time_conversion_factor",
    "seasonal_model",
    "deseason",
]

COEFF_LABELS = ["constant", "trend", "sin_annual", "cos_annual", "sin_semiannual",
                "cos_semiannual"]


def time_conversion_factor(src, dst, days_per_month=30.417, days_per_year=365.0):
    """Conversion factor from the time unit ``src`` to ``dst`` (trend.py:115-164).  Recognized:
    "ns", "s", "min", "hr", "day", "mon" (30.417 days unless ``days_per_month``) and "yr" (365
    days unless ``days_per_year``)."""
    ns_from = {
        "ns": 1.0,
        "s": 1.0e9,
        "min": 1.0e9 * 60.0,
        "hr": 1.0e9 * 60.0 * 60.0,
        "day": 1.0e9 * 60.0 * 60.0 * 24.0,
        "mon": 1.0e9 * 60.0 * 60.0 * 24.0 * days_per_month,
        "yr": 1.0e9 * 60.0 * 60.0 * 24.0 * days_per_year,
    }
    ns_to = {k: 1.0 / v for k, v in ns_from.items()}
    assert str(src) in ns_from.keys(), f"Source unit `{src}` not recognized"
    assert str(dst) in ns_to.keys(), f"Destination unit `{dst}` not recognized"
    return ns_from[src] * ns_to[dst]


# ---------------------------------------------------------------------------------------
# the time axis: everything that depends on it alone is made here, on the host
# ---------------------------------------------------------------------------------------
def fit_axis(x):
    """``(xt, s, xmean)`` of a numeric axis: xt = (x - xmean) / s with xmean the mean over the
    whole axis and s = max|x - xmean| (1 if that is 0) -- the centred, scaled abscissa the fit
    kernel accumulates in (include/momlevel_trend.h)."""
    x = np.asarray(x, dtype=np.float64)
    xmean = float(np.mean(x))
    d = x - xmean
    s = float(np.max(np.abs(d))) if d.size else 0.0
    if not s > 0.0:
        s = 1.0
    return d / s, s, xmean


def seasonal_model_matrix(time_dec):
    """The 6-row model matrix of trend.py:403-410 / :511-520 for decimal years ``time_dec`` and
    its pseudo-inverse (numpy.linalg.pinv, float64): ``(model (6, nt), pmodel (nt, 6))``."""
    time_dec = np.asarray(time_dec, dtype=np.float64)
    model = np.array(
        [np.ones(len(time_dec))]
        + [time_dec - np.mean(time_dec)]
        + [np.sin(2 * np.pi * time_dec)]
        + [np.cos(2 * np.pi * time_dec)]
        + [np.sin(4 * np.pi * time_dec)]
        + [np.cos(4 * np.pi * time_dec)]
    )
    return model, np.linalg.pinv(model)


def decimal_year(time_values):
    """year + (dayofyear - 1 + hour / 24) / 365 of trend.py:397-401, for calendar objects or
    numpy.datetime64"""
    time_values = np.asarray(time_values)
    if time_values.dtype.kind == "M":
        t = time_values.astype("datetime64[ns]")
        year0 = t.astype("datetime64[Y]")
        year = year0.astype(np.int64) + 1970
        doy = (t.astype("datetime64[D]") - year0.astype("datetime64[D]")).astype(np.int64) + 1
        hour = (t.astype("datetime64[h]") - t.astype("datetime64[D]").astype("datetime64[h]")
                ).astype(np.int64)
    elif cftime_lite.is_calendar_axis(time_values):
        year = np.array([t.year for t in time_values], dtype=np.int64)
        doy = np.array([cftime_lite.day_of_year(t) for t in time_values], dtype=np.int64)
        hour = np.array([t.hour for t in time_values], dtype=np.int64)
    else:
        raise TypeError("seasonal_model needs a time coordinate of calendar objects or "
                        "numpy.datetime64")
    return year + (doy - 1 + hour / 24) / 365


def deseason_decimal_year(time_values):
    """arange(nt) / daysinyear[t] of trend.py:500-504 with the per-step 365 / 366 array of
    :772-779 -- the reference's own abscissa, odd as it is"""
    time_values = np.asarray(time_values)
    if not cftime_lite.is_calendar_axis(time_values):
        raise TypeError("deseason needs a time coordinate of calendar objects (year, calendar)")
    daysinyear = np.array([366 if cftime_lite.is_leap(t.year, t.calendar) else 365
                           for t in time_values])
    return np.arange(len(time_values)) / daysinyear


# ---------------------------------------------------------------------------------------
# public functions
# ---------------------------------------------------------------------------------------
@accepts_xarray
def broadcast_trend(slope, dim_arr, subtract_time_zero=False):
    """Broadcast a trend along a dimension to obtain the fitted line ``m * x`` (trend.py:20-112).

    ``slope``: a DataArray; ``dim_arr``: the 1-d dimension array, e.g. the time axis.  For an axis
    of calendar objects the time unit of the trend is read from the slope's ``units`` attribute
    (``"m yr-1"``); without one, nanoseconds are assumed and a warning is issued (:57-99).  The
    result has the slope's dims followed by the dimension's, as xarray's ``slope * index`` has
    (:105); ``subtract_time_zero`` returns anomalies relative to the first step (:108-110).
    One HIP pass (mlx_time_apply) writes the line."""
    assert isinstance(slope, DataArray), "Input `slope` must be a DataArray object"
    assert isinstance(dim_arr, DataArray), "Input `dim_arr` must be a DataArray object"
    assert len(dim_arr.dims) == 1, "Input `dim_arr` can only have one dimension"
    dim_name = dim_arr.dims[0]
    axis = (np.asarray(dim_arr.coords[dim_name].values) if dim_name in dim_arr.coords
            else np.asarray(dim_arr.values))
    data = slope.data if slope.is_device else np.asarray(slope.values, dtype=np.float64)

    if cftime_lite.is_calendar_axis(axis):
        warn_time_units = False
        if "units" in slope.attrs.keys():
            units = slope.attrs["units"].split(" ")
            units = [x.replace("-1", "") for x in units if "-1" in x]
            if len(units) == 0:
                warn_time_units = True
            elif len(units) == 1:
                units = units[0]
                if units != "ns":
                    factor = 1.0 / time_conversion_factor(units, "ns")
                    data = data * factor
            else:
                raise ValueError(
                    f"Units attribute for slope `{slope.name}` "
                    + f"has multiple time definitions: {slope.attrs['units']}. "
                )
        else:
            warn_time_units = True
        if warn_time_units:
            warnings.warn(
                "Unable to determine time unit of slope/trend. "
                + "Assuming Xarray's default nanoseconds (ns). "
                + "To fix this, ensure that the slope array has a units "
                + "attribute that describes the time units of the trend, "
                + "e.g. `m yr-1`"
            )

    x = cftime_lite.axis_to_numeric(axis)
    mode = "trend_anom" if subtract_time_zero else "trend"
    line = _apply_line(None, mode, x, data, None, slope.is_device)
    coords = dict(slope.coords)
    coords[dim_name] = DataArray(axis, (dim_name,), None, dim_arr.attrs, dim_name)
    return DataArray(to_end(line), slope.dims + (dim_name,), coords)


def _apply_line(y, mode, x, slope, intercept, on_device):
    """mlx_time_apply's straight-line modes on cells of any shape -> (nt,) + cells; host slopes
    (and records) go up and the line comes back through hostio"""
    from . import core, engine, hostio

    if on_device:
        return core.time_apply(y, mode, x, slope, intercept)
    device = engine.device_of()
    out = core.time_apply(None if y is None else hostio.to_device(y, device), mode, x,
                          hostio.to_device(np.asarray(slope, dtype=np.float64), device),
                          None if intercept is None else
                          hostio.to_device(np.asarray(intercept, dtype=np.float64), device))
    return hostio.to_host(out)


def _fit(arr, dim):
    """(record, x, slope, intercept) of ``arr`` along ``dim``: slope per unit of the numeric axis"""
    rec = Record(arr, dim)
    x = cftime_lite.axis_to_numeric(axis_values(arr, dim))
    xt, s, xmean = fit_axis(x)

    def block(y, _cells):
        from . import core

        return core.time_linfit(y, xt, s, xmean)

    slope, intercept = rec.walk(block, 0, 12)
    return rec, x, slope, intercept


@accepts_xarray
def calc_linear_trend(arr, dim="time", time_units=None):
    """Linear trend of a DataArray along ``dim`` (trend.py:214-290): a Dataset holding
    ``{name}_slope`` and ``{name}_intercept``, the input's attrs plus a ``comment`` on each.

    The reference calls xarray's ``polyfit(dim, 1)`` (:252): numpy's least squares per cell on the
    steps where the cell is not NaN, x being the coordinate as numbers -- nanoseconds since
    1970-01-01 of its own calendar for a time axis.  Here one HIP pass (mlx_time_linfit) fits every
    cell.  For an axis of calendar objects the slope is converted to ``time_units`` ("ns", "s",
    "min", "hr", "day", "mon", "yr"; default "ns") and its ``units`` attribute becomes
    ``"<units>  <time_units>-1"`` or ``" <time_units>-1"`` (:268-285)."""
    assert isinstance(arr, DataArray), "`_detrend_array` only supports `xarray.DataArray` objects"
    varname = arr.name
    rec, _x, slope, intercept = _fit(arr, dim)
    coords = rest_coords(arr, rec.rest_dims)

    slope_attrs = dict(arr.attrs)
    slope_attrs["comment"] = "Slope of linear trend"
    intercept_attrs = dict(arr.attrs)
    intercept_attrs["comment"] = "Y-intercept of linear trend"

    if cftime_lite.is_calendar_axis(axis_values(arr, dim)):
        factor, slope_attrs["units"] = slope_units(slope_attrs, time_units)
        slope = slope * factor

    dsout = Dataset()
    dsout[f"{varname}_slope"] = DataArray(slope, rec.rest_dims, coords, slope_attrs,
                                          f"{varname}_slope")
    dsout[f"{varname}_intercept"] = DataArray(intercept, rec.rest_dims, coords, intercept_attrs,
                                              f"{varname}_intercept")
    return dsout


def _detrend_array(arr, dim="time", order=1, mode="remove"):
    """trend.py:167-211: fit, build the line ``slope * x`` (``+ intercept`` for "remove"),
    subtract it -- mlx_time_linfit and mlx_time_apply on the record, uploaded once when it is the
    host's.  The pointwise pass keeps the reference's operator order: given the same slope and
    intercept it is bit-identical to numpy."""
    assert isinstance(arr, DataArray), "`_detrend_array` only supports `xarray.DataArray` objects"
    assert order == 1, "Only linear detrending (i.e. `order=1`) is supported in this version."
    if mode not in ["remove", "correct"]:
        raise ValueError(f"Unknown detrend mode '{mode}'")
    varname = arr.name
    rec = Record(arr, dim)
    x = cftime_lite.axis_to_numeric(axis_values(arr, dim))
    xt, s, xmean = fit_axis(x)

    def block(y, _cells):
        from . import core

        m, b = core.time_linfit(y, xt, s, xmean)
        return m, b, core.time_apply(y, mode, x, m, b if mode == "remove" else None)

    slope, intercept, result = rec.walk(block, 1, 12)
    coords = rest_coords(arr, rec.rest_dims)
    slope = DataArray(slope, rec.rest_dims, coords, None, f"{varname}_slope")
    intercept = DataArray(intercept, rec.rest_dims, coords, None, f"{varname}_intercept")
    attrs = dict(arr.attrs)
    attrs["detrend_comment"] = (
        f"detrended using momlevel (mode={mode}) with m={slope} and b={intercept}"
    )
    out = DataArray(rec.back(result), arr.dims, arr.coords, attrs, varname)
    return out


@accepts_xarray
def linear_detrend(xobj, dim="time", order=1, mode="remove"):
    """Linearly detrend a DataArray or every variable of a Dataset that has ``dim``
    (trend.py:293-357).  ``mode="remove"`` returns anomalies about the fitted line,
    ``mode="correct"`` subtracts ``slope * x`` only and keeps the magnitude of the data.  Variables
    without ``dim`` pass through; ``order != 1`` is an ``AssertionError``, an unknown mode a
    ``ValueError``; a Dataset holding ``time_bnds`` / ``average_T1`` / ``average_T2`` /
    ``average_DT`` gets the reference's warning (:333-338)."""
    if isinstance(xobj, DataArray):
        return _detrend_array(xobj, dim=dim, order=order, mode=mode)
    if isinstance(xobj, Dataset):
        varlist = list(xobj.keys())
        questionable_vars = ["time_bnds", "average_T1", "average_T2", "average_DT"]
        if any(var in varlist for var in questionable_vars):
            warnings.warn(
                "Incompatible variable detected. "
                + f"Check your dataset for the following and remove: {questionable_vars}"
            )
        result = Dataset(attrs=xobj.attrs)
        for name, c in xobj.coords.items():
            result._set(name, c, is_coord=True)
        for var in varlist:
            result[var] = (
                _detrend_array(xobj[var], dim=dim, order=order, mode=mode)
                if dim in xobj[var].dims
                else xobj[var]
            )
        return result
    raise TypeError("Input must be xarray.DataArray or xarray.Dataset")


def _project_apply(rec, model, pmodel, want):
    """coefficients (6, ...) and / or the model and residual records (nt, ...) of the K-term fit:
    mlx_time_project, then mlx_time_apply"""
    def block(y, _cells):
        from . import core

        coef = core.time_project(y, pmodel)
        outs = []
        for w in want:
            outs.append(coef if w == "coeff" else core.time_apply(
                y, "model_resid" if w == "residuals" else "model", model, coef))
        return tuple(outs)

    steps = sum(1 for w in want if w != "coeff")
    return rec.walk(block, steps, model.shape[0] * 18)


@accepts_xarray
def seasonal_model(da_timeseries, tcoord="time", return_model=False):
    """Residuals of a time series (of any dimensionality) about a model of a constant, a linear
    trend and annual and semi-annual harmonics (trend.py:360-461); with ``return_model`` the tuple
    ``(smodel, residuals)``.

    Decimal year = year + (dayofyear - 1 + hour / 24) / 365 (:397-401); the 6-row model matrix and
    ``numpy.linalg.pinv`` of it are built on the host in float64 (:403-412); the coefficients
    ``pmodel.dot(ts)`` (:428), the model ``model.dot(coeff)`` (:430) and the residuals (:431) are
    HIP passes over the record.  As in numpy's dot, one NaN step makes a cell NaN throughout.  The
    residuals keep the input's dims; the model has the time dimension last, as the reference's
    ``dot`` leaves it.  ``standard_name`` / ``long_name`` / ``units`` as :433-458."""
    assert isinstance(da_timeseries, DataArray), "Input must be a DataArray"
    da_timeseries = da_timeseries.reset_coords(drop=True)
    time_values = axis_values(da_timeseries, tcoord)
    model, pmodel = seasonal_model_matrix(decimal_year(time_values))
    rec = Record(da_timeseries, tcoord)
    smodel, residuals = _project_apply(rec, model, pmodel, ("model", "residuals"))

    attrs = da_timeseries.attrs
    if "standard_name" in attrs.keys():
        _standard_name_m = attrs["standard_name"] + "_smodel"
        _standard_name_r = attrs["standard_name"] + "_sresid"
    else:
        _standard_name_m = "smodel"
        _standard_name_r = "sresid"
    if "long_name" in attrs.keys():
        _long_name_m = "Seasonal model, " + attrs["long_name"]
        _long_name_r = "Seasonal residuals, " + attrs["long_name"]
    else:
        _long_name_m = "Seasonal model"
        _long_name_r = "Seasonal residuals"
    _units = attrs["units"] if "units" in attrs.keys() else ""

    smodel = DataArray(to_end(smodel), rec.rest_dims + (tcoord,), da_timeseries.coords,
                       {"standard_name": _standard_name_m, "long_name": _long_name_m,
                        "units": _units})
    residuals = DataArray(rec.back(residuals), da_timeseries.dims, da_timeseries.coords,
                          {"standard_name": _standard_name_r, "long_name": _long_name_r,
                           "units": _units}, da_timeseries.name)
    if return_model:
        return smodel, residuals
    return residuals


@accepts_xarray
def deseason(arr, tdim="time", output_format="residuals"):
    """Remove a linear trend and the annual and semi-annual cycle from a DataArray along ``tdim``
    (trend.py:683-856): ``output_format`` "residuals", "model" or "coeff" (the six coefficients,
    dims ``("coeff", ...)`` labelled constant, trend, sin_annual, cos_annual, sin_semiannual,
    cos_semiannual).  Results are time-first (:820-825).

    Decimal year = arange(nt) / daysinyear[t] with the per-step 365 / 366 array of the calendar
    (:500-504, :772-779): the reference's abscissa as it is.  Model matrix and pinv on the host
    (:511-523); coefficients, model and residuals (:526-532) are HIP passes; NaN propagates through
    a cell as in numpy's dot.  Attributes as :832-854 (the input's own attrs are left alone)."""
    assert isinstance(arr, DataArray), "Input must be an xarray DataArray"
    core_dims = list(arr.dims)
    assert tdim in core_dims, (
        f"Core dim {tdim} not found. " + "Specify alternate with tdim option."
    )
    if output_format not in ("residuals", "model", "coeff"):
        raise ValueError(f"output_format {output_format} not recognized")
    attrs = dict(arr.attrs)
    time_values = axis_values(arr, "time" if "time" in arr.coords else tdim)  # (:776 arr.time)
    model, pmodel = seasonal_model_matrix(deseason_decimal_year(time_values))
    rec = Record(arr, tdim)
    (data,) = _project_apply(rec, model, pmodel, (output_format,))

    coords = rest_coords(arr, rec.rest_dims)
    if output_format == "coeff":
        dims = ("coeff",) + rec.rest_dims
        labels = np.empty(6, dtype=object)
        labels[:] = COEFF_LABELS
        coords["coeff"] = DataArray(labels, ("coeff",), None, None, "coeff")
    else:
        dims = (tdim,) + rec.rest_dims
        coords = {k: v for k, v in arr.coords.items()}

    attrs.pop("standard_name", None)
    if output_format == "residuals":
        if "long_name" in attrs.keys():
            attrs["long_name"] = (
                attrs["long_name"] + " residuals from detrending and deseasonalizing"
            )
        attrs["processing"] = "Residuals from detrending and deseasonalizing"
    elif output_format == "model":
        if "long_name" in attrs.keys():
            attrs["long_name"] = (
                attrs["long_name"] + " model of linear trend and seasonal cycle"
            )
        attrs["processing"] = "Model of linear trend and seasonal cycle"
    else:
        if "long_name" in attrs.keys():
            attrs["long_name"] = (
                attrs["long_name"] + " seasonal model polynomial coefficients"
            )
        attrs["processing"] = "Seasonal model polynomial coefficients"
        attrs.pop("units", None)
    return DataArray(data, dims, coords, attrs, arr.name)
