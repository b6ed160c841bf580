"""extremes - order statistics of a (time, ...) record on the GPU: quantiles and medians along time,
over the whole record, per calendar month or per year, and the count of steps above a threshold.

EXTENSION: momlevel has no such functions.  They are what an extremes analysis of a sea-level record
starts from: the median, the 5-95 % range, the 99th percentile of daily sea level, the days a cell
spends above its own 99th percentile, each year's 99th percentile for a non-stationary fit.  On the
host these mean ``numpy.nanquantile`` over a NaN-holding ``(time, y, x)`` array -- one Python call
per cell.

A quantile is a selection, not a sum: one kernel (csrc/momlevel_quantile.hip,
``core.time_quantile``) finds every cell's order statistics by radix select in registers and
interpolates them as numpy's ``method="linear"`` does; a second (``core.time_exceed_count``) counts
the steps above a per-cell threshold.  include/momlevel_quantile.h states the contract,
tests/quantile_numpy.py restates it with ``numpy.sort``.  float64 results are value-identical to
``numpy.nanquantile(y[sel], q, axis=0)`` -- what xarray's ``.quantile(q, dim="time")`` gives -- up
to the sign of a zero.

Placement is the record module's (``record.Record``): device in, device out; host arrays in blocks
of cells.  A cell's selection never leaves its lane, so the block size never changes a bit.

Dtypes: float32 records give float32 (selected and interpolated in float64, rounded once -- the
convention of the grouped statistics, not numpy's float32 lerp); integer and boolean records are
computed and returned as float64; float16 and long double records are refused.  Counts are int64.
"""

import numpy as np

from .adapters import accepts_xarray
from .labeled import DataArray, Dataset
from .record import Record, check_record_dtype, over, plan_groups

__all__ = ["time_quantile", "time_median", "exceedance_count"]

GROUPINGS = (None, "month", "year")


def _plan(xobj, tcoord, by, time_axis_year=None):
    """the group plan of ``by`` from the record's time coordinate; None for the whole record"""
    from . import climatology

    if by not in GROUPINGS:
        raise ValueError(f"by must be None, 'month' or 'year', got {by!r}")
    if by is None:
        if time_axis_year is not None:
            raise ValueError("time_axis_year names the year of a by='month' axis")
        return None
    try:
        time_da = xobj[tcoord]
    except KeyError as exc:
        raise ValueError(f"by='{by}' needs the coordinate '{tcoord}'") from exc
    if by == "month":
        return climatology.annual_cycle_plan(time_da, tcoord, time_axis_year)
    if time_axis_year is not None:
        raise ValueError("time_axis_year names the year of a by='month' axis")
    return climatology.yearly_plan(time_da, tcoord)


# ---------------------------------------------------------------------------------------
# public functions
# ---------------------------------------------------------------------------------------
@accepts_xarray
def time_quantile(xobj, q, tcoord="time", by=None, time_axis_year=None):
    """Quantiles along ``tcoord``, NaNs skipped: the values of xarray's
    ``.quantile(q, dim=tcoord)`` (numpy's ``nanquantile``, ``method="linear"``).

    ``q``: a number or a sequence of numbers in [0, 1]; anything else is a ``ValueError`` before
    any upload.  ``by=None``: the whole record, and ``tcoord`` disappears.  ``by="month"``: one
    step per calendar month over all years (``climatology.annual_cycle_plan``: 12 steps on the
    month mid-points of ``time_axis_year`` or of the middle year; daily records are fine).
    ``by="year"``: one step per calendar year present (``climatology.yearly_plan``).

    A sequence ``q`` gives a leading ``"quantile"`` dim with a float64 coordinate; a scalar ``q``
    gives a scalar ``quantile`` coordinate and no dim (xarray's layout).  The remaining dims keep
    the input's order; attrs, name and encoding are carried.  A cell without a valid step is NaN.
    A DataArray, or every numeric variable of a Dataset that has ``tcoord``."""
    from . import core

    levels = core.quantile_levels(q)
    scalar = np.ndim(q) == 0
    plan = _plan(xobj, tcoord, by, time_axis_year)
    time = None if plan is None else plan.time  # (the plan's axis, or gone with the whole record)
    qcoord = {"quantile": DataArray(np.float64(levels[0]) if scalar else levels.copy(),
                                    () if scalar else ("quantile",), None, None, "quantile")}

    def one(da):
        check_record_dtype(da)
        rec = Record(da, tcoord)
        groups = plan_groups(plan, rec.nt)

        def block(y, _cells):
            return (core.time_quantile(y, levels, groups(y.device)),)

        (res,) = rec.walk(block, 0, levels.size * (1 if plan is None else plan.ngroups))
        # res: (nq, groups, cells...)
        if plan is None:
            res = res[:, 0]
        if scalar:
            return rec.labeled(res[0], time, (), qcoord)
        return rec.labeled(res, time, ("quantile",), qcoord)

    return over(xobj, tcoord, one, time, qcoord)


@accepts_xarray
def time_median(xobj, tcoord="time", by=None, time_axis_year=None):
    """The median along ``tcoord``, NaNs skipped: ``time_quantile(xobj, 0.5, ...)``."""
    return time_quantile(xobj, 0.5, tcoord=tcoord, by=by, time_axis_year=time_axis_year)


def _threshold_rows(threshold, da, rec, tcoord, ngroups):
    """``threshold`` as (ngroups, n) float64 rows, a host array or a device tensor: a number, a
    per-cell field without ``tcoord``, or a field whose ``tcoord`` has one step per group"""
    if isinstance(threshold, DataArray):
        dims = tuple(d for d in threshold.dims)
        if set(dims) - {tcoord} != set(rec.rest_dims) or len(dims) != len(set(dims)):
            raise ValueError(f"the threshold's dims {dims} must be the record's {rec.rest_dims}, "
                             f"with or without '{tcoord}'")
        if tcoord in dims:
            if threshold.sizes[tcoord] != ngroups:
                raise ValueError(f"the threshold has {threshold.sizes[tcoord]} steps of '{tcoord}' "
                                 f"for {ngroups} group(s)")
            data = threshold.transpose(tcoord, *rec.rest_dims).data
        else:
            data = threshold.transpose(*rec.rest_dims).data
        if not hasattr(data, "movedim"):
            data = np.asarray(DataArray(data).values, dtype=np.float64)
        else:
            import torch

            data = data.to(torch.float64)
        data = data.reshape((-1, rec.n))
        if data.shape[0] != ngroups:
            data = data.expand(ngroups, rec.n) if hasattr(data, "expand") else np.broadcast_to(
                data, (ngroups, rec.n))
        return data
    value = np.asarray(threshold, dtype=np.float64)
    if value.ndim != 0:
        raise TypeError("threshold must be a number or a DataArray")
    return np.broadcast_to(value, (ngroups, rec.n))


@accepts_xarray
def exceedance_count(xobj, threshold, tcoord="time", by=None):
    """How many steps of ``tcoord`` lie above ``threshold``: strictly, compared in float64; a NaN
    step or a NaN threshold counts nothing.  int64.

    ``threshold``: a number; a per-cell field without ``tcoord``; or a field whose ``tcoord`` has
    one step per group -- what ``time_quantile(..., by=...)`` returned, so that
    ``exceedance_count(eta, time_quantile(eta, 0.99, by="month"), by="month")`` counts, month by
    month, the days above that month's 99th percentile.  For a Dataset record the threshold may be
    a Dataset too (variables are matched by name).  ``by`` as in ``time_quantile``; the result has
    ``tcoord`` where the input had it (``by=None``: no ``tcoord``)."""
    from . import core

    plan = _plan(xobj, tcoord, by)
    time = None if plan is None else plan.time
    if isinstance(threshold, Dataset) and not isinstance(xobj, Dataset):
        raise TypeError("a Dataset threshold needs a Dataset record")
    if not isinstance(threshold, (DataArray, Dataset)) and np.ndim(threshold) != 0:
        raise TypeError("threshold must be a number, a DataArray or a Dataset")

    def one(da):
        check_record_dtype(da)
        rec = Record(da, tcoord)
        groups = plan_groups(plan, rec.nt)
        ngroups = 1 if plan is None else plan.ngroups
        thr = threshold
        if isinstance(thr, Dataset):
            if da.name not in thr.data_vars:
                raise ValueError(f"the threshold dataset has no variable '{da.name}'")
            thr = thr[da.name]
        rows = _threshold_rows(thr, da, rec, tcoord, ngroups)

        def block(y, cells):
            part = rows[:, cells]
            if not hasattr(part, "movedim"):
                part = np.ascontiguousarray(part)
            return (core.time_exceed_count(y, core._f64(part, y.device), groups(y.device)),)

        (res,) = rec.walk(block, 0, 2 * ngroups)
        return rec.labeled(res[0] if plan is None else res, time)

    return over(xobj, tcoord, one, time)
