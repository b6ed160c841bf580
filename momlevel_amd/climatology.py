"""climatology - grouped time statistics of a (time, ...) record on the GPU: what stands behind
``util.monthly_average`` and ``util.annual_cycle``.

The reference (src/momlevel/util.py:454-511 and :122-196) runs xarray's ``groupby`` over the
calendar fields of the time coordinate and reduces every group on one CPU thread.  Both functions
are the same computation: a NaN-skipping statistic over groups of time steps, one result row per
group.  Here the host makes only what depends on the time axis alone -- a *plan*: which steps form
which group (``steps`` / ``offsets``) and the new time axis -- and one HIP pass over the record
(csrc/momlevel_clim.hip, ``core.time_group_stat``) reduces every group of every cell.

Placement is the record module's (``record.Record``): device in, device out; host arrays in blocks
of cells.  A group is never split between threads, so the block size never changes a bit.

Arithmetic: float64 results are bit-identical to numpy's nanmean / nanstd (ddof = 0) / nanmin /
nanmax over axis 0 of the selected rows.  float32 records keep their dtype: they are accumulated in
float64 and rounded once (what xarray gives with bottleneck installed; not numpy's float32 running
sum).  Integer and boolean records are computed and returned as float64 -- a deviation for min /
max, where xarray keeps the integer dtype.  float16 and long double records are refused.
"""

import numpy as np

from . import cftime_lite, record
from .cftime_lite import DatetimeLite
from .labeled import DataArray

__all__ = ["GroupPlan", "monthly_plan", "annual_cycle_plan", "yearly_plan", "grouped_stat"]

STATS = ("mean", "std", "min", "max")


class GroupPlan:
    """Which steps form which group, and the time axis of the result.

    ``steps`` (int32) lists time indices, ``offsets`` (int64, ngroups + 1) cuts it into groups:
    group g is ``steps[offsets[g]:offsets[g + 1]]``, in the order the steps have on the axis.
    ``time`` is the new coordinate (a DataArray of ngroups calendar objects)."""

    def __init__(self, members, new_time, tcoord):
        self.sizes = [len(m) for m in members]
        self.ngroups = len(members)
        self.steps = np.concatenate([np.asarray(m, dtype=np.int64) for m in members]).astype(np.int32)
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        axis = np.empty(len(new_time), dtype=object)
        axis[:] = list(new_time)
        self.time = DataArray(axis, (tcoord,), None, None, tcoord)


def _calendar_values(time_da, what):
    values = np.asarray(time_da.values).reshape(-1)
    if not cftime_lite.is_calendar_axis(values):
        raise TypeError(f"{what} needs a time coordinate of calendar objects (year, month, "
                        "calendar): cftime.datetime or cftime_lite.DatetimeLite")
    return values


def _like_axis(points, sample):
    """the mid-points as objects of the kind the input axis holds: DatetimeLite stays, a cftime
    axis gets cftime.datetime (so that xarray sees a CFTimeIndex, as with the reference)"""
    if isinstance(sample, DatetimeLite):
        return points
    try:
        import cftime

        return [cftime.datetime(p.year, p.month, p.day, p.hour, p.minute, calendar=p.calendar)
                for p in points]
    except Exception:
        return points


def month_midpoints(year, calendar):
    """bounds[i] + (bounds[i + 1] - bounds[i]) / 2 over the 13 month starts of ``year``
    (util.py:169-178, :492-502): ``cftime_lite.monthly_midpoints`` of that one year"""
    return cftime_lite.monthly_midpoints(int(year), 1, calendar)


def monthly_plan(time_da, tcoord="time"):
    """Plan of ``monthly_average`` (util.py:485-508): one group per (year, month) present, in
    ascending order; the new axis holds the 12 month mid-points of each year present.  A year that
    lacks a calendar month is a ``ValueError`` (the reference fails there too: it assigns a
    12-point axis to fewer groups)."""
    values = _calendar_values(time_da, "monthly_average")
    calendar = values[0].calendar
    years = np.array([t.year for t in values], dtype=np.int64)
    months = np.array([t.month for t in values], dtype=np.int64)
    members, new_time = [], []
    for yr in sorted(set(years.tolist())):
        in_year = years == yr
        present = sorted(set(months[in_year].tolist()))
        if present != list(range(1, 13)):
            missing = [m for m in range(1, 13) if m not in present]
            raise ValueError(f"monthly_average: year {yr} lacks the calendar months {missing}; "
                             "every year of the record must hold all 12")
        for mon in range(1, 13):
            members.append(np.nonzero(in_year & (months == mon))[0])
        new_time += month_midpoints(yr, calendar)
    return GroupPlan(members, _like_axis(new_time, values[0]), tcoord)


def _microseconds(t):
    """whole microseconds since 1970-01-01 00:00 of the object's own calendar, as an exact integer"""
    seconds = ((cftime_lite.days_since_1970(t) * 24 + t.hour) * 60 + t.minute) * 60 + getattr(t, "second", 0)
    return seconds * 1_000_000 + getattr(t, "microsecond", 0)


def mid_year(first, last):
    """the year of ``first + (last - first) / 2`` (util.py:163-167), in the objects' own calendar;
    integer arithmetic: a mid-point that falls on a Jan 1 00:00 belongs to the year it opens"""
    calendar = first.calendar
    twice_mid = _microseconds(first) + _microseconds(last)
    year = min(first.year, last.year)
    while 2 * _microseconds(DatetimeLite(year + 1, 1, 1, calendar=calendar)) <= twice_mid:
        year += 1
    return year


def annual_cycle_plan(time_da, tcoord="time", time_axis_year=None):
    """Plan of ``annual_cycle`` (util.py:160-194): one group per calendar month 1..12 over all
    years; the new axis holds the month mid-points of ``time_axis_year``, or of the year in the
    middle between the first and the last time value.  A record that lacks a calendar month is a
    ``ValueError`` (the reference fails there too, assigning 12 points to fewer groups)."""
    values = _calendar_values(time_da, "annual_cycle")
    calendar = values[0].calendar
    months = np.array([t.month for t in values], dtype=np.int64)
    missing = [m for m in range(1, 13) if not np.any(months == m)]
    if missing:
        raise ValueError(f"annual_cycle: the record lacks the calendar months {missing}")
    year = int(time_axis_year) if time_axis_year is not None else mid_year(values[0], values[-1])
    members = [np.nonzero(months == mon)[0] for mon in range(1, 13)]
    return GroupPlan(members, _like_axis(month_midpoints(year, calendar), values[0]), tcoord)


def yearly_plan(time_da, tcoord="time"):
    """One group per calendar year present, in ascending order, with any number of steps per year
    (a daily record, a year cut short); the new axis holds ``cftime_lite.year_midpoint`` of each
    year.  EXTENSION: what ``extremes.time_quantile(..., by="year")`` goes by."""
    values = _calendar_values(time_da, "yearly_plan")
    calendar = values[0].calendar
    years = np.array([t.year for t in values], dtype=np.int64)
    present = sorted(set(years.tolist()))
    members = [np.nonzero(years == yr)[0] for yr in present]
    points = [cftime_lite._from_day_of_year(yr, cftime_lite.days_in_year(yr, calendar) / 2.0,
                                            calendar) for yr in present]
    return GroupPlan(members, _like_axis(points, values[0]), tcoord)


def grouped_stat(xobj, tcoord, plan, stat):
    """``stat`` over the groups of ``plan`` for a DataArray, or for every numeric variable of a
    Dataset that has ``tcoord``.  Results have ``tcoord`` leading.  Dataset: non-numeric variables
    are skipped and variables without ``tcoord`` are left out (the reference's groupby over time
    drops them); coordinates not on ``tcoord`` are kept; attrs and encoding of the variables are
    carried."""
    if stat not in STATS:
        raise ValueError(f"stat must be one of {STATS}, got '{stat}'")

    def one(da):
        """the record with ``tcoord`` leading, reduced group by group on the device"""
        from . import core

        record.check_record_dtype(da)
        rec = record.Record(da, tcoord)
        groups = record.plan_groups(plan, rec.nt)

        def block(y, _cells):
            return (core.time_group_stat(y, groups(y.device), stat=stat),)

        (res,) = rec.walk(block, 0, plan.ngroups)
        # (the groups lead wherever the input had tcoord: a leading dim with the plan's axis)
        return rec.labeled(res, None, (tcoord,), {tcoord: plan.time})

    return record.over(xobj, tcoord, one, plan.time, required=False)
