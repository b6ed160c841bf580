"""The few calendar facts ``annual_average``, the trend module and the test-data time axes need.

The reference uses cftime (absent from this image).  ``DatetimeLite`` exposes
the attributes momlevel reads from a ``cftime.datetime`` -- ``year``, ``month``,
``day``, ``hour``, ``calendar``, ``daysinmonth`` -- so either kind of object can
sit in a time coordinate handed to ``util.annual_average``.
"""

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

_DPM = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)


def is_leap(year, calendar):
    calendar = calendar.lower()
    if calendar in ("noleap", "365_day", "360_day"):
        return False
    if calendar in ("all_leap", "366_day"):
        return True
    if calendar == "julian":
        return year % 4 == 0
    if calendar in ("standard", "gregorian", "proleptic_gregorian"):
        return (year % 4 == 0 and year % 100 != 0) or year % 400 == 0
    raise ValueError(f"unsupported calendar {calendar!r}")


def days_in_month(year, month, calendar):
    if calendar.lower() == "360_day":
        return 30
    return _DPM[month - 1] + (1 if (month == 2 and is_leap(year, calendar)) else 0)


def days_in_year(year, calendar):
    return sum(days_in_month(year, m, calendar) for m in range(1, 13))


@dataclass(frozen=True, order=True)
class DatetimeLite:
    year: int
    month: int
    day: int
    hour: int = 0
    minute: int = 0
    calendar: str = "noleap"

    @property
    def daysinmonth(self):
        return days_in_month(self.year, self.month, self.calendar)

    def __str__(self):
        return (f"{self.year:04d}-{self.month:02d}-{self.day:02d} "
                f"{self.hour:02d}:{self.minute:02d}:00")


def _from_day_of_year(year, doy, calendar):
    """doy: fractional days since Jan 1 00:00 of ``year`` (0-based)."""
    whole = int(doy)
    minutes = int(round((doy - whole) * 1440.0))
    month = 1
    while whole >= days_in_month(year, month, calendar):
        whole -= days_in_month(year, month, calendar)
        month += 1
    return DatetimeLite(year, month, whole + 1, minutes // 60, minutes % 60, calendar)


def year_midpoint(year, calendar):
    """bounds[0] + (bounds[1] - bounds[0]) / 2 of util.py:93-98 (a cftime.datetime when cftime
    is installed, so that xarray sees a CFTimeIndex as it does with the reference)."""
    mid = _from_day_of_year(year, days_in_year(year, calendar) / 2.0, calendar)
    try:
        import cftime

        return cftime.datetime(mid.year, mid.month, mid.day, mid.hour, mid.minute,
                               calendar=calendar)
    except Exception:
        return mid


def monthly_midpoints(start_year, nyears, calendar):
    """Monthly ('MS') mid-point axis of test_data/time.py:66-101."""
    out = []
    for y in range(start_year, start_year + nyears):
        doy = 0.0
        for m in range(1, 13):
            n = days_in_month(y, m, calendar)
            out.append(_from_day_of_year(y, doy + n / 2.0, calendar))
            doy += n
    return out


def daily_midpoints(start_year, nyears, calendar):
    """Daily ('D') mid-day axis of test_data/time.py:75-94: one step per day of ``nyears`` whole
    years, each at 12:00."""
    out = []
    for y in range(start_year, start_year + nyears):
        for m in range(1, 13):
            for d in range(1, days_in_month(y, m, calendar) + 1):
                out.append(DatetimeLite(y, m, d, 12, 0, calendar))
    return out


@lru_cache(maxsize=None)
def _year_start_day(year, calendar):
    """whole days from 1970-01-01 to Jan 1 of ``year``, both in ``calendar``"""
    if year >= 1970:
        return sum(days_in_year(y, calendar) for y in range(1970, year))
    return -sum(days_in_year(y, calendar) for y in range(year, 1970))


def day_of_year(t):
    """1-based day of the year of a calendar object (cftime's ``dayofyr``)"""
    cal = t.calendar
    return sum(days_in_month(t.year, m, cal) for m in range(1, t.month)) + t.day


def days_since_1970(t):
    """whole days from 1970-01-01 of the object's own calendar to its date"""
    return _year_start_day(t.year, t.calendar.lower()) + day_of_year(t) - 1


def ns_since_1970(t):
    """float64 nanoseconds since 1970-01-01 00:00 of the object's own calendar: what xarray's
    ``get_clean_interp_index`` makes of a CFTimeIndex (datetime_to_numeric, offset 1970-01-01,
    datetime_unit "ns") -- the x of ``polyfit`` and of ``broadcast_trend``."""
    seconds = ((days_since_1970(t) * 24 + t.hour) * 60 + t.minute) * 60 + getattr(t, "second", 0)
    return float(seconds * 1_000_000_000 + getattr(t, "microsecond", 0) * 1000)


def is_calendar_axis(values):
    """does the coordinate hold calendar objects (DatetimeLite, cftime.datetime)?  -- the
    reference's ``isinstance(index, CFTimeIndex)`` test (trend.py:59-60, :269-270)"""
    values = np.asarray(values)
    return (values.dtype == object and values.size > 0
            and all(hasattr(values.flat[0], a) for a in ("year", "month", "day", "calendar")))


def axis_to_numeric(values):
    """A coordinate as the float64 numbers a fit along it uses: calendar objects -> ns since
    1970-01-01 00:00 in their calendar; numpy.datetime64 -> ns since the epoch; a numeric
    coordinate keeps its own values."""
    values = np.asarray(values)
    if is_calendar_axis(values):
        return np.array([ns_since_1970(t) for t in values.ravel()], dtype=np.float64)
    if values.dtype.kind == "M":
        return values.astype("datetime64[ns]").astype(np.int64).astype(np.float64)
    return values.astype(np.float64)
