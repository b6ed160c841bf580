"""numpy restatement of what momlevel.trend computes, for the parity tests of the trend kernels.

Not product code and not the checker under oracle/: three small functions the new tests compare
against.  The reference fits through xarray's ``polyfit`` -- ``numpy.polyfit(x, y, 1)`` on the steps
where a column is not NaN, x being the coordinate as float64 numbers (nanoseconds since
1970-01-01 00:00 of the axis's own calendar for a time axis) -- and models the seasonal cycle with
``numpy.linalg.pinv`` and ``dot`` (src/momlevel/trend.py:252, :403-431, :511-532).
"""

import datetime

import numpy as np

_CUM = (0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334)  # days before month m, no leap day


def _julian_day_number(y, m, d, gregorian):
    """the astronomers' day number of a civil date (Fliegel / Van Flandern form)"""
    a = (14 - m) // 12
    yy = y + 4800 - a
    mm = m + 12 * a - 3
    jdn = d + (153 * mm + 2) // 5 + 365 * yy + yy // 4
    return jdn - yy // 100 + yy // 400 - 32045 if gregorian else jdn - 32083


def days_since_1970(year, month, day, calendar):
    """Whole days from 1970-01-01 of ``calendar`` to the date -- by closed forms, not by the
    month-by-month counting of momlevel_amd.cftime_lite."""
    calendar = calendar.lower()
    if calendar in ("noleap", "365_day"):
        return 365 * (year - 1970) + _CUM[month - 1] + day - 1
    if calendar == "360_day":
        return 360 * (year - 1970) + 30 * (month - 1) + day - 1
    if calendar in ("standard", "gregorian", "proleptic_gregorian"):
        return datetime.date(year, month, day).toordinal() - datetime.date(1970, 1, 1).toordinal()
    if calendar == "julian":
        return (_julian_day_number(year, month, day, False)
                - _julian_day_number(1970, 1, 1, False))
    raise ValueError(calendar)


def ns_axis(times):
    """float64 nanoseconds since 1970-01-01 00:00 of each object's own calendar"""
    out = []
    for t in times:
        minutes = (days_since_1970(t.year, t.month, t.day, t.calendar) * 24 + t.hour) * 60 + t.minute
        out.append(float(minutes * 60 * 1_000_000_000))
    return np.array(out, dtype=np.float64)


def polyfit_columns(x, y):
    """``numpy.polyfit(x, column, 1)`` for every column of ``y`` (nt, ...) with the column's NaN
    rows dropped; an all-NaN column gives NaN (xarray's ``_nanpolyfit_1d``).  -> (slope, intercept)
    shaped y.shape[1:], float64."""
    x = np.asarray(x, dtype=np.float64)
    y2 = np.asarray(y).reshape(len(x), -1).astype(np.float64)
    slope = np.full(y2.shape[1], np.nan)
    intercept = np.full(y2.shape[1], np.nan)
    for j in range(y2.shape[1]):
        ok = ~np.isnan(y2[:, j])
        if ok.sum() >= 2:
            slope[j], intercept[j] = np.polyfit(x[ok], y2[ok, j], 1)
    shape = np.asarray(y).shape[1:]
    return slope.reshape(shape), intercept.reshape(shape)


def model_matrix(time_dec):
    """the 6-row model of trend.py:403-410 / :511-520"""
    time_dec = np.asarray(time_dec, dtype=np.float64)
    return np.array([
        np.ones(len(time_dec)),
        time_dec - np.mean(time_dec),
        np.sin(2 * np.pi * time_dec),
        np.cos(2 * np.pi * time_dec),
        np.sin(4 * np.pi * time_dec),
        np.cos(4 * np.pi * time_dec),
    ])


def seasonal_fit(time_dec, y):
    """pinv / dot of trend.py:523-532 on every column of ``y`` (nt, ...): (coeff (6, ...), model
    (nt, ...), residuals (nt, ...)); a NaN step makes its column NaN, as BLAS dot does"""
    y = np.asarray(y)
    y2 = y.reshape(y.shape[0], -1).astype(np.float64)
    model = model_matrix(time_dec)
    pmodel = np.linalg.pinv(model)
    coeff = np.dot(y2.T, pmodel).T            # (6, cells)
    smodel = np.dot(coeff.T, model).T         # (nt, cells)
    bad = np.isnan(y2).any(axis=0)
    coeff[:, bad] = np.nan
    smodel[:, bad] = np.nan
    resid = y2 - smodel
    return (coeff.reshape((6,) + y.shape[1:]), smodel.reshape(y.shape), resid.reshape(y.shape))


def decimal_year(times):
    """year + (dayofyear - 1 + hour / 24) / 365 (trend.py:397-401)"""
    out = []
    for t in times:
        doy = (days_since_1970(t.year, t.month, t.day, t.calendar)
               - days_since_1970(t.year, 1, 1, t.calendar) + 1)
        out.append(t.year + (doy - 1 + t.hour / 24) / 365)
    return np.array(out)
