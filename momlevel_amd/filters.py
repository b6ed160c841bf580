"""filters - smoothing along time on the GPU: rolling means and sums, Lanczos low-pass filters,
arbitrary FIR weights and running least-squares trends of a (time, ...) record.

EXTENSION: momlevel has no such functions.  They are the step that happens to almost every sea-level
record before anyone looks at it: a centred 12- or 13-month running mean to take the seasons out, a
low-pass to isolate decadal variability, the rate of rise over sliding 20-year windows, a 30-day
mean of a daily gauge series.

All of them are ONE kernel (csrc/momlevel_filter.hip, ``core.time_filter``), a banded linear
operator along time,

    out[t] = sum_k w[t, k] * y[t - lead + k],   k = 0 .. W-1,

with different weight tables made here, on the host, from what depends on the time axis alone.  A
step is *valid* when it lies inside the record and is not NaN; invalid steps add nothing; fewer than
``min_count`` valid steps give NaN; the normalised form divides by the sum of the valid steps'
weights.  The sum runs in float64 with k ascending, every output summed afresh
(include/momlevel_filter.h states the contract, tests/filter_numpy.py restates it in numpy).

Placement is the record module's (``record.Record``): device in, device out; host arrays in blocks
of cells.  Each cell is filtered on its own, so the block size never changes a bit of the result.
The time axis and the order of the dims come back as they went in.

Dtypes: float32 records give float32 (the float64 result rounded once, the convention of the
grouped statistics); everything else is computed and returned as float64.  ``rolling_trend`` always
gives float64.
"""

import numpy as np

from . import cftime_lite
from .adapters import accepts_xarray
from .record import Record, axis_values, check_record_dtype, over, per_device, slope_units

__all__ = [
    "rolling_mean",
    "rolling_sum",
    "time_filter",
    "lanczos_weights",
    "lowpass",
    "rolling_trend",
    "window_lead",
    "trend_table",
]


# ---------------------------------------------------------------------------------------
# what depends on the window and the time axis alone: made here, on the host
# ---------------------------------------------------------------------------------------
def window_lead(window, center=True):
    """Steps of a window that lie BEFORE its output step.  Centred: ``window // 2``, so the window
    of step t is ``[t - window // 2, t + (window - 1) // 2]`` (the pandas / xarray convention for
    even windows); trailing: ``window - 1``, the window ``[t - window + 1, t]``."""
    window = _window(window)
    return window // 2 if center else window - 1


def _window(window, nt=None):
    if int(window) != window or int(window) < 1:
        raise ValueError(f"window must be a whole number of steps >= 1, got {window}")
    window = int(window)
    if nt is not None and window > nt:
        raise ValueError(f"window ({window} steps) is longer than the record ({nt} steps)")
    return window


def _min_periods(min_periods, window, default):
    if min_periods is None:
        return default
    if int(min_periods) != min_periods or not 1 <= int(min_periods) <= window:
        raise ValueError(f"min_periods must lie in [1, {window}], got {min_periods}")
    return int(min_periods)


def lanczos_weights(window, cutoff):
    """Lanczos low-pass weights (Duchon 1979) of an odd ``window = 2m + 1``:
    ``w_k = 2 fc sinc(2 fc k) sinc(k / (m + 1))`` for k = -m .. m with ``fc = 1 / cutoff`` in cycles
    per step (``cutoff``: the period, in steps, above which variability passes) and numpy's
    normalised sinc, divided by their sum.  float64, host-side numpy."""
    window = _window(window)
    if window % 2 == 0:
        raise ValueError(f"a Lanczos window is odd (2m + 1), got {window}")
    cutoff = float(cutoff)
    if not (np.isfinite(cutoff) and cutoff > 0.0):
        raise ValueError(f"cutoff must be a positive number of steps, got {cutoff}")
    m = (window - 1) // 2
    k = np.arange(-m, m + 1, dtype=np.float64)
    fc = 1.0 / cutoff
    w = 2.0 * fc * np.sinc(2.0 * fc * k) * np.sinc(k / (m + 1))
    return w / np.sum(w)


def trend_table(x, window, lead):
    """The ``(nt, window)`` table of a running least-squares slope against the abscissa ``x``:
    row t holds ``B[t, k] = (x_k - xbar_t) / sum_j (x_j - xbar_t)^2`` over the steps
    ``t - lead + k`` of its window, in float64, so that ``sum_k B[t, k] y_k`` is the slope of the
    straight-line fit to that window.  Rows of windows that leave the record are zero (the kernel
    gives NaN there: ``min_count = window``).  A window on which ``x`` does not vary is a
    ``ValueError``."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    nt = x.size
    window = _window(window, nt)
    if window < 2:
        raise ValueError("a trend needs a window of at least 2 steps")
    if not 0 <= int(lead) < window:
        raise ValueError(f"lead must lie in [0, {window}), got {lead}")
    table = np.zeros((nt, window), dtype=np.float64)
    first = np.arange(nt - window + 1)  # first step of every complete window
    xs = x[first[:, None] + np.arange(window)[None, :]]
    d = xs - np.mean(xs, axis=1, keepdims=True)
    ss = np.sum(d * d, axis=1, keepdims=True)
    if not (np.all(np.isfinite(ss)) and np.all(ss > 0.0)):
        raise ValueError("the time coordinate does not vary (or is not finite) over some window")
    table[first + int(lead)] = d / ss
    return table


# ---------------------------------------------------------------------------------------
# the record through the kernel
# ---------------------------------------------------------------------------------------
def _filter_array(da, tcoord, weights, lead, min_count, normalise, float64_out=False):
    """one DataArray through ``core.time_filter``; ``weights``: (W,) or (nt, W), host float64 ->
    ``(record, result (nt, cells...))``"""
    import torch

    from . import core, hostio

    check_record_dtype(da)
    rec = Record(da, tcoord)
    weights = core.filter_weights(weights, rec.nt)
    uploaded = per_device(lambda device: hostio.to_device(weights, device, torch.float64).contiguous())

    def block(y, _cells):
        return (core.time_filter(y, uploaded(y.device), lead, min_count, normalise,
                                 out_dtype=torch.float64 if float64_out else None),)

    (res,) = rec.walk(block, 1, 0)
    return rec, res


def _rolling(xobj, window, tcoord, center, min_periods, normalise):
    def one(da):
        w = _window(window, da.sizes[tcoord])
        mp = _min_periods(min_periods, w, w)
        rec, data = _filter_array(da, tcoord, np.ones(w), window_lead(w, center), mp, normalise)
        return rec.labeled(data)

    _min_periods(min_periods, _window(window), _window(window))  # (refused before any variable)
    return over(xobj, tcoord, one)


# ---------------------------------------------------------------------------------------
# public functions
# ---------------------------------------------------------------------------------------
@accepts_xarray
def rolling_mean(xobj, window, tcoord="time", center=True, min_periods=None):
    """Running mean over ``window`` steps of ``tcoord``: the values of xarray's
    ``.rolling({tcoord: window}, center=center, min_periods=min_periods).mean()``.

    The window of step t is ``[t - window // 2, t + (window - 1) // 2]`` when centred (the pandas /
    xarray convention for even windows) and ``[t - window + 1, t]`` otherwise.  The mean skips NaN
    and runs over the steps of the window that exist: a step with fewer than ``min_periods``
    (default ``window``) valid steps in its window is NaN -- with the default, the half-window at
    each end and every window that holds a NaN.  Weights of 1, normalised by the count of valid
    steps, summed in float64 in time order.  float32 records give float32 (the float64 mean rounded
    once); everything else gives float64.  A DataArray, or every numeric variable of a Dataset that
    has ``tcoord``."""
    return _rolling(xobj, window, tcoord, center, min_periods, True)


@accepts_xarray
def rolling_sum(xobj, window, tcoord="time", center=True, min_periods=None):
    """Running NaN-skipping sum over ``window`` steps of ``tcoord``: ``rolling_mean``'s windows and
    ``min_periods`` without the division."""
    return _rolling(xobj, window, tcoord, center, min_periods, False)


@accepts_xarray
def time_filter(xobj, weights, tcoord="time", center=True, lead=None, skipna=False,
                min_periods=None):
    """Apply 1-D ``weights`` along ``tcoord``: ``out[t] = sum_k weights[k] * y[t - lead + k]`` (the
    weights are applied as listed, not reversed: for a symmetric filter that is the convolution).

    ``lead``: steps of the window before its output step; default ``len(weights) // 2`` when
    ``center``, else ``len(weights) - 1`` (a trailing window).  ``skipna=False``: the plain sum --
    NaN wherever the window holds a NaN or leaves the record, that is within a half-window of the
    ends.  ``skipna=True``: invalid steps are left out and the sum is divided by the sum of the
    weights present; at least ``min_periods`` (default 1) valid steps, else NaN."""
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim != 1 or w.size < 1:
        raise ValueError("weights must be a 1-D sequence of at least one weight")
    if not np.isfinite(w).all():
        raise ValueError("weights must be finite")
    W = int(w.size)
    if lead is None:
        lead = window_lead(W, center)
    if int(lead) != lead or not 0 <= int(lead) < W:
        raise ValueError(f"lead must lie in [0, {W}), got {lead}")
    if min_periods is not None and not skipna:
        raise ValueError("min_periods needs skipna=True: the plain sum wants every step")
    mp = _min_periods(min_periods, W, 1) if skipna else W

    def one(da):
        _window(W, da.sizes[tcoord])
        rec, data = _filter_array(da, tcoord, w, int(lead), mp, bool(skipna))
        return rec.labeled(data)

    return over(xobj, tcoord, one)


@accepts_xarray
def lowpass(xobj, cutoff, window=None, tcoord="time", edges="nan"):
    """Lanczos low-pass along ``tcoord``: ``time_filter`` with ``lanczos_weights(window, cutoff)``,
    centred.  ``cutoff``: the period in steps above which variability passes.  ``window`` defaults
    to the smallest odd number >= ``3 * cutoff``.  ``edges="nan"``: the half-windows at both ends
    (and every window that holds a NaN) are NaN; ``edges="renormalise"``: missing steps are left out
    and the weights present renormalised, as long as ``m + 1`` of the ``2m + 1`` steps are valid."""
    if edges not in ("nan", "renormalise"):
        raise ValueError(f"edges must be 'nan' or 'renormalise', got '{edges}'")
    if window is None:
        window = int(np.ceil(3.0 * float(cutoff)))
        window += 1 - window % 2
    w = lanczos_weights(window, cutoff)
    m = (w.size - 1) // 2
    if edges == "nan":
        return time_filter(xobj, w, tcoord=tcoord, center=True)
    return time_filter(xobj, w, tcoord=tcoord, center=True, skipna=True, min_periods=m + 1)


@accepts_xarray
def rolling_trend(xobj, window, tcoord="time", time_units=None, center=True):
    """Least-squares slope of every complete, NaN-free window of ``window`` steps against the actual
    time coordinate (``cftime_lite.axis_to_numeric``, as ``calc_linear_trend``: months of unequal
    length count): the rate of rise over sliding windows.

    The host builds the table ``B[t, k] = (x_k - xbar_t) / sum_j (x_j - xbar_t)^2`` in float64
    (``trend_table``) and the kernel applies row t to the window of step t.  A window that leaves
    the record or holds a NaN step gives NaN: a NaN-skipping fit is not a fixed linear operator and
    is out of scope.  The result is float64 and named ``<name>_slope``; windows are placed as in
    ``rolling_mean``.  For a calendar axis slope and ``units`` attribute are converted to
    ``time_units`` by ``record.slope_units``, as in ``calc_linear_trend``."""
    def one(da):
        w = _window(window, da.sizes[tcoord])
        lead = window_lead(w, center)
        axis = axis_values(da, tcoord)
        table = trend_table(cftime_lite.axis_to_numeric(axis), w, lead)
        rec, slope = _filter_array(da, tcoord, table, lead, w, False, float64_out=True)
        attrs = dict(da.attrs)
        attrs["comment"] = f"Slope of linear trend over running windows of {w} steps"
        if cftime_lite.is_calendar_axis(axis):
            factor, attrs["units"] = slope_units(attrs, time_units)
            slope = slope * factor
        return rec.labeled(slope, attrs=attrs, name=f"{da.name}_slope")

    return over(xobj, tcoord, one)
