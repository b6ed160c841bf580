"""CPU: the host side of the trend module -- unit conversion, the numeric time axis, the daily test
data, the units / warning logic of broadcast_trend, the model matrices, and the C ABI of
include/momlevel_trend.h (symbols, binding table, argument errors).  No kernel runs here."""

import ctypes
import importlib
import json
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import trend_numpy as tn
from momlevel_amd import _lib, cftime_lite, test_data, trend
from momlevel_amd.cftime_lite import DatetimeLite
from momlevel_amd.labeled import DataArray
from test_static_names import _undefined

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "momlevel_trend.h")
DAY_NS = 86400.0e9


@pytest.fixture(scope="module")
def trend_goldens():
    with open(os.path.join(ROOT, "tests", "golden", "trend_goldens.json")) as f:
        return json.load(f)


def test_time_conversion_factor(trend_goldens):
    for src, dst, want in trend_goldens["time_conversion_factor"]:
        got = trend.time_conversion_factor(src, dst)
        if (src, dst) == ("mon", "day"):
            assert np.allclose(got, want)
        else:
            assert got == want
    assert trend.time_conversion_factor("yr", "day", days_per_year=360.0) == 360.0
    with pytest.raises(AssertionError):
        trend.time_conversion_factor("fortnight", "day")


@pytest.mark.parametrize("calendar, date, days", [
    # hand-counted whole days since 1970-01-01 of the same calendar
    ("noleap", (1979, 1, 1), 9 * 365),
    ("noleap", (1981, 2, 15), 11 * 365 + 31 + 14),
    ("360_day", (1981, 2, 15), 11 * 360 + 30 + 14),
    ("gregorian", (2000, 3, 1), 30 * 365 + 7 + 31 + 29),       # leap days 1972 ... 1996; 2000 leap
    ("gregorian", (2101, 3, 1), 131 * 365 + 32 + 31 + 28),     # 2100 is no leap year
    ("julian", (2101, 3, 1), 131 * 365 + 33 + 31 + 28),        # ... but it is one in the Julian
    ("julian", (1969, 12, 31), -1),
])
def test_ns_axis_against_hand_counted_days(calendar, date, days):
    t = DatetimeLite(*date, 12, 30, calendar)
    assert cftime_lite.days_since_1970(t) == days
    want = (days + 12.5 / 24) * DAY_NS
    got = cftime_lite.axis_to_numeric(np.array([t], dtype=object))
    assert got.dtype == np.float64 and got[0] == want
    assert tn.ns_axis([t])[0] == want


@pytest.mark.parametrize("calendar", ["noleap", "julian", "gregorian", "360_day"])
@pytest.mark.parametrize("frequency", ["MS", "D"])
def test_ns_axis_of_the_test_data_axes(calendar, frequency):
    d = test_data.generate_test_data_time(start_year=1979, nyears=6, calendar=calendar,
                                          frequency=frequency)
    times = d["time"].values
    x = cftime_lite.axis_to_numeric(times)
    assert np.array_equal(x, tn.ns_axis(times))
    assert (np.diff(x) > 0).all()
    year_days = sum(cftime_lite.days_in_year(y, calendar) for y in range(1979, 1985))
    if frequency == "D":
        assert len(x) == year_days
        assert (np.diff(x) == DAY_NS).all()                      # one step per day, at mid-day
        assert x[0] == (cftime_lite.days_since_1970(times[0]) + 0.5) * DAY_NS
        assert times[0].hour == 12 and (times[0].month, times[0].day) == (1, 1)
        assert (times[-1].month, times[-1].day) == (12, 30 if calendar == "360_day" else 31)
    else:
        assert len(x) == 72
        first = cftime_lite.days_in_month(1979, 1, calendar) / 2.0  # mid-January
        assert x[0] == (9 * cftime_lite.days_in_year(1970, calendar) + first
                        + (2 if calendar in ("julian", "gregorian") else 0)) * DAY_NS


def test_other_axes_keep_their_numbers():
    x = cftime_lite.axis_to_numeric(np.array([1.5, 2.5, 4.0], dtype=np.float32))
    assert x.dtype == np.float64 and x.tolist() == [1.5, 2.5, 4.0]
    t = np.array(["1970-01-02", "2001-03-04T05:06:07"], dtype="datetime64[s]")
    got = cftime_lite.axis_to_numeric(t)
    assert got[0] == DAY_NS and got[1] == float(t[1].astype("datetime64[ns]").astype(np.int64))
    assert not cftime_lite.is_calendar_axis(t) and not cftime_lite.is_calendar_axis(x)


def test_daily_test_data_draws_the_same_numbers():
    d = test_data.generate_test_data_time(start_year=1979, nyears=5, frequency="D")
    nt = 5 * 365
    assert d["var_a"].shape == (nt, 5, 5) and d["var_a"].dims == ("time", "lat", "lon")
    assert np.array_equal(d["var_a"].values, np.random.default_rng(123).normal(100, 20, (nt, 5, 5)))
    assert np.array_equal(d["var_b"].values, np.random.default_rng(246).normal(100, 20, (nt, 5, 5)))
    assert d["var_a"].attrs == {"first_attribute": "foo", "second_attribute": "bar"}
    m = test_data.generate_test_data_time()  # the default is the monthly axis, as before
    assert m["var_a"].shape == (60, 5, 5) and m["time"].values[0] == DatetimeLite(1981, 1, 16, 12)
    with pytest.raises(ValueError):
        test_data.generate_test_data_time(frequency="W")
    from momlevel_amd import timeseries_data
    from momlevel_amd.test_data import generate_test_data_time

    assert generate_test_data_time is timeseries_data.generate_test_data_time  # one function, one place
    assert np.array_equal(m["var_a"].values, np.random.default_rng(123).normal(100, 20, (60, 5, 5)))
    assert list(m.keys()) == ["var_a", "var_b"] and sorted(m.coords) == ["lat", "lon", "time"]


def test_fit_axis_is_centred_and_scaled():
    x = tn.ns_axis(test_data.generate_test_data_time(nyears=2, frequency="D")["time"].values)
    xt, s, xmean = trend.fit_axis(x)
    assert xmean == np.mean(x) and s == np.max(np.abs(x - xmean))
    assert np.max(np.abs(xt)) == 1.0 and abs(xt.sum()) < 1e-9
    assert trend.fit_axis([3.0, 3.0])[1] == 1.0  # a constant axis: scale 1, not 0


def _ready_or_no_device(call):
    """run ``call``; without a device the host logic ends in MomlevelHipError, which is fine here"""
    try:
        call()
    except _lib.MomlevelHipError:
        pass


def test_broadcast_trend_units_and_warning_logic():
    d = test_data.generate_test_data_time(nyears=1)
    slope = DataArray(np.ones((5, 5)), ("lat", "lon"), None, None, "var_a_slope")
    with pytest.warns(UserWarning, match="Unable to determine time unit"):
        _ready_or_no_device(lambda: trend.broadcast_trend(slope, d["time"]))
    slope.attrs["units"] = "m"  # no time unit in it
    with pytest.warns(UserWarning, match="Unable to determine time unit"):
        _ready_or_no_device(lambda: trend.broadcast_trend(slope, d["time"]))
    slope.attrs["units"] = "m yr-1 s-1"
    with pytest.raises(ValueError, match="multiple time definitions"):
        trend.broadcast_trend(slope, d["time"])
    for units in (" ns-1", "m  yr-1", " day-1"):
        slope.attrs["units"] = units
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            _ready_or_no_device(lambda: trend.broadcast_trend(slope, d["time"]))
    # a numeric axis has no unit handling at all: no warning without a units attribute
    slope.attrs.clear()
    axis = DataArray(np.arange(4.0), ("time",), None, None, "time")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _ready_or_no_device(lambda: trend.broadcast_trend(slope, axis))
    with pytest.raises(AssertionError):
        trend.broadcast_trend(np.ones(3), d["time"])
    with pytest.raises(AssertionError):
        trend.broadcast_trend(slope, d["var_a"])


def test_argument_checks_of_the_public_functions():
    d = test_data.generate_test_data_time(nyears=1)
    with pytest.raises(AssertionError):
        trend.linear_detrend(d["var_a"], order=2)
    with pytest.raises(ValueError, match="Unknown detrend mode"):
        trend.linear_detrend(d["var_a"], mode="flatten")
    with pytest.raises(TypeError):
        trend.linear_detrend(np.ones(4))
    with pytest.raises(ValueError, match="not recognized"):
        trend.deseason(d["var_a"], output_format="phase")
    with pytest.raises(AssertionError):
        trend.deseason(d["var_a"], tdim="t")


def test_model_matrices():
    d = test_data.generate_test_data_time(start_year=1979, nyears=5, frequency="D",
                                          calendar="gregorian")
    times = d["time"].values
    dec = trend.decimal_year(times)
    assert np.array_equal(dec, tn.decimal_year(times))
    assert dec[0] == 1979 + 0.5 / 365 and dec[-1] == 1983 + (364 + 0.5) / 365
    assert np.isclose(trend.decimal_year(times[365 + 59:365 + 60])[0], 1980 + 59.5 / 365)  # Feb 29
    model, pmodel = trend.seasonal_model_matrix(dec)
    assert model.shape == (6, len(times)) and pmodel.shape == (len(times), 6)
    assert np.array_equal(model, tn.model_matrix(dec))
    assert np.array_equal(pmodel, np.linalg.pinv(tn.model_matrix(dec)))
    assert np.allclose(model @ pmodel, np.eye(6), atol=1e-9)
    # deseason: arange(nt) / daysinyear[t], the leap year's steps divided by 366
    dd = trend.deseason_decimal_year(times)
    assert dd[0] == 0.0 and dd[364] == 364 / 365 and dd[365] == 365 / 366 and dd[731] == 731 / 365
    # numpy.datetime64 axes give the same decimal year as the calendar objects
    t64 = np.array([f"{t.year:04d}-{t.month:02d}-{t.day:02d}T{t.hour:02d}" for t in times],
                   dtype="datetime64[h]")
    assert np.array_equal(trend.decimal_year(t64), dec)
    with pytest.raises(TypeError):
        trend.deseason_decimal_year(t64)


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mlx_[a-z0-9_]+)\s*\(", text)))


def test_trend_header_binding_and_exports_agree():
    declared = _declared(HEADER)
    assert declared == sorted(_lib.TREND_SIGNATURES) and len(declared) == 4
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in momlevel_trend.h but not exported"
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                             text=True, check=True).stdout
        exported = sorted(set(re.findall(r"\b(mlx_time_[a-z0-9_]+)\b", out)))
        assert exported == declared
    text = open(HEADER).read()
    for name, val in re.findall(r"#define (MLX_[A-Z0-9_]+)\s+\(?(-?\d+)\)?", text):
        assert getattr(_lib, name[4:]) == int(val), name
    assert _lib.load_trend() is _lib.load()


def test_the_main_abi_is_untouched():
    main = _declared(os.path.join(ROOT, "include", "momlevel_hip.h"))
    assert len(main) == 28 and len(_lib.SIGNATURES) == 28
    assert not set(main) & set(_lib.TREND_SIGNATURES)
    assert _lib.ABI_VERSION == 9 and _lib.load().mlx_version() == 9


def test_argument_errors_need_no_gpu():
    lib = _lib.load_trend()
    f = 1 << 20  # 16-byte aligned, non-NULL, never dereferenced: the checks precede every HIP call
    big = 1 << 30
    F64, F32 = _lib.DTYPE_F64, _lib.DTYPE_F32
    assert lib.mlx_time_fit_workspace_bytes(0, 10, 5) == 0
    assert lib.mlx_time_fit_workspace_bytes(10, 10, 9) == 0
    assert lib.mlx_time_fit_workspace_bytes(100, 10, 5) == 5 * 10 * 8        # one window
    assert lib.mlx_time_fit_workspace_bytes(1200, 10, 6) == 5 * 6 * 10 * 8   # windows of 256 steps
    assert lib.mlx_time_fit_workspace_bytes(1 << 20, 3, 1) == 16 * 3 * 8     # never more than 16

    def linfit(y=f, dtype=F64, xt=f, nt=10, n=10, s=1.0, slope=f, icpt=f, ws=f, wsb=big):
        return lib.mlx_time_linfit(y, dtype, xt, nt, n, s, 0.0, slope, icpt, ws, wsb, None)

    for kw in (dict(y=None), dict(xt=None), dict(slope=None), dict(icpt=None), dict(ws=None)):
        assert linfit(**kw) == -1 and "NULL" in _lib.last_error()
    for kw in (dict(nt=0), dict(n=0), dict(nt=-3), dict(nt=1 << 31), dict(s=0.0)):
        assert linfit(**kw) == -2 and _lib.last_error()
    assert linfit(dtype=7) == -3
    assert linfit(wsb=8) == -4 and linfit(ws=f + 8) == -4
    assert linfit(y=f + 4) == -5 and linfit(y=f + 2, dtype=F32) == -5

    def project(y=f, P=f, K=6, nt=10, n=10, coef=f, ws=f, wsb=big):
        return lib.mlx_time_project(y, F32, P, K, nt, n, coef, ws, wsb, None)

    for kw in (dict(y=None), dict(P=None), dict(coef=None), dict(ws=None)):
        assert project(**kw) == -1 and "NULL" in _lib.last_error()
    for kw in (dict(K=0), dict(K=9), dict(nt=0), dict(n=-1)):
        assert project(**kw) == -2 and _lib.last_error()
    assert project(wsb=0) == -4

    def apply(y=f, mode=_lib.APPLY_REMOVE, xm=f, a=f, b=f, K=0, nt=10, n=10, out=f):
        return lib.mlx_time_apply(y, F64, mode, xm, a, b, K, nt, n, out, None)

    for kw in (dict(y=None), dict(xm=None), dict(a=None), dict(b=None), dict(out=None),
               dict(y=None, mode=_lib.APPLY_MODEL_RESID, K=6)):
        assert apply(**kw) == -1 and "NULL" in _lib.last_error()
    for kw in (dict(nt=0), dict(n=0), dict(nt=65535 * 64 + 1), dict(mode=_lib.APPLY_MODEL, K=0),
               dict(mode=_lib.APPLY_MODEL_RESID, K=9)):
        assert apply(**kw) == -2 and _lib.last_error()
    assert apply(mode=6) == -3 and apply(mode=-1) == -3
    assert apply(out=f + 4) == -5


def test_a_library_without_the_trend_kernels_is_an_error(monkeypatch):
    class Bare:
        def __getattr__(self, name):
            raise AttributeError(name)

    monkeypatch.setattr(_lib, "_trend_bound", False)
    monkeypatch.setattr(_lib, "load", lambda: Bare())
    with pytest.raises(_lib.MomlevelHipError, match="does not export mlx_time"):
        _lib.load_trend()


def test_trend_source_sha_is_its_own():
    from momlevel_amd.csrc import build

    assert len(build.trend_source_sha()) == 16 and build.trend_source_sha() != build.source_sha()
    names = {os.path.basename(p) for p in build.TIMED_SOURCES}
    assert "momlevel_trend.hip" not in names and "momlevel_trend.h" not in names
    assert any(p.endswith("momlevel_trend.hip") for p in build.SOURCES)


def test_no_undefined_globals_in_the_trend_module():
    assert _undefined(importlib.import_module("momlevel_amd.trend")) == []
    assert _undefined(importlib.import_module("momlevel_amd.cftime_lite")) == []
    assert _undefined(importlib.import_module("momlevel_amd.timeseries_data")) == []
