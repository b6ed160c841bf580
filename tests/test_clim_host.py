"""CPU: the host side of the grouped time statistics -- the calendar plans of monthly_average and
annual_cycle (momlevel_amd.climatology), the checks of a group list, the numpy restatement against
the reference's goldens, and the C ABI of include/momlevel_clim.h (symbol, binding table, argument
errors).  No kernel runs here."""

import ctypes
import importlib
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import clim_numpy as cn
from momlevel_amd import _lib, cftime_lite, climatology, test_data, util
from momlevel_amd.cftime_lite import DatetimeLite
from momlevel_amd.labeled import DataArray
from test_static_names import _undefined

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "momlevel_clim.h")


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "clim_goldens.json")) as f:
        return json.load(f)


def _axis(values, name="time"):
    a = np.empty(len(values), dtype=object)
    a[:] = list(values)
    return DataArray(a, (name,), None, None, name)


# ---- plans ------------------------------------------------------------------------------------
def test_monthly_plan_group_sizes_in_a_leap_year():
    time = _axis(cftime_lite.daily_midpoints(1980, 2, "standard"))  # 1980 is a leap year
    plan = climatology.monthly_plan(time)
    assert plan.ngroups == 24
    assert plan.sizes[:12] == [31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]
    assert plan.sizes[12:] == [31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]
    assert plan.steps.dtype == np.int32 and plan.offsets.dtype == np.int64
    assert np.array_equal(plan.steps, np.arange(366 + 365))  # back to back, ascending
    assert np.array_equal(plan.offsets, np.concatenate([[0], np.cumsum(plan.sizes)]))
    noleap = climatology.monthly_plan(_axis(cftime_lite.daily_midpoints(1980, 1, "noleap")))
    assert noleap.sizes[1] == 28
    julian = climatology.monthly_plan(_axis(cftime_lite.daily_midpoints(1900, 1, "julian")))
    assert julian.sizes[1] == 29  # 1900 is a leap year in the Julian calendar only
    assert climatology.monthly_plan(_axis(cftime_lite.daily_midpoints(1900, 1, "standard"))).sizes[1] == 28


def test_monthly_plan_axis_is_the_monthly_midpoints():
    for calendar in ("noleap", "standard", "julian"):
        plan = climatology.monthly_plan(_axis(cftime_lite.daily_midpoints(1979, 3, calendar)), "time")
        assert plan.time.dims == ("time",) and plan.time.name == "time"
        assert list(plan.time.values) == cftime_lite.monthly_midpoints(1979, 3, calendar)
    # years need not be consecutive, steps need not be sorted: a group lists its steps in axis order
    days = cftime_lite.daily_midpoints(1990, 1, "noleap") + cftime_lite.daily_midpoints(1985, 1, "noleap")
    plan = climatology.monthly_plan(_axis(days))
    assert list(plan.time.values) == (cftime_lite.monthly_midpoints(1985, 1, "noleap")
                                      + cftime_lite.monthly_midpoints(1990, 1, "noleap"))
    assert np.array_equal(plan.steps[:31], 365 + np.arange(31))  # January 1985 comes first


def test_annual_cycle_plan_groups_and_axis():
    time = _axis(cftime_lite.monthly_midpoints(1979, 5, "noleap"))
    plan = climatology.annual_cycle_plan(time)
    assert plan.ngroups == 12 and plan.sizes == [5] * 12
    assert np.array_equal(plan.steps[:5], [0, 12, 24, 36, 48])       # all Januaries
    assert np.array_equal(plan.steps[-5:], [11, 23, 35, 47, 59])     # all Decembers
    # the mid-year rule: start + (end - start) / 2 of 1979-01-16 12:00 .. 1983-12-16 12:00 is in 1981
    assert climatology.mid_year(time.values[0], time.values[-1]) == 1981
    assert list(plan.time.values) == cftime_lite.monthly_midpoints(1981, 1, "noleap")
    over = climatology.annual_cycle_plan(time, time_axis_year=2001)
    assert list(over.time.values) == cftime_lite.monthly_midpoints(2001, 1, "noleap")
    leap = climatology.annual_cycle_plan(_axis(cftime_lite.monthly_midpoints(1979, 5, "standard")),
                                         time_axis_year="1984")
    assert leap.time.values[1] == DatetimeLite(1984, 2, 15, 12, 0, "standard")  # 29 days: mid 15th 12:00
    # a daily record is grouped by month just the same
    daily = climatology.annual_cycle_plan(_axis(cftime_lite.daily_midpoints(1979, 2, "noleap")))
    assert daily.sizes == [62, 56, 62, 60, 62, 60, 62, 62, 60, 62, 60, 62]


def test_mid_year_rule():
    a = DatetimeLite(1979, 1, 1, 0, 0, "standard")
    assert climatology.mid_year(a, DatetimeLite(1980, 12, 30, 0, 0, "standard")) == 1979  # 1979-12-31 12:00
    assert climatology.mid_year(a, DatetimeLite(1980, 12, 31, 0, 0, "standard")) == 1980  # 1980-01-01 00:00
    assert climatology.mid_year(a, DatetimeLite(1981, 1, 1, 0, 0, "standard")) == 1980    # 1980-01-01 12:00
    assert climatology.mid_year(a, a) == 1979


def test_value_errors():
    days = cftime_lite.daily_midpoints(1979, 2, "noleap")
    with pytest.raises(ValueError, match="year 1980 lacks the calendar months \\[12\\]"):
        climatology.monthly_plan(_axis(days[:-31]))
    months = cftime_lite.monthly_midpoints(1979, 2, "noleap")
    with pytest.raises(ValueError, match="lacks the calendar months \\[3\\]"):
        climatology.annual_cycle_plan(_axis([t for t in months if t.month != 3]))
    dset = test_data.generate_test_data_time(nyears=2)
    with pytest.raises(ValueError) as exc:
        util.annual_cycle(dset, func="median")
    assert str(exc.value) == "Unknown argument 'func=median' to annual cycle"
    with pytest.raises(ValueError, match="lacks the calendar months"):
        util.annual_cycle(dset.isel(time=slice(0, 7)))
    with pytest.raises(TypeError, match="calendar objects"):
        climatology.monthly_plan(_axis(list(range(24))))
    half = DataArray(np.zeros((24, 3), dtype=np.float16), ("time", "x"),
                     {"time": dset["time"]}, None, "h")
    with pytest.raises(TypeError, match="float16 records are not supported"):
        util.annual_cycle(half)


def test_exports():
    assert "monthly_average" in util.__all__ and "annual_cycle" in util.__all__
    import momlevel_amd

    assert momlevel_amd.util.annual_cycle is util.annual_cycle
    assert momlevel_amd.util.monthly_average is util.monthly_average
    assert _undefined(importlib.import_module("momlevel_amd.climatology")) == []
    assert _undefined(importlib.import_module("momlevel_amd.util")) == []


def test_check_groups_refuses_on_the_host():
    from momlevel_amd import core

    steps, offsets = core.check_groups([0, 2, 1, 1], [0, 0, 3, 4], nt=3)
    assert steps.dtype == np.int32 and offsets.dtype == np.int64  # empty and repeated groups are fine
    for bad_steps, bad_offsets in (([0, 3], [0, 2]), ([-1, 0], [0, 2]), ([0, 1], [0, 2, 1]),
                                   ([0, 1], [0, 3]), ([0, 1], [-1, 2]), ([], [0, 0]), ([0], [0]),
                                   ([0.5], [0, 1])):
        with pytest.raises(ValueError):
            core.check_groups(bad_steps, bad_offsets, nt=3)


# ---- the numpy restatement reproduces the reference's goldens ---------------------------------
def test_restatement_reproduces_the_goldens(gold):
    for case in gold["monthly_average"]:
        dset = test_data.generate_test_data_time(**case["dataset"])
        for var in ("var_a", "var_b"):
            got = cn.monthly_average(dset[var].values, dset["time"].values).sum()
            assert abs(got - case[var]) <= 1e-9 * abs(case[var]), (case, var, got)
    for case in gold["annual_cycle_of_monthly_average"]:
        dset = test_data.generate_test_data_time(**case["dataset"])
        mids = cftime_lite.monthly_midpoints(case["dataset"]["start_year"], case["dataset"]["nyears"],
                                             case["dataset"]["calendar"])
        for var in ("var_a", "var_b"):
            monthly = cn.monthly_average(dset[var].values, dset["time"].values)
            got = cn.annual_cycle(monthly, mids, case["func"]).sum()
            assert abs(got - case[var]) <= 1e-9 * abs(case[var]), (case, var, got)


# ---- the C ABI --------------------------------------------------------------------------------
def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mlx_[a-z0-9_]+)\s*\(", text)))


def test_clim_header_binding_and_exports_agree():
    declared = _declared(HEADER)
    assert declared == sorted(_lib.CLIM_SIGNATURES) == ["mlx_clim_group_stat"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in momlevel_clim.h but not exported"
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                             text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(mlx_clim_[a-z0-9_]+)\b", out))) == declared
    # the prototype, argument for argument: 11 arguments, int status
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    proto = re.search(r"int\s+mlx_clim_group_stat\s*\(([^)]*)\)", text).group(1)
    args = [" ".join(a.split()) for a in proto.split(",")]
    ctype = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p,
             "const int32_t *": ctypes.c_void_p, "const int64_t *": ctypes.c_void_p,
             "int64_t ": ctypes.c_int64, "int ": ctypes.c_int}
    want = [next(v for k, v in ctype.items() if a.startswith(k)) for a in args]
    restype, argtypes = _lib.CLIM_SIGNATURES["mlx_clim_group_stat"]
    assert restype is ctypes.c_int and argtypes == want
    consts = re.findall(r"#define (MLX_[A-Z0-9_]+)\s+\(?(-?\d+)\)?", open(HEADER).read())
    assert [n for n, _ in consts] == ["MLX_STAT_MEAN", "MLX_STAT_STD", "MLX_STAT_MIN", "MLX_STAT_MAX"]
    for name, val in consts:
        assert getattr(_lib, name[4:]) == int(val), name
    assert _lib.load_clim() is _lib.load()
    # the main ABI and the trend table do not know the symbol; the version has not moved
    assert "mlx_clim_group_stat" not in _lib.SIGNATURES and "mlx_clim_group_stat" not in _lib.TREND_SIGNATURES
    assert _lib.ABI_VERSION == 9 and _lib.load().mlx_version() == 9


def test_argument_errors_need_no_gpu():
    lib = _lib.load_clim()
    f = 1 << 20  # 16-byte aligned, non-NULL, never dereferenced: the checks precede every HIP call
    F64, F32 = _lib.DTYPE_F64, _lib.DTYPE_F32

    def stat(y=f, dtype=F64, steps=f, offsets=f, nsel=12, ngroups=3, nt=12, n=10,
             what=_lib.STAT_MEAN, out=f):
        return lib.mlx_clim_group_stat(y, dtype, steps, offsets, nsel, ngroups, nt, n, what, out, None)

    for kw in (dict(y=None), dict(steps=None), dict(offsets=None), dict(out=None)):
        assert stat(**kw) == -1 and "NULL" in _lib.last_error()
    for kw in (dict(nt=0), dict(n=0), dict(ngroups=0), dict(nsel=0), dict(nt=-3), dict(n=-1),
               dict(ngroups=-2), dict(nt=1 << 31), dict(n=(1 << 38) + 1)):
        assert stat(**kw) == -2 and _lib.last_error()
    assert stat(dtype=7) == -3 and stat(dtype=_lib.DTYPE_F32_UPCAST) == -3
    assert stat(what=4) == -3 and stat(what=-1) == -3 and "MLX_STAT" in _lib.last_error()
    assert stat(y=f + 4) == -5 and stat(y=f + 2, dtype=F32) == -5 and stat(out=f + 4) == -5
    assert stat(steps=f + 2) == -5 and stat(offsets=f + 4) == -5


def test_a_library_without_the_kernel_is_an_error(monkeypatch):
    class Bare:
        def __getattr__(self, name):
            raise AttributeError(name)

    monkeypatch.setattr(_lib, "_clim_bound", False)
    monkeypatch.setattr(_lib, "load", lambda: Bare())
    with pytest.raises(_lib.MomlevelHipError, match="does not export mlx_clim_group_stat"):
        _lib.load_clim()


def test_clim_source_sha_is_its_own():
    from momlevel_amd.csrc import build

    assert len(build.clim_source_sha()) == 16
    assert build.clim_source_sha() not in (build.source_sha(), build.trend_source_sha())
    names = {os.path.basename(p) for p in build.TIMED_SOURCES}
    assert "momlevel_clim.hip" not in names and "momlevel_clim.h" not in names
    assert any(p.endswith("momlevel_clim.hip") for p in build.SOURCES)
    assert any(p.endswith("momlevel_clim.h") for p in build.DEPENDS)
