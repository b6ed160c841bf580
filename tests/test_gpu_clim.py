"""GPU: util.monthly_average / util.annual_cycle (momlevel_amd.climatology; csrc/momlevel_clim.hip)
against the reference's own goldens and against the numpy restatement tests/clim_numpy.py.

Gates (none taken from what the kernel gives):
  * the reference's goldens (tests/golden/clim_goldens.json), rtol 1e-9: they are printed to that
    many digits and were reproduced to all of them with numpy alone (tests/test_clim_host.py);
  * float64: every statistic BIT-equal to numpy's nanmean / nanstd / nanmin / nanmax over axis 0 of
    the selected rows, NaN placement included -- the arithmetic contract of include/momlevel_clim.h;
  * float32: bit-equal to the float64 restatement rounded once to float32.
The test fields hold no negative zeros, so numpy's sign of a zero sum is not part of what is asked.
Every compared figure is printed before it is asserted.
"""

import json
import os

import numpy as np
import pytest
import torch

import clim_numpy as cn
from conftest import assert_bit_equal
from momlevel_amd import cftime_lite, climatology, core, record, test_data, util
from momlevel_amd.labeled import DataArray, Dataset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = ("mean", "std", "min", "max")


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "clim_goldens.json")) as f:
        return json.load(f)


def _close(got, want, what):
    got = float(got)
    print(f"{what}: got {got!r} golden {want!r} rel {abs(got - want) / abs(want):.2e}")
    assert abs(got - want) <= 1e-9 * abs(want), what


def _bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} vs {want.dtype}"
    both = ~np.isnan(want) & ~np.isnan(got)
    differ = int(np.sum(got[both] != want[both]))
    print(f"{what}: shape {got.shape} {got.dtype}, NaN got {int(np.isnan(got).sum())} "
          f"want {int(np.isnan(want).sum())}, finite values that differ: {differ} of {int(both.sum())}")
    assert_bit_equal(got, want, what)


def _axis(values):
    a = np.empty(len(values), dtype=object)
    a[:] = list(values)
    return DataArray(a, ("time",), None, None, "time")


def _monthly_axis(nyears, calendar="noleap", start=1979):
    return _axis(cftime_lite.monthly_midpoints(start, nyears, calendar))


def _on_device(da):
    out = DataArray(torch.from_numpy(np.ascontiguousarray(da.values)).cuda(), da.dims, da.coords,
                    da.attrs, da.name)
    out.encoding = dict(da.encoding)
    return out


def _field(shape, seed, dtype=np.float64):
    """a noisy field, time leading: land cells (every step NaN) and cells with a few NaN steps"""
    rng = np.random.default_rng(seed)
    y = rng.normal(100.0, 20.0, shape)
    flat = y.reshape(shape[0], -1)
    cells = flat.shape[1]
    flat[:, rng.random(cells) < 0.2] = np.nan                      # land
    holes = rng.random(flat.shape) < 0.05                          # some NaN steps
    flat[holes] = np.nan
    if cells > 3:
        flat[: shape[0] - 1, 3] = np.nan                           # one valid step in the whole record
    return y.astype(dtype)


# ---- (a) the reference's goldens through the public functions -------------------------------
def test_goldens_monthly_average(gold):
    for case in gold["monthly_average"]:
        kw = case["dataset"]
        dset = test_data.generate_test_data_time(**kw)
        res = util.monthly_average(dset)
        assert isinstance(res, Dataset) and sorted(res.keys()) == ["var_a", "var_b"]
        assert list(res["time"].values) == cftime_lite.monthly_midpoints(
            kw["start_year"], kw["nyears"], kw["calendar"])
        for var in ("var_a", "var_b"):
            assert res[var].dims == ("time", "lat", "lon") and res[var].shape == (24, 5, 5)
            assert res[var].dtype == np.float64 and res[var].attrs["first_attribute"] == "foo"
            _close(res[var].values.sum(), case[var], f"monthly_average {kw['calendar']} Dataset {var}")
            one = util.monthly_average(dset[var])
            assert isinstance(one, DataArray) and one.name == var and one.dims == ("time", "lat", "lon")
            _close(one.values.sum(), case[var], f"monthly_average {kw['calendar']} DataArray {var}")
            _bits(one.values, res[var].values, "DataArray and Dataset paths")
            _bits(one.values, cn.monthly_average(dset[var].values, dset["time"].values),
                  f"monthly_average {kw['calendar']} {var} against numpy")


def test_goldens_annual_cycle(gold):
    for case in gold["annual_cycle_of_monthly_average"]:
        kw, func = case["dataset"], case["func"]
        dset = test_data.generate_test_data_time(**kw)
        res = util.annual_cycle(util.monthly_average(dset), func=func)
        assert isinstance(res, Dataset) and len(res["time"]) == 12
        assert list(res["time"].values) == cftime_lite.monthly_midpoints(1981, 1, kw["calendar"])
        for var in ("var_a", "var_b"):
            assert res[var].dims == ("time", "lat", "lon") and res[var].shape == (12, 5, 5)
            _close(res[var].values.sum(), case[var], f"annual_cycle {func} {kw['calendar']} Dataset {var}")
            one = util.annual_cycle(util.monthly_average(dset[var]), func=func)
            assert isinstance(one, DataArray) and len(one["time"]) == 12
            _close(one.values.sum(), case[var], f"annual_cycle {func} {kw['calendar']} DataArray {var}")


# ---- (b) float64: bit-equal to numpy ----------------------------------------------------------
@pytest.mark.parametrize("func", STATS)
@pytest.mark.parametrize("where", ["device", "host"])
def test_annual_cycle_float64_bits(func, where):
    time = _monthly_axis(9, "standard")
    for shape in ((108, 6, 8), (108, 7, 9), (108, 5)):  # n = 48 (packs), 63 and 5 (odd: one cell a lane)
        dims = ("time", "lat", "lon")[: len(shape)]
        da = DataArray(_field(shape, seed=shape[-1]), dims, {"time": time}, {"units": "m"}, "eta")
        da.encoding = {"dtype": "float32"}
        arg = _on_device(da) if where == "device" else da
        res = util.annual_cycle(arg, func=func)
        assert res.is_device == (where == "device") and res.dims == dims and res.name == "eta"
        assert res.attrs == {"units": "m"} and res.encoding == {"dtype": "float32"}
        want = cn.annual_cycle(da.values, time.values, func)
        assert np.isnan(want).any() and not np.isnan(want).all()  # land stays land, the rest is data
        _bits(res.values, want, f"annual_cycle {func} {where} {shape}")


@pytest.mark.parametrize("where", ["device", "host"])
def test_monthly_average_float64_bits(where):
    days = cftime_lite.daily_midpoints(1980, 2, "standard")  # groups of 31, 29, 31, 30 ... 28 ... steps
    time = _axis(days)
    for shape in ((731, 4, 6), (731, 3, 5)):
        da = DataArray(_field(shape, seed=11), ("time", "lat", "lon"), {"time": time}, None, "zos")
        res = util.monthly_average(_on_device(da) if where == "device" else da)
        assert res.shape == (24,) + shape[1:] and res.is_device == (where == "device")
        _bits(res.values, cn.monthly_average(da.values, days), f"monthly_average {where} {shape}")


def test_single_step_groups_and_time_not_leading():
    # one year of monthly data: every group of annual_cycle holds ONE step; std is 0 where valid
    time = _monthly_axis(1)
    y = _field((12, 6, 7), seed=5)
    for func in STATS:
        da = DataArray(np.ascontiguousarray(np.moveaxis(y, 0, 2)), ("lat", "lon", "time"),
                       {"time": time}, None, "v")
        for arg in (da, _on_device(da)):
            res = util.annual_cycle(arg, func=func)
            assert res.dims == ("time", "lat", "lon")  # time leads the result
            want = cn.annual_cycle(y, time.values, func)
            if func != "std":
                assert_bit_equal(want, y, "a one-step group is the step itself")
            _bits(res.values, want, f"one-step groups, time last, {func}")
    # time in the middle, several steps per group
    time = _monthly_axis(4)
    y = _field((48, 5, 6), seed=6)
    da = _on_device(DataArray(np.ascontiguousarray(np.moveaxis(y, 0, 1)), ("lat", "time", "lon"),
                              {"time": time}, None, "v"))
    for func in STATS:
        res = util.annual_cycle(da, func=func)
        assert res.dims == ("time", "lat", "lon") and res.is_device
        _bits(res.values, cn.annual_cycle(y, time.values, func), f"time in the middle, {func}")


def test_block_size_never_changes_a_bit(monkeypatch):
    time = _monthly_axis(6)
    y = _field((72, 9, 11), seed=8)
    da = DataArray(y, ("time", "lat", "lon"), {"time": time}, None, "v")
    for func in STATS:
        monkeypatch.setattr(record, "BLOCK_CELLS", None)
        whole = util.annual_cycle(da, func=func).values
        _bits(whole, cn.annual_cycle(y, time.values, func), f"one block, {func}")
        for block in (1, 7, 32):  # 99 cells: blocks of odd and even width, a ragged last block
            monkeypatch.setattr(record, "BLOCK_CELLS", block)
            _bits(util.annual_cycle(da, func=func).values, whole, f"blocks of {block} cells, {func}")


def test_more_groups_than_a_grid_dimension_holds():
    nt, n = 70001, 6  # one group per step: more than 65535 groups
    rng = np.random.default_rng(3)
    y = rng.normal(0.0, 1.0, (nt, n))
    y[rng.random((nt, n)) < 0.1] = np.nan
    steps, offsets = np.arange(nt), np.arange(nt + 1)
    yd = torch.from_numpy(y).cuda()
    for stat in ("mean", "min", "max"):
        _bits(core.time_group_stat(yd, steps, offsets, stat).cpu().numpy(), y, f"{nt} one-step groups, {stat}")
    got = core.time_group_stat(yd, steps, offsets, "std").cpu().numpy()
    _bits(got, np.where(np.isnan(y), np.nan, 0.0), f"{nt} one-step groups, std")
    # groups of 7 steps listed in DESCENDING time order (visited as listed), an empty group, and a
    # group that repeats a step
    steps = np.concatenate([np.arange(nt)[::-1], [5, 5, 7]])
    offsets = np.concatenate([np.arange(0, nt + 1, 7), [nt, nt, nt + 3]])  # ... an empty group, then [5, 5, 7]
    for stat in STATS:
        got = core.time_group_stat(yd, steps, offsets, stat).cpu().numpy()
        assert np.isnan(got[-2]).all()  # the empty group
        _bits(got, cn.grouped(y, steps, offsets, stat), f"reversed, repeated and empty groups, {stat}")


# ---- (c) float32 ------------------------------------------------------------------------------
@pytest.mark.parametrize("func", STATS)
def test_float32_is_the_float64_result_rounded_once(func):
    time = _monthly_axis(7, "julian")
    for shape in ((84, 6, 8), (84, 5, 6), (84, 7, 9)):  # n = 48 (4 a lane), 30 (2 a lane), 63 (1)
        y = _field(shape, seed=shape[1], dtype=np.float32)
        da = DataArray(y, ("time", "lat", "lon"), {"time": time}, None, "t")
        want = cn.annual_cycle(y, time.values, func).astype(np.float32)
        for arg, where in ((da, "host"), (_on_device(da), "device")):
            res = util.annual_cycle(arg, func=func)
            assert res.dtype == np.float32 and res.is_device == (where == "device")
            _bits(res.values, want, f"float32 {func} {where} {shape}")


def test_integers_and_booleans_compute_as_float64():
    time = _monthly_axis(3)
    rng = np.random.default_rng(2)
    for y in (rng.integers(-50, 50, (36, 4, 5)).astype(np.int32), rng.random((36, 4, 5)) < 0.5):
        da = DataArray(y, ("time", "lat", "lon"), {"time": time}, None, "k")
        for func in STATS:
            for arg in (da, _on_device(da)):
                res = util.annual_cycle(arg, func=func)
                assert res.dtype == np.float64
                _bits(res.values, cn.annual_cycle(y, time.values, func), f"{y.dtype} {func}")


# ---- (d) the labelled Dataset path ---------------------------------------------------------------
def test_dataset_with_a_string_variable_and_a_timeless_variable():
    dset = test_data.generate_test_data_time(nyears=3, start_year=1990, calendar="standard")
    dset["var_a"].encoding["dtype"] = "float32"
    dset["label"] = DataArray(np.array(["x"] * 36, dtype=object), ("time",))
    dset["names"] = DataArray(np.array(["ab"] * 36), ("time",))
    dset["static"] = DataArray(np.arange(25.0).reshape(5, 5), ("lat", "lon"))
    dset["f32"] = DataArray(dset["var_b"].values.astype(np.float32), ("time", "lat", "lon"))
    dset["lonfirst"] = DataArray(np.ascontiguousarray(dset["var_b"].values.transpose(2, 0, 1)),
                                 ("lon", "time", "lat"))
    dset.attrs = {"title": "t"}
    for func in STATS:
        res = util.annual_cycle(dset, func=func, time_axis_year=2000)
        assert sorted(res.keys()) == ["f32", "lonfirst", "var_a", "var_b"]  # strings, static: left out
        assert sorted(res.coords) == ["lat", "lon", "time"]
        assert list(res["time"].values) == cftime_lite.monthly_midpoints(2000, 1, "standard")
        assert res["var_a"].attrs == dset["var_a"].attrs and res["var_a"].encoding == {"dtype": "float32"}
        assert res["f32"].dtype == np.float32 and res["lonfirst"].dims == ("time", "lon", "lat")
        _bits(res["var_a"].values, cn.annual_cycle(dset["var_a"].values, dset["time"].values, func),
              f"Dataset var_a {func}")
        _bits(res["lonfirst"].values, res["var_b"].values.transpose(0, 2, 1), f"Dataset lonfirst {func}")
    assert "title" in dset.attrs and dset["var_a"].dims == ("time", "lat", "lon")  # the input is left alone


# ---- (e) one realistic size ------------------------------------------------------------------
def test_realistic_size_on_the_device():
    nt, ny, nx = 1200, 270, 360
    gen = torch.Generator(device="cuda").manual_seed(17)
    y = torch.randn((nt, ny, nx), generator=gen, device="cuda", dtype=torch.float32) * 0.3 + 1.0
    y[:, torch.rand((ny, nx), generator=gen, device="cuda") < 0.3] = float("nan")       # land
    y[torch.rand((nt, ny, nx), generator=gen, device="cuda") < 0.01] = float("nan")     # gaps
    time = _monthly_axis(100, "noleap", start=1900)
    da = DataArray(y, ("time", "yh", "xh"), {"time": time}, None, "steric")
    sub = y[:, ::7, ::11].cpu().numpy()
    for func in ("mean", "std"):
        res = util.annual_cycle(da, func=func)
        assert res.is_device and res.shape == (12, ny, nx) and res.dtype == np.float32
        want = cn.annual_cycle(sub, time.values, func).astype(np.float32)
        _bits(res.data[:, ::7, ::11].cpu().numpy(), want, f"(1200, 270, 360) float32 {func}, strided subset")
    plan = climatology.annual_cycle_plan(time)
    assert plan.sizes == [100] * 12 and list(res["time"].values) == cftime_lite.monthly_midpoints(1950, 1, "noleap")
