"""GPU: momlevel_amd.extremes at its public level -- time_quantile, time_median and
exceedance_count on DataArrays and Datasets, host and device records, whole record and by calendar
month / year -- against tests/quantile_numpy.py over the plans' members.  A three-year daily record
on a 6 x 5 plane serves every test."""

import numpy as np
import pytest
import torch

import quantile_numpy as qn
from momlevel_amd import climatology, extremes, record
from momlevel_amd.cftime_lite import daily_midpoints
from momlevel_amd.labeled import DataArray, Dataset

pytestmark = pytest.mark.gpu

DEV = "cuda"
NY, NX = 6, 5
AXIS = np.array(daily_midpoints(2001, 3, "noleap"), dtype=object)
NT = AXIS.size
_cache = {}


def _values(dtype):
    if dtype not in _cache:
        rng = np.random.default_rng(31)
        y = rng.normal(0.0, 0.1, (NT, NY, NX)) + 0.1 * np.sin(np.arange(NT) / 58.0)[:, None, None]
        y[rng.random(y.shape) < 0.05] = np.nan
        y[:, 0, 0] = np.nan  # a land cell
        _cache[dtype] = y.astype(dtype)
    return _cache[dtype]


def _record(dtype=np.float64, device=False, dims=("time", "yh", "xh")):
    y = _values(dtype)
    coords = {"time": DataArray(AXIS, ("time",), None, None, "time"),
              "yh": DataArray(np.arange(NY) * 1.0, ("yh",), None, None, "yh"),
              "xh": DataArray(np.arange(NX) * 1.0, ("xh",), None, None, "xh")}
    da = DataArray(torch.from_numpy(y).to(DEV) if device else y, ("time", "yh", "xh"), coords,
                   {"units": "m"}, "zos")
    da.encoding = {"dtype": "float32"}
    return da if dims == da.dims else da.transpose(*dims)


def _host(da):
    return da.data.cpu().numpy() if da.is_device else np.asarray(da.values)


def _want(dtype, q, plan=None):
    y = _values(dtype).reshape(NT, -1)
    res = qn.time_quantile(y, q, *((None, None) if plan is None else (plan.steps, plan.offsets)))
    res = qn.rounded_once(res) if dtype == np.float32 else res
    return res.reshape(res.shape[:2] + (NY, NX))


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("float64", "float32"))
def test_host_and_device_records_agree_bit_for_bit(dtype, monkeypatch):
    q = [0.05, 0.5, 0.95]
    dev = extremes.time_quantile(_record(dtype, device=True), q)
    assert dev.is_device and dev.data.is_cuda and dev.dims == ("quantile", "yh", "xh")
    monkeypatch.setattr(record, "BLOCK_CELLS", 7)  # the host record goes up in five blocks of cells
    host = extremes.time_quantile(_record(dtype), q)
    assert not host.is_device and host.dtype == dtype and host.shape == (3, NY, NX)
    assert _host(dev).tobytes() == host.values.tobytes()
    qn.assert_values(host.values, _want(dtype, q)[:, 0], "whole record")
    assert np.isnan(host.values[:, 0, 0]).all() and not np.isnan(host.values[:, 1:]).any()
    cnt_dev = extremes.exceedance_count(_record(dtype, device=True), dev[1])
    cnt_host = extremes.exceedance_count(_record(dtype), DataArray(host.values[1], ("yh", "xh")))
    assert cnt_dev.is_device and cnt_dev.data.dtype == torch.int64 and cnt_host.dtype == np.int64
    assert np.array_equal(_host(cnt_dev), cnt_host.values)
    y = _values(dtype).reshape(NT, -1)
    assert np.array_equal(cnt_host.values.reshape(1, -1),
                          qn.exceed_count(y, host.values[1].reshape(1, -1)))


def test_blocked_host_exceedance_slices_a_per_cell_threshold(monkeypatch):
    """A host float32 record (yh 5, time 24, xh 7) goes up in five blocks of 7 cells against a
    threshold that differs in every cell, with a NaN cell: every block must meet its own slice of
    the threshold.  Exactly the single-call device result and the numpy restatement (int64)."""
    rng = np.random.default_rng(33)
    y = rng.normal(0.0, 1.0, (5, 24, 7)).astype(np.float32)
    y[2, :, 3] = np.nan
    thr = rng.normal(0.0, 0.5, (5, 7))
    flat = np.moveaxis(y, 1, 0).reshape(24, 35)
    want = qn.exceed_count(flat, thr.reshape(1, 35)).reshape(5, 7)
    # (the check has teeth: the first block's thresholds for every block give other counts)
    assert not np.array_equal(want, qn.exceed_count(flat, np.tile(thr[0], 5)[None]).reshape(5, 7))
    monkeypatch.setattr(record, "BLOCK_CELLS", 7)
    dev = extremes.exceedance_count(
        DataArray(torch.from_numpy(y).to(DEV), ("yh", "time", "xh"), None, None, "zos"),
        DataArray(thr, ("yh", "xh")))
    host = extremes.exceedance_count(DataArray(y, ("yh", "time", "xh"), None, None, "zos"),
                                     DataArray(thr, ("yh", "xh")))
    assert dev.is_device and dev.data.dtype == torch.int64 and dev.dims == ("yh", "xh")
    assert not host.is_device and host.dtype == np.int64 and host.dims == ("yh", "xh")
    assert np.array_equal(host.values, want) and np.array_equal(_host(dev), want)
    assert want[2, 3] == 0


def test_scalar_against_sequence_layout_and_the_median():
    da = _record()
    seq = extremes.time_quantile(da, [0.5])
    one = extremes.time_quantile(da, 0.5)
    assert seq.dims == ("quantile", "yh", "xh") and one.dims == ("yh", "xh")
    assert seq.coords["quantile"].dims == ("quantile",) and one.coords["quantile"].dims == ()
    assert seq.coords["quantile"].values.tolist() == [0.5]
    assert float(one.coords["quantile"].values) == 0.5
    assert "time" not in one.coords and one.attrs == {"units": "m"} and one.name == "zos"
    assert one.encoding == {"dtype": "float32"}
    assert seq.values[0].tobytes() == one.values.tobytes()
    med = extremes.time_median(da)
    assert med.dims == ("yh", "xh") and med.values.tobytes() == one.values.tobytes()
    qn.assert_values(med.values, _want(np.float64, 0.5)[0, 0], "median")
    with np.errstate(invalid="ignore"):
        ref = np.nanmedian(_values(np.float64)[:, 1:], axis=0)
    qn.assert_values(med.values[1:], ref, "numpy.nanmedian")


def test_tcoord_not_leading():
    da = _record(np.float32, device=True, dims=("yh", "time", "xh"))
    res = extremes.time_quantile(da, [0.25, 0.75], by="year")
    assert res.dims == ("quantile", "yh", "time", "xh") and res.shape == (2, NY, 3, NX)
    assert res.is_device
    plan = climatology.yearly_plan(da["time"], "time")
    qn.assert_values(np.moveaxis(_host(res), 2, 1), _want(np.float32, [0.25, 0.75], plan), "by year")
    flat = extremes.time_quantile(da, 0.75)
    assert flat.dims == ("yh", "xh")
    qn.assert_values(_host(flat), _want(np.float32, 0.75)[0, 0], "whole record")


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("float64", "float32"))
def test_by_month_and_by_year(dtype):
    da = _record(dtype)
    month = climatology.annual_cycle_plan(da["time"], "time")
    year = climatology.yearly_plan(da["time"], "time")
    assert sorted(month.sizes) == [84] + [90] * 4 + [93] * 7 and year.sizes == [365] * 3
    q = [0.5, 0.99]
    by_month = extremes.time_quantile(da, q, by="month")
    assert by_month.dims == ("quantile", "time", "yh", "xh") and by_month.shape == (2, 12, NY, NX)
    assert [t.month for t in by_month.coords["time"].values] == list(range(1, 13))
    assert {t.year for t in by_month.coords["time"].values} == {2002}
    qn.assert_values(by_month.values, _want(dtype, q, month), "by month")
    by_year = extremes.time_quantile(da, q, by="year")
    assert by_year.shape == (2, 3, NY, NX)
    assert [t.year for t in by_year.coords["time"].values] == [2001, 2002, 2003]
    qn.assert_values(by_year.values, _want(dtype, q, year), "by year")
    med = extremes.time_median(da, by="month", time_axis_year=1990)
    assert {t.year for t in med.coords["time"].values} == {1990}
    assert med.values.tobytes() == by_month.values[0].tobytes()


def test_dataset_with_a_non_numeric_variable_and_one_without_tcoord():
    da = _record(device=True)
    ds = Dataset({"zos": da, "label": DataArray(np.array(["a"] * NT), ("time",)),
                  "depth": DataArray(np.ones((NY, NX)), ("yh", "xh")),
                  "days": DataArray(np.arange(NT * NX).reshape(NT, NX), ("time", "xh"))})
    res = extremes.time_quantile(ds, [0.1, 0.9])
    assert sorted(res.data_vars) == ["days", "zos"] and "time" not in res.coords
    assert res["zos"].is_device and res["zos"].dims == ("quantile", "yh", "xh")
    assert res["quantile"].values.tolist() == [0.1, 0.9]
    qn.assert_values(_host(res["zos"]), _want(np.float64, [0.1, 0.9])[:, 0], "dataset, zos")
    days = np.arange(NT * NX).reshape(NT, NX)
    assert res["days"].dtype == np.float64  # integers are computed and returned as float64
    qn.assert_values(np.asarray(res["days"].values), np.quantile(days, [0.1, 0.9], axis=0), "days")


def test_exceedance_count_of_the_monthly_quantiles():
    da = _record(device=True)
    p90 = extremes.time_quantile(da, 0.9, by="month")
    assert p90.is_device and p90.dims == ("time", "yh", "xh")
    cnt = extremes.exceedance_count(da, p90, by="month")
    assert cnt.is_device and cnt.data.dtype == torch.int64 and cnt.dims == ("time", "yh", "xh")
    assert cnt.name == "zos" and [t.month for t in cnt.coords["time"].values] == list(range(1, 13))
    plan = climatology.annual_cycle_plan(da["time"], "time")
    y = _values(np.float64).reshape(NT, -1)
    thr = qn.time_quantile(y, 0.9, plan.steps, plan.offsets)[0]
    want = qn.exceed_count(y, thr, plan.steps, plan.offsets).reshape(12, NY, NX)
    got = _host(cnt)
    assert np.array_equal(got, want)
    # no ties in this record: c - ceil(0.9 (c - 1)) - [0.9 (c - 1) is whole] steps lie above
    c = np.stack([np.sum(~np.isnan(y[sel]), axis=0) for sel in
                  (plan.steps[plan.offsets[g]:plan.offsets[g + 1]] for g in range(12))])
    vi = (c - 1) * 0.9
    formula = np.where(c > 0, c - np.ceil(vi) - (vi == np.floor(vi)), 0).astype(np.int64)
    assert np.array_equal(want.reshape(12, -1), formula) and not got[:, 0, 0].any()
    # a number and a per-cell field
    whole = extremes.exceedance_count(da, 0.1)
    assert whole.dims == ("yh", "xh")
    assert np.array_equal(_host(whole).reshape(1, -1), qn.exceed_count(y, np.full((1, NY * NX), 0.1)))
    per_year = extremes.exceedance_count(da, extremes.time_median(da), by="year")
    med = qn.time_quantile(y, 0.5)[0]
    yp = climatology.yearly_plan(da["time"], "time")
    assert np.array_equal(_host(per_year).reshape(3, -1),
                          qn.exceed_count(y, np.broadcast_to(med, (3, NY * NX)), yp.steps, yp.offsets))
