"""GPU: the public functions of momlevel_amd.filters on labelled data -- rolling_mean / rolling_sum,
time_filter, lowpass and rolling_trend -- against the numpy restatement tests/filter_numpy.py (bit
for bit) and, for the running slopes, against numpy.polyfit per window (1e-10 of max|slope|, the
project's gate for sums).  Host and device inputs must give identical bits."""

import numpy as np
import pytest
import torch

import filter_numpy as fn
from conftest import assert_bit_equal
from momlevel_amd import cftime_lite, filters, record, trend
from momlevel_amd.labeled import DataArray, Dataset

pytestmark = pytest.mark.gpu


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


def _np(da):
    return da.data.cpu().numpy() if da.is_device else np.asarray(da.values)


def _field(shape, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    y = rng.normal(0.2, 0.05, shape)
    y[rng.random(shape) < 0.04] = np.nan
    y[:, 0, 0] = np.nan  # land
    return y.astype(dtype)


# ---- rolling_mean / rolling_sum ---------------------------------------------------------------------
@pytest.mark.parametrize("window", (12, 13))
def test_rolling_mean_time_axis_not_leading(window):
    time = _monthly_axis(3)
    y = _field((36, 5, 6), seed=window)  # time leading here ...
    da = DataArray(np.ascontiguousarray(np.moveaxis(y, 0, 1)), ("lat", "time", "lon"),
                   {"time": time}, {"units": "m"}, "eta")  # ... and in the middle there
    da.encoding = {"_FillValue": 1e20}
    for center in (True, False):
        for mp in (None, 1, 7):
            host = filters.rolling_mean(da, window, center=center, min_periods=mp)
            dev = filters.rolling_mean(_on_device(da), window, center=center, min_periods=mp)
            assert host.dims == dev.dims == da.dims and host.name == dev.name == "eta"
            assert host.attrs == {"units": "m"} and host.encoding == {"_FillValue": 1e20}
            assert dev.is_device and not host.is_device
            assert host.coords["time"].values.tolist() == time.values.tolist()
            want = np.moveaxis(fn.rolling_mean_nanmean(y, window, center, mp), 0, 1)
            what = f"rolling_mean W={window} centre={center} min_periods={mp}"
            assert_bit_equal(_np(host), want, what + " (host)")
            assert_bit_equal(_np(dev), _np(host), what + " (device against host)")
            assert _np(host).dtype == np.float64
    # the default is "complete windows only": a half-window of NaN at each end
    full = _np(filters.rolling_mean(da, window))
    lead = window // 2
    assert np.isnan(full[:, :lead]).all() and np.isnan(full[:, 36 - (window - 1 - lead):]).all()
    s = filters.rolling_sum(da, window, min_periods=1)
    assert_bit_equal(_np(s), np.moveaxis(fn.time_filter(y, np.ones(window), lead, 1), 0, 1),
                     "rolling_sum")


def test_rolling_mean_dataset_and_dtypes():
    time = _monthly_axis(3)
    y = _field((36, 5, 6), seed=1)
    dset = Dataset()
    dset["eta"] = DataArray(y, ("time", "lat", "lon"), {"time": time}, {"units": "m"})
    dset["f32"] = DataArray(y.astype(np.float32), ("time", "lat", "lon"))
    dset["count"] = DataArray(np.arange(36 * 4, dtype=np.int32).reshape(36, 4), ("time", "k"))
    dset["names"] = DataArray(np.array(["ab"] * 36), ("time",))
    dset["label"] = DataArray(np.array(["x"] * 36, dtype=object), ("time",))
    dset["static"] = DataArray(np.arange(30.0).reshape(5, 6), ("lat", "lon"))
    out = filters.rolling_mean(dset, 12, min_periods=6)
    assert sorted(out.data_vars.keys()) == ["count", "eta", "f32"]
    assert "time" in out.coords and out["eta"].attrs == {"units": "m"}
    want = fn.rolling_mean_nanmean(y, 12, True, 6)
    assert_bit_equal(_np(out["eta"]), want, "Dataset eta")
    f32 = _np(out["f32"])
    assert f32.dtype == np.float32  # the float64 mean of the float32 values, rounded once
    assert_bit_equal(f32, fn.rolling_mean_nanmean(y.astype(np.float32), 12, True, 6).astype(np.float32),
                     "Dataset f32")
    cnt = _np(out["count"])
    assert cnt.dtype == np.float64  # an integer record gives float64
    assert_bit_equal(cnt, fn.rolling_mean_nanmean(dset["count"].values, 12, True, 6), "Dataset count")
    dev32 = filters.rolling_mean(_on_device(dset["f32"]), 12, min_periods=6)
    assert dev32.data.dtype == torch.float32
    assert_bit_equal(_np(dev32), f32, "float32 on the device")
    ints = DataArray(torch.arange(36 * 4, dtype=torch.int64).reshape(36, 4).cuda(), ("time", "k"),
                     None, None, "count")
    devint = filters.rolling_mean(ints, 12, min_periods=6)
    assert devint.data.dtype == torch.float64
    assert_bit_equal(_np(devint), cnt, "integers on the device")


def test_host_record_walked_in_blocks(monkeypatch):
    y = _field((36, 5, 6), seed=2)
    da = DataArray(y, ("time", "lat", "lon"), {"time": _monthly_axis(3)}, None, "eta")
    whole = _np(filters.rolling_mean(da, 5, min_periods=2))
    monkeypatch.setattr(record, "BLOCK_CELLS", 7)
    assert_bit_equal(_np(filters.rolling_mean(da, 5, min_periods=2)), whole, "blocks of 7 cells")


# ---- lowpass / time_filter ---------------------------------------------------------------------------
def test_lowpass_of_two_sinusoids():
    nt, cutoff = 240, 24
    t = np.arange(nt, dtype=np.float64)
    y = (np.sin(2 * np.pi * t / 6.0)[:, None] + np.sin(2 * np.pi * t / 60.0)[:, None]
         * np.array([1.0, 0.5, 2.0])[None, :])
    da = DataArray(y, ("time", "x"), None, None, "eta")
    window = 73  # the default: the smallest odd number >= 3 * cutoff
    w = filters.lanczos_weights(window, cutoff)
    m = (window - 1) // 2
    for da_ in (da, _on_device(da)):
        nan_edges = filters.lowpass(da_, cutoff)
        got = _np(nan_edges)
        assert_bit_equal(got, fn.time_filter(y, w, m), "lowpass, edges='nan'")
        assert np.isnan(got[:m]).all() and np.isnan(got[nt - m:]).all()
        assert not np.isnan(got[m:nt - m]).any()
        assert_bit_equal(_np(filters.lowpass(da_, cutoff, window=window)), got, "the default window")
        renorm = _np(filters.lowpass(da_, cutoff, edges="renormalise"))
        assert_bit_equal(renorm, fn.time_filter(y, w, m, m + 1, normalise=True),
                         "lowpass, edges='renormalise'")
        assert np.isfinite(renorm).all()
        assert nan_edges.dims == da.dims and nan_edges.name == "eta"
    # time_filter with the same weights is the same thing; a lead that is not the centre shifts it
    assert_bit_equal(_np(filters.time_filter(da, w)), got, "time_filter against lowpass")
    shifted = _np(filters.time_filter(da, w[:5], lead=1, skipna=True, min_periods=3))
    assert_bit_equal(shifted, fn.time_filter(y, w[:5], 1, 3, normalise=True), "lead=1, skipna")
    trailing = _np(filters.time_filter(da, [0.25, 0.25, 0.5], center=False))
    assert_bit_equal(trailing, fn.time_filter(y, [0.25, 0.25, 0.5], 2), "trailing")


# ---- rolling_trend ------------------------------------------------------------------------------------
def test_rolling_trend_on_a_monthly_axis():
    window, nyears = 24, 10
    time = _monthly_axis(nyears)
    nt = 12 * nyears
    x = cftime_lite.axis_to_numeric(time.values)
    assert len(set(np.diff(x).tolist())) > 1  # months of unequal length
    y = _field((nt, 3, 4), seed=9)  # scattered NaN steps, a land cell
    y[:, 1, 1] = np.random.default_rng(9).normal(0.2, 0.05, nt)
    y[17, 1, 1] = np.nan  # every window that holds this step, and no other, is NaN in this cell
    y[:, 0, 0] = np.nan
    b = 3.0e-3  # per year
    factor = 1.0 / trend.time_conversion_factor("ns", "yr")
    y[:, 2, 3] = 1.5 + b / factor * (x - x[0])  # a line sampled exactly
    da = DataArray(y, ("time", "yh", "xh"), {"time": time}, {"units": "m"}, "eta")
    lead = filters.window_lead(window, True)
    table = filters.trend_table(x, window, lead)
    want = fn.time_filter(y, table, lead) * factor
    poly = fn.polyfit_slopes(x, y, window, lead) * factor
    for da_ in (da, _on_device(da)):
        out = filters.rolling_trend(da_, window, time_units="yr")
        got = _np(out)
        assert out.name == "eta_slope" and out.dims == da.dims and got.dtype == np.float64
        assert_bit_equal(got, want, "rolling_trend against the restatement")
        assert np.array_equal(np.isnan(got), np.isnan(poly))
        ok = ~np.isnan(poly)
        scale = np.max(np.abs(poly[ok]))
        err = np.max(np.abs(got[ok] - poly[ok])) / scale
        print(f"rolling_trend W={window}: max |slope - polyfit| / max|slope| = {err:.2e}")
        assert err <= 1e-10
        complete = ~np.isnan(got[:, 2, 3])
        assert complete.sum() == nt - window + 1
        assert np.max(np.abs(got[complete, 2, 3] - b)) <= 1e-10 * scale
        assert np.isnan(got[:, 0, 0]).all()
        holds = (np.arange(nt) - lead <= 17) & (17 <= np.arange(nt) - lead + window - 1)
        assert np.isnan(got[holds, 1, 1]).all() and not np.isnan(got[~holds & complete, 1, 1]).any()
        assert out.attrs["units"] == trend.calc_linear_trend(da_, time_units="yr")["eta_slope"].attrs["units"]
    f32 = filters.rolling_trend(DataArray(y.astype(np.float32), da.dims, {"time": time}, None, "eta"),
                                window, time_units="yr", center=False)
    assert _np(f32).dtype == np.float64 and "units" in f32.attrs
    assert f32.attrs["units"] == trend.calc_linear_trend(
        DataArray(y.astype(np.float32), da.dims, {"time": time}, None, "eta"),
        time_units="yr")["eta_slope"].attrs["units"]
    # a numeric axis: slope per unit of the coordinate, no units attribute made
    plain = filters.rolling_trend(DataArray(y[:, 2, :], ("time", "xh"), None, None, "eta"), 5)
    assert "units" not in plain.attrs and plain.name == "eta_slope"
