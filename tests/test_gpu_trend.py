"""GPU: the trend module (momlevel_amd.trend; csrc/momlevel_trend.hip) against the reference's own
goldens and against the numpy restatement tests/trend_numpy.py.

Gates (none taken from what the kernels give):
  * the reference's goldens (tests/golden/trend_goldens.json), rtol 1e-9: they are printed to that
    many digits and were reproduced to all of them with numpy alone;
  * parity with numpy.polyfit per column: NaN placement identical; the fitted line at every step
    within 1e-10 * max|y|; the intercept within 1e-10 * max|y| * (1 + |mean(x)| / span(x)) (it is
    the line extrapolated from the centre of the axis to x = 0); the slope within 1e-10 relative.
    1e-10 is the project's parity gate for sums; numpy's own lstsq sits at 1e-15 ..
    2e-13 on these measures.  The test fields carry a trend of at least half the noise's standard
    deviation over the record, so that "relative" is asked of a slope the data determine;
  * the pointwise passes are bit-identical to the numpy expression evaluated from the slope and
    intercept the GPU itself returned.
Every figure is printed before it is asserted.
"""

import json
import os
import warnings

import numpy as np
import pytest
import torch

import trend_numpy as tn
from conftest import assert_bit_equal
from momlevel_amd import cftime_lite, record, steric, test_data, trend, util
from momlevel_amd.labeled import DataArray, Dataset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 1e-10


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "trend_goldens.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def dset8(gold):
    return test_data.generate_test_data_time(**gold["dataset"])


def _close(got, want, what):
    got = float(got)
    print(f"{what}: got {got!r} golden {want!r} rel {abs(got - want) / abs(want):.2e}")
    assert abs(got - want) <= 1e-9 * abs(want), what


def _on_device(da):
    return DataArray(torch.from_numpy(np.ascontiguousarray(da.values)).cuda(), da.dims, da.coords,
                     da.attrs, da.name)


# ---- (a) the reference's goldens through the public functions -------------------------------
def test_goldens_calc_linear_trend(dset8, gold):
    res = trend.calc_linear_trend(dset8["var_a"])
    assert sorted(res.keys()) == ["var_a_intercept", "var_a_slope"]
    assert res["var_a_slope"].dims == ("lat", "lon") and res["var_a_slope"].dtype == np.float64
    _close(res["var_a_intercept"].values.sum(), gold["intercept_sum"], "intercept sum")
    assert res["var_a_slope"].attrs["units"] == gold["units_default"]
    assert res["var_a_slope"].attrs["comment"] == "Slope of linear trend"
    assert res["var_a_intercept"].attrs["comment"] == "Y-intercept of linear trend"
    assert res["var_a_slope"].attrs["first_attribute"] == "foo"
    assert "units" not in res["var_a_intercept"].attrs and "comment" not in dset8["var_a"].attrs
    yr = trend.calc_linear_trend(dset8["var_a"], time_units="yr")
    _close(yr["var_a_slope"].values.sum(), gold["slope_sum_per_year"], "slope sum per year")
    _close(yr["var_a_intercept"].values.sum(), gold["intercept_sum"], "intercept sum (yr)")
    assert yr["var_a_slope"].attrs["units"] == gold["units_yr"]
    with_units = DataArray(dset8["var_a"].data, dset8["var_a"].dims, dset8["var_a"].coords,
                           {"units": "m"}, "eta")
    assert trend.calc_linear_trend(with_units, time_units="yr")["eta_slope"].attrs["units"] == "m  yr-1"


def test_goldens_broadcast_trend(dset8, gold):
    for units in (None, "yr"):
        slope = trend.calc_linear_trend(dset8["var_a"], time_units=units)["var_a_slope"]
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # the units attribute names the time unit: no warning
            line = trend.broadcast_trend(slope, dset8["time"])
        assert line.dims == ("lat", "lon", "time") and line.shape == (5, 5, 1825)
        _close(line.values.sum(), gold["broadcast_trend_sum"], f"broadcast_trend sum ({units})")
    anom = trend.broadcast_trend(slope, dset8["time"], subtract_time_zero=True)
    full = line.values
    assert_bit_equal(anom.values, full - full[..., :1], "subtract_time_zero")


def test_goldens_linear_detrend(dset8, gold):
    res = trend.linear_detrend(dset8["var_a"], mode="correct")
    assert res.dims == ("time", "lat", "lon") and res.name == "var_a"
    assert res.attrs["first_attribute"] == "foo" and "mode=correct" in res.attrs["detrend_comment"]
    _close(res.values.sum(), gold["correct_sum_var_a"], "correct sum, full field")
    cell = trend.linear_detrend(dset8["var_a"][:, 0, 0], mode="correct")
    assert cell.dims == ("time",)
    _close(cell.values.sum(), gold["correct_sum_var_a_cell00"], "correct sum, cell (0,0)")
    assert_bit_equal(cell.values, res.values[:, 0, 0], "a cell alone and in its field")
    # mode="remove": the residuals of a least-squares line sum to zero (the reference's golden for
    # it, 1e-9, is rounding noise under allclose's atol and is not asserted)
    rem = trend.linear_detrend(dset8["var_a"])
    print("remove: |sum| / sum|y| =", abs(rem.values.sum()) / np.abs(dset8["var_a"].values).sum())
    assert abs(rem.values.sum()) <= GATE * np.abs(dset8["var_a"].values).sum()


def test_goldens_dataset_path_and_the_util_shim(dset8, gold):
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # none of the questionable variables is in this dataset
        res = trend.linear_detrend(dset8, mode="correct")
    assert isinstance(res, Dataset) and sorted(res.keys()) == ["var_a", "var_b"]
    _close(res["var_a"].values.sum(), gold["correct_sum_var_a"], "Dataset var_a")
    _close(res["var_b"].values.sum(), gold["correct_sum_var_b"], "Dataset var_b")
    extra = dset8.copy()
    extra["average_DT"] = DataArray(np.ones(1825), ("time",))
    extra["static"] = DataArray(np.arange(25.0).reshape(5, 5), ("lat", "lon"))
    with pytest.warns(UserWarning, match="Incompatible variable detected"):
        res2 = trend.linear_detrend(extra[["var_a", "average_DT", "static"]], mode="correct")
    assert np.array_equal(res2["static"].values, extra["static"].values)  # no time: passes through
    assert_bit_equal(res2["var_a"].values, res["var_a"].values, "var_a in either dataset")
    with pytest.warns(DeprecationWarning):
        shim = util.linear_detrend(dset8["var_a"][:, 0, 0], mode="correct")
    _close(shim.values.sum(), gold["correct_sum_var_a_cell00"], "util.linear_detrend")


# ---- (b) parity against numpy.polyfit per column ----------------------------------------------
def _axis(kind, nt):
    """(coordinate values, numeric x) of a monthly / daily / numeric axis of nt steps"""
    if kind == "monthly":
        times = np.empty(nt, dtype=object)
        times[:] = cftime_lite.monthly_midpoints(1960, nt // 12, "gregorian")
        return times, tn.ns_axis(times)
    if kind == "daily":
        times = np.empty(nt, dtype=object)
        times[:] = cftime_lite.daily_midpoints(1979, nt // 365, "noleap")
        return times, tn.ns_axis(times)
    # uneven steps from 0: an axis far from its origin (|mean| >> span) would make numpy's own
    # uncentred least squares, the yardstick here, lose digits with the square of that ratio
    x = np.cumsum(np.random.default_rng(nt).uniform(0.05, 0.45, nt))
    return x, x


def _field(nt, shape, dtype, seed):
    """noise (sd 20) about 100 plus a per-cell trend of +-(0.5 .. 1.5) * 20 over the record; a land
    mask (all-NaN cells); cells with 30 % scattered NaN steps, each keeping >= 3 valid steps"""
    r = np.random.default_rng(seed)
    n = int(np.prod(shape))
    rate = r.uniform(0.5, 1.5, n) * r.choice([-1.0, 1.0], n) * 20.0
    y = r.normal(100.0, 20.0, (nt, n)) + rate * np.linspace(-0.5, 0.5, nt)[:, None]
    land = r.random(n) < 0.2
    land[0], land[-1] = True, False  # at least one cell of each kind, whatever the draw
    y[:, land] = np.nan
    drop = int(0.3 * nt)
    if nt - drop >= 3 and drop > 0:
        for j in np.nonzero(~land & (r.random(n) < 0.4))[0]:
            y[r.choice(nt, drop, replace=False), j] = np.nan
    return y.reshape((nt,) + shape).astype(dtype)


PARITY = [(3, "numeric"), (24, "monthly"), (365, "daily"), (1825, "daily"), (4097, "numeric")]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(7, 9), (6, 7), (4, 8), (13,)])
@pytest.mark.parametrize("nt, kind", PARITY)
def test_fit_parity_with_numpy_polyfit(nt, kind, shape, dtype):
    coord, x = _axis(kind, nt)
    y = _field(nt, shape, dtype, seed=nt * 31 + len(shape) + shape[0])
    lead = ("time",) + tuple(f"d{i}" for i in range(len(shape)))
    axis = (nt + shape[0]) % (len(shape) + 1)              # where the fit dimension sits
    dims = lead[1:1 + axis] + ("time",) + lead[1 + axis:]
    data = np.ascontiguousarray(np.moveaxis(y, 0, axis))
    arr = DataArray(data, dims, {"time": DataArray(coord, ("time",))}, {"units": "m"}, "eta")
    want_m, want_b = tn.polyfit_columns(x, y)
    ymax = np.nanmax(np.abs(y.astype(np.float64)))
    span = x.max() - x.min()
    for place in ("host", "device"):
        a = arr if place == "host" else _on_device(arr)
        res = trend.calc_linear_trend(a, dim="time")
        assert res["eta_slope"].is_device == (place == "device")
        m, b = res["eta_slope"].values, res["eta_intercept"].values
        assert res["eta_slope"].dims == lead[1:] and m.dtype == np.float64
        assert np.array_equal(np.isnan(m), np.isnan(want_m)), "NaN placement of the slope"
        assert np.array_equal(np.isnan(b), np.isnan(want_b)), "NaN placement of the intercept"
        ok = ~np.isnan(want_m)
        assert ok.any() and (~ok).any()
        xs = x.reshape((nt,) + (1,) * len(shape))
        line = np.max(np.abs((m * xs + b) - (want_m * xs + want_b))[:, ok]) / ymax
        icpt = np.max(np.abs(b - want_b)[ok]) / (ymax * (1 + abs(x.mean()) / span))
        slope = np.max(np.abs(m - want_m)[ok] / np.abs(want_m[ok]))
        print(f"nt={nt} {kind} {shape} {np.dtype(dtype).name} {place}: line {line:.2e} "
              f"intercept {icpt:.2e} slope {slope:.2e}")
        assert line <= GATE and icpt <= GATE and slope <= GATE


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nt, kind, calendar", [(1825, "D", "noleap"), (1200, "MS", "gregorian")])
def test_seasonal_fits_match_pinv_and_dot(nt, kind, calendar, dtype):
    """sequential-t projection against BLAS dot: coefficients, model and residuals within 1e-10 of
    the data's scale (numpy against itself in another order: 3e-16)"""
    years = nt // (365 if kind == "D" else 12)
    d = test_data.generate_test_data_time(start_year=1979, nyears=years, calendar=calendar,
                                          frequency=kind)
    times = d["time"].values
    r = np.random.default_rng(nt)
    y = (r.normal(100, 20, (nt, 6, 7)) + 30 * np.sin(2 * np.pi * tn.decimal_year(times))[:, None, None]
         ).astype(dtype)
    arr = DataArray(np.ascontiguousarray(y.transpose(1, 0, 2)), ("lat", "time", "lon"),
                    {"time": d["time"]}, {"standard_name": "eta", "long_name": "Eta", "units": "m"},
                    "eta")
    scale = np.abs(y).max()
    coeff, model, resid = tn.seasonal_fit(tn.decimal_year(times), y)
    smodel, sresid = trend.seasonal_model(_on_device(arr), return_model=True)
    assert sresid.dims == ("lat", "time", "lon") and smodel.dims == ("lat", "lon", "time")
    assert sresid.is_device and sresid.dtype == np.float64
    e_m = np.abs(np.moveaxis(smodel.values, -1, 0) - model).max() / scale
    e_r = np.abs(np.moveaxis(sresid.values, 1, 0) - resid).max() / scale
    print(f"seasonal_model {kind} {np.dtype(dtype).name}: model {e_m:.2e} residuals {e_r:.2e}")
    assert e_m <= GATE and e_r <= GATE
    assert smodel.attrs == {"standard_name": "eta_smodel", "long_name": "Seasonal model, Eta",
                            "units": "m"}
    assert sresid.attrs == {"standard_name": "eta_sresid", "long_name": "Seasonal residuals, Eta",
                            "units": "m"}
    assert trend.seasonal_model(arr).dims == ("lat", "time", "lon")

    dec = trend.deseason_decimal_year(times)
    coeff, model, resid = tn.seasonal_fit(dec, y)
    for fmt, want in (("coeff", coeff), ("model", model), ("residuals", resid)):
        got = trend.deseason(arr, output_format=fmt)
        assert got.dims == (("coeff" if fmt == "coeff" else "time"), "lat", "lon")
        err = np.abs(got.values - want).max() / scale
        print(f"deseason {fmt} {kind} {np.dtype(dtype).name}: {err:.2e}")
        assert err <= GATE
        assert "standard_name" not in got.attrs and ("units" in got.attrs) == (fmt != "coeff")
    assert got.attrs["long_name"] == "Eta residuals from detrending and deseasonalizing"
    assert got.attrs["processing"] == "Residuals from detrending and deseasonalizing"
    assert arr.attrs["standard_name"] == "eta"  # the input's attrs are left alone


# ---- (c) the pointwise passes are numpy's, bit for bit ------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(7, 9), (6, 8)])
def test_pointwise_passes_are_bit_identical_to_numpy(shape, dtype):
    nt = 365
    coord, x = _axis("daily", nt)
    y = _field(nt, shape, dtype, seed=5)
    arr = DataArray(y, ("time", "a", "b"), {"time": DataArray(coord, ("time",))}, None, "eta")
    fit = trend.calc_linear_trend(arr)  # slope per ns: what linear_detrend uses itself
    m, b = fit["eta_slope"].values, fit["eta_intercept"].values
    xs = x[:, None, None]
    for a in (arr, _on_device(arr)):
        rem = trend.linear_detrend(a)
        cor = trend.linear_detrend(a, mode="correct")
        line = trend.broadcast_trend(fit["eta_slope"] if a is arr else _on_device(fit["eta_slope"]),
                                     arr.coords["time"])
        assert rem.dtype == np.float64 and cor.dtype == np.float64 and line.dtype == np.float64
        assert rem.is_device == a.is_device and line.is_device == a.is_device
        assert_bit_equal(rem.values, y - (m * xs + b), "mode=remove")
        assert_bit_equal(cor.values, y - m * xs, "mode=correct")
        assert_bit_equal(np.moveaxis(line.values, -1, 0), m * xs, "broadcast_trend")


# ---- (d) a NaN step takes its whole cell in the projected fits ---------------------------------
def test_one_nan_step_makes_the_cell_nan_in_seasonal_fits():
    d = test_data.generate_test_data_time(start_year=1979, nyears=2, frequency="D")
    y = d["var_a"].values.copy()
    y[100, 1, 2] = np.nan
    arr = DataArray(y, d["var_a"].dims, d["var_a"].coords, d["var_a"].attrs, "var_a")
    hit = np.zeros((5, 5), dtype=bool)
    hit[1, 2] = True
    for fmt in ("residuals", "model", "coeff"):
        got = trend.deseason(arr, output_format=fmt)
        assert np.array_equal(np.isnan(got.values), np.broadcast_to(hit, got.shape)), fmt
    coeff = trend.deseason(arr, output_format="coeff")
    assert coeff.dims == ("coeff", "lat", "lon") and coeff.shape == (6, 5, 5)
    assert list(coeff.coords["coeff"].values) == ["constant", "trend", "sin_annual", "cos_annual",
                                                  "sin_semiannual", "cos_semiannual"]
    smodel, resid = trend.seasonal_model(arr, return_model=True)
    assert np.array_equal(np.isnan(resid.values), np.broadcast_to(hit, resid.shape))
    assert np.array_equal(np.isnan(smodel.values), np.broadcast_to(hit[..., None], smodel.shape))


# ---- (e) determinism, block independence, the documented deviation ---------------------------
def test_results_are_deterministic_and_independent_of_the_cell_blocks(monkeypatch):
    nt = 1825
    coord, x = _axis("daily", nt)
    y = _field(nt, (9, 11), np.float64, seed=77)
    arr = DataArray(y, ("time", "a", "b"), {"time": DataArray(coord, ("time",))}, None, "eta")

    def everything(a):
        fit = trend.calc_linear_trend(a)
        return [fit["eta_slope"].values, fit["eta_intercept"].values,
                trend.linear_detrend(a).values, trend.deseason(a, output_format="coeff").values,
                trend.deseason(a).values]

    base = everything(arr)
    for what, again in (("second call", everything(arr)), ("device", everything(_on_device(arr)))):
        for g, w in zip(again, base):
            assert_bit_equal(g, w, what)
    for block in (1, 7, 32, 50):  # blocks of cells that change the pack width and leave a tail
        monkeypatch.setattr(record, "BLOCK_CELLS", block)
        for g, w in zip(everything(arr), base):
            assert_bit_equal(g, w, f"blocks of {block} cells")


def test_fewer_than_two_valid_steps_give_nan():
    """the documented deviation: numpy's lstsq would return a minimum-norm answer and a RankWarning"""
    y = np.random.default_rng(1).normal(size=(24, 6))
    y[1:, 0] = np.nan          # one valid step
    y[:, 1] = np.nan           # none
    y[2:, 2] = np.nan          # two: a line through them
    arr = DataArray(y, ("time", "x"), {"time": DataArray(np.arange(24.0), ("time",))}, None, "v")
    fit = trend.calc_linear_trend(arr)
    m, b = fit["v_slope"].values, fit["v_intercept"].values
    assert np.isnan(m[:2]).all() and np.isnan(b[:2]).all() and not np.isnan(m[2:]).any()
    assert np.isclose(m[2], y[1, 2] - y[0, 2]) and np.isclose(b[2], y[0, 2])
    assert "units" not in fit["v_slope"].attrs  # a numeric axis: no time-unit handling


# ---- (f) end to end on a steric() result -------------------------------------------------------
def test_trend_of_a_steric_result_end_to_end(monkeypatch):
    d = test_data.generate_test_data(nyears=2)
    res, _ = steric(d, domain="local")
    eta = res["steric"]
    fit = trend.calc_linear_trend(eta, time_units="yr")
    x = tn.ns_axis(eta.coords["time"].values)
    want_m, want_b = tn.polyfit_columns(x, eta.values)
    m = fit["steric_slope"].values / trend.time_conversion_factor("yr", "ns")
    ok = ~np.isnan(want_m)
    assert np.array_equal(np.isnan(m), ~ok) and ok.any()
    e_m = np.max(np.abs(m - want_m)[ok] / np.abs(want_m[ok]))
    e_b = np.max(np.abs(fit["steric_intercept"].values - want_b)[ok]) / (
        np.nanmax(np.abs(eta.values)) * (1 + abs(x.mean()) / (x.max() - x.min())))
    print(f"steric trend: slope {e_m:.2e} intercept {e_b:.2e}")
    assert e_m <= GATE and e_b <= GATE
    assert fit["steric_slope"].attrs["units"].endswith(" yr-1")

    # device tensors in: device tensors out, and the record never crosses the host link
    dd = d.copy()
    for k in ("thetao", "so", "volcello"):
        dd[k] = DataArray(torch.from_numpy(d[k].values).cuda(), d[k].dims)
    dres, _ = steric(dd, domain="local")
    assert dres["steric"].is_device
    from momlevel_amd import hostio

    moved = []
    for name in ("to_device", "to_host", "upload", "download_into"):
        real = getattr(hostio, name)

        def spy(*args, _real=real, _name=name, **kw):
            big = max((a.numel() * a.element_size() if isinstance(a, torch.Tensor) else
                       getattr(a, "nbytes", 0)) for a in args)
            moved.append((_name, big))
            return _real(*args, **kw)

        monkeypatch.setattr(hostio, name, spy)
    dfit = trend.calc_linear_trend(dres["steric"], time_units="yr")
    resid = trend.linear_detrend(dres["steric"])
    monkeypatch.undo()
    assert dfit["steric_slope"].is_device and dfit["steric_intercept"].is_device and resid.is_device
    record = dres["steric"].data.numel() * 8
    print("host link on the device path:", moved)
    assert all(nbytes <= 24 * 8 for _, nbytes in moved) and record > 24 * 8  # the axis table only
    assert_bit_equal(dfit["steric_slope"].values, fit["steric_slope"].values, "device path")
