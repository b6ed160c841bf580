"""CPU: the numpy restatement tests/quantile_numpy.py against numpy's own nanquantile, the C ABI of
include/momlevel_quantile.h (symbols, binding table, argument errors -- they precede every HIP
call), ``climatology.yearly_plan`` and the Python layer of momlevel_amd.extremes (validation of q,
dims, coords and dtypes of the results) through stubs of the two core calls.  No GPU."""

import ctypes
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

import quantile_numpy as qn
from momlevel_amd import _lib, climatology, core, extremes
from momlevel_amd.cftime_lite import DatetimeLite, daily_midpoints
from momlevel_amd.labeled import DataArray, Dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "momlevel_quantile.h")
NAMES = ["mlx_quantile_block_cells", "mlx_quantile_exceed_count", "mlx_quantile_select",
         "mlx_quantile_unroll"]
LEVELS = (0.0, 0.01, 0.25, 0.5, 0.9, 0.99, 1.0)


def _columns(nt, rng):
    """(nt, 60): random data, five-level ties, 30 % NaN, all-NaN columns, +-inf"""
    y = rng.normal(0.0, 1.0, (nt, 60))
    y[:, 12:24] = rng.integers(0, 5, (nt, 12)) * 0.25 - 0.5
    holes = rng.random((nt, 12)) < 0.3
    y[:, 24:36][holes] = np.nan
    y[:, 36:40] = np.nan
    y[:, 40:50][rng.random((nt, 10)) < 0.2] = np.inf
    y[:, 45:55][rng.random((nt, 10)) < 0.2] = -np.inf
    y[:, 55:60][rng.random((nt, 5)) < 0.3] = np.nan
    return y


def _nanquantile(y, q):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # all-NaN slices, inf - inf
        return np.nanquantile(y, q, axis=0)


# ---- the restatement against numpy ----------------------------------------------------------------
def test_restatement_is_numpy_nanquantile():
    rng = np.random.default_rng(20)
    cells = 0
    for nt in range(1, 41):
        y = _columns(nt, rng)
        for q in LEVELS + (float(rng.random()),):
            want = _nanquantile(y, q)
            got = qn.time_quantile(y, q)[0, 0]
            qn.assert_values(got, want, f"nt={nt} q={q}")
            cells += got.size
    assert cells == 19200


def test_restatement_groups_and_levels():
    rng = np.random.default_rng(21)
    y = _columns(30, rng)
    steps = np.array([3, 1, 2, 2, 29, 0, 7, 8, 9], dtype=np.int32)
    offsets = np.array([0, 4, 4, 5, 9], dtype=np.int64)
    got = qn.time_quantile(y, [0.25, 0.5], steps, offsets)
    assert got.shape == (2, 4, 60) and np.isnan(got[:, 1]).all()  # the empty group
    for gi, sel in enumerate(([3, 1, 2, 2], None, [29], [0, 7, 8, 9])):
        if sel is not None:
            qn.assert_values(got[1, gi], _nanquantile(y[sel], 0.5), f"group {gi}")
    # a one-step group is its step -- but for an infinite one: numpy's lerp makes inf - inf of it
    want = np.where(np.isinf(y[29]), np.nan, y[29])
    assert np.isinf(y[29]).any() and np.array_equal(got[0, 2], want, equal_nan=True)


def test_float32_rule_is_the_float64_result_rounded_once():
    rng = np.random.default_rng(22)
    y = _columns(37, rng).astype(np.float32)
    differs = 0
    for q in LEVELS + (1.0 / 3.0,):
        want = _nanquantile(y.astype(np.float64), q).astype(np.float32)
        got = qn.rounded_once(qn.time_quantile(y, q)[0, 0])
        qn.assert_values(got, want, f"float32 q={q}")
        differs += int(np.sum(~qn_equal(got, _nanquantile(y, q))))
    print(f"cells where numpy's float32 lerp differs from the rounded-once rule: {differs}")


def qn_equal(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def test_restatement_on_hand_computed_columns():
    y = np.array([[1.0, np.nan, 5.0], [2.0, np.nan, np.nan], [4.0, np.nan, np.nan],
                  [8.0, np.nan, np.nan], [16.0, np.nan, np.nan]])
    assert qn.time_quantile(y, 0.5)[0, 0].tolist()[::2] == [4.0, 5.0]
    assert np.isnan(qn.time_quantile(y, 0.5)[0, 0, 1])
    # c = 5: q = 0.1 -> vi = 0.4 (g < 0.5), q = 0.15 -> vi = 0.6 (g >= 0.5)
    assert qn.time_quantile(y, 0.1)[0, 0, 0] == 1.0 + 1.0 * (4.0 * 0.1)
    assert qn.time_quantile(y, 0.15)[0, 0, 0] == 2.0 - 1.0 * (1.0 - 4.0 * 0.15)
    assert qn.time_quantile(y, [0.0, 1.0])[:, 0, 0].tolist() == [1.0, 16.0]
    thr = np.array([[2.0, 0.0, np.nan]])
    assert qn.exceed_count(y, thr).tolist() == [[3, 0, 0]]
    assert qn.exceed_count(y, thr).dtype == np.int64


# ---- the calendar plan -----------------------------------------------------------------------------
@pytest.mark.parametrize("calendar, days", [("noleap", (365, 365, 365)), ("standard", (365, 366, 365))])
def test_yearly_plan_on_a_daily_axis(calendar, days):
    axis = np.array(daily_midpoints(2003, 3, calendar), dtype=object)
    assert axis.size == sum(days)
    plan = climatology.yearly_plan(DataArray(axis, ("time",), None, None, "time"), "time")
    assert plan.ngroups == 3 and tuple(plan.sizes) == days
    assert plan.steps.dtype == np.int32 and plan.offsets.dtype == np.int64
    assert plan.steps.tolist() == list(range(sum(days)))
    assert plan.offsets.tolist() == [0] + np.cumsum(days).tolist()
    mids = list(plan.time.values)
    assert [t.year for t in mids] == [2003, 2004, 2005] and plan.time.dims == ("time",)
    assert all(isinstance(t, DatetimeLite) for t in mids)
    # the middle of the year: July 2 12:00 of a 365-day year, July 2 00:00 of a leap year
    assert [(t.month, t.day, t.hour) for t in mids] == [(7, 2, 12 if d == 365 else 0) for d in days]


def test_yearly_plan_takes_ragged_and_unordered_years():
    axis = np.array([DatetimeLite(2001, 3, 1), DatetimeLite(1999, 12, 31), DatetimeLite(2001, 1, 5),
                     DatetimeLite(2001, 7, 9)], dtype=object)
    plan = climatology.yearly_plan(DataArray(axis, ("t",), None, None, "t"), "t")
    assert plan.ngroups == 2 and plan.sizes == [1, 3] and plan.steps.tolist() == [1, 0, 2, 3]
    assert [t.year for t in plan.time.values] == [1999, 2001] and plan.time.dims == ("t",)
    with pytest.raises(TypeError):
        climatology.yearly_plan(DataArray(np.arange(4.0), ("t",), None, None, "t"), "t")
    assert "yearly_plan" in climatology.__all__


# ---- the Python layer through stubs of the core calls ---------------------------------------------
@pytest.fixture
def stubbed(monkeypatch):
    """core.time_quantile / time_exceed_count answered by the restatement on CPU tensors, host
    records walked in blocks of 7 cells without a device"""
    from momlevel_amd import engine, hostio, record

    calls = []

    def time_quantile(y, q, steps=None, offsets=None, out=None):
        lists = (None, None) if steps is None else (steps.steps.numpy(), steps.offsets.numpy())
        calls.append(("q", tuple(y.shape), None if steps is None else steps.ngroups))
        res = qn.time_quantile(y.numpy(), q, *lists)
        return torch.from_numpy(res.astype(np.float32 if y.dtype == torch.float32 else np.float64))

    def time_exceed_count(y, thr, steps=None, offsets=None):
        lists = (None, None) if steps is None else (steps.steps.numpy(), steps.offsets.numpy())
        calls.append(("x", tuple(y.shape), tuple(thr.shape)))
        return torch.from_numpy(qn.exceed_count(y.numpy(), thr.numpy(), *lists))

    monkeypatch.setattr(core, "time_quantile", time_quantile)
    monkeypatch.setattr(core, "time_exceed_count", time_exceed_count)
    monkeypatch.setattr(record, "BLOCK_CELLS", 7)
    monkeypatch.setattr(engine, "device_of", lambda *a, **k: torch.device("cpu"))
    monkeypatch.setattr(hostio, "to_device", lambda x, device, dtype=None: torch.from_numpy(
        np.ascontiguousarray(x)) if dtype is None else torch.from_numpy(
        np.ascontiguousarray(x)).to(dtype))
    monkeypatch.setattr(hostio, "to_host", lambda t: t.numpy())
    return calls


def _daily(nyears=3, ny=6, nx=5, dtype=np.float64, seed=5):
    axis = np.array(daily_midpoints(2001, nyears, "noleap"), dtype=object)
    rng = np.random.default_rng(seed)
    y = rng.normal(0.0, 1.0, (axis.size, ny, nx)).astype(dtype)
    y[rng.random(y.shape) < 0.1] = np.nan
    y[:, 0, 0] = np.nan
    coords = {"time": DataArray(axis, ("time",), None, None, "time"),
              "yh": DataArray(np.arange(ny) * 1.0, ("yh",), None, None, "yh"),
              "xh": DataArray(np.arange(nx) * 1.0, ("xh",), None, None, "xh")}
    da = DataArray(y, ("time", "yh", "xh"), coords, {"units": "m"}, "zos")
    da.encoding = {"dtype": "float32"}
    return da


@pytest.mark.parametrize("bad", (-0.1, 1.5, np.nan, [0.5, 2.0], [], [[0.1, 0.2]], "median", None))
def test_q_is_validated_before_anything_else(stubbed, bad):
    with pytest.raises(ValueError):
        extremes.time_quantile(_daily(1), bad)
    with pytest.raises(ValueError):
        core.quantile_levels(bad)
    assert stubbed == []


def test_other_refusals(stubbed):
    da = _daily(1)
    for kw in (dict(by="season"), dict(tcoord="t"), dict(time_axis_year=2000),
               dict(by="year", time_axis_year=2000)):
        with pytest.raises(ValueError):
            extremes.time_quantile(da, 0.5, **kw)
    with pytest.raises(TypeError):
        extremes.time_quantile(np.ones((4, 3)), 0.5)
    with pytest.raises(TypeError):
        extremes.time_quantile(DataArray(np.ones((4, 3), dtype=np.float16), ("time", "x")), 0.5)
    with pytest.raises(TypeError):
        extremes.exceedance_count(da, [1.0, 2.0])
    with pytest.raises(ValueError):
        extremes.exceedance_count(da, DataArray(np.ones(5), ("xh",)))
    with pytest.raises(ValueError):  # 12 thresholds for one group
        extremes.exceedance_count(da, extremes.time_quantile(da, 0.9, by="month"))
    assert core.quantile_levels(0.5).tolist() == [0.5] and core.quantile_levels([0, 1]).dtype == np.float64


def test_layout_of_scalar_and_sequence_q(stubbed):
    da = _daily(1)
    want = qn.time_quantile(da.values, [0.05, 0.5, 0.95])[:, 0].reshape(3, 6, 5)
    seq = extremes.time_quantile(da, [0.05, 0.5, 0.95])
    assert seq.dims == ("quantile", "yh", "xh") and seq.dtype == np.float64
    assert seq.coords["quantile"].dims == ("quantile",)
    assert seq.coords["quantile"].values.dtype == np.float64
    assert seq.coords["quantile"].values.tolist() == [0.05, 0.5, 0.95]
    assert "time" not in seq.coords and set(seq.coords) == {"quantile", "yh", "xh"}
    assert seq.attrs == {"units": "m"} and seq.name == "zos" and seq.encoding == {"dtype": "float32"}
    qn.assert_values(seq.values, want, "sequence q")
    one = extremes.time_quantile(da, 0.5)
    assert one.dims == ("yh", "xh") and one.coords["quantile"].dims == ()
    assert float(one.coords["quantile"].values) == 0.5
    qn.assert_values(one.values, want[1], "scalar q")
    qn.assert_values(extremes.time_median(da).values, want[1], "median")
    single = extremes.time_quantile(da, [0.5])
    assert single.dims == ("quantile", "yh", "xh") and single.shape == (1, 6, 5)
    # host records went through in blocks of 7 cells: 30 cells are 5 calls a variable
    assert [c[1] for c in stubbed[:5]] == [(365, 7)] * 4 + [(365, 2)]


def test_grouped_layout_keeps_the_input_order_of_dims(stubbed):
    da = _daily(3, dtype=np.float32).transpose("yh", "time", "xh")
    by_month = extremes.time_quantile(da, [0.5, 0.99], by="month", time_axis_year=1990)
    assert by_month.dims == ("quantile", "yh", "time", "xh") and by_month.shape == (2, 6, 12, 5)
    assert by_month.dtype == np.float32
    axis = by_month.coords["time"].values
    assert [t.month for t in axis] == list(range(1, 13)) and {t.year for t in axis} == {1990}
    plan = climatology.annual_cycle_plan(da["time"], "time", 1990)
    y = da.transpose("time", "yh", "xh").values
    want = qn.rounded_once(qn.time_quantile(y, [0.5, 0.99], plan.steps, plan.offsets))
    qn.assert_values(np.moveaxis(by_month.values, 2, 1).reshape(2, 12, 30), want, "by month")
    by_year = extremes.time_quantile(da, 0.99, by="year")
    assert by_year.dims == ("yh", "time", "xh") and by_year.shape == (6, 3, 5)
    assert [t.year for t in by_year.coords["time"].values] == [2001, 2002, 2003]
    assert extremes.time_median(da, by="year").dims == ("yh", "time", "xh")


def test_dataset_rules_and_exceedance_layout(stubbed):
    da = _daily(2)
    ds = Dataset({"zos": da, "label": DataArray(np.array(["a"] * da.shape[0]), ("time",)),
                  "depth": DataArray(np.ones((6, 5)), ("yh", "xh")),
                  "count": DataArray(np.arange(da.shape[0] * 5).reshape(-1, 5), ("time", "xh"))})
    res = extremes.time_quantile(ds, 0.9, by="year")
    assert sorted(res.data_vars) == ["count", "zos"]
    assert res["zos"].dims == ("time", "yh", "xh") and res["zos"].shape == (2, 6, 5)
    assert res["count"].dtype == np.float64 and res["time"].shape == (2,)
    assert float(res["quantile"].values) == 0.9
    with pytest.raises(ValueError):
        extremes.time_quantile(ds, 0.9, tcoord="t")
    # counts: a number, a per-cell field, and the grouped quantiles themselves
    y = da.values.reshape(da.shape[0], -1)
    n0 = extremes.exceedance_count(da, 0.5)
    assert n0.dims == ("yh", "xh") and n0.dtype == np.int64 and n0.name == "zos"
    assert np.array_equal(n0.values.reshape(-1), qn.exceed_count(y, np.full((1, 30), 0.5))[0])
    med = extremes.time_median(da)
    n1 = extremes.exceedance_count(da, med)
    assert np.array_equal(n1.values.reshape(1, -1), qn.exceed_count(y, med.values.reshape(1, -1)))
    p90 = extremes.time_quantile(da, 0.9, by="month")
    n2 = extremes.exceedance_count(da.transpose("yh", "xh", "time"), p90, by="month")
    assert n2.dims == ("yh", "xh", "time") and n2.shape == (6, 5, 12) and n2.dtype == np.int64
    plan = climatology.annual_cycle_plan(da["time"], "time")
    want = qn.exceed_count(y, p90.values.reshape(12, -1), plan.steps, plan.offsets)
    assert np.array_equal(np.moveaxis(n2.values, 2, 0).reshape(12, -1), want)
    nds = extremes.exceedance_count(ds, res, by="year")
    assert sorted(nds.data_vars) == ["count", "zos"] and nds["zos"].dtype == np.int64


def test_package_exports_the_module():
    import momlevel_amd

    assert momlevel_amd.extremes is extremes and "extremes" in momlevel_amd.__all__
    assert "EXTENSION" in extremes.__doc__ and "extremes" in momlevel_amd.__doc__
    assert extremes.__all__ == ["time_quantile", "time_median", "exceedance_count"]


# ---- the C ABI -------------------------------------------------------------------------------------
def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_binding_table_and_library_agree():
    text = _header_text()
    declared = sorted(set(re.findall(r"\b(mlx_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.QUANTILE_SIGNATURES) == NAMES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in momlevel_quantile.h but not exported"
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                             text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(mlx_quantile_[a-z0-9_]+)\b", out))) == declared
    ctype = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p,
             "const double *": ctypes.c_void_p, "const int32_t *": ctypes.c_void_p,
             "const int64_t *": ctypes.c_void_p, "int64_t *": ctypes.c_void_p,
             "int64_t ": ctypes.c_int64, "int ": ctypes.c_int}
    protos = re.findall(r"\b(int64_t|int)\s+(mlx_[a-z_]+)\s*\(([^)]*)\)", text)
    assert sorted(p[1] for p in protos) == declared
    for ret, name, args in protos:
        args = [" ".join(a.split()) for a in args.split(",")]
        restype, argtypes = _lib.QUANTILE_SIGNATURES[name]
        assert restype is (ctypes.c_int if ret == "int" else ctypes.c_int64), name
        if args == ["void"]:
            assert argtypes == []
            continue
        assert argtypes == [next(v for k, v in ctype.items() if a.startswith(k)) for a in args], name
        if ret == "int":
            assert args[-1] == "void *stream", name
    assert re.findall(r"#define MLX_(QUANTILE_[A-Z_]+)\s+(\d+)", text) == [("QUANTILE_MAX_Q", "8")]
    assert _lib.QUANTILE_MAX_Q == 8
    assert _lib.load_quantile() is _lib.load()


def test_geometry_queries():
    assert core.quantile_block_cells(np.float64) * 2 == core.quantile_block_cells(np.float32)
    assert core.quantile_block_cells() % 64 == 0 and core.quantile_unroll() >= 1
    lib = _lib.load_quantile()
    assert lib.mlx_quantile_block_cells(2) == 0 and lib.mlx_quantile_block_cells(-1) == 0


def test_other_tables_and_the_abi_version_are_untouched():
    for name in _lib.QUANTILE_SIGNATURES:
        for table in (_lib.SIGNATURES, _lib.TREND_SIGNATURES, _lib.CLIM_SIGNATURES,
                      _lib.GAUGE_SIGNATURES, _lib.SPICE_SIGNATURES, _lib.VORT_SIGNATURES,
                      _lib.AREA_SIGNATURES, _lib.LAYER_SIGNATURES, _lib.FILTER_SIGNATURES,
                      _lib.PATH_SIGNATURES):
            assert name not in table
    assert len(_lib.SIGNATURES) == 28
    assert _lib.ABI_VERSION == 9 and _lib.load().mlx_version() == 9


F = 1 << 20  # a pointer that is never dereferenced: the checks precede every HIP call


def _args(kw):
    a = dict(y=F, dt=_lib.DTYPE_F64, steps=F, offsets=F, nsel=24, ngroups=12, nt=0, n=10)
    a.update(kw)
    return a


def select_call(lib, **kw):
    """mlx_quantile_select with arguments that pass every check but nt (0), ``kw`` replacing some"""
    a = _args(dict(dict(q=(0.5, 0.99), out=F), **kw))
    q = a["q"]
    qbuf = None if q is None else (ctypes.c_double * max(len(q), 1))(*q)
    nq = a.get("nq", 0 if q is None else len(q))
    return lib.mlx_quantile_select(a["y"], a["dt"], a["steps"], a["offsets"], a["nsel"],
                                   a["ngroups"], a["nt"], a["n"], qbuf, nq, a["out"], None)


def exceed_call(lib, **kw):
    a = _args(dict(dict(thr=F, out=F), **kw))
    return lib.mlx_quantile_exceed_count(a["y"], a["dt"], a["steps"], a["offsets"], a["nsel"],
                                         a["ngroups"], a["nt"], a["n"], a["thr"], a["out"], None)


NULL, SHAPE, ENUM, ALIGN = -1, -2, -3, -5
SHARED_REFUSALS = [
    (dict(y=None), NULL), (dict(out=None), NULL), (dict(steps=None), NULL),
    (dict(offsets=None), NULL), (dict(steps=None, offsets=None), NULL),  # 12 groups of no list
    (dict(dt=2), ENUM), (dict(dt=-1), ENUM), (dict(dt=7), ENUM),
    (dict(nt=0), SHAPE), (dict(nt=-4), SHAPE), (dict(n=0), SHAPE), (dict(n=-1), SHAPE),
    (dict(nsel=0), SHAPE), (dict(nsel=-3), SHAPE), (dict(ngroups=0), SHAPE),
    (dict(ngroups=-1), SHAPE), (dict(nt=1 << 31), SHAPE), (dict(nsel=1 << 31), SHAPE),
    (dict(n=(1 << 38) + 1), SHAPE), (dict(nt=1 << 30, n=1 << 38), SHAPE),
    (dict(ngroups=1 << 40, n=1 << 38), SHAPE),
    (dict(steps=None, offsets=None, ngroups=1, nsel=19), SHAPE),  # no list: nsel is nt
    (dict(y=F + 4), ALIGN), (dict(y=F + 2, dt=1), ALIGN), (dict(steps=F + 2), ALIGN),
    (dict(offsets=F + 4), ALIGN), (dict(out=F + 4), ALIGN),
]
SELECT_REFUSALS = [
    (dict(q=None), NULL), (dict(q=(), nq=0), SHAPE), (dict(q=(0.5,) * 9), SHAPE),
    (dict(q=(0.5,), nq=-1), SHAPE), (dict(q=(0.5, 1.5)), ENUM), (dict(q=(-0.25,)), ENUM),
    (dict(q=(float("nan"),)), ENUM), (dict(out=F + 2, dt=1), ALIGN),
]
EXCEED_REFUSALS = [(dict(thr=None), NULL), (dict(thr=F + 4), ALIGN), (dict(out=F + 4, dt=1), ALIGN)]


def test_argument_errors_need_no_gpu():
    lib = _lib.load_quantile()
    for kw, code in SHARED_REFUSALS:
        kw = dict(dict(nt=20), **kw)
        assert select_call(lib, **kw) == code and _lib.last_error(), kw
        assert exceed_call(lib, **kw) == code and _lib.last_error(), kw
    for kw, code in SELECT_REFUSALS:
        assert select_call(lib, **dict(dict(nt=20), **kw)) == code and _lib.last_error(), kw
    for kw, code in EXCEED_REFUSALS:
        assert exceed_call(lib, **dict(dict(nt=20), **kw)) == code and _lib.last_error(), kw
    assert "NULL" in (select_call(lib, nt=20, out=None), _lib.last_error())[1]
    assert "[0, 1]" in (select_call(lib, nt=20, q=(2.0,)), _lib.last_error())[1]
    assert "nsel must equal nt" in (exceed_call(lib, nt=20, steps=None, offsets=None, ngroups=1),
                                    _lib.last_error())[1]


def test_a_library_without_the_kernels_is_an_error(monkeypatch):
    class Bare:
        def __getattr__(self, name):
            raise AttributeError(name)

    monkeypatch.setattr(_lib, "_quantile_bound", False)
    monkeypatch.setattr(_lib, "load", lambda: Bare())
    with pytest.raises(_lib.MomlevelHipError, match="does not export mlx_[a-z_]+: rebuild"):
        _lib.load_quantile()


def test_features_has_the_row_and_a_sha_of_its_own():
    from momlevel_amd.csrc import build

    assert build.FEATURES["quantile"] == ["eos_device.hpp", "mlx_internal.hpp", "mlx_pack.hpp",
                                          "mlx_record.hpp", "include/momlevel_quantile.h"]
    assert len(build.quantile_source_sha()) == 16
    assert build.quantile_source_sha() == build.feature_source_sha("quantile")
    assert build.quantile_source_sha() not in (build.source_sha(), build.clim_source_sha(),
                                               build.filter_source_sha())
    names = {os.path.basename(p) for p in build.TIMED_SOURCES}
    assert "momlevel_quantile.hip" not in names and "momlevel_quantile.h" not in names
    assert any(p.endswith("momlevel_quantile.hip") for p in build.SOURCES)
    assert any(p.endswith("momlevel_quantile.h") for p in build.DEPENDS)
    text = open(os.path.join(ROOT, "momlevel_amd", "csrc", "momlevel_quantile.hip")).read()
    assert "#pragma clang fp contract(off)" in text and "atomic" not in text.replace("atomics", "")
    assert "__shared__" not in text
