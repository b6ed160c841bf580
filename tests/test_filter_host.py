"""CPU: the numpy restatement tests/filter_numpy.py against numpy's own nanmean and polyfit (and its
tap-loop form for long records against the restatement, bit for bit), the C
ABI of include/momlevel_filter.h (symbols, binding table, argument errors -- they precede every HIP
call), the host-side tables of momlevel_amd.filters (window placement, Lanczos weights, the running
least-squares table) and every Python-level refusal.  No GPU."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import filter_numpy as fn
from conftest import assert_bit_equal
from momlevel_amd import _lib, core, filters
from momlevel_amd.cftime_lite import DatetimeLite, axis_to_numeric
from momlevel_amd.labeled import DataArray, Dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "momlevel_filter.h")
NAMES = ["mlx_filter_apply", "mlx_filter_tile", "mlx_filter_tiles_per_block",
         "mlx_filter_window_edge"]


def _record(nt=60, n=37, seed=3):
    rng = np.random.default_rng(seed)
    y = rng.normal(0.1, 0.05, (nt, n))
    y[rng.random((nt, n)) < 0.05] = np.nan
    y[:, 4] = np.nan  # a land column
    return y


def _monthly_axis(nt, calendar="noleap", year0=1990):
    return np.array([DatetimeLite(year0 + m // 12, m % 12 + 1, 16, calendar=calendar)
                     for m in range(nt)], dtype=object)


# ---- the restatement against numpy ----------------------------------------------------------------
@pytest.mark.parametrize("window, center", [(1, True), (4, True), (5, True), (12, False), (13, True),
                                            (60, True)])
def test_restatement_is_nanmean_over_the_window(window, center):
    y = _record()
    lead = filters.window_lead(window, center)
    for mp in (1, window):
        got = fn.time_filter(y, np.ones(window), lead, mp, normalise=True)
        assert_bit_equal(got, fn.rolling_mean_nanmean(y, window, center, mp),
                         f"window {window} min_periods {mp}")
    assert np.isnan(got[:, 4]).all()


WEIGHT_SEED = 11


@pytest.mark.parametrize("window, center", [(1, True), (4, True), (5, True), (12, False), (13, True),
                                            (60, True)])
def test_the_tap_loop_is_the_restatement_bit_for_bit(window, center):
    """filter_numpy.time_filter_taps (a loop over the taps, for long records) against time_filter
    (the loop over steps and taps): both leads and one that is neither, every min_count that
    matters, both normalisations, a row and a table of weights"""
    y = _record()
    y[:, 7] = -0.0  # (the sign of a zero sum is part of the bits)
    nt = y.shape[0]
    rng = np.random.default_rng(WEIGHT_SEED + window)
    row = rng.normal(0.0, 1.0, window)
    table = rng.normal(0.0, 1.0, (nt, window))
    leads = sorted({filters.window_lead(window, center), filters.window_lead(window, not center),
                    (window - 1) // 3})
    for lead in leads:
        for w in (np.ones(window), row, table):
            sums = fn.tap_sums(y, w, lead)
            for mc in sorted({1, min(2, window), window}):
                for norm in (False, True):
                    want = fn.time_filter(y, w, lead, mc, norm)
                    what = f"W={window} lead={lead} w{np.shape(w)} mc={mc} norm={norm}"
                    assert_bit_equal(fn.time_filter_taps(y, w, lead, mc, norm), want, what)
                    assert_bit_equal(fn.finish(*sums, mc, norm), want, what + " (finish)")
        assert_bit_equal(fn.time_filter_taps(y, row, lead), fn.time_filter(y, row, lead), "default mc")
    y32 = y.astype(np.float32)
    assert_bit_equal(fn.time_filter_taps(y32, row, leads[0], 1), fn.time_filter(y32, row, leads[0], 1),
                     "a float32 record")
    assert fn.time_filter_taps(y32, row, leads[0], 1).dtype == np.float64


def test_restatement_on_a_hand_computed_series():
    y = np.array([[1.0, -0.0], [2.0, -0.0], [np.nan, -0.0], [4.0, -0.0], [8.0, -0.0]])
    s = fn.time_filter(y, [1.0, 1.0, 1.0], 1, 1)
    assert s[:, 0].tolist() == [3.0, 3.0, 6.0, 12.0, 12.0]
    # a window of -0.0 sums to -0.0 where every step exists, to +0.0 where one is outside
    assert np.signbit(s[1:4, 1]).all() and not np.signbit(s[[0, 4], 1]).any()
    m = fn.time_filter(y, [1.0, 1.0, 1.0], 1, 2, normalise=True)
    assert m[:, 0].tolist() == [1.5, 1.5, 3.0, 6.0, 6.0]
    full = fn.time_filter(y, [1.0, 1.0, 1.0], 1)
    assert np.isnan(full[:, 0]).tolist() == [True, True, True, True, True]
    assert fn.time_filter(y, [0.5, 2.0], 1, 2)[:, 0].tolist()[1] == 0.5 * 1.0 + 2.0 * 2.0  # trailing
    table = np.arange(10.0).reshape(5, 2)
    assert fn.time_filter(y, table, 0, 2)[3, 0] == 6.0 * 4.0 + 7.0 * 8.0  # row t for output t
    assert fn.time_filter(y.astype(np.float32), [1.0], 0).dtype == np.float64


@pytest.mark.parametrize("window", (3, 24, 59))
def test_running_slope_table_against_polyfit(window):
    nt = 60
    x = axis_to_numeric(_monthly_axis(nt))  # months of 28 / 30 / 31 days, in ns
    assert len(set(np.diff(x).tolist())) == 3
    y = _record(nt, 9, seed=5)
    y[:, 4] = np.linspace(-1.0, 1.0, nt)
    lead = filters.window_lead(window, True)
    table = filters.trend_table(x, window, lead)
    got = fn.time_filter(y, table, lead)
    want = fn.polyfit_slopes(x, y, window, lead)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and not np.isnan(want).all()
    m = ~np.isnan(want)
    err = np.max(np.abs(got[m] - want[m])) / np.max(np.abs(want[m]))
    print(f"W={window}: max |table slope - polyfit| / max|slope| = {err:.2e}")
    assert err < 1e-10


def test_trend_table_rows():
    x = np.array([0.0, 1.0, 3.0, 6.0, 10.0])
    t = filters.trend_table(x, 3, 1)
    assert t.shape == (5, 3) and not t[0].any() and not t[4].any()  # incomplete windows: zero rows
    d = x[1:4] - np.mean(x[1:4])
    assert t[2].tolist() == (d / np.sum(d * d)).tolist()
    assert abs(t[2] @ (2.0 + 3.0 * x[1:4]) - 3.0) < 1e-14 and abs(t[2].sum()) < 1e-16
    trailing = filters.trend_table(x, 3, 2)
    assert not trailing[:2].any() and trailing[2:].any(axis=1).all()
    for bad in (dict(window=1, lead=0), dict(window=6, lead=0), dict(window=3, lead=3),
                dict(window=3, lead=-1)):
        with pytest.raises(ValueError):
            filters.trend_table(x, **bad)
    with pytest.raises(ValueError, match="does not vary"):
        filters.trend_table(np.array([0.0, 1.0, 1.0, 1.0, 2.0]), 3, 1)


# ---- window placement and the Lanczos weights ------------------------------------------------------
def test_window_lead_for_odd_even_centred_trailing():
    assert [filters.window_lead(w, True) for w in (1, 2, 3, 4, 12, 13)] == [0, 1, 1, 2, 6, 6]
    assert [filters.window_lead(w, False) for w in (1, 2, 3, 4, 12, 13)] == [0, 1, 2, 3, 11, 12]
    for w in (1, 2, 5, 12):
        for center in (True, False):
            lead = filters.window_lead(w, center)
            lo, hi = fn.window_bounds(20, w, center, 100)
            assert (lo, hi) == (20 - lead, 20 - lead + w)
    # pandas' even centred window [t - w/2, t + w/2 - 1]
    assert fn.window_bounds(20, 12, True, 100) == (14, 26)


@pytest.mark.parametrize("window, cutoff", [(3, 2.0), (13, 6.0), (73, 24.0), (241, 80.0), (9, 24.0)])
def test_lanczos_weights(window, cutoff):
    w = filters.lanczos_weights(window, cutoff)
    m = (window - 1) // 2
    assert w.dtype == np.float64 and w.shape == (window,)
    assert abs(np.sum(w) - 1.0) <= 1e-15
    assert np.array_equal(w, w[::-1])
    assert w[m] == np.max(w)
    k = np.arange(-m, m + 1)
    raw = 2.0 / cutoff * np.sinc(2.0 * k / cutoff) * np.sinc(k / (m + 1.0))
    # absolute: beside a zero of sinc the rounding of its argument (k * 2 / cutoff here, 2 * fc * k
    # there) is the whole weight; the weights are O(2 / cutoff) <= 1
    np.testing.assert_allclose(w, raw / raw.sum(), rtol=0, atol=1e-15)


def test_lanczos_refusals():
    for bad in (12, 0, -3, 2.5):
        with pytest.raises(ValueError):
            filters.lanczos_weights(bad, 6.0)
    for cutoff in (0.0, -2.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            filters.lanczos_weights(13, cutoff)


# ---- Python-level refusals: all before any device work ----------------------------------------------
def _da(nt=24):
    return DataArray(np.ones((nt, 2, 3)), ("time", "yh", "xh"), None, None, "eta")


@pytest.mark.parametrize("fn_", (filters.rolling_mean, filters.rolling_sum))
def test_rolling_refusals(fn_):
    da = _da()
    for kw in (dict(window=0), dict(window=-1), dict(window=25), dict(window=2.5),
               dict(window=12, min_periods=0), dict(window=12, min_periods=13),
               dict(window=12, tcoord="t")):
        with pytest.raises(ValueError):
            fn_(da, **kw)
    with pytest.raises(ValueError):
        fn_(Dataset({"eta": da}), 12, tcoord="t")
    with pytest.raises(TypeError):
        fn_(np.ones((24, 3)), 12)


def test_time_filter_lowpass_and_trend_refusals():
    da = _da()
    for w in ([], [[1.0, 2.0]], [1.0, np.nan], [1.0, np.inf], np.ones(25)):
        with pytest.raises(ValueError):
            filters.time_filter(da, w)
    for kw in (dict(lead=3), dict(lead=-1), dict(min_periods=2), dict(skipna=True, min_periods=0),
               dict(skipna=True, min_periods=4), dict(tcoord="t")):
        with pytest.raises(ValueError):
            filters.time_filter(da, [1.0, 2.0, 1.0], **kw)
    for kw in (dict(cutoff=6, window=12), dict(cutoff=6, edges="wrap"), dict(cutoff=12),
               dict(cutoff=6, tcoord="t")):
        with pytest.raises(ValueError):
            filters.lowpass(da, **kw)
    for kw in (dict(window=1), dict(window=0), dict(window=25), dict(window=12, tcoord="t")):
        with pytest.raises(ValueError):
            filters.rolling_trend(da, **kw)


def test_core_filter_weights_refusals():
    assert core.filter_weights([1, 2, 3], 5).dtype == np.float64
    assert core.filter_weights(np.ones((5, 3)), 5).shape == (5, 3)
    for w, nt in (([], 5), (np.ones((4, 3)), 5), (np.ones(6), 5), ([1.0, np.nan], 5),
                  ([np.inf], 5), (np.ones((2, 2, 2)), 2)):
        with pytest.raises(ValueError):
            core.filter_weights(w, nt)


def test_package_exports_the_module():
    import momlevel_amd

    assert momlevel_amd.filters is filters and "filters" in momlevel_amd.__all__
    assert "EXTENSION" in filters.__doc__ and "filters" in momlevel_amd.__doc__
    for name in ("rolling_mean", "rolling_sum", "time_filter", "lanczos_weights", "lowpass",
                 "rolling_trend"):
        assert name in filters.__all__ and callable(getattr(filters, name))


# ---- the C ABI -------------------------------------------------------------------------------------
def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_filter_header_declares_exactly_the_three_symbols():
    text = _header_text()
    declared = sorted(set(re.findall(r"\b(mlx_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.FILTER_SIGNATURES) == NAMES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in momlevel_filter.h but not exported"
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                             text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(mlx_filter_[a-z0-9_]+)\b", out))) == declared
    ctype = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p,
             "const double *": ctypes.c_void_p, "int64_t ": ctypes.c_int64, "int ": ctypes.c_int}
    protos = re.findall(r"\b(int64_t|int)\s+(mlx_[a-z_]+)\s*\(([^)]*)\)", text)
    assert sorted(p[1] for p in protos) == declared
    for ret, name, args in protos:
        args = [" ".join(a.split()) for a in args.split(",")]
        restype, argtypes = _lib.FILTER_SIGNATURES[name]
        assert restype is (ctypes.c_int if ret == "int" else ctypes.c_int64), name
        if args == ["void"]:
            assert argtypes == []
            continue
        assert argtypes == [next(v for k, v in ctype.items() if a.startswith(k)) for a in args], name
    assert protos[-1][1] == "mlx_filter_apply" and protos[-1][2].split(",")[-1].strip() == "void *stream"
    assert re.findall(r"#define MLX_(FILTER_[A-Z_]+)\s+(\d+)", text) == [("FILTER_NORMALISE", "1")]
    assert _lib.FILTER_NORMALISE == 1
    assert _lib.load_filter() is _lib.load()


def test_geometry_queries():
    tile, edges = core.filter_tile(), core.filter_window_edges()
    assert tile >= 1 and len(edges) >= 1
    assert list(edges) == sorted(set(edges)) and edges[0] >= 1
    lib = _lib.load_filter()
    assert lib.mlx_filter_window_edge(len(edges)) == 0 and lib.mlx_filter_window_edge(-1) == 0


def test_tiles_per_block_is_plain_arithmetic():
    """per = ceil(ntiles / gy) with gy = min(ceil(target / gx), ntiles): 1 until the launch has its
    blocks without cutting time, then it grows with the cells and with the record"""
    per, tile = core.filter_tiles_per_block, core.filter_tile()
    assert per(1, 1, 1) == 1 and per(96, 2052, 4) == 1 and per(96, 1023, 1) == 1
    # one block of cells: every tile has a block of its own until there are more tiles than the
    # target; the first record past it gives two tiles to all blocks but the last
    hi = 1
    while per(tile * hi + 1, 6, 2) == 1:
        hi *= 2
    lo = hi // 2  # the most tiles that still get a block each lies in (lo, hi]: bisect
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if per(tile * mid + 1, 6, 2) == 1 else (lo, mid)
    target = hi
    assert 1 < target <= 65535
    assert per(tile * target, 6, 2) == 1 and per(tile * target + 1, 6, 2) == 2
    assert per(tile * 2 * target, 6, 2) == 2 and per(tile * 2 * target + 1, 6, 2) == 3
    for v in (1, 2, 4):  # one block of cells at every width
        assert per(tile * target + 1, 4 * v, v) == 2
    # per never shrinks along either axis, and the blocks along time cover the tiles
    for v, n in ((1, 5), (2, 6), (4, 8), (1, 190465), (4, 1 << 21)):
        last = 1
        for nt in (1, tile, tile + 1, 96, 1200, tile * target + 1, 1 << 20):
            p = per(nt, n, v)
            assert last <= p <= -(-nt // tile), (nt, n, v)
            last = p
    wide = [per(96, n, 1) for n in (1, 1 << 10, 1 << 16, 1 << 18, 1 << 20, 1 << 24)]
    assert wide == sorted(wide) and wide[0] == 1 and wide[-1] == -(-96 // tile)
    # refused: extents mlx_filter_apply refuses, widths that are no pack or do not divide n
    lib = _lib.load_filter()
    for nt, n, v in ((0, 6, 2), (-1, 6, 2), (96, 0, 1), (96, -4, 4), (1 << 30, 6, 2),
                     (96, (1 << 38) + 1, 1), (1 << 29, 1 << 38, 2), (96, 6, 0), (96, 6, 3),
                     (96, 6, 8), (96, 6, -1), (96, 6, 4), (96, 5, 2)):
        assert lib.mlx_filter_tiles_per_block(nt, n, v) == 0, (nt, n, v)


def test_other_tables_and_the_abi_version_are_untouched():
    for name in _lib.FILTER_SIGNATURES:
        for table in (_lib.SIGNATURES, _lib.TREND_SIGNATURES, _lib.CLIM_SIGNATURES,
                      _lib.GAUGE_SIGNATURES, _lib.SPICE_SIGNATURES, _lib.VORT_SIGNATURES,
                      _lib.AREA_SIGNATURES, _lib.LAYER_SIGNATURES):
            assert name not in table
    assert len(_lib.SIGNATURES) == 28 and len(_lib.LAYER_SIGNATURES) == 3
    assert _lib.ABI_VERSION == 9 and _lib.load().mlx_version() == 9


def filter_call(lib, **kw):
    """mlx_filter_apply with arguments that pass every check (pointers that are never dereferenced:
    the checks precede every HIP call), ``kw`` replacing some"""
    f = 1 << 20
    a = dict(y=f, dt=_lib.DTYPE_F64, w=f, W=5, stride=0, lead=2, mc=5, flags=0, nt=0, n=10, out=f,
             odt=_lib.DTYPE_F64)
    a.update(kw)
    return lib.mlx_filter_apply(a["y"], a["dt"], a["w"], a["W"], a["stride"], a["lead"], a["mc"],
                               a["flags"], a["nt"], a["n"], a["out"], a["odt"], None)


REFUSALS = [
    (dict(y=None), -1), (dict(w=None), -1), (dict(out=None), -1),
    (dict(dt=2), -3), (dict(dt=-1), -3), (dict(odt=2), -3), (dict(odt=7), -3),
    (dict(flags=2), -3), (dict(flags=3), -3), (dict(flags=-1), -3),
    (dict(nt=0), -2), (dict(nt=-4), -2), (dict(n=0), -2), (dict(n=-1), -2),
    (dict(nt=1 << 30), -2), (dict(n=(1 << 38) + 1), -2), (dict(nt=1 << 29, n=1 << 38), -2),
    (dict(W=0), -2), (dict(W=-1), -2), (dict(W=21, lead=2, mc=5), -2),
    (dict(lead=-1), -2), (dict(lead=5), -2),
    (dict(mc=0), -2), (dict(mc=6), -2),
    (dict(stride=1), -2), (dict(stride=4), -2), (dict(stride=-5), -2), (dict(stride=20), -2),
    (dict(y=(1 << 20) + 4), -5), (dict(y=(1 << 20) + 2, dt=1), -5), (dict(out=(1 << 20) + 4), -5),
    (dict(out=(1 << 20) + 2, odt=1), -5), (dict(w=(1 << 20) + 4), -5),
]


def test_argument_errors_need_no_gpu():
    lib = _lib.load_filter()
    for kw, code in REFUSALS:
        kw = dict(dict(nt=20), **kw)
        assert filter_call(lib, **kw) == code and _lib.last_error(), kw
    assert "NULL" in (filter_call(lib, nt=20, out=None), _lib.last_error())[1]
    assert "min_count" in (filter_call(lib, nt=20, mc=6), _lib.last_error())[1]
    assert "w_stride" in (filter_call(lib, nt=20, stride=3), _lib.last_error())[1]


def test_a_library_without_the_kernel_is_an_error(monkeypatch):
    class Bare:
        def __getattr__(self, name):
            raise AttributeError(name)

    monkeypatch.setattr(_lib, "_filter_bound", False)
    monkeypatch.setattr(_lib, "load", lambda: Bare())
    with pytest.raises(_lib.MomlevelHipError, match="does not export mlx_[a-z_]+: rebuild"):
        _lib.load_filter()


def test_features_has_the_row_and_a_sha_of_its_own():
    from momlevel_amd.csrc import build

    assert build.FEATURES["filter"] == ["eos_device.hpp", "mlx_internal.hpp", "mlx_pack.hpp",
                                        "mlx_record.hpp", "include/momlevel_filter.h"]
    assert len(build.filter_source_sha()) == 16
    assert build.filter_source_sha() == build.feature_source_sha("filter")
    assert build.filter_source_sha() not in (build.source_sha(), build.clim_source_sha(),
                                             build.layer_source_sha(), build.area_source_sha())
    names = {os.path.basename(p) for p in build.TIMED_SOURCES}
    assert "momlevel_filter.hip" not in names and "momlevel_filter.h" not in names
    assert any(p.endswith("momlevel_filter.hip") for p in build.SOURCES)
    assert any(p.endswith("momlevel_filter.h") for p in build.DEPENDS)
    text = open(os.path.join(ROOT, "momlevel_amd", "csrc", "momlevel_filter.hip")).read()
    assert "#pragma clang fp contract(off)" in text and "atomic" not in text.replace("atomics", "")
