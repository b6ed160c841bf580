"""CPU: the C ABI of include/momlevel_smooth.h (symbols, binding table, geometry queries, argument
errors -- they precede every HIP call), the host-side weights and refusals of momlevel_amd.spatial,
and the numpy restatement tests/smooth_numpy.py against a direct, non-separable 2-D normalised
convolution.  No GPU."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import momlevel_amd
import smooth_numpy as sn
from momlevel_amd import _lib, core, spatial
from momlevel_amd.labeled import DataArray, Dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "momlevel_smooth.h")
NAMES = ["mlx_smooth_apply", "mlx_smooth_max_window", "mlx_smooth_record_rows",
         "mlx_smooth_record_window", "mlx_smooth_tile_h", "mlx_smooth_tile_w", "mlx_smooth_tiled"]


# ---- the C ABI ----------------------------------------------------------------------------------
def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_smooth_header_binding_and_exports_agree():
    text = _header_text()
    declared = sorted(set(re.findall(r"\b(mlx_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.SMOOTH_PROTOTYPES) == NAMES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in momlevel_smooth.h but not exported"
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                             text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(mlx_smooth_[a-z0-9_]+)\b", out))) == declared
    ctype = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p,
             "const double *": ctypes.c_void_p, "int64_t ": ctypes.c_int64, "int ": ctypes.c_int}
    rtype = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    protos = re.findall(r"\b(int|int64_t)\s+(mlx_[a-z_]+)\s*\(([^)]*)\)", text)
    assert sorted(p[1] for p in protos) == declared
    for ret, name, args in protos:
        args = [" ".join(a.split()) for a in args.split(",")]
        want = [] if args == ["void"] else [next(v for k, v in ctype.items() if a.startswith(k))
                                           for a in args]
        restype, argtypes = _lib.SMOOTH_PROTOTYPES[name]
        assert restype is rtype[ret] and argtypes == want, name
    assert protos[-1][1] == "mlx_smooth_apply" and protos[-1][2].split(",")[-1].strip() == "void *stream"
    flags = dict(re.findall(r"#define MLX_(SMOOTH_[A-Z_]+)\s+(\d+)", text))
    assert flags == {"SMOOTH_FILL": "1", "SMOOTH_RESIDUAL": "2"}
    assert (_lib.SMOOTH_FILL, _lib.SMOOTH_RESIDUAL) == (1, 2)
    assert _lib.load_smooth() is _lib.load()


def test_other_tables_and_the_abi_version_are_untouched():
    others = [v for k, v in vars(_lib).items() if k.endswith("SIGNATURES")]
    for name in _lib.SMOOTH_PROTOTYPES:
        for table in others + [_lib.EOF_PROTOTYPES]:
            assert name not in table
    assert len(_lib.SIGNATURES) == 28 and len(_lib.EOF_PROTOTYPES) == 5
    assert _lib.ABI_VERSION == 9 and _lib.load().mlx_version() == 9
    assert _lib._GROUPS["smooth"][0] is _lib.SMOOTH_PROTOTYPES
    assert all(name.startswith("mlx_smooth_") for name in _lib.SMOOTH_PROTOTYPES)
    assert "MLX_ABI_VERSION" not in open(HEADER).read().replace("does not move MLX_ABI_VERSION", "")


def test_geometry_queries():
    lib = _lib.load_smooth()
    th, tw = core.smooth_tile(np.float64)
    assert th == lib.mlx_smooth_tile_h() >= 1
    assert tw == lib.mlx_smooth_tile_w(_lib.DTYPE_F64) >= 4 and tw % 4 == 0
    assert core.smooth_tile(np.float32)[1] % 4 == 0
    assert lib.mlx_smooth_tile_w(2) == 0 and lib.mlx_smooth_tile_w(-1) == 0
    assert core.smooth_max_window() >= 33
    assert core.smooth_record_window() >= 1
    with pytest.raises(TypeError):
        core.smooth_tile(np.int32)


def test_launch_queries_are_plain_arithmetic():
    """a block row per record up to the cap; the tiled path for windows up to the largest, rows of
    whole packs and a plane of at least one tile each way -- five conditions, each flipped alone"""
    rows = core.smooth_record_rows
    cap = rows(1 << 30)
    assert 1 < cap <= 65535 and rows(1 << 38) == cap
    for nrec in (1, 2, 1000, cap - 1, cap):
        assert rows(nrec) == nrec
    assert rows(cap + 1) == rows(cap + 3) == cap
    assert rows(0) == 0 and rows(-5) == 0 and rows((1 << 38) + 1) == 0
    tiled = core.smooth_tiled
    th, tw = core.smooth_tile(np.float64)
    maxw = core.smooth_max_window()
    assert maxw <= th + 20 and maxw <= tw  # (so that the planes below hold the largest window)
    ny, nx = th + 20, tw + 4
    assert tiled(maxw, maxw, ny, nx) == 1 and tiled(1, 1, th, tw) == 1 and tiled(maxw, 1, th, tw) == 1
    assert tiled(maxw + 1, maxw, ny, nx) == 0              # Wx
    assert tiled(maxw, maxw + 1, ny, nx) == 0              # Wy
    assert [tiled(maxw, maxw, ny, nx + d) for d in (1, 2, 3, 4)] == [0, 0, 0, 1]  # whole packs
    assert tiled(1, 1, th - 1, nx) == 0 and tiled(1, 1, th, nx) == 1  # a tile of rows
    assert tiled(1, 1, ny, tw - 4) == 0 and tiled(1, 1, ny, tw) == 1  # a tile of columns
    assert tiled(3, 3, 1, 4) == 0 and tiled(3, 1, 1, 4) == 0
    # extents that mlx_smooth_apply refuses
    for Wx, Wy, y, x in ((0, 1, ny, nx), (1, 0, ny, nx), (-1, 1, ny, nx), (1, 1, 0, nx), (1, 1, ny, 0),
                         (1, 1, -th, nx), (1, 1, ny, -tw), (1, th + 1, th, nx), (tw + 4, 1, ny, tw),
                         (1, 1, 1 << 20, 1 << 19)):
        assert tiled(Wx, Wy, y, x) == 0, (Wx, Wy, y, x)
    assert tiled(1, 1, 1 << 19, 1 << 19) == 1  # (2^38 cells: the largest plane)
    lib = _lib.load_smooth()
    assert lib.mlx_smooth_record_rows(cap + 1) == cap and lib.mlx_smooth_tiled(3, 3, th, tw) == 1


def smooth_call(lib, **kw):
    """mlx_smooth_apply with arguments that pass every check (pointers that are never dereferenced:
    the checks precede every HIP call), ``kw`` replacing some"""
    f = 1 << 20
    a = dict(v=f, dt=_lib.DTYPE_F64, area=2 * f, adt=_lib.DTYPE_F32, wx=3 * f, Wx=5, stride=0,
             lx=2, wy=4 * f, Wy=3, ly=1, per=1, mc=1, flags=0, nrec=0, ny=6, nx=8, out=8 * f,
             odt=_lib.DTYPE_F64)
    a.update(kw)
    return lib.mlx_smooth_apply(a["v"], a["dt"], a["area"], a["adt"], a["wx"], a["Wx"], a["stride"],
                                a["lx"], a["wy"], a["Wy"], a["ly"], a["per"], a["mc"], a["flags"],
                                a["nrec"], a["ny"], a["nx"], a["out"], a["odt"], None)


F = 1 << 20
REFUSALS = [
    (dict(v=None), -1), (dict(area=None), -1), (dict(wx=None), -1), (dict(wy=None), -1),
    (dict(out=None), -1),
    (dict(dt=2), -3), (dict(dt=-1), -3), (dict(adt=2), -3), (dict(adt=7), -3), (dict(odt=2), -3),
    (dict(odt=-1), -3), (dict(flags=4), -3), (dict(flags=7), -3), (dict(flags=-1), -3),
    (dict(per=2), -3), (dict(per=-1), -3),
    (dict(nrec=-1), -2), (dict(ny=0), -2), (dict(nx=0), -2), (dict(ny=-3), -2), (dict(nx=-1), -2),
    (dict(nrec=(1 << 38) // 48 + 1), -2), (dict(ny=1 << 20, nx=1 << 19), -2),
    (dict(Wx=0), -2), (dict(Wx=9, lx=2), -2), (dict(Wx=-1), -2),
    (dict(Wy=0), -2), (dict(Wy=7, ly=1), -2),
    (dict(lx=-1), -2), (dict(lx=5), -2), (dict(ly=-1), -2), (dict(ly=3), -2),
    (dict(mc=0), -2), (dict(mc=16), -2), (dict(mc=-2), -2),
    (dict(stride=1), -2), (dict(stride=4), -2), (dict(stride=-5), -2), (dict(stride=8), -2),
    (dict(v=F + 4), -5), (dict(v=F + 2, dt=1), -5), (dict(area=2 * F + 2), -5),
    (dict(area=2 * F + 4, adt=0), -5), (dict(out=8 * F + 4), -5), (dict(out=8 * F + 2, odt=1), -5),
    (dict(wx=3 * F + 4), -5), (dict(wy=4 * F + 4), -5),
    # an out that overlaps an operand: v (2 records of 48 float64), area, wx, wy; ranges that only
    # touch do not overlap
    (dict(out=F), -2), (dict(out=F + 8 * 95), -2), (dict(out=F - 8 * 95), -2),
    (dict(out=2 * F + 4 * 47, odt=1), -2), (dict(out=3 * F + 32), -2), (dict(out=4 * F + 16), -2),
    (dict(out=F + 8 * 96), 0), (dict(out=F - 8 * 96), 0), (dict(out=3 * F + 40), 0),
]


def test_argument_errors_need_no_gpu():
    lib = _lib.load_smooth()
    assert smooth_call(lib) == 0  # nrec == 0: nothing to do, no launch
    assert smooth_call(lib, v=None, out=None) == 0  # (pointers are not looked at)
    for kw, code in REFUSALS:
        if code == 0:
            continue  # (accepted arguments would launch: the GPU tests run them)
        kw = dict(dict(nrec=2), **kw)
        assert smooth_call(lib, **kw) == code and _lib.last_error(), kw
    assert "NULL" in (smooth_call(lib, nrec=2, out=None), _lib.last_error())[1]
    assert "min_count" in (smooth_call(lib, nrec=2, mc=16), _lib.last_error())[1]
    assert "wx_stride" in (smooth_call(lib, nrec=2, stride=3), _lib.last_error())[1]
    assert "overlaps" in (smooth_call(lib, nrec=2, out=F), _lib.last_error())[1]
    assert "lap" in (smooth_call(lib, nrec=2, Wx=9), _lib.last_error())[1]
    # a table of x weights is ny rows long: its range is checked as such
    assert smooth_call(lib, nrec=2, stride=5, out=3 * F + 8 * 29) == -2
    # refused arguments are refused for an empty record too
    assert smooth_call(lib, mc=0) == -2 and smooth_call(lib, dt=5) == -3


def test_a_library_without_the_kernels_is_an_error(monkeypatch):
    class Bare:
        def __getattr__(self, name):
            raise AttributeError(name)

    monkeypatch.setattr(_lib, "_smooth_bound", False)
    monkeypatch.setattr(_lib, "load", lambda: Bare())
    with pytest.raises(_lib.MomlevelHipError, match="does not export mlx_[a-z_]+: rebuild"):
        _lib.load_smooth()


def test_features_has_the_row_and_a_sha_of_its_own():
    from momlevel_amd.csrc import build

    assert build.FEATURES["smooth"] == ["mlx_internal.hpp", "mlx_pack.hpp",
                                        "include/momlevel_smooth.h"]
    assert len(build.smooth_source_sha()) == 16
    assert build.smooth_source_sha() == build.feature_source_sha("smooth")
    assert build.smooth_source_sha() not in (build.source_sha(), build.area_source_sha(),
                                             build.filter_source_sha(), build.vort_source_sha())
    names = {os.path.basename(p) for p in build.TIMED_SOURCES}
    assert "momlevel_smooth.hip" not in names and "momlevel_smooth.h" not in names
    assert any(p.endswith("momlevel_smooth.hip") for p in build.SOURCES)
    assert any(p.endswith("momlevel_smooth.h") for p in build.DEPENDS)
    text = open(os.path.join(ROOT, "momlevel_amd", "csrc", "momlevel_smooth.hip")).read()
    assert "#pragma clang fp contract(off)" in text and "atomic" not in text.replace("atomics", "")
    assert "__shared__" in text and "asm" not in text


# ---- the weights ----------------------------------------------------------------------------------
def test_boxcar_and_gaussian_weights():
    for width in (1, 2, 3, 9):
        w = spatial.boxcar_weights(width)
        assert w.dtype == np.float64 and w.shape == (width,) and np.array_equal(w, w[::-1])
        assert abs(w.sum() - 1.0) <= 1e-15
    for sigma, truncate in ((0.5, 3.0), (1.0, 3.0), (2.5, 2.0), (5.3, 3.0)):
        w = spatial.gaussian_weights(sigma, truncate)
        m = max(1, int(truncate * sigma + 0.5))
        assert w.dtype == np.float64 and w.shape == (2 * m + 1,)
        assert np.array_equal(w, w[::-1]) and w[m] == w.max() and abs(w.sum() - 1.0) <= 1e-15
        k = np.arange(-m, m + 1)
        raw = np.exp(-0.5 * (k / sigma) ** 2)
        np.testing.assert_allclose(w, raw / raw.sum(), rtol=1e-15)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            spatial.boxcar_weights(bad)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            spatial.gaussian_weights(bad)
        with pytest.raises(ValueError):
            spatial.gaussian_weights(1.0, truncate=bad)


@pytest.mark.parametrize("kind", ("gaussian", "boxcar"))
def test_length_scale_weights_widen_where_the_grid_converges(kind):
    dx = 100.0 * np.cos(np.deg2rad(np.array([0.0, 30.0, 60.0, 75.0, 80.0])))
    t = spatial.length_scale_weights(150.0, dx, kind)
    assert t.dtype == np.float64 and t.shape[0] == dx.size and t.shape[1] % 2 == 1
    assert np.array_equal(t, t[:, ::-1])  # every row symmetric about the centre column
    np.testing.assert_allclose(t.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    support = (t != 0.0).sum(axis=1)
    assert list(support) == sorted(support) and support[0] < support[-1] == t.shape[1]
    mid = t.shape[1] // 2
    for r in range(dx.size):  # zero-padded symmetrically
        half = support[r] // 2
        assert not t[r, :mid - half].any() and not t[r, mid + half + 1:].any()
        assert t[r, mid - half:mid + half + 1].all()
    if kind == "gaussian":
        assert np.array_equal(t[0][t[0] != 0], spatial.gaussian_weights(1.5))
    for bad in (dict(scale=0.0), dict(scale=np.nan), dict(dx_rows=[1.0, 0.0]),
                dict(dx_rows=[1.0, np.nan]), dict(dx_rows=[[1.0]]), dict(dx_rows=[]),
                dict(kind="lanczos")):
        kw = dict(dict(scale=1.0, dx_rows=[1.0], kind=kind), **bad)
        with pytest.raises(ValueError):
            spatial.length_scale_weights(**kw)


def test_core_smooth_weights_refusals():
    wx, wy = core.smooth_weights([1, 2, 1], [1, 1, 1, 1, 1], 6, 8)
    assert wx.dtype == wy.dtype == np.float64 and wx.shape == (3,) and wy.shape == (5,)
    assert core.smooth_weights(np.ones((6, 3)), [1.0], 6, 8)[0].shape == (6, 3)
    for bx, by in (([], [1.0]), ([1.0], []), (np.ones((5, 3)), [1.0]), (np.ones(9), [1.0]),
                   ([1.0], np.ones(7)), ([1.0, np.nan], [1.0]), ([1.0], [np.inf]),
                   (np.ones((2, 2, 2)), [1.0]), ([1.0], np.ones((2, 2)))):
        with pytest.raises(ValueError):
            core.smooth_weights(bx, by, 6, 8)


# ---- Python-level refusals: all before any device work -----------------------------------------------
def _record():
    eta = DataArray(np.ones((3, 6, 8)), ("time", "yh", "xh"), None, {"units": "m"}, "zos")
    area = DataArray(np.ones((6, 8)), ("yh", "xh"), None, None, "areacello")
    return eta, area


@pytest.mark.parametrize("fn", (spatial.smooth, spatial.highpass))
def test_refusals_come_before_any_device_work(fn, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(spatial.core, "require_device", boom)
    monkeypatch.setattr(spatial.engine, "device_of", boom)
    monkeypatch.setattr(spatial.hostio, "to_device", boom)
    eta, area = _record()
    neg = area.values.copy()
    neg[2, 3] = -1.0
    with pytest.raises(ValueError, match="negative areas"):
        fn(eta, neg, [1.0, 1.0, 1.0])
    inf = area.values.copy()
    inf[0, 0] = np.inf
    with pytest.raises(ValueError, match="infinite areas"):
        fn(eta, inf, [1.0, 1.0, 1.0])
    for w in ([1.0, np.nan, 1.0], [1.0, np.inf, 1.0], [], np.ones(9), np.ones((2, 2, 2))):
        with pytest.raises(ValueError):
            fn(eta, area, w, [1.0])
    with pytest.raises(ValueError, match="centred window is odd"):
        fn(eta, area, [1.0, 1.0])
    with pytest.raises(ValueError, match="centred window is odd"):
        fn(eta, area, [1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="needs weights_y"):
        fn(eta, area, np.ones((6, 3)))
    with pytest.raises(ValueError, match="one row per row"):
        fn(eta, area, np.ones((5, 3)), [1.0])
    with pytest.raises(ValueError):
        fn(eta, area, [1.0, 1.0, 1.0], np.ones(7))  # taller than the plane
    for mc in (0, 10, 2.5, -1):
        with pytest.raises(ValueError, match="min_count"):
            fn(eta, area, [1.0, 1.0, 1.0], min_count=mc)
    with pytest.raises(ValueError, match="a 2-D"):
        fn(eta, np.ones(48), [1.0])
    with pytest.raises(ValueError, match="last two must be"):
        fn(DataArray(np.ones((6, 3, 8)), ("yh", "time", "xh")), area, [1.0])
    with pytest.raises(ValueError, match="is not areacello's"):
        fn(DataArray(np.ones((3, 6, 8)), ("time", "yh", "xh")), np.ones((8, 6)), [1.0])
    with pytest.raises(ValueError, match="at least the two dims"):
        fn(np.ones(8), area, [1.0])
    with pytest.raises(TypeError):
        fn([[1.0, 2.0]], area, [1.0])
    with pytest.raises(TypeError):
        fn(eta.astype(np.float16), area, [1.0])


def test_the_module_is_published():
    assert momlevel_amd.spatial is spatial and "spatial" in momlevel_amd.__all__
    assert spatial.__all__ == ["smooth", "highpass", "boxcar_weights", "gaussian_weights",
                               "length_scale_weights"]
    assert "EXTENSION" in spatial.__doc__ and "spatial" in momlevel_amd.__doc__
    assert "momlevel_smooth.h" in momlevel_amd.__doc__
    for f in (spatial.smooth, spatial.highpass):
        assert "EXTENSION" in f.__doc__
    for text in (spatial.__doc__, open(HEADER).read()):
        assert "fold" in text and "halo exchange" in text  # what is not built is said
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "spatial.smooth" in readme and "spatial.highpass" in readme
    # the time filters and the area means keep their own lists
    assert "smooth" not in momlevel_amd.filters.__all__ + momlevel_amd.regional.__all__


def test_no_undefined_globals_in_the_new_module():
    from test_static_names import _undefined

    assert _undefined(spatial) == []


# ---- the restatement against a direct 2-D convolution ----------------------------------------------
def _plane(seed=4, ny=7, nx=9):
    rng = np.random.default_rng(seed)
    v = rng.normal(0.3, 1.0, (ny, nx))
    area = rng.uniform(1.0, 3.0, (ny, nx))
    v[1, 2] = np.nan
    v[5, 8] = np.nan
    area[3, 4] = np.nan
    area[0, 0] = 0.0
    area[4:6, 0:2] = 0.0
    return v, area


@pytest.mark.parametrize("periodic", (True, False))
@pytest.mark.parametrize("table", (False, True))
def test_the_restatement_against_a_direct_2d_convolution(periodic, table):
    """a tolerance, not bits: the direct form adds the n = Wx * Wy = 15 terms of a cell in one sum.
    In either form a term carries 3 roundings and passes through fewer than n adds, so with
    u = 2^-53 num is within (n + 3) u S of its exact value, S the sum of the terms' magnitudes, and
    den (positive weights) within (n + 3) u den.  The two quotients therefore differ by at most
    2 (n + 3) u S / den from the errors of the two nums, as much again from the two dens
    (|num| <= S), and one rounding of each division."""
    v, area = _plane()
    rng = np.random.default_rng(9)
    wy = np.array([0.25, 0.5, 0.25])
    wx = rng.uniform(0.5, 1.5, (7, 5)) if table else np.array([0.1, 0.2, 0.4, 0.2, 0.1])
    got = sn.plane_smooth(v[None], area, wx, wy, 2, 1, periodic, 1, fill=True)[0]
    want = sn.direct_2d(v, area, wx, wy, 2, 1, periodic)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and not np.isnan(want).all()
    a = np.where(np.isnan(area) | ~(area > 0), 0.0, area)
    scale = sn.direct_2d(np.where(np.isnan(v), np.nan, np.abs(v)), area, wx, wy, 2, 1, periodic)
    m = ~np.isnan(want)
    bound = 4 * (15 + 3) * 2.0 ** -53 * scale[m] + 2.0 ** -52 * np.abs(want[m])  # scale = S / den
    err = np.abs(got[m] - want[m])
    print(f"max |separable - direct| / bound = {np.max(err / bound):.3f}")
    assert (err <= bound).all() and a.sum() > 0
    # a record of ones is exactly 1.0 wherever it is not NaN
    ones = sn.plane_smooth(np.where(np.isnan(v), np.nan, 1.0)[None], area, wx, wy, 2, 1, periodic, 1)
    assert set(np.unique(ones[~np.isnan(ones)])) == {1.0}
    # without fill the invalid centres are NaN and nothing else changes
    nofill = sn.plane_smooth(v[None], area, wx, wy, 2, 1, periodic, 1)[0]
    centre = ~np.isnan(v) & (a > 0)
    assert np.isnan(nofill[~centre]).all()
    assert np.array_equal(nofill[centre].view(np.int64), got[centre].view(np.int64))
    # residual + smooth is the record, to the bit, where both are valid
    high = sn.plane_smooth(v[None], area, wx, wy, 2, 1, periodic, 1, residual=True)[0]
    both = ~np.isnan(high)
    assert both.any() and np.array_equal(both, ~np.isnan(nofill))
    assert np.array_equal(high[both], v[both] - nofill[both])


def test_the_restatement_on_a_hand_computed_plane():
    v = np.array([[[1.0, 2.0, np.nan, 4.0], [8.0, 16.0, 32.0, 64.0]]])
    area = np.array([[1.0, 1.0, 1.0, 2.0], [0.0, 1.0, 1.0, 1.0]])
    box = [1.0, 1.0, 1.0]
    s = sn.plane_smooth(v, area, box, [1.0], 1, 0, False, 1, fill=True)[0]
    assert s[0].tolist() == [1.5, 1.5, (2.0 + 8.0) / 3.0, 4.0]
    assert s[1].tolist() == [16.0, 24.0, 112.0 / 3.0, 48.0]
    p = sn.plane_smooth(v, area, box, [1.0], 1, 0, True, 1, fill=True)[0]
    assert p[0].tolist() == [(8.0 + 1.0 + 2.0) / 4.0, 1.5, (2.0 + 8.0) / 3.0, (8.0 + 1.0) / 3.0]
    c = sn.plane_smooth(v, area, box, [1.0], 1, 0, False, 3)[0]
    assert np.isnan(c[0]).tolist() == [True, True, True, True]
    assert np.isnan(c[1]).tolist() == [True, True, False, True]
    y = sn.plane_smooth(v, area, [1.0], [1.0, 1.0], 0, 0, False, 1)[0]  # rows j, j + 1
    assert y[0].tolist()[1] == 9.0 and y[1].tolist()[1:] == [16.0, 32.0, 64.0]
    assert np.isnan(y[1, 0]) and np.isnan(y[0, 2])
    r32 = sn.plane_smooth(v.astype(np.float32), area, box, [1.0], 1, 0, False, 1, out_dtype=np.float32)
    assert r32.dtype == np.float32
    assert sn.plane_smooth(v.astype(np.float32), area, box, [1.0], 1, 0, False, 1).dtype == np.float64
