"""CPU: the host side of the tide-gauge feature -- the numpy restatement against the reference's
NWA12 goldens, the C ABI of include/momlevel_gauge.h (symbols, binding table, argument errors), the
gauge table parser and the argument checks of extract_tidegauge.  No kernel runs here.

The fixtures hold the NWA12 grid, the 117 US gauges and the 16 rows of the reference's
geolocate_points_reference.csv.  The reference's tests/test_tidegauge.py sums (ssh_max of
NWA12_sample_grid_data.nc) are NOT pinned: that file is netCDF-4 / HDF5 and nothing that reads it
is installed where the fixtures are made (tests/golden/make_tidegauge_golden.py)."""

import ctypes
import importlib
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import gauge_numpy as gn
from momlevel_amd import _lib, test_data, tidegauge, util
from test_static_names import _undefined

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "momlevel_gauge.h")


# ---- the numpy restatement reproduces the reference ---------------------------------------------
def test_restatement_reproduces_the_reference_on_nwa12():
    grid, gold = gn.nwa12()
    assert grid["geolat"].shape == grid["geolon"].shape == grid["mask"].shape == (146, 100)
    assert grid["mask"].dtype == np.uint8 and int(grid["mask"].sum()) == 8509
    assert len(gold["gauges"]["name"]) == 117 and len(gold["reference"]["name"]) == 16
    got = gn.locate(grid["geolat"], grid["geolon"], gold["gauges"]["lat"], gold["gauges"]["lon"],
                    grid["mask"], threshold=gold["threshold"], rad_earth=gold["rad_earth"])
    assert [gold["gauges"]["name"][i] for i in got["which"]] == gold["reference"]["name"]
    assert np.array_equal(got["mod_index"], gold["reference"]["mod_index"])
    ref = np.array(gold["reference"]["distance"])
    rel = np.max(np.abs(got["distance"] - ref) / ref)
    print("restatement vs reference CSV, max relative distance difference:", rel)
    assert rel <= 1e-4  # the reference's own rtol (tests/test_util.py:231); the CSV is rounded


def test_restatement_rules():
    lat = np.array([[0.0, 0.0, 10.0], [0.0, np.nan, 10.0]])
    lon = np.array([[0.0, 0.0, 5.0], [0.0, 3.0, 5.0]])
    mask = np.array([[0.0, 1.0, 1.0], [1.0, 1.0, np.nan]])
    idx, ang, _ = gn.nearest(lat, lon, [0.0, 10.0], [0.0, 5.0], mask)
    assert idx.tolist() == [1, 2] and ang.tolist() == [0.0, 0.0]  # duplicates: the lowest valid index
    got = gn.locate(lat, lon, [0.0, 10.0], [0.0, 5.0], mask)
    assert got["mod_index"].tolist() == [0, 1]
    none = gn.locate(lat, lon, [0.0], [0.0], np.zeros((2, 3)))
    assert none["which"].size == 0


# ---- the C ABI ----------------------------------------------------------------------------------
def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_gauge_header_binding_and_exports_agree():
    text = _header_text()
    declared = sorted(set(re.findall(r"\b(mlx_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.GAUGE_SIGNATURES)
    assert all(name.startswith("mlx_gauge_") for name in declared)
    assert {"mlx_gauge_prepare", "mlx_gauge_nearest", "mlx_gauge_gather"} <= set(declared)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in momlevel_gauge.h but not exported"
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                             text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(mlx_gauge_[a-z0-9_]+)\b", out))) == declared
        # the pinned prefixes of the other headers have not grown
        assert len(set(re.findall(r"\b(mlx_time_[a-z0-9_]+)\b", out))) == 4
        assert sorted(set(re.findall(r"\b(mlx_clim_[a-z0-9_]+)\b", out))) == ["mlx_clim_group_stat"]
    # every prototype, argument for argument
    ctype = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p,
             "const double *": ctypes.c_void_p, "double *": ctypes.c_void_p,
             "const int64_t *": ctypes.c_void_p, "int64_t *": ctypes.c_void_p,
             "uint8_t *": ctypes.c_void_p, "int64_t ": ctypes.c_int64, "size_t ": ctypes.c_size_t,
             "int ": ctypes.c_int}
    rtype = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}
    protos = re.findall(r"\b(int|int64_t|size_t)\s+(mlx_gauge_[a-z_]+)\s*\(([^)]*)\)", text)
    assert sorted(p[1] for p in protos) == declared
    for ret, name, args in protos:
        args = [" ".join(a.split()) for a in args.split(",")]
        want = [next(v for k, v in ctype.items() if a.startswith(k)) for a in args]
        restype, argtypes = _lib.GAUGE_SIGNATURES[name]
        assert restype is rtype[ret] and argtypes == want, name
    consts = dict(re.findall(r"#define (MLX_GAUGE_[A-Z0-9_]+)\s+\(?(-?\d+)\)?", open(HEADER).read()))
    assert list(consts) == ["MLX_GAUGE_ROW_X", "MLX_GAUGE_ROW_Y", "MLX_GAUGE_ROW_Z",
                            "MLX_GAUGE_ROW_PHI", "MLX_GAUGE_ROW_LAM", "MLX_GAUGE_ROWS"]
    for name, val in consts.items():
        assert getattr(_lib, name[4:]) == int(val), name
    assert _lib.load_gauge() is _lib.load()


def test_other_tables_and_the_abi_version_are_untouched():
    for name in _lib.GAUGE_SIGNATURES:
        assert name not in _lib.SIGNATURES and name not in _lib.TREND_SIGNATURES
        assert name not in _lib.CLIM_SIGNATURES
    assert len(_lib.SIGNATURES) == 28 and len(_lib.TREND_SIGNATURES) == 4
    assert list(_lib.CLIM_SIGNATURES) == ["mlx_clim_group_stat"]
    assert _lib.ABI_VERSION == 9 and _lib.load().mlx_version() == 9


def test_argument_errors_need_no_gpu():
    lib = _lib.load_gauge()
    f = 1 << 20  # 16-byte aligned, non-NULL, never dereferenced: the checks precede every HIP call
    F64, F32 = _lib.DTYPE_F64, _lib.DTYPE_F32

    def prepare(lat=f, lon=f, dtype=F64, mask=None, mdtype=F64, n=10, table=f, valid=f):
        return lib.mlx_gauge_prepare(lat, lon, dtype, mask, mdtype, n, table, valid, None)

    for kw in (dict(lat=None), dict(lon=None), dict(table=None), dict(valid=None)):
        assert prepare(**kw) == -1 and "NULL" in _lib.last_error()
    for kw in (dict(n=0), dict(n=-4), dict(n=(1 << 38) + 1)):
        assert prepare(**kw) == -2 and _lib.last_error()
    assert prepare(dtype=7) == -3 and prepare(dtype=_lib.DTYPE_F32_UPCAST) == -3
    assert prepare(mask=f, mdtype=5) == -3
    assert prepare(lat=f + 4) == -5 and prepare(lon=f + 2, dtype=F32) == -5
    assert prepare(mask=f + 4) == -5 and prepare(table=f + 4) == -5

    def nearest(points=f, n=100, gauges=f, ng=3, split=0, index=f, angle=f, ws=f, nbytes=1 << 30):
        return lib.mlx_gauge_nearest(points, n, gauges, ng, split, index, angle, ws, nbytes, None)

    for kw in (dict(points=None), dict(gauges=None), dict(index=None), dict(angle=None), dict(ws=None)):
        assert nearest(**kw) == -1 and "NULL" in _lib.last_error()
    for kw in (dict(n=0), dict(ng=0), dict(n=-1), dict(ng=-1), dict(split=-1), dict(ng=1 << 31),
               dict(n=(1 << 38) + 1)):
        assert nearest(**kw) == -2 and _lib.last_error()
    assert nearest(points=f + 4) == -5 and nearest(index=f + 4) == -5 and nearest(angle=f + 2) == -5
    assert nearest(nbytes=3 * 16 - 1) == -4 and nearest(ws=f + 8) == -4
    assert "workspace" in _lib.last_error()
    assert nearest(split=7, nbytes=7 * 3 * 16 - 1) == -4

    # the cut of the points: what was asked for, within [1, min(n, 65535)]; sizes follow
    assert lib.mlx_gauge_nearest_split(100, 3, 0) == 1
    assert lib.mlx_gauge_nearest_split(100, 3, 4) == 4 and lib.mlx_gauge_nearest_split(100, 3, 1) == 1
    assert lib.mlx_gauge_nearest_split(100, 3, 1000) == 100
    assert 1 < lib.mlx_gauge_nearest_split(1080 * 1440, 1500, 0) <= 65535
    assert lib.mlx_gauge_nearest_split(1 << 30, 1, 1 << 20) <= 65535
    assert lib.mlx_gauge_nearest_split(0, 3, 0) == 0 and lib.mlx_gauge_nearest_split(5, 0, 0) == 0
    assert lib.mlx_gauge_nearest_workspace_bytes(100, 3, 4) == 4 * 3 * 16
    assert lib.mlx_gauge_nearest_workspace_bytes(0, 3, 0) == 0

    def gather(y=f, dtype=F64, index=f, nrest=7, n=100, ng=3, out=f):
        return lib.mlx_gauge_gather(y, dtype, index, nrest, n, ng, out, None)

    for kw in (dict(y=None), dict(index=None), dict(out=None)):
        assert gather(**kw) == -1 and "NULL" in _lib.last_error()
    for kw in (dict(nrest=0), dict(n=0), dict(ng=0), dict(nrest=-1), dict(n=-5), dict(ng=-2),
               dict(nrest=1 << 31), dict(ng=1 << 31), dict(n=(1 << 38) + 1),
               dict(nrest=(1 << 31) - 1, n=1 << 38)):
        assert gather(**kw) == -2 and _lib.last_error()
    assert gather(dtype=9) == -3 and gather(dtype=_lib.DTYPE_F32_UPCAST) == -3
    assert gather(y=f + 4) == -5 and gather(y=f + 2, dtype=F32) == -5 and gather(out=f + 4) == -5
    assert gather(index=f + 4) == -5


def test_a_library_without_the_kernels_is_an_error(monkeypatch):
    class Bare:
        def __getattr__(self, name):
            raise AttributeError(name)

    monkeypatch.setattr(_lib, "_gauge_bound", False)
    monkeypatch.setattr(_lib, "load", lambda: Bare())
    with pytest.raises(_lib.MomlevelHipError, match="does not export mlx_gauge_"):
        _lib.load_gauge()


def test_gauge_source_sha_is_its_own():
    from momlevel_amd.csrc import build

    assert len(build.gauge_source_sha()) == 16
    assert build.gauge_source_sha() not in (build.source_sha(), build.trend_source_sha(),
                                            build.clim_source_sha(), build.strat_source_sha())
    names = {os.path.basename(p) for p in build.TIMED_SOURCES}
    assert "momlevel_gauge.hip" not in names and "momlevel_gauge.h" not in names
    assert any(p.endswith("momlevel_gauge.hip") for p in build.SOURCES)
    assert any(p.endswith("momlevel_gauge.h") for p in build.DEPENDS)


def test_exports():
    import momlevel_amd

    assert momlevel_amd.tidegauge is tidegauge and "tidegauge" in momlevel_amd.__all__
    assert "extract_tidegauge" in tidegauge.__all__ and "locate" in tidegauge.__all__
    for name in ("geolocate_points", "tile_nominal_coords", "validate_tidegauge_data"):
        assert name in util.__all__ and callable(getattr(util, name))
    assert _undefined(importlib.import_module("momlevel_amd.tidegauge")) == []
    assert _undefined(importlib.import_module("momlevel_amd.util")) == []
    assert _undefined(importlib.import_module("momlevel_amd.core")) == []


# ---- the gauge table ------------------------------------------------------------------------------
def test_csv_parsing(tmp_path):
    path = tmp_path / "gauges.csv"
    path.write_text("Country,PSMSL_site,PSMSLID,lat,lon\n"
                    "United States,\"KEY WEST, FL\",188,24.55,-81.81\n"
                    "Canada,HALIFAX,96,44.67,-63.58\n\n")
    table = tidegauge.read_gauge_table(str(path))
    assert list(table) == ["Country", "name", "PSMSLID", "lat", "lon"]  # PSMSL_site -> name
    assert table["name"] == ["KEY WEST, FL", "HALIFAX"] and table["PSMSLID"] == [188, 96]
    assert table["lat"] == [24.55, 44.67] and table["lon"] == [-81.81, -63.58]
    assert tidegauge.read_gauge_table(path)["name"] == table["name"]  # a path-like works too
    for broken in ("name,lat\nA,1.0\n", "site,lat,lon\nA,1.0,2.0\n", "name,lon\nA,2.0\n"):
        path.write_text(broken)
        with pytest.raises(KeyError, match="lacks the columns"):
            tidegauge.read_gauge_table(str(path))
    with pytest.raises(AssertionError):
        tidegauge.read_gauge_table(str(tmp_path / "absent.csv"))
    # in-memory tables: a mapping, and anything frame-like (columns + item access)
    mapping = {"PSMSL_site": ("A", "B"), "lat": np.array([1.0, 2.0]), "lon": [3.0, 4.0]}
    assert tidegauge.read_gauge_table(mapping) == {"name": ["A", "B"], "lat": [1.0, 2.0],
                                                   "lon": [3.0, 4.0]}
    with pytest.raises(KeyError):
        tidegauge.read_gauge_table({"name": ["A"], "lat": [1.0]})
    with pytest.raises(ValueError, match="differ in length"):
        tidegauge.read_gauge_table({"name": ["A"], "lat": [1.0], "lon": [1.0, 2.0]})

    class Frame:
        columns = ["name", "lat", "lon"]

        def __getitem__(self, key):
            return {"name": ["X"], "lat": [5.0], "lon": [6.0]}[key]

    assert tidegauge.read_gauge_table(Frame()) == {"name": ["X"], "lat": [5.0], "lon": [6.0]}


def test_bundled_tables_are_not_shipped():
    for name in ("us", "global"):
        with pytest.raises(FileNotFoundError, match="pass the path"):
            tidegauge.read_gauge_table(name)
    dset = test_data.generate_test_data()
    with pytest.raises(FileNotFoundError, match="not shipped"):
        tidegauge.extract_tidegauge(dset.thetao, xcoord=dset.geolon, ycoord=dset.geolat)


# ---- validate_tidegauge_data: the cases of the reference's tests/test_util.py:167-207 -----------
def test_validate_tidegauge_data_cases():
    dset = test_data.generate_test_data()
    util.validate_tidegauge_data(dset.thetao, "xh", "yh", None)                        # 1
    with pytest.raises(AssertionError):
        util.validate_tidegauge_data(dset, "xh", "yh", None)                           # 2
    with pytest.raises(AssertionError, match="`geolon` not found in input array"):
        util.validate_tidegauge_data(dset.thetao, "geolon", "geolat", None)            # 3
    util.validate_tidegauge_data(dset.thetao, dset.geolon, dset.geolat, None)          # 4
    with pytest.raises(AssertionError, match="ycoord must either be"):
        util.validate_tidegauge_data(dset.thetao, dset.geolon, np.array(dset.geolat), None)  # 5
    util.validate_tidegauge_data(dset.thetao, dset.geolon, dset.geolat, dset.areacello * 0.0)  # 6
    with pytest.raises(AssertionError, match="mask be a DataArray"):
        util.validate_tidegauge_data(dset.thetao, dset.geolon, dset.geolat, "wet")     # 7
    # extract_tidegauge runs the same checks before anything else
    with pytest.raises(AssertionError, match="not found in input array"):
        tidegauge.extract_tidegauge(dset.thetao, csv={"name": [], "lat": [], "lon": []})


def test_tile_nominal_coords():
    dset = test_data.generate_test_data()
    with pytest.warns(UserWarning, match="Constructing coordinates from 1-D vectors"):
        lon2d, lat2d = util.tile_nominal_coords(dset.xh, dset.yh)
    assert lon2d.sum().values == lat2d.sum().values
    assert np.allclose(lon2d.sum().values, 75.0)  # the reference's tests/test_util.py:210-213
    assert lon2d.dims == lat2d.dims == ("yh", "xh") and lon2d.name == "geolon" and lat2d.name == "geolat"
    assert np.array_equal(lon2d.values[0], dset.xh.values) and np.array_equal(lat2d.values[:, 0], dset.yh.values)
    assert set(lon2d.coords) == {"yh", "xh"}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        util.tile_nominal_coords(dset.xh, dset.yh, warn=False)
    with pytest.raises(AssertionError):
        util.tile_nominal_coords(np.arange(3.0), dset.yh)


def test_located_grid_positions():
    loc = tidegauge.Located(np.array([0, 2]), np.array([1.0, 2.0]), np.array([7, 205]), (3, 100),
                            np.array([5, 150]), (np.zeros(2), np.zeros(2)), np.array([7, -1, 205]),
                            np.array([1.0, np.nan, 2.0]))
    assert len(loc) == 2 and loc.iy.tolist() == [0, 2] and loc.ix.tolist() == [7, 5]
    flat = tidegauge.Located(np.array([0]), np.array([1.0]), np.array([7]), (300,), np.array([5]),
                             (np.zeros(1), np.zeros(1)), np.array([7]), np.array([1.0]))
    assert flat.iy.tolist() == [0] and flat.ix.tolist() == [7]


# ---- the helpers of tests/test_gpu_tidegauge_edges.py ---------------------------------------------
LATTICE_NS = (1, 255, 256, 257, 511, 513, 1024, 1025, 2337, 40 * 64)


@pytest.mark.parametrize("edges_valid", (True, False))
@pytest.mark.parametrize("kind", ("U", "D"))
def test_lattice_helper_agrees_with_a_float64_argmin(kind, edges_valid):
    for n in LATTICE_NS:
        pq, pok = gn.lattice_points(n, kind, edges_valid)
        gq, gok = gn.lattice_gauges(n, kind)
        assert np.array_equal(np.sort(pq // 4), np.arange(n) if kind == "U" else np.arange(n) // 2)
        edges = [i for i in gn.LATTICE_EDGES + (n - 1,) if i < n]
        assert np.all(pok[edges] == edges_valid) and int((~gok).sum()) == 3
        if n >= 255:
            assert 0.03 * n < (~pok).sum() < 0.2 * n
        points, gauges = gn.lattice_table(pq, pok), gn.lattice_table(gq, gok)
        assert points.shape == (5, n) and gauges.shape == (5, gq.size)
        bad = points[:, ~pok]
        assert np.all(bad[:3] == np.inf) and np.isnan(bad[3:]).all() and not points[1:, pok].any()
        want = gn.lattice_nearest(pq, pok, gq, gok)
        # float64, as the search computes it: the squared chord, numpy's first minimum
        with np.errstate(invalid="ignore"):
            d = (gauges[0][:, None] - points[0][None, :]) ** 2
        d[:, ~pok] = np.inf
        got = np.where(gok & pok.any(), np.argmin(np.where(np.isnan(d), np.inf, d), axis=1), -1)
        assert np.array_equal(got, want), (n, kind)
        assert np.all(pok[want[want >= 0]]) and np.array_equal(want < 0, ~gok | ~pok.any())
        if kind == "U":  # every valid point is the winner of the gauge on its own value
            assert np.array_equal(np.unique(want[want >= 0]), np.nonzero(pok)[0])
            mine = np.nonzero(pok)[0]
            assert np.array_equal(want[gok][pq[mine] // 4], mine)
        else:  # v + 0.5 ties across two values, v and v + 0.25 across the two copies of one
            tied = (d == d.min(axis=1)[:, None]).sum(axis=1)
            assert n < 255 or (tied[gok] == 4).any() and (tied[gok] == 2).any()


def test_stacked_rows_and_their_expected_winners():
    for copies in (20, 40):
        lat, lon, mask, wet = gn.stacked_rows(copies)
        m = 70
        assert lat.shape == lon.shape == mask.shape == (copies, m) and len(wet) == m
        assert np.array_equal(lat, np.tile(lat[0], (copies, 1))) and len(set(lat[0])) == m
        sets = set(wet)
        assert set(gn.TIE_SETS) <= sets and (copies - 1,) in sets and () in sets
        assert (set(gn.TIE_SETS_40) <= sets) == (copies == 40)
        assert wet.count(()) == 1 and wet[gn.TIE_DRY_COLUMN] == ()
        for c, s in enumerate(wet):
            assert np.array_equal(np.nonzero(mask[:, c])[0], sorted(s))
        # a candidate of a later part meets one of an earlier part in a lower lane of the 16
        assert any(max(s) >= 16 and min(s) % 16 > max(s) % 16 for s in sets if s)
        for dlat, dlon in ((0.0, 0.0), (0.01, -0.01)):
            index, _angle, _gap = gn.nearest(lat, lon, lat[0] + dlat, lon[0] + dlon, mask)
            direct = np.array([min(s) * m + c if s else -1 for c, s in enumerate(wet)])
            assert np.array_equal(index[direct >= 0], direct[direct >= 0])
            dry = gn.TIE_DRY_COLUMN
            assert index[dry] % m in (dry - 1, dry + 1) and index[dry] // m == min(wet[index[dry] % m])
            one_row = (mask.sum(axis=0) > 0).astype(np.float64)
            _i, _a, gap = gn.nearest(lat[0], lon[0], lat[0, dry] + dlat, lon[0, dry] + dlon, one_row)
            assert gap[0] >= 1e-9


def test_the_real_coordinate_cases_exclude_no_gauge():
    lat, lon, mask, _glat, _glon = gn.synthetic_grid(41, 57, 1, 11)
    dry = mask.reshape(-1) == 0.0
    assert lat.size == 2337 and int(dry.sum()) == 709
    index, angle, gap = gn.nearest(lat, lon, lat, lon, mask)
    assert np.array_equal(index[~dry], np.nonzero(~dry)[0]) and np.all(angle[~dry] == 0.0)
    assert not np.any(index[dry] == np.nonzero(dry)[0])
    print("41x57, dry gauges: smallest relative gap", gap[dry].min())
    assert gap.min() >= 1e-9 and 1.2e-4 < gap[dry].min() < 1.3e-4
    lat2, _lon2, mask2, glat, glon = gn.synthetic_grid(41, 57, 513, 11)
    assert np.array_equal(lat2, lat) and np.array_equal(mask2, mask)  # the gauges are drawn last
    _i, _a, gap = gn.nearest(lat, lon, glat, glon, mask)
    print("41x57, 513 gauges: smallest relative gap", gap.min())
    assert gap.min() >= 1e-9
    lib = _lib.load_gauge()
    for ny, nx in ((257, 510), (257, 511)):
        lat, lon, mask, glat, glon = gn.synthetic_grid(ny, nx, 5, 5)
        _i, _a, gap = gn.nearest(lat, lon, glat, glon, mask)
        print(f"{ny}x{nx}, 5 gauges: smallest relative gap", gap.min())
        assert gap.min() >= 1e-9
        n = ny * nx
        assert 16 < lib.mlx_gauge_nearest_split(n, 5, n) <= 65535
        assert 16 < lib.mlx_gauge_nearest_split(n, 5, 0) <= 65535
    assert lib.mlx_gauge_nearest_split(131070, 5, 131070) == 65535
    assert lib.mlx_gauge_nearest_split(131070, 5, 65536) == 65535


def test_antipodes_round_above_one_in_numpy():
    lat, lon, glat, glon = gn.antipodes(0.25)
    assert lat.size == 721 and lat[0] == -90.0 and lat[360] == 0.0 and lat[-1] == 90.0
    assert np.array_equal(glat, -lat) and np.all(glon - lon == 180.0)
    args = np.deg2rad([glat, glon, lat, lon])
    h = gn.haversine_h(*args)
    print("h > 1 at", int((h > 1.0).sum()), "of 721; largest h - 1:", float(h.max() - 1.0))
    assert (h > 1.0).sum() >= 3
    with np.errstate(invalid="ignore"):
        angle = gn.haversine(*args)
    short = np.pi - angle[~np.isnan(angle)]
    print("numpy's own pi - angle reaches", float(short.max()))
    assert short.max() <= 2.0 * np.sqrt(2.0 * 16 * 2.0 ** -53)  # the GPU test's bound holds for numpy
