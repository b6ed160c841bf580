"""CPU: the C ABI of include/momlevel_area.h (symbols, binding table, argument errors), the region
planning of momlevel_amd.regional as pure functions, and its labelled layer (dims, coords, attrs,
refusals) with the device pass replaced by the numpy restatement (tests/area_numpy.py).  No GPU."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import area_numpy as an
import momlevel_amd
from momlevel_amd import _lib, core, regional
from momlevel_amd.labeled import DataArray, Dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "momlevel_area.h")
NAMES = ["mlx_area_anomaly", "mlx_area_mean", "mlx_area_mean_workspace_bytes", "mlx_area_tile"]


# ---- the C ABI ----------------------------------------------------------------------------------
def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_area_header_binding_and_exports_agree():
    text = _header_text()
    declared = sorted(set(re.findall(r"\b(mlx_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.AREA_SIGNATURES) == NAMES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in momlevel_area.h but not exported"
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                             text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(mlx_area_[a-z0-9_]+)\b", out))) == declared
    ctype = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p,
             "const int32_t *": ctypes.c_void_p, "const double *": ctypes.c_void_p,
             "double *": ctypes.c_void_p, "int64_t ": ctypes.c_int64, "size_t ": ctypes.c_size_t,
             "int ": ctypes.c_int}
    rtype = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}
    protos = re.findall(r"\b(int|int64_t|size_t)\s+(mlx_area_[a-z_]+)\s*\(([^)]*)\)", text)
    assert sorted(p[1] for p in protos) == declared
    for ret, name, args in protos:
        args = [" ".join(a.split()) for a in args.split(",")]
        want = [next(v for k, v in ctype.items() if a.startswith(k)) for a in args]
        restype, argtypes = _lib.AREA_SIGNATURES[name]
        assert restype is rtype[ret] and argtypes == want, name
        if ret == "int":
            assert args[-1] == "void *stream", name  # the caller's stream last
    for name, val in re.findall(r"#define MLX_(AREA_[A-Z_]+)\s+(\d+)", text):
        assert getattr(_lib, name) == int(val), name
    assert _lib.AREA_MAX_SLOTS >= 16 and core.AREA_MAX_SLOTS == _lib.AREA_MAX_SLOTS
    assert core.AREA_WINDOW == _lib.AREA_WINDOW >= 1
    assert _lib.load_area() is _lib.load()


def test_other_tables_and_the_abi_version_are_untouched():
    for name in _lib.AREA_SIGNATURES:
        for table in (_lib.SIGNATURES, _lib.TREND_SIGNATURES, _lib.CLIM_SIGNATURES,
                      _lib.GAUGE_SIGNATURES, _lib.SPICE_SIGNATURES, _lib.VORT_SIGNATURES):
            assert name not in table
    assert len(_lib.SIGNATURES) == 28 and len(_lib.VORT_SIGNATURES) == 5
    assert _lib.ABI_VERSION == 9 and _lib.load().mlx_version() == 9


def test_the_tile_is_a_function_of_the_record_dtype():
    lib = _lib.load_area()
    t64, t32 = core.area_tile(np.float64), core.area_tile(np.float32)
    assert t64 == lib.mlx_area_tile(_lib.DTYPE_F64) > 0 and t32 == lib.mlx_area_tile(_lib.DTYPE_F32) > 0
    assert t64 % 512 == 0 and t32 % 1024 == 0  # whole 16-byte packs for each of 256 threads
    for bad in (2, 3, 4, 7, -1):
        assert lib.mlx_area_tile(bad) == 0
    with pytest.raises(TypeError):
        core.area_tile(np.float16)
    # 16 bytes per (record, tile, slot); 0 for what the call refuses
    ws = lib.mlx_area_mean_workspace_bytes
    F64, F32 = _lib.DTYPE_F64, _lib.DTYPE_F32
    assert ws(3, t64 + 1, 5, F64) == 3 * 2 * 5 * 16 and ws(3, t64, 5, F64) == 3 * 5 * 16
    assert ws(3, t64 + 1, 5, F32) == 3 * 5 * 16 and ws(0, 10, 1, F64) == 0 and ws(2, 0, 1, F64) == 0
    for bad in ((-1, 4, 1, F64), (1, -4, 1, F64), (1, 4, 0, F64), (1, 4, _lib.AREA_MAX_SLOTS + 1, F64),
                (1, 4, 1, 2), (1 << 20, 1 << 20, 1, F64)):
        assert ws(*bad) == 0, bad


def test_argument_errors_need_no_gpu():
    lib = _lib.load_area()
    f = 1 << 20  # 16-byte aligned, non-NULL, never dereferenced: the checks precede every HIP call
    F64, F32 = _lib.DTYPE_F64, _lib.DTYPE_F32
    big = 1 << 40

    def mean(v=f, vdt=F64, area=f, adt=F64, slot=f, nslots=3, nrec=2, plane=10, out=f, wsum=f,
             ws=f, nbytes=big):
        return lib.mlx_area_mean(v, vdt, area, adt, slot, nslots, nrec, plane, out, wsum, ws, nbytes, None)

    def anom(v=f, vdt=F64, slot=f, nslots=3, m=f, nrec=2, plane=10, out=f):
        return lib.mlx_area_anomaly(v, vdt, slot, nslots, m, nrec, plane, out, None)

    for kw in (dict(v=None), dict(area=None), dict(out=None), dict(ws=None)):
        assert mean(**kw) == -1 and "NULL" in _lib.last_error(), kw
    assert mean(wsum=None, ws=None) == -1  # (wsum alone may be NULL: it is optional)
    for kw in (dict(v=None), dict(m=None), dict(out=None)):
        assert anom(**kw) == -1 and "NULL" in _lib.last_error(), kw
    for kw in (dict(nrec=-1), dict(plane=-1), dict(nslots=0), dict(nslots=-2),
               dict(nslots=_lib.AREA_MAX_SLOTS + 1), dict(slot=None), dict(nrec=1 << 20, plane=(1 << 18) + 1),
               dict(plane=1 << 39), dict(nrec=(1 << 26) + 1, plane=1)):
        assert mean(**kw) == -2 and _lib.last_error(), kw
    assert mean(slot=None, nslots=2) == -2 and "one region" in _lib.last_error()
    for kw in (dict(nrec=-1), dict(plane=-1), dict(nslots=0), dict(slot=None), dict(plane=1 << 39),
               dict(nslots=(1 << 24) + 1)):
        assert anom(**kw) == -2 and _lib.last_error(), kw
    assert anom(nslots=_lib.AREA_MAX_SLOTS + 1, nrec=0) == 0  # (no accumulators: not capped here)
    for bad in (2, 3, 4, 7, -1):  # (MLX_DTYPE_F32_UPCAST and the mixed codes are not operand dtypes)
        assert mean(vdt=bad) == -3 and mean(adt=bad) == -3 and anom(vdt=bad) == -3
        assert _lib.last_error()
    need = lib.mlx_area_mean_workspace_bytes(2, 10, 3, F64)
    assert need == 2 * 3 * 16
    assert mean(nbytes=need - 1) == -4 and "workspace" in _lib.last_error()
    assert mean(nbytes=0) == -4 and mean(ws=f + 4) == -4
    for kw in (dict(v=f + 4), dict(area=f + 4), dict(slot=f + 2), dict(out=f + 4), dict(wsum=f + 4),
               dict(v=f + 2, vdt=F32), dict(area=f + 1, adt=F32)):
        assert mean(**kw) == -5 and _lib.last_error(), kw
    for kw in (dict(v=f + 4), dict(slot=f + 1), dict(m=f + 4), dict(out=f + 4), dict(v=f + 2, vdt=F32)):
        assert anom(**kw) == -5 and _lib.last_error(), kw
    # float32 operands need their own alignment only
    assert mean(v=f + 4, vdt=F32, nrec=0) == 0
    # nothing to do: no launch, whatever the pointers
    assert mean(nrec=0) == 0 and mean(plane=0) == 0
    assert mean(v=None, area=None, out=None, ws=None, nbytes=0, nrec=0) == 0
    assert anom(nrec=0) == 0 and anom(v=None, m=None, out=None, plane=0) == 0


def test_a_library_without_the_kernels_is_an_error(monkeypatch):
    class Bare:
        def __getattr__(self, name):
            raise AttributeError(name)

    monkeypatch.setattr(_lib, "_area_bound", False)
    monkeypatch.setattr(_lib, "load", lambda: Bare())
    with pytest.raises(_lib.MomlevelHipError, match="does not export mlx_area_[a-z_]+: rebuild"):
        _lib.load_area()


def test_area_source_sha_is_its_own():
    from momlevel_amd.csrc import build

    assert len(build.area_source_sha()) == 16
    assert build.area_source_sha() not in (build.source_sha(), build.vort_source_sha(),
                                           build.spice_source_sha(), build.clim_source_sha())
    names = {os.path.basename(p) for p in build.TIMED_SOURCES}
    assert "momlevel_area.hip" not in names and "momlevel_area.h" not in names
    assert any(p.endswith("momlevel_area.hip") for p in build.SOURCES)
    assert any(p.endswith("momlevel_area.h") for p in build.DEPENDS)
    text = open(os.path.join(ROOT, "momlevel_amd", "csrc", "momlevel_area.hip")).read()
    assert "#pragma clang fp contract(off)" in text and "atomic" not in text.replace("atomics", "")
    assert "-ffp-contract=off" in build.FLAGS


# ---- region planning ------------------------------------------------------------------------------
def test_ids_from_the_map():
    lab = np.array([[7, 2, 2, 0], [-3, 1000, 7, 2]])
    ids, slot = regional.plan_regions(lab)
    assert ids.dtype == np.int64 and ids.tolist() == [2, 7, 1000]
    assert slot.dtype == np.int32 and slot.tolist() == [[1, 0, 0, -1], [-1, 2, 1, 0]]


def test_explicit_absent_and_duplicate_ids():
    lab = np.array([[7, 2, 2, 0], [-3, 1000, 7, 2]])
    ids, slot = regional.plan_regions(lab, [1000, 5, 2])  # (5 does not occur; 7 is left out)
    assert ids.tolist() == [1000, 5, 2]
    assert slot.tolist() == [[-1, 2, 2, -1], [-1, 0, -1, 2]]
    ids, slot = regional.plan_regions(lab, np.array([2.0]))  # (whole floats are ids too)
    assert ids.tolist() == [2] and (slot >= 0).sum() == 3
    ids, slot = regional.plan_regions(lab, [])
    assert ids.size == 0 and np.all(slot == -1)
    with pytest.raises(ValueError, match="duplicates"):
        regional.plan_regions(lab, [2, 7, 2])
    with pytest.raises(ValueError, match="positive"):
        regional.plan_regions(lab, [2, 0])
    with pytest.raises(ValueError, match="positive"):
        regional.plan_regions(lab, [-3])
    with pytest.raises(ValueError, match="integers"):
        regional.plan_regions(lab, [2.5])


def test_labels_without_a_region_and_float_maps():
    lab = np.array([[1.0, np.nan, 3.0], [0.0, -2.0, 3.0]])
    ids, slot = regional.plan_regions(lab)
    assert ids.tolist() == [1, 3] and slot.tolist() == [[0, -1, 1], [-1, -1, 1]]
    assert regional.region_labels(lab).dtype == np.int64
    assert regional.region_labels(lab.astype(np.float32)).tolist() == [[1, 0, 3], [0, -2, 3]]
    assert regional.region_labels(np.array([[True, False]])).tolist() == [[1, 0]]
    ids, slot = regional.plan_regions(np.full((2, 2), np.nan))
    assert ids.size == 0 and np.all(slot == -1)
    with pytest.raises(ValueError, match="whole numbers"):
        regional.plan_regions(np.array([[1.5, 2.0]]))
    with pytest.raises(ValueError, match="whole numbers"):
        regional.plan_regions(np.array([[np.inf, 2.0]]))
    with pytest.raises(TypeError):
        regional.plan_regions(np.array([["a", "b"]]))


def test_grouping_above_the_cap():
    cap = core.AREA_MAX_SLOTS
    assert regional.slot_groups(1) == [(0, 1)] and regional.slot_groups(cap) == [(0, cap)]
    assert regional.slot_groups(cap + 1) == [(0, cap), (cap, 1)]
    assert regional.slot_groups(0) == [] and regional.slot_groups(7, cap=3) == [(0, 3), (3, 3), (6, 1)]
    slot = np.array([[-1, 0, 1, 2], [3, 4, 5, 6]], dtype=np.int32)
    g = regional.group_slot_map(slot, 3, 3)
    assert g.dtype == np.int32 and g.tolist() == [[-1, -1, -1, -1], [0, 1, 2, -1]]
    # the launches partition the ids: every cell of a region is in exactly one of them
    seen = sum((regional.group_slot_map(slot, s, n) >= 0).astype(int) for s, n in regional.slot_groups(7, cap=3))
    assert seen.tolist() == [[0, 1, 1, 1], [1, 1, 1, 1]]


# ---- the labelled layer, the device pass replaced by the restatement -----------------------------
@pytest.fixture
def on_numpy(monkeypatch):
    def records(da, maps, want_anomaly):
        ydim, xdim = maps.dims
        regional.derived.check_trailing(da, ydim, xdim, da.name or "the record")
        v, area = da.values, maps.area.reshape(maps.shape)
        if maps.ids is None:
            mean, den = an.area_mean(v, area)
            anom = an.area_anomaly(v, mean) if want_anomaly else None
            return mean[..., None], den[..., None], anom
        label, ids = maps.slot.reshape(maps.shape), list(range(maps.nslots))
        mean, den = an.area_mean(v, area, label, ids)
        return mean, den, an.area_anomaly(v, mean, label, ids) if want_anomaly else None

    monkeypatch.setattr(regional, "_records", records)


def _record():
    rng = np.random.default_rng(5)
    time = DataArray(np.arange(3.0), ("time",), None, {"axis": "T"}, "time")
    yh = DataArray(np.arange(4.0), ("yh",), None, None, "yh")
    xh = DataArray(np.arange(5.0), ("xh",), None, None, "xh")
    eta = DataArray(rng.normal(size=(3, 4, 5)), ("time", "yh", "xh"), {"time": time, "yh": yh, "xh": xh},
                    {"long_name": "Steric sea level", "units": "m", "standard_name": "x"}, "steric")
    eta.values[:, 0, 0] = np.nan
    area = DataArray(rng.uniform(1.0, 2.0, (4, 5)), ("yh", "xh"), {"yh": yh, "xh": xh}, {"units": "m2"},
                     "areacello")
    basin = DataArray(np.array([[1, 1, 2, 2, 0]] * 4), ("yh", "xh"))
    return eta, area, basin


def test_dims_coords_and_attrs_of_the_mean(on_numpy):
    eta, area, basin = _record()
    m = regional.area_mean(eta, area)
    assert m.dims == ("time",) and m.name == "steric" and set(m.coords) == {"time"}
    assert m.attrs == {"long_name": "Area-weighted mean of Steric sea level", "units": "m",
                       "cell_methods": "area: mean"}
    ref, den = an.area_mean(eta.values, area.values)
    assert np.array_equal(m.values, ref) and m.values.dtype == np.float64
    m2, d = regional.area_mean(eta, area, return_area=True)
    assert np.array_equal(d.values, den) and d.dims == ("time",) and d.attrs["units"] == "m2"
    bare = regional.area_mean(DataArray(eta.values[0], ("yh", "xh")), area)
    assert bare.dims == () and bare.attrs == {"cell_methods": "area: mean"}
    r = regional.area_mean(eta, area, regions=basin)
    assert r.dims == ("time", "region") and r.coords["region"].values.tolist() == [1, 2]
    assert set(r.coords) == {"time", "region"}
    r = regional.area_mean(eta, area, regions=basin.values.astype(float), region_ids=[2, 9])
    assert r.values.shape == (3, 2) and r.coords["region"].values.tolist() == [2, 9]
    assert np.all(np.isnan(r.values[:, 1])) and np.all(np.isfinite(r.values[:, 0]))


def test_dims_coords_and_attrs_of_the_anomaly(on_numpy):
    eta, area, basin = _record()
    a, m = regional.area_anomaly(eta, area, regions=basin, return_mean=True)
    assert a.dims == eta.dims and set(a.coords) == {"time", "yh", "xh"} and a.name == "steric"
    assert a.attrs["units"] == "m" and a.attrs["long_name"].endswith("of Steric sea level")
    assert m.dims == ("time", "region")
    assert np.all(np.isnan(a.values[:, :, 4])) and np.isfinite(a.values[:, 1, 1]).all()
    assert regional.area_anomaly(eta, area).dims == eta.dims


def test_datasets(on_numpy):
    eta, area, basin = _record()
    d = Dataset(attrs={"title": "t"})
    d["steric"] = eta
    d["count"] = DataArray(np.arange(60).reshape(3, 4, 5), ("time", "yh", "xh"))
    d["series"] = DataArray(np.arange(3.0), ("time",))
    d["names"] = DataArray(np.array(["a", "b", "c"]), ("time",))
    d["steric"].encoding["dtype"] = "float32"
    m = regional.area_mean(d, area)
    assert sorted(m.keys()) == ["count", "steric"] and m.attrs == {"title": "t"}
    assert m["steric"].encoding == {"dtype": "float32"} and m["count"].values.dtype == np.float64
    assert "time" in m.coords and "yh" not in m.coords
    means, dens = regional.area_mean(d, area, regions=basin, return_area=True)
    assert means["steric"].dims == ("time", "region") and sorted(dens.keys()) == ["count", "steric"]
    a = regional.area_anomaly(d, area)
    assert sorted(a.keys()) == ["count", "series", "steric"] and a.attrs == {"title": "t"}
    assert np.array_equal(a["series"].values, d["series"].values) and "yh" in a.coords
    assert a["steric"].encoding == {"dtype": "float32"}
    with pytest.raises(TypeError):
        regional.area_mean(np.zeros((4, 5)), area)


def test_wrong_trailing_dims_raise():
    eta, area, basin = _record()
    swapped = DataArray(np.zeros((3, 5, 4)), ("time", "xh", "yh"))
    with pytest.raises(ValueError, match=r"has dims \('time', 'xh', 'yh'\): its last two must be \('yh', 'xh'\)"):
        regional.area_mean(swapped, area)
    with pytest.raises(ValueError, match=r"has dims \('yh', 'xh', 'time'\)"):
        regional.area_anomaly(DataArray(np.zeros((4, 5, 3)), ("yh", "xh", "time"), None, None, "eta"), area)
    with pytest.raises(ValueError, match="is not areacello's"):
        regional.area_mean(DataArray(np.zeros((3, 4, 6)), ("time", "yh", "xh")), area)
    with pytest.raises(ValueError, match="2-D"):
        regional.area_mean(eta, DataArray(np.ones((3, 4, 5)), ("time", "yh", "xh")))
    with pytest.raises(ValueError, match="regions has dims"):
        regional.area_mean(eta, area, regions=DataArray(basin.values.T.copy(), ("xh", "yh")))
    with pytest.raises(ValueError, match="does not cover"):
        regional.area_mean(eta, area, regions=np.ones((4, 6), int))
    with pytest.raises(ValueError, match="needs a regions map"):
        regional.area_mean(eta, area, region_ids=[1])
    with pytest.raises(ValueError, match="duplicates"):
        regional.area_mean(eta, area, regions=basin, region_ids=[1, 1])
    for bad in (np.float16, np.longdouble):
        with pytest.raises(TypeError):
            regional.area_mean(eta.astype(bad), area)
        with pytest.raises(TypeError):
            regional.area_mean(eta, area.astype(bad))


def test_negative_area_raises():
    eta, area, basin = _record()
    bad = area.copy()
    bad.values[2, 3] = -1.0
    with pytest.raises(ValueError, match="negative areas"):
        regional.area_mean(eta, bad)
    with pytest.raises(ValueError, match="negative areas"):
        regional.area_anomaly(eta, bad, regions=basin)
    nan = area.copy()
    nan.values[2, 3] = np.nan  # (NaN is no weight, not an error)
    regional._Maps(nan, None, None)


def test_the_module_is_published():
    assert momlevel_amd.regional is regional and "regional" in momlevel_amd.__all__
    assert regional.__all__ == ["area_anomaly", "area_mean"]
    assert "EXTENSION" in regional.area_mean.__doc__ and "unpinned" in regional.area_mean.__doc__
    assert "sum(mean * den) / sum(den)" in regional.area_mean.__doc__


def test_no_undefined_globals_in_the_new_module():
    from test_static_names import _undefined

    assert _undefined(regional) == []
