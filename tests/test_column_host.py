"""CPU: the numpy restatement tests/column_numpy.py against hand-computed columns and against an
independent spelling (np.interp), the C ABI of include/momlevel_column.h (symbols, binding table,
argument errors -- they precede every HIP call) and the refusals of derived.calc_mld /
calc_isosurface_depth / calc_isopycnal_depth.  No GPU."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import column_numpy as cn
from momlevel_amd import _lib, core, derived
from momlevel_amd.labeled import DataArray, Dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "momlevel_column.h")
NAMES = ["mlx_column_block_cells", "mlx_column_crossing", "mlx_column_record_rows"]
NAN = np.nan
Z = np.array([5.0, 15.0, 25.0, 35.0, 45.0])
UP = [1.0, 2.0, 4.0, 8.0, 16.0]
DOWN = [16.0, 8.0, 4.0, 2.0, 1.0]


def _one(x, targets, mode=cn.RISE, relative=False, miss=cn.MISS_NAN, kref=0, floor=None, z=None):
    """one record, one cell: the depths of ``targets`` (a list) in the column ``x``"""
    x = np.asarray(x, dtype=np.float64).reshape(1, -1, 1)
    z = Z[:x.shape[1]] if z is None else z
    floor = None if floor is None else np.array([floor])
    out = cn.column_crossing(x, z, kref, mode, relative, miss, targets, floor=floor)
    assert out.shape == (1, len(targets), 1) and out.dtype == np.float64
    return out[0, :, 0].tolist()


# ---- the restatement against columns computed by hand ---------------------------------------------
def test_each_mode_on_hand_computed_columns():
    # RISE, absolute: 2 -> 4 crosses 3 half way between 15 and 25; a value met exactly is its level
    assert _one(UP, [3.0, 2.0, 12.0]) == [20.0, 15.0, 40.0]
    # RISE, relative to level 1: 2 + 5 = 7, three quarters of the way from 4 to 8
    assert _one(UP, [5.0], relative=True, kref=1) == [32.5]
    # FALL, absolute and relative to level 0 (16 - 10 = 6)
    assert _one(DOWN, [3.0], mode=cn.FALL) == [30.0]
    assert _one(DOWN, [10.0], mode=cn.FALL, relative=True) == [20.0]
    # DEPART: either way from the reference value; the target is on the side the column left by
    assert _one([10.0, 10.25, 11.25, 9.0], [0.75], mode=cn.DEPART, relative=True) == [20.0]
    assert _one([10.0, 10.25, 9.25, 12.0], [0.5], mode=cn.DEPART, relative=True) == [22.5]
    # ... and the targets of one launch do not see each other
    assert _one(UP, [12.0, 3.0]) == [40.0, 20.0]


def test_step_1_land_is_nan_whatever_the_miss_policy():
    for miss in (cn.MISS_NAN, cn.MISS_FLOOR):
        got = _one([NAN, 2.0, 4.0, 8.0, 16.0], [3.0, 5.0], miss=miss, floor=99.0)
        assert np.isnan(got).all()
        assert np.isnan(_one([NAN] * 5, [3.0], miss=miss, kref=2)).all()


def test_step_2_a_column_shallower_than_the_reference_level_is_a_miss():
    col = [1.0, 2.0, NAN, NAN, NAN]
    assert np.isnan(_one(col, [0.5], relative=True, kref=2)).all()
    # FLOOR without a floor field: the deepest level with a value, counted from the surface
    assert _one(col, [0.5, 9.0], relative=True, kref=2, miss=cn.MISS_FLOOR) == [15.0, 15.0]
    assert _one([1.0, NAN, 3.0, NAN, NAN], [0.5], relative=True, kref=3, miss=cn.MISS_FLOOR) == [5.0]
    assert _one(col, [0.5], relative=True, kref=2, miss=cn.MISS_FLOOR, floor=17.5) == [17.5]


def test_step_4_an_outcrop_is_nan():
    for miss in (cn.MISS_NAN, cn.MISS_FLOOR):
        assert np.isnan(_one(UP, [0.5], miss=miss)).all()  # the surface is above 0.5 already
        assert np.isnan(_one(UP, [1.0], miss=miss)).all()  # ... or exactly on it
        assert np.isnan(_one(DOWN, [16.0], mode=cn.FALL, miss=miss)).all()
        assert np.isnan(_one(UP, [3.0], kref=2, miss=miss)).all()  # judged at kref, not at the surface
    assert _one(UP, [0.5, 3.0])[1] == 20.0  # ... and alone


def test_step_5_the_sea_floor_ends_the_scan_and_the_first_crossing_wins():
    col = [1.0, 2.0, NAN, 8.0, 16.0]  # values below the floor are not looked at
    assert np.isnan(_one(col, [5.0])).all()
    assert _one(col, [5.0, 1.5], miss=cn.MISS_FLOOR) == [15.0, 10.0]
    # crossing, un-crossing, crossing again: 1 -> 4 crosses 3 two thirds of the way down
    got = _one([1.0, 4.0, 2.0, 6.0, 7.0], [3.0, 5.0])
    assert got == [5.0 + ((3.0 - 1.0) / (4.0 - 1.0)) * 10.0, 25.0 + ((5.0 - 2.0) / (6.0 - 2.0)) * 10.0]
    got = _one([9.0, 6.0, 8.0, 5.0, 1.0], [7.0], mode=cn.FALL)
    assert got == [5.0 + ((7.0 - 9.0) / (6.0 - 9.0)) * 10.0]
    # the scan starts at kref: a crossing above it does not count
    assert _one([1.0, 4.0, 2.0, 6.0, 7.0], [3.0], kref=2) == [25.0 + ((3.0 - 2.0) / (6.0 - 2.0)) * 10.0]


def test_step_6_no_crossing_and_the_floor_field():
    assert np.isnan(_one(UP, [20.0])).all()
    assert _one(UP, [20.0], miss=cn.MISS_FLOOR) == [45.0]  # the deepest level with a value
    assert _one(UP[:3] + [NAN, NAN], [20.0], miss=cn.MISS_FLOOR) == [25.0]
    assert _one(UP, [20.0, 3.0], miss=cn.MISS_FLOOR, floor=51.0) == [51.0, 20.0]
    assert np.isnan(_one(UP, [20.0], miss=cn.MISS_FLOOR, floor=NAN)).all()  # a NaN floor is a NaN
    assert np.isnan(_one(UP, [20.0], miss=cn.MISS_NAN, floor=51.0)).all()


def test_no_scan_is_a_miss():
    # nz = 1, and kref = nz - 1
    assert np.isnan(_one([1.0], [3.0])).all()
    assert _one([1.0], [3.0], miss=cn.MISS_FLOOR) == [5.0]
    assert np.isnan(_one([1.0], [0.5], miss=cn.MISS_FLOOR)).all()  # (an outcrop still is one)
    assert _one(UP, [0.5], relative=True, kref=4, miss=cn.MISS_FLOOR) == [45.0]
    assert _one(UP, [0.5], relative=True, kref=4, miss=cn.MISS_FLOOR, floor=60.0) == [60.0]
    assert np.isnan(_one(UP, [0.5], mode=cn.DEPART, relative=True, kref=4)).all()


def test_float32_fields_widen_exactly_and_records_are_independent():
    x = np.array([UP, DOWN, [NAN] * 5], dtype=np.float32).T.reshape(1, 5, 3)
    x = np.concatenate([x, x[:, :, ::-1]])
    out = cn.column_crossing(x, Z, 0, cn.RISE, False, cn.MISS_FLOOR, [3.0])
    assert out[0, 0, 0] == 20.0 and np.isnan(out[0, 0, 1]) and np.isnan(out[0, 0, 2])
    assert out[1, 0, 2] == 20.0 and np.isnan(out[1, 0, 0])
    assert cn.nearest_level(Z, 10.0) == 0 and cn.nearest_level(Z, 10.1) == 1  # ties: the shallower
    assert cn.nearest_level(Z, 1000.0) == 4 and cn.nearest_level(Z, -3.0) == 0


def test_sigma_is_the_float64_density_of_the_widened_values():
    from oracle import momlevel_numpy as o

    T = np.array([20.0, 4.0, NAN], dtype=np.float32)
    S = np.array([35.0, 34.5, 35.0], dtype=np.float32)
    s = cn.sigma(T, S, 101325.0)
    assert s.dtype == np.float64 and np.isnan(s[2])
    assert np.array_equal(s[:2], o.wright_density(T.astype(np.float64), S.astype(np.float64), 101325.0)[:2])
    assert not np.array_equal(s[:2], o.wright_density(T, S, 101325.0)[:2].astype(np.float64))
    assert 1020.0 < s[0] < s[1] < 1030.0
    assert cn.sigma(T, S, 0.0, "linear")[0] == 1000.0 + ((-0.2 * 20.0) + (0.8 * 35.0))


# ---- the restatement against an independent spelling -------------------------------------------------
def test_absolute_rise_is_np_interp_on_monotone_columns():
    """Both are the same linear interpolation with at most four roundings each and a fraction <= 1:
    |depth - np.interp(tgt, x, z)| <= 16 * 2^-53 * z[k+1]"""
    rng = np.random.default_rng(11)
    nz, plane = 12, 400
    z = np.cumsum(rng.uniform(1.0, 60.0, nz))
    x = np.cumsum(rng.uniform(1e-3, 2.0, (nz, plane)), axis=0) + rng.normal(0.0, 5.0, plane)
    frac = rng.uniform(0.001, 0.999, (3, plane))
    worst = 0.0
    for c in range(plane):
        tg = x[0, c] + frac[:, c] * (x[-1, c] - x[0, c])
        got = cn.column_crossing(x[None, :, c:c + 1], z, 0, cn.RISE, False, cn.MISS_NAN, tg)[0, :, 0]
        ref = np.interp(tg, x[:, c], z)
        k1 = np.searchsorted(x[:, c], tg, side="left")  # the level of the hit
        bound = 16 * 2.0 ** -53 * z[k1]
        assert np.all((z[k1 - 1] <= got) & (got <= z[k1]))
        assert np.all(np.abs(got - ref) <= bound), (c, got, ref)
        worst = max(worst, float(np.max(np.abs(got - ref) / bound)))
    print(f"worst |restatement - np.interp| / bound = {worst:.3f}")


# ---- the C ABI -------------------------------------------------------------------------------------
def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_column_header_declares_exactly_the_three_symbols():
    text = _header_text()
    declared = sorted(set(re.findall(r"\b(mlx_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.COLUMN_SIGNATURES) == NAMES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in momlevel_column.h but not exported"
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                             text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(mlx_column_[a-z0-9_]+)\b", out))) == declared
    ctype = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p,
             "const double *": ctypes.c_void_p, "double *": ctypes.c_void_p,
             "int64_t ": ctypes.c_int64, "int ": ctypes.c_int, "double ": ctypes.c_double}
    protos = re.findall(r"\b(int64_t|int)\s+(mlx_column_[a-z_]+)\s*\(([^)]*)\)", text)
    assert sorted(p[1] for p in protos) == declared
    for ret, name, args in protos:
        args = [" ".join(a.split()) for a in args.split(",")]
        restype, argtypes = _lib.COLUMN_SIGNATURES[name]
        assert restype is (ctypes.c_int64 if ret == "int64_t" else ctypes.c_int), name
        assert argtypes == [next(v for k, v in ctype.items() if a.startswith(k)) for a in args], name
        if name == "mlx_column_crossing":
            assert args[-1] == "void *stream"  # the caller's stream last
    defines = dict(re.findall(r"#define MLX_(COLUMN_[A-Z_]+)\s+(\d+)", text))
    assert defines == {"COLUMN_MAX_TARGETS": "8", "COLUMN_RISE": "0", "COLUMN_FALL": "1",
                       "COLUMN_DEPART": "2", "COLUMN_MISS_NAN": "0", "COLUMN_MISS_FLOOR": "1"}
    assert _lib.COLUMN_MAX_TARGETS == core.COLUMN_MAX_TARGETS == 8
    assert (_lib.COLUMN_RISE, _lib.COLUMN_FALL, _lib.COLUMN_DEPART) == (cn.RISE, cn.FALL, cn.DEPART) == (0, 1, 2)
    assert (_lib.COLUMN_MISS_NAN, _lib.COLUMN_MISS_FLOOR) == (cn.MISS_NAN, cn.MISS_FLOOR) == (0, 1)
    assert core.COLUMN_MODES == {"rise": 0, "fall": 1, "depart": 2}
    assert core.COLUMN_MISS == {"nan": 0, "floor": 1}
    assert _lib.load_column() is _lib.load()
    assert "tests/column_numpy.py" in open(HEADER).read()


def test_launch_queries_are_plain_arithmetic():
    """256 threads of one 16-byte pack of the wider field, or of one cell; a block row per record
    up to the cap"""
    f64, f32 = np.float64, np.float32
    cells = core.column_block_cells
    assert cells(f64) == cells(f64, f64) == cells(f64, f32) == cells(f32, f64) == 512
    assert cells(f32) == cells(f32, f32) == 1024
    for a, b in ((f64, None), (f32, None), (f32, f64), (f32, f32)):
        assert cells(a, b, generic=True) == 256
    lib = _lib.load_column()
    assert lib.mlx_column_block_cells(2, 0, 0, 0) == 0 and lib.mlx_column_block_cells(0, 1, 5, 0) == 0
    assert lib.mlx_column_block_cells(1, 0, 5, 0) == 1024  # FIELD source: b_dtype is not looked at
    rows = core.column_record_rows
    cap = rows(10 ** 9)
    assert 1 < cap <= 65535 and rows(1 << 38) == cap
    for nrec in (1, 2, 1000, cap - 1, cap):
        assert rows(nrec) == nrec
    assert rows(cap + 1) == cap
    assert rows(0) == 0 and rows(-5) == 0 and rows((1 << 38) + 1) == 0


def test_other_tables_and_the_abi_version_are_untouched():
    others = [v for k, v in vars(_lib).items() if k.endswith("SIGNATURES") and k != "COLUMN_SIGNATURES"]
    assert len(others) == 11
    for name in _lib.COLUMN_SIGNATURES:
        for table in others:
            assert name not in table
    assert len(_lib.SIGNATURES) == 28 and len(_lib.LAYER_SIGNATURES) == 3
    assert _lib.ABI_VERSION == 9 and _lib.load().mlx_version() == 9
    assert _lib._GROUPS["column"][0] is _lib.COLUMN_SIGNATURES


def column_call(lib, **kw):
    """mlx_column_crossing with arguments that pass every check (pointers that are never
    dereferenced: the checks precede every HIP call), ``kw`` replacing some"""
    f = 1 << 20
    a = dict(a=f, adt=_lib.DTYPE_F64, b=f, bdt=_lib.DTYPE_F32, eos=0, p_ref=101325.0, nrec=2, nz=3,
             plane=10, z=f, kref=1, mode=0, relative=0, miss=1, targets=[1027.0, 1027.5], nt=None,
             floor=f, out=f)
    a.update(kw)
    keep = []

    def host(v):
        if v is None or isinstance(v, int):
            return v
        keep.append(np.ascontiguousarray(v, dtype=np.float64))
        return keep[-1].ctypes.data

    nt = a["nt"] if a["nt"] is not None else len(a["targets"])
    return lib.mlx_column_crossing(a["a"], a["adt"], a["b"], a["bdt"], a["eos"], a["p_ref"],
                                   a["nrec"], a["nz"], a["plane"], a["z"], a["kref"], a["mode"],
                                   a["relative"], a["miss"], host(a["targets"]), nt, a["floor"],
                                   a["out"], None)


REFUSALS = [
    (dict(adt=2), -3), (dict(adt=-1), -3), (dict(bdt=3), -3), (dict(bdt=-1), -3), (dict(eos=2), -3),
    (dict(eos=-1), -3), (dict(mode=3), -3), (dict(mode=-1), -3), (dict(relative=2), -3),
    (dict(relative=-1), -3), (dict(miss=2), -3), (dict(miss=-1), -3),
    (dict(nt=0), -2), (dict(nt=-1), -2), (dict(nt=9, targets=[1.0] * 9), -2),
    (dict(nz=0), -2), (dict(nz=-3), -2), (dict(kref=-1), -2), (dict(kref=3), -2),
    (dict(nrec=-1), -2), (dict(plane=-1), -2),
    (dict(nrec=1 << 20, nz=1, kref=0, plane=(1 << 18) + 1), -2), (dict(plane=1 << 39), -2),
    (dict(nrec=1 << 13, nz=1 << 13, plane=(1 << 12) + 1), -2), (dict(nz=(1 << 38) + 1), -2),
    (dict(a=None), -1), (dict(z=None), -1), (dict(targets=None, nt=2), -1), (dict(out=None), -1),
    (dict(a=(1 << 20) + 4), -5), (dict(a=(1 << 20) + 2, adt=1), -5), (dict(b=(1 << 20) + 2), -5),
    (dict(b=(1 << 20) + 4, bdt=0), -5), (dict(z=(1 << 20) + 4), -5), (dict(floor=(1 << 20) + 4), -5),
    (dict(out=(1 << 20) + 4), -5),
    (dict(targets=[NAN, 5.0]), -2), (dict(targets=[5.0, NAN], relative=1), -2),
    (dict(targets=[0.0, 5.0], relative=1), -2), (dict(targets=[5.0, -0.03], relative=1), -2),
    (dict(mode=2, relative=0), -2), (dict(mode=2, relative=1, targets=[0.2, 0.0]), -2),
]


def test_argument_errors_need_no_gpu():
    lib = _lib.load_column()
    for kw, code in REFUSALS:
        assert column_call(lib, **kw) == code and _lib.last_error(), kw
    assert "NULL" in (column_call(lib, out=None), _lib.last_error())[1]
    assert "2^38" in (column_call(lib, plane=1 << 39), _lib.last_error())[1]
    assert "DEPART" in (column_call(lib, mode=2), _lib.last_error())[1]
    # nothing to do: no launch, whatever the pointers
    assert column_call(lib, nrec=0) == 0 and column_call(lib, plane=0) == 0
    assert column_call(lib, nrec=0, a=None, z=None, out=None) == 0
    # ... but the shape and enum checks come first
    assert column_call(lib, nrec=0, nz=0) == -2 and column_call(lib, plane=0, adt=5) == -3
    assert column_call(lib, nrec=0, mode=2) == -2
    # FIELD source: b_dtype and eos are not looked at; absolute targets may be <= 0
    assert column_call(lib, nrec=0, b=None, bdt=7, eos=9) == 0
    assert column_call(lib, nrec=0, targets=[-2.0, 0.0]) == 0
    # a float32 field needs its own alignment only; floor is optional
    assert column_call(lib, a=(1 << 20) + 4, adt=1, nrec=0, floor=None) == 0


def test_a_library_without_the_kernel_is_an_error(monkeypatch):
    class Bare:
        def __getattr__(self, name):
            raise AttributeError(name)

    monkeypatch.setattr(_lib, "_column_bound", False)
    monkeypatch.setattr(_lib, "load", lambda: Bare())
    with pytest.raises(_lib.MomlevelHipError, match="does not export mlx_column_[a-z_]+: rebuild"):
        _lib.load_column()


def test_features_has_the_row_and_a_sha_of_its_own():
    from momlevel_amd.csrc import build

    assert build.FEATURES["column"] == ["eos_device.hpp", "mlx_internal.hpp", "mlx_pack.hpp",
                                        "include/momlevel_column.h"]
    assert len(build.column_source_sha()) == 16
    assert build.column_source_sha() == build.feature_source_sha("column")
    assert build.column_source_sha() not in (build.source_sha(), build.layer_source_sha(),
                                             build.strat_source_sha(), build.quantile_source_sha())
    names = {os.path.basename(p) for p in build.TIMED_SOURCES}
    assert "momlevel_column.hip" not in names and "momlevel_column.h" not in names
    assert any(p.endswith("momlevel_column.hip") for p in build.SOURCES)
    assert any(p.endswith("momlevel_column.h") for p in build.DEPENDS)
    text = open(os.path.join(ROOT, "momlevel_amd", "csrc", "momlevel_column.hip")).read()
    assert "#pragma clang fp contract(off)" in text and "__shared__" not in text
    assert "atomic" not in text.replace("atomics", "")
    assert "__builtin_amdgcn_ballot_w64" in text  # the wave-wide exit
    assert "wright_density<kF64, double, ExactOps>" in text  # the one density of eos_device.hpp


# ---- what the public functions refuse before any device work ----------------------------------------
DIMS = ("time", "z_l", "yh", "xh")


def _field(z=Z[:4], shape=(2, 4, 3, 5), dims=DIMS, dtype=np.float64):
    return DataArray(np.ones(shape, dtype=dtype), dims, {"z_l": DataArray(np.asarray(z), ("z_l",))})


def test_public_refusals_need_no_gpu():
    f = _field()
    for bad in ([5.0, 15.0, 15.0, 35.0], [5.0, 25.0, 15.0, 35.0], [35.0, 25.0, 15.0, 5.0],
                [5.0, 15.0, NAN, 35.0]):
        with pytest.raises(ValueError, match="increase strictly"):
            derived.calc_mld(_field(z=bad), criterion="temperature")
        with pytest.raises(ValueError, match="increase strictly"):
            derived.calc_isosurface_depth(_field(z=bad), 20.0, direction="decreasing")
        with pytest.raises(ValueError, match="increase strictly"):
            derived.calc_isopycnal_depth(_field(z=bad), _field(z=bad), [1027.0])
    with pytest.raises(ValueError, match="needs so"):
        derived.calc_mld(f)
    with pytest.raises(ValueError, match="needs so"):
        derived.calc_mld(f, criterion="density", threshold=0.01)
    for bad in (0.0, -0.2, [0.2, 0.0], [0.2, NAN]):
        with pytest.raises(ValueError, match="threshold must be > 0"):
            derived.calc_mld(f, criterion="temperature", threshold=bad)
        with pytest.raises(ValueError, match="threshold must be > 0"):
            derived.calc_mld(f, f, threshold=bad)
    with pytest.raises(ValueError, match="criterion"):
        derived.calc_mld(f, f, criterion="salinity")
    # more dims behind z than two; z not a dim; no coordinate values
    five = _field(shape=(4, 2, 3, 5), dims=("z_l", "member", "yh", "xh"))
    with pytest.raises(ValueError, match="two horizontal dims"):
        derived.calc_mld(five, criterion="temperature")
    with pytest.raises(ValueError, match="two horizontal dims"):
        derived.calc_isosurface_depth(five, [20.0], direction="decreasing")
    with pytest.raises(ValueError, match="two horizontal dims"):
        derived.calc_isopycnal_depth(five, five, 1027.0)
    with pytest.raises(ValueError, match="two horizontal dims"):
        derived.calc_isosurface_depth(_field(shape=(4, 5), dims=("z_l", "xh")), 20.0, direction="increasing")
    with pytest.raises(ValueError, match="not a dimension"):
        derived.calc_mld(f, criterion="temperature", zcoord="lev")
    with pytest.raises(ValueError, match="no coordinate values"):
        derived.calc_mld(DataArray(np.ones((2, 4, 3, 5)), DIMS), criterion="temperature")
    with pytest.raises(ValueError, match="expected depth's plane"):
        derived.calc_mld(f, criterion="temperature", deptho=np.ones((3, 4)))
    with pytest.raises(ValueError, match="agree in dims and shape"):
        derived.calc_mld(f, _field(shape=(2, 4, 3, 4)))
    with pytest.raises(ValueError, match="agree in dims and shape"):
        derived.calc_isopycnal_depth(f, _field(shape=(4, 2, 3, 5), dims=("z_l", "time", "yh", "xh")), 1027.0)
    with pytest.raises(TypeError, match="Dataset is not accepted"):
        derived.calc_isosurface_depth(Dataset({"a": f}), 20.0)
    with pytest.raises(TypeError, match="float16"):
        derived.calc_mld(_field(dtype=np.float16), criterion="temperature")
    with pytest.raises(ValueError, match="direction"):
        derived.calc_isosurface_depth(f, 20.0, direction="up")
    with pytest.raises(ValueError, match="missing"):
        derived.calc_isosurface_depth(f, 20.0, direction="increasing", missing="zero")
    with pytest.raises(ValueError, match="no NaN"):
        derived.calc_isosurface_depth(f, [20.0, NAN], direction="increasing")
    with pytest.raises(ValueError, match="no NaN"):
        derived.calc_isopycnal_depth(f, f, [])
    with pytest.raises(AssertionError, match="between 0 and 7500"):
        derived.calc_isopycnal_depth(f, f, 1027.0, level=8000.0)
    with pytest.raises(AssertionError, match="between 0 and 7500"):
        derived.calc_mld(f, f, level=-1.0)
    with pytest.raises(ValueError, match="equation of state"):
        derived.calc_isopycnal_depth(f, f, 1027.0, eos="teos10")
    for name in ("calc_mld", "calc_isosurface_depth", "calc_isopycnal_depth"):
        assert name in derived.__all__
