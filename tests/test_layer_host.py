"""CPU: the numpy restatement tests/layer_numpy.py against hand-computed columns, the C ABI of
include/momlevel_layer.h (symbols, binding table, argument errors -- they precede every HIP call),
derived.layer_bounds and the refusals of derived.calc_layer_integral.  No GPU."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import layer_numpy as ln
from momlevel_amd import _lib, core, derived
from momlevel_amd.labeled import DataArray, Dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "momlevel_layer.h")
NAMES = ["mlx_layer_integral", "mlx_layer_record_blocks", "mlx_layer_steps"]
INF = np.inf


# ---- the restatement against columns computed by hand ---------------------------------------------
Z_I = np.array([0.0, 10.0, 30.0, 60.0, 100.0])
X = np.array([1.0, 2.0, 4.0, 8.0]).reshape(1, 4, 1)  # one record, one cell
FLOOR = np.array([45.0])  # a partial bottom cell: 15 m of level 2, nothing of level 3


def _one(top, bottom, depth=FLOOR, x=X, **kw):
    return ln.layer_integral(x, Z_I, depth, [top], [bottom], **kw)[0, 0, 0]


def test_restatement_on_hand_computed_columns():
    assert _one(0.0, INF) == 10 * 1 + 20 * 2 + 15 * 4 == 110.0  # the partial bottom cell
    assert _one(0.0, 20.0) == 10 * 1 + 10 * 2 == 30.0  # a cut inside level 1 ...
    assert _one(20.0, INF) == 10 * 2 + 15 * 4 == 80.0  # ... whose two parts add up
    assert _one(10.0, 30.0) == 20 * 2 == 40.0  # cuts on interfaces: exactly level 1
    assert _one(0.0, 10.0) == 10.0 and _one(30.0, INF) == 60.0
    assert _one(60.0, INF) == 0.0 and _one(70.0, 90.0) == 0.0  # wholly below the floor
    assert _one(0.0, INF, scale=-0.5) == -55.0
    # the thicknesses themselves: calc_dz(top, bottom)
    assert ln.layer_dz(Z_I, FLOOR, 0.0, None)[:, 0].tolist() == [10.0, 20.0, 15.0, 0.0]
    assert ln.layer_dz(Z_I, FLOOR, 20.0, 40.0)[:, 0].tolist() == [0.0, 10.0, 10.0, 0.0]
    # calc_dz where top and the floor cut the SAME cell: min(zbot - top, depth - ztop), not depth - top
    assert ln.layer_dz(Z_I, FLOOR, 40.0, None)[:, 0].tolist() == [0.0, 0.0, 15.0, 0.0]
    assert ln.layer_dz(Z_I, FLOOR, 50.0, None)[:, 0].tolist() == [0.0, 0.0, 10.0, 0.0]


def test_restatement_skips_nan_terms_and_masks_land():
    x = X.copy()
    x[0, 1, 0] = np.nan
    assert _one(0.0, INF, x=x) == 10 * 1 + 15 * 4
    x[0, :, 0] = np.nan
    assert _one(0.0, INF, x=x) == 0.0 and not np.signbit(_one(0.0, INF, x=x))  # all NaN: +0.0
    x = X.copy()
    x[0, 3, 0] = np.inf  # below the floor: 0 * inf is NaN, skipped
    assert _one(0.0, INF, x=x) == 110.0
    land = np.array([np.nan])
    assert _one(0.0, INF, depth=land) == 0.0  # fillna(0.0): no thickness
    assert np.isnan(_one(0.0, INF, depth=land, surface=np.array([np.nan])))
    assert _one(0.0, INF, surface=np.array([3.0])) == 110.0
    out = ln.layer_integral(np.concatenate([X, 2 * X]).astype(np.float32), Z_I, FLOOR,
                            [0.0, 0.0], [20.0, INF])
    assert out.dtype == np.float64 and out.shape == (2, 2, 1)
    assert out[:, :, 0].tolist() == [[30.0, 110.0], [60.0, 220.0]]
    assert ln.abs_sum(-X, Z_I, FLOOR)[0, 0] == 110.0


# ---- layer_bounds ---------------------------------------------------------------------------------
def test_layer_bounds_takes_both_spellings():
    t, b = derived.layer_bounds([0, 700, 2000, None])
    assert t.dtype == b.dtype == np.float64
    assert t.tolist() == [0.0, 700.0, 2000.0] and b.tolist() == [700.0, 2000.0, INF]
    t, b = derived.layer_bounds([(0, 700), (0, 2000), (700.5, None)])  # pairs may overlap
    assert t.tolist() == [0.0, 0.0, 700.5] and b.tolist() == [700.0, 2000.0, INF]
    t, b = derived.layer_bounds(np.array([0.0, 10.0, 30.0]))
    assert t.tolist() == [0.0, 10.0] and b.tolist() == [10.0, 30.0]
    t, b = derived.layer_bounds([(5, 6)])
    assert t.tolist() == [5.0] and b.tolist() == [6.0]
    t, b = derived.layer_bounds([0, None])
    assert t.tolist() == [0.0] and b.tolist() == [INF]
    t, b = derived.layer_bounds([(k, k + 1) for k in range(11)])  # more than one launch: fine here
    assert t.size == 11


@pytest.mark.parametrize("bad", [
    [], None, [0], [-1, 10], [0, np.nan], [(0, np.nan)], [(np.nan, 5)], [(-2, 5)], [(0, -5)],
    [10, 10], [10, 5], [(5, 5)], [(7, 3)], [0, None, 10], [None, 10], [(None, 10)], [(0, 5), 7],
    [(0, 5, 9)], "ab",
])
def test_layer_bounds_refusals(bad):
    with pytest.raises(ValueError):
        derived.layer_bounds(bad)


# ---- calc_layer_integral: what is refused before any device work -----------------------------------
def _field():
    x = np.ones((2, 4, 3, 5))
    return (DataArray(x, ("time", "z_l", "yh", "xh"), {"z_l": DataArray(0.5 * (Z_I[1:] + Z_I[:-1]), ("z_l",))}),
            DataArray(Z_I, ("z_i",)), DataArray(np.full((3, 5), 45.0), ("yh", "xh")))


def test_a_layer_inside_one_cell_is_refused():
    f, zi, dep = _field()
    for layers in ([(12, 28)], [(0, 10), (31.0, 59.0)], [35, 40]):
        with pytest.raises(ValueError, match="strictly inside one model cell"):
            derived.calc_layer_integral(f, zi, dep, layers)
    # on an interface, or across one: not refused by this check
    derived._check_layers_in_cells(*derived.layer_bounds([(10, 28), (12, 30), (12, 31), (10, 30)]), Z_I)


def test_calc_layer_integral_refusals_need_no_gpu():
    f, zi, dep = _field()
    with pytest.raises(TypeError, match="Dataset is not accepted"):
        derived.calc_layer_integral(Dataset({"a": f}), zi, dep, [0, None])
    with pytest.raises(TypeError):
        derived.calc_layer_integral(DataArray(f.values.astype(np.int32), f.dims), zi, dep, [0, None])
    with pytest.raises(ValueError, match="not a dimension"):
        derived.calc_layer_integral(f, zi, dep, [0, None], zcoord="lev")
    with pytest.raises(ValueError, match="interfaces holds"):
        derived.calc_layer_integral(f, Z_I[:-1], dep, [0, None])
    with pytest.raises(ValueError, match="expected depth's plane"):
        derived.calc_layer_integral(f, zi, DataArray(np.ones((3, 4)), ("yh", "xh")), [0, None])
    with pytest.raises(ValueError, match="expected depth's plane"):  # z must lead the plane
        derived.calc_layer_integral(DataArray(np.ones((4, 2, 3, 5)), ("z_l", "time", "yh", "xh")),
                                    zi, dep, [0, None])
    with pytest.raises(ValueError):
        derived.calc_layer_integral(f, zi, dep, [10, 5])
    with pytest.raises(AssertionError, match="Depth values"):
        derived.calc_layer_integral(f, zi, DataArray(np.full((3, 5), -1.0), ("yh", "xh")), [0, None])
    with pytest.raises(AssertionError, match="interfaces"):
        derived.calc_layer_integral(f, -Z_I, dep, [0, None])
    with pytest.raises(ValueError, match="wet"):
        derived.calc_layer_integral(f, zi, dep, [0, None], wet=np.ones((3, 4)))


# ---- the C ABI -------------------------------------------------------------------------------------
def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_layer_header_declares_exactly_the_two_symbols():
    text = _header_text()
    declared = sorted(set(re.findall(r"\b(mlx_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.LAYER_SIGNATURES) == NAMES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in momlevel_layer.h but not exported"
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                             text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(mlx_layer_[a-z0-9_]+)\b", out))) == declared
    ctype = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p,
             "const double *": ctypes.c_void_p, "double *": ctypes.c_void_p,
             "int64_t ": ctypes.c_int64, "int ": ctypes.c_int, "double ": ctypes.c_double}
    protos = re.findall(r"\b(int)\s+(mlx_layer_[a-z_]+)\s*\(([^)]*)\)", text)
    assert sorted(p[1] for p in protos) == declared
    for _, name, args in protos:
        args = [" ".join(a.split()) for a in args.split(",")]
        restype, argtypes = _lib.LAYER_SIGNATURES[name]
        assert restype is ctypes.c_int
        if args == ["void"]:
            assert argtypes == []
            continue
        assert argtypes == [next(v for k, v in ctype.items() if a.startswith(k)) for a in args], name
        if name != "mlx_layer_record_blocks":  # (a query: host arithmetic, no stream)
            assert args[-1] == "void *stream", name  # the caller's stream last
    assert re.findall(r"#define MLX_(LAYER_[A-Z_]+)\s+(\d+)", text) == [("LAYER_MAX", "8")]
    assert _lib.LAYER_MAX == core.LAYER_MAX == 8
    assert core.LAYER_STEPS == lib.mlx_layer_steps() >= 1
    assert _lib.load_layer() is _lib.load()


def test_record_blocks_is_plain_arithmetic():
    """min(ceil(nrec / steps), cap): a block row per group of records up to the cap"""
    S, blocks = core.LAYER_STEPS, core.layer_record_blocks
    cap = blocks(10 ** 9)
    assert 1 < cap <= 65535 and blocks(1 << 38) == cap  # (a grid's y holds at most 65535)
    for nrec in (1, S - 1, S, S + 1, 2 * S + 3, 1000, S * (cap - 1), S * (cap - 1) + 1):
        if nrec >= 1:
            assert blocks(nrec) == -(-nrec // S), nrec
    assert blocks(S * cap) == cap == blocks(S * cap + 1) == blocks(S * cap + S + 1)
    assert blocks(0) == 0 and blocks(-5) == 0 and blocks((1 << 38) + 1) == 0


def test_other_tables_and_the_abi_version_are_untouched():
    for name in _lib.LAYER_SIGNATURES:
        for table in (_lib.SIGNATURES, _lib.TREND_SIGNATURES, _lib.CLIM_SIGNATURES,
                      _lib.GAUGE_SIGNATURES, _lib.SPICE_SIGNATURES, _lib.VORT_SIGNATURES,
                      _lib.AREA_SIGNATURES):
            assert name not in table
    assert len(_lib.SIGNATURES) == 28 and len(_lib.AREA_SIGNATURES) == 4
    assert _lib.ABI_VERSION == 9 and _lib.load().mlx_version() == 9


def layer_call(lib, **kw):
    """mlx_layer_integral with arguments that pass every check (pointers that are never
    dereferenced: the checks precede every HIP call), ``kw`` replacing some"""
    f = 1 << 20
    a = dict(x=f, dt=_lib.DTYPE_F64, nrec=2, nz=3, plane=10, z_i=f, depth=f, top=[0.0, 5.0],
             bottom=[5.0, np.inf], nl=None, surface=f, scale=1.0, out=f)
    a.update(kw)
    keep = []

    def host(v):
        if v is None or isinstance(v, int):
            return v
        keep.append(np.ascontiguousarray(v, dtype=np.float64))
        return keep[-1].ctypes.data

    nl = a["nl"] if a["nl"] is not None else len(a["top"])
    return lib.mlx_layer_integral(a["x"], a["dt"], a["nrec"], a["nz"], a["plane"], a["z_i"],
                                  a["depth"], host(a["top"]), host(a["bottom"]), nl, a["surface"],
                                  a["scale"], a["out"], None)


REFUSALS = [
    (dict(dt=2), -3), (dict(dt=3), -3), (dict(dt=-1), -3), (dict(dt=7), -3),
    (dict(nl=0), -2), (dict(nl=-1), -2), (dict(nl=9, top=[0.0] * 9, bottom=[1.0] * 9), -2),
    (dict(nz=0), -2), (dict(nz=-3), -2), (dict(nrec=-1), -2), (dict(plane=-1), -2),
    (dict(nrec=1 << 20, nz=1, plane=(1 << 18) + 1), -2), (dict(plane=1 << 39), -2),
    (dict(nrec=1 << 13, nz=1 << 13, plane=(1 << 12) + 1), -2), (dict(nz=(1 << 38) + 1), -2),
    (dict(x=None), -1), (dict(z_i=None), -1), (dict(depth=None), -1), (dict(top=None, nl=2), -1),
    (dict(bottom=None, nl=2), -1), (dict(out=None), -1),
    (dict(x=(1 << 20) + 4), -5), (dict(x=(1 << 20) + 2, dt=1), -5), (dict(z_i=(1 << 20) + 4), -5),
    (dict(depth=(1 << 20) + 4), -5), (dict(surface=(1 << 20) + 4), -5), (dict(out=(1 << 20) + 4), -5),
    (dict(top=[np.nan, 5.0]), -2), (dict(bottom=[5.0, np.nan]), -2), (dict(top=[-1.0, 5.0]), -2),
    (dict(bottom=[0.0, 9.0]), -2), (dict(top=[0.0, 9.0], bottom=[5.0, 8.0]), -2),
]


def test_argument_errors_need_no_gpu():
    lib = _lib.load_layer()
    for kw, code in REFUSALS:
        assert layer_call(lib, **kw) == code and _lib.last_error(), kw
    assert "NULL" in (layer_call(lib, out=None), _lib.last_error())[1]
    assert "2^38" in (layer_call(lib, plane=1 << 39), _lib.last_error())[1]
    # nothing to do: no launch, whatever the pointers
    assert layer_call(lib, nrec=0) == 0 and layer_call(lib, plane=0) == 0
    assert layer_call(lib, nrec=0, x=None, z_i=None, depth=None, out=None) == 0
    # ... but the shape and dtype checks come first
    assert layer_call(lib, nrec=0, nz=0) == -2 and layer_call(lib, plane=0, dt=5) == -3
    # a float32 field needs its own alignment only; surface is optional
    assert layer_call(lib, x=(1 << 20) + 4, dt=1, nrec=0) == 0


def test_a_library_without_the_kernel_is_an_error(monkeypatch):
    class Bare:
        def __getattr__(self, name):
            raise AttributeError(name)

    monkeypatch.setattr(_lib, "_layer_bound", False)
    monkeypatch.setattr(_lib, "load", lambda: Bare())
    with pytest.raises(_lib.MomlevelHipError, match="does not export mlx_layer_[a-z_]+: rebuild"):
        _lib.load_layer()


def test_features_has_the_row_and_a_sha_of_its_own():
    from momlevel_amd.csrc import build

    assert build.FEATURES["layer"] == ["mlx_internal.hpp", "mlx_pack.hpp", "include/momlevel_layer.h"]
    assert len(build.layer_source_sha()) == 16
    assert build.layer_source_sha() == build.feature_source_sha("layer")
    assert build.layer_source_sha() not in (build.source_sha(), build.area_source_sha(),
                                            build.vort_source_sha(), build.strat_source_sha())
    names = {os.path.basename(p) for p in build.TIMED_SOURCES}
    assert "momlevel_layer.hip" not in names and "momlevel_layer.h" not in names
    assert any(p.endswith("momlevel_layer.hip") for p in build.SOURCES)
    assert any(p.endswith("momlevel_layer.h") for p in build.DEPENDS)
    text = open(os.path.join(ROOT, "momlevel_amd", "csrc", "momlevel_layer.hip")).read()
    assert "#pragma clang fp contract(off)" in text and "atomic" not in text.replace("atomics", "")
    assert "calc_dz_cell" in text  # the one definition shared with K2 and k_calc_dz
    hip = open(os.path.join(ROOT, "momlevel_amd", "csrc", "momlevel_hip.hip")).read()
    assert "dz_default" not in hip and hip.count("calc_dz_cell<") == 2
