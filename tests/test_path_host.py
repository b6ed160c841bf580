"""CPU: the path queries of the pointwise EOS entry points (include/momlevel_path.h) --
mlx_path_eos_map and mlx_path_eos_promote, the rules eos_map_impl and promote_go launch by.  Host
arithmetic: every condition of the fast layout flipped one at a time from a call that is fast, the
rules that depend on the function, the cells a lane takes for each of the 26 operand kinds, and
the arguments that are refused.  tests/test_gpu_eos_matrix.py sizes its cases from these answers
and asserts the path of each case from them."""

import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from momlevel_amd import _lib, core
from conftest import MIX_KINDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "momlevel_path.h")
NAMES = ["mlx_path_eos_map", "mlx_path_eos_promote"]

F64, F32, UP = _lib.DTYPE_F64, _lib.DTYPE_F32, _lib.DTYPE_F32_UPCAST
W, LIN = _lib.EOS_WRIGHT, _lib.EOS_LINEAR
DENS, DT, DS, AL, BE, IBH = (_lib.FUNC_DENSITY, _lib.FUNC_DRHO_DTEMP, _lib.FUNC_DRHO_DSAL,
                             _lib.FUNC_ALPHA, _lib.FUNC_BETA, _lib.FUNC_IBH)
ALL = _lib.PATH_ALIGNED_ALL


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_path_header_declares_exactly_the_two_symbols():
    text = _header_text()
    declared = sorted(set(re.findall(r"\b(mlx_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.PATH_SIGNATURES) == NAMES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in momlevel_path.h but not exported"
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                             text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(mlx_path_[a-z0-9_]+)\b", out))) == declared
    ctype = {"int64_t *": ctypes.POINTER(ctypes.c_int64), "int *": ctypes.POINTER(ctypes.c_int),
             "int64_t ": ctypes.c_int64, "int ": ctypes.c_int}
    protos = re.findall(r"\b(int)\s+(mlx_[a-z_]+)\s*\(([^)]*)\)", text)
    assert sorted(p[1] for p in protos) == declared
    for _, name, args in protos:
        args = [" ".join(a.split()) for a in args.split(",")]
        restype, argtypes = _lib.PATH_SIGNATURES[name]
        assert restype is ctypes.c_int, name
        assert argtypes == [next(v for k, v in ctype.items() if a.startswith(k)) for a in args], name
    for name, val in re.findall(r"#define MLX_(PATH_[A-Z0-9_]+)\s+(\d+)", text):
        assert getattr(_lib, name) == int(val), name
    assert _lib.load_path() is _lib.load()


def test_other_tables_and_the_abi_version_are_untouched():
    for name in _lib.PATH_SIGNATURES:
        for table in (_lib.SIGNATURES, _lib.TREND_SIGNATURES, _lib.CLIM_SIGNATURES,
                      _lib.GAUGE_SIGNATURES, _lib.SPICE_SIGNATURES, _lib.VORT_SIGNATURES,
                      _lib.AREA_SIGNATURES, _lib.LAYER_SIGNATURES, _lib.FILTER_SIGNATURES):
            assert name not in table
        assert not name.startswith("mlx_time_")
    assert len(_lib.SIGNATURES) == 28 and len(_lib.FILTER_SIGNATURES) == 4
    assert _lib.ABI_VERSION == 9 and _lib.load().mlx_version() == 9


def k0(dtype=F64, p_mode=_lib.P_ZPROF, eos=W, func=DENS, plane=6, sT=18, sS=18, flags=0,
       aligned16=ALL):
    return core.k0_path(dtype, p_mode, eos, func, plane, sT, sS, flags, aligned16)


def test_k0_geometry():
    """cells a block covers: 256 threads x 2 packs of 16 bytes on the fast paths, x 4 cells on the
    generic one; one launch length for every path"""
    kind, cells64, steps = k0()
    assert kind == "fast" and cells64 == 256 * 2 * 2 and steps >= 1
    for dtype in (F32, UP):
        assert k0(dtype=dtype, plane=8, sT=24, sS=24) == ("fast", 256 * 2 * 4, steps)
    assert k0(plane=5, sT=15, sS=15) == ("generic", 256 * 4, steps)
    assert k0(dtype=F32, plane=5, sT=15, sS=15) == ("generic", 256 * 4, steps)
    assert k0(p_mode=_lib.P_FULL3D) == ("fast_p3d", cells64, steps)
    assert 1 <= steps <= 65535  # the launch's grid.z
    # NULL result pointers: the path alone
    lib = _lib.load_path()
    assert lib.mlx_path_eos_map(F64, _lib.P_ZPROF, W, DENS, 6, 18, 18, 0, ALL, None, None) == _lib.PATH_FAST


@pytest.mark.parametrize("dtype,pack", [(F64, 2), (F32, 4), (UP, 4)])
def test_every_condition_of_the_fast_layout_flipped_alone(dtype, pack):
    plane = 3 * pack
    base = dict(dtype=dtype, plane=plane, sT=3 * plane, sS=3 * plane)
    assert k0(**base)[0] == "fast"
    assert k0(**base, p_mode=_lib.P_FULL3D)[0] == "fast_p3d"
    # the EOS
    assert k0(**{**base, "eos": LIN})[0] == "generic"
    # the pressure form: scalar and (t,z,y,x) have no fast kernel
    for p_mode in (_lib.P_SCALAR, _lib.P_FULL4D):
        assert k0(**base, p_mode=p_mode)[0] == "generic"
    # whole packs: the plane, each time stride
    for off in range(1, pack):
        assert k0(**{**base, "plane": plane + off})[0] == "generic"
        assert k0(**{**base, "sT": 3 * plane + off})[0] == "generic"
        assert k0(**{**base, "sS": 3 * plane + off})[0] == "generic"
    assert k0(**{**base, "sT": 0})[0] == "fast" and k0(**{**base, "sS": 0})[0] == "fast"  # held
    assert k0(**{**base, "sT": 6 * plane})[0] == "fast"  # a strided time view
    # the alignment of T, S and out, one at a time; a z profile needs none of its own
    for bit in (_lib.PATH_ALIGNED_T, _lib.PATH_ALIGNED_S, _lib.PATH_ALIGNED_OUT):
        assert k0(**base, aligned16=ALL & ~bit)[0] == "generic"
        assert k0(**base, p_mode=_lib.P_FULL3D, aligned16=ALL & ~bit)[0] == "generic"
    assert k0(**base, aligned16=ALL & ~_lib.PATH_ALIGNED_P)[0] == "fast"
    # ... a (z,y,x) pressure field read in packs does
    assert k0(**base, p_mode=_lib.P_FULL3D, aligned16=ALL & ~_lib.PATH_ALIGNED_P)[0] == "generic"
    # fused arithmetic changes the arithmetic, not the shape
    assert k0(**base, flags=_lib.FLAG_FMA) == k0(**base)
    assert k0(**base, p_mode=_lib.P_FULL3D, flags=_lib.FLAG_FMA)[0] == "fast_p3d"
    assert k0(**{**base, "plane": plane + 1}, flags=_lib.FLAG_FMA)[0] == "generic"


def test_rules_that_depend_on_the_function():
    geo = dict(plane=8, sT=24, sS=24)
    for func in (DT, DS, AL, BE):
        assert k0(func=func, **geo)[0] == "fast"  # float64: all five functions
        for dtype in (F32, UP):  # float32 fields: the density alone
            assert k0(dtype=dtype, func=func, **geo)[0] == "generic"
            assert k0(dtype=dtype, func=DENS, **geo)[0] == "fast"
        # a (z,y,x) pressure field is fast for the density only
        assert k0(func=func, p_mode=_lib.P_FULL3D, **geo)[0] == "generic"
    for dtype in (F64, F32, UP):
        assert k0(dtype=dtype, func=DENS, p_mode=_lib.P_FULL3D, **geo)[0] == "fast_p3d"
        for p_mode in (_lib.P_SCALAR, _lib.P_ZPROF, _lib.P_FULL3D, _lib.P_FULL4D):
            for eos in (W, LIN):  # the inverse barometer is never fast
                assert k0(dtype=dtype, func=IBH, p_mode=p_mode, eos=eos, **geo)[0] == "generic"


def test_k0_query_refuses_what_the_entry_point_refuses():
    lib = _lib.load_path()

    def rc(dtype=F64, p_mode=_lib.P_ZPROF, eos=W, func=DENS, plane=6, sT=18, sS=18, flags=0,
           aligned16=ALL):
        return lib.mlx_path_eos_map(dtype, p_mode, eos, func, plane, sT, sS, flags, aligned16, None, None)

    assert rc() == _lib.PATH_FAST
    for kw in (dict(dtype=9), dict(dtype=-1), dict(dtype=_lib.DTYPE_T32_S64),
               dict(dtype=_lib.DTYPE_T64_S32), dict(p_mode=4), dict(p_mode=-1), dict(eos=2),
               dict(func=-1), dict(func=_lib.FUNC_DENSITY_REF), dict(flags=_lib.FLAG_SKIP_DRY),
               dict(flags=_lib.FLAG_FMA, func=AL), dict(flags=_lib.FLAG_FMA, func=IBH),
               dict(aligned16=16), dict(aligned16=-1)):
        assert rc(**kw) == -3, kw  # MLX_E_ENUM
        assert _lib.last_error()
    for kw in (dict(plane=0), dict(plane=-2), dict(plane=(1 << 40) + 1), dict(sT=-1), dict(sS=-1)):
        assert rc(**kw) == -2, kw  # MLX_E_SHAPE
    with pytest.raises(_lib.MomlevelHipError, match="mlx_path_eos_map"):
        k0(eos=5)


# ---- mlx_path_eos_promote -----------------------------------------------------------------------------
PROMOTE_FUNCS = [("wright", f) for f in ("density", "drho_dtemp", "drho_dsal", "alpha", "beta",
                                         "inverse_barometer")] + \
                [("linear", f) for f in ("density", "drho_dtemp", "drho_dsal", "alpha", "beta",
                                         "inverse_barometer", "density_ref")]


@pytest.mark.parametrize("kinds", MIX_KINDS + ["www"])
def test_cells_a_lane_takes_for_every_kind(kinds):
    """4 cells when float32 arrays and python floats give a float32 result, 2 as soon as a float64
    array takes part or the result is float64, 1 without the alignment; the result kind is float64
    exactly when a float64 array is read or numpy's expression makes one (full_like of a weak T)"""
    for eos, func in PROMOTE_FUNCS:
        read = kinds if (eos == "wright" or func in ("inverse_barometer", "density_ref")) else kinds[:2] + "w"
        width, dtype = core.promote_path(kinds, eos, func)
        assert core.promote_path(kinds, eos, func, aligned16=0) == (1, dtype)
        # one pointer off 16 bytes at a time: it counts when it is an array that is read
        for i, bit in enumerate((_lib.PATH_ALIGNED_T, _lib.PATH_ALIGNED_S, _lib.PATH_ALIGNED_P)):
            assert core.promote_path(kinds, eos, func, ALL & ~bit) == \
                ((1 if read[i] != "w" else width), dtype), (kinds, eos, func, i)
        assert core.promote_path(kinds, eos, func, ALL & ~_lib.PATH_ALIGNED_OUT) == (1, dtype)
        assert core.promote_path(read, eos, func) == (width, dtype)  # an unread pressure: no part
        if "d" in read:
            assert (width, dtype) == (2, torch.float64), (kinds, eos, func)
        else:
            assert width == (4 if dtype == torch.float32 else 2), (kinds, eos, func)
            weak_T_full_like = eos == "linear" and func in ("alpha", "beta") and read[0] == "w"
            constant = eos == "linear" and func in ("drho_dtemp", "drho_dsal")
            if "f" in read and not weak_T_full_like and not constant:
                assert dtype == torch.float32, (kinds, eos, func)
            if weak_T_full_like:  # np.full_like(python float) is a float64 array
                assert (width, dtype) == (2, torch.float64), (kinds, eos, func)


def test_the_result_kinds_the_launcher_names_are_all_there():
    assert core.promote_path("ffw") == (4, torch.float32)
    assert core.promote_path("fff") == (4, torch.float32)
    assert core.promote_path("fwf") == (4, torch.float32)
    assert core.promote_path("wff", "wright", "alpha") == (4, torch.float32)
    assert core.promote_path("ffd") == (2, torch.float64)
    assert core.promote_path("dff") == (2, torch.float64)
    assert core.promote_path("wfw", "linear", "alpha") == (2, torch.float64)  # float32 arrays, float64 out
    assert core.promote_path("wfd", "linear", "beta") == (2, torch.float64)   # (p unread)
    assert core.promote_path("ffd", "linear", "density") == (4, torch.float32)  # (p unread)
    assert core.promote_path("ffd", "linear", "inverse_barometer") == (2, torch.float64)
    assert core.promote_path("ffd", "linear", "density_ref") == (2, torch.float64)


def test_promote_query_refuses_what_the_entry_point_refuses():
    lib = _lib.load_path()
    K = _lib.KIND_F32
    assert lib.mlx_path_eos_promote(K, K, K, W, DENS, ALL, None) == 4
    assert lib.mlx_path_eos_promote(K, K, K, W, DENS, 16, None) == -3
    assert lib.mlx_path_eos_promote(K, K, K, W, DENS, -1, None) == -3
    for args in ((3, K, K, W, DENS), (K, -1, K, W, DENS), (K, K, 7, W, DENS), (K, K, K, 2, DENS),
                 (K, K, K, W, 7), (K, K, K, W, -1), (K, K, K, W, _lib.FUNC_DENSITY_REF)):
        assert lib.mlx_path_eos_promote(*args, ALL, None) == -3, args
    assert lib.mlx_path_eos_promote(K, K, 7, LIN, DENS, ALL, None) == 4  # the unread pressure's kind too
