"""ctypes binding of libmomlevel_hip.so (the C ABI declared in include/momlevel_hip.h).

The library is the ONLY compute backend of momlevel_amd: there is no CPU or
torch fallback.  If it is missing (or was never built) every entry point raises
``MomlevelHipError`` -- loudly, by design.
"""

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# MOMLEVEL_AMD_LIB: bind another build of the SAME library (scripts/sanitize_host.py points it at
# the host-sanitized build of the HIP sources); the default is the in-tree libmomlevel_hip.so.
# load() refuses anything that is not a HIP build of the ABI (mlx_build_kind) or that lives under
# the checker's directory oracle/: the CPU restatement exports the same symbols and must never
# stand in for the device library.
LIB_PATH = os.environ.get("MOMLEVEL_AMD_LIB") or os.path.join(HERE, "libmomlevel_hip.so")
_ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")

# ---- constants mirrored from include/momlevel_hip.h --------------------------------
ABI_VERSION = 9
EOS_WRIGHT, EOS_LINEAR = 0, 1
FUNC_DENSITY, FUNC_DRHO_DTEMP, FUNC_DRHO_DSAL, FUNC_ALPHA, FUNC_BETA, FUNC_IBH = 0, 1, 2, 3, 4, 5
FUNC_DENSITY_REF = 6  # eos.linear.density(..., rho_ref=x): mlx_eos_map_promote only
P_SCALAR, P_ZPROF, P_FULL3D, P_FULL4D = 0, 1, 2, 3
DTYPE_F64, DTYPE_F32, DTYPE_F32_UPCAST = 0, 1, 2
DTYPE_T32_S64, DTYPE_T64_S32 = 3, 4  # theta / salinity of different dtypes (K1 / K2 only)
FLAG_SKIP_DRY = 1
FLAG_FMA = 2
FLAG_DRHO_F32 = 4  # K2 only: delta_rho_out holds float32 elements (eta stays float64)
BUILD_HIP, BUILD_HOST = 1, 2
KIND_F64, KIND_F32, KIND_WEAK = 0, 1, 2  # operand kinds of mlx_eos_map_promote
STRAT_N2, STRAT_TURNER = 0, 1  # mlx_stratification's func
# ---- constants mirrored from include/momlevel_trend.h ------------------------------
TREND_MAX_TERMS = 8
(APPLY_REMOVE, APPLY_CORRECT, APPLY_TREND, APPLY_TREND_ANOM, APPLY_MODEL_RESID,
 APPLY_MODEL) = range(6)
# ---- constants mirrored from include/momlevel_clim.h -------------------------------
STAT_MEAN, STAT_STD, STAT_MIN, STAT_MAX = range(4)
# ---- constants mirrored from include/momlevel_gauge.h ------------------------------
GAUGE_ROW_X, GAUGE_ROW_Y, GAUGE_ROW_Z, GAUGE_ROW_PHI, GAUGE_ROW_LAM = range(5)
GAUGE_ROWS = 5
# ---- constants mirrored from include/momlevel_vort.h -------------------------------
VORT_UNITS_M, VORT_UNITS_CM = 0, 1
VORT_TILE_LANES, VORT_TILE_H, VORT_TILE_BANDS = 64, 16, 4
# ---- constants mirrored from include/momlevel_area.h -------------------------------
AREA_MAX_SLOTS = 16
AREA_WINDOW = 32
# ---- constants mirrored from include/momlevel_layer.h ------------------------------
LAYER_MAX = 8
# ---- constants mirrored from include/momlevel_filter.h -----------------------------
FILTER_NORMALISE = 1
# ---- constants mirrored from include/momlevel_quantile.h ----------------------------
QUANTILE_MAX_Q = 8
# ---- constants mirrored from include/momlevel_column.h -----------------------------
COLUMN_MAX_TARGETS = 8
COLUMN_RISE, COLUMN_FALL, COLUMN_DEPART = 0, 1, 2
COLUMN_MISS_NAN, COLUMN_MISS_FLOOR = 0, 1
# ---- constants mirrored from include/momlevel_eof.h --------------------------------
GRAM_MAX_SPLIT = 32
# ---- constants mirrored from include/momlevel_smooth.h -----------------------------
SMOOTH_FILL, SMOOTH_RESIDUAL = 1, 2
# ---- constants mirrored from include/momlevel_regrid.h -----------------------------
REGRID_PROPAGATE, REGRID_NO_RENORM = 1, 2
# ---- constants mirrored from include/momlevel_census.h -----------------------------
CENSUS_CLOSED_0, CENSUS_CLOSED_1 = 1, 2  # bits of mlx_census_histogram's `closed`
# ---- constants mirrored from include/momlevel_path.h -------------------------------
PATH_GENERIC, PATH_FAST, PATH_FAST_P3D = 0, 1, 2
PATH_ALIGNED_T, PATH_ALIGNED_S, PATH_ALIGNED_OUT, PATH_ALIGNED_P = 1, 2, 4, 8
PATH_ALIGNED_ALL = 15


def flag_tchunk(steps):
    """MLX_FLAG_TCHUNK(steps): K1 tuning hint (time steps per block, multiple of 8; 0 = default)."""
    return ((int(steps) // 8) & 0xFF) << 8


EOS_IDS = {"wright": EOS_WRIGHT, "linear": EOS_LINEAR}
FUNC_IDS = {
    "density": FUNC_DENSITY,
    "drho_dtemp": FUNC_DRHO_DTEMP,
    "drho_dsal": FUNC_DRHO_DSAL,
    "alpha": FUNC_ALPHA,
    "beta": FUNC_BETA,
}

_vp = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
_dbl = ctypes.c_double
_sz = ctypes.c_size_t
_u64 = ctypes.c_uint64

# symbol -> (restype, argtypes); the single source of truth for tests/test_abi.py
SIGNATURES = {
    "mlx_version": (_int, []),
    "mlx_last_error": (_int, [ctypes.c_char_p, _sz]),
    "mlx_build_kind": (_int, []),
    "mlx_last_kernel": (_int, [ctypes.c_char_p, _sz]),
    "mlx_eos_map": (
        _int,
        [_vp, _vp, _int, _vp, _int, _int, _int, _i64, _i64, _i64, _i64, _i64, _int, _vp, _vp],
    ),
    "mlx_eos_map_promote": (
        _int,
        [_vp, _int, _i64, _vp, _int, _i64, _vp, _int, _i64, _int, _int, _dbl, _i64, _vp,
         ctypes.POINTER(ctypes.c_int), _vp],
    ),
    "mlx_inverse_barometer": (
        _int,
        [_vp, _vp, _int, _vp, _int, _int, _dbl, _i64, _i64, _i64, _i64, _i64, _vp, _vp],
    ),
    "mlx_steric_global_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "mlx_steric_global": (
        _int,
        [_vp, _vp, _int, _vp, _vp, _int, _int, _i64, _i64, _i64, _i64, _i64, _int, _vp, _vp, _sz,
         _vp],
    ),
    "mlx_steric_global_decomp_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "mlx_steric_global_decomp": (
        _int,
        [_vp, _vp, _vp, _vp, _int, _vp, _vp, _int, _int, _i64, _i64, _i64, _i64, _i64, _int, _vp,
         _vp, _sz, _vp],
    ),
    "mlx_fold_mask": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "mlx_steric_local": (
        _int,
        [_vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _dbl,
         _i64, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp],
    ),
    "mlx_steric_local_decomp": (
        _int,
        [_vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _dbl,
         _i64, _i64, _i64, _i64, _i64, _int, _vp, _i64, _vp, _i64, _vp],
    ),
    "mlx_nansum_workspace_bytes": (_sz, [_i64]),
    "mlx_nansum": (_int, [_vp, _i64, _vp, _vp, _sz, _vp]),
    "mlx_masso": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _sz, _vp]),
    "mlx_group_weighted_mean": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "mlx_stream_probe": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "mlx_stream_probe_mix": (_int, [_vp, _vp, _int, _i64, _vp, _int, _vp]),
    "mlx_valu_probe": (_int, [_i64, _vp, ctypes.POINTER(ctypes.c_int64), _vp]),
    "mlx_calc_dz": (_int, [_vp, _vp, _i64, _i64, _dbl, _dbl, _int, _int, _vp, _vp]),
    "mlx_host_copy": (_int, [_vp, _vp, _sz, _int, _int]),
    "mlx_host_copy_masked": (_int, [_vp, _vp, _vp, _sz, _int, _int]),
    "mlx_stratification": (_int, [_vp, _vp, _int, _vp, _i64, _i64, _i64, _int, _int, _vp, _int,
                                  _dbl, _dbl, _i64, _i64, _i64, _vp, _vp]),
    "mlx_adjust_negative_n2": (_int, [_vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    "mlx_wave_speed_where_time0": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "mlx_synth_field": (
        _int,
        [_vp, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _u64, _int,
         _dbl, _dbl, _vp, _vp],
    ),
}


# The trend entry points (include/momlevel_trend.h): a table of their own, bound by load_trend() on
# first use -- SIGNATURES stays the set include/momlevel_hip.h declares, which every build of that
# ABI (the checker's host restatement, the sanitized build) exports.
TREND_SIGNATURES = {
    "mlx_time_fit_workspace_bytes": (_sz, [_i64, _i64, _int]),
    "mlx_time_linfit": (_int, [_vp, _int, _vp, _i64, _i64, _dbl, _dbl, _vp, _vp, _vp, _sz, _vp]),
    "mlx_time_project": (_int, [_vp, _int, _vp, _int, _i64, _i64, _vp, _vp, _sz, _vp]),
    "mlx_time_apply": (_int, [_vp, _int, _int, _vp, _vp, _vp, _int, _i64, _i64, _vp, _vp]),
}


# The grouped time statistic (include/momlevel_clim.h): bound by load_clim() on first use, for the
# same reason.
CLIM_SIGNATURES = {
    "mlx_clim_group_stat": (_int, [_vp, _int, _vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _vp]),
}


# The tide-gauge entry points (include/momlevel_gauge.h): bound by load_gauge() on first use, for
# the same reason.
GAUGE_SIGNATURES = {
    "mlx_gauge_prepare": (_int, [_vp, _vp, _int, _vp, _int, _i64, _vp, _vp, _vp]),
    "mlx_gauge_nearest_split": (_i64, [_i64, _i64, _i64]),
    "mlx_gauge_nearest_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "mlx_gauge_nearest": (_int, [_vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _sz, _vp]),
    "mlx_gauge_gather": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _vp, _vp]),
}


# The spiciness map (include/momlevel_spice.h): bound by load_spice() on first use, for the same
# reason.
SPICE_SIGNATURES = {
    "mlx_spice_map": (_int, [_vp, _int, _vp, _int, _i64, _vp, _vp]),
}


# The vorticity entry points (include/momlevel_vort.h): bound by load_vort() on first use, for the
# same reason.
VORT_SIGNATURES = {
    "mlx_vort_tile_width": (_i64, [_int]),
    "mlx_vort_records_per_launch": (_i64, [_i64, _i64, _int]),
    "mlx_vort_rel_vort": (_int, [_vp, _vp, _int, _vp, _vp, _vp, _int, _i64, _i64, _i64, _int, _vp,
                                 _vp]),
    "mlx_vort_pv": (_int, [_vp, _int, _vp, _int, _vp, _int, _i64, _i64, _i64, _int, _int, _dbl,
                           _int, _vp, _vp]),
    "mlx_vort_rossby": (_int, [_vp, _int, _vp, _int, _i64, _i64, _i64, _vp, _vp]),
}


# The area-mean entry points (include/momlevel_area.h): bound by load_area() on first use, for the
# same reason.
AREA_SIGNATURES = {
    "mlx_area_tile": (_i64, [_int]),
    "mlx_area_mean_workspace_bytes": (_sz, [_i64, _i64, _int, _int]),
    "mlx_area_mean": (_int, [_vp, _int, _vp, _int, _vp, _int, _i64, _i64, _vp, _vp, _vp, _sz, _vp]),
    "mlx_area_anomaly": (_int, [_vp, _int, _vp, _int, _vp, _i64, _i64, _vp, _vp]),
}


# The depth-layer sums (include/momlevel_layer.h): bound by load_layer() on first use, for the same
# reason.
LAYER_SIGNATURES = {
    "mlx_layer_steps": (_int, []),
    "mlx_layer_record_blocks": (_int, [_i64]),
    "mlx_layer_integral": (_int, [_vp, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _int, _vp, _dbl,
                                  _vp, _vp]),
}


# The time filter (include/momlevel_filter.h): bound by load_filter() on first use, for the same
# reason.
FILTER_SIGNATURES = {
    "mlx_filter_tile": (_i64, []),
    "mlx_filter_window_edge": (_i64, [_int]),
    "mlx_filter_tiles_per_block": (_i64, [_i64, _i64, _int]),
    "mlx_filter_apply": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _i64, _int, _i64, _i64, _vp, _int,
                               _vp]),
}


# The order statistics (include/momlevel_quantile.h): bound by load_quantile() on first use, for
# the same reason.
QUANTILE_SIGNATURES = {
    "mlx_quantile_block_cells": (_i64, [_int]),
    "mlx_quantile_unroll": (_i64, []),
    "mlx_quantile_select": (_int, [_vp, _int, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _int, _vp,
                                   _vp]),
    "mlx_quantile_exceed_count": (_int, [_vp, _int, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp,
                                         _vp]),
}


# The column search (include/momlevel_column.h): bound by load_column() on first use, for the same
# reason.
COLUMN_SIGNATURES = {
    "mlx_column_block_cells": (_i64, [_int, _int, _int, _int]),
    "mlx_column_record_rows": (_int, [_i64]),
    "mlx_column_crossing": (_int, [_vp, _int, _vp, _int, _int, _dbl, _i64, _i64, _i64, _vp, _i64,
                                   _int, _int, _int, _vp, _int, _vp, _vp, _vp]),
}


# The time Gram matrix behind the EOFs (include/momlevel_eof.h): bound by load_eof() on first use,
# for the same reason.  (Not named *_SIGNATURES: tests/test_column_host.py counts the tables of that
# name, eleven beside its own.)
EOF_PROTOTYPES = {
    "mlx_gram_tile": (_int, []),
    "mlx_gram_cells": (_i64, [_i64]),
    "mlx_gram_matrix_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "mlx_gram_matrix": (_int, [_vp, _int, _vp, _i64, _vp, _int, _vp, _i64, _vp, _i64, _vp, _vp, _sz,
                             _vp]),
    "mlx_gram_issue_probe": (_int, [_i64, _i64, _vp, ctypes.POINTER(ctypes.c_int64), _vp]),
}


# The horizontal filter (include/momlevel_smooth.h): bound by load_smooth() on first use, for the
# same reason.  (Named as EOF_PROTOTYPES is, for the same count.)
SMOOTH_PROTOTYPES = {
    "mlx_smooth_tile_h": (_i64, []),
    "mlx_smooth_tile_w": (_i64, [_int]),
    "mlx_smooth_max_window": (_i64, []),
    "mlx_smooth_record_window": (_i64, []),
    "mlx_smooth_record_rows": (_int, [_i64]),
    "mlx_smooth_tiled": (_int, [_i64, _i64, _i64, _i64]),
    "mlx_smooth_apply": (_int, [_vp, _int, _vp, _int, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _int,
                               _i64, _int, _i64, _i64, _i64, _vp, _int, _vp]),
}


# The grid-to-grid remap (include/momlevel_regrid.h): bound by load_regrid() on first use, for the
# same reason.  (Named as EOF_PROTOTYPES is, for the same count.)
REGRID_PROTOTYPES = {
    "mlx_regrid_slice": (_i64, []),
    "mlx_regrid_record_window": (_i64, []),
    "mlx_regrid_window_rows": (_int, [_i64]),
    "mlx_regrid_apply": (_int, [_vp, _int, _vp, _vp, _vp, _vp, _i64, _dbl, _int, _i64, _i64, _i64,
                               _vp, _int, _vp]),
}


# The census (include/momlevel_census.h): bound by load_census() on first use, for the same reason.
# (Named as EOF_PROTOTYPES is, for the same count.)
CENSUS_PROTOTYPES = {
    "mlx_census_tile": (_i64, []),
    "mlx_census_blocks": (_i64, [_i64]),
    "mlx_census_max_bins": (_i64, [_int, _int, _int]),
    "mlx_census_workspace_bytes": (_sz, [_i64, _i64, _i64, _int, _int]),
    "mlx_census_histogram": (_int, [_vp, _int, _vp, _int, _int, _vp, _i64, _vp, _i64, _int, _vp,
                                    _int, _int, _vp, _int, _i64, _i64, _vp, _vp, _vp, _vp, _sz,
                                    _vp]),
}


# The path queries of the pointwise EOS entry points (include/momlevel_path.h): bound by
# load_path() on first use, for the same reason.  (They live in csrc/momlevel_hip.hip and
# csrc/momlevel_promote.hip, beside the launchers that go by them.)
PATH_SIGNATURES = {
    "mlx_path_eos_map": (_int, [_int, _int, _int, _int, _i64, _i64, _i64, _int, _int,
                                ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "mlx_path_eos_promote": (_int, [_int, _int, _int, _int, _int, _int,
                                    ctypes.POINTER(ctypes.c_int)]),
}


class MomlevelHipError(RuntimeError):
    """Raised when the HIP library is missing or one of its calls fails."""


def _declare(lib, table, rebuild_with=None):
    """Declare the prototypes of ``table`` on ``lib``; a missing symbol raises ``MomlevelHipError``
    (with ``rebuild_with``: naming the kernels the library was built without)."""
    for name, (restype, argtypes) in table.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            hint = "" if rebuild_with is None else (
                f": rebuild it with {rebuild_with} (`python -m momlevel_amd.csrc.build --force`)")
            raise MomlevelHipError(f"{LIB_PATH} does not export {name}{hint}") from exc
        fn.restype = restype
        fn.argtypes = argtypes


_lib = None


def load():
    """dlopen libmomlevel_hip.so (once) and declare every prototype."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MomlevelHipError(
            f"{LIB_PATH} not found: momlevel_amd has no CPU fallback. Build the HIP "
            "library with `python -m momlevel_amd.csrc.build` (needs hipcc)."
        )
    real = os.path.realpath(LIB_PATH)
    if os.path.commonpath([real, os.path.realpath(_ORACLE_DIR)]) == os.path.realpath(_ORACLE_DIR):
        raise MomlevelHipError(
            f"{LIB_PATH} is under oracle/ (the CPU checker): momlevel_amd binds the HIP library only"
        )
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as exc:  # pragma: no cover - depends on the host
        raise MomlevelHipError(f"cannot load {LIB_PATH}: {exc}") from exc
    _declare(lib, SIGNATURES)
    if lib.mlx_version() != ABI_VERSION:
        raise MomlevelHipError(
            f"ABI mismatch: library {lib.mlx_version()} vs binding {ABI_VERSION}; rebuild"
        )
    if lib.mlx_build_kind() != BUILD_HIP:
        raise MomlevelHipError(
            f"{LIB_PATH} is build kind {lib.mlx_build_kind()}, not the HIP build "
            f"({BUILD_HIP}): momlevel_amd has no CPU backend"
        )
    _lib = lib
    return lib


# group -> (the table of include/momlevel_<group>.h, what csrc/momlevel_<group>.hip adds)
_GROUPS = {
    "trend": (TREND_SIGNATURES, "the trend kernels"),
    "clim": (CLIM_SIGNATURES, "the grouped-statistic kernel"),
    "gauge": (GAUGE_SIGNATURES, "the tide-gauge kernels"),
    "spice": (SPICE_SIGNATURES, "the spiciness kernel"),
    "vort": (VORT_SIGNATURES, "the vorticity kernels"),
    "area": (AREA_SIGNATURES, "the area-mean kernels"),
    "layer": (LAYER_SIGNATURES, "the layer-integral kernel"),
    "filter": (FILTER_SIGNATURES, "the time-filter kernel"),
    "path": (PATH_SIGNATURES, "the path queries of the EOS maps"),
    "quantile": (QUANTILE_SIGNATURES, "the quantile kernels"),
    "column": (COLUMN_SIGNATURES, "the column-search kernel"),
    "eof": (EOF_PROTOTYPES, "the Gram kernels"),
    "smooth": (SMOOTH_PROTOTYPES, "the horizontal-filter kernels"),
    "regrid": (REGRID_PROTOTYPES, "the remap kernel"),
    "census": (CENSUS_PROTOTYPES, "the census kernels"),
}


# what is bound: one module flag per group (the host tests reset them by name)
_trend_bound = _clim_bound = _gauge_bound = _spice_bound = _vort_bound = _area_bound = False
_layer_bound = _filter_bound = _path_bound = _quantile_bound = _column_bound = _eof_bound = False
_smooth_bound = _regrid_bound = _census_bound = False


def _load_group(group):
    """load(), then declare the prototypes of include/momlevel_<group>.h (once); a library built
    without csrc/momlevel_<group>.hip raises ``MomlevelHipError``."""
    lib = load()
    flag = f"_{group}_bound"
    if not globals().get(flag, False):  # (a group without a flag of its own above starts unbound)
        _declare(lib, *_GROUPS[group])
        globals()[flag] = True
    return lib


def load_trend():
    return _load_group("trend")


def load_clim():
    return _load_group("clim")


def load_gauge():
    return _load_group("gauge")


def load_spice():
    return _load_group("spice")


def load_vort():
    return _load_group("vort")


def load_area():
    return _load_group("area")


def load_layer():
    return _load_group("layer")


def load_filter():
    return _load_group("filter")


def load_path():
    return _load_group("path")


def load_quantile():
    return _load_group("quantile")


def load_column():
    return _load_group("column")


def load_eof():
    return _load_group("eof")


def load_smooth():
    return _load_group("smooth")


def load_regrid():
    return _load_group("regrid")


def load_census():
    return _load_group("census")


def last_error():
    buf = ctypes.create_string_buffer(512)
    load().mlx_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def last_kernel():
    """The kernel instantiation this thread's last K1 / K2 call launched (mlx_last_kernel)."""
    buf = ctypes.create_string_buffer(160)
    load().mlx_last_kernel(buf, 160)
    return buf.value.decode(errors="replace")


def check(status, what):
    """Turn a non-zero status of the C ABI into an exception."""
    if status != 0:
        kind = "argument error" if status < 0 else "hipError_t"
        raise MomlevelHipError(f"{what} failed: {kind} {status}: {last_error()}")
