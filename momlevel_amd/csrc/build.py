"""Build libmomlevel_hip.so (gfx950) in-tree with hipcc.

    python -m momlevel_amd.csrc.build [--force]

hipcc cross-compiles without a GPU.  The .so lands in momlevel_amd/ so that it
travels with the source tree (it is git-ignored, not gpurun-ignored).
``-ffp-contract=off`` is REQUIRED: the kernels reproduce the reference's numpy
arithmetic operator for operator (no FMA contraction); see csrc/eos_device.hpp.
"""

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
ROOT = os.path.dirname(PKG)
_TIMED_UNITS = ["momlevel_hip.hip", "momlevel_promote.hip"]
# feature -> what its translation unit csrc/momlevel_<feature>.hip includes, in the order its sha
# hashes them.  One row per feature: SOURCES, DEPENDS and <feature>_source_sha() follow.
FEATURES = {
    "strat": ["eos_device.hpp", "mlx_internal.hpp", "mlx_pack.hpp"],
    "trend": ["eos_device.hpp", "mlx_internal.hpp", "mlx_pack.hpp", "mlx_record.hpp",
              "include/momlevel_trend.h"],
    "clim": ["eos_device.hpp", "mlx_internal.hpp", "mlx_pack.hpp", "mlx_record.hpp",
             "include/momlevel_clim.h"],
    "gauge": ["eos_device.hpp", "mlx_internal.hpp", "mlx_pack.hpp", "mlx_record.hpp",
              "include/momlevel_gauge.h"],
    "spice": ["mlx_internal.hpp", "mlx_pack.hpp", "include/momlevel_spice.h"],
    "vort": ["mlx_internal.hpp", "mlx_pack.hpp", "include/momlevel_vort.h"],
    "area": ["mlx_internal.hpp", "mlx_pack.hpp", "include/momlevel_area.h"],
    "layer": ["mlx_internal.hpp", "mlx_pack.hpp", "include/momlevel_layer.h"],
    "filter": ["eos_device.hpp", "mlx_internal.hpp", "mlx_pack.hpp", "mlx_record.hpp",
               "include/momlevel_filter.h"],
    "quantile": ["eos_device.hpp", "mlx_internal.hpp", "mlx_pack.hpp", "mlx_record.hpp",
                 "include/momlevel_quantile.h"],
    "column": ["eos_device.hpp", "mlx_internal.hpp", "mlx_pack.hpp", "include/momlevel_column.h"],
    "eof": ["eos_device.hpp", "mlx_internal.hpp", "mlx_pack.hpp", "mlx_record.hpp",
            "include/momlevel_eof.h"],
    "smooth": ["mlx_internal.hpp", "mlx_pack.hpp", "include/momlevel_smooth.h"],
    "regrid": ["mlx_internal.hpp", "mlx_pack.hpp", "include/momlevel_regrid.h"],
    "census": ["mlx_internal.hpp", "mlx_pack.hpp", "include/momlevel_census.h"],
}


def _path(name):
    return os.path.join(ROOT, name) if name.startswith("include/") else os.path.join(HERE, name)


def _feature_files(feature):
    return [_path(f"momlevel_{feature}.hip")] + [_path(name) for name in FEATURES[feature]]


SOURCES = [_path(name) for name in _TIMED_UNITS + [f"momlevel_{f}.hip" for f in FEATURES]
           + ["host_copy.cpp"]]
LIB = os.path.join(PKG, "libmomlevel_hip.so")

FLAGS = [
    "--offload-arch=gfx950",
    "-O3",
    "-ffp-contract=off",
    "-fPIC",
    "-shared",
    "-std=c++17",
    "-Wall",
    "-Wno-unused-variable",
    "-Wno-sometimes-uninitialized",
]


# What the timed kernels are built from: the sources of their translation units, the headers
# those include, the public header and the compiler flags.  bench.py and the profile summaries
# stamp this sha on their numbers; a committed counter profile is quoted only while it matches.
TIMED_SOURCES = [
    os.path.join(HERE, "momlevel_hip.hip"),
    os.path.join(HERE, "eos_device.hpp"),
    os.path.join(HERE, "mlx_internal.hpp"),
    os.path.join(HERE, "momlevel_promote.hip"),
    os.path.join(HERE, "eos_promote.hpp"),
    os.path.join(ROOT, "include", "momlevel_hip.h"),
    os.path.join(ROOT, "include", "momlevel_path.h"),
]
# what the library is rebuilt for: every source and header above, and this file
DEPENDS = sorted({*SOURCES, *TIMED_SOURCES, *(p for f in FEATURES for p in _feature_files(f)),
                  os.path.abspath(__file__)})


def source_sha(paths=None, flags=True):
    """sha256 (first 16 hex digits) of ``paths`` (default TIMED_SOURCES) and, with ``flags``, of
    the compiler flags"""
    import hashlib

    h = hashlib.sha256()
    for path in (TIMED_SOURCES if paths is None else paths):
        with open(path, "rb") as f:
            h.update(f.read())
    if flags:
        h.update(" ".join(FLAGS).encode())
    return h.hexdigest()[:16]


def feature_source_sha(feature):
    """a feature's own guard: csrc/momlevel_<feature>.hip (+ what it includes, + flags)"""
    return source_sha(_feature_files(feature))


def strat_source_sha():
    """the stratification kernels' own guard: csrc/momlevel_strat.hip (+ what it includes, + flags)"""
    return feature_source_sha("strat")


def trend_source_sha():
    """the trend kernels' own guard: csrc/momlevel_trend.hip (+ what it includes, + flags)"""
    return feature_source_sha("trend")


def clim_source_sha():
    """the grouped-statistic kernel's own guard: csrc/momlevel_clim.hip (+ what it includes, + flags)"""
    return feature_source_sha("clim")


def gauge_source_sha():
    """the tide-gauge kernels' own guard: csrc/momlevel_gauge.hip (+ what it includes, + flags)"""
    return feature_source_sha("gauge")


def spice_source_sha():
    """the spiciness kernel's own guard: csrc/momlevel_spice.hip (+ what it includes, + flags)"""
    return feature_source_sha("spice")


def vort_source_sha():
    """the vorticity kernels' own guard: csrc/momlevel_vort.hip (+ what it includes, + flags)"""
    return feature_source_sha("vort")


def area_source_sha():
    """the area-mean kernels' own guard: csrc/momlevel_area.hip (+ what it includes, + flags)"""
    return feature_source_sha("area")


def layer_source_sha():
    """the layer-integral kernel's own guard: csrc/momlevel_layer.hip (+ what it includes, + flags)"""
    return feature_source_sha("layer")


def filter_source_sha():
    """the time-filter kernel's own guard: csrc/momlevel_filter.hip (+ what it includes, + flags)"""
    return feature_source_sha("filter")


def quantile_source_sha():
    """the quantile kernels' own guard: csrc/momlevel_quantile.hip (+ what it includes, + flags)"""
    return feature_source_sha("quantile")


def column_source_sha():
    """the column-search kernel's own guard: csrc/momlevel_column.hip (+ what it includes, + flags)"""
    return feature_source_sha("column")


def eof_source_sha():
    """the Gram kernels' own guard: csrc/momlevel_eof.hip (+ what it includes, + flags)"""
    return feature_source_sha("eof")


def smooth_source_sha():
    """the horizontal-filter kernels' own guard: csrc/momlevel_smooth.hip (+ what it includes, + flags)"""
    return feature_source_sha("smooth")


def regrid_source_sha():
    """the remap kernel's own guard: csrc/momlevel_regrid.hip (+ what it includes, + flags)"""
    return feature_source_sha("regrid")


def census_source_sha():
    """the census kernels' own guard: csrc/momlevel_census.hip (+ what it includes, + flags)"""
    return feature_source_sha("census")


def hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found (looked on PATH and in /opt/rocm/bin)")
    return exe


def is_stale():
    if not os.path.exists(LIB):
        return True
    lib_mtime = os.path.getmtime(LIB)
    return any(os.path.getmtime(p) > lib_mtime for p in DEPENDS)


def build(force=False, verbose=False, extra_flags=()):
    """Compile the library if it is missing or older than its sources; return its path."""
    if not force and not is_stale():
        return LIB
    cmd = [hipcc()] + FLAGS + list(extra_flags) + SOURCES + ["-o", LIB + ".tmp"]
    if verbose:
        print(" ".join(cmd), flush=True)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc failed ({res.returncode}):\n{res.stdout}\n{res.stderr}")
    if verbose and res.stderr:
        print(res.stderr)
    os.replace(LIB + ".tmp", LIB)
    return LIB


if __name__ == "__main__":
    path = build(force="--force" in sys.argv, verbose=True)
    print(path)
