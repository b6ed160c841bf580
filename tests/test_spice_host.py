"""CPU: the host side of the spiciness feature -- the numpy restatement against the reference's
vectors within the parity bounds (which guards the fixture and the bounds themselves), the C ABI of
include/momlevel_spice.h (symbols, binding table, argument errors) and the public surface.  No
kernel runs here."""

import ctypes
import importlib
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import spice_numpy as sn
from momlevel_amd import _lib
from test_static_names import _undefined

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "momlevel_spice.h")


# ---- the fixture and the bounds -------------------------------------------------------------------
def test_fixture_holds_the_cases():
    vec, gold = sn.fixture()
    assert set(vec) == {"grid", "int32", "nan", "nan_f32"} | {
        f"{d}_{v}" for d in ("uni", "nrm") for v in sn.VARIANTS}
    assert list(vec["grid"][0].shape) == gold["grid_shape"] == [31, 42]
    for d in ("uni", "nrm"):
        for v, (dt, ds) in sn.VARIANTS.items():
            T, S, pi = vec[f"{d}_{v}"]
            assert T.shape == S.shape == pi.shape == (4096,)
            assert (T.dtype, S.dtype, pi.dtype) == (dt, ds, np.float64)
    assert vec["int32"][0].dtype == np.int32 and vec["int32"][2].dtype == np.float64
    T, S, pi = vec["nan"]
    nT, nS = np.isnan(T), np.isnan(S)
    assert (nT & ~nS).sum() >= 3 and (nS & ~nT).sum() >= 3 and (nT & nS).sum() >= 3
    assert np.array_equal(np.isnan(pi), nT | nS)
    assert np.array_equal(np.isnan(vec["nan_f32"][2]), nT | nS)
    size = os.path.getsize(os.path.join(sn.GOLDEN, "spice_vectors.npz"))
    assert size < 1 << 20


def test_restatement_meets_both_bounds_on_every_vector():
    vec, _ = sn.fixture()
    for name, (T, S, ref) in vec.items():
        got = sn.horner(T, S)
        A = sn.magnitude(T, S)
        lim = sn.bound(T, S)
        ok = ~np.isnan(ref)
        assert np.array_equal(np.isnan(got), ~ok), name
        assert ok.sum() >= 80 and np.all(A[ok] > 0.0), name  # (the bound never degenerates)
        unit = 2.0 ** -24 if np.float32 in (T.dtype, S.dtype) else 2.0 ** -53
        worst = np.max(np.abs(got[ok] - ref[ok]) / (unit * A[ok]))
        print(f"{name:12s} worst |restatement - reference| = {worst:6.2f} units of "
              f"{'2^-24' if unit > 1e-10 else '2^-53'} A   (min A {A[ok].min():.3g})")
        assert np.all(np.abs(got[ok] - ref[ok]) <= lim[ok]), name


def test_restatement_reproduces_the_reference_sum():
    vec, gold = sn.fixture()
    T, S, ref = vec["grid"]
    total = sn.horner(T, S).sum()
    print("sum over the grid:", repr(total), "reference:", repr(gold["grid_sum_reference"]),
          "pinned by the reference's test:", repr(gold["grid_sum"]))
    assert gold["grid_sum_reference"] == ref.sum()
    assert np.allclose(ref.sum(), gold["grid_sum"])  # the reference's own assertion
    assert abs(total - gold["grid_sum"]) <= grid_sum_tolerance(T, S, ref)


def grid_sum_tolerance(T, S, ref):
    """the cells' bounds added up, plus the rounding of two pairwise sums of n terms (numpy's
    sum, once per side: <= (log2 n + 8) u sum |pi| each -- blocks of 8 are summed in sequence)"""
    n = ref.size
    return sn.bound(T, S).sum() + 2.0 * (np.log2(n) + 8.0) * 2.0 ** -53 * np.abs(ref).sum()


def test_table_is_the_papers():
    # the two leading terms of Flament's fit: pi ~ 0.77442 (S - 35) + 0.051655 theta near the origin
    assert sn.B.shape == (6, 5) and sn.B[0][0] == 0.0
    assert sn.B[0][1] == 7.7442e-1 and sn.B[1][0] == 5.1655e-2
    assert sn.horner(np.array([0.0]), np.array([35.0]))[0] == 0.0
    assert sn.magnitude(np.array([0.0]), np.array([36.0]))[0] == pytest.approx(np.abs(sn.B[0]).sum())


# ---- the C ABI ----------------------------------------------------------------------------------
def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_spice_header_binding_and_exports_agree():
    text = _header_text()
    declared = sorted(set(re.findall(r"\b(mlx_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.SPICE_SIGNATURES) == ["mlx_spice_map"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in momlevel_spice.h but not exported"
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                             text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(mlx_spice_[a-z0-9_]+)\b", out))) == declared
    ctype = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p,
             "double *": ctypes.c_void_p, "int64_t ": ctypes.c_int64, "int ": ctypes.c_int}
    protos = re.findall(r"\b(int)\s+(mlx_spice_[a-z_]+)\s*\(([^)]*)\)", text)
    assert [p[1] for p in protos] == declared
    for _, name, args in protos:
        args = [" ".join(a.split()) for a in args.split(",")]
        want = [next(v for k, v in ctype.items() if a.startswith(k)) for a in args]
        restype, argtypes = _lib.SPICE_SIGNATURES[name]
        assert restype is ctypes.c_int and argtypes == want, name
        assert [a.split()[-1].lstrip("*") for a in args] == [
            "theta", "theta_dtype", "so", "so_dtype", "n", "out", "stream"]
    assert "infinite" in open(HEADER).read().lower()  # outside the contract, and said so
    assert _lib.load_spice() is _lib.load()


def test_other_tables_and_the_abi_version_are_untouched():
    for name in _lib.SPICE_SIGNATURES:
        assert name not in _lib.SIGNATURES and name not in _lib.TREND_SIGNATURES
        assert name not in _lib.CLIM_SIGNATURES and name not in _lib.GAUGE_SIGNATURES
    assert len(_lib.SIGNATURES) == 28 and len(_lib.TREND_SIGNATURES) == 4
    assert len(_lib.CLIM_SIGNATURES) == 1 and len(_lib.GAUGE_SIGNATURES) == 5
    assert _lib.ABI_VERSION == 9 and _lib.load().mlx_version() == 9


def test_argument_errors_need_no_gpu():
    lib = _lib.load_spice()
    f = 1 << 20  # 16-byte aligned, non-NULL, never dereferenced: the checks precede every HIP call
    F64, F32 = _lib.DTYPE_F64, _lib.DTYPE_F32

    def call(theta=f, tdt=F64, so=f, sdt=F64, n=10, out=f):
        return lib.mlx_spice_map(theta, tdt, so, sdt, n, out, None)

    for kw in (dict(theta=None), dict(so=None), dict(out=None)):
        assert call(**kw) == -1 and "NULL" in _lib.last_error()
    for kw in (dict(n=-1), dict(n=-(1 << 40)), dict(n=(1 << 38) + 1)):
        assert call(**kw) == -2 and _lib.last_error()
    for bad in (2, 3, 4, 7, -1):  # (MLX_DTYPE_F32_UPCAST and the mixed codes are not operand dtypes)
        assert call(tdt=bad) == -3 and call(sdt=bad) == -3
    assert call(theta=f + 4) == -5 and call(so=f + 4) == -5 and call(out=f + 4) == -5
    assert call(theta=f + 2, tdt=F32) == -5 and call(so=f + 1, sdt=F32) == -5
    # element alignment is all that is asked of float32 operands
    assert call(theta=f + 4, tdt=F32, so=f + 12, sdt=F32, n=0) == 0
    # n == 0: nothing to do, nothing launched, whatever the pointers
    assert call(n=0) == 0 and call(theta=None, so=None, out=None, n=0) == 0


def test_a_library_without_the_kernel_is_an_error(monkeypatch):
    class Bare:
        def __getattr__(self, name):
            raise AttributeError(name)

    monkeypatch.setattr(_lib, "_spice_bound", False)
    monkeypatch.setattr(_lib, "load", lambda: Bare())
    with pytest.raises(_lib.MomlevelHipError, match="does not export mlx_spice_map: rebuild"):
        _lib.load_spice()


def test_spice_source_sha_is_its_own():
    from momlevel_amd.csrc import build

    assert len(build.spice_source_sha()) == 16
    assert build.spice_source_sha() not in (build.source_sha(), build.trend_source_sha(),
                                            build.clim_source_sha(), build.strat_source_sha(),
                                            build.gauge_source_sha())
    names = {os.path.basename(p) for p in build.TIMED_SOURCES}
    assert "momlevel_spice.hip" not in names and "momlevel_spice.h" not in names
    assert any(p.endswith("momlevel_spice.hip") for p in build.SOURCES)
    assert any(p.endswith("momlevel_spice.hip") for p in build.DEPENDS)
    assert any(p.endswith("momlevel_spice.h") for p in build.DEPENDS)


# ---- the public surface ---------------------------------------------------------------------------
def test_exports():
    import momlevel_amd
    from momlevel_amd import core, derived
    from momlevel_amd.spice import flament

    assert momlevel_amd.spice.flament is flament and "spice" in momlevel_amd.__all__
    assert flament.__all__ == ["spice"]
    assert list(inspect.signature(flament.spice).parameters) == ["thetao", "so"]
    assert "calc_spice" in derived.__all__
    assert list(inspect.signature(derived.calc_spice).parameters) == ["thetao", "so"]
    assert list(inspect.signature(core.spice_map).parameters) == ["theta", "so", "out"]
    assert "spiciness" not in momlevel_amd.__doc__.split("Everything else")[1]
    assert "momlevel_spice.h" in momlevel_amd.__doc__
    for mod in ("momlevel_amd.spice.flament", "momlevel_amd.derived", "momlevel_amd.core",
                "momlevel_amd.eos._dispatch"):
        assert _undefined(importlib.import_module(mod)) == []


def test_the_host_pipeline_takes_its_kernel():
    from momlevel_amd.eos import _dispatch

    assert list(inspect.signature(_dispatch._host_pipeline).parameters) == ["operands", "kernel"]
    # one pipeline: the EOS entry is a caller of it, and so is spice()
    assert "_host_pipeline(" in inspect.getsource(_dispatch._evaluate_host_chunked)
    from momlevel_amd.spice import flament
    assert "_dispatch._host_pipeline(" in inspect.getsource(flament.spice)
    assert "Uploader" not in inspect.getsource(flament)
    # ... and that evaluator is a caller of the one loop, which takes ITS kernel as an argument too
    from momlevel_amd import hostio
    assert "hostio.pipeline_rows(" in inspect.getsource(_dispatch._host_pipeline)
    assert "Uploader" not in inspect.getsource(_dispatch)
    assert list(inspect.signature(hostio.pipeline_rows).parameters) == [
        "bounds", "device", "stage", "kernel", "out"]
