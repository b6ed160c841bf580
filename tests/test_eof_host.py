"""CPU: the C ABI of include/momlevel_eof.h (symbols, binding table, geometry queries, argument
errors), the host rules of momlevel_amd.eof (sign rule, North's errors, variance fractions,
refusals) and the numpy restatement tests/eof_numpy.py against a direct SVD and, on the record of
tests/eof_cases.py, against its own recomputation in long double.  No GPU."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import eof_cases as ec
import eof_numpy as en
import momlevel_amd
from momlevel_amd import _lib, core, eof
from momlevel_amd.labeled import DataArray, Dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "momlevel_eof.h")
NAMES = ["mlx_gram_cells", "mlx_gram_issue_probe", "mlx_gram_matrix",
         "mlx_gram_matrix_workspace_bytes", "mlx_gram_tile"]


# ---- the C ABI ----------------------------------------------------------------------------------
def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_eof_header_binding_and_exports_agree():
    text = _header_text()
    declared = sorted(set(re.findall(r"\b(mlx_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.EOF_PROTOTYPES) == NAMES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in momlevel_eof.h but not exported"
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                             text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(mlx_gram_[a-z0-9_]+)\b", out))) == declared
    ctype = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p,
             "const double *": ctypes.c_void_p, "double *": ctypes.c_void_p,
             "int64_t *": ctypes.POINTER(ctypes.c_int64), "int64_t ": ctypes.c_int64,
             "size_t ": ctypes.c_size_t, "int ": ctypes.c_int}
    rtype = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}
    protos = re.findall(r"\b(int|int64_t|size_t)\s+(mlx_[a-z_]+)\s*\(([^)]*)\)", text)
    assert sorted(p[1] for p in protos) == declared
    for ret, name, args in protos:
        args = [" ".join(a.split()) for a in args.split(",")]
        want = [] if args == ["void"] else [next(v for k, v in ctype.items() if a.startswith(k))
                                           for a in args]
        restype, argtypes = _lib.EOF_PROTOTYPES[name]
        assert restype is rtype[ret] and argtypes == want, name
        if ret == "int" and want:
            assert args[-1] == "void *stream", name  # the caller's stream last
    for name, val in re.findall(r"#define MLX_(GRAM_[A-Z_]+)\s+(\d+)", text):
        assert getattr(_lib, name) == int(val) == getattr(core, name), name
    assert _lib.load_eof() is _lib.load()


def test_other_tables_and_the_abi_version_are_untouched():
    others = [v for k, v in vars(_lib).items() if k.endswith("SIGNATURES")]
    assert len(others) == 12  # (every other table; this header's own is EOF_PROTOTYPES)
    for name in _lib.EOF_PROTOTYPES:
        for table in others:
            assert name not in table
    assert len(_lib.SIGNATURES) == 28 and len(_lib.TREND_SIGNATURES) == 4
    assert _lib.ABI_VERSION == 9 and _lib.load().mlx_version() == 9
    assert _lib._GROUPS["eof"][0] is _lib.EOF_PROTOTYPES
    # every entry point of the header carries its own prefix: mlx_time_ stays the trend header's
    assert all(name.startswith("mlx_gram_") for name in _lib.EOF_PROTOTYPES)
    assert "MLX_ABI_VERSION" not in open(HEADER).read().replace("do not move MLX_ABI_VERSION", "")


def test_the_ranges_are_a_function_of_n_alone():
    lib = _lib.load_eof()
    tile = core.gram_tile()
    assert tile == lib.mlx_gram_tile() and tile % 16 == 0 and tile >= 16
    base = core.gram_cells(1)
    assert base % 16 == 0 and base >= 16
    split = _lib.GRAM_MAX_SPLIT
    for n in (1, 2, base - 1, base, base + 1, split * base):
        assert core.gram_cells(n) == base
    for n in (split * base + 1, 1080 * 1440, (1 << 38) - 5, 1 << 38):
        cells = core.gram_cells(n)
        assert cells % 16 == 0 and cells >= base
        assert -(-n // cells) <= split < -(-n // (cells - 16))  # (the smallest such multiple of 16)
    assert core.gram_cells(0) == 0 and core.gram_cells(-3) == 0
    # 8 bytes per element of a tile, tile pair and range; nt2 == 0 asks for the symmetric form
    ws = lib.mlx_gram_matrix_workspace_bytes
    per = 8 * tile * tile
    assert ws(1, 0, 1) == per and ws(tile, 0, base) == per and ws(tile + 1, 0, base) == 3 * per
    assert ws(tile + 1, 0, base + 1) == 6 * per and ws(2 * tile + 5, 0, 3 * base + 7) == 6 * 4 * per
    assert ws(tile + 1, 1, 5) == 2 * per and ws(3, 2 * tile + 1, 2 * base) == 3 * 2 * per
    n = 1080 * 1440
    assert ws(1200, 0, n) == 55 * -(-n // core.gram_cells(n)) * per  # (10 row tiles: 55 pairs)
    for bad in ((0, 0, 5), (-1, 0, 5), (4, -1, 5), (4, 0, 0), (4, 0, -2), (1 << 31, 0, 1),
                (4, 1 << 31, 1), (4, 0, (1 << 38) + 1), (1 << 30, 0, 1 << 30), (1 << 22, 0, 4)):
        assert ws(*bad) == 0, bad


def gram_call(lib, **kw):
    """mlx_gram_matrix with arguments that pass every check (pointers that are never dereferenced:
    the checks precede every HIP call), ``kw`` replacing some"""
    f = 1 << 20
    a = dict(y1=f, dt1=_lib.DTYPE_F64, c1=f, nt1=5, y2=f, dt2=_lib.DTYPE_F32, c2=f, nt2=3, scale=f,
             n=10, G=f, ws=f, nbytes=1 << 40)
    a.update(kw)
    return lib.mlx_gram_matrix(a["y1"], a["dt1"], a["c1"], a["nt1"], a["y2"], a["dt2"], a["c2"],
                             a["nt2"], a["scale"], a["n"], a["G"], a["ws"], a["nbytes"], None)


F = 1 << 20
REFUSALS = [
    (dict(dt1=2), -3), (dict(dt1=-1), -3), (dict(dt2=3), -3), (dict(dt2=7), -3),
    (dict(dt1=4, y2=None), -3),
    (dict(nt1=0), -2), (dict(nt1=-4), -2), (dict(nt2=0), -2), (dict(nt2=-1), -2), (dict(n=0), -2),
    (dict(n=-7), -2), (dict(nt1=0, y2=None), -2),
    (dict(nt1=1 << 31), -2), (dict(nt2=1 << 31), -2), (dict(n=(1 << 38) + 1), -2),
    (dict(nt1=1 << 30, n=1 << 30), -2), (dict(nt2=1 << 30, n=1 << 30), -2),
    (dict(nt1=1 << 22, nt2=1 << 22, n=4), -2),  # (too many tile pairs for one grid)
    (dict(y1=None), -1), (dict(G=None), -1), (dict(ws=None), -1),
    (dict(nbytes=0), -4), (dict(nbytes=2047), -4), (dict(ws=F + 4), -4),
    (dict(y1=F + 4), -5), (dict(y1=F + 2, dt1=1), -5), (dict(y2=F + 2), -5),
    (dict(y2=F + 4, dt2=0), -5), (dict(c1=F + 4), -5), (dict(c2=F + 4), -5), (dict(scale=F + 4), -5),
    (dict(G=F + 4), -5),
]


def test_argument_errors_need_no_gpu():
    lib = _lib.load_eof()
    for kw, code in REFUSALS:
        assert gram_call(lib, **kw) == code and _lib.last_error(), kw
    assert "NULL" in (gram_call(lib, G=None), _lib.last_error())[1]
    assert "workspace" in (gram_call(lib, nbytes=8), _lib.last_error())[1]
    assert gram_call(lib, nbytes=lib.mlx_gram_matrix_workspace_bytes(5, 3, 10) - 1) == -4
    # the symmetric form ignores nt2, dtype2 and center2
    need = lib.mlx_gram_matrix_workspace_bytes(5, 0, 10)
    assert gram_call(lib, y2=None, dt2=9, nt2=-3, c2=F + 4, nbytes=need - 8) == -4
    # a float32 record needs its own alignment only; the maps are optional
    assert gram_call(lib, y1=F + 4, dt1=1, c1=None, c2=None, scale=None, nbytes=0) == -4
    # the probe's own refusals
    probe = lib.mlx_gram_issue_probe
    assert probe(0, 1, F, None, None) == -2 and probe(1, 0, F, None, None) == -2
    assert probe(1, (1 << 20) + 1, F, None, None) == -2
    assert probe(1, 1, None, None, None) == -1 and probe(1, 1, F + 4, None, None) == -5


def test_a_library_without_the_kernels_is_an_error(monkeypatch):
    class Bare:
        def __getattr__(self, name):
            raise AttributeError(name)

    monkeypatch.setattr(_lib, "_eof_bound", False)
    monkeypatch.setattr(_lib, "load", lambda: Bare())
    with pytest.raises(_lib.MomlevelHipError, match="does not export mlx_[a-z_]+: rebuild"):
        _lib.load_eof()


def test_features_has_the_row_and_a_sha_of_its_own():
    from momlevel_amd.csrc import build

    assert build.FEATURES["eof"] == ["eos_device.hpp", "mlx_internal.hpp", "mlx_pack.hpp",
                                     "mlx_record.hpp", "include/momlevel_eof.h"]
    assert len(build.eof_source_sha()) == 16
    assert build.eof_source_sha() == build.feature_source_sha("eof")
    assert build.eof_source_sha() not in (build.source_sha(), build.area_source_sha(),
                                          build.trend_source_sha(), build.column_source_sha())
    names = {os.path.basename(p) for p in build.TIMED_SOURCES}
    assert "momlevel_eof.hip" not in names and "momlevel_eof.h" not in names
    assert any(p.endswith("momlevel_eof.hip") for p in build.SOURCES)
    assert any(p.endswith("momlevel_eof.h") for p in build.DEPENDS)
    text = open(os.path.join(ROOT, "momlevel_amd", "csrc", "momlevel_eof.hip")).read()
    assert "#pragma clang fp contract(off)" in text and "atomic" not in text.replace("atomics", "")
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in text and "record_fits" in text
    assert "(lane >> 4) + 4 * r" in text  # the float64 C/D row map, not 4 * (lane >> 4) + r


def test_the_new_core_functions_take_no_result_buffer():
    import inspect

    for name in ("gram_tile", "gram_cells", "time_gram", "gram_issue_probe"):
        params = inspect.signature(getattr(core, name)).parameters
        assert not any(p == "out" or p.endswith("_out") for p in params), name
    assert list(inspect.signature(core.time_gram).parameters) == ["y1", "y2", "center1", "center2",
                                                                  "scale"]


# ---- the host rules ---------------------------------------------------------------------------------
def test_the_sign_rule():
    pcs = np.array([[1.0, -3.0, 2.0, 0.5], [-2.0, 1.0, -2.0, -0.5], [0.5, 3.0, 1.0, 0.25]])
    out = eof.fix_signs(pcs)
    # column 0: largest |.| is -2 -> flipped; 1: the tie |-3| = |3| goes to index 0 -> flipped;
    # 2: the tie 2 = |-2| goes to index 0, positive -> kept; 3: the tie goes to index 0 -> kept
    assert np.array_equal(out, pcs * np.array([-1.0, -1.0, 1.0, 1.0]))
    assert np.array_equal(eof.fix_signs(out), out) and out is not pcs
    assert np.array_equal(en.fix_signs(pcs), out)


def test_north_errors_fractions_and_the_decomposition():
    rng = np.random.default_rng(2)
    a = rng.normal(size=(9, 40))
    a -= a.mean(axis=0)
    cov = a @ a.T / 8
    lam, frac, err, pcs = eof.decompose(cov, 4, ddof=1)
    ref = np.linalg.eigvalsh(cov)[::-1]
    assert np.allclose(lam, ref[:4], rtol=1e-13, atol=0) and np.all(np.diff(lam) < 0)
    assert np.allclose(frac, ref[:4] / ref.sum(), rtol=1e-12) and frac.sum() < 1.0
    assert np.array_equal(err, lam * np.sqrt(2.0 / 9)) and np.array_equal(err, eof.north_error(lam, 9))
    assert pcs.shape == (9, 4)
    assert np.allclose(pcs.T @ pcs / 8, np.eye(4), atol=1e-13)  # unit variance, orthogonal
    assert np.allclose(cov @ pcs, pcs * lam, atol=1e-12 * lam[0])
    for k in range(4):
        assert pcs[np.argmax(np.abs(pcs[:, k])), k] > 0
    _, frac_all, _, _ = eof.decompose(cov, 8)
    assert abs(frac_all.sum() - 1.0) < 1e-12  # (the ninth eigenvalue of centred data is 0)


def test_the_area_scale():
    area = np.array([[4.0, 0.0, -1.0], [np.nan, 9.0, 2.25]])
    s = eof.area_scale(area, (2, 3))
    assert s.dtype == np.float64 and s.shape == (6,)
    assert np.array_equal(s[[0, 4, 5]], [2.0, 3.0, 1.5]) and np.isnan(s[[1, 2, 3]]).all()
    assert np.array_equal(eof.area_scale(DataArray(area.astype(np.float32), ("yh", "xh")), (2, 3)),
                          s, equal_nan=True)
    assert eof.area_scale(None, (2, 3)) is None
    with pytest.raises(ValueError, match="does not cover"):
        eof.area_scale(area, (3, 2))
    _, ref = en.cell_maps(np.zeros((2, 2, 3)), area)
    assert np.array_equal(ref, s, equal_nan=True)


def _record():
    rng = np.random.default_rng(8)
    time = DataArray(np.arange(6.0), ("time",), None, {"axis": "T"}, "time")
    eta = DataArray(rng.normal(size=(6, 4, 5)), ("time", "yh", "xh"), {"time": time},
                    {"units": "m"}, "zos")
    return eta, np.ones((4, 5))


def test_refusals_come_before_any_device_work(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(eof.core, "require_device", boom)
    monkeypatch.setattr(eof.engine, "device_of", boom)
    eta, area = _record()
    for neofs in (6, 7, 0, -1):
        with pytest.raises(ValueError, match="neofs must be 1 .. nt - 1 = 5"):
            eof.calc_eofs(eta, area, neofs=neofs)
    with pytest.raises(ValueError, match="'time' must be the leading dim"):
        eof.calc_eofs(DataArray(np.zeros((4, 6, 5)), ("yh", "time", "xh")), neofs=2)
    with pytest.raises(ValueError, match="'time' must be the leading dim"):
        eof.time_covariance(DataArray(np.zeros((4, 5, 6)), ("yh", "xh", "time")))
    with pytest.raises(ValueError, match="no 'time'"):
        eof.time_covariance(DataArray(np.zeros((6, 4, 5)), ("t", "yh", "xh")))
    with pytest.raises(ValueError, match="no 't'"):
        eof.calc_eofs(eta, tcoord="t")
    for bad in (np.ones((5, 4)), np.ones((4, 5, 1)), np.ones(20), np.ones((6, 4, 5))):
        with pytest.raises(ValueError, match="areacello .* does not cover"):
            eof.calc_eofs(eta, bad, neofs=2)
        with pytest.raises(ValueError, match="areacello .* does not cover"):
            eof.time_covariance(eta, bad)
        with pytest.raises(ValueError, match="areacello .* does not cover"):
            eof.project_field(eta, np.zeros((2, 4, 5)), bad)
    with pytest.raises(ValueError, match="ddof"):
        eof.time_covariance(eta, ddof=2)
    with pytest.raises(ValueError, match="no covariance"):
        eof.time_covariance(DataArray(np.zeros((1, 4, 5)), ("time", "yh", "xh")))
    with pytest.raises(ValueError, match=r"eofs .* must be \(mode,\)"):
        eof.project_field(eta, np.zeros((2, 5, 4)))
    with pytest.raises(ValueError, match="center .* does not cover"):
        eof.project_field(eta, np.zeros((2, 4, 5)), center=np.zeros((5, 4)))
    with pytest.raises(TypeError):
        eof.calc_eofs(Dataset({"zos": eta}))
    with pytest.raises(TypeError):
        eof.calc_eofs([[1.0, 2.0]])
    with pytest.raises(TypeError):
        eof.calc_eofs(eta.astype(np.float16), neofs=2)


def test_the_module_is_published():
    assert momlevel_amd.eof is eof and "eof" in momlevel_amd.__all__
    assert eof.__all__ == ["calc_eofs", "project_field", "time_covariance"]
    for f in (eof.time_covariance, eof.calc_eofs, eof.project_field):
        assert "EXTENSION" in f.__doc__
    assert "unpinned" in eof.time_covariance.__doc__
    assert "nt * 2**-53 * max|P|" in eof.calc_eofs.__doc__  # the uncentred term is stated
    assert eof.MODES_PER_PASS == _lib.TREND_MAX_TERMS == 8


def test_no_undefined_globals_in_the_new_module():
    from test_static_names import _undefined

    assert _undefined(eof) == []


# ---- the restatement against a direct SVD -----------------------------------------------------------
def test_the_restatement_against_an_svd_of_the_weighted_anomalies():
    rng = np.random.default_rng(11)
    nt, n = 12, 30
    y = rng.normal(1.0, 2.0, (nt, 5, 6))
    y[:, 0, 0] = np.nan  # land
    y[4, 2, 3] = np.nan  # one missing step: the cell is left out
    area = rng.uniform(1.0, 3.0, (5, 6))
    area[1, 1] = np.nan
    area[3, 4] = 0.0
    flat = y.reshape(nt, n)
    used = ~np.isnan(flat).any(axis=0) & (area.reshape(-1) > 0)
    assert used.sum() == n - 4
    anom = flat[:, used] - flat[:, used].mean(axis=0)
    X = anom * np.sqrt(area.reshape(-1)[used])
    U, sv, Vt = np.linalg.svd(X, full_matrices=False)
    lam = sv ** 2 / (nt - 1)

    r = en.calc_eofs(y, area, neofs=nt - 1)
    assert np.allclose(r["eigenvalues"], lam[:nt - 1], rtol=1e-12, atol=1e-13 * lam[0])
    assert np.allclose(r["variance_fraction"], lam[:nt - 1] / lam.sum(), rtol=1e-12, atol=1e-13)
    assert np.array_equal(r["eigenvalue_error"], r["eigenvalues"] * np.sqrt(2.0 / nt))
    pcs_svd = en.fix_signs(U[:, :nt - 1] * np.sqrt(nt - 1))
    assert (-np.diff(lam[:nt])).min() > 1e-3 * lam[0]  # (no near-degenerate pair: the pcs are pinned)
    assert np.allclose(r["pcs"], pcs_svd, atol=1e-9)
    # nt - 1 modes span every centred series: the maps reproduce the anomalies of every complete
    # cell, the two without weight included
    eofs = r["eofs"].reshape(nt - 1, n)
    full = ~np.isnan(flat).any(axis=0)
    whole = flat[:, full] - flat[:, full].mean(axis=0)
    assert np.abs(r["pcs"] @ eofs[:, full] - whole).max() <= 1e-12 * np.abs(whole).max()
    assert np.isnan(eofs[:, np.isnan(flat).any(axis=0)]).all()
    assert not np.isnan(eofs[:, ~np.isnan(flat).any(axis=0)]).any()
    # weighted orthogonality of the maps: sum_c area E_j E_k = lambda_k delta_jk
    w = area.reshape(-1)[used]
    gram = (eofs[:, used] * w) @ eofs[:, used].T
    assert np.allclose(gram, np.diag(lam[:nt - 1]), atol=1e-12 * lam[0])
    # projecting the record onto its own maps returns its pcs
    ppc = en.project_field(y, r["eofs"][:4], area)
    assert np.abs(ppc - r["pcs"][:, :4]).max() <= 1e-10
    # the module's host half makes the same numbers of the same matrix
    lam2, frac2, err2, pcs2 = eof.decompose(en.time_covariance(y, area), nt - 1)
    assert np.array_equal(lam2, r["eigenvalues"]) and np.array_equal(pcs2, r["pcs"])
    assert np.array_equal(frac2, r["variance_fraction"]) and np.array_equal(err2, r["eigenvalue_error"])


# ---- the restatement against itself in long double, at the size the kernel splits ------------------
LD = np.longdouble


def _ld_gram(y1, y2, center1, center2, scale):
    """en.time_gram with b and the sum over the cells in long double.  Excluded cells are dropped
    instead of zeroed, and the symmetric form is summed block row by block row above the diagonal
    and mirrored; einsum, which is several times quicker than matmul without a BLAS: this keeps the
    test to a few seconds."""
    flat = lambda a: np.asarray(a).reshape(np.shape(a)[0], -1)  # noqa: E731
    keep = ~np.isnan(center1) & ~np.isnan(scale)
    if y2 is not None:
        keep &= ~np.isnan(center2)
    s = scale[keep].astype(LD)
    b1 = (flat(y1)[:, keep].astype(LD) - center1[keep].astype(LD)[None, :]) * s[None, :]
    if y2 is not None:
        b2 = (flat(y2)[:, keep].astype(LD) - center2[keep].astype(LD)[None, :]) * s[None, :]
        return np.einsum("sc,tc->st", b1, b2)
    nt = b1.shape[0]
    G = np.zeros((nt, nt), dtype=LD)
    for i in range(0, nt, 16):
        G[i:i + 16, i:] = np.einsum("sc,tc->st", b1[i:i + 16], b1[i:])
    return np.triu(G) + np.triu(G, 1).T


def _ld_center(y):
    """en.cell_maps' per-cell mean, summed in long double (NaN where any step is missing)"""
    flat = y.reshape(y.shape[0], -1)
    full = ~np.isnan(flat).any(axis=0)
    center = np.full(flat.shape[1], np.nan, dtype=LD)
    center[full] = (flat[:, full].astype(LD) * (LD(1) / y.shape[0])).sum(axis=0)
    return center


def _ld_calc_eofs(y, area, neofs):
    """en.calc_eofs step for step, the Gram sum and the maps in long double, eigh on the float64
    cast of the covariance matrix"""
    nt = y.shape[0]
    center, scale = _ld_center(y), en.cell_maps(y, area)[1]
    cov = _ld_gram(y, None, center, None, scale) / (nt - 1)
    lam, vec = np.linalg.eigh(cov.astype(np.float64))
    lam, vec = lam[::-1], vec[:, ::-1]
    pcs = en.fix_signs(vec[:, :neofs] * np.sqrt(nt - 1))
    full = ~np.isnan(center)
    eofs = np.full((neofs, center.size), np.nan, dtype=LD)
    anom = y.reshape(nt, -1)[:, full].astype(LD) - center[full][None, :]
    eofs[:, full] = np.einsum("tk,tc->kc", pcs.astype(LD), anom) / (nt - 1)
    return {"cov": cov, "eigenvalues": lam[:neofs].copy(),
            "variance_fraction": lam[:neofs] / np.trace(cov.astype(np.float64)), "pcs": pcs,
            "eofs": eofs.reshape((neofs,) + y.shape[1:])}


def _ld_project_field(y, eofs, area, center=None):
    """en.project_field with both Gram sums in long double"""
    nmode = eofs.shape[0]
    scale = en.cell_maps(y, area)[1]
    cen = _ld_center(y) if center is None else np.asarray(center).reshape(-1)
    land = np.where(np.isnan(eofs.reshape(nmode, -1)).any(axis=0), np.nan, 0.0)
    num = _ld_gram(y, eofs, cen, land, scale)
    den = _ld_gram(eofs, None, np.where(np.isnan(cen), np.nan, land), None, scale)
    return num / np.diag(den)[None, :]


@pytest.mark.skipif(np.finfo(LD).nmant < 63, reason="long double is no wider than double here")
def test_the_restatement_sits_a_tenth_inside_the_gates_of_the_size_case():
    """tests/test_gpu_eof_sizes.py gates the GPU against tests/eof_numpy.py in float64 on the record
    of tests/eof_cases.py.  Those gates mean something only if the restatement's OWN rounding at
    that size is well inside them: here it is recomputed with the Gram sums and the maps in long
    double (64-bit significand), and the float64 restatement must differ from that by at most one
    tenth of each gate -- which leaves the kernel its own rounding of the same order.

    Nothing of the planted case had to be changed to meet the tenth.  Observed, as fractions of a
    TENTH of the gate (1.0 would just pass): covariance 1.4e-4, eigenvalues 2.5e-5, variance
    fractions 3.3e-5, planted pcs 3.6e-5, planted eofs 1.4e-5, pseudo-PCs of the record 2.2e-3,
    pseudo-PCs of the other period 1.9e-3.  The pseudo-PCs of both sides are taken onto the SAME
    maps (the restatement's), as the GPU test does: the eight noise modes are near-degenerate, and
    their maps are not pinned by any gate."""
    nt = core.gram_tile() + 5
    y, area = ec.planted(nt)
    n = y[0].size
    assert core.gram_cells(n) > core.gram_cells(1)
    assert -(-n // core.gram_cells(n)) == _lib.GRAM_MAX_SPLIT  # (the size the GPU test runs at)
    ref, ld = en.calc_eofs(y, area, neofs=ec.NEOFS), _ld_calc_eofs(y, area, ec.NEOFS)
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    lam1 = ref["eigenvalues"][0]
    for k in range(3):  # (the condition on the input that the eigenvector gates rest on)
        assert ref["eigenvalues"][k] - ref["eigenvalues"][k + 1] >= lam1 / 10
    cov = en.time_covariance(y, area)
    ratios = {"covariance": np.abs(f64(cov - ld["cov"])).max() / (ec.GATE_COV * np.abs(cov).max()),
              "eigenvalues": np.abs(ref["eigenvalues"] - ld["eigenvalues"]).max()
              / (ec.GATE_LAMBDA * lam1),
              "variance fractions": np.abs(ref["variance_fraction"] - ld["variance_fraction"]).max()
              / ec.GATE_LAMBDA}
    assert np.array_equal(np.isnan(ref["eofs"]), np.isnan(ld["eofs"]))
    pcs = max(np.abs(ref["pcs"][:, k] - ld["pcs"][:, k]).max() / np.abs(ref["pcs"][:, k]).max()
              for k in range(3))
    maps = max(np.nanmax(np.abs(f64(ref["eofs"][k] - ld["eofs"][k])))
               / np.nanmax(np.abs(ref["eofs"][k])) for k in range(3))
    ratios["planted pcs"], ratios["planted eofs"] = pcs / ec.GATE_MODES, maps / ec.GATE_MODES
    own = en.project_field(y, ref["eofs"], area)
    want = _ld_project_field(y, ref["eofs"], area)
    ratios["pseudo-PCs, the record"] = np.abs(f64(own - want)).max() / ec.GATE_PPC
    center = en.cell_maps(y)[0].reshape(y.shape[1:])
    other = y[ec.OTHER_PERIOD] + ec.OTHER_SHIFT
    got = en.project_field(other, ref["eofs"], area, center=center)
    want = _ld_project_field(other, ref["eofs"], area, center=center)
    ratios["pseudo-PCs, another period"] = np.abs(f64(got - want)).max() / ec.GATE_PPC
    for name, r in ratios.items():
        print(f"{name}: float64 restatement against long double = {10 * r:.2e} of a tenth of "
              "the gate")
    for name, r in ratios.items():
        assert r <= 0.1, (name, r)
