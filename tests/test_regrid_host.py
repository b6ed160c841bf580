"""CPU: the C ABI of include/momlevel_regrid.h (symbols, binding table, geometry queries, argument
errors -- they precede every HIP call), the table builders, the packed layout and the refusals of
momlevel_amd.regrid, and the numpy restatement tests/regrid_numpy.py by hand and against scipy's
sparse product.  No GPU."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import momlevel_amd
import regrid_numpy as rn
from momlevel_amd import _lib, core, regrid
from momlevel_amd.labeled import DataArray, Dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "momlevel_regrid.h")
NAMES = ["mlx_regrid_apply", "mlx_regrid_record_window", "mlx_regrid_slice", "mlx_regrid_window_rows"]
U = 2.0 ** -53


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


# ---- the C ABI ----------------------------------------------------------------------------------
def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_regrid_header_binding_and_exports_agree():
    text = _header_text()
    declared = sorted(set(re.findall(r"\b(mlx_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.REGRID_PROTOTYPES) == NAMES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in momlevel_regrid.h but not exported"
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                             text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(mlx_regrid_[a-z0-9_]+)\b", out))) == declared
    ctype = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p,
             "const double *": ctypes.c_void_p, "const int64_t *": ctypes.c_void_p,
             "const int32_t *": ctypes.c_void_p, "int64_t ": ctypes.c_int64, "int ": ctypes.c_int,
             "double ": ctypes.c_double}
    rtype = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    protos = re.findall(r"\b(int|int64_t)\s+(mlx_[a-z_]+)\s*\(([^)]*)\)", text)
    assert sorted(p[1] for p in protos) == declared
    for ret, name, args in protos:
        args = [" ".join(a.split()) for a in args.split(",")]
        want = [] if args == ["void"] else [next(v for k, v in ctype.items() if a.startswith(k))
                                           for a in args]
        restype, argtypes = _lib.REGRID_PROTOTYPES[name]
        assert restype is rtype[ret] and argtypes == want, name
    assert protos[-1][1] == "mlx_regrid_apply" and protos[-1][2].split(",")[-1].strip() == "void *stream"
    flags = dict(re.findall(r"#define MLX_(REGRID_[A-Z_]+)\s+(\d+)", text))
    assert flags == {"REGRID_PROPAGATE": "1", "REGRID_NO_RENORM": "2"}
    assert (_lib.REGRID_PROPAGATE, _lib.REGRID_NO_RENORM) == (rn.PROPAGATE, rn.NO_RENORM) == (1, 2)
    assert _lib.load_regrid() is _lib.load()


def test_other_tables_and_the_abi_version_are_untouched():
    others = [v for k, v in vars(_lib).items() if k.endswith("SIGNATURES")]
    for name in _lib.REGRID_PROTOTYPES:
        for table in others + [_lib.EOF_PROTOTYPES, _lib.SMOOTH_PROTOTYPES]:
            assert name not in table
    assert len(_lib.SIGNATURES) == 28 and len(_lib.SMOOTH_PROTOTYPES) == 7
    assert _lib.ABI_VERSION == 9 and _lib.load().mlx_version() == 9
    assert _lib._GROUPS["regrid"][0] is _lib.REGRID_PROTOTYPES
    assert "MLX_ABI_VERSION" not in open(HEADER).read().replace("does not move MLX_ABI_VERSION", "")


def test_geometry_queries():
    lib = _lib.load_regrid()
    assert core.regrid_slice() == lib.mlx_regrid_slice() == 64  # one lane per destination of a wave
    assert core.regrid_record_window() == lib.mlx_regrid_record_window() >= 1


def test_launch_queries_are_plain_arithmetic():
    """a block row per window of records up to the cap"""
    rows, R = core.regrid_window_rows, core.regrid_record_window()
    cap = rows(1 << 30)
    assert 1 < cap <= 65535 and rows(1 << 38) == cap
    assert rows(1) == rows(R) == 1 and rows(R + 1) == 2
    for nwin in (2, 1000, cap - 1, cap):
        assert rows(R * nwin) == nwin and rows(R * (nwin - 1) + 1) == nwin
    assert rows(R * cap + 1) == rows(R * cap + R + 1) == cap
    assert rows(0) == 0 and rows(-5) == 0 and rows((1 << 38) + 1) == 0
    assert _lib.load_regrid().mlx_regrid_window_rows(R * cap + 1) == cap


F = 1 << 20


def regrid_call(lib, **kw):
    """mlx_regrid_apply with arguments that pass every check (pointers that are never dereferenced:
    the checks precede every HIP call), ``kw`` replacing some.  2 records of 48 sources to 70
    destinations (two slices: slice_ptr holds 3), 100 entries."""
    a = dict(v=F, dt=_lib.DTYPE_F64, sp=2 * F, ln=3 * F, col=4 * F, S=5 * F, ne=100, mf=0.0, flags=0,
             nrec=0, nsrc=48, ndst=70, out=8 * F, odt=_lib.DTYPE_F64)
    a.update(kw)
    return lib.mlx_regrid_apply(a["v"], a["dt"], a["sp"], a["ln"], a["col"], a["S"], a["ne"],
                                a["mf"], a["flags"], a["nrec"], a["nsrc"], a["ndst"], a["out"],
                                a["odt"], None)


REFUSALS = [
    (dict(v=None), -1), (dict(sp=None), -1), (dict(ln=None), -1), (dict(col=None), -1),
    (dict(S=None), -1), (dict(out=None), -1),
    (dict(dt=2), -3), (dict(dt=-1), -3), (dict(odt=2), -3), (dict(odt=7), -3),
    (dict(flags=4), -3), (dict(flags=8), -3), (dict(flags=-1), -3),
    (dict(nrec=-1), -2), (dict(nsrc=-1), -2), (dict(ndst=-1), -2), (dict(ne=-1), -2),
    (dict(nsrc=1 << 31), -2), (dict(nsrc=(1 << 31) + 5), -2),
    (dict(nrec=(1 << 38) // 70 + 1), -2), (dict(nrec=(1 << 32), nsrc=1 << 10), -2),
    (dict(ndst=(1 << 38) + 1, nrec=1), -2),
    (dict(mf=-0.25), -2), (dict(mf=1.5), -2), (dict(mf=float("nan")), -2), (dict(mf=float("inf")), -2),
    (dict(v=F + 4), -5), (dict(v=F + 2, dt=1), -5), (dict(out=8 * F + 4), -5),
    (dict(out=8 * F + 2, odt=1), -5), (dict(sp=2 * F + 4), -5), (dict(S=5 * F + 4), -5),
    (dict(ln=3 * F + 2), -5), (dict(col=4 * F + 2), -5),
    # an out (2 x 70 float64 = 1120 bytes) that overlaps an operand: v (2 x 48 float64), slice_ptr
    # (3 int64), len (70 int32), col (100 int32), S (100 float64)
    (dict(out=F), -2), (dict(out=F + 8 * 95), -2), (dict(out=F - 8 * 139), -2),
    (dict(out=2 * F + 16), -2), (dict(out=3 * F + 4 * 68), -2), (dict(out=4 * F + 4 * 96), -2),
    (dict(out=5 * F + 8 * 99), -2), (dict(out=5 * F - 8 * 139), -2),
]
ACCEPTED = [dict(out=F + 8 * 96), dict(out=F - 8 * 140), dict(out=2 * F + 24), dict(out=3 * F + 4 * 70),
            dict(out=4 * F + 4 * 100), dict(out=5 * F + 8 * 100)]  # (ranges that only touch)


def test_argument_errors_need_no_gpu():
    lib = _lib.load_regrid()
    assert regrid_call(lib) == 0  # nrec == 0: nothing to do, no launch
    assert regrid_call(lib, nrec=2, ndst=0) == 0  # ndst == 0 too
    assert regrid_call(lib, v=None, out=None) == 0  # (pointers are not looked at)
    for kw, code in REFUSALS:
        kw = dict(dict(nrec=2), **kw)
        assert regrid_call(lib, **kw) == code and _lib.last_error(), kw
    assert "NULL" in (regrid_call(lib, nrec=2, out=None), _lib.last_error())[1]
    assert "min_frac" in (regrid_call(lib, nrec=2, mf=2.0), _lib.last_error())[1]
    assert "overlaps" in (regrid_call(lib, nrec=2, out=F), _lib.last_error())[1]
    assert "2^31" in (regrid_call(lib, nrec=2, nsrc=1 << 31), _lib.last_error())[1]
    assert "2^38" in (regrid_call(lib, nrec=1 << 33, nsrc=1 << 10), _lib.last_error())[1]
    assert "flags" in (regrid_call(lib, nrec=2, flags=4), _lib.last_error())[1]
    # refused sizes, flags and fractions are refused for an empty record too
    assert regrid_call(lib, mf=2.0) == -2 and regrid_call(lib, dt=5) == -3
    assert regrid_call(lib, flags=16) == -3 and regrid_call(lib, nsrc=-2) == -2
    # (the accepted ranges of ACCEPTED would launch: tests/test_gpu_regrid_edges.py runs them)
    assert len(ACCEPTED) == 6


def test_a_library_without_the_kernel_is_an_error(monkeypatch):
    class Bare:
        def __getattr__(self, name):
            raise AttributeError(name)

    monkeypatch.setattr(_lib, "_regrid_bound", False)
    monkeypatch.setattr(_lib, "load", lambda: Bare())
    with pytest.raises(_lib.MomlevelHipError, match="does not export mlx_[a-z_]+: rebuild"):
        _lib.load_regrid()


def test_features_has_the_row_and_a_sha_of_its_own():
    from momlevel_amd.csrc import build

    assert build.FEATURES["regrid"] == ["mlx_internal.hpp", "mlx_pack.hpp",
                                        "include/momlevel_regrid.h"]
    assert len(build.regrid_source_sha()) == 16
    assert build.regrid_source_sha() == build.feature_source_sha("regrid")
    assert build.regrid_source_sha() not in (build.source_sha(), build.area_source_sha(),
                                             build.smooth_source_sha(), build.gauge_source_sha())
    names = {os.path.basename(p) for p in build.TIMED_SOURCES}
    assert "momlevel_regrid.hip" not in names and "momlevel_regrid.h" not in names
    assert any(p.endswith("momlevel_regrid.hip") for p in build.SOURCES)
    assert any(p.endswith("momlevel_regrid.h") for p in build.DEPENDS)
    text = open(os.path.join(ROOT, "momlevel_amd", "csrc", "momlevel_regrid.hip")).read()
    assert "#pragma clang fp contract(off)" in text and "atomic" not in text.replace("atomics", "")
    assert "asm" not in text


def test_the_module_is_published():
    assert momlevel_amd.regrid is regrid and "regrid" in momlevel_amd.__all__
    assert regrid.__all__ == ["Plan", "from_triplets", "coarsen_weights", "conservative_weights",
                              "nearest_weights", "apply", "coarsen"]
    assert "EXTENSION" in regrid.__doc__ and "regrid" in momlevel_amd.__doc__
    assert "momlevel_regrid.h" in momlevel_amd.__doc__
    for f in (regrid.apply, regrid.coarsen):
        assert "EXTENSION" in f.__doc__
    for text in (regrid.__doc__, open(HEADER).read()):  # what is not built is said
        assert "ilinear" in text and "curvilinear" in text and "fold" in text and "ranks" in text
    assert "area_mean" in regrid.__doc__ and "area_mean" in regrid.apply.__doc__
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "regrid.apply" in readme and "regrid.coarsen" in readme
    assert "3.20" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_no_undefined_globals_in_the_new_module():
    from test_static_names import _undefined

    assert _undefined(regrid) == []


# ---- the restatement ----------------------------------------------------------------------------
def test_the_restatement_on_a_hand_computed_table():
    """three destinations over five sources: d0 = {0: 1, 1: 3}, d1 = {} (no entry), d2 = {2: 2, 3: 2,
    4: 4}; record 0 has no NaN, record 1 has source 1 and sources 2, 3 NaN, record 2 all of d2's"""
    indptr = np.array([0, 2, 2, 5])
    col = np.array([0, 1, 2, 3, 4], dtype=np.int32)
    S = np.array([1.0, 3.0, 2.0, 2.0, 4.0])
    nan = np.nan
    v = np.array([[1.0, 2.0, 4.0, 8.0, 16.0], [1.0, nan, nan, nan, 16.0], [5.0, 6.0, nan, nan, nan]])
    out = rn.apply_csr(v, indptr, col, S, 3)
    assert out.dtype == np.float64 and out.shape == (3, 3)
    assert out[0].tolist()[::2] == [7.0 / 4.0, (8.0 + 16.0 + 64.0) / 8.0]
    assert out[1].tolist()[::2] == [1.0, 16.0] and out[2, 0] == 23.0 / 4.0
    assert np.isnan(out[:, 1]).all() and np.isnan(out[2, 2])
    assert (_bits(out)[np.isnan(out)] == 0x7FF8000000000000).all()  # canonical
    # min_frac: record 1 keeps 1 of 4 at d0 and 4 of 8 at d2
    half = rn.apply_csr(v, indptr, col, S, 3, min_frac=0.5)
    assert np.isnan(half[1, 0]) and half[1, 2] == 16.0 and half[0, 0] == 1.75
    full = rn.apply_csr(v, indptr, col, S, 3, min_frac=1.0)
    assert np.isnan(full[1]).all() and full[0, 2] == 11.0
    # the plain sum of what is present, and the propagating sum
    plain = rn.apply_csr(v, indptr, col, S, 3, flags=rn.NO_RENORM)
    assert plain[0].tolist()[::2] == [7.0, 88.0] and plain[1].tolist()[::2] == [1.0, 64.0]
    assert np.isnan(plain[2, 2]) and np.isnan(plain[:, 1]).all()
    prop = rn.apply_csr(v, indptr, col, S, 3, flags=rn.PROPAGATE)
    assert prop[0].tolist()[::2] == [7.0, 88.0] and np.isnan(prop[1]).all()
    assert prop[2, 0] == 23.0 and np.isnan(prop[2, 1:]).all()
    assert np.array_equal(_bits(rn.apply_csr(v, indptr, col, S, 3, flags=3)), _bits(prop))
    # float32: widened exactly, rounded once
    r32 = rn.apply_csr(v.astype(np.float32), indptr, col, S, 3)
    assert r32.dtype == np.float32 and r32[0, 0] == np.float32(1.75)
    assert (_bits(r32)[np.isnan(r32)] == 0x7FC00000).all()
    assert rn.apply_csr(v.astype(np.float32), indptr, col, S, 3, out_dtype=np.float64).dtype == np.float64
    # a record of ones is exactly 1.0 wherever it is not NaN
    ones = rn.apply_csr(np.where(np.isnan(v), nan, 1.0), indptr, col, np.array([0.1, 0.7, 0.3, 0.9, 1.3]), 3)
    assert set(np.unique(ones[~np.isnan(ones)])) == {1.0}
    # entries out of range carry no weight: the same result as the table without them
    wild = rn.apply_csr(v, np.array([0, 3, 3, 7]), np.array([0, 1, 5, -1, 2, 3, 4]),
                        np.array([1.0, 3.0, 9.0, 9.0, 2.0, 2.0, 4.0]), 3, min_frac=0.5)
    assert np.array_equal(_bits(wild), _bits(half))


def test_the_restatement_against_scipy():
    """PROPAGATE on NaN-free data is the sparse product; only the order of summation differs, so
    per destination |ours - scipy| <= len * 2^-52 * sum_k |S_k v_k|"""
    from scipy import sparse

    rng = np.random.default_rng(3)
    nsrc, ndst, nrec = 120, 37, 4
    length = rng.integers(0, 30, ndst)
    length[:3] = (0, 1, 29)
    indptr = np.concatenate([[0], np.cumsum(length)])
    col = np.concatenate([np.sort(rng.choice(nsrc, n, replace=False)) for n in length]).astype(np.int32)
    S = rng.normal(0.0, 1.0, col.size)
    v = rng.normal(0.0, 10.0, (nrec, nsrc))
    got = rn.apply_csr(v, indptr, col, S, ndst, flags=rn.PROPAGATE)
    A = sparse.csr_matrix((S, col, indptr), shape=(ndst, nsrc))
    want = (A @ v.T).T
    scale = (abs(A) @ np.abs(v).T).T
    ok = length > 0
    assert np.isnan(got[:, ~ok]).all() and not np.isnan(got[:, ok]).any()
    err = np.abs(got[:, ok] - want[:, ok])
    bound = length[ok] * 2.0 ** -52 * scale[:, ok]
    print(f"max |restatement - scipy| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()


# ---- the packed layout ----------------------------------------------------------------------------
@pytest.mark.parametrize("ndst", (1, 63, 64, 65, 130))
def test_the_packed_layout_unpacks_to_its_rows(ndst):
    L = core.regrid_slice()
    rng = np.random.default_rng(ndst)
    length = rng.integers(0, 7, ndst)
    length[0] = 0
    if ndst > 2:
        length[1], length[ndst - 1] = 1, 40
    indptr = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(500, n, replace=False)) for n in length] + [[]]).astype(np.int32)
    S = rng.uniform(0.5, 2.0, col.size)
    sp, ln, pc, pS = regrid.pack_rows(indptr, col, S, L)
    nslices = -(-ndst // L)
    assert sp.dtype == np.int64 and ln.dtype == np.int32 and pc.dtype == np.int32 and pS.dtype == np.float64
    assert sp.shape == (nslices + 1,) and ln.shape == (ndst,) and pc.shape == pS.shape == (int(sp[-1]),)
    assert np.array_equal(ln, length)
    for s in range(nslices):  # every slice padded to its longest row, no further
        assert sp[s + 1] - sp[s] == L * length[s * L:(s + 1) * L].max()
    i2, c2, S2 = rn.unpack(sp, ln, pc, pS, ndst, L)
    assert np.array_equal(i2, indptr) and np.array_equal(c2, col) and np.array_equal(_bits(S2), _bits(S))
    assert (pc == -1).sum() == pc.size - col.size and (pS[pc == -1] == 0.0).all()  # the padding
    plan = regrid.Plan(indptr, col, S, (20, 25), (1, ndst))
    assert all(np.array_equal(a, b) for a, b in zip(plan.packed, (sp, ln, pc, pS)))
    assert plan.packed is plan.packed and plan.nnz == col.size
    v = rng.normal(0, 1, (2, 500))
    assert np.array_equal(_bits(rn.apply_packed(v, sp, ln, pc, pS, ndst, L)),
                          _bits(rn.apply_csr(v, indptr, col, S, ndst)))


def test_an_empty_table_packs():
    sp, ln, pc, pS = regrid.pack_rows(np.zeros(4, dtype=np.int64), [], [], 64)
    assert sp.tolist() == [0, 0] and ln.tolist() == [0, 0, 0] and pc.size == pS.size == 0
    sp, ln, pc, pS = regrid.pack_rows(np.zeros(1, dtype=np.int64), [], [], 64)
    assert sp.tolist() == [0] and ln.size == 0


# ---- the builders ---------------------------------------------------------------------------------
def _through(plan, v, **kw):
    """a (nrec, ny, nx) record through the plan's rows by the restatement"""
    flat = np.asarray(v).reshape(v.shape[0], -1)
    return rn.apply_csr(flat, plan.indptr, plan.col, plan.S, plan.ndst, **kw).reshape(
        (v.shape[0],) + plan.dst_shape)


def test_coarsen_weights_on_a_plane_that_divides_evenly():
    """the bits of a direct reshape-and-sum: blocks summed source row by source row, column by
    column -- the ascending order of the flat source index"""
    rng = np.random.default_rng(5)
    ny, nx, fy, fx = 8, 12, 4, 3
    area = rng.uniform(1.0, 2.0, (ny, nx))
    v = rng.normal(0.0, 1.0, (2, ny, nx))
    plan = regrid.coarsen_weights(area, fy, fx)
    assert plan.src_shape == (ny, nx) and plan.dst_shape == (2, 4) and plan.dst_dims == ("yh", "xh")
    assert plan.nnz == ny * nx and np.array_equal(np.diff(plan.indptr), np.full(8, 12))
    blocks_a = area.reshape(2, fy, 4, fx).transpose(0, 2, 1, 3).reshape(2, 4, fy * fx)
    blocks_v = v.reshape(2, 2, fy, 4, fx).transpose(0, 1, 3, 2, 4).reshape(2, 2, 4, fy * fx)
    num, den = np.zeros((2, 2, 4)), np.zeros((2, 4))
    for k in range(fy * fx):
        num = num + blocks_a[..., k] * blocks_v[..., k]
        den = den + blocks_a[..., k]
    assert np.array_equal(_bits(_through(plan, v)), _bits(num / den))


def test_coarsen_weights_with_land_and_ragged_edges():
    rng = np.random.default_rng(6)
    ny, nx = 7, 10
    area = rng.uniform(1.0, 2.0, (ny, nx))
    area[0:3, 0:3] = 0.0       # a whole block of land
    area[3, 4] = np.nan
    area[5, 5] = -1.0
    v = rng.normal(0.0, 1.0, (1, ny, nx))
    plan = regrid.coarsen_weights(DataArray(area, ("y", "x")), 3, 3)
    assert plan.dst_shape == (3, 4) and plan.dst_dims == ("y", "x")
    wet = area > 0
    assert plan.nnz == wet.sum()
    out = _through(plan, v)[0]
    assert np.isnan(out[0, 0]) and np.isnan(out).sum() == 1
    for J in range(3):
        for I in range(4):
            a = np.where(wet, area, 0.0)[3 * J:3 * J + 3, 3 * I:3 * I + 3]
            if a.sum() > 0:
                want = (a * v[0, 3 * J:3 * J + 3, 3 * I:3 * I + 3]).sum() / a.sum()
                assert abs(out[J, I] - want) <= 16 * U * np.abs(v).max()
    # (the second block of rows 3..5 holds the NaN and the negative area.)  The east edge: cut (one
    # column in the last block) or completed from the row's start
    assert np.diff(plan.indptr).reshape(3, 4)[1].tolist() == [9, 7, 9, 3]
    wrap = regrid.coarsen_weights(area, 3, 3, periodic_x=True)
    last = wrap.col[wrap.indptr[7]:wrap.indptr[8]]  # destination (1, 3): rows 3..5, columns 9, 0, 1
    assert sorted(set(int(c) % nx for c in last)) == [0, 1, 9] and np.all(np.diff(last) > 0)
    assert regrid.coarsen_weights(area, 1, 1).nnz == wet.sum()  # the identity coarsening
    for bad in (dict(fy=0), dict(fx=-1), dict(fy=1.5)):
        with pytest.raises(ValueError):
            regrid.coarsen_weights(area, **dict(dict(fy=2, fx=2), **bad))
    with pytest.raises(ValueError, match="infinite"):
        regrid.coarsen_weights(np.where(area == area[6, 6], np.inf, area), 2, 2)
    with pytest.raises(ValueError, match="2-D"):
        regrid.coarsen_weights(area[0], 2, 2)


def _areas(lat_b, lon_b):
    lat_b, lon_b = np.asarray(lat_b, dtype=np.float64), np.asarray(lon_b, dtype=np.float64)
    band = np.abs(np.diff(np.sin(np.deg2rad(lat_b))))
    return band[:, None] * np.deg2rad(np.abs(np.diff(lon_b)))[None, :]


def test_conservative_weights_sum_to_the_cell_and_conserve_the_integral():
    src = (np.linspace(-90, 90, 91), np.linspace(0, 360, 181))      # 2 degrees
    dst = (np.linspace(-90, 90, 37), np.linspace(0, 360, 73))       # 5 degrees
    plan = regrid.conservative_weights(*src, *dst)
    assert plan.src_shape == (90, 180) and plan.dst_shape == (36, 72) and plan.dst_dims == ("lat", "lon")
    assert np.array_equal(plan.dst_coords["lat"].values, np.arange(-87.5, 90, 5.0))
    assert plan.dst_coords["lon"].dims == ("lon",)
    length = np.diff(plan.indptr)
    assert length.min() >= 9 and length.max() <= 16
    # every (full) destination cell's weights sum to its own area within len * 2^-52 relative
    A = _areas(*dst).reshape(-1)
    total = np.array([plan.S[plan.indptr[d]:plan.indptr[d + 1]].sum() for d in range(plan.ndst)])
    rel = np.abs(total - A) / A
    print(f"max |sum S - A| / (len 2^-52 A) = {np.max(rel / (length * 2.0 ** -52)):.3f}")
    assert (rel <= length * 2.0 ** -52).all()
    # a NaN-free field keeps its integral within 4 nsrc 2^-53 sum |a v|
    rng = np.random.default_rng(8)
    v = rng.normal(1.0, 2.0, (1, 90, 180))
    a = _areas(*src)
    out = _through(plan, v)
    lhs, rhs = (A.reshape(36, 72) * out[0]).sum(), (a * v[0]).sum()
    bound = 4 * plan.nsrc * U * np.abs(a * v[0]).sum()
    print(f"|sum A out - sum a v| / bound = {abs(lhs - rhs) / bound:.4f}")
    assert abs(lhs - rhs) <= bound
    assert not np.isnan(out).any()


def test_conservative_weights_wrap_in_longitude_and_give_the_identity():
    lat_b = np.linspace(-60, 60, 7)
    # the same cells cut at another meridian and named in another turn: 0..360 against -180..180
    plan = regrid.conservative_weights(lat_b, np.linspace(0, 360, 13), lat_b, np.linspace(-180, 180, 13))
    assert np.array_equal(np.diff(plan.indptr), np.ones(72))
    want = (np.arange(72).reshape(6, 12) // 12) * 12 + (np.arange(72).reshape(6, 12) % 12 + 6) % 12
    assert np.array_equal(plan.col, want.reshape(-1))
    # a destination cell astride the source's seam takes from both ends of the row
    seam = regrid.conservative_weights(lat_b, np.linspace(0, 360, 13), lat_b[2:4], [-45.0, 45.0])
    assert seam.dst_shape == (1, 1) and seam.col.tolist() == [24, 25, 34, 35]
    assert abs(seam.S.sum() - _areas(lat_b[2:4], [-45.0, 45.0])[0, 0]) <= 4 * 2.0 ** -52 * seam.S.sum()
    assert np.allclose(seam.S / seam.S.sum(), [1 / 3, 1 / 6, 1 / 6, 1 / 3], rtol=1e-14)
    # an identical source and destination grid gives the identity: one entry per cell, its own;
    # a descending latitude axis too
    for lat in (np.linspace(-90, 90, 19), np.linspace(90, -90, 19)):
        lon_b = np.linspace(20.0, 380.0, 25)
        same = regrid.conservative_weights(lat, lon_b, lat, lon_b)
        assert np.array_equal(same.indptr, np.arange(18 * 24 + 1))
        assert np.array_equal(same.col, np.arange(18 * 24))
        assert np.array_equal(_bits(same.S), _bits(_areas(lat, lon_b).reshape(-1)))
        v = np.random.default_rng(2).normal(0, 1, (1, 18, 24))
        out = _through(same, v)
        assert (np.abs(out - v) <= 2.0 ** -52 * np.abs(v)).all()  # (S v) / S: two roundings
        assert np.array_equal(_bits(_through(same, v, flags=rn.PROPAGATE)),
                              _bits(same.S.reshape(1, 18, 24) * v))
    # a source mask: masked cells carry no entry
    mask = np.ones((6, 12))
    mask[2, 3], mask[4, 5] = 0.0, np.nan
    masked = regrid.conservative_weights(lat_b, np.linspace(0, 360, 13), lat_b, np.linspace(0, 360, 13), mask)
    assert masked.nnz == 70 and 2 * 12 + 3 not in masked.col and 4 * 12 + 5 not in masked.col
    for bad in ([0.0], [0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [[0.0, 1.0]], [0.0, np.nan]):
        with pytest.raises(ValueError):
            regrid.conservative_weights(bad, [0.0, 1.0], [0.0, 1.0], [0.0, 1.0])
    with pytest.raises(ValueError, match="-90"):
        regrid.conservative_weights([0.0, 91.0], [0.0, 1.0], [0.0, 1.0], [0.0, 1.0])
    with pytest.raises(ValueError, match="360"):
        regrid.conservative_weights([0.0, 1.0], [0.0, 361.0], [0.0, 1.0], [0.0, 1.0])
    with pytest.raises(ValueError, match="src_mask"):
        regrid.conservative_weights(lat_b, [0.0, 1.0], lat_b, [0.0, 1.0], np.ones((2, 2)))


def test_from_triplets():
    row = np.array([2, 0, 2, 0, 2])
    col = np.array([4, 1, 2, 0, 3])
    S = np.array([4.0, 3.0, 2.0, 1.0, 2.5])
    plan = regrid.from_triplets(row, col, S, (1, 5), (3, 1), dst_dims=("y", "x"),
                                dst_coords={"y": [10.0, 20.0, 30.0]})
    assert plan.indptr.tolist() == [0, 2, 2, 5] and plan.col.tolist() == [0, 1, 2, 3, 4]
    assert plan.S.tolist() == [1.0, 3.0, 2.0, 2.5, 4.0] and plan.col.dtype == np.int32
    assert plan.nsrc == 5 and plan.ndst == 3 and plan.dst_dims == ("y", "x")
    assert plan.dst_coords["y"].dims == ("y",) and plan.dst_coords["y"].values.tolist() == [10.0, 20.0, 30.0]
    one = regrid.from_triplets(row + 1, col + 1, S, (1, 5), (3, 1), one_based=True)
    assert np.array_equal(one.indptr, plan.indptr) and np.array_equal(one.col, plan.col)
    assert np.array_equal(one.S, plan.S) and one.dst_dims == ("lat", "lon")
    with pytest.raises(ValueError, match="one .row, col. pair"):
        regrid.from_triplets([0, 1, 0], [2, 2, 2], [1.0, 1.0, 1.0], (1, 5), (3, 1))
    for r, c in (([3], [0]), ([-1], [0]), ([0], [5]), ([0], [-1])):
        with pytest.raises(ValueError, match="outside"):
            regrid.from_triplets(r, c, [1.0], (1, 5), (3, 1))
    with pytest.raises(ValueError, match="outside"):  # one-based input has no index 0
        regrid.from_triplets([0], [1], [1.0], (1, 5), (3, 1), one_based=True)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="finite"):
            regrid.from_triplets([0], [0], [bad], (1, 5), (3, 1))
    with pytest.raises(ValueError):
        regrid.from_triplets([0, 1], [0], [1.0], (1, 5), (3, 1))
    with pytest.raises(ValueError, match="integers"):
        regrid.from_triplets([0.5], [0], [1.0], (1, 5), (3, 1))
    with pytest.raises(ValueError):
        regrid.from_triplets([0], [0], [1.0], (5,), (3, 1))
    with pytest.raises(ValueError, match="destination plane"):
        regrid.from_triplets([0], [0], [1.0], (1, 5), (3, 1), dst_dims=("y", "x"),
                             dst_coords={"y": [1.0, 2.0]})
    empty = regrid.from_triplets([], [], [], (2, 2), (2, 3))
    assert empty.nnz == 0 and empty.indptr.tolist() == [0] * 7


# ---- Python-level refusals: all before any device work -----------------------------------------------
@pytest.mark.parametrize("fn", ("apply", "coarsen"))
def test_refusals_come_before_any_device_work(fn, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(regrid.core, "require_device", boom)
    monkeypatch.setattr(regrid.core, "regrid_apply", boom)
    monkeypatch.setattr(regrid.engine, "device_of", boom)
    monkeypatch.setattr(regrid.engine, "to_device", boom)
    monkeypatch.setattr(regrid.hostio, "to_device", boom)
    area = np.ones((6, 8))
    plan = regrid.coarsen_weights(area, 2, 2)
    eta = DataArray(np.ones((3, 6, 8)), ("time", "yh", "xh"), None, {"units": "m"}, "zos")

    def call(x, **kw):
        if fn == "apply":
            return regrid.apply(x, plan, **kw)
        return regrid.coarsen(x, area, 2, 2, **kw)

    for mf in (-0.1, 1.1, np.nan, "half"):
        with pytest.raises(ValueError, match="min_frac"):
            call(eta, min_frac=mf)
    with pytest.raises(ValueError, match="source plane"):
        call(DataArray(np.ones((3, 8, 6)), ("time", "yh", "xh")))
    with pytest.raises(ValueError, match="source plane"):
        call(np.ones((6, 9)))
    with pytest.raises(ValueError, match="at least the two dims"):
        call(np.ones(8))
    with pytest.raises(TypeError):
        call([[1.0, 2.0]])
    with pytest.raises(TypeError):
        call(eta.astype(np.float16))
    with pytest.raises(ValueError, match="one source plane"):
        call(Dataset({"steps": DataArray(np.arange(3.0), ("time",))}))
    if fn == "apply":
        with pytest.raises(TypeError, match="regrid.Plan"):
            regrid.apply(eta, (plan.indptr, plan.col, plan.S))
    else:
        with pytest.raises(ValueError):
            regrid.coarsen(eta, area, 0, 2)
        with pytest.raises(ValueError, match="2-D"):
            regrid.coarsen(eta, np.ones(48), 2, 2)


def test_core_regrid_apply_refuses_host_operands():
    with pytest.raises((TypeError, _lib.MomlevelHipError)):
        core.regrid_apply(np.ones((2, 4)), (None,) * 4, 4, 2)
