"""CPU: the C ABI of include/momlevel_census.h (symbols, binding table, geometry queries, argument
errors -- they precede every HIP call), the plans and the refusals of momlevel_amd.census, and the
numpy restatement tests/census_numpy.py against numpy.histogramdd and numpy.histogram.  No GPU."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import census_numpy as cn
import momlevel_amd
from momlevel_amd import _lib, census, core
from momlevel_amd.labeled import DataArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "momlevel_census.h")
NAMES = ["mlx_census_blocks", "mlx_census_histogram", "mlx_census_max_bins", "mlx_census_tile",
         "mlx_census_workspace_bytes"]


# ---- the C ABI ----------------------------------------------------------------------------------
def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_census_header_binding_and_exports_agree():
    text = _header_text()
    declared = sorted(set(re.findall(r"\b(mlx_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.CENSUS_PROTOTYPES) == NAMES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in momlevel_census.h but not exported"
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                             text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(mlx_census_[a-z0-9_]+)\b", out))) == declared
    ctype = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p,
             "const double *": ctypes.c_void_p, "double *": ctypes.c_void_p,
             "int64_t *": ctypes.c_void_p, "int64_t ": ctypes.c_int64, "int ": ctypes.c_int,
             "size_t ": ctypes.c_size_t}
    rtype = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}
    protos = re.findall(r"\b(int|int64_t|size_t)\s+(mlx_[a-z_]+)\s*\(([^)]*)\)", text)
    assert sorted(p[1] for p in protos) == declared
    for ret, name, args in protos:
        args = [" ".join(a.split()) for a in args.split(",")]
        want = [] if args == ["void"] else [next(v for k, v in ctype.items() if a.startswith(k))
                                           for a in args]
        restype, argtypes = _lib.CENSUS_PROTOTYPES[name]
        assert restype is rtype[ret] and argtypes == want, name
    assert protos[-1][1] == "mlx_census_histogram"
    assert protos[-1][2].split(",")[-1].strip() == "void *stream"
    assert (_lib.CENSUS_CLOSED_0, _lib.CENSUS_CLOSED_1) == (1, 2)
    assert _lib.load_census() is _lib.load()


def test_other_tables_and_the_abi_version_are_untouched():
    others = [v for k, v in vars(_lib).items() if k.endswith("SIGNATURES")]
    assert len(others) == 12  # SIGNATURES and the eleven feature tables of that name
    for name in _lib.CENSUS_PROTOTYPES:
        for table in others + [_lib.EOF_PROTOTYPES, _lib.SMOOTH_PROTOTYPES, _lib.REGRID_PROTOTYPES]:
            assert name not in table
    assert len(_lib.SIGNATURES) == 28 and len(_lib.REGRID_PROTOTYPES) == 4
    assert _lib.ABI_VERSION == 9 and _lib.load().mlx_version() == 9
    assert _lib._GROUPS["census"][0] is _lib.CENSUS_PROTOTYPES and _lib._census_bound in (True, False)
    assert "MLX_ABI_VERSION" not in open(HEADER).read().replace("do not move MLX_ABI_VERSION", "")


def test_geometry_queries_are_pure_functions():
    lib = _lib.load_census()
    T = core.census_tile()
    assert T == lib.mlx_census_tile() == 1024  # four cells a thread, 256 threads
    assert [core.census_blocks(n) for n in (-1, 0, 1, T, 8 * T, 8 * T + 1, 16 * T, 16 * T + 1)] == \
        [0, 0, 1, 1, 1, 2, 2, 3]
    top = core.census_blocks(75 * 1080 * 1440)
    assert top == core.census_blocks(1 << 38) == core.census_blocks(8 * T * top) and top >= 256
    assert core.census_blocks((1 << 38) + 1) == 0
    for n in (1, 5000, 10 ** 7):  # blocks never outnumber tiles, and repeat
        assert 1 <= core.census_blocks(n) <= -(-n // T) and core.census_blocks(n) == core.census_blocks(n)
    # the cap: what 64 KiB of LDS hold beside the edges, four private tables of 4 / 12 / 20 bytes
    for D in (1, 2):
        caps = [core.census_max_bins(D, w, v) for w, v in ((0, 0), (1, 0), (1, 1))]
        assert caps[0] > caps[1] > caps[2] >= 512
        for cap, per in zip(caps, (4, 12, 20)):
            edges = cap + 1 if D == 1 else cap + 3
            assert 8 * edges + 4 * per * cap <= 65536 < 8 * (edges + 1) + 4 * per * (cap + 1)
    assert core.census_max_bins(1, False, True) == 0 == core.census_max_bins(3) == core.census_max_bins(0)
    # the workspace: records x blocks x bins x outputs words; it never scales with ncells x nbins
    assert core.census_workspace_bytes(3, 16 * T + 1, 7, True, True) == 3 * 3 * 7 * 3 * 8
    assert core.census_workspace_bytes(3, 16 * T + 1, 7) == 3 * 3 * 7 * 8
    assert core.census_workspace_bytes(1, 1 << 38, 100, True) == top * 100 * 2 * 8
    for bad in ((-1, 10, 7), (1, -1, 7), (1, 10, 0), (1, (1 << 38) + 1, 7), (1 << 30, 1 << 20, 7),
                (1, 10, core.census_max_bins(1) + 1)):
        assert core.census_workspace_bytes(*bad) == 0
    assert core.census_workspace_bytes(1, 10, 7, False, True) == 0


F = 1 << 20


def census_call(lib, **kw):
    """mlx_census_histogram with arguments that pass every check (pointers that are never
    dereferenced: the checks precede every HIP call), ``kw`` replacing some.  nrec = 0 by default."""
    a = dict(f0=F, dt0=0, f1=2 * F, dt1=1, D=2, e0=3 * F, n0=3, e1=4 * F, n1=5, closed=3, w=5 * F,
             wdt=0, wpr=0, val=6 * F, vdt=1, nrec=0, ncells=100, count=7 * F, wsum=8 * F,
             vsum=9 * F, ws=10 * F, nws=1 << 20)
    a.update(kw)
    return lib.mlx_census_histogram(a["f0"], a["dt0"], a["f1"], a["dt1"], a["D"], a["e0"], a["n0"],
                                    a["e1"], a["n1"], a["closed"], a["w"], a["wdt"], a["wpr"],
                                    a["val"], a["vdt"], a["nrec"], a["ncells"], a["count"],
                                    a["wsum"], a["vsum"], a["ws"], a["nws"], None)


CAP = 744  # mlx_census_max_bins(2, 1, 1); checked below
REFUSALS = [
    (dict(f0=None), -1), (dict(f1=None), -1), (dict(e0=None), -1), (dict(e1=None), -1),
    (dict(count=None), -1), (dict(wsum=None), -1), (dict(vsum=None), -1), (dict(ws=None), -1),
    (dict(dt0=2), -3), (dict(dt0=-1), -3), (dict(dt1=7), -3), (dict(wdt=2), -3), (dict(vdt=-1), -3),
    (dict(closed=4), -3), (dict(closed=-1), -3),
    (dict(D=0), -2), (dict(D=3), -2), (dict(n0=0), -2), (dict(n1=0), -2), (dict(n0=-4), -2),
    (dict(D=1, n1=2), -2), (dict(w=None), -2),  # (val without w)
    (dict(n0=CAP + 1, n1=1), -2), (dict(n0=2, n1=CAP // 2 + 1), -2), (dict(n0=1 << 40, n1=1 << 40), -2),
    (dict(nrec=-1), -2), (dict(ncells=-1), -2), (dict(ncells=(1 << 38) + 1, nrec=1), -2),
    (dict(nrec=(1 << 40) // 100 + 1), -2), (dict(nrec=1 << 22, ncells=1 << 30), -2),
    (dict(f0=F + 4), -5), (dict(f1=2 * F + 2), -5), (dict(w=5 * F + 4), -5), (dict(val=6 * F + 2), -5),
    (dict(e0=3 * F + 4), -5), (dict(e1=4 * F + 4), -5), (dict(count=7 * F + 4), -5),
    (dict(wsum=8 * F + 4), -5), (dict(vsum=9 * F + 4), -5),
    (dict(nws=2 * 1 * 15 * 3 * 8 - 1), -4), (dict(ws=10 * F + 4), -4),
]


def test_argument_errors_need_no_gpu():
    lib = _lib.load_census()
    assert lib.mlx_census_max_bins(2, 1, 1) == CAP
    assert census_call(lib) == 0  # nrec == 0: nothing to do, no launch
    assert census_call(lib, nrec=2, ncells=0) == 0  # ncells == 0 too
    assert census_call(lib, f0=None, count=None, ws=None) == 0  # (pointers are not looked at)
    for kw, code in REFUSALS:
        kw = dict(dict(nrec=2), **kw)
        assert census_call(lib, **kw) == code and _lib.last_error(), kw
    assert "NULL" in (census_call(lib, nrec=2, count=None), _lib.last_error())[1]
    assert "bin groups" in (census_call(lib, nrec=2, n0=CAP + 1, n1=1), _lib.last_error())[1]
    assert "val needs w" in (census_call(lib, nrec=2, w=None), _lib.last_error())[1]
    assert "2^38" in (census_call(lib, nrec=1, ncells=1 << 39), _lib.last_error())[1]
    assert "workspace" in (census_call(lib, nrec=2, nws=8), _lib.last_error())[1]
    assert "D must be" in (census_call(lib, nrec=2, D=3), _lib.last_error())[1]
    # refused sizes, dtypes and flags are refused for an empty record too
    assert census_call(lib, D=0) == -2 and census_call(lib, dt0=5) == -3
    assert census_call(lib, closed=8) == -3 and census_call(lib, n0=0) == -2
    # what is absent is not looked at: no weights -> wsum / vsum / their dtypes may be anything
    assert census_call(lib, w=None, val=None, wdt=9, vdt=9, wsum=None, vsum=None) == 0
    assert census_call(lib, D=1, n1=1, f1=None, e1=None, dt1=9) == 0


def test_a_library_without_the_kernel_is_an_error(monkeypatch):
    class Bare:
        def __getattr__(self, name):
            raise AttributeError(name)

    monkeypatch.setattr(_lib, "_census_bound", False)
    monkeypatch.setattr(_lib, "load", lambda: Bare())
    with pytest.raises(_lib.MomlevelHipError, match="does not export mlx_[a-z_]+: rebuild"):
        _lib.load_census()


def test_features_has_the_row_and_a_sha_of_its_own():
    from momlevel_amd.csrc import build

    assert build.FEATURES["census"] == ["mlx_internal.hpp", "mlx_pack.hpp",
                                        "include/momlevel_census.h"]
    assert len(build.census_source_sha()) == 16
    assert build.census_source_sha() == build.feature_source_sha("census")
    assert build.census_source_sha() not in (build.source_sha(), build.area_source_sha(),
                                             build.regrid_source_sha(), build.smooth_source_sha())
    names = {os.path.basename(p) for p in build.TIMED_SOURCES}
    assert "momlevel_census.hip" not in names and "momlevel_census.h" not in names
    assert any(p.endswith("momlevel_census.hip") for p in build.SOURCES)
    assert any(p.endswith("momlevel_census.h") for p in build.DEPENDS)
    text = open(os.path.join(ROOT, "momlevel_amd", "csrc", "momlevel_census.hip")).read()
    assert "#pragma clang fp contract(off)" in text and "atomic" not in text.replace("atomics", "")
    assert "asm" not in text
    log = open(os.path.join(ROOT, "profiles", "census_kernels.log")).read()
    assert build.census_source_sha() in log


def test_the_module_is_published():
    assert momlevel_amd.census is census and "census" in momlevel_amd.__all__
    assert census.__all__ == ["histogram", "ts_census", "bin_edges"]
    assert "EXTENSION" in census.__doc__ and "census" in momlevel_amd.__doc__
    assert "momlevel_census.h" in momlevel_amd.__doc__
    for f in (census.histogram, census.ts_census):
        assert "EXTENSION" in f.__doc__
    assert "calc_pdens" in census.ts_census.__doc__ and "calc_spice" in census.ts_census.__doc__
    for text in (census.__doc__, open(HEADER).read()):  # what is not built is said; static maps too
        assert "more than two" in text.lower() and "ranks" in text and "global memory" in text
        assert "regrid" in text and "area_mean" in text
    assert "poison" in census.__doc__ and "left out" in census.histogram.__doc__
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "census.histogram" in readme and "census.ts_census" in readme
    assert "3.21" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_no_undefined_globals_in_the_new_module():
    from test_static_names import _undefined

    assert _undefined(census) == []


# ---- the restatement against numpy's own ----------------------------------------------------------
E0 = np.array([-2.0, -0.5, 0.0, 0.25, 1.0, 1.5, 4.0, 9.0])
E1 = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 8.0])


def _specials(e):
    return np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf),
                           [np.nan, np.inf, -np.inf, -0.0, 0.0, 1e30, -1e30]])


@pytest.mark.parametrize("dt", (np.float64, np.float32))
def test_the_restatement_is_numpy_histogram(dt):
    rng = np.random.default_rng(1)
    f = np.concatenate([rng.uniform(-3.0, 10.0, 4000), _specials(E0)]).astype(dt)[None]
    w = rng.uniform(0.0, 2.0, f.shape[1])
    count, wsum, _ = cn.census([f], [E0], w)
    ok = ~np.isnan(f[0])  # (numpy.histogram refuses NaN in a range search only; mask it anyway)
    want = np.histogram(f[0][ok].astype(np.float64), bins=E0)[0]
    assert count.dtype == np.int64 and np.array_equal(count[0], want)
    want_w = np.histogram(f[0][ok].astype(np.float64), bins=E0, weights=w[ok])[0]
    assert np.allclose(wsum[0], want_w, rtol=1e-13, atol=0)
    i, inside = cn.bin_index(E0, np.array([9.0, -0.0, 0.0, -2.0, np.nextafter(dt(-2.0), dt(-3.0)),
                                           np.nan, np.inf, -np.inf], dtype=dt))
    assert i[:4].tolist() == [6, 2, 2, 0] and inside.tolist() == [True] * 4 + [False] * 4
    i, inside = cn.bin_index(E0, np.array([9.0, 4.0]), closed=False)  # a bin group's open end
    assert inside.tolist() == [False, True] and i[1] == 6


@pytest.mark.parametrize("dt", (np.float64, np.float32))
def test_the_restatement_is_numpy_histogramdd(dt):
    rng = np.random.default_rng(2)
    n = 6000
    f0 = np.concatenate([rng.uniform(-3.0, 10.0, n), _specials(E0), rng.uniform(-1, 5, 22)]).astype(dt)
    f1 = np.concatenate([rng.uniform(-1.0, 9.0, n), rng.uniform(0, 4, 31), _specials(E1)[:22]]).astype(dt)
    w = rng.uniform(0.0, 2.0, f0.size)
    v = rng.normal(0.0, 3.0, f0.size)
    count, wsum, vsum = cn.census([f0[None], f1[None]], [E0, E1], w, v[None])
    ok = ~np.isnan(f0) & ~np.isnan(f1)
    sample = np.stack([f0[ok], f1[ok]], axis=1).astype(np.float64)
    assert np.array_equal(count[0], np.histogramdd(sample, bins=[E0, E1])[0])
    assert np.allclose(wsum[0], np.histogramdd(sample, bins=[E0, E1], weights=w[ok])[0], rtol=1e-13)
    assert np.allclose(vsum[0], np.histogramdd(sample, bins=[E0, E1], weights=(w * v)[ok])[0],
                       rtol=1e-10, atol=1e-10)
    assert cn.left_out([f0[None], f1[None]], [E0, E1])[0] == f0.size - count.sum()


def test_the_restatement_masks_nan_weights_and_values_and_windows_static_weights():
    f = np.array([[0.1, 0.1, 0.1, 0.3, 5.0], [0.1, 0.3, 0.3, 0.3, 0.3]])
    w = np.array([1.0, np.nan, 2.0, 4.0, 8.0])
    v = np.array([[1.0, 1.0, np.nan, 3.0, 1.0], [2.0, 2.0, 2.0, 2.0, np.nan]])
    count, wsum, vsum = cn.census([f], [E0], w, v)
    assert count[0].tolist() == [0, 0, 1, 1, 0, 0, 1] and count[1].tolist() == [0, 0, 1, 2, 0, 0, 0]
    assert wsum[0].tolist() == [0, 0, 1.0, 4.0, 0, 0, 8.0] and vsum[1].tolist() == [0, 0, 2.0, 12.0, 0, 0, 0]
    only = cn.census([f], [E0], w)
    assert only[0][0].tolist() == [0, 0, 2, 1, 0, 0, 1] and only[2] is None
    per = cn.census([f], [E0], np.stack([w, w]), v)
    assert all(np.array_equal(a, b) for a, b in zip(per, (count, wsum, vsum)))
    # bin groups tile the table: the groups' tables are the whole table's blocks
    whole = cn.census([f, f[::-1]], [E0, E0], w, v)
    for g in census.plan_bin_groups((7, 7), 10) + census.plan_bin_groups((7, 7), 3):
        e = [E0[a:b + 1] for a, b in g]
        part = cn.census([f, f[::-1]], e, w, v, closed=census.group_closed(g, (7, 7)))
        box = (slice(None),) + tuple(slice(a, b) for a, b in g)
        assert all(np.array_equal(p, x[box]) for p, x in zip(part, whole))


# ---- the plans ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,cap", (((1,), 1), ((7,), 7), ((7,), 3), ((745,), 744), ((1491,), 744),
                                       ((3, 5), 15), ((3, 5), 14), ((3, 5), 5), ((3, 5), 4), ((3, 5), 1),
                                       ((100, 100), 1169), ((64, 64), 1169), ((1, 2000), 744),
                                       ((2000, 1), 744)))
def test_every_bin_lies_in_exactly_one_group(shape, cap):
    groups = census.plan_bin_groups(shape, cap)
    seen = np.zeros(shape, dtype=np.int64)
    for g in groups:
        assert len(g) == len(shape) and all(0 <= a < b <= n for (a, b), n in zip(g, shape))
        assert np.prod([b - a for a, b in g]) <= cap
        seen[tuple(slice(a, b) for a, b in g)] += 1
        assert census.group_closed(g, shape) == sum(1 << d for d, (_, b) in enumerate(g) if b == shape[d])
    assert (seen == 1).all()
    assert len(groups) >= -(-int(np.prod(shape)) // cap)
    if len(shape) == 1 or shape[1] <= cap:  # bands: no more launches than the bins need, + 1 row's slack
        rows = 1 if len(shape) == 1 else shape[1]
        assert len(groups) == -(-shape[0] // max(1, cap // rows))
    assert census.plan_bin_groups(shape, cap) == groups
    assert len(census.plan_bin_groups((100, 100), 1169)) == 10  # "a few passes"


def test_bad_plans_are_refused():
    for shape, cap in (((0,), 4), ((3, 0), 4), ((3,), 0), ((2, 2, 2), 4), ((), 4)):
        with pytest.raises(ValueError):
            census.plan_bin_groups(shape, cap)


@pytest.mark.parametrize("nrec,per,bound,cap", ((0, 100, 1000, 8), (1, 100, 1000, 8), (25, 100, 1000, 8),
                                                (25, 100, 1000, 100), (25, 2000, 1000, 8),
                                                (1000, 24, None, None), (7, 1 << 27, None, None)))
def test_the_record_windows_keep_the_workspace_under_the_bound(nrec, per, bound, cap):
    wins = census.plan_record_windows(nrec, 5000, per, bound=bound, cap=cap)
    bound = census.WORKSPACE_BOUND if bound is None else bound
    cap = census.RECORD_WINDOW if cap is None else cap
    assert [w[0] for w in wins[1:]] == [w[1] for w in wins[:-1]]  # (no gap, no overlap)
    assert (wins[0][0], wins[-1][1]) == (0, nrec) if nrec else wins == []
    for i0, i1 in wins:
        assert 1 <= i1 - i0 <= cap
        assert (i1 - i0) * per <= bound or i1 - i0 == 1  # (one record at least)
    if nrec and per <= bound:
        assert max(i1 - i0 for i0, i1 in wins) == min(nrec, cap, bound // per)
    # 2^40 elements a launch
    assert census.plan_record_windows(5, 1 << 39, 8) == [(0, 2), (2, 4), (4, 5)]
    assert census.WORKSPACE_BOUND == 256 << 20 and census.RECORD_WINDOW == 256


def test_bin_edges():
    e = census.bin_edges(-2.0, 30.0, 64)
    assert e.dtype == np.float64 and e.shape == (65,) and np.array_equal(e, np.linspace(-2.0, 30.0, 65))
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            census.bin_edges(0.0, 1.0, bad)


# ---- Python-level refusals: all before any device work -------------------------------------------------
def test_refusals_come_before_any_device_work(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(census.core, "require_device", boom)
    monkeypatch.setattr(census.core, "census", boom)
    monkeypatch.setattr(census.engine, "device_of", boom)
    monkeypatch.setattr(census.engine, "to_device", boom)
    monkeypatch.setattr(census.hostio, "to_device", boom)
    dims = ("time", "z_l", "yh", "xh")
    th = DataArray(np.ones((3, 2, 4, 5)), dims, None, None, "thetao")
    so = DataArray(np.ones((3, 2, 4, 5), dtype=np.float32), dims, None, None, "so")
    vol = DataArray(np.ones((2, 4, 5)), dims[1:], None, None, "volcello")
    e = census.bin_edges(0.0, 2.0, 4)
    with pytest.raises(ValueError, match="more than two"):
        census.histogram(th, so, th, bins=(e, e, e))
    with pytest.raises(ValueError, match="one or two fields"):
        census.histogram(bins=e)
    for bad in (th.astype(np.float16), th.astype(np.int32), th.astype(np.int64)):
        with pytest.raises(TypeError, match="convert"):
            census.histogram(bad, bins=e)
        with pytest.raises(TypeError, match="convert"):
            census.histogram(th, bins=e, weights=bad)
        with pytest.raises(TypeError, match="convert"):
            census.histogram(th, bins=e, weights=th, values=bad)
    with pytest.raises(ValueError, match="shapes .* differ"):
        census.histogram(th, so[:, :1], bins=(e, e))
    for w in (np.ones((4, 5)), np.ones((3, 4, 5)), np.ones((2, 4, 6)), np.ones(5), np.ones((3, 1, 4, 5))):
        with pytest.raises(ValueError, match="weights of shape .* broadcast"):
            census.histogram(th, bins=e, weights=w)
    with pytest.raises(ValueError, match="values of shape"):
        census.histogram(th, bins=e, weights=vol, values=vol)
    with pytest.raises(ValueError, match="values need weights.*pass weights"):
        census.histogram(th, bins=e, values=th)
    for bad, text in (([0.0, 1.0, 1.0], "increase strictly"), ([0.0, 2.0, 1.0], "increase strictly"),
                      ([0.0, np.nan, 1.0], "NaN or infinite"), ([0.0, np.inf], "NaN or infinite"),
                      ([1.0], "at least two edges"), ([], "at least two edges"),
                      (5, "at least two edges"), ([[0.0, 1.0], [2.0, 3.0]], "must be a 1-D array")):
        with pytest.raises(ValueError, match=text):
            census.histogram(th, bins=bad)
    with pytest.raises(ValueError, match="one edge array per field"):
        census.histogram(th, so, bins=e)
    with pytest.raises(ValueError, match="one edge array per field"):
        census.histogram(th, so, bins=(e,))
    with pytest.raises(ValueError, match="at least two edges"):
        census.histogram(th, so, bins=(e, 7))
    with pytest.raises(ValueError, match="first dim"):
        census.histogram(th, bins=e, tcoord="z_l")
    with pytest.raises(TypeError, match="must be a DataArray"):
        census.histogram([[1.0, 2.0]], bins=e)
    with pytest.raises(ValueError, match="more than two"):
        census.ts_census(th, so, vol, e, e) if False else census.histogram(th, so, vol, bins=(e, e, e))
    with pytest.raises(ValueError, match="weights of shape"):
        census.ts_census(th, so, np.ones((4, 5)), e, e)


def test_the_plan_of_a_call():
    dims = ("time", "z_l", "yh", "xh")
    th = DataArray(np.ones((3, 2, 4, 5)), dims, None, None, "thetao")
    e, e2 = census.bin_edges(0.0, 2.0, 4), census.bin_edges(0.0, 1.0, 9)
    p = census._Plan((th, th), (e, e2), np.ones((2, 4, 5), dtype=np.float32), th, "time")
    assert (p.lead, p.nrec, p.ncells, p.shape) == (1, 3, 40, (4, 9)) and not p.w_per_record
    assert p.labeled and [x.name for x in p.per_record()] == ["thetao", "thetao", "thetao"]
    p = census._Plan((th,), e, th, None, "time")
    assert p.w_per_record and len(p.per_record()) == 2 and p.shape == (4,)
    p = census._Plan((th.values,), [e], None, None, "time")  # no such dim: one table of everything
    assert (p.lead, p.nrec, p.ncells, p.labeled) == (0, 1, 120, False)
    p = census._Plan((th[0],), (e,), th[0], th[0], "time")
    assert (p.lead, p.nrec, p.ncells, p.w_per_record) == (0, 1, 40, False)
    assert census._bin_names(p.fields) == ["thetao"]
    assert census._bin_names([th, th]) == ["thetao_0", "thetao_1"]
    assert census._bin_names([DataArray(np.ones(3)), th]) == ["field0", "thetao"]
    mean = census._class_mean(np.array([0, 2]), np.array([0.0, 4.0]), np.array([0.0, 6.0]))
    assert np.isnan(mean[0]) and mean[1] == 1.5


def test_core_census_refuses_host_operands():
    with pytest.raises((TypeError, _lib.MomlevelHipError)):
        core.census([np.ones((2, 4))], [np.arange(3.0)])
