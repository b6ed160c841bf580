"""CPU: the reading of the reference's C-grid group (tests/vort_numpy.py) against the reference's
own pinned sums (tests/golden/vort_goldens.json), the C ABI of include/momlevel_vort.h (symbols,
binding table, argument errors) and the argument handling of derived.calc_rel_vort / calc_pv /
calc_coriolis / calc_rossby_rd that needs no device.  No GPU."""

import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import vort_numpy as vn
from conftest import assert_bit_equal
from momlevel_amd import _lib, core, derived
from momlevel_amd.labeled import DataArray, Dataset
from momlevel_amd.test_data import generate_test_data, generate_test_data_uv
from oracle import momlevel_numpy as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "momlevel_vort.h")

dset1 = generate_test_data()
dset3 = generate_test_data_uv()


# ---- the reading against the reference's pins -----------------------------------------------------
@pytest.fixture(scope="module")
def restated():
    """zeta, N^2 and the wave speed of the reference's datasets by the numpy restatements"""
    zeta = vn.rel_vort(dset3.uo.values, dset3.vo.values, dset3.dxCu.values, dset3.dyCv.values,
                       dset3.areacello_bu.values)
    d = o.generate_test_data()
    n2 = o.calc_n2(d["thetao"], d["so"], d["z_l"])
    speed = o.calc_wave_speed_4d_quirk(n2, o.calc_dz(d["z_l"], d["z_i"], d["deptho"]))
    return zeta, n2, speed


def _pin(name, got):
    g = vn.goldens()
    half = g["half_unit_of_the_last_printed_digit"][name]
    print(f"{name}: restated {got!r}, pinned {g[name]!r}, difference {abs(got - g[name]):.3e}, "
          f"half a unit of the last printed digit {half:.0e}")
    assert abs(got - g[name]) <= half, name


def test_the_generator_draws_are_the_references():
    d = o.generate_test_data()
    assert np.array_equal(dset1.thetao.values, d["thetao"])
    assert dset3.uo.dims == ("time", "z_l", "yh", "xq") and dset3.vo.dims == ("time", "z_l", "yq", "xh")
    assert dset3.dxCu.dims == ("yh", "xq") and dset3.dyCv.dims == ("yq", "xh")
    assert dset3.Coriolis.dims == dset3.areacello_bu.dims == ("yq", "xq")
    assert np.array_equal(dset3.uo.values, np.random.default_rng(123).normal(0.0061, 0.08, (5, 5, 5, 5)))
    assert np.array_equal(dset3.vo.values, np.random.default_rng(123).normal(0.00077, 0.04, (5, 5, 5, 5)))
    assert np.array_equal(dset3.Coriolis.values, np.random.default_rng(123).normal(1.21e-5, 0.00011, (5, 5)))
    assert np.array_equal(dset3.xq.values, [1.5, 2.5, 3.5, 4.5, 5.5])
    assert np.isclose(dset3.areacello_bu.values.sum(), 3.6111092e14)
    assert np.all(dset3.dxCu.values == 1.0) and np.all(dset3.dyCv.values == 1.0)


def test_pv_pins(restated):
    zeta, n2, _ = restated
    _pin("calc_pv_m_sum", float(vn.pv(zeta, dset3.Coriolis.values, n2, units="m").sum()))
    _pin("calc_pv_cm_sum", float(vn.pv(zeta, dset3.Coriolis.values, n2, units="cm").sum()))


def test_rossby_and_coriolis_pins(restated):
    _, _, speed = restated
    f = vn.coriolis(dset1.geolat.values)
    _pin("calc_coriolis_sum", float(f.sum()))
    assert speed.shape == (5, 5, 5, 5)  # (z_l, yh, xh, time)
    rd = vn.rossby_rd(speed, f[None, :, :, None])
    rd = np.where(np.isinf(rd), np.nan, rd)  # (the reference's test: xr.where(isinf, nan, rd))
    _pin("calc_rossby_rd_sum", float(np.nansum(rd)))


def test_periodic_padding_is_not_the_reference(restated):
    """the guard of the reading: wrapping instead of zero fill misses the ``cm`` pin by far"""
    _, n2, _ = restated
    g = vn.goldens()
    zeta = vn.rel_vort(dset3.uo.values, dset3.vo.values, dset3.dxCu.values, dset3.dyCv.values,
                       dset3.areacello_bu.values, periodic=True)
    wrapped = float(vn.pv(zeta, dset3.Coriolis.values, n2, units="cm", periodic=True).sum())
    print("periodic padding:", wrapped, "pinned:", g["calc_pv_cm_sum"])
    assert not np.allclose(wrapped, g["calc_pv_cm_sum"])
    assert abs(wrapped - g["calc_pv_cm_periodic_sum"]) < 0.01
    assert "constrains nothing" in g["calc_rel_vort_note"] and abs(g["calc_rel_vort_sum"]) < 1e-8


def test_the_stencils_of_the_restatement():
    """the two grids written out by hand on a 2 x 3 plane"""
    u = np.array([[1.0, 2.0, 4.0], [8.0, 16.0, 32.0]])
    one = np.ones((2, 3))
    # non-symmetric: f[k+1] - f[k], 0.0 past the end
    assert np.array_equal(vn.diff(u, -2), [[7.0, 14.0, 28.0], [-8.0, -16.0, -32.0]])
    assert np.array_equal(vn.diff(u, -1), [[1.0, 2.0, -4.0], [8.0, 16.0, -32.0]])
    assert np.array_equal(vn.interp(u, -1), [[1.5, 3.0, 2.0], [12.0, 24.0, 16.0]])
    assert np.array_equal(vn.rel_vort(u, u, one, one, one), -vn.diff(u, -2) + vn.diff(u, -1))
    # symmetric: f[k] - f[k-1] for k = 0..n, both ends 0.0
    assert np.array_equal(vn.diff(u, -1, symmetric=True), [[1.0, 1.0, 2.0, -4.0], [8.0, 8.0, 16.0, -32.0]])
    assert vn.diff(u, -2, symmetric=True).shape == (3, 3)
    assert np.array_equal(vn.interp(u, -2, symmetric=True), [[0.5, 1.0, 2.0], [4.5, 9.0, 18.0], [4.0, 8.0, 16.0]])
    us, vs = np.ones((2, 4)), np.ones((3, 3))
    assert vn.rel_vort(us, vs, us, vs, np.ones((3, 4)), symmetric=True).shape == (3, 4)
    # dtypes are numpy's promotions
    f32 = np.float32
    assert vn.rel_vort(u.astype(f32), u.astype(f32), one.astype(f32), one.astype(f32), one.astype(f32)).dtype == f32
    assert vn.rel_vort(u.astype(f32), u.astype(f32), one, one, one).dtype == np.float64
    z32, n32 = np.ones((2, 3), f32), np.ones((2, 3), f32)
    assert vn.pv(z32, one.astype(f32), n32, units="cm").dtype == f32
    assert vn.pv(z32, one, n32).dtype == np.float64 and vn.pv(z32, one.astype(f32), n32.astype(float)).dtype == np.float64
    with pytest.raises(ValueError, match="unknown units option `km`"):
        vn.pv(z32, one, n32, units="km")


# ---- the C ABI ----------------------------------------------------------------------------------
def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_vort_header_binding_and_exports_agree():
    text = _header_text()
    declared = sorted(set(re.findall(r"\b(mlx_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.VORT_SIGNATURES) == [
        "mlx_vort_pv", "mlx_vort_records_per_launch", "mlx_vort_rel_vort", "mlx_vort_rossby",
        "mlx_vort_tile_width"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in momlevel_vort.h but not exported"
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                             text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(mlx_vort_[a-z0-9_]+)\b", out))) == declared
    ctype = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p, "int64_t ": ctypes.c_int64,
             "int ": ctypes.c_int, "double ": ctypes.c_double}
    protos = re.findall(r"\b(int|int64_t)\s+(mlx_vort_[a-z_]+)\s*\(([^)]*)\)", text)
    assert sorted(p[1] for p in protos) == declared
    for ret, name, args in protos:
        args = [" ".join(a.split()) for a in args.split(",")]
        want = [next(v for k, v in ctype.items() if a.startswith(k)) for a in args]
        restype, argtypes = _lib.VORT_SIGNATURES[name]
        assert restype is (ctypes.c_int if ret == "int" else ctypes.c_int64) and argtypes == want, name
        if ret == "int":
            assert args[-1] == "void *stream", name  # the caller's stream last
    for name, val in re.findall(r"#define MLX_(VORT_[A-Z_]+)\s+(\d+)", text):
        assert getattr(_lib, name) == int(val), name
    assert _lib.load_vort() is _lib.load()
    assert core.vort_tile() == (_lib.VORT_TILE_LANES * 2, _lib.VORT_TILE_LANES * 4, _lib.VORT_TILE_H,
                                _lib.VORT_TILE_BANDS)
    assert lib.mlx_vort_tile_width(7) == 0


def test_records_per_launch_is_plain_arithmetic():
    """step = budget // (tiles of one record): the budget is what one tile a record gives, a plane
    of t tiles gets a t-th of it, and a plane that cannot be moved in packs gets 0"""
    step = core.vort_records_per_launch
    W64, W32, H, bands = core.vort_tile()
    rows = H * bands  # rows of a block
    for dt, W, P in ((np.float64, W64, 2), (np.float32, W32, 4)):
        budget = step(1, P, dt)
        assert budget > 1 and step(2, P, dt) == step(rows, W, dt) == budget  # one tile a record
        for ny, nx, tiles in ((rows + 1, P, 2), (rows, W + P, 2), (rows + 1, W + P, 4),
                              (3 * rows, 2 * W, 6), (1080, 1440 - 1440 % P,
                                                     -(-1080 // rows) * -(-(1440 - 1440 % P) // W))):
            assert step(ny, nx, dt) == budget // tiles, (ny, nx, dt)
        for nx in (1, P - 1, P + 1, W + 1):  # not a whole number of packs: cell by cell
            assert step(2, nx, dt) == 0
        assert step(0, P, dt) == 0 and step(2, 0, dt) == 0 and step(-1, P, dt) == 0
        assert step(1 << 20, P << 20, dt) == 0  # ny * nx > 2^38
        assert step(rows * 65536, P, dt) == 0 and step(rows * 65535, P, dt) == budget // 65535
    assert step(2, 2, np.float32) == 0 and step(2, 4, np.float64) == step(2, 2, np.float64)
    lib = _lib.load_vort()
    assert lib.mlx_vort_records_per_launch(2, 4, 7) == 0
    with pytest.raises(TypeError):
        step(2, 4, np.float16)


def test_other_tables_and_the_abi_version_are_untouched():
    for name in _lib.VORT_SIGNATURES:
        for table in (_lib.SIGNATURES, _lib.TREND_SIGNATURES, _lib.CLIM_SIGNATURES,
                      _lib.GAUGE_SIGNATURES, _lib.SPICE_SIGNATURES):
            assert name not in table
    assert len(_lib.SIGNATURES) == 28 and len(_lib.SPICE_SIGNATURES) == 1
    assert _lib.ABI_VERSION == 9 and _lib.load().mlx_version() == 9


def test_argument_errors_need_no_gpu():
    lib = _lib.load_vort()
    f = 1 << 20  # 16-byte aligned, non-NULL, never dereferenced: the checks precede every HIP call
    F64, F32 = _lib.DTYPE_F64, _lib.DTYPE_F32

    def zeta(u=f, v=f, fdt=F64, dx=f, dy=f, area=f, mdt=F64, nrec=2, ny=4, nx=6, sym=0, out=f):
        return lib.mlx_vort_rel_vort(u, v, fdt, dx, dy, area, mdt, nrec, ny, nx, sym, out, None)

    def pv(z=f, zdt=F64, c=f, cdt=F64, n=f, ndt=F64, nrec=2, ny=4, nx=6, interp=1, sym=0, g=9.8,
           units=0, out=f):
        return lib.mlx_vort_pv(z, zdt, c, cdt, n, ndt, nrec, ny, nx, interp, sym, g, units, out, None)

    def rossby(c=f, cdt=F64, fp=f, fdt=F64, outer=2, plane=3, inner=4, out=f):
        return lib.mlx_vort_rossby(c, cdt, fp, fdt, outer, plane, inner, out, None)

    for kw in (dict(u=None), dict(v=None), dict(dx=None), dict(dy=None), dict(area=None), dict(out=None)):
        assert zeta(**kw) == -1 and "NULL" in _lib.last_error()
    for kw in (dict(z=None), dict(c=None), dict(n=None), dict(out=None)):
        assert pv(**kw) == -1 and "NULL" in _lib.last_error()
    for kw in (dict(c=None), dict(fp=None), dict(out=None)):
        assert rossby(**kw) == -1 and "NULL" in _lib.last_error()
    for kw in (dict(nrec=-1), dict(ny=0), dict(nx=0), dict(ny=-3), dict(ny=1, sym=1), dict(nx=1, sym=1),
               dict(nrec=1 << 20, ny=1 << 10, nx=(1 << 8) + 1), dict(ny=1 << 39), dict(ny=1 << 20, nx=1 << 20)):
        assert zeta(**kw) == -2 and _lib.last_error(), kw
        assert pv(**kw) == -2 and _lib.last_error(), kw
    for kw in (dict(outer=-1), dict(plane=-1), dict(inner=-1), dict(outer=1 << 20, plane=1 << 20)):
        assert rossby(**kw) == -2 and _lib.last_error(), kw
    for bad in (2, 3, 4, 7, -1):  # (MLX_DTYPE_F32_UPCAST and the mixed codes are not operand dtypes)
        assert zeta(fdt=bad) == -3 and zeta(mdt=bad) == -3
        assert pv(zdt=bad) == -3 and pv(cdt=bad) == -3 and pv(ndt=bad) == -3
        assert rossby(cdt=bad) == -3 and rossby(fdt=bad) == -3
    assert zeta(sym=2) == -3 and pv(sym=-1) == -3 and pv(interp=2) == -3
    assert pv(units=2) == -3 and "units" in _lib.last_error()
    for kw in (dict(u=f + 4), dict(v=f + 4), dict(dx=f + 4), dict(dy=f + 4), dict(area=f + 4), dict(out=f + 4),
               dict(u=f + 2, fdt=F32), dict(area=f + 1, mdt=F32), dict(out=f + 2, fdt=F32, mdt=F32)):
        assert zeta(**kw) == -5 and _lib.last_error(), kw
    for kw in (dict(z=f + 4), dict(c=f + 4), dict(n=f + 4), dict(out=f + 4), dict(n=f + 2, ndt=F32)):
        assert pv(**kw) == -5, kw
    assert rossby(c=f + 4) == -5 and rossby(fp=f + 2, fdt=F32) == -5 and rossby(out=f + 4) == -5
    # nothing to do: no launch, whatever the pointers
    assert zeta(nrec=0) == 0 and zeta(u=None, v=None, out=None, nrec=0) == 0
    assert pv(nrec=0) == 0 and rossby(outer=0) == 0 and rossby(c=None, inner=0) == 0


def test_a_library_without_the_kernels_is_an_error(monkeypatch):
    class Bare:
        def __getattr__(self, name):
            raise AttributeError(name)

    monkeypatch.setattr(_lib, "_vort_bound", False)
    monkeypatch.setattr(_lib, "load", lambda: Bare())
    with pytest.raises(_lib.MomlevelHipError, match="does not export mlx_vort_[a-z_]+: rebuild"):
        _lib.load_vort()


def test_vort_source_sha_is_its_own():
    from momlevel_amd.csrc import build

    assert len(build.vort_source_sha()) == 16
    assert build.vort_source_sha() not in (build.source_sha(), build.trend_source_sha(),
                                           build.clim_source_sha(), build.strat_source_sha(),
                                           build.gauge_source_sha(), build.spice_source_sha())
    names = {os.path.basename(p) for p in build.TIMED_SOURCES}
    assert "momlevel_vort.hip" not in names and "momlevel_vort.h" not in names
    assert any(p.endswith("momlevel_vort.hip") for p in build.SOURCES)
    assert any(p.endswith("momlevel_vort.hip") for p in build.DEPENDS)
    assert any(p.endswith("momlevel_vort.h") for p in build.DEPENDS)
    text = open(os.path.join(ROOT, "momlevel_amd", "csrc", "momlevel_vort.hip")).read()
    assert "#pragma clang fp contract(off)" in text


# ---- the public surface, without a device ---------------------------------------------------------
def test_signatures_are_the_references():
    for name in ("calc_coriolis", "calc_rel_vort", "calc_pv", "calc_rossby_rd"):
        assert name in derived.__all__
    assert list(inspect.signature(derived.calc_coriolis).parameters) == ["lat"]
    sig = inspect.signature(derived.calc_rel_vort)
    assert list(sig.parameters) == ["dset", "varname_map", "coord_dict", "symmetric"]
    assert [p.default for p in sig.parameters.values()][1:] == [None, None, False]
    sig = inspect.signature(derived.calc_pv)
    assert list(sig.parameters) == ["zeta", "coriolis", "n2", "gravity", "coord_dict", "symmetric",
                                    "units", "interp_n2"]
    assert [p.default for p in sig.parameters.values()][3:] == [9.8, None, False, "m", True]
    assert list(inspect.signature(derived.calc_rossby_rd).parameters) == ["wave_speed", "coriolis"]
    from momlevel_amd import test_data

    from momlevel_amd import staggered_data

    assert test_data.generate_test_data_uv is staggered_data.generate_test_data_uv  # one function, one place


def test_missing_fields_are_named():
    d = dset3.drop_vars(["vo", "dyCv"])
    with pytest.raises(ValueError, match="Input dataset missing fields: ") as exc:
        derived.calc_rel_vort(d)
    listed = re.search(r"\[(.*)\]", str(exc.value)).group(1)
    assert {s.strip(" '") for s in listed.split(",")} == {"vo", "dyCv"}
    with pytest.raises(ValueError, match="Input dataset missing fields: "):
        derived.calc_rel_vort(dset3, varname_map={"u": "uo", "v": "vo", "dx": "dxCu", "dy": "dyCv",
                                                  "area": "area_bu"})  # (not in this dataset)
    with pytest.raises(ValueError, match="coord_dict is missing the keys"):
        derived.calc_rel_vort(dset3, coord_dict={"xcenter": "xh", "ycenter": "yh"})


def test_unknown_units():
    zeta = DataArray(np.zeros((5, 5, 5, 5)), ("time", "z_l", "yq", "xq"))
    n2 = DataArray(np.zeros((5, 5, 5, 5)), ("time", "z_l", "yh", "xh"))
    with pytest.raises(ValueError, match="unknown units option `mm`"):
        derived.calc_pv(zeta, dset3.Coriolis, n2, units="mm")


def _swapped(da, *dims):
    return DataArray(np.ascontiguousarray(np.moveaxis(da.values, -1, -2)), dims, None, da.attrs)


def test_misplaced_dims_are_refused():
    d = dset3.copy()
    d["uo"] = _swapped(dset3.uo, "time", "z_l", "xq", "yh")
    with pytest.raises(ValueError, match=r"uo has dims \('time', 'z_l', 'xq', 'yh'\)"):
        derived.calc_rel_vort(d)
    d = dset3.copy()
    d["vo"] = DataArray(np.moveaxis(dset3.vo.values, 1, -1).copy(), ("time", "yq", "xh", "z_l"))
    with pytest.raises(ValueError, match=r"vo has dims \('time', 'yq', 'xh', 'z_l'\)"):
        derived.calc_rel_vort(d)
    d = dset3.copy()
    d["dxCu"] = _swapped(dset3.dxCu, "xq", "yh")
    with pytest.raises(ValueError, match=r"dxCu has dims \('xq', 'yh'\)"):
        derived.calc_rel_vort(d)
    d = dset3.copy()
    d["vo"] = dset3.vo.isel(time=slice(0, 3))
    with pytest.raises(ValueError, match="must share their leading dims"):
        derived.calc_rel_vort(d)
    zeta = DataArray(np.zeros((5, 5, 5)), ("z_l", "yq", "xq"))
    n2 = DataArray(np.zeros((5, 5, 5)), ("z_l", "yh", "xh"))
    with pytest.raises(ValueError, match=r"n2 has dims \('yh', 'z_l', 'xh'\)"):
        derived.calc_pv(zeta, dset3.Coriolis, DataArray(np.zeros((5, 5, 5)), ("yh", "z_l", "xh")))
    with pytest.raises(ValueError, match=r"coriolis has dims \('yh', 'xh'\)"):
        derived.calc_pv(zeta, DataArray(np.zeros((5, 5)), ("yh", "xh")), n2)
    with pytest.raises(ValueError, match="must share their leading dims"):
        derived.calc_pv(zeta, dset3.Coriolis, DataArray(np.zeros((4, 5, 5)), ("z_l", "yh", "xh")))
    with pytest.raises(ValueError, match="must lie on the points of zeta"):
        derived.calc_pv(zeta, dset3.Coriolis, n2, interp_n2=False)
    speed = DataArray(np.zeros((5, 4, 3)), ("yh", "time", "xh"))
    with pytest.raises(ValueError, match="not a contiguous run"):
        derived.calc_rossby_rd(speed, DataArray(np.ones((5, 3)), ("yh", "xh")))
    with pytest.raises(ValueError, match="does not fit"):
        derived.calc_rossby_rd(DataArray(np.zeros((4, 5, 3)), ("time", "yh", "xh")),
                               DataArray(np.ones((5, 4)), ("yh", "xh")))


def test_lengths_against_symmetric():
    # equal lengths are a non-symmetric grid ...
    with pytest.raises(ValueError, match=r"'yq' has 5 points and 'yh' has 5; a symmetric grid needs 6"):
        derived.calc_rel_vort(dset3, symmetric=True)
    # ... and corner dims one longer are a symmetric one
    d = Dataset()
    d["uo"] = DataArray(np.zeros((2, 4, 6)), ("z_l", "yh", "xq"))
    d["vo"] = DataArray(np.zeros((2, 5, 5)), ("z_l", "yq", "xh"))
    d["dxCu"] = DataArray(np.ones((4, 6)), ("yh", "xq"))
    d["dyCv"] = DataArray(np.ones((5, 5)), ("yq", "xh"))
    d["areacello_bu"] = DataArray(np.ones((5, 6)), ("yq", "xq"))
    with pytest.raises(ValueError, match=r"'yq' has 5 points and 'yh' has 4; a non-symmetric grid needs 4"):
        derived.calc_rel_vort(d)
    zeta = DataArray(np.zeros((2, 5, 6)), ("z_l", "yq", "xq"))
    n2 = DataArray(np.zeros((2, 4, 5)), ("z_l", "yh", "xh"))
    f = DataArray(np.zeros((5, 6)), ("yq", "xq"))
    with pytest.raises(ValueError, match="a non-symmetric grid needs 4 corner points"):
        derived.calc_pv(zeta, f, n2)
    with pytest.raises(ValueError, match="a symmetric grid needs 6 corner points"):
        derived.calc_pv(DataArray(np.zeros((2, 5, 5)), ("z_l", "yq", "xq")),
                        DataArray(np.zeros((5, 5)), ("yq", "xq")),
                        DataArray(np.zeros((2, 5, 5)), ("z_l", "yh", "xh")), symmetric=True)


def test_dtypes_are_checked_before_any_launch():
    d = dset3.copy()
    d["vo"] = dset3.vo.astype(np.float32)
    with pytest.raises(TypeError, match="uo is float64 and vo is float32"):
        derived.calc_rel_vort(d)
    for bad in (np.float16, np.longdouble, np.int32):
        d = dset3.copy()
        d["uo"], d["vo"] = dset3.uo.astype(bad), dset3.vo.astype(bad)
        with pytest.raises(TypeError):
            derived.calc_rel_vort(d)
    d = dset3.copy()
    d["dyCv"] = dset3.dyCv.astype(np.float32)
    with pytest.raises(TypeError, match="must share one dtype"):
        derived.calc_rel_vort(d)
    zeta = DataArray(np.zeros((5, 5, 5), np.float16), ("z_l", "yq", "xq"))
    with pytest.raises(TypeError):
        derived.calc_pv(zeta, dset3.Coriolis, DataArray(np.zeros((5, 5, 5)), ("z_l", "yh", "xh")))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_calc_coriolis_is_numpys_expression(dtype):
    lat = DataArray(dset1.geolat.values.astype(dtype), dset1.geolat.dims, dict(dset1.geolat.coords),
                    dset1.geolat.attrs, "geolat")
    f = derived.calc_coriolis(lat)
    want = 2.0 * (2.0 * np.pi / (60.0 * 60.0 * 24.0)) * np.sin(lat.values * np.pi / 180.0)
    assert type(f.values) is np.ndarray and f.values.dtype == want.dtype == dtype
    assert_bit_equal(f.values, want)
    assert_bit_equal(f.values, vn.coriolis(lat.values))
    assert f.dims == ("yh", "xh") and f.name is None and set(f.coords) == set(lat.coords)
    assert f.attrs == {"standard_name": "coriolis_parameter", "long_name": "Coriolis parameter",
                       "units": "s-1"}
    assert list(f.attrs) == ["standard_name", "long_name", "units"]
    if dtype == np.float64:
        _pin("calc_coriolis_sum", float(f.values.sum()))
    # a masked latitude means NaN; lat = 0 is exactly 0
    masked = np.ma.masked_array(lat.values, mask=lat.values > 50)
    fm = derived.calc_coriolis(DataArray(masked, ("yh", "xh")))
    assert np.array_equal(np.isnan(fm.values), lat.values > 50)
    assert derived.calc_coriolis(DataArray(np.zeros((1, 2)), ("yh", "xh"))).values.tolist() == [[0.0, 0.0]]


def test_no_undefined_globals_in_the_new_module():
    import importlib

    from test_static_names import _undefined

    assert _undefined(importlib.import_module("momlevel_amd.staggered_data")) == []
