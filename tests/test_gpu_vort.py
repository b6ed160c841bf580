"""GPU: core.rel_vort / potential_vorticity / rossby_radius (csrc/momlevel_vort.hip) and
derived.calc_rel_vort / calc_pv / calc_coriolis / calc_rossby_rd against the operator-for-operator
numpy restatement (tests/vort_numpy.py), BIT FOR BIT: over the edges of a pack, a wave and a tile
in x and in y, on both grids, for every dtype combination; and the kernels' own invariants -- a
cell depends on its own operands only, not on nrec, the tile, the alignment or the path."""

import numpy as np
import pytest
import torch

import vort_numpy as vn
from conftest import assert_bit_equal
from momlevel_amd import _lib, core, derived
from momlevel_amd.labeled import DataArray
from momlevel_amd.test_data import generate_test_data, generate_test_data_uv

pytestmark = pytest.mark.gpu

# the tile of the packed path (include/momlevel_vort.h; test_vort_host.py checks the mirror)
W64, W32 = _lib.VORT_TILE_LANES * 2, _lib.VORT_TILE_LANES * 4
H, BANDS = _lib.VORT_TILE_H, _lib.VORT_TILE_BANDS
NXS = sorted({1, 2, 3, 127, 128, 129, W64 - 1, W64, W64 + 1, W32 - 1, W32, W32 + 1})
NYS = sorted({1, 2, H - 1, H, H + 1, 2 * H + 1, BANDS * H + 1})  # (the last: a second block in y)
NREC = 3
F64, F32 = np.float64, np.float32
ZETA_DTYPES = [(F64, F64), (F32, F32), (F32, F64), (F64, F32)]  # (fields, metrics)
PV_DTYPES = [(z, c, n) for z in (F64, F32) for c in (F64, F32) for n in (F64, F32)]  # (zeta, f, n2)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, ref, what):
    """bit for bit (no NaN in the sweeps: the integer views must agree)"""
    got = got.cpu().numpy()
    assert got.dtype == ref.dtype and got.shape == ref.shape, f"{what}: {got.dtype}{got.shape} vs {ref.dtype}{ref.shape}"
    view = np.int64 if ref.dtype == F64 else np.int32
    if not np.array_equal(got.view(view), np.ascontiguousarray(ref).view(view)):
        assert_bit_equal(got, ref, what)
        raise AssertionError(f"{what}: bits differ")


@pytest.fixture(scope="module")
def pool():
    """random planes of the largest extents, in both dtypes, on the host and on the device; every
    case cuts its operands out of them"""
    rng = np.random.default_rng(20020187)
    ny, nx = max(NYS) + 1, max(NXS) + 1
    host = {
        "u": rng.normal(0.0061, 0.08, (NREC, ny, nx)), "v": rng.normal(0.00077, 0.04, (NREC, ny, nx)),
        "dx": rng.uniform(2.0e4, 3.0e4, (ny, nx)), "dy": rng.uniform(1.0e4, 3.0e4, (ny, nx)),
        "area": rng.uniform(4.0e8, 9.0e8, (ny, nx)), "zeta": rng.normal(0.0, 1.0e-5, (NREC, ny, nx)),
        "f": rng.normal(1.21e-5, 1.1e-4, (ny, nx)), "n2": rng.normal(1.0e-5, 2.0e-5, (NREC, ny, nx)),
    }
    out = {}
    for name, a in host.items():
        for dt in (F64, F32):
            b = a.astype(dt)
            out[name, dt] = (b, _dev(b))
    return out


def _cut(pool, name, dt, nrec, ny, nx):
    h, d = pool[name, dt]
    if h.ndim == 3:
        return np.ascontiguousarray(h[:nrec, :ny, :nx]), d[:nrec, :ny, :nx].contiguous()
    return np.ascontiguousarray(h[:ny, :nx]), d[:ny, :nx].contiguous()


# ---- the tiling sweep -----------------------------------------------------------------------------
@pytest.mark.parametrize("nx", NXS)
def test_rel_vort_over_the_edges_of_pack_wave_and_tile(pool, nx):
    cases = 0
    for nrec in (1, NREC):
        for ny in NYS:
            for s in (0, 1):
                if s and (ny < 2 or nx < 2):
                    continue  # (a symmetric corner plane has at least two points a side)
                for fd, md in ZETA_DTYPES:
                    uh, ud = _cut(pool, "u", fd, nrec, ny - s, nx)
                    vh, vd = _cut(pool, "v", fd, nrec, ny, nx - s)
                    dxh, dxd = _cut(pool, "dx", md, nrec, ny - s, nx)
                    dyh, dyd = _cut(pool, "dy", md, nrec, ny, nx - s)
                    ah, ad = _cut(pool, "area", md, nrec, ny, nx)
                    ref = vn.rel_vort(uh, vh, dxh, dyh, ah, symmetric=bool(s))
                    got = core.rel_vort(ud, vd, dxd, dyd, ad, symmetric=bool(s))
                    _same(got, ref, f"zeta nrec={nrec} ny={ny} nx={nx} sym={s} {fd.__name__}/{md.__name__}")
                    cases += 1
    print(f"nx={nx}: {cases} calls bit-identical to numpy")


@pytest.mark.parametrize("nx", NXS)
def test_pv_over_the_edges_of_pack_wave_and_tile(pool, nx):
    cases = 0
    for nrec in (1, NREC):
        for ny in NYS:
            for interp, s in ((0, 0), (1, 0), (1, 1)):
                if s and (ny < 2 or nx < 2):
                    continue
                for zd, cd, nd in PV_DTYPES:
                    zh, zt = _cut(pool, "zeta", zd, nrec, ny, nx)
                    fh, ft = _cut(pool, "f", cd, nrec, ny, nx)
                    nh, nt = _cut(pool, "n2", nd, nrec, ny - s, nx - s)
                    for units in ("m", "cm"):
                        ref = vn.pv(zh, fh, nh, gravity=9.8, symmetric=bool(s), units=units, interp=bool(interp))
                        got = core.potential_vorticity(zt, ft, nt, gravity=9.8, interp=bool(interp),
                                                       symmetric=bool(s), units=units)
                        _same(got, ref, f"pv nrec={nrec} ny={ny} nx={nx} interp={interp} sym={s} {units} "
                                        f"{zd.__name__}/{cd.__name__}/{nd.__name__}")
                        cases += 1
    print(f"nx={nx}: {cases} calls bit-identical to numpy")


# ---- a cell depends on its own operands only ------------------------------------------------------
def _five(pool, fd, md, ny, nx):
    rng = np.random.default_rng(5)
    u = _dev(rng.normal(0.0, 0.1, (5, ny, nx)).astype(fd))
    v = _dev(rng.normal(0.0, 0.1, (5, ny, nx)).astype(fd))
    n2 = _dev(rng.normal(1e-5, 2e-5, (5, ny, nx)).astype(fd))
    return u, v, n2, _cut(pool, "dx", md, 1, ny, nx)[1], _cut(pool, "dy", md, 1, ny, nx)[1], \
        _cut(pool, "area", md, 1, ny, nx)[1], _cut(pool, "f", md, 1, ny, nx)[1]


@pytest.mark.parametrize("nx", [W64 + 2, W64 + 1])  # (packed; cell by cell)
@pytest.mark.parametrize("fd,md", ZETA_DTYPES)
def test_record_slices_offset_pointers_and_two_runs(pool, fd, md, nx):
    ny = 2 * H + 1
    u, v, n2, dx, dy, area, f = _five(pool, fd, md, ny, nx)
    whole = core.rel_vort(u, v, dx, dy, area)
    pvs = {k: core.potential_vorticity(whole, f, n2, units=k) for k in ("m", "cm")}
    flat = core.potential_vorticity(whole, f, n2, interp=False)
    # records [1:3] of a five-record call are the call on the sliced views
    assert torch.equal(core.rel_vort(u[1:3], v[1:3], dx, dy, area), whole[1:3])
    for k in ("m", "cm"):
        assert torch.equal(core.potential_vorticity(whole[1:3], f, n2[1:3], units=k), pvs[k][1:3])
    assert torch.equal(core.potential_vorticity(whole[1:3], f, n2[1:3], interp=False), flat[1:3])
    # two runs agree
    assert torch.equal(core.rel_vort(u, v, dx, dy, area), whole)
    assert torch.equal(core.potential_vorticity(whole, f, n2, units="cm"), pvs["cm"])

    # every operand one element off a 16-byte boundary: the same bits
    def off(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
        view = buf[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        return view

    assert torch.equal(core.rel_vort(off(u), off(v), off(dx), off(dy), off(area)), whole)
    assert torch.equal(core.rel_vort(off(u), v, dx, dy, area), whole)
    assert torch.equal(core.rel_vort(u, v, dx, dy, off(area)), whole)
    out = off(torch.empty_like(whole))
    assert core.rel_vort(u, v, dx, dy, area, out=out).data_ptr() == out.data_ptr()
    assert torch.equal(out, whole)
    assert torch.equal(core.potential_vorticity(off(whole), off(f), off(n2)), pvs["m"])
    assert torch.equal(core.potential_vorticity(whole, f, off(n2), units="cm"), pvs["cm"])
    assert torch.equal(core.potential_vorticity(whole, off(f), n2, interp=False), flat)


@pytest.mark.parametrize("nx", [2 * W64 + 4, 2 * W64 + 3])  # (packed; cell by cell)
def test_nan_placement(nx):
    ny = BANDS * H + 2
    rng = np.random.default_rng(9)
    u, v = rng.normal(0.0, 0.1, (2, ny, nx)), rng.normal(0.0, 0.1, (2, ny, nx))
    one = _dev(np.ones((ny, nx)))
    f = _dev(rng.normal(1e-5, 1e-4, (ny, nx)))
    n2 = rng.normal(1e-5, 2e-5, (2, ny, nx))
    clean = core.rel_vort(_dev(u), _dev(v), one, one, one)
    assert bool(torch.isfinite(clean).all())  # the last row and column too: the padding is 0.0
    pv_clean = core.potential_vorticity(clean, f, _dev(n2))
    assert bool(torch.isfinite(pv_clean).all())
    # an interior cell, the edges of a pack, of a wave's tile in x and in y, of a block, the last ones
    for j, i in ((3, 5), (H, W64), (H - 1, W64 - 1), (BANDS * H, 2 * W64), (1, 1), (ny - 1, nx - 1), (0, 0)):
        un = u.copy()
        un[1, j, i] = np.nan
        got = torch.isnan(core.rel_vort(_dev(un), _dev(v), one, one, one)).cpu().numpy()
        want = np.zeros((2, ny, nx), bool)
        want[1, j, i] = True
        if j > 0:
            want[1, j - 1, i] = True
        assert np.array_equal(got, want), ("u", j, i)
        vn_ = v.copy()
        vn_[0, j, i] = np.nan
        got = torch.isnan(core.rel_vort(_dev(u), _dev(vn_), one, one, one)).cpu().numpy()
        want = np.zeros((2, ny, nx), bool)
        want[0, j, i] = True
        if i > 0:
            want[0, j, i - 1] = True
        assert np.array_equal(got, want), ("v", j, i)
        nn = n2.copy()
        nn[1, j, i] = np.nan
        got = torch.isnan(core.potential_vorticity(clean, f, _dev(nn))).cpu().numpy()
        want = np.zeros((2, ny, nx), bool)
        want[1, max(j - 1, 0):j + 1, max(i - 1, 0):i + 1] = True
        assert np.array_equal(got, want), ("n2", j, i)
        flat = torch.isnan(core.potential_vorticity(clean, f, _dev(nn), interp=False)).cpu().numpy()
        assert flat.sum() == 1 and flat[1, j, i]
        # the cells beside the poisoned ones are those of the clean call
        ok = ~got
        assert torch.equal(core.potential_vorticity(clean, f, _dev(nn))[torch.from_numpy(ok).cuda()],
                           pv_clean[torch.from_numpy(ok).cuda()])


def test_rossby_radius_layouts_and_dtypes():
    rng = np.random.default_rng(3)
    for cd in (F64, F32):
        for fd in (F64, F32):
            for outer, plane, inner in ((1, 35, 1), (4, 35, 1), (5, 35, 6), (1, 1, 7), (3, 300, 129)):
                c = rng.normal(2.0, 1.0, (outer, plane, inner)).astype(cd)
                f = rng.normal(0.0, 1e-4, plane).astype(fd)
                f[0] = 0.0
                c[0, 0, 0] = 0.0  # 0 / 0
                c[-1, 0, -1] = np.nan
                got = core.rossby_radius(_dev(c), _dev(f)).cpu().numpy()
                ref = vn.rossby_rd(c, f[None, :, None])
                assert got.dtype == ref.dtype
                assert_bit_equal(got, ref)
                assert np.array_equal(np.isinf(got), np.isinf(ref)) and np.isnan(got[0, 0, 0])


# ---- argument errors launch nothing ---------------------------------------------------------------
def test_argument_errors_launch_nothing():
    lib = _lib.load_vort()
    ny, nx = 4, 6
    t = {k: torch.ones((2, ny, nx) if k in "uvzn" else (ny, nx), dtype=torch.float64, device="cuda")
         for k in ("u", "v", "z", "n", "dx", "dy", "area", "f")}
    out = torch.full((2, ny, nx), -7.0, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    p = {k: x.data_ptr() for k, x in t.items()}
    o = out.data_ptr()
    D, S = _lib.DTYPE_F64, _lib.DTYPE_F32
    zeta = lambda *a: lib.mlx_vort_rel_vort(*a, st)  # noqa: E731
    pv = lambda *a: lib.mlx_vort_pv(*a, st)  # noqa: E731
    calls = {
        "zeta u NULL": (zeta(None, p["v"], D, p["dx"], p["dy"], p["area"], D, 2, ny, nx, 0, o), -1),
        "zeta out NULL": (zeta(p["u"], p["v"], D, p["dx"], p["dy"], p["area"], D, 2, ny, nx, 0, None), -1),
        "zeta nrec < 0": (zeta(p["u"], p["v"], D, p["dx"], p["dy"], p["area"], D, -2, ny, nx, 0, o), -2),
        "zeta nx = 0": (zeta(p["u"], p["v"], D, p["dx"], p["dy"], p["area"], D, 2, ny, 0, 0, o), -2),
        "zeta dtype": (zeta(p["u"], p["v"], 2, p["dx"], p["dy"], p["area"], D, 2, ny, nx, 0, o), -3),
        "zeta symmetric": (zeta(p["u"], p["v"], D, p["dx"], p["dy"], p["area"], D, 2, ny, nx, 3, o), -3),
        "zeta alignment": (zeta(p["u"] + 4, p["v"], D, p["dx"], p["dy"], p["area"], D, 1, ny, nx, 0, o), -5),
        "pv n2 NULL": (pv(p["z"], D, p["f"], D, None, D, 2, ny, nx, 1, 0, 9.8, 0, o), -1),
        "pv units": (pv(p["z"], D, p["f"], D, p["n"], D, 2, ny, nx, 1, 0, 9.8, 5, o), -3),
        "pv interp": (pv(p["z"], D, p["f"], D, p["n"], D, 2, ny, nx, 2, 0, 9.8, 0, o), -3),
        "pv dtype": (pv(p["z"], D, p["f"], 9, p["n"], D, 2, ny, nx, 1, 0, 9.8, 0, o), -3),
        "pv ny = 1, symmetric": (pv(p["z"], D, p["f"], D, p["n"], D, 2, 1, nx, 1, 1, 9.8, 0, o), -2),
        "pv out alignment": (pv(p["z"], D, p["f"], D, p["n"], D, 1, ny, nx, 1, 0, 9.8, 0, o + 4), -5),
        "rossby plane < 0": (lib.mlx_vort_rossby(p["u"], D, p["f"], D, 2, -1, 3, o, st), -2),
        "rossby f alignment": (lib.mlx_vort_rossby(p["u"], D, p["f"] + 2, S, 2, 4, 6, o, st), -5),
    }
    for what, (rc, code) in calls.items():
        assert rc == code, what
    assert zeta(p["u"], p["v"], D, p["dx"], p["dy"], p["area"], D, 0, ny, nx, 0, o) == 0
    assert lib.mlx_vort_rossby(p["u"], D, p["f"], D, 2, 0, 6, o, st) == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())  # nothing ran
    u, v, dx, dy, area, f, n2 = (t[k] for k in ("u", "v", "dx", "dy", "area", "f", "n"))
    for bad in (dict(u=u.cpu()), dict(v=v.float()), dict(area=area.float()), dict(dx=dx.half()),
                dict(u=u[:, :3]), dict(v=v[:1]), dict(dy=dy[:, :5]), dict(u=u[:, :, ::2], v=v[:, :, ::2]),
                dict(out=out.float()), dict(out=out[:1]), dict(symmetric=True)):
        kw = dict(u=u, v=v, dx=dx, dy=dy, area=area)
        kw.update(bad)
        with pytest.raises((TypeError, ValueError)):
            core.rel_vort(**kw)
    with pytest.raises(TypeError, match="u and v must have the same dtype"):
        core.rel_vort(u, v.float(), dx, dy, area)
    for bad in (dict(units="km"), dict(coriolis=f[:3]), dict(n2=n2[:1]), dict(symmetric=True),
                dict(zeta=u.half()), dict(out=out.float())):
        kw = dict(zeta=u, coriolis=f, n2=n2)
        kw.update(bad)
        with pytest.raises((TypeError, ValueError)):
            core.potential_vorticity(**kw)
    with pytest.raises((TypeError, ValueError)):
        core.rossby_radius(u, f[:2])
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ---- the public functions -------------------------------------------------------------------------
dset1 = generate_test_data()
dset3 = generate_test_data_uv()
ZETA_ATTRS = {"standard_name": "ocean_relative_vorticity", "long_name": "Ocean relative vorticity",
              "units": "s-1"}


def _on_device(da):
    return DataArray(_dev(da.values), da.dims, dict(da.coords), da.attrs, da.name)


def _pin(name, got):
    g = vn.goldens()
    half = g["half_unit_of_the_last_printed_digit"][name]
    print(f"{name}: kernels {got!r}, pinned {g[name]!r}, difference {abs(got - g[name]):.3e}, "
          f"half a unit of the last printed digit {half:.0e}")
    assert abs(got - g[name]) <= half, name


def test_the_references_pins_through_the_kernels():
    zeta = derived.calc_rel_vort(dset3)
    assert isinstance(zeta, DataArray) and type(zeta.values) is np.ndarray and not zeta.is_device
    assert zeta.dims == ("time", "z_l", "yq", "xq") and zeta.attrs == ZETA_ATTRS
    assert list(zeta.attrs) == list(ZETA_ATTRS)
    assert {"time", "z_l", "yq", "xq"} <= set(zeta.coords) and "xh" not in zeta.coords
    assert_bit_equal(zeta.values, vn.rel_vort(dset3.uo.values, dset3.vo.values, dset3.dxCu.values,
                                              dset3.dyCv.values, dset3.areacello_bu.values))
    print("sum of zeta:", repr(zeta.values.sum()), "(the reference's pin", vn.goldens()["calc_rel_vort_sum"],
          "constrains nothing)")
    n2 = derived.calc_n2(dset1.thetao, dset1.so)
    for units, name, attr in (("m", "calc_pv_m_sum", "m-1 s-1"), ("cm", "calc_pv_cm_sum", "10^14 cm-1 s-1")):
        pv = derived.calc_pv(zeta, dset3.Coriolis, n2, units=units)
        assert pv.dims == zeta.dims and type(pv.values) is np.ndarray
        assert pv.attrs == {"long_name": "Ocean potential vorticity", "units": attr}
        assert_bit_equal(pv.values, vn.pv(zeta.values, dset3.Coriolis.values, n2.values, units=units))
        _pin(name, float(pv.values.sum()))
    flat = derived.calc_pv(zeta, dset3.Coriolis, DataArray(n2.values, zeta.dims), interp_n2=False)
    assert_bit_equal(flat.values, vn.pv(zeta.values, dset3.Coriolis.values, n2.values, interp=False))
    # the Rossby radius of the (z_l, yh, xh, time) wave speed
    speed = derived.calc_wave_speed(n2, derived.calc_dz(dset1.z_l, dset1.z_i, dset1.deptho))
    assert speed.dims == ("z_l", "yh", "xh", "time")
    f = derived.calc_coriolis(dset1.geolat)
    rd = derived.calc_rossby_rd(speed, f)
    assert rd.dims == speed.dims and rd.name is None and type(rd.values) is np.ndarray
    assert rd.attrs == {"long name": "Rossby radius of deformation", "units": "m"}
    assert_bit_equal(rd.values, vn.rossby_rd(speed.values, f.values[None, :, :, None]))
    _pin("calc_rossby_rd_sum", float(np.nansum(np.where(np.isinf(rd.values), np.nan, rd.values))))


def test_device_in_device_out_and_float32():
    d = dset3.copy()
    for k in ("uo", "vo", "dxCu", "dyCv", "areacello_bu"):
        d[k] = _on_device(dset3[k])
    zeta = derived.calc_rel_vort(d)
    assert zeta.is_device and zeta.dims == ("time", "z_l", "yq", "xq")
    host = derived.calc_rel_vort(dset3)
    assert_bit_equal(zeta.values, host.values)
    n2 = derived.calc_n2(dset1.thetao, dset1.so)
    pv = derived.calc_pv(zeta, _on_device(dset3.Coriolis), _on_device(n2), units="cm")
    assert pv.is_device
    assert_bit_equal(pv.values, derived.calc_pv(host, dset3.Coriolis, n2, units="cm").values)
    f = derived.calc_coriolis(_on_device(dset1.geolat))
    assert f.is_device
    assert_bit_equal(f.values, vn.coriolis(dset1.geolat.values))
    # float32 throughout is float32 arithmetic; float32 fields on float64 metrics are float64
    d32 = dset3.copy()
    for k in ("uo", "vo"):
        d32[k] = dset3[k].astype(F32)
    z = derived.calc_rel_vort(d32)
    assert z.values.dtype == F64
    assert_bit_equal(z.values, vn.rel_vort(d32.uo.values, d32.vo.values, dset3.dxCu.values,
                                           dset3.dyCv.values, dset3.areacello_bu.values))
    for k in ("dxCu", "dyCv", "areacello_bu"):
        d32[k] = dset3[k].astype(F32)
    z = derived.calc_rel_vort(d32)
    assert z.values.dtype == F32
    assert_bit_equal(z.values, vn.rel_vort(d32.uo.values, d32.vo.values, d32.dxCu.values,
                                           d32.dyCv.values, d32.areacello_bu.values))
    pv32 = derived.calc_pv(z, dset3.Coriolis.astype(F32), n2.astype(F32), units="cm")
    assert pv32.values.dtype == F32
    assert_bit_equal(pv32.values, vn.pv(z.values, dset3.Coriolis.values.astype(F32),
                                        n2.values.astype(F32), units="cm"))
    # masked arrays mean NaN
    from lazy_array import as_masked

    un = dset3.uo.values.copy()
    un[2, 1, 3, 2] = np.nan
    dm, dn = dset3.copy(), dset3.copy()
    dm["uo"] = DataArray(as_masked(un), dset3.uo.dims)
    dn["uo"] = DataArray(un, dset3.uo.dims)
    zm = derived.calc_rel_vort(dm).values
    assert np.isnan(zm).sum() == 2
    assert_bit_equal(zm, derived.calc_rel_vort(dn).values)


def test_a_symmetric_grid_and_other_dimension_names():
    rng = np.random.default_rng(77)
    ny, nx = 7, 9  # centre points; corners are one longer
    from momlevel_amd.labeled import Dataset

    d = Dataset()
    d["u"] = DataArray(rng.normal(0, 0.1, (3, ny, nx + 1)), ("lev", "y", "xc"))
    d["v"] = DataArray(rng.normal(0, 0.1, (3, ny + 1, nx)), ("lev", "yc", "x"))
    d["dxu"] = DataArray(rng.uniform(1e4, 2e4, (ny, nx + 1)), ("y", "xc"))
    d["dyv"] = DataArray(rng.uniform(1e4, 2e4, (ny + 1, nx)), ("yc", "x"))
    d["abu"] = DataArray(rng.uniform(1e8, 2e8, (ny + 1, nx + 1)), ("yc", "xc"))
    names = {"xcenter": "x", "ycenter": "y", "xcorner": "xc", "ycorner": "yc"}
    vmap = {"u": "u", "v": "v", "dx": "dxu", "dy": "dyv", "area": "abu"}
    zeta = derived.calc_rel_vort(d, varname_map=vmap, coord_dict=names, symmetric=True)
    assert zeta.dims == ("lev", "yc", "xc") and zeta.shape == (3, ny + 1, nx + 1)
    assert_bit_equal(zeta.values, vn.rel_vort(d.u.values, d.v.values, d.dxu.values, d.dyv.values,
                                              d.abu.values, symmetric=True))
    f = DataArray(rng.normal(0, 1e-4, (ny + 1, nx + 1)), ("yc", "xc"))
    n2 = DataArray(rng.normal(1e-5, 1e-5, (3, ny, nx)), ("lev", "y", "x"))
    pv = derived.calc_pv(zeta, f, n2, gravity=9.81, coord_dict=names, symmetric=True)
    assert_bit_equal(pv.values, vn.pv(zeta.values, f.values, n2.values, gravity=9.81, symmetric=True))


def test_calc_rossby_rd_layouts_with_the_equator():
    rng = np.random.default_rng(21)
    lat = np.array([[-30.0, 0.0, 30.0], [0.0, 45.0, 60.0]])
    f = derived.calc_coriolis(DataArray(lat, ("yh", "xh")))
    assert f.values[0, 1] == 0.0 and f.values[1, 0] == 0.0
    c2 = rng.uniform(0.5, 3.0, (2, 3))
    c2[1, 0] = 0.0  # 0 / 0 at the equator
    c2[1, 2] = np.nan
    for speed, shaped in ((DataArray(c2, ("yh", "xh")), f.values),
                          (DataArray(np.stack([c2, 2 * c2]), ("time", "yh", "xh")), f.values[None]),
                          (DataArray(np.stack([c2, 2 * c2, 3 * c2])[..., None] * np.ones(4), ("z_l", "yh", "xh", "time")),
                           f.values[None, :, :, None])):
        rd = derived.calc_rossby_rd(speed, f)
        ref = vn.rossby_rd(speed.values, shaped)
        assert rd.dims == speed.dims and rd.values.dtype == F64
        assert_bit_equal(rd.values, ref)
        assert np.array_equal(np.isinf(rd.values), np.isinf(ref)) and np.isinf(rd.values).any()
        assert np.isnan(rd.values).sum() == 2 * speed.values.size // c2.size
    dev = derived.calc_rossby_rd(_on_device(DataArray(c2, ("yh", "xh"))), f)
    assert dev.is_device
    assert_bit_equal(dev.values, vn.rossby_rd(c2, f.values))
    r32 = derived.calc_rossby_rd(DataArray(c2.astype(F32), ("yh", "xh")), DataArray(f.values.astype(F32), ("yh", "xh")))
    assert r32.values.dtype == F32
    assert_bit_equal(r32.values, vn.rossby_rd(c2.astype(F32), f.values.astype(F32)))


def test_xarray_in_kind(monkeypatch):
    import fake_xarray
    from momlevel_amd import adapters

    monkeypatch.setattr(adapters, "xr", fake_xarray)
    x = adapters.to_xarray(dset3)
    zeta = derived.calc_rel_vort(x)
    assert isinstance(zeta, fake_xarray.DataArray) and zeta.dims == ("time", "z_l", "yq", "xq")
    assert dict(zeta.attrs) == ZETA_ATTRS and "yq" in zeta.coords
    host = derived.calc_rel_vort(dset3)
    assert_bit_equal(np.asarray(zeta.values), host.values)
    n2 = derived.calc_n2(dset1.thetao, dset1.so)
    pv = derived.calc_pv(zeta, x["Coriolis"], adapters.to_xarray(n2))
    assert isinstance(pv, fake_xarray.DataArray)
    assert_bit_equal(np.asarray(pv.values), derived.calc_pv(host, dset3.Coriolis, n2).values)
    f = derived.calc_coriolis(adapters.to_xarray(dset1.geolat))
    assert isinstance(f, fake_xarray.DataArray) and dict(f.attrs)["units"] == "s-1"
    rd = derived.calc_rossby_rd(adapters.to_xarray(DataArray(np.ones((5, 5)), ("yh", "xh"))), f)
    assert isinstance(rd, fake_xarray.DataArray) and "long name" in rd.attrs


def test_lazy_4d_fields_walk_groups_of_time_steps(monkeypatch):
    from lazy_array import CountingLazy, MaskedLazy
    from momlevel_amd import hostio

    zeta_ref = derived.calc_rel_vort(dset3).values
    n2 = derived.calc_n2(dset1.thetao, dset1.so)
    pv_ref = derived.calc_pv(DataArray(zeta_ref, ("time", "z_l", "yq", "xq")), dset3.Coriolis, n2, units="cm").values
    pieces = []
    real = hostio.Uploader.submit

    def counting(self, arrays):
        pieces.append([tuple(a.shape) for a in arrays])
        return real(self, arrays)

    monkeypatch.setattr(hostio.Uploader, "submit", counting)
    monkeypatch.setattr(hostio, "PIPELINE_ELEMS", 100)
    monkeypatch.setattr(hostio, "PIECE_ELEMS", 2 * 125)  # two time steps a group
    d = dset3.copy()
    lazy_u, lazy_v = CountingLazy(dset3.uo.values), MaskedLazy(dset3.vo.values)
    d["uo"] = DataArray(lazy_u, dset3.uo.dims)
    d["vo"] = DataArray(lazy_v, dset3.vo.dims)
    zeta = derived.calc_rel_vort(d)
    assert type(zeta.values) is np.ndarray
    assert_bit_equal(zeta.values, zeta_ref)
    assert pieces == [[(2, 5, 5, 5)] * 2] * 2 + [[(1, 5, 5, 5)] * 2]
    assert len(lazy_u.reads) == 3 and lazy_u.largest_read == 2 * 125 * 8 and len(lazy_v.reads) == 3
    pieces.clear()
    lazy_n = CountingLazy(n2.values)
    pv = derived.calc_pv(DataArray(zeta_ref, ("time", "z_l", "yq", "xq")), dset3.Coriolis,
                         DataArray(lazy_n, n2.dims), units="cm")
    assert_bit_equal(pv.values, pv_ref)
    assert len(pieces) == 3 and len(lazy_n.reads) == 3 and lazy_n.largest_read == 2 * 125 * 8
    pieces.clear()
    assert_bit_equal(derived.calc_rel_vort(dset3).values, zeta_ref)  # plain host arrays walk too
    assert len(pieces) == 3
