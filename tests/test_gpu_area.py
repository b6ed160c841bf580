"""GPU: core.area_mean / area_anomaly (csrc/momlevel_area.hip) and regional.area_mean /
area_anomaly against the numpy restatement tests/area_numpy.py -- the only yardstick: the functions
are an extension, the reference has no counterpart.

The gates are the project's gate for every sum (README, "Sums ... gate 1e-10"), on the scale of the
sum itself:  |mean - mean_ref| <= 1e-10 * sum|w v| / den_ref  and  |den - den_ref| <= 1e-10 * den_ref,
NaN placement identical.  (On the CPU a pairwise and a sequential order of the same terms differ by
about 3e-17 of that scale on a 33 x 257 plane.)  Every test prints the worst ratio it saw.  The
invariants -- two runs, the split of the records, offset pointers, a record of ones, host against
device input -- and the anomaly are BIT FOR BIT."""

import numpy as np
import pytest
import torch

import area_numpy as an
from momlevel_amd import core, derived, regional
from momlevel_amd.labeled import DataArray
from momlevel_amd.steric import steric
from momlevel_amd.test_data import generate_test_data

pytestmark = pytest.mark.gpu

GATE = 1e-10
F64, F32 = np.float64, np.float32
CAP, WINDOW = core.AREA_MAX_SLOTS, core.AREA_WINDOW
NRECS = (1, 2, WINDOW + 1)


def _factor(n):
    """a true 2-D factorisation of n closest to a square, or None for a prime"""
    for a in range(int(n ** 0.5), 1, -1):
        if n % a == 0:
            return (a, n // a)
    return None


PLANES = ["1", "3x5", "7x129", "tile-1", "tile", "tile+1", "2tile+3"]


def _planes(name, dtype):
    """the planes of one case: the named size as (1, n) and, where n has one, as a true 2-D
    factorisation"""
    if "tile" not in name:
        return [tuple(int(n) for n in name.split("x"))] if "x" in name else [(1, 1)]
    tile = core.area_tile(dtype)
    n = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "2tile+3": 2 * tile + 3}[name]
    return [(1, n)] + ([_factor(n)] if _factor(n) else [])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int64)


def _case(shape, nrec, vdt, adt, seed):
    """a record with about 30 % land (NaN in every record), a few NaNs of its own per record, one
    all-NaN record (the second, when there is one), and an area with NaNs of its own"""
    rng = np.random.default_rng(seed)
    v = rng.normal(0.1, 1.0, (nrec,) + shape)
    land = rng.random(shape) < 0.3
    v[:, land] = np.nan
    v[rng.random(v.shape) < 0.02] = np.nan
    if nrec >= 2:
        v[1] = np.nan
    area = rng.uniform(4.0e8, 9.0e8, shape)
    area[rng.random(shape) < 0.05] = np.nan
    return v.astype(vdt), area.astype(adt)


def _gate(mean, den, v, area, label=None, ids=None, what=""):
    """the value gates of the module docstring; returns the worst ratios (mean, den)"""
    mean, den = np.asarray(mean), np.asarray(den)
    ref, den_ref = an.area_mean(v, area, label, ids)
    assert mean.dtype == den.dtype == F64 and mean.shape == ref.shape == den.shape, what
    assert np.array_equal(np.isnan(mean), np.isnan(ref)), f"{what}: NaN placement of the mean"
    assert not np.isnan(den).any(), what
    regions = [np.ones(area.shape, bool)] if label is None else [label == r for r in ids]
    scale = []
    for inside in regions:
        valid = ~np.isnan(v) & ~np.isnan(area) & inside
        w = np.where(valid, area.astype(F64), 0.0)
        scale.append(np.abs(w * np.where(valid, v.astype(F64), 0.0)).sum(axis=(-2, -1)))
    scale = scale[0] if label is None else np.stack(scale, axis=-1)
    ok = den_ref > 0
    assert np.array_equal(den == 0, ~ok), f"{what}: where nothing is valid"
    worst_m = worst_d = 0.0
    if ok.any():
        worst_d = float(np.max(np.abs(den - den_ref)[ok] / den_ref[ok]))
        nz = ok & (scale > 0)
        assert np.all(mean[ok & ~nz] == 0.0), what  # (every valid value 0: the mean is 0)
        if nz.any():
            worst_m = float(np.max(np.abs(mean - ref)[nz] / (scale[nz] / den_ref[nz])))
    assert worst_m <= GATE and worst_d <= GATE, f"{what}: mean {worst_m:.2e} den {worst_d:.2e}"
    return worst_m, worst_d


# ---- the tiling sweep -----------------------------------------------------------------------------
@pytest.mark.parametrize("vdt", [F64, F32], ids=["v64", "v32"])
@pytest.mark.parametrize("plane", PLANES)
def test_global_mean_over_the_edges_of_the_tile(vdt, plane):
    worst = (0.0, 0.0)
    for k, shape in enumerate(_planes(plane, vdt)):
        for nrec in NRECS:
            for adt in (F64, F32):
                v, area = _case(shape, nrec, vdt, adt, 10 * PLANES.index(plane) + 100 * k + nrec)
                mean, den = core.area_mean(_dev(v).reshape(nrec, -1), _dev(area).reshape(-1))
                r = _gate(mean.cpu().numpy()[:, 0], den.cpu().numpy()[:, 0], v, area,
                          what=f"{shape} nrec={nrec} {vdt.__name__}/{adt.__name__}")
                worst = max(worst[0], r[0]), max(worst[1], r[1])
    print(f"plane {plane} {_planes(plane, vdt)} {vdt.__name__}: worst ratio mean {worst[0]:.2e}, "
          f"den {worst[1]:.2e} (gate {GATE:.0e})")


# ---- regions ----------------------------------------------------------------------------------------
def _labels(shape, ids, seed):
    """every id, 0 and -3 scattered over the plane"""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array(list(ids) + [0, -3]), size=shape)


@pytest.mark.parametrize("nids", [1, 3, CAP, CAP + 1])
@pytest.mark.parametrize("vdt", [F64, F32], ids=["v64", "v32"])
def test_regional_means(vdt, nids):
    tile = core.area_tile(vdt)
    shape = (1, 2 * tile + 3) if nids != 3 else _factor(tile + 1) or (1, tile + 1)
    ids = [2, 7, 1000] if nids == 3 else list(range(3, 3 + 2 * nids, 2))
    nrec = 3
    v, area = _case(shape, nrec, vdt, F64, 40 + nids)
    label = _labels(shape, ids, 50 + nids)
    v[2][label == ids[-1]] = np.nan  # a region without a valid cell in one record
    eta = DataArray(_dev(v), ("time", "yh", "xh"), None, {"long_name": "eta", "units": "m"}, "eta")
    a = DataArray(_dev(area), ("yh", "xh"))
    mean, den = regional.area_mean(eta, a, regions=label, return_area=True)
    assert mean.is_device and den.is_device and mean.dims == ("time", "region")
    assert mean.coords["region"].values.tolist() == sorted(ids)
    m, d = mean.values, den.values
    worst = _gate(m, d, v, area, label, sorted(ids), what=f"{nids} regions {vdt.__name__}")
    last = sorted(ids).index(ids[-1])
    assert np.isnan(m[2, last]) and d[2, last] == 0.0 and np.isfinite(m[0, last])
    assert np.isnan(m[1]).all() and np.isfinite(np.delete(m[2], last)).all()
    # labels 0 and -3 are in no region: the valid areas of the regions leave theirs out
    out = np.isin(label, (0, -3)) & ~np.isnan(area) & ~np.isnan(v[0])
    total = np.where(~np.isnan(v[0]) & ~np.isnan(area), area, 0.0).sum()
    assert out.any() and abs(d[0].sum() - (total - area[out].sum())) <= 1e-9 * total
    # an explicit order, an absent id: the same bits row by row, NaN for the absent one
    order = [ids[-1], 999999] + ids[:-1]
    m2 = regional.area_mean(eta, a, regions=label.astype(F32), region_ids=order).values
    assert np.isnan(m2[:, 1]).all()
    back = [sorted(ids).index(r) for r in [ids[-1]] + ids[:-1]]
    # (a slot's sums do not depend on the other slots or on the launch it went in: the same bits)
    assert np.array_equal(_bits(np.delete(m2, 1, axis=1)), _bits(m[:, back]))
    print(f"{nids} regions {vdt.__name__}: worst ratio mean {worst[0]:.2e}, den {worst[1]:.2e}")


@pytest.mark.parametrize("vdt", [F64, F32], ids=["v64", "v32"])
def test_no_slot_map_is_a_map_of_one_label(vdt):
    tile = core.area_tile(vdt)
    nrec, plane = 3, 2 * tile + 3
    v, area = _case((1, plane), nrec, vdt, F32, 61)
    vd, ad = _dev(v).reshape(nrec, plane), _dev(area).reshape(plane)
    m0, d0 = core.area_mean(vd, ad)
    m1, d1 = core.area_mean(vd, ad, torch.zeros(plane, dtype=torch.int32, device="cuda"), 1)
    assert np.array_equal(_bits(m0), _bits(m1)) and np.array_equal(_bits(d0), _bits(d1))
    # ... and a slot of its own among others changes nothing for it either
    slot = torch.full((plane,), 2, dtype=torch.int32, device="cuda")
    m3, d3 = core.area_mean(vd, ad, slot, 3)
    assert np.array_equal(_bits(m0[:, 0]), _bits(m3[:, 2])) and np.array_equal(_bits(d0[:, 0]), _bits(d3[:, 2]))
    assert np.isnan(m3[:, :2].cpu().numpy()).all() and (d3[:, :2] == 0).all()


# ---- invariants, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("vdt", [F64, F32], ids=["v64", "v32"])
def test_runs_splits_and_offset_pointers_give_the_same_bits(vdt):
    tile = core.area_tile(vdt)
    nrec, plane = WINDOW + 8, tile + 7  # (an odd plane: every other record starts off a pack)
    ids = [2, 7, 1000]
    v, area = _case((1, plane), nrec, vdt, F64, 71)
    label = _labels((1, plane), ids, 72)
    _, slot = regional.plan_regions(label)
    vd, ad, sd = _dev(v).reshape(nrec, plane), _dev(area).reshape(plane), _dev(slot).reshape(plane)
    for args in ((vd, ad), (vd, ad, sd, 3)):
        m, d = core.area_mean(*args)
        m2, d2 = core.area_mean(*args)
        assert np.array_equal(_bits(m), _bits(m2)) and np.array_equal(_bits(d), _bits(d2))  # two runs
        # records [0:5] in one call, [0:2] and [2:5] in two; and a split inside a later window
        for lo, cut, hi in ((0, 2, 5), (0, 7, nrec)):
            whole = core.area_mean(args[0][lo:hi].contiguous(), *args[1:])
            parts = [core.area_mean(args[0][a:b].contiguous(), *args[1:]) for a, b in ((lo, cut), (cut, hi))]
            for k in (0, 1):
                assert np.array_equal(_bits(whole[k]), _bits(torch.cat([p[k] for p in parts])))
                assert np.array_equal(_bits(whole[k]), _bits((m, d)[k][lo:hi]))
    # the same plane through pointers offset by one element: views into padded buffers
    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
        buf[1:] = t.reshape(-1)
        out = buf[1:].view(t.shape)
        assert out.is_contiguous() and out.data_ptr() == buf.data_ptr() + t.element_size()
        return out

    m, d = core.area_mean(vd, ad, sd, 3)
    for moved in ((shifted(vd), ad, sd), (vd, shifted(ad), sd), (vd, ad, shifted(sd)),
                  (shifted(vd), shifted(ad), shifted(sd))):
        ms, ds = core.area_mean(*moved, 3)
        assert np.array_equal(_bits(m), _bits(ms)) and np.array_equal(_bits(d), _bits(ds))
    anom = core.area_anomaly(vd, m, sd)
    out = shifted(torch.empty_like(anom))
    for moved in ((shifted(vd), sd, None), (vd, shifted(sd), None), (vd, sd, out)):
        got = core.area_anomaly(moved[0], m, moved[1], out=moved[2])
        assert np.array_equal(_bits(anom), _bits(got))


@pytest.mark.parametrize("vdt", [F64, F32], ids=["v64", "v32"])
def test_a_record_of_ones_has_a_mean_of_exactly_one(vdt):
    tile = core.area_tile(vdt)
    shape = (3, tile + 5)
    v, area = _case(shape, 2, vdt, F64, 81)
    ones = np.where(np.isnan(v[0]), np.nan, 1.0).astype(vdt)[None]
    label = _labels(shape, [2, 7, 1000], 82)
    label[:, :9] = 55  # a region that is all land
    ones[0][label == 55] = np.nan
    eta, a = DataArray(_dev(ones), ("time", "yh", "xh")), DataArray(_dev(area), ("yh", "xh"))
    for kw in ({}, dict(regions=label)):
        mean, den = regional.area_mean(eta, a, return_area=True, **kw)
        m, d = mean.values, den.values
        assert (d > 0).any() and np.all(m[d > 0] == 1.0) and np.isnan(m[d == 0]).all()
    assert (d == 0).sum() == 1


def test_host_input_equals_device_input(monkeypatch):
    from lazy_array import CountingLazy

    tile = core.area_tile(F64)
    shape, nt, nz = (3, tile // 2 + 5), 5, 2
    rng = np.random.default_rng(91)
    v = rng.normal(size=(nt, nz) + shape)
    v[:, :, rng.random(shape) < 0.3] = np.nan
    area = rng.uniform(1.0, 2.0, shape).astype(F32)
    label = _labels(shape, [2, 7, 1000], 92)
    dims = ("time", "z_l", "yh", "xh")
    a = DataArray(area, ("yh", "xh"))
    dev = DataArray(_dev(v), dims)
    want_m, want_d = regional.area_mean(dev, DataArray(_dev(area), ("yh", "xh")), regions=label, return_area=True)
    want_a = regional.area_anomaly(dev, a, regions=label)
    assert want_m.is_device and want_a.is_device and want_m.dims == ("time", "z_l", "region")
    host = DataArray(v, dims)
    plain = regional.area_mean(host, a, regions=label)  # a small host record: one upload
    assert type(plain.values) is np.ndarray and np.array_equal(_bits(plain.values), _bits(want_m.values))
    pieces = []
    from momlevel_amd import hostio

    real = hostio.Uploader.submit

    def counting(self, arrays):
        pieces.append([tuple(x.shape) for x in arrays])
        return real(self, arrays)

    monkeypatch.setattr(hostio.Uploader, "submit", counting)
    monkeypatch.setattr(hostio, "PIPELINE_ELEMS", 100)
    monkeypatch.setattr(hostio, "PIECE_ELEMS", 2 * nz * shape[0] * shape[1])  # two steps a group
    for src in (host, DataArray(CountingLazy(v), dims)):
        pieces.clear()
        m, d = regional.area_mean(src, a, regions=label, return_area=True)
        assert pieces == [[(2, nz) + shape]] * 2 + [[(1, nz) + shape]]
        assert type(m.values) is np.ndarray and m.values.shape == (nt, nz, 3)
        assert np.array_equal(_bits(m.values), _bits(want_m.values))
        assert np.array_equal(_bits(d.values), _bits(want_d.values))
        an_, mm = regional.area_anomaly(src, a, regions=label, return_mean=True)
        assert type(an_.values) is np.ndarray and an_.values.shape == v.shape
        assert np.array_equal(_bits(an_.values), _bits(want_a.values))
        assert np.array_equal(_bits(mm.values), _bits(want_m.values))
        g = regional.area_mean(src, a)
        assert np.array_equal(_bits(g.values), _bits(regional.area_mean(dev, a).values))
    lazy = CountingLazy(v)
    regional.area_mean(DataArray(lazy, dims), a)
    assert len(lazy.reads) == 3 and lazy.largest_read == 2 * nz * shape[0] * shape[1] * 8  # never whole


# ---- the anomaly ------------------------------------------------------------------------------------
@pytest.mark.parametrize("vdt", [F64, F32], ids=["v64", "v32"])
def test_anomaly_is_numpys_subtraction_of_the_kernels_mean(vdt):
    tile = core.area_tile(vdt)
    ids = [2, 7, 1000]
    for shape, nrec in (((7, 129), 2), ((1, 2 * tile + 3), WINDOW + 1), (_factor(tile - 1), 3)):
        v, area = _case(shape, nrec, vdt, F32, 101 + nrec)
        label = _labels(shape, ids, 102)
        eta, a = DataArray(_dev(v), ("time", "yh", "xh")), DataArray(_dev(area), ("yh", "xh"))
        for kw, lab in ((dict(regions=label), label), ({}, None)):
            anom, mean = regional.area_anomaly(eta, a, return_mean=True, **kw)
            assert anom.is_device and anom.dims == eta.dims and anom.values.dtype == F64
            same = regional.area_mean(eta, a, **kw)
            assert np.array_equal(_bits(mean.values), _bits(same.values))  # the mean area_mean returns
            want = an.area_anomaly(v, mean.values, lab, ids)
            assert np.array_equal(np.isnan(anom.values), np.isnan(want))
            assert np.array_equal(_bits(anom.values), _bits(want)), f"{shape} {vdt.__name__} {sorted(kw)}"
            if lab is not None:
                assert np.isnan(anom.values[:, np.isin(label, (0, -3))]).all()  # NaN outside the regions
                inside = np.isin(label, ids) & ~np.isnan(v[0])
                assert inside.any() and np.isfinite(anom.values[0][inside]).all()


# ---- end to end -------------------------------------------------------------------------------------
def test_the_global_mean_of_a_steric_result_end_to_end(monkeypatch):
    d = generate_test_data()
    dd = d.copy()
    for k in ("thetao", "so", "volcello"):
        dd[k] = DataArray(torch.from_numpy(d[k].values).cuda(), d[k].dims)
    res, _ = steric(dd, domain="local")
    eta = res["steric"]
    assert eta.is_device and eta.dims[-2:] == ("yh", "xh")
    from momlevel_amd import hostio

    moved = []
    for name in ("to_device", "to_host", "upload", "download_into"):
        real = getattr(hostio, name)

        def spy(*args, _real=real, _name=name, **kw):
            moved.append((_name, max(a.numel() * a.element_size() if isinstance(a, torch.Tensor)
                                     else getattr(a, "nbytes", 0) for a in args)))
            return _real(*args, **kw)

        monkeypatch.setattr(hostio, name, spy)
    mean, den = regional.area_mean(eta, d["areacello"], return_area=True)
    anom = regional.area_anomaly(eta, d["areacello"])
    monkeypatch.undo()
    assert mean.is_device and den.is_device and anom.is_device and mean.dims == eta.dims[:-2]
    plane = d["areacello"].values.size * 8
    print("host link on the device path:", moved)
    assert all(nbytes <= plane for _, nbytes in moved)  # the 2-D map only, never the record
    field, area = eta.values, d["areacello"].values
    worst = _gate(mean.values, den.values, field, area, what="steric")
    # the anomaly has an area mean of zero, on the scale of the gate
    am, ad = regional.area_mean(anom, d["areacello"], return_area=True)
    valid = ~np.isnan(field) & ~np.isnan(area)
    w = np.where(valid, area, 0.0)
    scale = np.abs(w * np.where(valid, field, 0.0)).sum(axis=(-2, -1)) / den.values
    assert not np.isnan(am.values).any() and np.all(np.abs(am.values) <= GATE * scale)
    pos = scale > 0  # (the first step of a steric record is 0.0 everywhere: its scale is 0)
    ratio = float(np.max(np.abs(am.values)[pos] / scale[pos]))
    print(f"steric: worst ratio mean {worst[0]:.2e}, den {worst[1]:.2e}; mean of the anomaly {ratio:.2e} "
          f"of the scale (gate {GATE:.0e})")
    assert ratio <= GATE
    assert mean.attrs["cell_methods"] == "area: mean" and mean.attrs.get("units") == eta.attrs.get("units")


def test_xarray_in_kind(monkeypatch):
    import fake_xarray
    from momlevel_amd import adapters

    monkeypatch.setattr(adapters, "xr", fake_xarray)
    v, area = _case((7, 129), 3, F32, F64, 111)
    label = _labels((7, 129), [2, 7, 1000], 112)
    eta = DataArray(v, ("time", "yh", "xh"), {"time": DataArray(np.arange(3.0), ("time",))},
                    {"long_name": "eta", "units": "m"}, "eta")
    a = DataArray(area, ("yh", "xh"))
    x, xa = adapters.to_xarray(eta), adapters.to_xarray(a)
    xl = adapters.to_xarray(DataArray(label, ("yh", "xh")))
    mean = regional.area_mean(x, xa, regions=xl)
    assert isinstance(mean, fake_xarray.DataArray) and mean.dims == ("time", "region")
    assert dict(mean.attrs) == {"long_name": "Area-weighted mean of eta", "units": "m",
                                "cell_methods": "area: mean"}
    host = regional.area_mean(eta, a, regions=label)
    assert np.array_equal(_bits(np.asarray(mean.values)), _bits(host.values))
    _gate(host.values, regional.area_mean(eta, a, regions=label, return_area=True)[1].values, v, area,
          label, [2, 7, 1000], what="xarray")
    anom, m = regional.area_anomaly(x, xa, regions=xl, return_mean=True)
    assert isinstance(anom, fake_xarray.DataArray) and isinstance(m, fake_xarray.DataArray)
    assert anom.dims == ("time", "yh", "xh") and np.asarray(anom.values).dtype == F64
