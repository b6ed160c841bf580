"""GPU: tidegauge.locate / extract_tidegauge and the three entry points of include/momlevel_gauge.h
(csrc/momlevel_gauge.hip) against the reference's NWA12 goldens and the numpy restatement
tests/gauge_numpy.py.

Gates (none taken from what the kernels give):
  * the reference's 16 NWA12 sites: names and mod_index EQUAL, distance within the reference's own
    rtol 1e-4 of its CSV (tests/test_util.py:231; the CSV is rounded);
  * distance within 1e-10 relative of the restatement -- the project's standing gate for results
    that are not pointwise: the device's sin / cos / asin are not numpy's bit for bit;
  * indices EQUAL to the restatement's haversine argmin.  A gauge whose best and second-best
    restated distances lie closer than 1e-9 relative would be left out of the index comparison;
    every test asserts that NO gauge is left out;
  * two searches that differ only in the split of the points: indices and angles bit-identical;
  * the gather: bit-equal to numpy fancy indexing, NaN payloads included.
The reference's tests/test_tidegauge.py sums (ssh_max of NWA12_sample_grid_data.nc) are not pinned:
the file is netCDF-4 / HDF5 and could not be read where the fixtures were made.
Every compared figure is printed before it is asserted.
"""

import functools
import warnings

import numpy as np
import pytest
import torch

import gauge_numpy as gn
import momlevel_amd as m
from momlevel_amd import core, test_data, tidegauge, util
from momlevel_amd.labeled import DataArray, Dataset

pytestmark = pytest.mark.gpu

GAP = 1e-9      # below this relative gap between best and second best an index is not compared
PARITY = 1e-10  # distance against the restatement
SIZES = ((96, 160, 257, 1), (37, 53, 65, 2), (5, 5, 3, 3), (64, 129, 1, 4))


@functools.lru_cache(maxsize=None)
def _synthetic(ny, nx, ng, seed):
    """the grid, the gauges and the restated answer, computed once and shared (a test that changes
    an array works on a copy)"""
    lat, lon, mask, glat, glon = gn.synthetic_grid(ny, nx, ng, seed)
    index, angle, gap = gn.nearest(lat, lon, glat, glon, mask)
    return lat, lon, mask, glat, glon, index, angle, gap


@functools.lru_cache(maxsize=None)
def _nwa12_restated():
    grid, gold = gn.nwa12()
    got = gn.locate(grid["geolat"], grid["geolon"], gold["gauges"]["lat"], gold["gauges"]["lon"],
                    grid["mask"], threshold=gold["threshold"], rad_earth=gold["rad_earth"])
    return grid, gold, got


def _search(lat, lon, mask, glat, glon, split=0):
    points, valid = core.gauge_prepare(lat, lon, mask)
    gauges, _ = core.gauge_prepare(glat, glon)
    index, angle = core.gauge_nearest(points, gauges, split=split)
    return index, angle, valid


def _compare(index, angle, want_index, want_angle, gap, what):
    index, angle = index.cpu().numpy(), angle.cpu().numpy()
    excluded = np.nonzero(gap < GAP)[0]
    print(f"{what}: {len(index)} gauges, smallest relative gap {gap.min():.3e}, "
          f"excluded from the index comparison: {excluded.tolist()}")
    assert excluded.size == 0, what
    differ = np.nonzero(index != want_index)[0]
    print(f"{what}: indices that differ: {differ.tolist()}")
    assert differ.size == 0, what
    found = want_index >= 0
    assert np.array_equal(np.isnan(angle), ~found), what
    zero = found & (want_angle == 0.0)
    assert np.all(angle[zero] == 0.0), what
    rest = found & ~zero
    rel = np.max(np.abs(angle[rest] - want_angle[rest]) / want_angle[rest]) if rest.any() else 0.0
    print(f"{what}: max relative angle difference {rel:.3e} (gate {PARITY:.0e}), "
          f"largest angle {np.rad2deg(np.nanmax(want_angle)) if found.any() else 0.0:.2f} deg")
    assert rel <= PARITY, what
    return rel


# ---- the NWA12 fixture ----------------------------------------------------------------------------
def test_locate_reproduces_the_reference_on_nwa12():
    grid, gold, want = _nwa12_restated()
    loc = tidegauge.locate(grid["geolat"], grid["geolon"], gold["gauges"]["lat"],
                           gold["gauges"]["lon"], mask=grid["mask"], threshold=gold["threshold"])
    names = [gold["gauges"]["name"][i] for i in loc.which]
    print("kept:", names)
    assert names == gold["reference"]["name"]
    print("mod_index:", loc.mod_index.tolist())
    assert loc.mod_index.tolist() == gold["reference"]["mod_index"]
    ref = np.array(gold["reference"]["distance"])
    rel_csv = np.max(np.abs(loc.distance - ref) / ref)
    print(f"distance vs the reference CSV: max relative difference {rel_csv:.3e} (gate 1e-4)")
    assert rel_csv <= 1e-4
    rel = np.max(np.abs(loc.distance - want["distance"]) / want["distance"])
    print(f"distance vs the restatement: max relative difference {rel:.3e} (gate {PARITY:.0e})")
    assert rel <= PARITY
    assert np.array_equal(loc.flat_index, want["flat_index"])
    assert np.array_equal(loc.iy * 100 + loc.ix, loc.flat_index)
    assert np.array_equal(loc.model_coords[0], grid["geolat"].reshape(-1)[loc.flat_index])
    assert np.array_equal(loc.model_coords[1], grid["geolon"].reshape(-1)[loc.flat_index])
    # every gauge of the table, kept or not, against the restatement
    index, angle, gap = gn.nearest(grid["geolat"], grid["geolon"], gold["gauges"]["lat"],
                                   gold["gauges"]["lon"], grid["mask"])
    got_index, got_angle, valid = _search(grid["geolat"], grid["geolon"], grid["mask"],
                                          gold["gauges"]["lat"], gold["gauges"]["lon"])
    assert int(valid.sum()) == 8509
    _compare(got_index, got_angle, index, angle, gap, "NWA12, all 117 gauges")


def test_extract_tidegauge_on_nwa12_device_record():
    grid, gold, want = _nwa12_restated()
    rng = np.random.default_rng(11)
    host = rng.normal(0.0, 1.0, (3, 146, 100)).astype(np.float32)
    host[:, grid["mask"] == 0] = np.nan
    yh = DataArray(grid["yh"], ("yh",), None, None, "yh")
    xh = DataArray(grid["xh"], ("xh",), None, None, "xh")
    arr = DataArray(torch.from_numpy(host).cuda(), ("time", "yh", "xh"),
                    {"yh": yh, "xh": xh, "time": DataArray(np.arange(3.0), ("time",), None, None, "time")},
                    {"units": "m"}, "ssh")
    geolon = DataArray(grid["geolon"], ("yh", "xh"), None, None, "geolon")
    geolat = DataArray(grid["geolat"], ("yh", "xh"), None, None, "geolat")
    wet = DataArray(grid["mask"], ("yh", "xh"), None, None, "wet")
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # disable_warning=True: silent
        res = tidegauge.extract_tidegauge(arr, xcoord=geolon, ycoord=geolat, csv=gold["gauges"],
                                          mask=wet, threshold=gold["threshold"])
    assert isinstance(res, Dataset) and list(res.data_vars) == gold["reference"]["name"]
    for j, name in enumerate(gold["reference"]["name"]):
        var = res[name]
        iy, ix = divmod(int(want["flat_index"][j]), 100)
        assert var.is_device and var.dims == ("time",) and var.data.is_contiguous()
        assert np.array_equal(var.values.view(np.uint32), host[:, iy, ix].view(np.uint32))
        assert var.attrs["mod_index"] == gold["reference"]["mod_index"][j] and var.attrs["units"] == "m"
        assert abs(var.attrs["distance"] - want["distance"][j]) <= PARITY * want["distance"][j]
        assert var.attrs["dim_vals"] == (grid["yh"][iy], grid["xh"][ix])
        assert var.attrs["model_coords"] == (grid["geolat"][iy, ix], grid["geolon"][iy, ix])
        g = gold["gauges"]["name"].index(name)
        assert var.attrs["real_coords"] == (gold["gauges"]["lat"][g], gold["gauges"]["lon"][g])
        assert var.attrs["dims"] == ("yh", "xh") and var.attrs["name"] == name
        assert "lat" not in var.attrs and "lon" not in var.attrs
    # the reference's warning, one per gauge at or beyond the threshold
    with pytest.warns(UserWarning, match="Unable to map site name") as caught:
        tidegauge.extract_tidegauge(arr, xcoord=geolon, ycoord=geolat, csv=gold["gauges"],
                                    mask=wet, threshold=gold["threshold"], disable_warning=False)
    assert len([w for w in caught if "Unable to map" in str(w.message)]) == 117 - 16
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no threshold: nothing is dropped, nothing warned
        everything = tidegauge.extract_tidegauge(arr, xcoord=geolon, ycoord=geolat,
                                                 csv=gold["gauges"], mask=wet, disable_warning=False)
    # (one name occurs twice in the table: as in the reference's dict of results, the later row wins)
    assert len(set(gold["gauges"]["name"])) == 116 and len(everything) == 116


def test_geolocate_points_on_frames():
    pd = pytest.importorskip("pandas")
    grid, gold, want = _nwa12_restated()
    index = pd.MultiIndex.from_product([grid["yh"], grid["xh"]], names=["yh", "xh"])
    df_model = pd.DataFrame({"geolon": grid["geolon"].reshape(-1), "geolat": grid["geolat"].reshape(-1),
                             "mask": grid["mask"].reshape(-1).astype(np.float64)}, index=index)
    df_loc = pd.DataFrame(gold["gauges"])
    res = util.geolocate_points(df_model, df_loc, threshold=gold["threshold"])
    assert list(res["name"]) == gold["reference"]["name"]
    assert list(res["mod_index"]) == gold["reference"]["mod_index"]
    assert np.allclose(res["distance"], gold["reference"]["distance"], rtol=1e-4)
    assert "lat" not in res.columns and list(res.index) == want["which"].tolist()
    iy, ix = divmod(int(want["flat_index"][0]), 100)
    assert res["dim_vals"].iloc[0] == (grid["yh"][iy], grid["xh"][ix])
    assert res["model_coords"].iloc[0] == (grid["geolat"][iy, ix], grid["geolon"][iy, ix])
    assert len(util.geolocate_points(df_model, df_loc)) == 117


# ---- the index contract on synthetic grids -------------------------------------------------------
@pytest.mark.parametrize("ny,nx,ng,seed", SIZES)
def test_indices_equal_the_restatement(ny, nx, ng, seed):
    lat, lon, mask, glat, glon, want_index, want_angle, gap = _synthetic(ny, nx, ng, seed)
    n = ny * nx
    lib_split = core._lib.load_gauge().mlx_gauge_nearest_split(n, ng, 0)
    print(f"{ny}x{nx}: {n} points, {ng} gauges, land {1 - mask.mean():.2f}, default split {lib_split}")
    if (ny, nx) == (96, 160):
        assert lib_split > 1  # the second stage combines several partials
    index, angle, valid = _search(lat, lon, mask, glat, glon)
    assert np.array_equal(valid.cpu().numpy().astype(bool), gn.valid_points(lat, lon, mask))
    _compare(index, angle, want_index, want_angle, gap, f"{ny}x{nx}")
    # float32 coordinates are widened exactly: the float64 search of the rounded positions
    lat32, lon32 = lat.astype(np.float32), lon.astype(np.float32)
    i32, a32, _ = _search(lat32, lon32, mask.astype(np.float32), glat, glon)
    i64, a64, _ = _search(lat32.astype(np.float64), lon32.astype(np.float64), mask, glat, glon)
    assert torch.equal(i32, i64) and torch.equal(a32.view(torch.int64), a64.view(torch.int64))


@pytest.mark.parametrize("ny,nx,ng,seed", SIZES[:2])
def test_the_split_of_the_points_changes_nothing(ny, nx, ng, seed):
    lat, lon, mask, glat, glon, want_index, _a, _g = _synthetic(ny, nx, ng, seed)
    points, _ = core.gauge_prepare(lat, lon, mask)
    gauges, _ = core.gauge_prepare(glat, glon)
    runs = {s: core.gauge_nearest(points, gauges, split=s) for s in (0, 1, 3, 64, ny * nx)}
    again = core.gauge_nearest(points, gauges, split=3)
    base_i, base_a = runs[1]
    assert np.array_equal(base_i.cpu().numpy(), want_index)
    for s, (i, a) in list(runs.items()) + [("3 again", again)]:
        same_i = torch.equal(i, base_i)
        same_a = torch.equal(a.view(torch.int64), base_a.view(torch.int64))
        print(f"{ny}x{nx} split {s}: indices identical {same_i}, angle bits identical {same_a}")
        assert same_i and same_a


# ---- ties, edges, masks --------------------------------------------------------------------------
def test_ties_go_to_the_lowest_flat_index():
    row_lat = np.linspace(-60.0, 60.0, 300)
    row_lon = np.linspace(-170.0, 170.0, 300)
    lat = np.tile(row_lat, (4, 1))  # every point exists four times: flat indices j, 300 + j, ...
    lon = np.tile(row_lon, (4, 1))
    glat, glon = row_lat[[7, 150, 299]] + 0.01, row_lon[[7, 150, 299]] - 0.01
    for split in (0, 1, 4, 7):  # 4: the duplicates lie in different parts, the second stage decides
        index, angle, _ = _search(lat, lon, None, glat, glon, split=split)
        print(f"split {split}: duplicates x4, winners {index.tolist()}")
        assert index.tolist() == [7, 150, 299]
    mask = np.ones((4, 300))
    mask[0, 150] = 0.0  # the first copy is land: the next one wins
    index, _, _ = _search(lat, lon, mask, glat, glon)
    assert index.tolist() == [7, 450, 299]
    # a gauge exactly on a grid point: distance 0.0
    index, angle, _ = _search(lat, lon, None, row_lat[[3, 200]], row_lon[[3, 200]])
    print("gauges on grid points:", index.tolist(), angle.tolist())
    assert index.tolist() == [3, 200] and angle.tolist() == [0.0, 0.0]


def test_gauges_at_the_poles():
    lat, lon, mask, _glat, _glon, _i, _a, _g = _synthetic(37, 53, 65, 2)
    glat, glon = np.array([90.0, -90.0, 90.0]), np.array([0.0, 123.0, -180.0])
    want_index, want_angle, gap = gn.nearest(lat, lon, glat, glon, mask)
    index, angle, _ = _search(lat, lon, mask, glat, glon)
    _compare(index, angle, want_index, want_angle, gap, "poles")
    assert index[0] == index[2]  # the longitude of a pole is immaterial


def test_masks_and_bad_coordinates():
    lat, lon, mask, glat, glon, _i, _a, _g = _synthetic(37, 53, 65, 2)
    lat, lon, mask = lat.copy(), lon.copy(), mask.copy()
    base, _, _ = _search(lat, lon, mask, glat, glon)
    winners = np.unique(base.cpu().numpy())
    # NaN in the mask means dry, 0.5 means dry, 2.0 means dry: only == 1.0 is wet
    odd = mask.copy().reshape(-1)
    odd[winners[0::3]], odd[winners[1::3]], odd[winners[2::3]] = np.nan, 0.5, 2.0
    odd = odd.reshape(mask.shape)
    want_index, want_angle, gap = gn.nearest(lat, lon, glat, glon, odd)
    index, angle, valid = _search(lat, lon, odd, glat, glon)
    assert not np.isin(index.cpu().numpy(), winners).any()
    assert int(valid.sum()) == int(mask.sum()) - len(winners)
    _compare(index, angle, want_index, want_angle, gap, "NaN / 0.5 / 2.0 in the mask")
    # NaN and infinite coordinates on land never win; on wet points they make the point invalid
    land = np.nonzero(mask.reshape(-1) == 0.0)[0]
    bad_lat, bad_lon = lat.copy().reshape(-1), lon.copy().reshape(-1)
    bad_lat[land[0::2]], bad_lon[land[1::2]] = np.nan, np.inf
    bad_lat[winners[0]] = np.nan
    bad_lat, bad_lon = bad_lat.reshape(lat.shape), bad_lon.reshape(lon.shape)
    want_index, want_angle, gap = gn.nearest(bad_lat, bad_lon, glat, glon, mask)
    index, angle, valid = _search(bad_lat, bad_lon, mask, glat, glon)
    assert int(valid.sum()) == int(mask.sum()) - 1 and not (index == int(winners[0])).any()
    _compare(index, angle, want_index, want_angle, gap, "NaN / inf coordinates")
    # a gauge without a position finds nothing
    index, angle, _ = _search(lat, lon, mask, [np.nan, 10.0], [5.0, np.inf])
    assert index.tolist() == [-1, -1] and bool(torch.isnan(angle).all())


def test_an_all_dry_mask_gives_an_empty_result():
    lat, lon, mask, glat, glon, _i, _a, _g = _synthetic(37, 53, 65, 2)
    index, angle, valid = _search(lat, lon, np.zeros_like(mask), glat, glon)
    torch.cuda.synchronize()
    assert int(valid.sum()) == 0 and bool((index == -1).all()) and bool(torch.isnan(angle).all())
    loc = tidegauge.locate(lat, lon, glat, glon, mask=np.zeros_like(mask), threshold=100.0)
    assert len(loc) == 0 and loc.flat_index.size == 0 and loc.all_index.tolist() == [-1] * 65
    arr = DataArray(torch.zeros((2, 37, 53), device="cuda"), ("time", "yh", "xh"))
    res = tidegauge.extract_tidegauge(
        arr, DataArray(lon, ("yh", "xh")), DataArray(lat, ("yh", "xh")),
        csv={"name": [f"g{i}" for i in range(65)], "lat": glat, "lon": glon},
        mask=DataArray(np.zeros_like(mask), ("yh", "xh")))
    assert len(res) == 0


def test_threshold_keeps_less_or_equal():
    lat, lon, mask, glat, glon, _i, _a, _g = _synthetic(37, 53, 65, 2)
    every = tidegauge.locate(lat, lon, glat, glon, mask=mask)
    assert len(every) == 65 and every.which.tolist() == list(range(65))
    cut = float(np.sort(every.distance)[20])  # the distance of one gauge, exactly
    some = tidegauge.locate(lat, lon, glat, glon, mask=mask, threshold=cut)
    print(f"threshold {cut!r}: kept {len(some)} of 65")
    assert len(some) == 21 and cut in some.distance.tolist()  # <= keeps the gauge at the threshold
    assert np.array_equal(some.which, np.nonzero(every.distance <= cut)[0])
    assert np.array_equal(some.distance, every.distance[some.which])
    half = tidegauge.locate(lat, lon, glat, glon, mask=mask, rad_earth=3.189e3)
    assert np.array_equal(half.distance * 2.0, every.distance)  # (6378 = 2 * 3189, exactly)


# ---- the gather ----------------------------------------------------------------------------------
def _record(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    y = rng.normal(0.0, 1.0, shape).astype(dtype)
    flat = y.reshape(-1)
    flat[rng.random(flat.size) < 0.1] = np.nan
    bits = flat.view(np.uint64 if dtype == np.float64 else np.uint32)
    bits[::17] = 0x7FF8000000000ABC if dtype == np.float64 else 0x7FC00ABC  # NaNs with a payload
    return y


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
@pytest.mark.parametrize("lead", ((7,), (2, 7)))
def test_gather_is_bit_equal_to_fancy_indexing(lead, dtype):
    lat, lon, mask, glat, glon, want_index, _a, _g = _synthetic(37, 53, 65, 2)
    host = _record(lead + (37, 53), dtype, seed=len(lead))
    dims = ("member", "time", "yh", "xh")[-len(lead) - 2:]
    geolon, geolat = DataArray(lon, ("yh", "xh")), DataArray(lat, ("yh", "xh"))
    table = {"name": [f"site_{i}" for i in range(65)], "lat": glat, "lon": glon}
    iy, ix = np.unravel_index(want_index, (37, 53))

    def check(res, device):
        assert list(res.data_vars) == table["name"]
        for g in (0, 1, 31, 64):
            var = res[f"site_{g}"]
            assert var.dims == dims[:-2] and var.is_device == device
            assert var.values.dtype == dtype and var.shape == lead
            want = host[..., iy[g], ix[g]]
            assert np.array_equal(_bits(var.values), _bits(want)), (g, device)

    on_device = DataArray(torch.from_numpy(host).cuda(), dims)
    res = tidegauge.extract_tidegauge(on_device, geolon, geolat, csv=table, mask=DataArray(mask, ("yh", "xh")))
    check(res, True)
    first, last = res["site_0"].data, res["site_64"].data
    assert first.is_contiguous() and last.is_contiguous()
    nrest = int(np.prod(lead))  # rows of ONE gather result: site g starts g * nrest elements in
    assert last.data_ptr() - first.data_ptr() == 64 * nrest * host.dtype.itemsize
    # host input gives a host result
    check(tidegauge.extract_tidegauge(DataArray(host, dims), geolon, geolat, csv=table,
                                      mask=DataArray(mask, ("yh", "xh"))), False)
    # a transposed, non-contiguous record (device and host): laid out by record.layout
    order = ("xh",) + dims[:-2] + ("yh",)
    perm = [dims.index(d) for d in order]
    turned = DataArray(torch.from_numpy(host).cuda().permute(*perm), order)
    assert not turned.data.is_contiguous()
    check(tidegauge.extract_tidegauge(turned, geolon, geolat, csv=table,
                                      mask=DataArray(mask, ("yh", "xh"))), True)
    check(tidegauge.extract_tidegauge(DataArray(host.transpose(perm), order), geolon, geolat,
                                      csv=table, mask=DataArray(mask, ("yh", "xh"))), False)


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32))
def test_gather_out_of_range_index_gives_a_nan_row(dtype):
    y = torch.arange(7 * 300, dtype=dtype, device="cuda").reshape(7, 300)
    out = core.gauge_gather(y, [0, 299, 300, -1, 17, 1 << 40])
    got = out.cpu().numpy()
    print(got[:, :3])
    assert out.shape == (6, 7) and out.dtype == dtype
    host = y.cpu().numpy()
    for row, i in ((0, 0), (1, 299), (4, 17)):
        assert np.array_equal(got[row], host[:, i])
    assert np.isnan(got[[2, 3, 5]]).all()
    assert torch.equal(core.gauge_gather(y, torch.tensor([5, 6], device="cuda")), y[:, 5:7].T)
    with pytest.raises(TypeError):
        core.gauge_gather(y, [0.5])
    with pytest.raises(ValueError):
        core.gauge_gather(y.reshape(7, 3, 100), [0])
    with pytest.raises(TypeError):
        core.gauge_gather(y.to(torch.float16), [0])
    with pytest.raises(ValueError):
        core.gauge_nearest(torch.zeros((3, 4), dtype=torch.float64, device="cuda"),
                           torch.zeros((5, 4), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        core.gauge_prepare(np.zeros(4), np.zeros(5))


# ---- end to end ----------------------------------------------------------------------------------
def test_steric_local_to_tide_gauges():
    dset = test_data.generate_test_data()
    result, _ = m.steric(dset, domain="local")
    eta = result["steric"]
    assert eta.dims == ("time", "yh", "xh")
    eta.coords["geolon"], eta.coords["geolat"] = dset.geolon, dset.geolat
    eta.coords.setdefault("yh", dset.yh)
    eta.coords.setdefault("xh", dset.xh)
    table = {"PSMSL_site": ["EQUATOR", "SOUTH", "NORTH_EAST"], "PSMSLID": [1, 2, 3],
             "lat": [1.0, -70.0, 40.0], "lon": [185.0, 30.0, -30.0]}
    res = tidegauge.extract_tidegauge(eta, csv=table)
    assert list(res.data_vars) == ["EQUATOR", "SOUTH", "NORTH_EAST"]
    values = eta.values
    for name, (iy, ix) in (("EQUATOR", (2, 2)), ("SOUTH", (0, 0)), ("NORTH_EAST", (3, 4))):
        var = res[name]
        print(name, var.attrs["distance"], var.attrs["dim_vals"], var.attrs["model_coords"])
        assert var.dims == ("time",) and var.name == name
        assert np.array_equal(np.asarray(var.values), values[:, iy, ix], equal_nan=True)
        assert var.attrs["dim_vals"] == (dset.yh.values[iy], dset.xh.values[ix])
        assert var.attrs["model_coords"] == (dset.geolat.values[iy, ix], dset.geolon.values[iy, ix])
        assert var.attrs["dims"] == ("yh", "xh") and var.attrs["name"] == name
        assert var.attrs["PSMSLID"] == table["PSMSLID"][table["PSMSL_site"].index(name)]
        for key, val in eta.attrs.items():
            assert var.attrs[key] == val
        want = gn.haversine(*np.deg2rad([var.attrs["real_coords"][0], var.attrs["real_coords"][1],
                                         var.attrs["model_coords"][0], var.attrs["model_coords"][1]]))
        assert abs(var.attrs["distance"] - want * 6.378e3) <= PARITY * want * 6.378e3
    assert res["SOUTH"].attrs["mod_index"] == 0 and res["EQUATOR"].attrs["mod_index"] == 12
    # 1-D xh / yh coordinates are tiled, with the reference's warning
    with pytest.warns(UserWarning, match="Constructing coordinates from 1-D vectors"):
        flat = tidegauge.extract_tidegauge(eta, xcoord="xh", ycoord="yh",
                                           csv={"name": ["A"], "lat": [4.2], "lon": [1.9]})
    assert np.array_equal(np.asarray(flat["A"].values), values[:, 3, 1], equal_nan=True)
    assert flat["A"].attrs["dim_vals"] == (4.0, 2.0) and flat["A"].attrs["model_coords"] == (4.0, 2.0)
