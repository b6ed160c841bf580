"""GPU: core.regrid_apply (csrc/momlevel_regrid.hip) and momlevel_amd.regrid against the numpy
restatement tests/regrid_numpy.py, BIT FOR BIT (integer views: the NaNs are canonical too) -- the
only yardstick: the function is an extension, the reference has no counterpart.

Shapes come from the kernel's geometry queries: one slice plus one destination, so that a second,
partial slice exists, and one record window plus one record; rows of 0, 1, 3 and 40 entries share
the first slice, so that its padding is walked.  The expected values are computed once per table
(``_want``) and shared."""

import functools

import numpy as np
import pytest
import torch

import regrid_numpy as rn
from momlevel_amd import core, regrid
from momlevel_amd.labeled import DataArray, Dataset

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
TORCH = {F64: torch.float64, F32: torch.float32}
NSRC = 301


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared cases are read-only)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == F64 else np.int32)


def assert_same_bits(got, want, what):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} cells differ, first at " \
                          f"{tuple(int(i) for i in np.argwhere(bad)[0])}"


@functools.lru_cache(maxsize=None)
def make_table(ndst, nsrc=NSRC, seed=0):
    """rows (indptr, col, S): lengths 0, 1, 3 and 40 first, then 0 .. 8; row 5 reads sources 7, 8
    and 9 only (make_record keeps them NaN); positive weights"""
    rng = np.random.default_rng(seed)
    length = rng.integers(0, 9, ndst)
    length[:4] = (0, 1, 3, 40)
    cols = [np.sort(rng.choice(nsrc, n, replace=False)) for n in length]
    if ndst > 5:
        cols[5], length[5] = np.array([7, 8, 9]), 3
    indptr = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    col = np.concatenate(cols).astype(np.int32)
    S = rng.uniform(0.25, 4.0, col.size)
    for a in (indptr, col, S):
        a.setflags(write=False)
    return indptr, col, S


@functools.lru_cache(maxsize=None)
def make_record(nrec, vdt=F64, nsrc=NSRC, seed=1):
    """isolated NaNs that differ between records; sources 7..9 NaN in every record"""
    rng = np.random.default_rng(seed)
    v = rng.normal(0.2, 1.0, (nrec, nsrc))
    v[rng.random(v.shape) < 0.08] = np.nan
    v[:, 7:10] = np.nan
    v = v.astype(vdt)
    v.setflags(write=False)
    return v


def _shape():
    return core.regrid_slice() + 1, core.regrid_record_window() + 1


def run(v, table, ndst, min_frac=0.0, propagate=False, renorm=True, out_dtype=None):
    packed = regrid.pack_rows(*table, core.regrid_slice())
    out = core.regrid_apply(v if isinstance(v, torch.Tensor) else _dev(v),
                            tuple(_dev(a) for a in packed), v.shape[1], ndst, min_frac,
                            propagate=propagate, renorm=renorm,
                            out_dtype=None if out_dtype is None else TORCH[out_dtype])
    torch.cuda.synchronize()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _want(ndst, nrec, vdt, odt, min_frac=0.0, flags=0):
    out = rn.apply_csr(make_record(nrec, vdt), *make_table(ndst), ndst, min_frac, flags, odt)
    out.setflags(write=False)
    return out


def test_the_geometry_gives_the_tests_their_shapes():
    ndst, nrec = _shape()
    assert ndst == 65 and nrec >= 2
    indptr, col, S = make_table(ndst)
    assert np.diff(indptr)[:4].tolist() == [0, 1, 3, 40] and np.diff(indptr).max() == 40
    v = make_record(nrec)
    assert np.isnan(v).any() and not np.isnan(v).all(axis=1).any()
    assert (np.isnan(v).sum(axis=1) > 3).all() and len({tuple(np.isnan(r)) for r in v}) == nrec


@pytest.mark.parametrize("odt", (F64, F32), ids=("o64", "o32"))
@pytest.mark.parametrize("vdt", (F64, F32), ids=("v64", "v32"))
def test_the_base_case_in_every_dtype(vdt, odt):
    ndst, nrec = _shape()
    got = run(make_record(nrec, vdt), make_table(ndst), ndst, out_dtype=odt)
    want = _want(ndst, nrec, vdt, odt)
    assert got.dtype == want.dtype == odt
    assert_same_bits(got, want, f"{vdt.__name__} -> {odt.__name__}")
    # row 0 has no entry and row 5 none that is valid: NaN in every record; the rest mostly not
    assert np.isnan(got[:, 0]).all() and np.isnan(got[:, 5]).all()
    assert np.isnan(got).sum() < got.size // 4
    default = run(make_record(nrec, vdt), make_table(ndst), ndst)
    assert default.dtype == vdt  # (the record's dtype when none is asked for)


@pytest.mark.parametrize("vdt", (F64, F32), ids=("v64", "v32"))
@pytest.mark.parametrize("min_frac", (0.0, 0.5, 1.0))
def test_min_frac(min_frac, vdt):
    ndst, nrec = _shape()
    got = run(make_record(nrec, vdt), make_table(ndst), ndst, min_frac=min_frac)
    assert_same_bits(got, _want(ndst, nrec, vdt, vdt, min_frac), f"min_frac={min_frac}")
    if min_frac == 1.0:  # only destinations whose every source is present survive
        v, (indptr, col, S) = make_record(nrec, vdt), make_table(ndst)
        whole = np.array([[not np.isnan(r[col[indptr[d]:indptr[d + 1]]]).any() and indptr[d + 1] > indptr[d]
                           for d in range(ndst)] for r in v])
        assert np.array_equal(~np.isnan(got), whole) and whole.any() and not whole.all()


@pytest.mark.parametrize("vdt", (F64, F32), ids=("v64", "v32"))
@pytest.mark.parametrize("mode", ("propagate", "no_renorm", "both"))
def test_the_modes(mode, vdt):
    ndst, nrec = _shape()
    flags = {"propagate": rn.PROPAGATE, "no_renorm": rn.NO_RENORM, "both": 3}[mode]
    got = run(make_record(nrec, vdt), make_table(ndst), ndst, min_frac=0.25,
              propagate=bool(flags & rn.PROPAGATE), renorm=not flags & rn.NO_RENORM)
    assert_same_bits(got, _want(ndst, nrec, vdt, vdt, 0.25, flags), mode)
    if mode == "both":  # PROPAGATE wins
        assert_same_bits(got, _want(ndst, nrec, vdt, vdt, 0.25, rn.PROPAGATE), "both == propagate")


@pytest.mark.parametrize("vdt", (F64, F32), ids=("v64", "v32"))
def test_a_record_of_ones_gives_exactly_one(vdt):
    ndst, nrec = _shape()
    ones = np.where(np.isnan(make_record(nrec, vdt)), np.nan, 1.0).astype(vdt)
    got = run(ones, make_table(ndst), ndst)
    assert set(np.unique(got[~np.isnan(got)])) == {1.0}
    assert np.array_equal(np.isnan(got), np.isnan(_want(ndst, nrec, vdt, vdt)))


def test_a_rows_bits_do_not_depend_on_the_table_around_it():
    """the rows of the base table at other places of a table of two slices and a half, between
    rows of other lengths"""
    ndst, nrec = _shape()
    indptr, col, S = make_table(ndst)
    rng = np.random.default_rng(11)
    big = 2 * core.regrid_slice() + 35
    place = rng.permutation(big)[:ndst]  # row d of the base table is row place[d] of the big one
    other = make_table(big, seed=5)
    rows = [(other[1][other[0][j]:other[0][j + 1]], other[2][other[0][j]:other[0][j + 1]])
            for j in range(big)]
    for d, j in enumerate(place):
        rows[j] = (col[indptr[d]:indptr[d + 1]], S[indptr[d]:indptr[d + 1]])
    table = (np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64),
             np.concatenate([c for c, _ in rows]).astype(np.int32), np.concatenate([w for _, w in rows]))
    got = run(make_record(nrec), table, big)
    assert_same_bits(got[:, place], _want(ndst, nrec, F64, F64), "rows moved to another table")
    # the same with one destination only: a table of one row
    for d in (2, 3):
        one = (np.array([0, indptr[d + 1] - indptr[d]]), col[indptr[d]:indptr[d + 1]],
               S[indptr[d]:indptr[d + 1]])
        assert_same_bits(run(make_record(nrec), one, 1)[:, 0], _want(ndst, nrec, F64, F64)[:, d],
                         f"row {d} alone")


@pytest.mark.parametrize("vdt", (F64, F32), ids=("v64", "v32"))
def test_a_records_bits_do_not_depend_on_the_records_around_it(vdt):
    ndst, _ = _shape()
    nrec = core.regrid_record_window() + 5
    v = _dev(make_record(nrec, vdt, seed=4))
    whole = run(v, make_table(ndst), ndst)
    part = run(v[5:9], make_table(ndst), ndst)  # (a view: it starts 5 * 301 elements into v)
    assert v[5:9].is_contiguous() and v[5:9].data_ptr() != v.data_ptr()
    assert_same_bits(part, whole[5:9], "records 5..8 of a longer record")
    assert_same_bits(whole, rn.apply_csr(make_record(nrec, vdt, seed=4), *make_table(ndst), ndst),
                     "the longer record")
    single = run(v[8:9], make_table(ndst), ndst)
    assert_same_bits(single, whole[8:9], "one record")


def test_two_runs_are_identical():
    ndst, nrec = _shape()
    first = run(make_record(nrec), make_table(ndst), ndst)
    second = run(make_record(nrec), make_table(ndst), ndst)
    assert_same_bits(first, second, "a second run")


# ---- the three builders through regrid.apply ------------------------------------------------------
def _through(plan, v, min_frac=0.0, flags=0):
    flat = np.asarray(v).reshape(-1, plan.nsrc)
    out = rn.apply_csr(flat, plan.indptr, plan.col, plan.S, plan.ndst, min_frac, flags)
    return out.reshape(v.shape[:-2] + plan.dst_shape)


@pytest.mark.parametrize("vdt", (F64, F32), ids=("v64", "v32"))
def test_coarsening_a_record_with_land(vdt):
    rng = np.random.default_rng(21)
    area = rng.uniform(4.0e8, 9.0e8, (16, 72))
    area[4:8, 8:16] = 0.0       # two whole blocks of land
    area[9, 30:50] = np.nan
    v = rng.normal(0.0, 1.0, (3, 16, 72))
    v[:, area == 0.0] = np.nan
    v[1, 12:, :7] = np.nan
    v = v.astype(vdt)
    plan = regrid.coarsen_weights(area, 4, 4)
    assert plan.dst_shape == (4, 18)
    want = _through(plan, v)
    got = regrid.apply(v, plan)
    assert isinstance(got, np.ndarray) and got.dtype == vdt and got.shape == (3, 4, 18)
    assert want.dtype == vdt
    assert_same_bits(got, want, "coarsen_weights 4 x 4")
    assert np.isnan(got[:, 1, 2:4]).all() and np.isnan(got[1, 3, 0]) and not np.isnan(got[0, 3, 0])
    dev = regrid.coarsen(_dev(v), area, 4, 4, min_frac=0.5)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == TORCH[vdt]
    want_half = rn.apply_csr(v.reshape(3, -1), plan.indptr, plan.col, plan.S, plan.ndst, 0.5, 0, vdt)
    assert_same_bits(dev, want_half.reshape(3, 4, 18), "coarsen, min_frac = 0.5, on the device")
    assert np.isnan(want_half).sum() > np.isnan(want).sum()
    strict = regrid.apply(v, plan, skipna=False)
    assert_same_bits(strict, rn.apply_csr(v.reshape(3, -1), plan.indptr, plan.col, plan.S, plan.ndst,
                                          0.0, rn.PROPAGATE, vdt).reshape(3, 4, 18), "skipna=False")
    plain = regrid.apply(v, plan, renorm=False)
    assert_same_bits(plain, rn.apply_csr(v.reshape(3, -1), plan.indptr, plan.col, plan.S, plan.ndst,
                                         0.0, rn.NO_RENORM, vdt).reshape(3, 4, 18), "renorm=False")


def test_conservative_remapping_from_two_to_five_degrees():
    src = (np.linspace(-40, 40, 41), np.linspace(0, 360, 181))
    dst = (np.linspace(-40, 40, 17), np.linspace(-180, 180, 73))
    rng = np.random.default_rng(22)
    mask = (rng.random((40, 180)) > 0.2).astype(F64)
    mask[10:21, 30:61] = 0.0  # a continent: destinations without a source, and with less than half
    plan = regrid.conservative_weights(*src, *dst, src_mask=mask)
    v = np.where(mask == 1.0, rng.normal(0.0, 1.0, (2, 40, 180)), np.nan)
    got = regrid.apply(v, plan, min_frac=0.5)
    assert got.shape == (2, 16, 72)
    assert_same_bits(got, _through(plan, v, 0.5), "conservative_weights 2 -> 5 degrees")
    assert 0 < np.isnan(got).sum() < got.size // 2
    # a constant field stays the constant, to the last rounding of the quotient
    c = regrid.apply(np.where(mask == 1.0, 1.0, np.nan)[None], plan)
    assert set(np.unique(c[~np.isnan(c)])) == {1.0}


def test_nearest_weights_of_seven_points():
    lat, lon = np.linspace(-30.0, 30.0, 13), np.linspace(0.0, 55.0, 12)
    rng = np.random.default_rng(23)
    mask = (rng.random((13, 12)) > 0.3).astype(F64)
    plat = np.array([[-29.0, -11.3, 0.2, 7.7, 18.1, 29.9, 80.0]])
    plon = np.array([[1.0, 50.2, 27.3, 13.9, 44.4, 3.3, 200.0]])
    plan = regrid.nearest_weights(lat, lon, plat, plon, mask=mask, threshold=1500.0)
    assert plan.src_shape == (13, 12) and plan.dst_shape == (1, 7)
    assert np.diff(plan.indptr).tolist() == [1, 1, 1, 1, 1, 1, 0]  # the last point is too far
    assert (plan.S == 1.0).all()
    # the nearest wet point by the haversine formula, in numpy
    g_lat, g_lon = np.meshgrid(np.deg2rad(lat), np.deg2rad(lon), indexing="ij")
    for p in range(6):
        a, b = np.deg2rad(plat[0, p]), np.deg2rad(plon[0, p])
        h = np.sin((g_lat - a) / 2) ** 2 + np.cos(a) * np.cos(g_lat) * np.sin((g_lon - b) / 2) ** 2
        h = np.where(mask == 1.0, h, np.inf).reshape(-1)
        assert plan.col[p] == np.argmin(h) and np.sort(h)[1] > h.min() * (1 + 1e-9), p
    v = rng.normal(0.0, 1.0, (2, 13, 12))
    got = regrid.apply(v, plan)
    assert got.shape == (2, 1, 7) and np.isnan(got[:, 0, 6]).all()
    assert_same_bits(got[:, 0, :6], v.reshape(2, -1)[:, plan.col], "nearest: the source's own bits")
    assert_same_bits(got, _through(plan, v), "nearest_weights")
    everywhere = regrid.nearest_weights(lat, lon, plat, plon, mask=mask)
    assert np.diff(everywhere.indptr).tolist() == [1] * 7


def test_a_large_host_record_goes_in_groups_of_leading_rows(monkeypatch):
    from momlevel_amd import hostio

    rng = np.random.default_rng(25)
    v = rng.normal(0.0, 1.0, (5, 8, 12)).astype(F32)
    v[rng.random(v.shape) < 0.1] = np.nan
    plan = regrid.coarsen_weights(rng.uniform(1.0, 2.0, (8, 12)), 2, 3)
    whole = regrid.apply(v, plan)
    monkeypatch.setattr(hostio, "PIPELINE_ELEMS", 100)
    monkeypatch.setattr(hostio, "PIECE_ELEMS", 2 * 8 * 12)  # two records a group
    grouped = regrid.apply(DataArray(v, ("time", "yh", "xh")), plan)
    assert grouped.dims == ("time", "yh", "xh") and grouped.dtype == F32 and grouped.shape == (5, 4, 4)
    assert_same_bits(grouped.values, whole, "groups of two leading rows")
    assert_same_bits(whole, _through(plan, v), "the restatement")


def test_labeled_dims_and_coords_of_the_result():
    rng = np.random.default_rng(24)
    v = rng.normal(0.0, 1.0, (3, 8, 12))
    time = DataArray(np.arange(3.0), ("time",), None, {"axis": "T"}, "time")
    yh = DataArray(np.linspace(-35.0, 35.0, 8), ("yh",), None, {"units": "degrees_north"}, "yh")
    geolon = DataArray(rng.random((8, 12)), ("yh", "xh"), None, None, "geolon")
    eta = DataArray(v, ("time", "yh", "xh"), {"time": time, "yh": yh, "geolon": geolon},
                    {"units": "m", "long_name": "sea level"}, "zos")
    plan = regrid.conservative_weights(np.linspace(-40, 40, 9), np.linspace(0, 360, 13),
                                       np.linspace(-40, 40, 5), np.linspace(0, 360, 7))
    want = _through(plan, v)
    out = regrid.apply(eta, plan)
    assert isinstance(out, DataArray) and out.dims == ("time", "lat", "lon") and out.name == "zos"
    assert out.shape == (3, 4, 6) and out.attrs == eta.attrs and not out.is_device
    assert set(out.coords) == {"time", "lat", "lon"}  # the plane's own coords are gone
    assert out.coords["lat"].values.tolist() == [-30.0, -10.0, 10.0, 30.0]
    assert out.coords["lon"].values.tolist() == [30.0, 90.0, 150.0, 210.0, 270.0, 330.0]
    assert_same_bits(out.values, want, "DataArray in")
    resident = regrid.apply(DataArray(_dev(v), eta.dims, eta.coords, eta.attrs, "zos"), plan)
    assert resident.is_device and resident.dims == out.dims
    assert_same_bits(resident.data, want, "a resident DataArray")
    four = regrid.apply(np.stack([v, v[::-1]]), plan)  # every leading index is a record of its own
    assert four.shape == (2, 3, 4, 6)
    assert_same_bits(four[1], want[::-1], "leading dims are records")
    plane = regrid.apply(v[0], plan)  # a bare plane is one record
    assert_same_bits(plane, want[0], "a 2-D record")
    ds = Dataset({"zos": eta, "steps": DataArray(np.arange(3.0), ("time",)),
                  "row": DataArray(np.arange(8.0), ("yh",))})
    got = regrid.apply(ds, plan)
    assert isinstance(got, Dataset) and set(got.data_vars) == {"zos", "steps"}
    assert got["zos"].dims == ("time", "lat", "lon")
    assert_same_bits(got["zos"].values, want, "Dataset: zos")
    assert np.array_equal(got["steps"].values, np.arange(3.0))
    coarse = regrid.coarsen(eta, DataArray(np.ones((8, 12)), ("yh", "xh")), 2, 3)
    assert coarse.dims == ("time", "yh", "xh") and coarse.shape == (3, 4, 4)
    assert set(coarse.coords) == {"time"}
