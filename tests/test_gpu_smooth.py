"""GPU: core.plane_smooth (csrc/momlevel_smooth.hip) against the numpy restatement
tests/smooth_numpy.py, BIT FOR BIT (integer views: the NaNs are canonical too) -- the only
yardstick: the function is an extension, the reference has no counterpart.

Shapes come from the kernel's geometry queries: one tile plus one row by one tile plus one pack, so
that a second tile exists each way and a window straddles both boundaries (taller where the window
is: Wy <= ny).  Dtypes, windows, the periodic seam and the closed edges, a per-row weight table,
land and invalid cells, every flag, the record window, a record of ones."""

import numpy as np
import pytest
import torch

import smooth_numpy as sn
from momlevel_amd import core

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
TORCH = {F64: torch.float64, F32: torch.float32}


def _geometry():
    th, tw = core.smooth_tile(F64)
    return th, tw, core.smooth_max_window(), core.smooth_record_window()


def _plane(Wy=1, dtype=F64):
    th, tw = core.smooth_tile(dtype)
    return max(th + 1, Wy), tw + 4  # (one pack of float32 is 4 cells: a whole pack for either dtype)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == F64 else np.int32)


def assert_same_bits(got, want, what):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} cells differ, first at " \
                          f"{tuple(int(i) for i in np.argwhere(bad)[0])}"


def make_case(nrec, ny, nx, vdt=F64, adt=F64, seed=0, land=True):
    """a record with isolated NaNs that differ between records, one block of land wider than a
    9 x 9 window (half of it NaN in v, half without area), and zero and NaN areas of its own"""
    rng = np.random.default_rng(seed)
    v = rng.normal(0.2, 1.0, (nrec, ny, nx))
    v[rng.random(v.shape) < 0.03] = np.nan
    area = rng.uniform(4.0e8, 9.0e8, (ny, nx))
    area[rng.random((ny, nx)) < 0.02] = 0.0
    area[rng.random((ny, nx)) < 0.02] = np.nan
    if land:
        v[:, 2:14, 20:36] = np.nan
        area[2:14, 36:52] = 0.0
    return v.astype(vdt), area.astype(adt)


def run(v, area, wx, wy, lx, ly, periodic=True, mc=1, fill=False, residual=False, out_dtype=None):
    out = core.plane_smooth(_dev(v), _dev(area), wx, wy, lx, ly, periodic, mc, fill=fill,
                            residual=residual, out_dtype=None if out_dtype is None else TORCH[out_dtype])
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check(v, area, wx, wy, lx, ly, periodic=True, mc=1, fill=False, residual=False, out_dtype=None,
          what=""):
    got = run(v, area, wx, wy, lx, ly, periodic, mc, fill, residual, out_dtype)
    want = sn.plane_smooth(v, area, wx, wy, lx, ly, periodic, mc, fill, residual,
                           out_dtype or v.dtype)
    assert got.dtype == want.dtype == (out_dtype or v.dtype)
    assert_same_bits(got, want, what)
    return got


def _weights(W, seed):
    return np.random.default_rng(seed).uniform(0.2, 1.0, W)


def test_the_geometry_gives_the_tests_their_shapes():
    th, tw, maxw, recwin = _geometry()
    assert th >= 2 and tw >= 8 and maxw >= 33 and recwin >= 1
    assert _plane()[0] > th and _plane()[1] > tw and _plane()[1] % 4 == 0


# ---- dtypes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("adt", (F64, F32), ids=("a64", "a32"))
@pytest.mark.parametrize("vdt", (F64, F32), ids=("v64", "v32"))
def test_dtypes_and_a_float32_result_is_the_float64_result_rounded_once(vdt, adt):
    ny, nx = _plane()
    v, area = make_case(2, ny, nx, vdt, adt, seed=1)
    wx, wy = _weights(5, 2), _weights(3, 3)
    r64 = check(v, area, wx, wy, 2, 1, out_dtype=F64, what=f"{vdt.__name__}/{adt.__name__} -> f64")
    r32 = check(v, area, wx, wy, 2, 1, out_dtype=F32, what=f"{vdt.__name__}/{adt.__name__} -> f32")
    assert_same_bits(r32, np.where(np.isnan(r64), np.float32(np.nan), r64.astype(F32)), "rounded once")
    native = check(v, area, wx, wy, 2, 1, what="the record's own dtype")
    assert native.dtype == vdt and np.isfinite(native).any() and np.isnan(native).any()


# ---- tile boundaries: every window class, both paths ---------------------------------------------
def _windows():
    _, _, maxw, _ = _geometry()
    # (Wx, Wy, lead_x, lead_y)
    return {"1x1": (1, 1, 0, 0), "3x3": (3, 3, 1, 1), "7x4-off": (7, 4, 5, 0), "4x9-off": (4, 9, 0, 7),
            "max": (maxw, maxw, maxw // 2, maxw // 2), "max+2": (maxw + 2, maxw + 2, maxw // 2 + 1, 3),
            "max-by-3": (maxw, 3, 0, 2), "3-by-max+2": (3, maxw + 2, 1, maxw)}


@pytest.mark.parametrize("periodic", (True, False), ids=("periodic", "closed"))
@pytest.mark.parametrize("name", list(_windows()))
def test_windows_across_the_tile_boundaries(name, periodic):
    """the window straddles the tile boundary each way, wraps at x = 0 (or leaves the plane there)
    and leaves the plane north and south; max + 2 takes the generic path"""
    Wx, Wy, lx, ly = _windows()[name]
    ny, nx = _plane(Wy)
    v, area = make_case(2, ny, nx, seed=10 + Wx)
    got = check(v, area, _weights(Wx, Wx), _weights(Wy, 100 + Wy), lx, ly, periodic, fill=True,
                what=f"{name} periodic={periodic}")
    assert np.isfinite(got).any()
    if name == "3x3":
        assert np.isnan(got[:, 6:10, 24:48]).all()  # den == 0 inside the land block


@pytest.mark.parametrize("vdt", (F64, F32), ids=("v64", "v32"))
def test_a_window_as_wide_as_the_plane(vdt):
    """Wx == nx: with periodic x every output column sums the whole row, each from its own start"""
    th, tw = core.smooth_tile(vdt)
    ny = th + 1
    for nx in (tw, 20):  # (the tiled path needs Wx <= max_window: nx = tile_w goes cell by cell)
        v, area = make_case(2, ny, nx, vdt, seed=nx, land=False)
        for periodic in (True, False):
            check(v, area, _weights(nx, 5), _weights(3, 6), nx // 2, 1, periodic,
                  what=f"Wx == nx == {nx} periodic={periodic}")
    _, _, maxw, _ = _geometry()
    nx = (maxw // 4) * 4  # the widest whole-pack plane the tiled path would take, were it a tile wide
    v, area = make_case(1, ny, nx, vdt, seed=3, land=False)
    check(v, area, _weights(nx, 7), [1.0], nx - 1, 0, True, what=f"Wx == nx == {nx}, trailing")


# ---- the weight table ----------------------------------------------------------------------------
@pytest.mark.parametrize("Wx", (3, 9, 35))
def test_a_table_with_one_row_of_x_weights_per_source_row(Wx):
    ny, nx = _plane(5)
    v, area = make_case(2, ny, nx, seed=20 + Wx)
    table = np.random.default_rng(Wx).uniform(0.1, 1.0, (ny, Wx))
    table[3, : Wx // 2] = 0.0  # a zero-padded row, as length_scale_weights makes them
    assert len({tuple(r) for r in table}) == ny
    for periodic in (True, False):
        got = check(v, area, table, _weights(5, 1), Wx // 2, 2, periodic, what=f"table Wx={Wx}")
        one_row = sn.plane_smooth(v, area, table[0], _weights(5, 1), Wx // 2, 2, periodic, 1)
        assert (_bits(got) != _bits(one_row)).any()  # (the rows are really used)


# ---- flags ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", (False, True), ids=("smooth", "residual"))
@pytest.mark.parametrize("fill", (False, True), ids=("nofill", "fill"))
@pytest.mark.parametrize("mc", ("1", "mid", "all"))
def test_min_count_fill_and_residual(mc, fill, residual):
    ny, nx = _plane()
    seen, cases = [], []
    for (Wx, Wy), vdt in (((5, 3), F64), ((9, 9), F32), ((35, 3), F64)):
        v, area = make_case(2, ny, nx, vdt, seed=30 + Wx)
        cases.append((v, area))
        count = {"1": 1, "mid": (Wx * Wy) // 2, "all": Wx * Wy}[mc]
        got = check(v, area, _weights(Wx, 1), _weights(Wy, 2), Wx // 2, Wy // 2, True, count, fill,
                    residual, what=f"{Wx}x{Wy} mc={count} fill={fill} residual={residual}")
        seen.append(got)
    got = seen[0]
    v, area = cases[0]
    centre = ~np.isnan(v) & (area > 0)[None]  # (NaN compares false)
    if mc == "1" and fill and not residual:
        assert np.isfinite(got[~centre]).any()  # filled from the neighbours
    if not fill or residual:
        assert np.isnan(got[~centre]).all()
    if mc == "all":
        assert np.isnan(got[:, 0]).all() and np.isfinite(got).any()  # the window leaves the plane


# ---- records --------------------------------------------------------------------------------------
@pytest.mark.parametrize("Wx", (3, 35), ids=("tiled", "generic"))
def test_one_more_record_than_the_window_and_each_record_alone(Wx):
    _, _, _, recwin = _geometry()
    ny, nx = _plane()
    v, area = make_case(recwin + 1, ny, nx, seed=40)
    v[1] = np.nan  # a record without a valid cell
    wx, wy = _weights(Wx, 3), _weights(3, 4)
    together = check(v, area, wx, wy, Wx // 2, 1, what=f"{recwin + 1} records")
    assert np.isnan(together[1]).all()
    for rec in (0, 1, recwin - 1, recwin):
        alone = run(v[rec:rec + 1], area, wx, wy, Wx // 2, 1)
        assert_same_bits(alone[0], together[rec], f"record {rec} alone")
    again = run(v, area, wx, wy, Wx // 2, 1)
    assert_same_bits(again, together, "a second run")


# ---- a record of ones -----------------------------------------------------------------------------
@pytest.mark.parametrize("vdt, adt", ((F64, F64), (F32, F32), (F64, F32)))
def test_a_record_of_ones_is_exactly_one(vdt, adt):
    _, _, maxw, _ = _geometry()
    ny, nx = _plane(maxw + 2)
    v, area = make_case(2, ny, nx, vdt, adt, seed=50)
    ones = np.where(np.isnan(v), np.nan, 1.0).astype(vdt)
    table = np.random.default_rng(4).uniform(0.1, 1.0, (ny, 7))
    for wx, wy, what in ((_weights(3, 1), _weights(3, 2), "3x3"), (table, _weights(5, 3), "table"),
                         (_weights(maxw, 5), _weights(maxw, 6), "max"),
                         (_weights(maxw + 2, 7), _weights(maxw + 2, 8), "max+2")):
        Wx, Wy = np.shape(wx)[-1], len(wy)
        for fill in (False, True):
            got = check(ones, area, wx, wy, Wx // 2, Wy // 2, True, 1, fill, what=f"ones {what}")
            assert set(np.unique(got[~np.isnan(got)]).tolist()) == {1.0}, what
