"""GPU: the tiled path of the horizontal filter (k_smooth_tiled, csrc/momlevel_smooth.hip) on planes
with real tilings, against tests/smooth_numpy.py BIT FOR BIT.  The other smooth suites run one
geometry -- a tile plus one row by a tile plus one pack -- where no tile has a neighbour on both
sides, no plane is a whole number of tiles and a call has three records of a wide window at most.

PLANES, from core.smooth_tile (th x tw): one tile, whose periodic halo is the tile itself; exact
multiples; four tiles each way with an interior tile and partial last ones; a second band of one
row; many tiles across.  WINDOWS: four and more per window class (the kernel is compiled for
windows up to 5, up to 9 and up to core.smooth_max_window), whose lead_x cover the four residues
mod 4 -- every shift of the staged row against the output columns -- and lead 0 and W - 1 each way.
LEGAL is the explicit table of the pairs whose window the plane holds (Wy <= ny); each sweep counts
the pairs it ran against it.

Every tiled call asserts its path from core.smooth_tiled and from the record's address.  The record
carries its block of land across the corner (th, tw) of four tiles where the plane has one.  Every
reference is asserted to hold finite values in half of its cells at least, and NaNs too where FILL
is not set, before anything is compared with it."""

import numpy as np
import pytest
import torch

import smooth_numpy as sn
from momlevel_amd import core
from out_contract import Guarded
from test_gpu_smooth import F32, F64, TORCH, _dev, _weights, assert_same_bits, make_case
from test_gpu_smooth_edges import _abi, _offset_by_one

pytestmark = pytest.mark.gpu

TH, TW = core.smooth_tile(F64)
MAXW, RECWIN = core.smooth_max_window(), core.smooth_record_window()

PLANES = {"one": (TH, TW), "exact": (2 * TH, 2 * TW), "interior": (3 * TH + 1, 3 * TW + 4),
          "band": (TH + 1, 3 * TW), "wide": (TH, 5 * TW + 8)}

# (Wx, Wy, lead_x, lead_y)
WINDOWS = {
    "s3x3": (3, 3, 0, 1), "s5x3": (5, 3, 1, 0), "s5x5": (5, 5, 2, 4), "s4x5": (4, 5, 3, 2),
    "m9x9": (9, 9, 0, 4), "m7x4": (7, 4, 5, 0), "m9x6": (9, 6, 2, 5), "m8x9": (8, 9, 7, 3),
    "max": (MAXW, MAXW, MAXW // 2, MAXW // 2), "max-by-3": (MAXW, 3, 0, 2), "3-by-max": (3, MAXW, 2, 0),
    "max-by-12": (MAXW, TH - 4, MAXW - 4, 5), "max-by-17": (MAXW, TH + 1, MAXW - 2, 9),
    "max-trailing": (MAXW, 5, MAXW - 1, 0),
}
CLASSES = {"S": (1, 5), "M": (6, 9), "L": (10, MAXW)}  # by max(Wx, Wy)

_LOW = ("s3x3", "s5x3", "s5x5", "s4x5", "m9x9", "m7x4", "m9x6", "m8x9", "max-by-3", "max-by-12",
        "max-trailing")  # Wy <= th
LEGAL = {
    "one": _LOW,
    "exact": _LOW + ("max-by-17",),
    "interior": _LOW + ("max-by-17", "max", "3-by-max"),
    "band": _LOW + ("max-by-17",),
    "wide": _LOW,
}
PAIRS = [(plane, window) for plane, names in LEGAL.items() for window in names]
ONE_PER_CLASS = ("s5x5", "m8x9", "max-by-17")


def _class(window):
    W = max(WINDOWS[window][:2])
    return next(c for c, (lo, hi) in CLASSES.items() if lo <= W <= hi)


def corner_case(nrec, ny, nx, vdt=F64, adt=F64, seed=0, p_nan=0.03, p_area=0.02):
    """test_gpu_smooth.make_case with its block of land across the corner (th, tw), where the plane
    has that corner: 12 rows by 32 columns on the halos of four tiles, its west half NaN in v, its
    east half without area"""
    if not (ny > TH and nx > TW):
        assert (p_nan, p_area) == (0.03, 0.02)
        return make_case(nrec, ny, nx, vdt, adt, seed)
    rng = np.random.default_rng(seed)
    v = rng.normal(0.2, 1.0, (nrec, ny, nx))
    v[rng.random(v.shape) < p_nan] = np.nan
    area = rng.uniform(4.0e8, 9.0e8, (ny, nx))
    area[rng.random((ny, nx)) < p_area] = 0.0
    area[rng.random((ny, nx)) < p_area] = np.nan
    v[:, TH - 6:TH + 6, TW - 16:TW] = np.nan
    area[TH - 6:TH + 6, TW:TW + 16] = 0.0
    return v.astype(vdt), area.astype(adt)


def _reference(v, area, wx, wy, lx, ly, periodic, mc, fill, residual, odt, what):
    """the restatement, once it is seen to be worth comparing with"""
    want = sn.plane_smooth(v, area, wx, wy, lx, ly, periodic, mc, fill, residual, odt)
    share = float(np.isfinite(want).mean())
    assert share >= 0.5, f"{what}: only {share:.2f} of the reference is finite"
    if not fill:
        assert np.isnan(want).any(), f"{what}: the reference has no NaN"
    return want


def _tiled(v, area, wx, wy, lx, ly, periodic, mc=1, fill=False, residual=False, out_dtype=None):
    """core.plane_smooth through k_smooth_tiled: the path is asserted from the query and from the
    addresses"""
    nrec, ny, nx = v.shape
    assert core.smooth_tiled(np.shape(wx)[-1], len(wy), ny, nx) == 1
    dv = _dev(v)
    assert dv.data_ptr() % 16 == 0
    out = core.plane_smooth(dv, _dev(area), wx, wy, lx, ly, periodic, mc, fill=fill, residual=residual,
                            out_dtype=None if out_dtype is None else TORCH[out_dtype])
    torch.cuda.synchronize()
    assert out.data_ptr() % 16 == 0
    return out.cpu().numpy()


def _generic(v, area, wx, wy, lx, ly, periodic, mc=1, fill=False, residual=False, out_dtype=None):
    """the same operands through k_smooth_cells: the record one element off the 16-byte grid"""
    out = core.plane_smooth(_offset_by_one(v), _dev(area), wx, wy, lx, ly, periodic, mc, fill=fill,
                            residual=residual, out_dtype=None if out_dtype is None else TORCH[out_dtype])
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _guarded(v, area, wx, wy, lx, ly, periodic, flags, odt):
    """mlx_smooth_apply itself into a guard-banded buffer that starts on a 16-byte boundary"""
    g = Guarded(v.shape, TORCH[odt], "cuda", offset=0)
    dv = _dev(v)
    assert core.smooth_tiled(wx.size, wy.size, v.shape[1], v.shape[2]) == 1
    assert dv.data_ptr() % 16 == 0 and g.view.data_ptr() % 16 == 0
    _abi(dv, _dev(area), _dev(wx), _dev(wy), lx, ly, periodic, 1, flags, g.view)
    return g


def test_the_tables_cover_what_they_claim():
    assert (TH, TW) == core.smooth_tile(F32) and TH >= 13 and TW >= MAXW + 4 and RECWIN >= 2
    for ny, nx in PLANES.values():
        assert nx % 4 == 0 and core.smooth_tiled(1, 1, ny, nx) == 1
    tiles = {name: (-(-ny // TH), -(-nx // TW)) for name, (ny, nx) in PLANES.items()}
    assert tiles == {"one": (1, 1), "exact": (2, 2), "interior": (4, 4), "band": (2, 3), "wide": (1, 6)}
    for cls in CLASSES:
        names = [w for w in WINDOWS if _class(w) == cls]
        assert len(names) >= 2
        wins = [WINDOWS[w] for w in names]
        assert {lx % 4 for _, _, lx, _ in wins} == {0, 1, 2, 3}, cls
        assert any(lx == 0 for _, _, lx, _ in wins) and any(lx == Wx - 1 for Wx, _, lx, _ in wins)
        assert any(ly == 0 for _, _, _, ly in wins) and any(ly == Wy - 1 for _, Wy, _, ly in wins)
    for shape in ((MAXW, MAXW), (MAXW, 3), (3, MAXW)):
        assert any(WINDOWS[w][:2] == shape for w in WINDOWS)
    # LEGAL is every pair whose window the plane holds, and every one of them is a tiled call
    for plane, (ny, nx) in PLANES.items():
        fits = {w for w, (Wx, Wy, lx, ly) in WINDOWS.items() if Wy <= ny and Wx <= nx}
        assert set(LEGAL[plane]) == fits and len(set(LEGAL[plane])) == len(LEGAL[plane]), plane
        for w in LEGAL[plane]:
            Wx, Wy, lx, ly = WINDOWS[w]
            assert core.smooth_tiled(Wx, Wy, ny, nx) == 1 and 0 <= lx < Wx and 0 <= ly < Wy
    assert len(PAIRS) == sum(len(v) for v in LEGAL.values()) == 60
    assert [_class(w) for w in ONE_PER_CLASS] == ["S", "M", "L"]
    assert all(w in LEGAL["interior"] and w in LEGAL["exact"] for w in ONE_PER_CLASS)


# ---- 1. the sweep -----------------------------------------------------------------------------------
@pytest.mark.parametrize("periodic", (True, False), ids=("periodic", "closed"))
def test_every_window_on_every_tiling_through_both_paths(periodic):
    ran = 0
    for n, (plane, window) in enumerate(PAIRS):
        ny, nx = PLANES[plane]
        Wx, Wy, lx, ly = WINDOWS[window]
        v, area = corner_case(2, ny, nx, seed=100 + n)
        wx, wy = _weights(Wx, n), _weights(Wy, 1000 + n)
        what = f"{plane} {ny}x{nx}, {window} {Wx}x{Wy} lead ({lx}, {ly}), periodic={periodic}"
        want = _reference(v, area, wx, wy, lx, ly, periodic, 1, True, False, F64, what)
        got = _tiled(v, area, wx, wy, lx, ly, periodic, fill=True)
        assert_same_bits(got, want, what)
        assert_same_bits(_generic(v, area, wx, wy, lx, ly, periodic, fill=True), got, what + ": cell by cell")
        ran += 1
    print(f"{ran} (plane, window) pairs of {len(PAIRS)}, periodic={periodic}, through both paths")
    assert ran == len(PAIRS)


# ---- 2. dtypes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("adt", (F64, F32), ids=("a64", "a32"))
@pytest.mark.parametrize("vdt", (F64, F32), ids=("v64", "v32"))
def test_every_dtype_combination_on_the_interior_plane(vdt, adt):
    ny, nx = PLANES["interior"]
    ran = 0
    for window in ONE_PER_CLASS:
        Wx, Wy, lx, ly = WINDOWS[window]
        v, area = corner_case(2, ny, nx, vdt, adt, seed=200 + Wx)
        wx, wy = _weights(Wx, 2), _weights(Wy, 3)
        res = {}
        for odt in (F64, F32):
            what = f"{window}: {vdt.__name__}/{adt.__name__} -> {odt.__name__}"
            want = _reference(v, area, wx, wy, lx, ly, True, 1, False, False, odt, what)
            res[odt] = _tiled(v, area, wx, wy, lx, ly, True, out_dtype=odt)
            assert res[odt].dtype == odt
            assert_same_bits(res[odt], want, what)
            ran += 1
        r64 = res[F64]
        assert_same_bits(res[F32], np.where(np.isnan(r64), np.float32(np.nan), r64.astype(F32)),
                         f"{window}: rounded once")
    print(f"{ran} (window, out dtype) cases for v {vdt.__name__}, area {adt.__name__}")
    assert ran == 2 * len(ONE_PER_CLASS)


# ---- 3. flags -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", (False, True), ids=("smooth", "residual"))
@pytest.mark.parametrize("fill", (False, True), ids=("nofill", "fill"))
def test_flags_and_min_count_on_the_interior_plane(fill, residual):
    """few isolated invalid cells (and the land), so that a window that must be whole often is"""
    ny, nx = PLANES["interior"]
    ran = 0
    for window in ("m7x4", "max-by-3"):
        Wx, Wy, lx, ly = WINDOWS[window]
        v, area = corner_case(2, ny, nx, seed=300 + Wx, p_nan=0.001, p_area=0.0005)
        wx, wy = _weights(Wx, 4), _weights(Wy, 5)
        whole = None
        for mc in (1, Wx * Wy // 2, Wx * Wy):
            what = f"{window} mc={mc} fill={fill} residual={residual}"
            want = _reference(v, area, wx, wy, lx, ly, True, mc, fill, residual, F64, what)
            got = _tiled(v, area, wx, wy, lx, ly, True, mc, fill, residual)
            assert_same_bits(got, want, what)
            assert whole is None or np.isnan(want).sum() > np.isnan(whole).sum()  # (mc bites)
            whole = want
            ran += 1
    assert ran == 6


# ---- 4. the weight table ------------------------------------------------------------------------------
@pytest.mark.parametrize("periodic", (True, False), ids=("periodic", "closed"))
@pytest.mark.parametrize("Wx", (9, MAXW))
def test_a_table_with_one_row_of_x_weights_per_source_row(Wx, periodic):
    ny, nx = PLANES["interior"]
    v, area = corner_case(2, ny, nx, seed=400 + Wx)
    table = np.random.default_rng(Wx).uniform(0.1, 1.0, (ny, Wx))
    table[3, : Wx // 2] = 0.0  # a zero-padded row, as length_scale_weights makes them
    assert len({tuple(r) for r in table}) == ny
    wy, lx = _weights(5, 1), Wx // 2 + 1
    what = f"table Wx={Wx} periodic={periodic}"
    want = _reference(v, area, table, wy, lx, 2, periodic, 1, False, False, F64, what)
    got = _tiled(v, area, table, wy, lx, 2, periodic)
    assert_same_bits(got, want, what)
    one_row = sn.plane_smooth(v, area, table[0], wy, lx, 2, periodic, 1)
    assert (got.view(np.int64) != one_row.view(np.int64)).any()  # (the rows are really used)


# ---- 5. long records ----------------------------------------------------------------------------------
def _twice(*a, **kw):
    first = _tiled(*a, **kw)
    assert_same_bits(_tiled(*a, **kw), first, "a second run")
    return first


@pytest.mark.parametrize("nrec", (RECWIN, 2 * RECWIN + 1), ids=("recwin", "2recwin+1"))
def test_long_records_and_the_records_around_a_window_alone(nrec):
    """a whole record window, and two and one record of a third: the prefetch of the next chunk
    hops from the last chunk of a record to the first of the next in every block"""
    ny, nx = PLANES["interior"]
    table = np.random.default_rng(7).uniform(0.1, 1.0, (ny, MAXW))
    cases = [(w,) + WINDOWS[w] + (None,) for w in ("s4x5", "m9x6", "max")]
    cases.append(("table", MAXW, 5, MAXW // 2, 2, table))
    ran = 0
    for name, Wx, Wy, lx, ly, wx in cases:
        v, area = corner_case(nrec, ny, nx, seed=500 + Wx + Wy)
        v[1] = np.nan  # a record without a valid cell
        wx, wy = _weights(Wx, 6) if wx is None else wx, _weights(Wy, 7)
        what = f"{name}, {nrec} records"
        want = _reference(v, area, wx, wy, lx, ly, True, 1, True, False, F64, what)
        together = _twice(v, area, wx, wy, lx, ly, True, fill=True)
        assert_same_bits(together, want, what)
        assert np.isnan(together[1]).all()
        alone = [rec for rec in (RECWIN - 1, RECWIN, 2 * RECWIN) if rec < nrec]
        assert len(alone) == (1 if nrec == RECWIN else 3)
        for rec in alone:
            one = _twice(v[rec:rec + 1], area, wx, wy, lx, ly, True, fill=True)
            assert_same_bits(one[0], together[rec], f"{what}: record {rec} alone")
        ran += 1
    assert ran == 4


# ---- 6. translation -----------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", ("one", "interior"))
@pytest.mark.parametrize("vdt", (F64, F32), ids=("v64", "v32"))
def test_rolling_the_plane_in_periodic_x_rolls_the_result(vdt, plane):
    """no restatement: with periodic x, v and area rolled by k columns give the result rolled by
    k columns, bit for bit -- tile seams, the staged packs and the wrap fall on other cells, the
    sums do not change.  (A table of x weights has one row per source ROW: it stays as it is.)
    k = 4 is one pack, k = tw one tile, k = tw + 4 both."""
    ny, nx = PLANES[plane]
    table = np.random.default_rng(8).uniform(0.1, 1.0, (ny, 9))
    cases = [WINDOWS[w] + (None,) for w in ("s5x3", "m9x6", "max-by-12")] + [(9, 5, 3, 2, table)]
    ran = 0
    for Wx, Wy, lx, ly, wx in cases:
        v, area = corner_case(2, ny, nx, vdt, seed=600 + Wx)
        wx, wy = _weights(Wx, 8) if wx is None else wx, _weights(Wy, 9)
        base = _tiled(v, area, wx, wy, lx, ly, True)
        assert np.isfinite(base).mean() >= 0.5 and np.isnan(base).any()
        for k in (4, TW, TW + 4):
            rolled = _tiled(np.roll(v, k, axis=2), np.roll(area, k, axis=1), wx, wy, lx, ly, True)
            assert_same_bits(rolled, np.roll(base, k, axis=2), f"{plane} {Wx}x{Wy} rolled by {k}")
            ran += 1
    assert ran == 12


# ---- 7. guard bands -----------------------------------------------------------------------------------
@pytest.mark.parametrize("odt", (F64, F32), ids=("o64", "o32"))
@pytest.mark.parametrize("plane, wide", (("exact", "max-by-17"), ("interior", "max")))
def test_the_tiled_result_is_written_inside_its_buffer_and_nowhere_else(plane, wide, odt):
    """whole tiles only, and partial tiles at both far edges"""
    ny, nx = PLANES[plane]
    ran = 0
    for window in ("s5x5", wide):
        Wx, Wy, lx, ly = WINDOWS[window]
        v, area = corner_case(3, ny, nx, seed=700 + Wx)
        wx, wy = _weights(Wx, 5), _weights(Wy, 6)
        for flags, (fill, residual) in ((0, (False, False)), (3, (True, True))):
            what = f"guarded {plane} {window} flags={flags} {odt.__name__}"
            want = _reference(v, area, wx, wy, lx, ly, True, 1, fill, residual, odt, what)
            g = _guarded(v, area, wx, wy, lx, ly, True, flags, odt)
            g.assert_intact(what)
            assert g.unwritten() == 0
            assert_same_bits(g.view, want, what)
            ran += 1
    assert ran == 4
