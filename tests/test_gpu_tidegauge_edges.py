"""GPU: the tide-gauge search of csrc/momlevel_gauge.hip (k_gauge_prepare, k_gauge_nearest,
k_gauge_combine) at every seam of its launch geometry -- the parts of the points, the 256-point
LDS tile, the 256-gauge block of the search and the 64-gauge block of the combine stage, ties
within a part and across more than 16 parts, the clamp of the part count to 65535, the prepare
table row by row, and far / antipodal winners.

Gates (none taken from what the kernels give):
  * the integer lattice (gauge_numpy.lattice_*): every chord^2 is exact in float64, so the index
    is EQUAL to int64 arithmetic and the angle is +0.0 bit for bit;
  * copies of one row: the winner is the lowest wet copy, from the chosen sets and from numpy's
    first-minimum argmin, which must agree;
  * real coordinates: the rule of test_gpu_tidegauge._compare (indices equal, no gauge excluded,
    angle within PARITY = 1e-10 relative);
  * the same search with another split, other companions or another alignment: bits identical;
  * the prepare table: phi, lam bit-equal to numpy.deg2rad, x, y, z within PARITY absolute;
  * antipodes: pi - angle <= 2 sqrt(2 m 2^-53), m = 16 ulps on the haversine argument h (four
    device sin / cos of a few ulp each, three products, one sum): asin is ill-conditioned at 1.
Every compared figure is printed before it is asserted."""

import functools
import math

import numpy as np
import pytest
import torch

import gauge_numpy as gn
from momlevel_amd import _lib, core
from test_gpu_tidegauge import GAP, PARITY, _compare

pytestmark = pytest.mark.gpu

X, Y, Z = _lib.GAUGE_ROW_X, _lib.GAUGE_ROW_Y, _lib.GAUGE_ROW_Z
PHI, LAM = _lib.GAUGE_ROW_PHI, _lib.GAUGE_ROW_LAM
LATTICE_NS = (1, 255, 256, 257, 511, 513, 1024, 1025, 2337)
ANTIPODE_ULPS = 16
ANTIPODE_BOUND = 2.0 * math.sqrt(2.0 * ANTIPODE_ULPS * 2.0 ** -53)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.view(torch.int64)


def _same(got, base, what):
    """index equal and angle bits equal between two searches"""
    same_i = torch.equal(got[0], base[0])
    same_a = torch.equal(_bits(got[1]), _bits(base[1]))
    print(f"{what}: indices identical {same_i}, angle bits identical {same_a}")
    assert same_i and same_a, what


def _splits(n, asked=(0, 1, 2, 3, 9, 17)):
    return sorted({s for s in asked if s <= n} | {n})


def _parts(n, ng, split):
    return _lib.load_gauge().mlx_gauge_nearest_split(n, ng, split)


# ---- 1. the integer lattice ----------------------------------------------------------------------
def _lattice_case(n, kind, edges_valid):
    pq, pok = gn.lattice_points(n, kind, edges_valid)
    gq, gok = gn.lattice_gauges(n, kind)
    # what makes the expectation exact: all positions are multiples of 0.25 in [0, 2^12), so every
    # difference is a multiple of 0.25 below 2^12 and every square a multiple of 2^-4 below 2^24
    assert pq.min() >= 0 and gq.min() >= 0 and max(pq.max(), gq.max()) < 4 * 2 ** 12
    assert (max(pq.max(), gq.max()) / 4.0) ** 2 < 2 ** 24  # (and 2^-4 * 2^53 > 2^24: no rounding)
    want = gn.lattice_nearest(pq, pok, gq, gok)
    return pq, pok, gq, gok, want


def _check_lattice(points, gauges, want, split, what):
    index, angle = core.gauge_nearest(points, gauges, split=split)
    index, abits = index.cpu().numpy(), _bits(angle).cpu().numpy()
    differ = np.nonzero(index != want)[0]
    print(f"{what}: {want.size} gauges, indices that differ: {differ[:20].tolist()}"
          f"{' ...' if differ.size > 20 else ''}")
    assert differ.size == 0, what
    found = want >= 0
    assert np.all(abits[found] == 0), f"{what}: the angle of a found point is not +0.0"
    assert np.isnan(angle.cpu().numpy()[~found]).all(), what
    return index


@pytest.mark.parametrize("edges_valid", (True, False), ids=("edges-valid", "edges-invalid"))
@pytest.mark.parametrize("kind", ("U", "D"))
@pytest.mark.parametrize("n", LATTICE_NS)
def test_lattice_argmin_is_exact_at_every_split(n, kind, edges_valid):
    pq, pok, gq, gok, want = _lattice_case(n, kind, edges_valid)
    points, gauges = _dev(gn.lattice_table(pq, pok)), _dev(gn.lattice_table(gq, gok))
    assert int((want < 0).sum()) == (3 if pok.any() else gq.size)
    for split in _splits(n):
        what = f"lattice {kind} n={n} split={split} ({_parts(n, gq.size, split)} parts)"
        index = _check_lattice(points, gauges, want, split, what)
        if kind == "U":  # every valid point is some gauge's winner: no slot of a tile or part untested
            assert np.array_equal(np.unique(index[index >= 0]), np.nonzero(pok)[0]), what
    if n == 2337:  # the seams this size is chosen for
        lib = _lib.load_gauge()
        assert lib.mlx_gauge_nearest_split(n, gq.size, 0) == 3
        assert lib.mlx_gauge_nearest_split(n, gq.size, 9) == 9 and -(-n // 9) == 260
        assert lib.mlx_gauge_nearest_split(n, gq.size, 17) == 17 and -(-n // 17) == 138


# ---- 2. the combine stage's tie rule -------------------------------------------------------------
@pytest.mark.parametrize("offset", (False, True), ids=("on-the-point", "offset"))
@pytest.mark.parametrize("copies", (20, 40))
def test_ties_across_more_than_sixteen_parts(copies, offset):
    m = 70
    lat, lon, mask, wet = gn.stacked_rows(copies, m)
    glat, glon = lat[0].copy(), lon[0].copy()
    if offset:
        glat, glon = glat + 0.01, glon - 0.01
    # expected, two ways: from the chosen sets and by numpy's first-minimum argmin
    want_index, want_angle, _gap = gn.nearest(lat, lon, glat, glon, mask)
    direct = np.array([min(s) * m + c if s else -1 for c, s in enumerate(wet)])
    chosen = direct >= 0
    assert np.array_equal(want_index[chosen], direct[chosen])
    dry = gn.TIE_DRY_COLUMN
    assert not chosen[dry] and chosen.sum() == m - 1 and want_index[dry] % m in (dry - 1, dry + 1)
    # (the dry column's own gap, among distinct points: copies tie exactly and are not a gap)
    one_row = (mask.sum(axis=0) > 0).astype(np.float64)
    _i, _a, row_gap = gn.nearest(lat[0], lon[0], glat[dry], glon[dry], one_row)
    print(f"{copies} copies: the dry column finds column {want_index[dry] % m}, gap {row_gap[0]:.3e}")
    assert row_gap[0] >= GAP

    points, _ = core.gauge_prepare(lat, lon, mask)
    gauges, _ = core.gauge_prepare(glat, glon)
    assert _parts(copies * m, m, copies) == copies > 16  # chunk = m: part p is copy p
    runs = {s: core.gauge_nearest(points, gauges, split=s) for s in (copies, 1, 0)}
    index = runs[copies][0].cpu().numpy()
    angle = runs[copies][1].cpu().numpy()
    differ = np.nonzero(index != want_index)[0]
    print(f"{copies} copies, split {copies}: columns whose winner differs {differ.tolist()}: "
          f"got copies {(index[differ] // m).tolist()}, wet {[wet[c] for c in differ]}")
    assert differ.size == 0
    if offset:
        rel = np.max(np.abs(angle - want_angle) / want_angle)
    else:
        assert np.all(angle[chosen] == 0.0)
        rel = abs(angle[dry] - want_angle[dry]) / want_angle[dry]
    print(f"max relative angle difference {rel:.3e} (gate {PARITY:.0e})")
    assert rel <= PARITY
    for s in (1, 0):
        _same(runs[s], runs[copies], f"{copies} copies, split {s} against split {copies}")


@pytest.mark.parametrize("edges_valid", (True, False), ids=("edges-valid", "edges-invalid"))
def test_lattice_duplicates_across_forty_parts(edges_valid):
    n = 40 * 64
    pq, pok, gq, gok, want = _lattice_case(n, "D", edges_valid)
    points, gauges = _dev(gn.lattice_table(pq, pok)), _dev(gn.lattice_table(gq, gok))
    assert _parts(n, gq.size, 40) == 40
    diff = np.abs(gq[:, None] - pq[None, :])
    diff[:, ~pok] = diff.max() + 1
    tied = ((diff == diff.min(axis=1)[:, None]).sum(axis=1) > 1) & gok
    print(f"gauges whose minimum is met at more than one point: {tied.sum()} of {gq.size}")
    assert tied.sum() > gq.size // 2
    _check_lattice(points, gauges, want, 40, f"lattice D n={n} split=40")


# ---- 3. every point its own gauge ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grid():
    lat, lon, mask, _glat, _glon = gn.synthetic_grid(41, 57, 1, 11)
    return lat, lon, mask


@functools.lru_cache(maxsize=None)
def _grid_restated():
    lat, lon, mask = _grid()
    return gn.nearest(lat, lon, lat, lon, mask)


def test_every_point_finds_itself():
    lat, lon, _mask = _grid()
    n = lat.size
    assert n == 2337
    points, valid = core.gauge_prepare(lat, lon)
    gauges, _ = core.gauge_prepare(lat, lon)
    assert bool(valid.all()) and torch.equal(_bits(points), _bits(gauges))
    base = None
    for split in (0, 1, 9, n):
        index, angle = core.gauge_nearest(points, gauges, split=split)
        off = torch.nonzero(index != torch.arange(n, device=index.device)).reshape(-1)
        print(f"split {split}: points that do not find themselves {off.tolist()[:20]}")
        assert off.numel() == 0
        assert bool((_bits(angle) == 0).all()), f"split {split}: angle is not +0.0 everywhere"
        base = base or (index, angle)
        _same((index, angle), base, f"no mask, split {split}")


def test_dry_points_find_their_wet_neighbour():
    lat, lon, mask = _grid()
    n = lat.size
    want_index, want_angle, gap = _grid_restated()
    dry = mask.reshape(-1) == 0.0
    assert int(dry.sum()) == 709
    assert np.array_equal(want_index[~dry], np.nonzero(~dry)[0])
    assert not np.any(want_index[dry] == np.nonzero(dry)[0])
    print(f"smallest relative gap among the dry gauges {gap[dry].min():.3e}")
    points, valid = core.gauge_prepare(lat, lon, mask)
    gauges, _ = core.gauge_prepare(lat, lon)
    assert np.array_equal(valid.cpu().numpy().astype(bool), ~dry)
    runs = {s: core.gauge_nearest(points, gauges, split=s) for s in (0, 1, 9, n)}
    _compare(runs[1][0], runs[1][1], want_index, want_angle, gap, "41x57, its own points as gauges")
    wet_angle = runs[1][1].cpu().numpy()[~dry]
    assert np.all(wet_angle.view(np.int64) == 0)
    for s in (0, 9, n):
        _same(runs[s], runs[1], f"masked, split {s} against split 1")


# ---- 4. a gauge's result is its own --------------------------------------------------------------
def _offset_copy(table):
    """the same (5, n) table one element into a larger flat buffer: 8- but not 16-byte aligned"""
    flat = torch.empty(table.numel() + 1, dtype=torch.float64, device=table.device)
    view = flat[1:].view(table.shape)
    view.copy_(table)
    assert view.is_contiguous() and view.data_ptr() % 16 == 8
    return view


def test_a_gauge_does_not_depend_on_its_companions():
    lat, lon, mask, glat, glon = gn.synthetic_grid(41, 57, 513, 11)
    assert np.array_equal(lat, _grid()[0]) and np.array_equal(mask, _grid()[2])
    want_index, want_angle, gap = gn.nearest(lat, lon, glat, glon, mask)
    points, _ = core.gauge_prepare(lat, lon, mask)
    gauges, _ = core.gauge_prepare(glat, glon)
    big = core.gauge_nearest(points, gauges)
    _compare(big[0], big[1], want_index, want_angle, gap, "41x57, 513 gauges")

    def cut(sel):
        return big[0][sel], big[1][sel]

    def search(sel):
        return core.gauge_nearest(points, gauges[:, sel].contiguous())

    for k in (1, 63, 64, 65, 255, 256, 257):
        _same(search(slice(0, k)), cut(slice(0, k)), f"the first {k} gauges alone")
    _same(search(slice(200, 457)), cut(slice(200, 457)), "gauges 200..456 alone")
    perm = torch.from_numpy(np.random.default_rng(513).permutation(513)).cuda()
    _same(search(perm), cut(perm), "all 513 gauges, permuted")
    _same(core.gauge_nearest(points, gauges), big, "the same call again")
    # prepared separately, a subset has the same table columns: prepare is per element too
    alone, _ = core.gauge_prepare(glat[200:457], glon[200:457])
    assert torch.equal(_bits(alone), _bits(gauges[:, 200:457].contiguous()))
    # tables that are 8- but not 16-byte aligned
    for split in (0, 9):
        ref = core.gauge_nearest(points, gauges, split=split)
        _same(core.gauge_nearest(_offset_copy(points), gauges, split=split), ref,
              f"points off by one element, split {split}")
        _same(core.gauge_nearest(points, _offset_copy(gauges), split=split), ref,
              f"gauges off by one element, split {split}")
        _same(core.gauge_nearest(_offset_copy(points), _offset_copy(gauges), split=split), ref,
              f"both off by one element, split {split}")


# ---- 5. more parts asked for than a launch may have ----------------------------------------------
@pytest.mark.parametrize("ny,nx", ((257, 510), (257, 511)))
def test_the_part_count_is_clamped_to_the_grid_limit(ny, nx):
    n, ng = ny * nx, 5
    lat, lon, mask, glat, glon = gn.synthetic_grid(ny, nx, ng, 5)
    parts = _parts(n, ng, n)
    print(f"{n} points, split {n}: {parts} parts; default {_parts(n, ng, 0)}")
    assert 16 < parts <= 65535 and (parts == 65535 or n != 131070)
    assert _parts(n, ng, 0) > 16
    want_index, want_angle, gap = gn.nearest(lat, lon, glat, glon, mask)
    points, _ = core.gauge_prepare(lat, lon, mask)
    gauges, _ = core.gauge_prepare(glat, glon)
    clamped = core.gauge_nearest(points, gauges, split=n)
    _compare(clamped[0], clamped[1], want_index, want_angle, gap, f"{ny}x{nx}, split {n}")
    for s in (1, 0):
        _same(core.gauge_nearest(points, gauges, split=s), clamped, f"{ny}x{nx} split {s} against {n}")


# ---- 6. the prepare table ------------------------------------------------------------------------
MASK_VALUES = (1.0, 1.0, 1.0, 0.0, 0.5, 2.0, float("nan"), -0.0, 1.0, 1.0)


def _prepare_inputs(n, cdtype, mdtype):
    rng = np.random.default_rng([6, n])
    lat, lon = rng.uniform(-90.0, 90.0, n), rng.uniform(-360.0, 360.0, n)
    if n >= 16:
        lat[[1, n - 2]], lat[2], lat[3] = np.nan, np.inf, -np.inf
        lon[[4, n - 3]], lon[5], lon[6] = np.nan, -np.inf, np.inf
        lat[7], lat[8], lon[9], lon[10], lon[11] = 90.0, -90.0, 180.0, -180.0, 0.0
    lat, lon = lat.astype(cdtype), lon.astype(cdtype)
    mask = None
    if mdtype is not None:
        mask = np.array(MASK_VALUES)[rng.integers(0, len(MASK_VALUES), n)]
        if n >= 16:
            mask[:16] = 1.0  # (the bad coordinates above are wet: the coordinate alone decides)
            mask[n - 1], mask[12], mask[13] = -0.0, np.nan, 0.5
        mask = mask.astype(mdtype)
    return lat, lon, mask


@pytest.mark.parametrize("mdtype", (None, np.float64, np.float32), ids=("no-mask", "mask64", "mask32"))
@pytest.mark.parametrize("cdtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("n", (1, 255, 256, 257, 1000))
def test_the_prepare_table_row_by_row(n, cdtype, mdtype):
    lat, lon, mask = _prepare_inputs(n, cdtype, mdtype)
    table, valid = core.gauge_prepare(lat, lon, mask)
    assert table.shape == (5, n) and table.dtype == torch.float64 and table.is_contiguous()
    assert valid.shape == (n,) and valid.dtype == torch.uint8
    table, valid = table.cpu().numpy(), valid.cpu().numpy()
    ok = gn.valid_points(lat, lon, mask)
    assert set(np.unique(valid).tolist()) <= {0, 1} and np.array_equal(valid.astype(bool), ok)
    if n >= 16:
        assert not ok[[1, 2, 3, 4, 5, 6, n - 2, n - 3]].any() and ok[[7, 8, 9, 10, 11]].all()
        assert mask is None or not ok[[12, 13, n - 1]].any()
    bad = table[:, ~ok]
    inf_bits, nan = np.float64(np.inf).view(np.int64), np.isnan
    assert np.all(bad[[X, Y, Z]].view(np.int64) == inf_bits) and nan(bad[[PHI, LAM]]).all()
    phi = np.deg2rad(lat.astype(np.float64))[ok]
    lam = np.deg2rad(lon.astype(np.float64))[ok]
    good = table[:, ok]
    phi_off = int((good[PHI].view(np.int64) != phi.view(np.int64)).sum())
    lam_off = int((good[LAM].view(np.int64) != lam.view(np.int64)).sum())
    print(f"n={n}: {ok.sum()} valid; phi bits differ at {phi_off}, lam bits differ at {lam_off}")
    assert phi_off == 0 and lam_off == 0
    want = np.stack([np.cos(phi) * np.cos(lam), np.cos(phi) * np.sin(lam), np.sin(phi)])
    worst = float(np.max(np.abs(good[[X, Y, Z]] - want))) if ok.any() else 0.0
    print(f"n={n}: largest |x, y, z - numpy| {worst:.3e} (gate {PARITY:.0e}, absolute)")
    assert worst <= PARITY


# ---- 7. far and opposite -------------------------------------------------------------------------
def _one_point(plat, plon, glat, glon):
    points, _ = core.gauge_prepare([plat], [plon])
    gauges, _ = core.gauge_prepare([glat], [glon])
    index, angle = core.gauge_nearest(points, gauges)
    return index, angle


def test_the_antipode_of_the_only_wet_point():
    lat, lon, glat, glon = gn.antipodes(0.25)
    assert lat.size == 721 and lat[0] == -90.0 and lat[-1] == 90.0
    h = gn.haversine_h(*np.deg2rad([glat, glon, lat, lon]))
    print(f"numpy's own h exceeds 1 for {(h > 1.0).sum()} of {h.size} pairs")
    assert (h > 1.0).sum() >= 3
    cases = list(zip(lat, lon, glat, glon))
    cases += [(90.0, 0.0, -90.0, g) for g in (0.0, 123.0, -180.0)]    # poles with any longitude
    cases += [(-90.0, 45.0, 90.0, g) for g in (45.0, 225.0, -77.5)]
    got = [_one_point(*c) for c in cases]
    index = torch.cat([g[0] for g in got]).cpu().numpy()
    angle = torch.cat([g[1] for g in got]).cpu().numpy()
    assert np.all(index == 0)
    short = math.pi - angle
    worst = int(np.nanargmax(short)) if not np.isnan(short).all() else 0
    print(f"{len(cases)} antipodal pairs: NaN angles {int(np.isnan(angle).sum())}, above pi "
          f"{int((angle > math.pi).sum())}, angle == pi {int((angle == math.pi).sum())}, "
          f"largest pi - angle {short[worst]:.3e} at latitude {cases[worst][0]} "
          f"(bound {ANTIPODE_BOUND:.3e})")
    assert not np.isnan(angle).any()
    assert np.all(angle <= math.pi)
    assert np.all(short <= ANTIPODE_BOUND)


@pytest.mark.parametrize("plat,plon,glat,glon", (
    (0.0, 0.0, 0.0, 90.0), (0.0, 0.0, 0.0, -90.0), (0.0, 37.0, 90.0, 5.0), (0.0, -120.0, -90.0, 0.0),
    (90.0, 0.0, 0.0, 77.0), (45.0, 10.0, 45.0, 190.0)))
def test_a_quarter_turn(plat, plon, glat, glon):
    index, angle = _one_point(plat, plon, glat, glon)
    angle = float(angle[0])
    rel = abs(angle - math.pi / 2) / (math.pi / 2)
    print(f"({plat}, {plon}) from ({glat}, {glon}): angle {angle!r}, relative difference from "
          f"pi / 2 {rel:.3e} (gate {PARITY:.0e})")
    assert int(index[0]) == 0 and rel <= PARITY
