"""numpy restatement of util.geolocate_points (src/momlevel/util.py:252-367) without scikit-learn:
the haversine distance of BallTree(metric="haversine") by brute force, numpy's argmin (lowest index
on a tie), the ``mask == 1.0`` filter, the ``<=`` threshold and ``mod_index``, the rank of the
chosen point among the valid ones.  Shared by tests/test_tidegauge_host.py and
tests/test_gpu_tidegauge.py; a test helper, not part of the product.

For tests/test_gpu_tidegauge_edges.py also: hand-made search tables on an integer lattice whose
argmin needs no floating point (lattice_*), stacked copies of one row with chosen wet copies
(stacked_rows) and the antipodal sweep (antipodes, haversine_h)."""

import json
import os

import numpy as np

from momlevel_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def haversine(phi1, lam1, phi2, lam2):
    """the angle in radians between (phi1, lam1) and (phi2, lam2), all in radians -- operator for
    operator scikit-learn's haversine_dist: 2 asin(sqrt(sin^2(dphi/2) + cos cos sin^2(dlam/2)))"""
    s0 = np.sin(0.5 * (phi1 - phi2))
    s1 = np.sin(0.5 * (lam1 - lam2))
    return 2.0 * np.arcsin(np.sqrt(s0 * s0 + np.cos(phi1) * np.cos(phi2) * s1 * s1))


def valid_points(lat, lon, mask=None):
    lat, lon = np.asarray(lat, dtype=np.float64).reshape(-1), np.asarray(lon, dtype=np.float64).reshape(-1)
    ok = np.isfinite(lat) & np.isfinite(lon)
    if mask is not None:
        ok &= np.asarray(mask, dtype=np.float64).reshape(-1) == 1.0  # (NaN == 1.0 is False: dry)
    return ok


def nearest(lat, lon, gauge_lat, gauge_lon, mask=None):
    """per gauge: (flat index of the nearest valid point or -1, angle in radians or NaN, relative
    gap between the best and the second-best distance -- inf when there is no second point)"""
    ok = valid_points(lat, lon, mask)
    flat = np.nonzero(ok)[0]
    phi2 = np.deg2rad(np.asarray(lat, dtype=np.float64).reshape(-1)[flat])
    lam2 = np.deg2rad(np.asarray(lon, dtype=np.float64).reshape(-1)[flat])
    glat = np.asarray(gauge_lat, dtype=np.float64).reshape(-1)
    glon = np.asarray(gauge_lon, dtype=np.float64).reshape(-1)
    index = np.full(glat.size, -1, dtype=np.int64)
    angle = np.full(glat.size, np.nan)
    gap = np.full(glat.size, np.inf)
    if flat.size == 0:
        return index, angle, gap
    for g in range(glat.size):
        d = haversine(np.deg2rad(glat[g]), np.deg2rad(glon[g]), phi2, lam2)
        if not np.isfinite(d).any():
            continue
        k = int(np.argmin(d))
        index[g], angle[g] = flat[k], d[k]
        if d.size > 1:
            second = np.partition(d, 1)[1]
            gap[g] = (second - d[k]) / second if second > 0 else 0.0
    return index, angle, gap


def locate(lat, lon, gauge_lat, gauge_lon, mask=None, threshold=None, rad_earth=6.378e03):
    """dict of arrays, one entry per kept gauge: which, distance (km), flat_index, mod_index"""
    index, angle, _gap = nearest(lat, lon, gauge_lat, gauge_lon, mask)
    distance = angle * rad_earth
    keep = index >= 0
    if threshold is not None:
        with np.errstate(invalid="ignore"):
            keep &= distance <= threshold
    which = np.nonzero(keep)[0]
    rank = np.cumsum(valid_points(lat, lon, mask)) - 1
    return {"which": which, "distance": distance[which], "flat_index": index[which],
            "mod_index": rank[index[which]]}


_FIXTURE = None


def nwa12():
    """the committed NWA12 fixture (tests/golden/make_tidegauge_golden.py), loaded once:
    (grid dict of arrays, goldens dict)"""
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(os.path.join(GOLDEN, "tidegauge_nwa12.npz")) as z:
            grid = {k: z[k] for k in z.files}
        with open(os.path.join(GOLDEN, "tidegauge_goldens.json")) as f:
            _FIXTURE = (grid, json.load(f))
    return _FIXTURE


def synthetic_grid(ny, nx, ngauges, seed):
    """a jittered global grid whose longitudes run -300 .. 60, about 30 % land, and gauges in
    -180 .. 180 / -80 .. 80: (lat (ny, nx), lon (ny, nx), mask (ny, nx) float64, glat, glon)"""
    rng = np.random.default_rng(seed)
    lat1 = np.linspace(-85.0, 85.0, ny)
    lon1 = np.linspace(-300.0, 60.0, nx, endpoint=False)
    lon, lat = np.meshgrid(lon1, lat1)
    lat = lat + rng.uniform(-0.3, 0.3, lat.shape) * (170.0 / max(ny, 2))
    lon = lon + rng.uniform(-0.3, 0.3, lon.shape) * (360.0 / nx)
    mask = (rng.uniform(size=lat.shape) > 0.3).astype(np.float64)
    glat = rng.uniform(-80.0, 80.0, ngauges)
    glon = rng.uniform(-180.0, 180.0, ngauges)
    return lat, lon, mask, glat, glon


# ---- the integer lattice: search tables whose argmin is exact --------------------------------------
# Every position is x = q / 4 with an integer 0 <= q < 4 * 2^12 on the first axis (y = z = 0, phi =
# lam = 0).  Differences are multiples of 0.25 below 2^12, squares multiples of 2^-4 below 2^24: the
# float64 chord^2 of every pair is exact, so the expected winner is integer arithmetic on q.
LATTICE_LIMIT = 4 << 12
LATTICE_EDGES = (0, 255, 256)  # and n - 1: valid in one variant, invalid in the other


def lattice_points(n, kind, edges_valid, seed=5):
    """(q (n) int64, ok (n) bool): kind "U" -- x is a permutation of 0 .. n-1, each value once;
    kind "D" -- x = perm // 2, each value twice at unrelated indices.  About 10 % of the points are
    invalid; the first, the last and both sides of index 256 are all valid or all invalid."""
    rng = np.random.default_rng([seed, n, int(kind == "D")])
    perm = rng.permutation(n).astype(np.int64)
    x = perm if kind == "U" else perm // 2
    ok = rng.random(n) >= 0.1
    ok[[i for i in LATTICE_EDGES + (n - 1,) if i < n]] = edges_valid
    return 4 * x, ok


def lattice_gauges(n, kind):
    """(q (ng) int64, ok (ng) bool): a gauge on every value v of the points' table -- for "D" also
    v + 0.5 (a four-way tie across two values) and v + 0.25 -- and three invalid gauges (first,
    middle, last)."""
    if kind == "U":
        q = 4 * np.arange(n, dtype=np.int64)
    else:
        q = (4 * np.arange((n + 1) // 2, dtype=np.int64)[:, None] + np.array([0, 2, 1])).reshape(-1)
    ok = np.ones(q.size + 3, dtype=bool)
    ok[[0, (q.size + 3) // 2, q.size + 2]] = False
    full = np.zeros(ok.size, dtype=np.int64)
    full[ok] = q
    return full, ok


def lattice_table(q, ok):
    """the (5, n) float64 table of mlx_gauge_prepare's layout for the lattice positions q / 4; an
    invalid column in the prepare kernel's own encoding: x = y = z = +inf, phi = lam = NaN"""
    assert q.min() >= 0 and q.max() < LATTICE_LIMIT
    table = np.zeros((_lib.GAUGE_ROWS, q.size))
    table[_lib.GAUGE_ROW_X] = q / 4.0
    assert np.array_equal(table[_lib.GAUGE_ROW_X] * 4.0, q)
    bad = ~ok
    for row in (_lib.GAUGE_ROW_X, _lib.GAUGE_ROW_Y, _lib.GAUGE_ROW_Z):
        table[row, bad] = np.inf
    table[_lib.GAUGE_ROW_PHI, bad] = table[_lib.GAUGE_ROW_LAM, bad] = np.nan
    return table


def lattice_nearest(pq, pok, gq, gok):
    """per gauge the valid point minimising (|gq - pq|, flat index), -1 for an invalid gauge or when
    no point is valid -- int64 arithmetic only"""
    n = pq.size
    flat = np.nonzero(pok)[0]
    index = np.full(gq.size, -1, dtype=np.int64)
    if flat.size == 0:
        return index
    for g0 in range(0, gq.size, 512):
        key = np.abs(gq[g0:g0 + 512, None] - pq[None, flat]) * n + flat[None, :]  # (distinct keys)
        index[g0:g0 + 512] = flat[np.argmin(key, axis=1)]
    index[~gok] = -1
    return index


# ---- copies of one row: which copy wins is the tie rule alone --------------------------------------
TIE_SETS = ((16, 1), (17, 16), (0, 16), (19, 3, 18), (15, 16))
TIE_SETS_40 = ((32, 17), (33, 16, 2))
TIE_DRY_COLUMN = 10


def stacked_rows(copies, m=70):
    """one row of m distinct points stacked ``copies`` times -- flat index = copy * m + column --
    and a mask that leaves chosen copies of each column wet: (lat, lon, mask, wet) with wet[c] the
    tuple of wet copies of column c.  The sets cycle over the columns; one of them is the last copy
    alone, and column TIE_DRY_COLUMN is dry in every copy."""
    row_lat, row_lon = np.linspace(-60.0, 60.0, m), np.linspace(-170.0, 170.0, m)
    sets = list(TIE_SETS) + (list(TIE_SETS_40) if copies >= 40 else []) + [(copies - 1,)]
    assert all(max(s) < copies for s in sets)
    wet = [sets[c % len(sets)] for c in range(m)]
    wet[TIE_DRY_COLUMN] = ()
    mask = np.zeros((copies, m))
    for c, s in enumerate(wet):
        mask[list(s), c] = 1.0
    return np.tile(row_lat, (copies, 1)), np.tile(row_lon, (copies, 1)), mask, wet


# ---- far and opposite ------------------------------------------------------------------------------
ANTIPODE_LON = 37.0


def antipodes(step=0.25, lon=ANTIPODE_LON):
    """(lat, lon, gauge lat, gauge lon): latitudes -90 .. 90 every ``step`` degrees at one longitude
    and the antipode (-lat, lon + 180) of each"""
    k = int(round(90.0 / step))
    lat = np.arange(-k, k + 1) * step
    return lat, np.full(lat.size, lon), -lat, np.full(lat.size, lon + 180.0)


def haversine_h(phi1, lam1, phi2, lam2):
    """the argument of the square root in ``haversine``: above 1 by rounding for some antipodes"""
    s0 = np.sin(0.5 * (phi1 - phi2))
    s1 = np.sin(0.5 * (lam1 - lam2))
    return s0 * s0 + np.cos(phi1) * np.cos(phi2) * s1 * s1
