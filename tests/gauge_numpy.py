"""numpy restatement of util.geolocate_points (src/momlevel/util.py:252-367) without scikit-learn:
the haversine distance of BallTree(metric="haversine") by brute force, numpy's argmin (lowest index
on a tie), the ``mask == 1.0`` filter, the ``<=`` threshold and ``mod_index``, the rank of the
chosen point among the valid ones.  Shared by tests/test_tidegauge_host.py and
tests/test_gpu_tidegauge.py; a test helper, not part of the product."""

import json
import os

import numpy as np

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
