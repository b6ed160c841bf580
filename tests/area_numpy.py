"""The numpy restatement of regional.area_mean / area_anomaly, and nothing more.  It is the ONLY
yardstick of these functions: they are an extension -- the reference has no counterpart, so there
is no golden from it (in xarray: ``xobj.weighted(areacello.fillna(0)).mean((ydim, xdim))``, which
is not importable where the tests run)."""

import numpy as np


def area_mean(v, area, label=None, ids=None):
    """``(mean, den)`` of ``v`` (..., ny, nx) over its last two axes, weighted by ``area`` (ny, nx):
    (...) without ``label``, (..., len(ids)) with the integer map ``label`` (ny, nx)."""
    v64, a64 = v.astype(np.float64), area.astype(np.float64)
    regions = [np.ones(area.shape, bool)] if label is None else [label == r for r in ids]
    means, dens = [], []
    for inside in regions:
        valid = ~np.isnan(v) & ~np.isnan(area) & inside
        w = np.where(valid, a64, 0.0)
        den = w.sum(axis=(-2, -1))
        num = (w * np.where(valid, v64, 0.0)).sum(axis=(-2, -1))
        with np.errstate(invalid="ignore", divide="ignore"):
            means.append(num / den)
        dens.append(den)
    if label is None:
        return means[0], dens[0]
    lead = v.shape[:-2]
    return (np.stack(means, axis=-1).reshape(lead + (len(ids),)),
            np.stack(dens, axis=-1).reshape(lead + (len(ids),)))


def area_anomaly(v, mean, label=None, ids=None):
    """``v64 - mean[rec, region(cell)]``, NaN in cells of no region; ``mean`` as area_mean returns it"""
    v64 = v.astype(np.float64)
    if label is None:
        return v64 - mean[..., None, None]
    out = np.full(v.shape, np.nan)
    for k, r in enumerate(ids):
        inside = np.broadcast_to(label == r, v.shape)
        out[inside] = (v64 - mean[..., k][..., None, None])[inside]
    return out
