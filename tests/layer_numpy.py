"""The numpy restatement of core.layer_integral / derived.calc_layer_integral, and nothing more.
It is the ONLY yardstick of these functions: they are an extension -- in the reference the sum is
spelled ``(calc_dz(levels, interfaces, depth, top=top, bottom=bottom) * x).sum("z_l")`` with
xarray, which is not importable where the tests run.  calc_dz's arithmetic is written out from the
reference's derived.py:295-318 (fraction=False); the sum over z is an explicit loop from +0.0.
It does not call momlevel_amd."""

import numpy as np


def layer_dz(z_i, depth, top, bottom):
    """calc_dz(top=top, bottom=bottom) -> (nz, ...) for ``depth`` (...); ``bottom`` None or +inf:
    no bottom (np.minimum(depth, inf) == depth)"""
    z_i = np.asarray(z_i, dtype=np.float64)
    depth = np.where(np.isnan(depth), 0.0, np.asarray(depth, dtype=np.float64))  # fillna(0.0)
    if bottom is not None:
        depth = np.minimum(depth, np.float64(bottom))
    shape = (z_i.size - 1,) + (1,) * depth.ndim
    ztop, zbot = z_i[:-1].reshape(shape), z_i[1:].reshape(shape)
    dz_field = zbot - ztop
    part = depth[None] - ztop
    part = np.where(part < 0.0, 0.0, part)
    result = np.minimum(part, dz_field)
    part = zbot - np.float64(top)
    part = np.where(part < 0.0, 0.0, part)
    return np.minimum(part, result)


def layer_integral(x, z_i, depth, tops, bottoms, surface=None, scale=1.0):
    """``out[r, l, c]`` for ``x`` (nrec, nz, ...), ``depth`` (...): float64 (nrec, nl, ...)"""
    x64 = np.asarray(x).astype(np.float64)  # exact for float32
    nrec, nz = x64.shape[:2]
    out = np.empty((nrec, len(tops)) + x64.shape[2:], dtype=np.float64)
    for l, (top, bottom) in enumerate(zip(tops, bottoms)):
        w = layer_dz(z_i, depth, top, bottom)
        acc = np.zeros((nrec,) + x64.shape[2:], dtype=np.float64)  # +0.0
        for z in range(nz):  # z ascending
            with np.errstate(invalid="ignore", over="ignore"):
                term = w[z][None] * x64[:, z]  # one IEEE multiply
            acc = np.where(np.isnan(term), acc, acc + np.where(np.isnan(term), 0.0, term))  # skipna
        with np.errstate(invalid="ignore", over="ignore"):
            out[:, l] = np.float64(scale) * acc
    if surface is not None:
        out[:, :, np.isnan(surface)] = np.nan
    return out


def abs_sum(x, z_i, depth, top=0.0, bottom=None):
    """sum_z |dz * x| per (record, cell), NaN terms skipped: the scale of the rounding bounds"""
    w = layer_dz(z_i, depth, top, bottom)
    with np.errstate(invalid="ignore", over="ignore"):
        term = np.abs(w[None] * np.asarray(x).astype(np.float64))
    return np.where(np.isnan(term), 0.0, term).sum(axis=1)
