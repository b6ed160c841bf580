"""The numpy restatement of core.column_crossing ("depth of the first crossing along z") and of what
derived.calc_mld / calc_isosurface_depth / calc_isopycnal_depth make of it, and nothing more.  It is
the ONLY yardstick of these functions: they are an extension, the reference has no counterpart.  The
rule is include/momlevel_column.h's, steps 1 to 6; every operator of the interpolation is one
float64 numpy operation in the header's parenthesisation.  It does not call momlevel_amd.

The SIGMA source is the float64 density of the numpy oracle (oracle/momlevel_numpy.py) on exactly
widened operands, whatever the dtype of theta and S: the header says why."""

import numpy as np

RISE, FALL, DEPART = 0, 1, 2
MISS_NAN, MISS_FLOOR = 0, 1


def sigma(theta, so, p_ref, eos="wright"):
    """x of the SIGMA source: float64 arithmetic on the widened values, one scalar pressure"""
    from oracle import momlevel_numpy as o

    T = np.asarray(theta).astype(np.float64)  # exact for float32
    S = np.asarray(so).astype(np.float64)
    with np.errstate(all="ignore"):
        if eos.lower() == "linear":
            return o.linear_density(T, S)
        return o.wright_density(T, S, float(p_ref))


def _hit(x, xref, tgt, v, mode):
    """(is x a hit, the target the interpolation aims at)"""
    with np.errstate(invalid="ignore"):
        if mode == RISE:
            return x >= tgt, tgt
        if mode == FALL:
            return x <= tgt, tgt
        return np.abs(x - xref) >= v, np.where(x > xref, xref + v, xref - v)


def column_crossing(x, z, kref, mode, relative, miss, targets, floor=None):
    """``out[r, j, c]`` for ``x`` (nrec, nz, plane) -- float32 is widened exactly -- level depths
    ``z`` (nz), ``targets`` (nt) and ``floor`` None or (plane): float64 (nrec, nt, plane)"""
    x = np.asarray(x).astype(np.float64)
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    targets = np.asarray(targets, dtype=np.float64).reshape(-1)
    nrec, nz, plane = x.shape
    assert z.size == nz and np.all(np.diff(z) > 0) and 0 <= kref < nz
    assert mode in (RISE, FALL, DEPART) and (relative or mode != DEPART)
    assert not np.isnan(targets).any() and (not relative or np.all(targets > 0))
    out = np.full((nrec, targets.size, plane), np.nan)
    land = np.isnan(x[:, 0])  # 1.
    xref = x[:, kref]
    shallow = np.isnan(xref) & ~land  # 2.
    # klast of a column whose scan never began: the deepest level above kref with no NaN at or above it
    zlast = np.full((nrec, plane), np.nan)
    run = ~land
    for k in range(kref):
        run = run & ~np.isnan(x[:, k])
        zlast = np.where(run, z[k], zlast)
    zlast = np.where(shallow, zlast, np.nan)
    # ... and of a column that is scanned: the last level before the first NaN below kref
    scanning = ~land & ~shallow
    alive = scanning.copy()
    for k in range(kref, nz):
        alive = alive & ~np.isnan(x[:, k])
        zlast = np.where(alive, z[k], zlast)
    for j, v in enumerate(targets):
        with np.errstate(invalid="ignore"):
            tgt = (xref + v if mode == RISE else xref - v) if relative else np.full_like(xref, v)
        hit0, _ = _hit(xref, xref, tgt, v, mode)
        res = np.full((nrec, plane), np.nan)
        open_ = scanning & ~hit0  # 4. an outcrop stays NaN
        alive = open_.copy()  # ... and still above the sea floor
        for k in range(kref, nz - 1):  # 5.
            x0, x1 = x[:, k], x[:, k + 1]
            alive = alive & ~np.isnan(x1)
            hit, t = _hit(x1, xref, tgt, v, mode)
            first = alive & hit
            with np.errstate(all="ignore"):
                depth = z[k] + ((t - x0) / (x1 - x0)) * (z[k + 1] - z[k])
            res = np.where(first, depth, res)
            alive = alive & ~first
            open_ = open_ & ~first
        missed = open_ | shallow  # 6.
        if miss == MISS_FLOOR:
            m = zlast if floor is None else np.broadcast_to(np.asarray(floor, np.float64), res.shape)
            res = np.where(missed, m, res)
        out[:, j] = res
    return out


def nearest_level(z, ref_depth):
    """the level nearest ``ref_depth``, ties to the shallower"""
    return int(np.argmin(np.abs(np.asarray(z, dtype=np.float64) - float(ref_depth))))
