"""The numpy restatement of include/momlevel_smooth.h: the specification the kernels of
csrc/momlevel_smooth.hip are gated against bit for bit.  A test helper, not part of the product.

Vectorised over cells, with Python loops over the taps k and l only: numpy's elementwise ``*`` and
``+`` are one IEEE operation each, in the order written here.  Adding 0.0 for a term that is not
valid gives the bits of skipping it, since the accumulators start at +0.0 and so never hold -0.0.
"""

import numpy as np

NAN64 = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


def _canonical(x):
    return np.where(np.isnan(x), NAN64, x)


def row_pass(v, area, wx, lead_x, periodic_x):
    """(Rn, Rd, Rc) of every (rec, r, i): float64, float64, int64"""
    v64 = np.asarray(v).astype(np.float64)
    a64 = np.asarray(area).astype(np.float64)
    nrec, ny, nx = v64.shape
    wx = np.asarray(wx, dtype=np.float64)
    table = wx.ndim == 2
    Wx = wx.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        valid = ~np.isnan(v64) & ~np.isnan(a64)[None] & (a64 > 0)[None]
        m = a64[None] * v64
        a3 = np.broadcast_to(a64[None], v64.shape)
        Rn = np.zeros(v64.shape)
        Rd = np.zeros(v64.shape)
        Rc = np.zeros(v64.shape, dtype=np.int64)
        cols = np.arange(nx)
        for k in range(Wx):
            c = cols - lead_x + k
            inside = np.ones(nx, dtype=bool) if periodic_x else (c >= 0) & (c < nx)
            c = c % nx
            ok = valid[:, :, c] & inside[None, None, :]
            X = wx[:, k][None, :, None] if table else wx[k]
            Rn = Rn + np.where(ok, X * m[:, :, c], 0.0)
            Rd = Rd + np.where(ok, X * a3[:, :, c], 0.0)
            Rc = Rc + ok
    return Rn, Rd, Rc


def plane_smooth(v, area, wx, wy, lead_x, lead_y, periodic_x, min_count, fill=False, residual=False,
                 out_dtype=None):
    """The contract of mlx_smooth_apply for ``v`` (nrec, ny, nx): float64, or the float64 result
    rounded once to ``out_dtype``"""
    v = np.asarray(v)
    area = np.asarray(area)
    v64 = v.astype(np.float64)
    a64 = area.astype(np.float64)
    nrec, ny, nx = v64.shape
    wy = np.asarray(wy, dtype=np.float64)
    Wy = wy.shape[0]
    Rn, Rd, Rc = row_pass(v, area, wx, lead_x, periodic_x)
    num = np.zeros(v64.shape)
    den = np.zeros(v64.shape)
    cnt = np.zeros(v64.shape, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for l in range(Wy):  # noqa: E741
            # output rows j whose source row j - lead_y + l lies in the plane
            j0, j1 = max(0, lead_y - l), min(ny, ny + lead_y - l)
            if j0 >= j1:
                continue
            r0, r1 = j0 - lead_y + l, j1 - lead_y + l
            num[:, j0:j1] = num[:, j0:j1] + wy[l] * Rn[:, r0:r1]
            den[:, j0:j1] = den[:, j0:j1] + wy[l] * Rd[:, r0:r1]
            cnt[:, j0:j1] = cnt[:, j0:j1] + Rc[:, r0:r1]
        smooth = num / den
        centre = ~np.isnan(v64) & ~np.isnan(a64)[None] & (a64 > 0)[None]
        res = np.where(centre, v64 - smooth, NAN64) if residual else smooth
        drop = cnt < min_count
        if not fill:
            drop = drop | ~centre
        res = _canonical(np.where(drop, NAN64, res))
    if out_dtype is not None and np.dtype(out_dtype) == np.float32:
        with np.errstate(over="ignore"):
            res = res.astype(np.float32)
        res = np.where(np.isnan(res), np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0], res)
    return res


def direct_2d(v, area, wx, wy, lead_x, lead_y, periodic_x):
    """The same filter as ONE non-separable 2-D normalised convolution, cell by cell in Python:
    sum_{l,k} wy[l] wx[r,k] a v / sum_{l,k} wy[l] wx[r,k] a over the valid cells.  Another order of
    summation: agrees with plane_smooth to rounding, not to the bit."""
    v64 = np.asarray(v, dtype=np.float64)
    a64 = np.asarray(area, dtype=np.float64)
    ny, nx = v64.shape
    wx = np.asarray(wx, dtype=np.float64)
    wy = np.asarray(wy, dtype=np.float64)
    out = np.full((ny, nx), np.nan)
    for j in range(ny):
        for i in range(nx):
            num = den = 0.0
            for l in range(wy.size):  # noqa: E741
                r = j - lead_y + l
                if not 0 <= r < ny:
                    continue
                X = wx[r] if wx.ndim == 2 else wx
                for k in range(X.size):
                    c = i - lead_x + k
                    if periodic_x:
                        c %= nx
                    elif not 0 <= c < nx:
                        continue
                    if np.isnan(v64[r, c]) or np.isnan(a64[r, c]) or not a64[r, c] > 0:
                        continue
                    num += wy[l] * X[k] * a64[r, c] * v64[r, c]
                    den += wy[l] * X[k] * a64[r, c]
            if den != 0.0:
                out[j, i] = num / den
    return out
