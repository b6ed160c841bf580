"""The numpy restatement of momlevel_amd.eof and of mlx_gram_matrix (include/momlevel_eof.h): the
specification the kernels and the module are gated against.  xarray's ``eofs`` package is not
importable where the tests run, so parity with it is unpinned."""

import numpy as np

F64 = np.float64


def weighted(y, center=None, scale=None, other_center=None):
    """b[s, c] = where(ok, (y[s, c] - center[c]) * scale[c], 0): two IEEE roundings per element"""
    y = np.asarray(y, dtype=F64)
    y = y.reshape(y.shape[0], -1)
    n = y.shape[1]
    cen = np.zeros(n) if center is None else np.asarray(center, dtype=F64).reshape(-1)
    scl = np.ones(n) if scale is None else np.asarray(scale, dtype=F64).reshape(-1)
    ok = ~np.isnan(cen) & ~np.isnan(scl)
    if other_center is not None:
        ok &= ~np.isnan(np.asarray(other_center, dtype=F64).reshape(-1))
    with np.errstate(invalid="ignore", over="ignore"):
        b = (y - cen[None, :]) * scl[None, :]
    return np.where(ok[None, :], b, 0.0)


def time_gram(y1, y2=None, center1=None, center2=None, scale=None):
    """G[s, t] = sum_c b1[s, c] * b2[t, c]; ``y2`` None: b2 = b1"""
    b1 = weighted(y1, center1, scale, None if y2 is None else center2)
    b2 = b1 if y2 is None else weighted(y2, center2, scale, center1)
    with np.errstate(invalid="ignore"):
        return b1 @ b2.T


def cell_maps(y, areacello=None):
    """(center, scale): the per-cell time mean (NaN where any step is missing) and sqrt(area)
    (NaN where the area is NaN or not positive; ones without an area)"""
    y = np.asarray(y, dtype=F64)
    nt = y.shape[0]
    flat = y.reshape(nt, -1)
    center = (flat * (1.0 / nt)).sum(axis=0)  # (NaN where any step is missing)
    if areacello is None:
        scale = np.ones(flat.shape[1])
    else:
        area = np.asarray(areacello, dtype=F64).reshape(-1)
        with np.errstate(invalid="ignore"):
            scale = np.where(area > 0, np.sqrt(np.where(area > 0, area, 1.0)), np.nan)
    return center, scale


def time_covariance(y, areacello=None, ddof=1):
    y = np.asarray(y, dtype=F64)
    center, scale = cell_maps(y, areacello)
    return time_gram(y, None, center, None, scale) / (y.shape[0] - ddof)


def fix_signs(pcs):
    """each column's element of largest magnitude positive, the lowest index on ties"""
    pcs = np.array(pcs, dtype=F64)
    for k in range(pcs.shape[1]):
        if pcs[np.argmax(np.abs(pcs[:, k])), k] < 0:
            pcs[:, k] = -pcs[:, k]
    return pcs


def calc_eofs(y, areacello=None, neofs=4, ddof=1):
    """dict of eigenvalues (neofs), variance_fraction, eigenvalue_error, pcs (nt, neofs) and eofs
    (neofs, ...): see momlevel_amd.eof.calc_eofs"""
    y = np.asarray(y, dtype=F64)
    nt = y.shape[0]
    if not 1 <= neofs <= nt - 1:
        raise ValueError("neofs must be 1 .. nt - 1")
    cov = time_covariance(y, areacello, ddof)
    lam, vec = np.linalg.eigh(cov)
    lam, vec = lam[::-1], vec[:, ::-1]
    pcs = fix_signs(vec[:, :neofs] * np.sqrt(nt - ddof))
    center, _ = cell_maps(y)
    anom = y.reshape(nt, -1) - center[None, :]
    eofs = (pcs.T @ anom) / (nt - ddof)
    return {
        "eigenvalues": lam[:neofs].copy(),
        "variance_fraction": lam[:neofs] / np.trace(cov),
        "eigenvalue_error": lam[:neofs] * np.sqrt(2.0 / nt),
        "pcs": pcs,
        "eofs": eofs.reshape((neofs,) + y.shape[1:]),
    }


def project_field(y, eofs, areacello=None, center=None):
    """pseudo-PCs (nt, mode): sum_c area (y - center) E_k / sum_c area E_k^2 over the cells where the
    maps, the area and the center are not NaN; ``center`` None is the record's own time mean"""
    y = np.asarray(y, dtype=F64)
    eofs = np.asarray(eofs, dtype=F64)
    nt, nmode = y.shape[0], eofs.shape[0]
    own, scale = cell_maps(y, areacello)
    cen = own if center is None else np.asarray(center, dtype=F64).reshape(-1)
    land = np.where(np.isnan(eofs.reshape(nmode, -1)).any(axis=0), np.nan, 0.0)
    num = time_gram(y, eofs, cen, land, scale)
    ok = ~np.isnan(cen)
    den = time_gram(eofs, None, np.where(ok, land, np.nan), None, scale)
    return num / np.diag(den)[None, :]
