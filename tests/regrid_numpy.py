"""The arithmetic contract of include/momlevel_regrid.h restated in numpy: a plain loop over
destinations and entries, the records of a destination carried side by side (elementwise float64
operations: the same IEEE operations a scalar loop performs).  Test infrastructure -- the
specification the kernel (csrc/momlevel_regrid.hip) is held to bit for bit -- and not part of the
product; it shares no code with momlevel_amd/regrid.py.

Two front ends over one row rule: ``apply_csr`` takes the table as rows (indptr, col, S), ``apply_packed``
as the device reads it (slice_ptr, len, col, S in slices of ``L`` rows, entry k of destination
d = s*L + lane at slice_ptr[s] + k*L + lane), so that tables no builder makes -- a col outside the
plane, a len that runs past the table -- have a stated result too."""

import numpy as np

PROPAGATE, NO_RENORM = 1, 2
NAN64 = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
NAN32 = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]


def _row(v, entries, nsrc, min_frac, flags, length):
    """one destination, every record: ``length`` is len[d], ``entries`` the list of (col, S) of the
    row's entries that lie inside the table, k ascending (an entry outside it carries no weight:
    adding +0.0 to a sum that started at +0.0 changes no bit) -> (nrec,) float64"""
    nrec = v.shape[0]
    nan = np.full(nrec, NAN64)
    if length <= 0:
        return nan
    num, den = np.zeros(nrec), np.zeros(nrec)
    cnt = np.zeros(nrec, dtype=np.int64)
    tot = np.float64(0.0)
    zero = np.zeros(nrec)
    for c, w in entries:
        in_range = 0 <= c < nsrc
        if not in_range:
            tot = tot + np.float64(0.0)
            num, den = num + zero, den + zero
            continue
        w = np.float64(w)
        x = v[:, c].astype(np.float64)  # exact
        tot = tot + w
        with np.errstate(invalid="ignore", over="ignore"):
            p = w * x
        if flags & PROPAGATE:
            num = num + p
        else:
            valid = ~np.isnan(x)
            num = num + np.where(valid, p, 0.0)
            den = den + np.where(valid, w, 0.0)
            cnt = cnt + valid
    if flags & PROPAGATE:
        res = num
    else:
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            res = num if flags & NO_RENORM else num / den
            res = np.where((cnt == 0) | (den < np.float64(min_frac) * tot), NAN64, res)
    return np.where(np.isnan(res), NAN64, res)


def _store(rows, out_dtype):
    out = np.stack(rows, axis=1) if rows else np.zeros((0, 0))
    if np.dtype(out_dtype) == np.float32:
        with np.errstate(over="ignore"):
            narrow = out.astype(np.float32)  # rounded once
        return np.where(np.isnan(out), NAN32, narrow)
    return out


def apply_csr(v, indptr, col, S, ndst, min_frac=0.0, flags=0, out_dtype=None):
    """``v`` (nrec, nsrc); row d of the table is entries indptr[d] .. indptr[d+1] - 1"""
    v = np.asarray(v)
    nrec, nsrc = v.shape
    rows = []
    for d in range(ndst):
        entries = [(int(col[e]), S[e]) for e in range(int(indptr[d]), int(indptr[d + 1]))]
        rows.append(_row(v, entries, nsrc, min_frac, flags, len(entries)))
    out = _store(rows, out_dtype or v.dtype)
    return out.reshape(nrec, ndst)


def apply_packed(v, slice_ptr, length, col, S, ndst, L, min_frac=0.0, flags=0, out_dtype=None):
    """the table as the device reads it; ``len(col)`` is nentries"""
    v = np.asarray(v)
    nrec, nsrc = v.shape
    nentries = len(col)
    rows = []
    for d in range(ndst):
        s, lane = divmod(d, L)
        p0 = int(slice_ptr[s])
        entries = []
        for k in range(max(int(length[d]), 0)):
            p = p0 + k * L + lane
            if not (0 <= p0 < nentries and p < nentries):
                break  # (positions ascend: every later entry lies outside the table too)
            entries.append((int(col[p]), S[p]))
        rows.append(_row(v, entries, nsrc, min_frac, flags, int(length[d])))
    out = _store(rows, out_dtype or v.dtype)
    return out.reshape(nrec, ndst)


def unpack(slice_ptr, length, col, S, ndst, L):
    """the packed table back as rows: (indptr, col, S)"""
    indptr = np.zeros(ndst + 1, dtype=np.int64)
    cols, vals = [], []
    for d in range(ndst):
        s, lane = divmod(d, L)
        for k in range(int(length[d])):
            p = int(slice_ptr[s]) + k * L + lane
            cols.append(int(col[p]))
            vals.append(float(S[p]))
        indptr[d + 1] = len(cols)
    return indptr, np.array(cols, dtype=np.int32), np.array(vals, dtype=np.float64)
