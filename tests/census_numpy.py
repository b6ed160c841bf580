"""The census of include/momlevel_census.h restated in numpy: mask, ``searchsorted`` and
``numpy.add.at`` on float64 and int64 arrays.  It is ``numpy.histogramdd`` with explicit edges
(tests/test_census_host.py holds it against numpy's own) with ONE difference: a cell whose weight or
value is NaN is masked out first -- numpy would add the NaN and poison the bin.

    fields   one or two (nrec, ncells) arrays, float32 or float64
    edges    one strictly increasing float64 array of n_d + 1 edges per field
    weights  None, (ncells,) or (nrec, ncells);  values  None or (nrec, ncells)

``np.add.at`` adds in ascending cell order; the kernel adds in another fixed order, so float sums
agree inside the summation-order bound and exactly when every partial sum is an integer below 2^53.
"""

import numpy as np


def bin_index(e, f, closed=True):
    """(index, inside): ``searchsorted(e, f, side="right") - 1`` on the exactly widened values, a
    value equal to the last edge in the last bin when ``closed``; ``inside`` is False below the
    first edge, above the last, for +-inf outside the edges and for NaN (numpy sorts it last)."""
    e = np.asarray(e, dtype=np.float64)
    f = np.asarray(f).astype(np.float64)
    n = e.size - 1
    i = np.searchsorted(e, f, side="right") - 1
    if closed:
        i = np.where(f == e[-1], n - 1, i)
    inside = (i >= 0) & (i < n)
    return np.where(inside, i, 0), inside


def census(fields, edges, weights=None, values=None, closed=3):
    """(count, wsum, vsum): (nrec,) + table arrays, int64 and float64; wsum / vsum None without
    weights / values.  ``closed``: bit d set when field d's last edge is closed (a whole table: 3)."""
    fields = [np.asarray(f) for f in fields]
    nrec, ncells = fields[0].shape
    shape = tuple(np.asarray(e).size - 1 for e in edges)
    nbins = int(np.prod(shape))
    count = np.zeros((nrec, nbins), dtype=np.int64)
    wsum = None if weights is None else np.zeros((nrec, nbins), dtype=np.float64)
    vsum = None if values is None else np.zeros((nrec, nbins), dtype=np.float64)
    for r in range(nrec):
        flat = np.zeros(ncells, dtype=np.int64)
        valid = np.ones(ncells, dtype=bool)
        for d, (f, e) in enumerate(zip(fields, edges)):
            i, inside = bin_index(e, f[r], bool(closed & (1 << d)))
            flat = flat * shape[d] + i
            valid &= inside
        if weights is not None:
            w = np.asarray(weights)
            w = (w[r] if w.ndim == 2 else w).astype(np.float64)
            valid &= ~np.isnan(w)
        if values is not None:
            v = np.asarray(values)[r].astype(np.float64)
            valid &= ~np.isnan(v)
        np.add.at(count[r], flat[valid], 1)
        if weights is not None:
            np.add.at(wsum[r], flat[valid], w[valid])
        if values is not None:
            np.add.at(vsum[r], flat[valid], w[valid] * v[valid])  # one rounding per product
    full = (nrec,) + shape
    return (count.reshape(full), None if wsum is None else wsum.reshape(full),
            None if vsum is None else vsum.reshape(full))


def abs_sums(fields, edges, weights, values=None, closed=3):
    """sum |w| and sum |w * v| per bin: the scales of the gate |sum - ref| <= 1e-10 * scale"""
    w = np.abs(np.asarray(weights, dtype=np.float64))
    _, sw, sv = census(fields, edges, w, None if values is None else
                       np.abs(np.asarray(values, dtype=np.float64)), closed)
    return sw, sv


def left_out(fields, edges, weights=None, values=None):
    """cells per record that the census leaves out"""
    count, _, _ = census(fields, edges, weights, values)
    ncells = np.asarray(fields[0]).shape[1]
    return ncells - count.reshape(count.shape[0], -1).sum(axis=1)
