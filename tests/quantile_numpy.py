"""The contract of include/momlevel_quantile.h restated in numpy: numpy.sort per column, then the
lerp of numpy 2.2's ``method="linear"`` spelled out.  No radix select, no partition: a different
route to the same order statistics than the kernel takes.

    c  = number of non-NaN listed steps        (c == 0: NaN)
    vi = (c - 1) * q
    vi >= c - 1: lo = hi = c - 1, prev = -1;   vi < 0: lo = hi = 0, prev = 0;
    else lo = floor(vi), hi = lo + 1, prev = lo
    g = vi - prev;  a, b = sorted[lo], sorted[hi];  d = b - a
    r = a + d * g;  g >= 0.5: r = b - d * (1 - g)

Everything runs in float64 whatever the record's dtype (float32 widens exactly); ``rounded_once``
gives what a float32 record's result must be.
"""

import numpy as np


def group_quantile(rows, q):
    """the quantile ``q`` of every column of ``rows`` (m, n) over its non-NaN values -> (n,) float64"""
    rows = np.asarray(rows, dtype=np.float64)
    m, n = rows.shape
    if m == 0:
        return np.full(n, np.nan)
    s = np.sort(rows, axis=0)  # NaN goes last
    c = np.sum(~np.isnan(rows), axis=0)
    top = (np.maximum(c, 1) - 1).astype(np.float64)
    vi = top * np.float64(q)
    above, below = vi >= top, vi < 0.0
    prev = np.floor(vi)
    lo, hi = prev.copy(), prev + 1.0
    lo[above] = hi[above] = top[above]
    prev[above] = -1.0
    lo[below] = hi[below] = prev[below] = 0.0
    g = vi - prev
    a = np.take_along_axis(s, lo.astype(np.int64)[None, :], axis=0)[0]
    b = np.take_along_axis(s, hi.astype(np.int64)[None, :], axis=0)[0]
    with np.errstate(invalid="ignore"):
        d = b - a
        r = a + d * g
        r = np.where(g >= 0.5, b - d * (1.0 - g), r)
    r[c == 0] = np.nan
    return r


def _members(nt, steps, offsets):
    if steps is None:
        return [np.arange(nt)]
    steps, offsets = np.asarray(steps), np.asarray(offsets)
    return [steps[offsets[g]:offsets[g + 1]] for g in range(offsets.size - 1)]


def time_quantile(y, q, steps=None, offsets=None):
    """(nq, ngroups, n) float64: every level of ``q`` over every group of rows of y (nt, n)"""
    y = np.asarray(y)
    y = y.reshape(y.shape[0], -1).astype(np.float64)
    levels = np.atleast_1d(np.asarray(q, dtype=np.float64))
    groups = _members(y.shape[0], steps, offsets)
    out = np.empty((levels.size, len(groups), y.shape[1]))
    for gi, sel in enumerate(groups):
        rows = y[sel]
        for qi, level in enumerate(levels):
            out[qi, gi] = group_quantile(rows, level)
    return out


def rounded_once(res):
    """a float32 record's result: the float64 result rounded once"""
    return np.asarray(res, dtype=np.float64).astype(np.float32)


def exceed_count(y, thr, steps=None, offsets=None):
    """(ngroups, n) int64: the steps of every group with y > thr (strict, in float64)"""
    y = np.asarray(y)
    y = y.reshape(y.shape[0], -1).astype(np.float64)
    groups = _members(y.shape[0], steps, offsets)
    thr = np.asarray(thr, dtype=np.float64).reshape(len(groups), -1)
    with np.errstate(invalid="ignore"):
        return np.stack([np.sum(y[sel] > thr[gi][None, :], axis=0, dtype=np.int64)
                         for gi, sel in enumerate(groups)])


def values_equal(got, want):
    """value identity: NaN where NaN, equal elsewhere (+0.0 == -0.0)"""
    return np.array_equal(np.asarray(got), np.asarray(want), equal_nan=True)


def assert_values(got, want, what=""):
    """value identity on every cell, and bit identity wherever the result is neither NaN nor zero"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, \
        f"{what}: {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    if not values_equal(got, want):
        bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ, first at {i}: "
                             f"{got[i]!r} against {want[i]!r}")
    plain = ~np.isnan(want) & (want != 0)
    kind = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    assert np.array_equal(np.ascontiguousarray(got)[plain].view(kind),
                          np.ascontiguousarray(want)[plain].view(kind)), f"{what}: bits differ"
