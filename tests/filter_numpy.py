"""The numpy restatement of the time filter (include/momlevel_filter.h, momlevel_amd.filters): the
arithmetic contract as a loop over the output steps t and the taps k, whole rows of cells at a time.

    out[t] = sum_k w[t, k] * y[t - lead + k],   k = 0 .. W-1 ascending

A step is valid when it lies inside [0, nt) and is not NaN.  acc starts at -0.0, wsum and cnt at 0;
each tap adds ``where(valid, w[k] * y, 0.0)`` (the product rounded, then the add), ``where(valid,
w[k], 0.0)`` and ``valid``; the result is NaN where cnt < min_count, else acc / wsum (normalised)
or acc.  float32 records are widened first; a float32 result is ``.astype(float32)`` of this one.

With weights of 1 and ``normalise`` this is bit-identical to ``numpy.nanmean(y[lo:hi], axis=0)``
masked by the valid count (``rolling_mean_nanmean`` below; checked in tests/test_filter_host.py).

``time_filter_taps`` is the same contract for records of 10^5 steps, where the loop over nt x W
takes tens of seconds: a loop over the W taps alone, each applied to the whole record shifted.  It
is held to ``time_filter`` bit for bit in tests/test_filter_host.py.
"""

import warnings

import numpy as np


def time_filter(y, w, lead, min_count=None, normalise=False):
    """float64 (nt, ...) result of the contract; ``w`` (W,) or (nt, W)"""
    y64 = np.asarray(y).astype(np.float64)
    nt = y64.shape[0]
    w = np.asarray(w, dtype=np.float64)
    W = w.shape[-1]
    min_count = W if min_count is None else int(min_count)
    assert 1 <= W <= nt and 0 <= lead < W and 1 <= min_count <= W
    cells = y64.shape[1:]
    out = np.empty_like(y64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for t in range(nt):
            wt = w if w.ndim == 1 else w[t]
            acc = np.full(cells, -0.0)
            wsum = np.zeros(cells)
            cnt = np.zeros(cells, dtype=np.int64)
            for k in range(W):
                s = t - lead + k
                row = y64[s] if 0 <= s < nt else np.full(cells, np.nan)
                valid = ~np.isnan(row)
                acc = acc + np.where(valid, wt[k] * row, 0.0)
                wsum = wsum + np.where(valid, wt[k], 0.0)
                cnt = cnt + valid
            res = acc / wsum if normalise else acc
            out[t] = np.where(cnt < min_count, np.nan, res)
    return out


def tap_sums(y, w, lead):
    """``(acc, wsum, cnt)`` of every output step at once, (nt, ...) each: the loop of ``time_filter``
    turned inside out.  It runs over the taps k only, ascending; tap k of ALL outputs is the record
    shifted by k - lead, read from a copy padded with NaN rows for the steps outside [0, nt).  Per
    output the start values (-0.0, 0, 0), the order of the adds and the ``where(valid, w * y, 0.0)``
    terms are ``time_filter``'s, so the sums are its sums bit for bit (tests/test_filter_host.py)."""
    y64 = np.asarray(y).astype(np.float64)
    nt = y64.shape[0]
    w = np.asarray(w, dtype=np.float64)
    W = w.shape[-1]
    assert 1 <= W <= nt and 0 <= lead < W and (w.ndim == 1 or w.shape == (nt, W))
    cells = y64.shape[1:]
    padded = np.full((nt + W - 1,) + cells, np.nan)
    padded[lead:lead + nt] = y64  # step s sits in row s + lead: tap k of output t is row t + k
    acc = np.full(y64.shape, -0.0)
    wsum = np.zeros(y64.shape)
    cnt = np.zeros(y64.shape, dtype=np.int64)
    term = np.empty(y64.shape)  # (buffers written in place: the record may be tens of MB)
    mask = np.empty(y64.shape, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(W):
            rows = padded[k:k + nt]
            wk = w[k] if w.ndim == 1 else w[:, k].reshape((nt,) + (1,) * len(cells))
            np.isnan(rows, out=mask)  # not valid
            np.multiply(wk, rows, out=term)
            np.copyto(term, 0.0, where=mask)  # where(valid, w[k] * y, 0.0)
            acc += term
            np.copyto(term, wk)
            np.copyto(term, 0.0, where=mask)  # where(valid, w[k], 0.0)
            wsum += term
            np.logical_not(mask, out=mask)  # valid
            cnt += mask
    return acc, wsum, cnt


def finish(acc, wsum, cnt, min_count, normalise=False):
    """the result of the contract from the three sums of ``tap_sums``"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        res = acc / wsum if normalise else acc
    return np.where(cnt < min_count, np.nan, res)


def time_filter_taps(y, w, lead, min_count=None, normalise=False):
    """``time_filter`` for long records: the same float64 (nt, ...) result, bit for bit, from a
    loop over the W taps instead of over nt x W (``tap_sums``)"""
    W = np.asarray(w).shape[-1]
    min_count = W if min_count is None else int(min_count)
    assert 1 <= min_count <= W
    return finish(*tap_sums(y, w, lead), min_count, normalise)


def window_bounds(t, window, center, nt):
    """[lo, hi) of the window of step t, clipped to the record: centred
    [t - window // 2, t + (window - 1) // 2], trailing [t - window + 1, t]"""
    lo = t - window // 2 if center else t - window + 1
    return max(lo, 0), min(lo + window, nt)


def rolling_mean_nanmean(y, window, center=True, min_periods=None):
    """xarray's ``.rolling(time=window, center=center, min_periods=min_periods).mean()`` values,
    said with numpy: nanmean over the steps of the window that exist, NaN where fewer than
    ``min_periods`` (default ``window``) of them are valid"""
    y64 = np.asarray(y).astype(np.float64)
    nt = y64.shape[0]
    min_periods = window if min_periods is None else min_periods
    out = np.empty_like(y64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for t in range(nt):
            lo, hi = window_bounds(t, window, center, nt)
            sel = y64[lo:hi]
            out[t] = np.where((~np.isnan(sel)).sum(axis=0) < min_periods, np.nan,
                              np.nanmean(sel, axis=0))
    return out


def polyfit_slopes(x, y, window, lead):
    """numpy.polyfit(x[window], y[window], 1)[0] per complete window (NaN elsewhere, and where the
    window holds a NaN); x is centred on the window's first step before the fit, which leaves the
    slope what it is and polyfit well conditioned"""
    x = np.asarray(x, dtype=np.float64)
    y64 = np.asarray(y).astype(np.float64)
    nt = y64.shape[0]
    flat = y64.reshape(nt, -1)
    out = np.full(flat.shape, np.nan)
    for t in range(nt):
        lo = t - lead
        if lo < 0 or lo + window > nt:
            continue
        seg = flat[lo:lo + window]
        ok = ~np.isnan(seg).any(axis=0)
        if ok.any():
            out[t, ok] = np.polyfit(x[lo:lo + window] - x[lo], seg[:, ok], 1)[0]
    return out.reshape(y64.shape)
