"""The numpy restatement of the grouped time statistics (momlevel_amd.climatology): select the
rows of a group, then numpy.nanmean / nanstd / nanmin / nanmax over axis 0 of the float64-widened
data.  The groups are made here from the calendar objects themselves, not from the package's plans.

With axis=0 on a (k, cells) selection numpy accumulates row after row, in order: that is the
arithmetic contract of include/momlevel_clim.h, and float64 results compare bit for bit.  (A
selection with ONE cell collapses to a 1-d pairwise sum in numpy; the bit-exact tests keep more
than one cell.)"""

import warnings

import numpy as np

FUNCS = {"mean": np.nanmean, "std": np.nanstd, "min": np.nanmin, "max": np.nanmax}


def group_stat(y, sel, stat):
    """``stat`` over the rows ``sel`` of ``y`` (time leading), float64; an empty or all-NaN group
    gives NaN"""
    y64 = np.asarray(y).astype(np.float64)
    sel = np.asarray(sel, dtype=np.int64)
    if sel.size == 0:
        return np.full(y64.shape[1:], np.nan)
    with warnings.catch_warnings():  # "Mean of empty slice", "All-NaN slice", "Degrees of freedom"
        warnings.simplefilter("ignore", RuntimeWarning)
        return FUNCS[stat](y64[sel], axis=0)


def grouped(y, steps, offsets, stat):
    """one row per group: group g is steps[offsets[g]:offsets[g + 1]]"""
    steps = np.asarray(steps)
    return np.stack([group_stat(y, steps[offsets[g]:offsets[g + 1]], stat)
                     for g in range(len(offsets) - 1)], axis=0)


def monthly_groups(time_values):
    """row indices per (year, month) present, ascending"""
    keys = [(t.year, t.month) for t in time_values]
    return [np.array([i for i, k in enumerate(keys) if k == key]) for key in sorted(set(keys))]


def cycle_groups(time_values):
    """row indices per calendar month 1..12, over all years"""
    months = [t.month for t in time_values]
    return [np.array([i for i, m in enumerate(months) if m == mon]) for mon in range(1, 13)]


def monthly_average(y, time_values):
    return np.stack([group_stat(y, sel, "mean") for sel in monthly_groups(time_values)], axis=0)


def annual_cycle(y, time_values, func="mean"):
    return np.stack([group_stat(y, sel, func) for sel in cycle_groups(time_values)], axis=0)
