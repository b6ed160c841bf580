"""GPU: the grouped time statistic (core.time_group_stat; csrc/momlevel_clim.hip) past one block of
cells, at every pack width, on groups that sit on the edges of the kernel's row batches.

The cell counts are test_gpu_trend_edges.py's (float64: 511, 512, 513, 1026, 1030; float32: 513,
1023, 1024, 1026, 2052 -- one, two and four cells a lane over up to four blocks of 256 lanes, the
last one ragged), and a record that fills a pack is also placed 1 and 2 elements into a flat buffer:
the narrower kernels must give the aligned result bit for bit.

One record of 60 steps and one group list serve every case: groups of 7, 0, 1, 8, 9, 15, 16, 17 and
24 steps (the batch of 8 row loads, the look-ahead of the step indices at 16, an empty group), the
steps of a group in no order and most steps in more than one group.  The field has land cells (one
beside the last cell of the last block), 5 % scattered NaN steps, a cell with one valid step in
the whole record and a cell that is NaN on the one step of the one-step group.

Gates (none taken from what the kernel gives): float64 results are bit-identical to
clim_numpy.grouped (numpy's nanmean / nanstd / nanmin / nanmax over axis 0 of the selected rows,
which accumulates row after row at these widths); float32 results are that float64 result rounded
once.  An empty group and an all-NaN (group, cell) give NaN.
"""

import numpy as np
import pytest
import torch

import clim_numpy as cn
from conftest import assert_bit_equal
from momlevel_amd import core

pytestmark = pytest.mark.gpu

DEV = "cuda"
NT = 60
SIZES = (7, 0, 1, 8, 9, 15, 16, 17, 24)
N64 = (511, 512, 513, 1026, 1030)
N32 = (513, 1023, 1024, 1026, 2052)
CELLS = [(np.float64, n) for n in N64] + [(np.float32, n) for n in N32]
CELL_IDS = [f"{np.dtype(d).name}-{n}" for d, n in CELLS]
HOLE = 5  # the cell that is NaN on the one-step group's step


def _groups():
    """(steps, offsets): every group a draw without replacement from the 60 steps, as drawn"""
    r = np.random.default_rng(60)
    steps = np.concatenate([r.choice(NT, k, replace=False) for k in SIZES]).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    assert np.any(np.diff(steps[:SIZES[0]]) < 0) and np.bincount(steps, minlength=NT).max() > 1
    return steps, offsets


STEPS, OFFSETS = _groups()
_cache = {}


def _record(n, dtype):
    """test_gpu_clim.py::_field on a flat cell axis, shared between the statistics of a case"""
    if (n, dtype) not in _cache:
        rng = np.random.default_rng(n)
        y = rng.normal(100.0, 20.0, (NT, n))
        land = rng.random(n) < 0.2
        land[0], land[n - 2], land[n - 1], land[3], land[HOLE] = True, True, False, False, False
        y[:, land] = np.nan
        y[rng.random((NT, n)) < 0.05] = np.nan
        y[: NT - 1, 3] = np.nan                      # one valid step in the whole record
        y[:, HOLE] = rng.normal(100.0, 20.0, NT)
        y[STEPS[OFFSETS[2]], HOLE] = np.nan           # the one-step group is all NaN in this cell
        y[:, n - 1] = rng.normal(100.0, 20.0, NT)    # the last cell of the last block holds data
        _cache[(n, dtype)] = (y.astype(dtype), land)
    return _cache[(n, dtype)]


def _placements(y):
    """test_gpu_pack_widths.py's: aligned and, where the cells fill a pack, 1 and 2 elements into a
    flat buffer"""
    rows, n = y.shape
    flat = torch.from_numpy(np.ascontiguousarray(y).reshape(-1))
    out = [("aligned", flat.to(DEV).view(rows, n))]
    if n % 2 == 0:
        for k in (1, 2):
            buf = torch.zeros(rows * n + 4, dtype=flat.dtype, device=DEV)
            buf[k:k + rows * n] = flat.to(DEV)
            view = buf[k:k + rows * n].view(rows, n)
            assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + k * flat.element_size()
            out.append((f"offset {k}", view))
    return out


@pytest.mark.parametrize("stat", ("mean", "std", "min", "max"))
@pytest.mark.parametrize("dtype, n", CELLS, ids=CELL_IDS)
def test_group_stat_across_blocks_and_batches(dtype, n, stat):
    y, land = _record(n, dtype)
    results = {label: core.time_group_stat(yd, STEPS, OFFSETS, stat).cpu().numpy()
               for label, yd in _placements(y)}
    got = results["aligned"]
    for label, other in results.items():
        assert_bit_equal(other, got, f"{stat}, {label} against aligned")
    want = cn.grouped(y, STEPS, OFFSETS, stat).astype(dtype)
    assert got.dtype == want.dtype and got.shape == (len(SIZES), n)
    assert np.isnan(want[1]).all(), "the empty group"
    assert np.isnan(want[2, HOLE]) and not np.isnan(want[:, HOLE]).all(), "an all-NaN (group, cell)"
    assert np.isnan(want[:, land]).all() and not np.isnan(want[[0] + list(range(3, 9)), n - 1]).any()
    both = ~np.isnan(want) & ~np.isnan(got)
    print(f"{stat} n={n} {np.dtype(dtype).name}: NaN got {int(np.isnan(got).sum())} want "
          f"{int(np.isnan(want).sum())}, finite values that differ: "
          f"{int(np.sum(got[both] != want[both]))} of {int(both.sum())}")
    assert_bit_equal(got, want, f"{stat} n={n} {np.dtype(dtype).name} against numpy")
