"""GPU: the time filter (core.time_filter; csrc/momlevel_filter.hip) past one block of cells, at
every pack width, on windows that sit on the edges of the kernel's walk and on records that end
inside a time tile.

The cell counts are test_gpu_clim_edges.py's (float64: 511, 512, 513, 1026, 1030; float32: 513,
1023, 1024, 1026, 2052 -- one, two and four cells a lane over up to four blocks of 256 lanes, the
last one ragged), and a record that fills a pack is also placed 1 and 2 elements into a flat buffer:
the narrower kernels must give the aligned result bit for bit.  So must a float64 result written 8
bytes off a 16-byte boundary; test_windows_on_every_edge also runs on 8 float32 cells for that.

The record has nt = min(96, about 2 1/2 time tiles) steps, but at least W + 3: tile and window edges
come from the library's own queries (core.filter_tile, core.filter_window_edges).  Windows: 1, 2, 3,
every edge and the lengths beside it, and nt; each centred and trailing, and one lead that is
neither.  The field has land columns (one beside the last cell of the last block), 5 % scattered
NaN, a cell with one valid step, a cell that is NaN on the first and on the last step, and a column
of -0.0.

Gates (none taken from what the kernel gives): float64 results are bit-identical to
filter_numpy.time_filter, NaN masks included; float32 results are that float64 result rounded once;
with weights of 1, normalised, the result is also bit-identical to core.time_group_stat over the
window's steps (the grouped-statistic kernel as an independent witness) wherever the valid count
reaches min_count.
"""

import numpy as np
import pytest
import torch

import filter_numpy as fn
from conftest import assert_bit_equal
from momlevel_amd import core
from test_gpu_clim_edges import CELL_IDS, CELLS, DEV, _placements

pytestmark = pytest.mark.gpu

ONE_VALID, ENDS_NAN, NEG_ZERO = 3, 5, 7  # special cells


def _nt(window):
    return max(min(96, (5 * core.filter_tile()) // 2), window + 3)


def _windows():
    edges = core.filter_window_edges()
    base = {1, 2, 3}
    for e in edges:
        base |= {e - 1, e, e + 1}
    return sorted(w for w in base if w >= 1)


_cache = {}


def _record(nt, n, dtype):
    if (nt, n, dtype) not in _cache:
        rng = np.random.default_rng(1000 * nt + n)
        y = rng.normal(0.0, 1.0, (nt, n))
        land = rng.random(n) < 0.2
        land[[0, n - 2]] = True
        land[[n - 1, ONE_VALID, ENDS_NAN, NEG_ZERO]] = False
        y[:, land] = np.nan
        y[rng.random((nt, n)) < 0.05] = np.nan
        y[:, ONE_VALID] = np.nan
        y[nt // 2, ONE_VALID] = 1.5
        y[:, ENDS_NAN] = rng.normal(0.0, 1.0, nt)
        y[[0, nt - 1], ENDS_NAN] = np.nan
        y[:, NEG_ZERO] = -0.0
        y[:, n - 1] = rng.normal(0.0, 1.0, nt)  # the last cell of the last block holds data
        _cache[(nt, n, dtype)] = (y.astype(dtype), land)
    return _cache[(nt, n, dtype)]


def _straddles_a_tile(nt, window, lead):
    """some stored output's window holds steps of two time tiles (or the window is one step)"""
    tile = core.filter_tile()
    for t in range(nt):
        lo, hi = max(t - lead, 0), min(t - lead + window, nt) - 1
        if lo // tile != hi // tile:
            return True
    return window == 1


def _modes(window, rng, nt):
    """(label, weights, min_count, normalise)"""
    ones = np.ones(window)
    row = rng.normal(0.0, 1.0, window)
    if window > 1:
        row[0], row[-1] = -abs(row[0]) - 0.1, abs(row[-1]) + 0.1  # mixed signs
    out = [("mean mc=1", ones, 1, True), ("mean mc=W", ones, window, True),
           ("sum mc=W", ones, window, False), ("sum mc=1", ones, 1, False),
           ("row norm mc=1", row, 1, True), ("row plain mc=W", row, window, False),
           ("table mc=W", rng.normal(0.0, 1.0, (nt, window)), window, False),
           ("table norm mc=1", rng.uniform(0.5, 1.5, (nt, window)), 1, True)]
    if window >= 2:
        out.append(("mean mc=2", ones, 2, True))
    return out


def _check(y, dtype, window, lead, label, w, mc, norm, placements):
    got = {name: core.time_filter(yd, w, lead, mc, norm).cpu().numpy() for name, yd in placements}
    want64 = fn.time_filter(y, w, lead, mc, norm)
    what = f"W={window} lead={lead} {label} n={y.shape[1]} {np.dtype(dtype).name}"
    aligned = got["aligned"]
    assert aligned.dtype == dtype and aligned.shape == y.shape
    for name, other in got.items():
        assert_bit_equal(other, aligned, f"{what}: {name} against aligned")
    assert_bit_equal(aligned, want64.astype(dtype), what)
    return want64


@pytest.mark.parametrize("dtype, n", CELLS + [(np.float32, 8)], ids=CELL_IDS + ["float32-8"])
def test_windows_on_every_edge(dtype, n):
    tile = core.filter_tile()
    rng = np.random.default_rng(n)
    for window in _windows():
        nt = _nt(window)
        assert nt >= window + 3 and nt > 2 * tile
        y, land = _record(nt, n, dtype)
        placements = _placements(y)
        leads = sorted({window // 2, window - 1, (window - 1) // 3})
        for lead in leads:
            assert _straddles_a_tile(nt, window, lead)
            for label, w, mc, norm in _modes(window, rng, nt):
                want = _check(y, dtype, window, lead, label, w, mc, norm, placements[:1])
                assert np.isnan(want[:, land]).all()
        # every placement, and the float64 output of a float32 record, on the centred window
        lead = window // 2
        _check(y, dtype, window, lead, "mean mc=1, placements", np.ones(window), 1, True, placements)
        full = core.time_filter(placements[0][1], np.ones(window), lead, 1, True,
                                out_dtype=torch.float64).cpu().numpy()
        assert_bit_equal(full, fn.time_filter(y, np.ones(window), lead, 1, True), "float64 out")
        # the same into a result 8 bytes off a 16-byte boundary: narrower packs, the aligned bits
        buf = torch.full((nt * n + 2,), -7.0, dtype=torch.float64, device=DEV)
        view = buf[1:1 + nt * n].view(nt, n)
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() == buf.data_ptr() + 8
        assert core.time_filter(placements[0][1], np.ones(window), lead, 1, True, out=view,
                                out_dtype=torch.float64) is view
        assert_bit_equal(view.cpu().numpy(), full, "float64 out, 8 bytes off")
        assert buf[0].item() == -7.0 and buf[-1].item() == -7.0, "wrote outside the result"
        low = core.time_filter(placements[0][1], np.ones(window), lead, 1, False,
                               out_dtype=torch.float32).cpu().numpy()
        assert_bit_equal(low, fn.time_filter(y, np.ones(window), lead, 1, False).astype(np.float32),
                         "float32 out")


@pytest.mark.parametrize("dtype, n", [CELLS[2], CELLS[8]], ids=[CELL_IDS[2], CELL_IDS[8]])
def test_the_whole_record_as_one_window(dtype, n):
    nt = _nt(1)
    y, _land = _record(nt, n, dtype)
    rng = np.random.default_rng(7)
    for lead in (nt // 2, nt - 1, 0):
        for label, w, mc, norm in _modes(nt, rng, nt)[:7]:
            _check(y, dtype, nt, lead, label, w, min(mc, nt), norm, _placements(y)[:1])


@pytest.mark.parametrize("dtype, n", [CELLS[3], CELLS[6]], ids=[CELL_IDS[3], CELL_IDS[6]])
def test_special_cells_and_the_grouped_statistic_as_witness(dtype, n):
    for window in _windows() + [_nt(1)]:
        nt = _nt(window)
        y, _land = _record(nt, n, dtype)
        yd = _placements(y)[0][1]
        for center in (True, False):
            lead = window // 2 if center else window - 1
            members = [np.arange(max(t - lead, 0), min(t - lead + window, nt)) for t in range(nt)]
            steps = np.concatenate(members)
            offsets = np.concatenate([[0], np.cumsum([len(m) for m in members])])
            witness = core.time_group_stat(yd, steps, offsets, "mean").cpu().numpy()
            valid = np.stack([(~np.isnan(y[m])).sum(axis=0) for m in members])
            inside = np.array([len(m) == window for m in members])
            for mc in sorted({1, min(2, window), window}):
                got = core.time_filter(yd, np.ones(window), lead, mc, True).cpu().numpy()
                assert np.array_equal(np.isnan(got), valid < mc), (window, center, mc)
                want = np.where(valid < mc, np.nan, witness).astype(dtype)
                # The one place where the two contracts part, by the sign of a zero: a window that
                # leaves the record adds +0.0 for each missing step (include/momlevel_filter.h),
                # a group simply does not list it (include/momlevel_clim.h).  -0.0 + 0.0 is +0.0.
                clipped = ~inside & ~np.isnan(want[:, NEG_ZERO])
                assert np.signbit(want[clipped, NEG_ZERO]).all()
                assert (got[clipped, NEG_ZERO] == 0.0).all()
                assert not np.signbit(got[clipped, NEG_ZERO]).any()
                want[clipped, NEG_ZERO] = 0.0
                assert_bit_equal(got, want,
                                 f"W={window} centre={center} mc={mc} against time_group_stat")
            # the special cells
            s = core.time_filter(yd, np.ones(window), lead, 1, False).cpu().numpy()
            assert np.signbit(s[inside, NEG_ZERO]).all() and (s[:, NEG_ZERO] == 0.0).all()
            assert not np.signbit(s[~inside, NEG_ZERO]).any()  # -0.0 + (+0.0 of a missing step)
            has = np.array([nt // 2 in m for m in members])
            assert np.array_equal(~np.isnan(s[:, ONE_VALID]), has) and (s[has, ONE_VALID] == 1.5).all()
            full = core.time_filter(yd, np.ones(window), lead, window, False).cpu().numpy()
            touched = np.array([0 in m or nt - 1 in m or len(m) < window for m in members])
            assert np.isnan(full[touched, ENDS_NAN]).all()
            assert not np.isnan(full[~touched, ENDS_NAN]).any()


def test_operand_refusals_on_the_device():
    y = torch.zeros((12, 6), dtype=torch.float64, device=DEV)
    for kw in (dict(w=[1.0] * 13, lead=0), dict(w=[1.0, 1.0], lead=2), dict(w=[1.0, 1.0], lead=-1),
               dict(w=[1.0, 1.0], lead=0, min_count=3), dict(w=[1.0, 1.0], lead=0, min_count=0),
               dict(w=[1.0, np.nan], lead=0), dict(w=np.ones((11, 2)), lead=0),
               dict(w=[1.0], lead=0, out=torch.zeros((12, 5), dtype=torch.float64, device=DEV))):
        with pytest.raises(ValueError):
            core.time_filter(y, **kw)
    with pytest.raises(TypeError):
        core.time_filter(y.cpu(), [1.0], 0)
    with pytest.raises(TypeError):
        core.time_filter(y, [1.0], 0, out_dtype=torch.float16)
    out = torch.empty((12, 6), dtype=torch.float32, device=DEV)
    assert core.time_filter(y, [1.0], 0, out=out, out_dtype=torch.float32) is out
    ints = torch.arange(24, device=DEV).reshape(12, 2)
    got = core.time_filter(ints, [1.0, 1.0], 1)
    assert got.dtype == torch.float64 and got[1].tolist() == [2.0, 4.0] and torch.isnan(got[0]).all()
    assert core.time_filter(y[:, :0], [1.0], 0).shape == (12, 0)
