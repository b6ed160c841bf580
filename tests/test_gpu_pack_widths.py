"""Every pack width of the trend, grouped-statistic and stratification kernels computes the same
bits (csrc/mlx_pack.hpp: a lane moves 4, 2 or 1 adjacent cells in one access; the entry points
choose by the cell count and by the alignment of the pointers).

A record of 8 cells takes the widest pack (4 float32 / 2 float64 cells; the stratification kernel
stops at 2 of either), 6 cells two to a lane, 7 cells one.  The 8-cell record is
then placed one and two elements into a flat buffer -- still contiguous, so nothing realigns it --
which takes the narrower kernels over the SAME values: their results must be the aligned ones bit
for bit, the arithmetic of a cell never depends on the pack it travels in.  The aligned result is
held against the numpy restatement of the feature's own GPU test, as that test asserts it.

The time axis is as short as each function allows: 4 steps for the fit, two groups of 3 for the
statistic, 3 levels for the stratification.  (The spiciness and vorticity kernels have their own:
test_views_and_prefixes_are_slices_of_the_whole, test_record_slices_offset_pointers_and_two_runs.)
The same placements over several blocks of cells, with a ragged last block, are in
test_gpu_trend_edges.py and test_gpu_clim_edges.py.
"""

import numpy as np
import pytest
import torch

import clim_numpy as cn
import trend_numpy as tn
from conftest import assert_bit_equal
from momlevel_amd import core, trend
from oracle import momlevel_numpy as o

pytestmark = pytest.mark.gpu

CELLS = (8, 6, 7)
DTYPES = [np.float64, np.float32]
GATE = 1e-10  # test_gpu_trend.py's gate on the fit


def _placements(y):
    """[(label, device tensor)] of the host record ``y`` (steps, cells): aligned in an allocation of
    its own and, for 8 cells, 1 and 2 elements into a flat buffer"""
    rows, n = y.shape
    flat = torch.from_numpy(np.ascontiguousarray(y).reshape(-1))
    out = [("aligned", flat.cuda().view(rows, n))]
    if n == 8:
        for k in (1, 2):
            buf = torch.zeros(rows * n + 4, dtype=flat.dtype, device="cuda")
            buf[k:k + rows * n] = flat.cuda()
            view = buf[k:k + rows * n].view(rows, n)
            assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + k * flat.element_size()
            out.append((f"offset {k}", view))
    return out


def _record(rows, n, dtype, seed):
    """noise about 100 with one land cell (every step NaN) and one NaN step elsewhere"""
    y = np.random.default_rng(seed).normal(100.0, 20.0, (rows, n))
    y[:, 1] = np.nan
    y[rows - 1, n - 2] = np.nan
    return y.astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", CELLS)
def test_linfit_and_remove(n, dtype):
    nt = 4
    x = np.cumsum(np.random.default_rng(nt).uniform(0.05, 0.45, nt))  # test_gpu_trend.py's numeric axis
    y = _record(nt, n, dtype, seed=n)
    xt, s, xmean = trend.fit_axis(x)
    results = {}
    for label, yd in _placements(y):
        m, b = core.time_linfit(yd, xt, s, xmean)
        rem = core.time_apply(yd, "remove", x, m, b)
        results[label] = tuple(t.cpu().numpy() for t in (m, b, rem))
    m, b, rem = results["aligned"]
    for label, got in results.items():
        for what, a, g in zip(("slope", "intercept", "remove"), results["aligned"], got):
            assert_bit_equal(g, a, f"{what}, {label} against aligned")
    # the fit against numpy.polyfit per column: test_fit_parity_with_numpy_polyfit's three measures
    want_m, want_b = tn.polyfit_columns(x, y)
    assert m.dtype == np.float64 and m.shape == (n,)
    assert np.array_equal(np.isnan(m), np.isnan(want_m)), "NaN placement of the slope"
    assert np.array_equal(np.isnan(b), np.isnan(want_b)), "NaN placement of the intercept"
    ok = ~np.isnan(want_m)
    assert ok.any() and (~ok).any()
    ymax = np.nanmax(np.abs(y.astype(np.float64)))
    span = x.max() - x.min()
    xs = x[:, None]
    line = np.max(np.abs((m * xs + b) - (want_m * xs + want_b))[:, ok]) / ymax
    icpt = np.max(np.abs(b - want_b)[ok]) / (ymax * (1 + abs(x.mean()) / span))
    slope = np.max(np.abs(m - want_m)[ok] / np.abs(want_m[ok]))
    print(f"n={n} {np.dtype(dtype).name}: line {line:.2e} intercept {icpt:.2e} slope {slope:.2e}")
    assert line <= GATE and icpt <= GATE and slope <= GATE
    # the pointwise pass is numpy's, bit for bit (test_pointwise_passes_are_bit_identical_to_numpy)
    assert rem.dtype == np.float64
    assert_bit_equal(rem, y - (m * xs + b), "mode=remove")


@pytest.mark.parametrize("stat", ("mean", "std", "min", "max"))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", CELLS)
def test_group_stat(n, dtype, stat):
    steps, offsets = np.array([0, 2, 4, 5, 3, 1]), np.array([0, 3, 6])  # two groups of 3, as listed
    y = _record(6, n, dtype, seed=10 + n)
    results = {label: core.time_group_stat(yd, steps, offsets, stat).cpu().numpy()
               for label, yd in _placements(y)}
    for label, got in results.items():
        assert_bit_equal(got, results["aligned"], f"{stat}, {label} against aligned")
    # numpy's nan-statistic over axis 0, in float64 and rounded once for a float32 record
    # (test_annual_cycle_float64_bits, test_float32_is_the_float64_result_rounded_once)
    want = cn.grouped(y, steps, offsets, stat).astype(dtype)
    assert np.isnan(want).any() and not np.isnan(want).all()
    assert results["aligned"].dtype == want.dtype
    assert_bit_equal(results["aligned"], want, f"{stat} against numpy")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", CELLS)
def test_n2(n, dtype):
    nt, nz = 2, 3
    z = np.cumsum(2.0 * 1.075 ** np.arange(nz)) - 1.0  # test_gpu_stratification.py's uneven levels
    r = np.random.default_rng(20 + n)
    T = r.uniform(-2.0, 30.0, (nt, nz, 1, n)).astype(dtype)
    S = r.uniform(30.0, 40.0, (nt, nz, 1, n)).astype(dtype)
    T[..., 1], S[..., 1] = np.nan, np.nan             # a land column
    T[:, nz - 1, :, n - 2], S[:, nz - 1, :, n - 2] = np.nan, np.nan  # a sub-bottom cell
    pres = z * 1.0e4 + 101325.0                       # derived.calc_n2's pressure
    results = {}
    rows = nt * nz
    for (label, Td), (_, Sd) in zip(_placements(T.reshape(rows, n)), _placements(S.reshape(rows, n))):
        n2 = core.stratification(Td.view(nt, nz, n), Sd.view(nt, nz, n), pres, z, func="n2")
        results[label] = n2.cpu().numpy().reshape(nt, nz, 1, n)
    for label, got in results.items():
        assert_bit_equal(got, results["aligned"], f"N^2, {label} against aligned")
    ref = o.calc_n2(T, S, z)  # test_n2_bit_identical_to_numpy
    assert results["aligned"].dtype == np.float64 and ref.dtype == np.float64
    assert np.isnan(ref).any() and not np.isnan(ref).all()
    assert_bit_equal(results["aligned"], ref, "calc_n2")
