"""GPU: the trend kernels (csrc/momlevel_trend.hip) past one block of cells, at every pack width and
at the edges of their time windows, through the ``core.*`` wrappers (exact shapes and pointers).

Every kernel's grid runs over the flattened cell axis, ``(blockIdx.x * 256 + threadIdx.x) * V`` with
V = 1, 2 or 4 cells a lane, chosen from ``n % V`` and the pointers' alignment.  The cell counts here
are the smallest that cross those edges:

  float64  511 (V=1, 2 blocks)  512 (V=2, one full block)  513 (V=1, 3 blocks, the last of ONE cell)
           1026 (V=2, 3 blocks, the last of 2 cells)  1030 (V=2, 3 blocks, the last of 6 cells)
  float32  513 (V=1, 3 blocks)  1023 (V=1, 4 blocks)  1024 (V=4, one full block)
           1026 (V=2: 1026 % 4 == 2; 3 blocks)  2052 (V=4, 3 blocks, the last of 4 cells)

A record that fills a pack is also placed 1 and 2 elements into a flat buffer, which takes the
narrower kernels over the same values: their results must be the aligned ones bit for bit, over
several blocks.  The fields are test_gpu_trend.py's (land cells, scattered NaN steps) with a land
cell, a cell of one valid step and a NaN step placed by hand, the NaN step in the last cell of the
last block and the land cell beside it (513 cells: the last block holds that one cell only).

Gates (none taken from what the kernels give):
  * time_linfit: numpy.polyfit per column with test_fit_parity_with_numpy_polyfit's three measures
    at its gate, 1e-10; NaN placement identical; fewer than 2 valid steps give NaN;
  * time_project: |coef - ref| <= 1e-10 * sum_t |P[t,k] * y[t,cell]|, ref the same sum in
    numpy.longdouble (a sequential float64 sum of these terms stays within 2.6e-16 of that scale);
  * time_apply: bit-identical to numpy in the header's operator order.
Every gated figure is printed before it is asserted.  Worst figures on an MI355X, of the 45 fits
and the 70 x 8 projections: line 1.78e-15 and intercept 1.21e-15 (nt=7, 1030 cells, float64), slope
3.57e-12 (nt=257, 1023 cells, float32); projection 3.70e-16 (nt=257, 1026 cells, float64).

Records of 4096 and 4097 steps (513 float64 and 1023 float32 cells) take the fits to windows longer
than 256 steps: sixteen windows -- asserted through mlx_time_fit_workspace_bytes -- of 256, and of
257 with a last one of 242, which ends every window in the remainder of the fit loop's unroll of 8.
Same measures, same gate.  Worst figures on an MI355X, of those 4 fits and 2 x 8 projections: line
1.05e-15 (nt=4096, 513 cells, float64), intercept 6.36e-16 (nt=4096, 1023 cells, float32), slope
2.85e-14 (nt=4097, 513 cells, float64); projection 4.53e-17 (nt=4097, 1023 cells, float32).
"""

import numpy as np
import pytest
import torch

import trend_numpy as tn
from conftest import assert_bit_equal
from momlevel_amd import _lib, core, trend

pytestmark = pytest.mark.gpu

GATE = 1e-10  # test_gpu_trend.py's gate on the fit; the project's gate for sums
DEV = "cuda"
N64 = (511, 512, 513, 1026, 1030)
N32 = (513, 1023, 1024, 1026, 2052)
CELLS = [(np.float64, n) for n in N64] + [(np.float32, n) for n in N32]
CELL_IDS = [f"{np.dtype(d).name}-{n}" for d, n in CELLS]
# three or more blocks with a ragged last one, at every pack width of either dtype
RAGGED = [(np.float64, 513), (np.float64, 1030), (np.float32, 513), (np.float32, 1026),
          (np.float32, 2052)]


def _pack(dtype, n):
    """cells a lane moves when every pointer is 16-byte aligned (pack_width of the .hip)"""
    v = 16 // np.dtype(dtype).itemsize
    while v > 1 and n % v:
        v //= 2
    return v


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _placements(y):
    """test_gpu_pack_widths.py's: [(label, device tensor)] of the host record ``y`` (steps, cells),
    aligned in an allocation of its own and, where the cells fill a pack, 1 and 2 elements into a
    flat buffer"""
    rows, n = y.shape
    flat = torch.from_numpy(np.ascontiguousarray(y).reshape(-1))
    out = [("aligned", flat.to(DEV).view(rows, n))]
    if _pack(y.dtype, n) > 1:
        for k in (1, 2):
            buf = torch.zeros(rows * n + 4, dtype=flat.dtype, device=DEV)
            buf[k:k + rows * n] = flat.to(DEV)
            view = buf[k:k + rows * n].view(rows, n)
            assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + k * flat.element_size()
            out.append((f"offset {k}", view))
    return out


def _land(n, r):
    land = r.random(n) < 0.2
    land[0], land[-1], land[n - 2] = True, False, True  # (n - 2: beside the last cell of the last block)
    land[1] = False
    return land


def _record(nt, n, dtype, seed, gaps=True):
    """test_gpu_trend.py::_field on a flat cell axis: noise (sd 20) about 100 plus a per-cell trend of
    +-(0.5 .. 1.5) * 20 over the record; land cells; with ``gaps``, cells with 30 % scattered NaN
    steps (each keeping >= 3 valid steps), ONE valid step in cell 1, and a NaN step in the last cell.
    Records shorter than 64 steps carry noise of sd 2: the slope measure is relative, so the data must
    determine the slope, and over a handful of steps noise of the trend's own size cancels it in some
    cell of a few thousand (a fitted slope 1e-5 of the trend turns rounding of 1e-16 into 1e-11)."""
    r = np.random.default_rng(seed)
    rate = r.uniform(0.5, 1.5, n) * r.choice([-1.0, 1.0], n) * 20.0
    y = r.normal(100.0, 20.0 if nt >= 64 else 2.0, (nt, n)) + rate * np.linspace(-0.5, 0.5, nt)[:, None]
    land = _land(n, r)
    y[:, land] = np.nan
    if gaps:
        drop = int(0.3 * nt)
        if nt - drop >= 3 and drop > 0:
            for j in np.nonzero(~land & (r.random(n) < 0.4))[0]:
                y[r.choice(nt, drop, replace=False), j] = np.nan
        y[1:, 1] = np.nan
        y[nt // 2, n - 1] = np.nan
    return y.astype(dtype)


def _axis(nt):
    """test_gpu_trend.py's numeric axis: uneven steps from 0"""
    return np.cumsum(np.random.default_rng(nt).uniform(0.05, 0.45, nt))


def _per_cell(n, seed, rows=None):
    """float64 values per cell as a fit returns them: NaN on the land cells"""
    r = np.random.default_rng(seed)
    a = r.normal(0.0, 3.0, n if rows is None else (rows, n))
    a[..., _land(n, r)] = np.nan
    return a


# ---- time_linfit --------------------------------------------------------------------------------
NT_FIT = (2, 7, 8, 9, 255, 256, 257, 513)  # the unroll of 8, the window of 256 (513: 256 + 256 + 1)
FIT_CASES = ([(257, d, n) for d, n in CELLS]
             + [(nt, d, n) for nt in NT_FIT if nt != 257 for d, n in RAGGED])


@pytest.mark.parametrize("nt, dtype, n", FIT_CASES,
                         ids=[f"{nt}-{np.dtype(d).name}-{n}" for nt, d, n in FIT_CASES])
def test_linfit_across_blocks_and_windows(nt, dtype, n):
    _linfit_case(nt, dtype, n)


def _linfit_case(nt, dtype, n):
    x = _axis(nt)
    y = _record(nt, n, dtype, seed=nt * 31 + n)
    xt, s, xmean = trend.fit_axis(x)
    results = {}
    for label, yd in _placements(y):
        m, b = core.time_linfit(yd, xt, s, xmean)
        results[label] = (m.cpu().numpy(), b.cpu().numpy())
    m, b = results["aligned"]
    for label, got in results.items():
        assert_bit_equal(got[0], m, f"slope, {label} against aligned")
        assert_bit_equal(got[1], b, f"intercept, {label} against aligned")
    want_m, want_b = tn.polyfit_columns(x, y)
    assert m.dtype == np.float64 and m.shape == (n,) and b.shape == (n,)
    assert np.array_equal(np.isnan(m), np.isnan(want_m)), "NaN placement of the slope"
    assert np.array_equal(np.isnan(b), np.isnan(want_b)), "NaN placement of the intercept"
    few = (~np.isnan(y)).sum(axis=0) < 2
    assert few[0] and few[1] and few[n - 2] and np.isnan(m[few]).all() and np.isnan(b[few]).all()
    ok = ~np.isnan(want_m)
    assert np.array_equal(ok, ~few) and ok.any() and (ok[-1] or nt == 2)
    ymax = np.nanmax(np.abs(y.astype(np.float64)))
    span = x.max() - x.min()
    xs = x[:, None]
    line = np.max(np.abs((m * xs + b) - (want_m * xs + want_b))[:, ok]) / ymax
    icpt = np.max(np.abs(b - want_b)[ok]) / (ymax * (1 + abs(x.mean()) / span))
    slope = np.max(np.abs(m - want_m)[ok] / np.abs(want_m[ok]))
    print(f"linfit nt={nt} n={n} {np.dtype(dtype).name}: line {line:.2e} intercept {icpt:.2e} "
          f"slope {slope:.2e}")
    assert line <= GATE and icpt <= GATE and slope <= GATE


# Records long enough for the fit's time windows to outgrow 256 steps (a daily record): from sixteen
# windows on the window is ceil(nt / 16).  4096: sixteen windows of exactly 256; 4097: sixteen of 257
# -- no multiple of the fit loop's unroll of 8, so every window ends in the remainder loop -- the
# last one ragged.  One cell a lane at either dtype, three and four blocks, the last of one cell.
NT_LONG = (4096, 4097)
LONG_CELLS = [(np.float64, 513), (np.float32, 1023)]
LONG_IDS = [f"{np.dtype(d).name}-{n}" for d, n in LONG_CELLS]
LONG_WINDOWS = 16


def _fit_windows(nt, n, nterms):
    """time windows of a fit over (nt, n), from the workspace the library asks for: ``nterms``
    float64 partial sums per cell and window"""
    nbytes = int(_lib.load_trend().mlx_time_fit_workspace_bytes(nt, n, nterms))
    assert nbytes > 0 and nbytes % (nterms * n * 8) == 0
    return nbytes // (nterms * n * 8)


def _assert_long_windows(nt, n, nterms, what):
    windows = _fit_windows(nt, n, nterms)
    shortest = -(-nt // windows)  # no window of `windows` equal ones can be shorter
    print(f"{what} nt={nt} n={n}: {windows} windows of {shortest} steps, the last of "
          f"{nt - (windows - 1) * shortest}")
    assert windows == LONG_WINDOWS
    assert shortest == (256 if nt == 256 * LONG_WINDOWS else 257)


@pytest.mark.parametrize("nt", NT_LONG)
@pytest.mark.parametrize("dtype, n", LONG_CELLS, ids=LONG_IDS)
def test_linfit_windows_longer_than_256_steps(dtype, n, nt):
    _assert_long_windows(nt, n, 5, "linfit")
    _linfit_case(nt, dtype, n)


# ---- time_project -------------------------------------------------------------------------------
NT_PROJECT = (1, 3, 4, 5, 256, 257, 513)  # the unroll of 4; <= 256: one window, written to coef itself


def _project_reference(P, y):
    """(sum_t P[t,k] * y[t,cell], sum_t |P[t,k] * y[t,cell]|) in numpy.longdouble, (K, n) each"""
    yl = y.astype(np.longdouble)
    ref = np.empty((P.shape[1], y.shape[1]), dtype=np.longdouble)
    scale = np.empty_like(ref)
    for k in range(P.shape[1]):
        terms = P[:, k].astype(np.longdouble)[:, None] * yl
        ref[k], scale[k] = terms.sum(axis=0), np.abs(terms).sum(axis=0)
    return ref, scale


@pytest.mark.parametrize("nt", NT_PROJECT)
@pytest.mark.parametrize("dtype, n", CELLS, ids=CELL_IDS)
def test_project_every_k_across_blocks_and_windows(dtype, n, nt):
    _project_case(dtype, n, nt)


@pytest.mark.parametrize("dtype, n", LONG_CELLS, ids=LONG_IDS)
def test_project_windows_longer_than_256_steps(dtype, n):
    nt = NT_LONG[-1]
    for K in (1, 8):
        _assert_long_windows(nt, n, K, f"project K={K}")
    _project_case(dtype, n, nt)


def _project_case(dtype, n, nt):
    v = _pack(dtype, n)
    seam = 256 * v if 256 * v + 1 < n else 255 * v  # the first (or last) pack of a block
    y = _record(nt, n, dtype, seed=nt * 17 + n, gaps=False)
    y[:, seam - 1:seam + 2] = np.random.default_rng(n).normal(100.0, 20.0, (nt, 3)).astype(dtype)
    y[nt // 2, seam] = np.nan
    bad = np.isnan(y).any(axis=0)
    assert bad[seam] and not bad[seam - 1] and not bad[seam + 1] and bad[n - 2] and not bad[n - 1]
    P8 = np.random.default_rng(nt).normal(0.0, 1.0, (nt, 8))
    ref8, scale8 = _project_reference(P8, y)
    placed = _placements(y)
    worst = 0.0
    for K in range(1, 9):
        P = np.ascontiguousarray(P8[:, :K])
        results = {label: core.time_project(yd, P).cpu().numpy() for label, yd in placed}
        coef = results["aligned"]
        assert coef.dtype == np.float64 and coef.shape == (K, n)
        for label, got in results.items():
            assert_bit_equal(got, coef, f"K={K}, {label} against aligned")
        # one NaN step takes all K coefficients of its cell and no other cell's
        assert np.array_equal(np.isnan(coef), np.broadcast_to(bad, (K, n))), f"K={K}: NaN placement"
        err = np.abs(coef[:, ~bad] - ref8[:K][:, ~bad]) / scale8[:K][:, ~bad]
        worst = max(worst, float(err.max()))
    print(f"project nt={nt} n={n} {np.dtype(dtype).name}: worst |coef - ref| / sum|P*y| {worst:.2e}")
    assert worst <= GATE


# ---- time_apply, straight-line modes ------------------------------------------------------------
NT_APPLY = (1, 63, 64, 65, 129)  # the window of 64


def _line(mode, y64, m, b, x):
    xs = x[:, None]
    if mode == "remove":
        return y64 - (m * xs + b)
    if mode == "correct":
        return y64 - m * xs
    if mode == "trend":
        return m * xs
    return m * xs - m * xs[0]


def _offset_out(nt, n):
    """(buffer, view): a float64 result view one element into its buffer, 8-byte aligned only"""
    buf = torch.full((nt * n + 2,), -7.0, dtype=torch.float64, device=DEV)
    view = buf[1:1 + nt * n].view(nt, n)
    assert view.data_ptr() == buf.data_ptr() + 8
    return buf, view


def _apply_everywhere(y, mode, xm, a, b):
    """the aligned result, after holding every placement of ``y`` and an ``out=`` view one element
    into its buffer to its bits"""
    reads_y = mode in ("remove", "correct", "model_resid")
    nt, n = y.shape
    ad, bd = _dev(a), None if b is None else _dev(b)
    placed = _placements(y) if reads_y else [("aligned", None if y.dtype == np.float32 else _dev(y))]
    base = core.time_apply(placed[0][1], mode, xm, ad, bd)
    assert base.dtype == torch.float64 and tuple(base.shape) == (nt, n)
    base = base.cpu().numpy()
    for label, yd in placed[1:]:
        assert_bit_equal(core.time_apply(yd, mode, xm, ad, bd).cpu().numpy(), base,
                         f"{mode}, {label} against aligned")
    buf, view = _offset_out(nt, n)
    got = core.time_apply(placed[0][1], mode, xm, ad, bd, out=view)
    assert got.data_ptr() == view.data_ptr()
    assert_bit_equal(view.cpu().numpy(), base, f"{mode}, out= one element into its buffer")
    assert buf[0].item() == -7.0 and buf[-1].item() == -7.0, "wrote outside the result"
    return base


@pytest.mark.parametrize("mode", ["remove", "correct", "trend", "trend_anom"])
@pytest.mark.parametrize("dtype, n", CELLS, ids=CELL_IDS)
def test_apply_line_modes_are_numpy_bit_for_bit(dtype, n, mode):
    m, b = _per_cell(n, seed=n), _per_cell(n, seed=n + 1)
    for nt in NT_APPLY:
        x = _axis(nt) + 3.0
        y = _record(nt, n, dtype, seed=nt * 13 + n)
        got = _apply_everywhere(y, mode, x, m, b if mode == "remove" else None)
        want = _line(mode, y.astype(np.float64), m, b, x)
        assert np.isnan(want).any() and not np.isnan(want).all()
        assert_bit_equal(got, want, f"{mode} nt={nt} n={n} {np.dtype(dtype).name}")


# ---- time_apply, model modes --------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4, 5, 6, 7, 8])  # KT = 4 (K <= 4), 6 and 8
@pytest.mark.parametrize("mode", ["model", "model_resid"])
@pytest.mark.parametrize("dtype, n", CELLS, ids=CELL_IDS)
def test_apply_model_modes_are_the_ascending_k_loop(dtype, n, mode, K):
    c = _per_cell(n, seed=n + K, rows=K)
    for nt in NT_APPLY:
        M = np.random.default_rng(nt + K).normal(0.0, 1.0, (K, nt))
        y = _record(nt, n, dtype, seed=nt * 11 + n)
        got = _apply_everywhere(y, mode, M, c, None)
        r = M[0][:, None] * c[0][None, :]
        for k in range(1, K):
            r = r + M[k][:, None] * c[k][None, :]
        want = y.astype(np.float64) - r if mode == "model_resid" else r
        assert np.isnan(want).any() and not np.isnan(want).all()
        assert_bit_equal(got, want, f"{mode} K={K} nt={nt} n={n} {np.dtype(dtype).name}")
