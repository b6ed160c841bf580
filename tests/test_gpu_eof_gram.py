"""GPU: core.time_gram (csrc/momlevel_eof.hip, include/momlevel_eof.h) against the numpy restatement
tests/eof_numpy.py.

EXACT CASES.  With integer-valued data, |y - center| <= 2^9, scale in {1, 2, 4} and n <= 2^20 every
b is an integer of magnitude <= 2^11, every product one <= 2^22 and every partial sum, in ANY order,
an integer below 2^42 < 2^53: float64 arithmetic is exact, so is the host's float64 matmul of the
same integers (checked against int64 arithmetic on the smaller shapes), and the assertion is bit
equality.  The cross form uses row-dependent, asymmetric operands: a swapped row and column, or the
float32 C/D row formula on the float64 MFMA shape, cannot pass.

FLOAT CASE.  |G - B @ B.T| <= 2 (n + 2) 2^-53 sum_c |b_s b_t| elementwise: the kernel's sum and the
host's both carry at most gamma_n (n products of one rounding each, n - 1 additions, in whatever
order), and b is bit-identical on both sides by construction (two IEEE roundings, no fma)."""

import numpy as np
import pytest
import torch

import eof_numpy as en
from momlevel_amd import _lib, core
from test_eof_host import REFUSALS, gram_call

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
NT_NAMES = ["1", "3", "16", "17", "tile", "tile+1", "2tile+5"]
N_NAMES = ["1", "3", "63", "cells-1", "cells", "cells+1", "3cells+7"]


def _nt(name):
    tile = core.gram_tile()
    return {"tile": tile, "tile+1": tile + 1, "2tile+5": 2 * tile + 5}.get(name) or int(name)


def _n(name):
    cells = core.gram_cells(1)
    n = {"cells-1": cells - 1, "cells": cells, "cells+1": cells + 1,
         "3cells+7": 3 * cells + 7}.get(name) or int(name)
    assert core.gram_cells(n) == cells and n <= 1 << 20  # (the sizes sit on the range's own edges)
    return n


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _ints(rng, nt, n, dtype, center):
    """integer-valued rows with |y - center| <= 2^9"""
    return (center[None, :] + rng.integers(-512, 513, (nt, n))).astype(dtype)


def _maps(rng, n, holes=True):
    """integer centers, scales in {1, 2, 4}, with a few excluded cells (NaN) in each"""
    c1 = rng.integers(-100, 101, n).astype(F64)
    c2 = rng.integers(-100, 101, n).astype(F64)
    s = rng.choice([1.0, 2.0, 4.0], n)
    if holes and n > 3:
        c1[rng.random(n) < 0.05] = np.nan
        c2[rng.random(n) < 0.05] = np.nan
        s[rng.random(n) < 0.05] = np.nan
    return c1, c2, s


def _exact(y1, y2, c1, c2, s):
    """the expected G of an exact case: float64 matmul of integers (module docstring)"""
    ref = en.time_gram(y1, y2, c1, c2, s)
    assert np.all(ref == np.rint(ref)) and np.abs(ref).max(initial=0) < 2.0 ** 53
    if ref.size * y1.shape[1] <= 1 << 22:  # int64 arithmetic, where it is quick
        b1 = en.weighted(y1, c1, s, None if y2 is None else c2).astype(np.int64)
        b2 = b1 if y2 is None else en.weighted(y2, c2, s, c1).astype(np.int64)
        assert np.array_equal(b1 @ b2.T, ref.astype(np.int64))
    return ref


def _gram(y1, y2=None, c1=None, c2=None, s=None):
    opt = lambda a: None if a is None else _dev(a)  # noqa: E731
    return _host(core.time_gram(_dev(y1), opt(y2), opt(c1), opt(c2), opt(s)))


# ---- exact cases ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("nt_name", NT_NAMES)
def test_symmetric_form_is_exact_on_integers(nt_name, dtype):
    nt = _nt(nt_name)
    for k, n_name in enumerate(N_NAMES):
        n = _n(n_name)
        rng = np.random.default_rng(1000 * NT_NAMES.index(nt_name) + k)
        c1, _, s = _maps(rng, n)
        y = _ints(rng, nt, n, dtype, np.where(np.isnan(c1), 0.0, c1))
        got = _gram(y, None, c1, None, s)
        assert got.shape == (nt, nt) and got.dtype == F64
        assert np.array_equal(_bits(got), _bits(_exact(y, None, c1, None, s))), (nt, n)
        assert np.array_equal(_bits(got), _bits(got.T.copy()))
    # no maps at all: center 0 and scale 1
    y = _ints(rng, nt, 63, dtype, np.zeros(63))
    assert np.array_equal(_bits(_gram(y)), _bits(_exact(y, None, None, None, None)))


@pytest.mark.parametrize("dtypes", [(F64, F64), (F32, F32), (F64, F32), (F32, F64)],
                         ids=["f64xf64", "f32xf32", "f64xf32", "f32xf64"])
@pytest.mark.parametrize("nt_name", NT_NAMES)
def test_cross_form_is_exact_on_integers(nt_name, dtypes):
    nt1 = _nt(nt_name)
    others = [_nt(x) for x in NT_NAMES]
    for k, n_name in enumerate(N_NAMES):
        n = _n(n_name)
        nt2 = others[(NT_NAMES.index(nt_name) + 1 + k) % len(others)]
        rng = np.random.default_rng(77 + 1000 * NT_NAMES.index(nt_name) + k)
        c1, c2, s = _maps(rng, n)
        y1 = _ints(rng, nt1, n, dtypes[0], np.where(np.isnan(c1), 0.0, c1))
        y2 = _ints(rng, nt2, n, dtypes[1], np.where(np.isnan(c2), 0.0, c2))
        got = _gram(y1, y2, c1, c2, s)
        assert got.shape == (nt1, nt2)
        assert np.array_equal(_bits(got), _bits(_exact(y1, y2, c1, c2, s))), (nt1, nt2, n)


@pytest.mark.parametrize("dtypes", [(F64, F64), (F32, F64), (F64, F32)],
                         ids=["f64xf64", "f32xf64", "f64xf32"])
def test_cross_form_keeps_rows_and_columns_apart(dtypes):
    """y1[s, c] = (s + 1) [c = s mod 5] picks, for row s, the cells of one residue: G[s, t] is
    (s + 1) times the sum of y2[t] over them -- different in every row AND every column"""
    tile, cells = core.gram_tile(), core.gram_cells(1)
    for nt1, nt2, n in ((37, tile + 9, 63), (tile + 9, 37, cells + 1), (2 * tile + 5, 21, 330)):
        s_idx, c_idx = np.arange(nt1)[:, None], np.arange(n)[None, :]
        y1 = ((s_idx + 1) * (c_idx % 5 == s_idx % 5)).astype(dtypes[0])
        t_idx = np.arange(nt2)[:, None]
        y2 = ((3 * t_idx + 1) * ((c_idx % 7) + 1) - (c_idx % 3) * t_idx * t_idx % 11).astype(dtypes[1])
        assert np.abs(y1).max() <= 512 and np.abs(y2).max() <= 2 ** 12  # (products below 2^21: exact)
        ref = np.array([[(s + 1) * y2[t, s % 5::5].astype(np.int64).sum() for t in range(nt2)]
                        for s in range(nt1)], dtype=np.int64)
        assert not np.array_equal(ref[:21, :21], ref[:21, :21].T)
        got = _gram(y1, y2)
        assert np.array_equal(got, ref.astype(F64)), (nt1, nt2, n)
        assert np.array_equal(_gram(y2, y1), ref.T.astype(F64)), (nt2, nt1, n)


# ---- the order is fixed -----------------------------------------------------------------------------
def _normal(seed, nt, n, dtype=F64):
    rng = np.random.default_rng(seed)
    y = rng.normal(0.3, 1.0, (nt, n)).astype(dtype)
    c = y.astype(F64).mean(axis=0)
    s = np.sqrt(rng.uniform(0.5, 2.0, n))
    c[rng.random(n) < 0.1] = np.nan
    s[rng.random(n) < 0.05] = np.nan
    return y, c, s


def test_float_case_within_the_derived_bound():
    tile, cells = core.gram_tile(), core.gram_cells(1)
    nt, n = tile + 1, 3 * cells + 7
    for dtype in (F64, F32):
        y, c, s = _normal(3, nt, n, dtype)
        got = _gram(y, None, c, None, s)
        b = en.weighted(y, c, s)
        ref, mag = b @ b.T, np.abs(b) @ np.abs(b).T
        bound = 2 * (n + 2) * 2.0 ** -53 * mag
        ratio = np.abs(got - ref) / bound
        print(f"{dtype.__name__}: worst |G - B@B.T| / bound = {ratio.max():.3e}")
        assert np.all(np.abs(got - ref) <= bound)
        y2, c2, _ = _normal(4, 40, n, dtype)
        got = _gram(y, y2, c, c2, s)
        b1, b2 = en.weighted(y, c, s, c2), en.weighted(y2, c2, s, c)
        assert np.all(np.abs(got - b1 @ b2.T) <= 2 * (n + 2) * 2.0 ** -53 * (np.abs(b1) @ np.abs(b2).T))


def test_two_runs_rows_and_views_agree_to_the_bit():
    tile, cells = core.gram_tile(), core.gram_cells(1)
    nt, n = tile + 40, cells + 77  # (an odd row length: every other row is off the 16-byte grid)
    for dtype in (F64, F32):
        y, c, s = _normal(5, nt, n, dtype)
        yd, cd, sd = _dev(y), _dev(c), _dev(s)
        G = _host(core.time_gram(yd, None, cd, None, sd))
        assert np.array_equal(_bits(G), _bits(G.T.copy()))
        assert np.array_equal(_bits(G), _bits(_host(core.time_gram(yd, None, cd, None, sd))))
        # a block of rows alone: the same bits as its block of the whole record's G
        sub = _host(core.time_gram(yd[5:37], None, cd, None, sd))
        assert np.array_equal(_bits(sub), _bits(G[5:37, 5:37]))
        # ... and the cross form of two blocks of rows: the same bits again
        cross = _host(core.time_gram(yd[5:37], yd[tile - 3:tile + 30], cd, cd, sd))
        assert np.array_equal(_bits(cross), _bits(G[5:37, tile - 3:tile + 30]))
        # operands that start one element into a larger buffer
        big = torch.empty(nt * n + 1, dtype=yd.dtype, device="cuda")
        big[1:] = yd.reshape(-1)
        cbig = torch.empty(n + 1, dtype=torch.float64, device="cuda")
        cbig[1:] = cd
        sbig = torch.empty(n + 1, dtype=torch.float64, device="cuda")
        sbig[1:] = sd
        view = big[1:].reshape(nt, n)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        off = _host(core.time_gram(view, None, cbig[1:], None, sbig[1:]))
        assert np.array_equal(_bits(off), _bits(G))


def test_excluded_cells_change_nothing_and_a_nan_poisons_its_row_and_column():
    tile, cells = core.gram_tile(), core.gram_cells(1)
    nt, n = tile + 3, cells + 5
    y, c, s = _normal(6, nt, n)
    G = _gram(y, None, c, None, s)
    assert np.isfinite(G).all()
    dirty = y.copy()
    out = np.isnan(c) | np.isnan(s)
    assert out.sum() > 20
    dirty[:, out] = np.where(np.arange(out.sum()) % 2 == 0, np.nan, np.inf)[None, :]
    dirty[::3, out] = -np.inf
    assert np.array_equal(_bits(_gram(dirty, None, c, None, s)), _bits(G))
    y2, c2, _ = _normal(7, 19, n)
    X = _gram(y, y2, c, c2, s)
    out2 = out | np.isnan(c2)
    dirty2 = y2.copy()
    dirty2[:, out2] = np.nan
    dirty[:, out2] = np.inf
    assert np.isfinite(X).all() and np.array_equal(_bits(_gram(dirty, dirty2, c, c2, s)), _bits(X))
    # a NaN at an included cell: exactly its row and column
    cell = int(np.flatnonzero(~out)[11])
    bad = y.copy()
    bad[tile + 1, cell] = np.nan
    P = _gram(bad, None, c, None, s)
    want = np.zeros((nt, nt), bool)
    want[tile + 1, :] = want[:, tile + 1] = True
    assert np.array_equal(np.isnan(P), want)
    assert np.array_equal(_bits(P[~want]), _bits(G[~want]))
    Xb = _gram(bad, y2, c, c2, s)
    cell_ok = ~np.isnan(c2[cell])
    assert np.array_equal(np.isnan(Xb).any(axis=1), (np.arange(nt) == tile + 1) & cell_ok)


# ---- refusals -----------------------------------------------------------------------------------------
def test_every_argument_error_is_raised():
    lib = _lib.load_eof()
    for kw, code in REFUSALS:
        assert gram_call(lib, **kw) == code and _lib.last_error(), kw
    y = torch.zeros((4, 6), dtype=torch.float64, device="cuda")
    with pytest.raises(TypeError):
        core.time_gram(y.cpu())
    with pytest.raises(ValueError, match="cells"):
        core.time_gram(y, torch.zeros((4, 7), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="center2"):
        core.time_gram(y, None, None, torch.zeros(6, dtype=torch.float64, device="cuda"))
    with pytest.raises(TypeError, match="float64"):
        core.time_gram(y, None, torch.zeros(6, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="6 elements"):
        core.time_gram(y, None, None, None, torch.zeros(5, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="contiguous"):
        core.time_gram(y, None, torch.zeros(12, dtype=torch.float64, device="cuda")[::2])
