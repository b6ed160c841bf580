"""GPU: core.time_gram (csrc/momlevel_eof.hip) where every real grid runs it -- past
GRAM_MAX_SPLIT * gram_cells(1) cells, where a block's range GROWS with n and there are always exactly
GRAM_MAX_SPLIT of them.  tests/test_gpu_eof_gram.py pins the kernel at the minimum range (at most four
ranges of gram_cells(1) cells); this file pins what that leaves open: k_gram_partial with ranges
longer than the minimum, the short last range of the grown regime and its short last chunk,
k_gram_finish adding GRAM_MAX_SPLIT partials an element, and the (range * npairs + pair) workspace
index with GRAM_MAX_SPLIT ranges times several tile pairs.

The yardsticks are those of tests/test_gpu_eof_gram.py, whose helpers are used as they stand.  EXACT
CASES: integer data with |y - center| <= 2^9, scale in {1, 2, 4} and n <= 2^20 -- products <= 2^22,
every partial sum in any order an integer below 2^42 < 2^53 -- so the assertion is BIT EQUALITY with
the host's float64 matmul of the same integers.  FLOAT CASE: |G - B @ B.T| <= 2 (n + 2) 2^-53
|B| @ |B|.T elementwise.  Every size asserts, through ``_plan``, that it IS in the grown regime: a
later change of MLX_GRAM_MAX_SPLIT or of the minimum range cannot silently move these tests back
into the minimum one."""

import numpy as np
import pytest
import torch

import eof_numpy as en
from momlevel_amd import _lib, core
from test_gpu_eof_gram import _bits, _dev, _exact, _gram, _host, _ints, _maps, _normal

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
CHUNK = 16  # cells per LDS stage of k_gram_partial: a range is a multiple of it (include/momlevel_eof.h)


def _ceil_div(a, b):
    return -(-a // b)


def _plan(n, grown=True):
    """(cells, ranges, cells of the last range) of a call over ``n`` cells, from the formula of
    include/momlevel_eof.h and checked against the library; ``grown``: the range is longer than the
    minimum one and there are exactly GRAM_MAX_SPLIT ranges"""
    split, base = _lib.GRAM_MAX_SPLIT, core.gram_cells(1)
    cells = max(base, _ceil_div(_ceil_div(n, split), CHUNK) * CHUNK)
    assert core.gram_cells(n) == cells
    ranges = _ceil_div(n, cells)
    assert ranges == split, (n, ranges)
    if grown:
        assert cells > base, (n, cells)
    return cells, ranges, n - (ranges - 1) * cells


def _sizes():
    """name -> (n, cells, cells of the last range), n computed from the library's constants"""
    split, base = _lib.GRAM_MAX_SPLIT, core.gram_cells(1)
    top = 1 << 20  # the largest n of the exactness argument
    assert top % (split * CHUNK) == 0 and top // split > base
    return {
        "split*base": (split * base, base, base),  # the last n of the minimum regime
        "split*base+1": (split * base + 1, base + CHUNK, base + 1 - CHUNK * (split - 1)),
        "split*(base+16)": (split * (base + CHUNK), base + CHUNK, base + CHUNK),
        "split*(base+16)+1": (split * (base + CHUNK) + 1, base + 2 * CHUNK,
                              base + CHUNK + 1 - CHUNK * (split - 1)),
        "2^20-1": (top - 1, top // split, top // split - 1),
        "2^20": (top, top // split, top // split),
    }


NEAR = ["split*base", "split*base+1", "split*(base+16)", "split*(base+16)+1"]
FAR = ["2^20-1", "2^20"]


def _n(name):
    n, cells, last = _sizes()[name]
    assert _plan(n, grown=name != "split*base") == (cells, _lib.GRAM_MAX_SPLIT, last), name
    if name == "split*base+1":
        assert last % CHUNK == 1  # (the last chunk of the last range holds one cell)
    return n


# ---- exact cases ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n_name", NEAR + FAR)
def test_symmetric_form_is_exact_on_integers_in_grown_ranges(n_name, dtype):
    """one record of the most rows a size is run with; its leading rows are the shorter records (the
    expected G of integers is exact, so a block of it is the expected G of the block's rows)"""
    tile, n = core.gram_tile(), _n(n_name)
    nts = [3, 17] if n_name in FAR else [17, tile + 1, 2 * tile + 5]  # 1, 3 and 6 tile pairs
    rng = np.random.default_rng(500 + (NEAR + FAR).index(n_name))
    c1, _, s = _maps(rng, n)
    y = _ints(rng, max(nts), n, dtype, np.where(np.isnan(c1), 0.0, c1))
    ref = _exact(y, None, c1, None, s)
    # _exact's int64 cross-check needs ref.size * n <= 2^22, which no record here meets: two rows do
    few = en.weighted(y[:2], c1, s).astype(np.int64)
    assert few.shape[0] ** 2 * n <= 1 << 22 and np.array_equal(few @ few.T, ref[:2, :2].astype(np.int64))
    yd, cd, sd = _dev(y), _dev(c1), _dev(s)
    for nt in nts:
        got = _host(core.time_gram(yd[:nt], None, cd, None, sd))
        assert got.shape == (nt, nt) and got.dtype == F64
        assert np.array_equal(_bits(got), _bits(ref[:nt, :nt])), (nt, n)
        assert np.array_equal(_bits(got), _bits(got.T.copy()))


@pytest.mark.parametrize("dtypes", [(F64, F64), (F32, F32), (F64, F32), (F32, F64)],
                         ids=["f64xf64", "f32xf32", "f64xf32", "f32xf64"])
@pytest.mark.parametrize("n_name", ["split*base+1", "split*(base+16)+1"])
def test_cross_form_is_exact_on_integers_in_grown_ranges(n_name, dtypes):
    tile, n = core.gram_tile(), _n(n_name)
    for k, (nt1, nt2) in enumerate(((tile + 9, 37), (21, 2 * tile + 5))):
        rng = np.random.default_rng(900 + 10 * NEAR.index(n_name) + k)
        c1, c2, s = _maps(rng, n)
        y1 = _ints(rng, nt1, n, dtypes[0], np.where(np.isnan(c1), 0.0, c1))
        y2 = _ints(rng, nt2, n, dtypes[1], np.where(np.isnan(c2), 0.0, c2))
        got = _gram(y1, y2, c1, c2, s)
        assert got.shape == (nt1, nt2)
        assert np.array_equal(_bits(got), _bits(_exact(y1, y2, c1, c2, s))), (nt1, nt2, n)


@pytest.mark.parametrize("dtypes", [(F64, F64), (F32, F64), (F64, F32)],
                         ids=["f64xf64", "f32xf64", "f64xf32"])
def test_cross_form_keeps_rows_and_columns_apart_in_grown_ranges(dtypes):
    """the residue construction of tests/test_gpu_eof_gram.py: y1[s, c] = (s + 1) [c = s mod 5], so
    G[s, t] is (s + 1) times the sum of y2[t] over one residue -- different in every row AND column"""
    tile, n = core.gram_tile(), _n("split*base+1")
    nt1, nt2 = tile + 9, 37
    s_idx, c_idx = np.arange(nt1)[:, None], np.arange(n)[None, :]
    y1 = ((s_idx + 1) * (c_idx % 5 == s_idx % 5)).astype(dtypes[0])
    t_idx = np.arange(nt2)[:, None]
    y2 = ((3 * t_idx + 1) * ((c_idx % 7) + 1) - (c_idx % 3) * t_idx * t_idx % 11).astype(dtypes[1])
    # products below 2^21 and n <= 2^17: every sum an integer below 2^38
    assert np.abs(y1).max() <= 512 and np.abs(y2).max() <= 2 ** 12 and n <= 1 << 17
    by_residue = np.stack([y2[:, r::5].astype(np.int64).sum(axis=1) for r in range(5)])  # (5, nt2)
    ref = (np.arange(nt1, dtype=np.int64)[:, None] + 1) * by_residue[np.arange(nt1) % 5]
    assert not np.array_equal(ref[:21, :21], ref[:21, :21].T)
    assert np.array_equal(_gram(y1, y2), ref.astype(F64)), (nt1, nt2, n)
    assert np.array_equal(_gram(y2, y1), ref.T.astype(F64)), (nt2, nt1, n)


# ---- invariants at a grown n, bit for bit -----------------------------------------------------------
def _seams(n):
    """cells on both sides of the first and the last range seam, and the last cell of all"""
    cells, ranges, last = _plan(n)
    assert last < cells and last % CHUNK != 0  # (a short last range with a short last chunk)
    return [cells - 1, cells, (ranges - 1) * cells - 1, (ranges - 1) * cells, n - 1]


@pytest.fixture(scope="module", params=[F64, F32], ids=["f64", "f32"])
def grown(request):
    """normal data at an odd grown n with a short last range; the maps EXCLUDE the five seam cells
    (``c``) or INCLUDE them (``c_in``, ``s_in``); the device copies and the clean G of each"""
    split, base, tile = _lib.GRAM_MAX_SPLIT, core.gram_cells(1), core.gram_tile()
    nt, n = tile + 40, split * (base + CHUNK) + 77  # (an odd row length)
    seams = _seams(n)
    y, c, s = _normal(15, nt, n, request.param)
    mean = y.astype(F64).mean(axis=0)
    c_in, s_in = c.copy(), s.copy()
    c_in[seams], s_in[seams] = mean[seams], 1.25
    s[seams] = s_in[seams]
    c[seams] = np.nan  # (excluded by the center alone)
    case = dict(nt=nt, n=n, tile=tile, seams=seams, y=y, c=c, s=s, c_in=c_in, s_in=s_in,
                yd=_dev(y), cd=_dev(c), sd=_dev(s), cd_in=_dev(c_in), sd_in=_dev(s_in))
    case["G"] = _host(core.time_gram(case["yd"], None, case["cd"], None, case["sd"]))
    case["G_in"] = _host(core.time_gram(case["yd"], None, case["cd_in"], None, case["sd_in"]))
    assert np.isfinite(case["G"]).all() and np.isfinite(case["G_in"]).all()
    assert not np.array_equal(case["G"], case["G_in"])  # (the seam cells do carry weight)
    return case


def test_two_runs_rows_and_views_agree_to_the_bit_in_grown_ranges(grown):
    g = grown
    nt, n, tile, yd, cd, sd, G = g["nt"], g["n"], g["tile"], g["yd"], g["cd"], g["sd"], g["G"]
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


def test_excluded_cells_at_the_range_seams_change_nothing(grown):
    g = grown
    out = np.isnan(g["c"]) | np.isnan(g["s"])
    assert out[g["seams"]].all() and out.sum() > 20
    dirty = g["y"].copy()
    dirty[:, out] = np.where(np.arange(out.sum()) % 2 == 0, np.nan, np.inf)[None, :]
    dirty[::3, out] = -np.inf
    assert not np.isfinite(dirty[:, g["seams"]]).any()
    got = _host(core.time_gram(_dev(dirty), None, g["cd"], None, g["sd"]))
    assert np.array_equal(_bits(got), _bits(g["G"]))


def test_a_nan_at_an_included_seam_cell_poisons_its_row_and_column(grown):
    g = grown
    nt, tile, G = g["nt"], g["tile"], g["G_in"]
    first_of_range_1, last_of_range_30, last_cell = g["seams"][1], g["seams"][2], g["seams"][4]
    assert last_of_range_30 == (_lib.GRAM_MAX_SPLIT - 1) * core.gram_cells(g["n"]) - 1
    bad = g["yd"].clone()
    for row, cell in ((3, first_of_range_1), (tile + 1, last_of_range_30), (nt - 1, last_cell)):
        assert not np.isnan(g["c_in"][cell]) and not np.isnan(g["s_in"][cell])
        keep = bad[row, cell].clone()
        bad[row, cell] = float("nan")
        P = _host(core.time_gram(bad, None, g["cd_in"], None, g["sd_in"]))
        bad[row, cell] = keep
        want = np.zeros((nt, nt), bool)
        want[row, :] = want[:, row] = True
        assert np.array_equal(np.isnan(P), want), (row, cell)
        assert np.array_equal(_bits(P[~want]), _bits(G[~want])), (row, cell)
    assert np.array_equal(_host(bad), g["y"])  # (the record is whole again: nothing carried over)


def test_float_case_within_the_derived_bound_in_grown_ranges(grown):
    g = grown
    n = g["n"]
    for name, c, s in (("G", g["c"], g["s"]), ("G_in", g["c_in"], g["s_in"])):
        b = en.weighted(g["y"], c, s)
        ref, mag = b @ b.T, np.abs(b) @ np.abs(b).T
        bound = 2 * (n + 2) * 2.0 ** -53 * mag
        ratio = np.abs(g[name] - ref) / bound
        print(f"{g['y'].dtype.name}, n = {n}: worst |G - B@B.T| / bound = {ratio.max():.3e}")
        assert np.all(np.abs(g[name] - ref) <= bound)
