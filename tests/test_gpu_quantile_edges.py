"""GPU: the quantile kernels (core.time_quantile / core.time_exceed_count;
csrc/momlevel_quantile.hip) at the edges of their geometry and of their keys.

Shapes are a few thousand cells at the most; block and unroll come from the library's own queries
(core.quantile_block_cells, core.quantile_unroll).  Gates, none taken from what the kernel gives:
float64 results are value-identical to tests/quantile_numpy.py (numpy.sort per column plus numpy's
lerp; bit-identical wherever the result is neither NaN nor zero -- the sign of a zero result is the
one freedom the contract leaves); float32 results are that float64 result rounded once; counts are
equal as int64.
"""

import numpy as np
import pytest
import torch

import quantile_numpy as qn
from momlevel_amd import core

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = (np.float64, np.float32)
LEVELS = (0.0, 0.5, 1.0 / 3.0, 0.99, 1.0)


def _pack(dtype):
    return 16 // np.dtype(dtype).itemsize


def _place(y, off=0):
    """the record on the device, its base ``off`` elements into a 16-byte aligned buffer"""
    rows, n = y.shape
    flat = torch.from_numpy(np.ascontiguousarray(y).reshape(-1))
    buf = torch.zeros(rows * n + 4, dtype=flat.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[off:off + rows * n] = flat.to(DEV)
    return buf[off:off + rows * n].view(rows, n)


def _quantile(y, q, steps=None, offsets=None, off=0):
    return core.time_quantile(_place(y, off), q, steps, offsets).cpu().numpy()


def _check(y, q, steps=None, offsets=None, off=0, what=""):
    got = _quantile(y, q, steps, offsets, off)
    want = qn.time_quantile(y, q, steps, offsets)
    if y.dtype == np.float32:
        want = qn.rounded_once(want)
    qn.assert_values(got, want, f"{what} {y.dtype.name} {y.shape} off={off}")
    return got


def _field(nt, n, dtype, seed, nan=0.3):
    rng = np.random.default_rng(seed)
    y = rng.normal(0.0, 1.0, (nt, n))
    y[rng.random((nt, n)) < nan] = np.nan
    return y.astype(dtype)


def _cells(dtype):
    pack, block = _pack(dtype), core.quantile_block_cells(dtype)
    assert block == 256 * pack or block % (64 * pack) == 0
    return (1, 2, 3, 5, pack * 64 - 1, pack * 64 + 1, block + 1, 3 * block + 3)


# ---- cells and steps -------------------------------------------------------------------------------
@pytest.mark.parametrize("off", (0, 1), ids=("aligned", "off-by-one"))
@pytest.mark.parametrize("dtype", DTYPES, ids=("float64", "float32"))
def test_cell_counts_at_both_alignments(dtype, off):
    nt = 2 * core.quantile_unroll() + 5
    for n in _cells(dtype):
        y = _field(nt, n, dtype, 100 + n)
        got = _check(y, [0.0, 0.5, 0.99], off=off, what=f"n={n}")
        assert got.shape == (3, 1, n) and got.dtype == y.dtype
        thr = got[1].astype(np.float64)  # the medians: a threshold that sits on sample values
        cnt = core.time_exceed_count(_place(y, off), torch.from_numpy(thr).to(DEV)).cpu().numpy()
        assert cnt.dtype == np.int64 and np.array_equal(cnt, qn.exceed_count(y, thr)), f"n={n}"


@pytest.mark.parametrize("off", (0, 1), ids=("aligned", "off-by-one"))
@pytest.mark.parametrize("dtype", DTYPES, ids=("float64", "float32"))
def test_record_lengths_around_the_unroll(dtype, off):
    U = core.quantile_unroll()
    for nt in sorted({1, 2, 3, U - 1, U, U + 1, 2 * U + 1, 300} - {0}):
        y = _field(nt, 40, dtype, 200 + nt, nan=0.2)
        _check(y, LEVELS, off=off, what=f"nt={nt}")


@pytest.mark.parametrize("dtype", DTYPES, ids=("float64", "float32"))
def test_nan_patterns(dtype):
    nt, n = 19, 48
    rng = np.random.default_rng(3)
    y = rng.normal(0.0, 1.0, (nt, n))
    y[:, 8:16] = np.nan                                  # all
    y[:, 16:24] = np.nan                                 # all but one
    y[rng.integers(0, nt, 8), np.arange(16, 24)] = rng.normal(0.0, 1.0, 8)
    y[:, 24:36][rng.random((nt, 12)) < 0.3] = np.nan     # random 30 %
    y[:, 36:48:2] = np.nan                               # land and wet cells inside one pack
    y[:, 41] = np.nan
    y = y.astype(dtype)
    for off in (0, 1):
        got = _check(y, LEVELS, off=off, what="NaN patterns")
        assert np.isnan(got[:, 0, 8:16]).all() and not np.isnan(got[:, 0, :8]).any()
        assert np.array_equal(got[0, 0, 16:24], got[4, 0, 16:24])  # one valid step: every q is it
        assert np.isnan(got[:, 0, 36:48:2]).all() and not np.isnan(got[:, 0, 37]).any()


# ---- the keys --------------------------------------------------------------------------------------
def _ladders(dtype, nt=40):
    """For every digit position of the key a column whose values agree above that digit and differ
    at it and below, at both signs; then columns that differ only in sign and exponent."""
    bits = np.dtype(dtype).itemsize * 8
    kind = np.uint64 if bits == 64 else np.uint32
    rng = np.random.default_rng(bits)
    base = np.array([1.2345678901234567], dtype=dtype).view(kind)[0]
    cols = []
    for p in range(bits // 4):
        low = bits - 4 * p  # the bits of digit p and below
        mask = kind((1 << low) - 1) if low < bits else kind(2 ** bits - 1)
        rnd = rng.integers(0, 2 ** bits, nt, dtype=np.uint64)
        pattern = (base & ~mask) | (rnd.astype(kind) & mask)
        cols.append(pattern)
        cols.append(pattern ^ kind(1 << (bits - 1)))  # the other sign
    mant_bits = 52 if bits == 64 else 23
    emax = (1 << (bits - 1 - mant_bits)) - 1  # the all-ones exponent: left out
    for _ in range(4):
        sign = rng.integers(0, 2, nt).astype(kind) << kind(bits - 1)
        expo = rng.integers(0, emax, nt).astype(kind) << kind(mant_bits)
        cols.append(sign | expo | (base & kind((1 << mant_bits) - 1)))
    return np.stack(cols, axis=1).view(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=("float64", "float32"))
def test_digit_ladders(dtype):
    y = _ladders(dtype)
    ndigits = np.dtype(dtype).itemsize * 2
    assert y.shape == (40, 2 * ndigits + 4)
    valid = ~np.isnan(y)
    assert valid[:, 2:].all() and valid.sum(axis=0).min() >= 30
    for p in (1, ndigits - 1):  # agree above the digit, differ at it
        k = y[:, 2 * p].view(np.uint64 if ndigits == 16 else np.uint32)
        shift = 4 * (ndigits - p)
        assert len(set((k >> shift).tolist())) == 1 and len(set((k >> (shift - 4)).tolist())) > 1
    for off in (0, 1):
        _check(y, LEVELS + (0.25, 0.75), off=off, what="digit ladders")


@pytest.mark.parametrize("dtype", DTYPES, ids=("float64", "float32"))
def test_special_values_and_heavy_ties(dtype):
    info = np.finfo(dtype)
    tiny = np.array([info.smallest_subnormal], dtype=dtype)[0]
    pool = np.array([0.0, -0.0, tiny, -tiny, 3 * tiny, info.tiny, -info.tiny, np.inf, -np.inf,
                     info.max, -info.max, 1.0, -1.0, np.nan], dtype=dtype)
    rng = np.random.default_rng(9)
    nt, n = 33, 24
    y = pool[rng.integers(0, pool.size, (nt, n))]
    y[:, 0] = np.where(rng.random(nt) < 0.5, 0.0, -0.0)        # only zeros
    y[:, 1] = pool[rng.integers(2, 5, nt)]                      # only subnormals
    y[:, 2] = np.where(rng.random(nt) < 0.5, np.inf, info.max)  # a == b == inf gives numpy's NaN
    y[:, 3] = np.inf
    y[:, 4] = -np.inf
    y[:, 5] = np.where(rng.random(nt) < 0.9, 1.0, -1.0)        # heavy ties: the closing pass, b = a
    y[:, 6] = 1.0
    y[:, 7] = rng.integers(0, 3, nt)
    y = y.astype(dtype)
    for off in (0, 1):
        got = _check(y, LEVELS + (0.1, 0.9), off=off, what="special values")
        assert (got[:, 0, 0] == 0).all() and np.isnan(got[:, 0, 3]).all() and (got[:, 0, 6] == 1).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=("float64", "float32"))
def test_levels(dtype):
    nt, n = 11, 12
    y = _field(nt, n, dtype, 11, nan=0.0)
    y[5:, 4:8] = np.nan       # c = 5
    y[10:, 8:] = np.nan       # c = 10
    # g = 0 exactly at k / (c - 1); g on both sides of 0.5 at c = 5: q = 0.1 and 0.15
    nine = [0.0, 0.1, 0.15, 0.25, 1.0 / 3.0, 0.5, 0.7, 0.99, 1.0]
    assert len(nine) > 8  # two launches
    got = _check(y, nine, what="nine levels")
    assert got.shape == (9, 1, n)
    s = np.sort(y[:5, 4:8].astype(np.float64), axis=0)
    assert np.array_equal(got[3, 0, 4:8].astype(np.float64), s[1])  # q = 1/4, c = 5: the 2nd smallest
    assert np.array_equal(got[6, 0, :4].astype(np.float64),
                          np.sort(y[:, :4].astype(np.float64), axis=0)[7])  # q = 0.7, c = 11
    for q in nine:
        one = _check(y, q, what=f"q={q}")
        assert np.array_equal(one[0], got[nine.index(q)], equal_nan=True)
    out = torch.empty((9, 1, n), dtype=torch.from_numpy(y).dtype, device=DEV)
    assert core.time_quantile(_place(y), nine, out=out) is out
    assert np.array_equal(out.cpu().numpy(), got, equal_nan=True)


# ---- groups ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("float64", "float32"))
def test_groups(dtype):
    nt, n = 60, 2 * core.quantile_block_cells(dtype) + 4
    y = _field(nt, n, dtype, 60, nan=0.1)
    y[:, 3] = np.nan
    rng = np.random.default_rng(61)
    members = [rng.permutation(nt)[:17],             # unordered
               np.array([4, 9, 4, 4, 30, 9]),        # a step listed more than once
               np.arange(10, 40), np.arange(25, 60),  # overlapping
               np.array([], dtype=np.int64),         # empty: a NaN row
               np.array([59]),                       # one step
               np.arange(nt)]
    steps = np.concatenate(members).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int64)
    for off in (0, 1):
        got = _check(y, [0.5, 0.9], steps, offsets, off=off, what="groups")
        assert got.shape == (2, len(members), n) and np.isnan(got[:, 4]).all()
        plain = _quantile(y, [0.5, 0.9], off=off)
        listed = _quantile(y, [0.5, 0.9], np.arange(nt), [0, nt], off=off)
        assert plain.tobytes() == listed.tobytes() == got[:, 6:7].tobytes(), "NULL lists"
    dup = qn.time_quantile(y, 0.5, [4, 9, 4, 4, 30, 9], [0, 6])
    once = qn.time_quantile(y, 0.5, [4, 9, 30], [0, 3])
    assert not qn.values_equal(dup, once)  # (the duplicates count)
    groups = core.upload_groups(steps, offsets, nt, DEV)
    again = core.time_quantile(_place(y), [0.5, 0.9], groups).cpu().numpy()
    assert again.tobytes() == _quantile(y, [0.5, 0.9], steps, offsets).tobytes()
    thr = qn.time_quantile(y, 0.9, steps, offsets)[0]
    cnt = core.time_exceed_count(_place(y), torch.from_numpy(thr).to(DEV), groups).cpu().numpy()
    assert np.array_equal(cnt, qn.exceed_count(y, thr, steps, offsets)) and not cnt[4].any()


@pytest.mark.parametrize("dtype", DTYPES, ids=("float64", "float32"))
def test_splitting_the_cells_changes_no_bit(dtype):
    block = core.quantile_block_cells(dtype)
    nt, n = 25, block + 38
    y = _field(nt, n, dtype, 77)
    whole = _quantile(y, LEVELS)
    for k in (1, 37, block):
        parts = np.concatenate([_quantile(y[:, :k], LEVELS), _quantile(y[:, k:], LEVELS)], axis=2)
        assert parts.tobytes() == whole.tobytes(), f"split at {k}"


# ---- counts ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("float64", "float32"))
def test_exceed_count(dtype):
    nt, n = 45, core.quantile_block_cells(dtype) + 6
    y = _field(nt, n, dtype, 45, nan=0.2)
    y[:, 2] = np.nan
    y[:, 5] = np.inf
    rng = np.random.default_rng(46)
    thr = rng.normal(0.0, 0.5, (1, n))
    pick = rng.integers(0, nt, n)
    own = y[pick, np.arange(n)].astype(np.float64)  # thresholds equal to sample values: strictness
    thr[0, ::3] = own[::3]
    thr[0, 7] = np.nan
    thr[0, 9] = -np.inf
    thr[0, 11] = np.inf
    want = qn.exceed_count(y, thr)
    assert want[0, 2] == 0 and want[0, 7] == 0 and want[0, 11] == 0
    assert want[0, 9] == np.sum(~np.isnan(y[:, 9]))
    for off in (0, 1):
        got = core.time_exceed_count(_place(y, off), torch.from_numpy(thr).to(DEV))
        assert got.dtype == torch.int64 and got.shape == (1, n) and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want), f"off={off}"
    got32 = core.time_exceed_count(_place(y), torch.from_numpy(thr.astype(np.float32)).to(DEV))
    assert np.array_equal(got32.cpu().numpy(), qn.exceed_count(y, thr.astype(np.float32)))
    # 8 cells fill a pack; a threshold 8 bytes off a 16-byte boundary takes the one-cell kernel: its
    # counts are the aligned ones
    y8, thr8 = np.ascontiguousarray(y[:, :8]), np.ascontiguousarray(thr[:, :8])
    buf = torch.zeros(8 + 2, dtype=torch.float64, device=DEV)
    buf[1:9] = torch.from_numpy(thr8[0]).to(DEV)
    shifted = buf[1:9].view(1, 8)
    assert buf.data_ptr() % 16 == 0 and shifted.data_ptr() == buf.data_ptr() + 8
    aligned = core.time_exceed_count(_place(y8), torch.from_numpy(thr8).to(DEV)).cpu().numpy()
    assert np.array_equal(aligned, qn.exceed_count(y8, thr8)) and aligned.any()
    assert core.time_exceed_count(_place(y8), shifted).cpu().numpy().tobytes() == aligned.tobytes()
    with pytest.raises(ValueError):
        core.time_exceed_count(_place(y), torch.zeros((2, n), dtype=torch.float64, device=DEV))
