"""GPU: the reduction and helper kernels of csrc/momlevel_hip.hip (and the area finish and the
gauge gather) past one block -- core.nansum, core.masso, K1's row reduction, core.area_mean,
core.group_weighted_mean, core.gauge_gather -- at the row lengths, plane sizes and alignments at
which they take another path.

These kernels ADD numbers, so the operands are INTEGER VALUED: every partial sum is then exact in
float64 whatever order a kernel adds in, the expected value is computed in numpy.int64 / Python int
on the host, and the assertion is bit equality -- a dropped, doubled or misplaced element cannot
hide behind a tolerance.  Each such case asserts what makes it exact: sum(|terms|) < 2**53.

Where the order is fixed by the kernel (group_weighted_mean) the operands are real valued and the
reference is numpy in that order; where a density is summed (K1 on a tall column) the one-hot
``vol0`` of test_gpu_wright.py carries one cell's density through the reduction bit for bit, and a
random ``vol0`` meets math.fsum at the 1e-12 gate that test_gpu_wright.py and test_gpu_kernels.py
use for the same sum.  No reference comes from the kernel under test or another of the project's
kernels; every input is drawn from a fixed seed.
"""

import math

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal
from momlevel_amd import _lib, core
from oracle import momlevel_numpy as o

pytestmark = pytest.mark.gpu

DEV = "cuda"
EXACT = 1 << 53  # integers below it, and sums of them that stay below it, are exact in float64
F64, F32 = np.float64, np.float32
NAN = float("nan")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _shifted(t):
    """``t``'s elements one element into a padded buffer: the same values off a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and buf.data_ptr() % 16 == 0
    assert out.data_ptr() == buf.data_ptr() + t.element_size()
    return out


# ---- 1. core.nansum: k_nansum_partial's two twins and k_reduce_rows ----------------------------------
# mlx_nansum gives a block 2048 elements up to 8192 blocks, then the blocks stride; k_reduce_rows adds
# the nb = ceil(n / 2048) partials: thread i the partials i, i + 256, ..., eight at a time while
# i + 7 * 256 < nb.  So no thread unrolls below nb = 1793, threads 0 .. nb - 1793 do at 1793 .. 2047,
# all do at 2048, thread 0 leaves the unrolled body for a one-element tail at 2049 and takes a
# second trip at 3841; 255 / 256 / 257 are the edges of the plain loop's first step.
# n = 2048 * nb is even (the 16-byte twin on an aligned array), n - 1 is odd (the scalar twin, the
# last block one element short); an even n one element into a padded buffer is the scalar twin too.
CHUNK, CAP = 2048, 8192
NBS = (1, 2, 255, 256, 257, 1792, 1793, 2047, 2048, 2049, 3841, 8191, 8192)
N_OVER = CAP * CHUNK + 3 * CHUNK + 1  # past the cap: the blocks stride, some for one more trip
NAN_RUN = 4096
NANSUM_CASES = ([(CHUNK * nb - odd, "aligned") for nb in NBS for odd in (0, 1)]
                + [(N_OVER - 1, "aligned"), (N_OVER, "aligned")]
                + [(CHUNK * nb, "offset") for nb in (257, 1793, 2049)])


class _Master:
    """N_OVER integer values with about 3 % NaN, on the device once; a case sums a prefix of it.
    ``sums`` / ``mags``: exclusive prefix sums (int64) of the values and of their magnitudes, NaN
    counting 0.  pattern "ones": every value 1.0 under the same NaN mask -- the sum is the count."""

    def __init__(self, pattern):
        rng = np.random.default_rng(20261019)
        vals = rng.integers(-(1 << 20), 1 << 20, N_OVER, dtype=np.int64)
        nan = rng.random(N_OVER) < 0.03
        if pattern == "ones":
            vals[:] = 1
        vals[nan] = 0
        self.sums = np.concatenate([[0], np.cumsum(vals)])
        self.mags = np.concatenate([[0], np.cumsum(np.abs(vals))])
        assert self.sums.dtype == np.int64 and int(self.mags[-1]) < EXACT
        x = vals.astype(F64)
        x[nan] = NAN
        self.pattern, self.nan = pattern, nan
        self.dev = _dev(x)

    def total(self, n, s, e):
        """(sum, sum of magnitudes) of the first ``n`` values without those in [s, e), as ints"""
        return (int(self.sums[n]) - int(self.sums[e] - self.sums[s]),
                int(self.mags[n]) - int(self.mags[e] - self.mags[s]))


@pytest.fixture(scope="module", params=["ints", "ones"])
def master(request):
    m = _Master(request.param)
    yield m
    m.dev = None
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n, placement", NANSUM_CASES,
                         ids=[f"{n}-{p}" for n, p in NANSUM_CASES])
def test_nansum_is_the_integer_sum(master, n, placement):
    """the first n values, with a run of NAN_RUN consecutive NaNs from n // 3 on (cut at the end of
    an array that short): the int64 sum of the rest, bit for bit"""
    s, e = n // 3, min(n // 3 + NAN_RUN, n)
    want, mag = master.total(n, s, e)
    assert mag < EXACT
    x = master.dev
    saved = x[s:e].clone()
    x[s:e] = NAN
    try:
        view = x[:n] if placement == "aligned" else _shifted(x[:n])
        # which twin: k_nansum_partial<true> needs an even n on a 16-byte boundary
        packed = n % 2 == 0 and view.data_ptr() % 16 == 0
        assert packed == (placement == "aligned" and n % 2 == 0)
        got = core.nansum(view).cpu().numpy()
    finally:
        x[s:e] = saved
    assert got.dtype == F64 and got.shape == ()
    assert_bit_equal(got, F64(want), f"nansum n={n} {placement}")
    if master.pattern == "ones":  # the sum of ones is the count of the values left
        left = ~master.nan[:n]
        left[s:e] = False
        assert want == int(left.sum())


@pytest.mark.parametrize("n", [CHUNK * 257, CHUNK * 257 - 1, 1])
def test_nansum_of_nothing_is_plus_zero(n):
    got = core.nansum(torch.full((n,), NAN, dtype=torch.float64, device=DEV)).cpu().numpy()
    assert_bit_equal(got, F64(0.0), f"all NaN, n={n}")


# ---- 2. core.masso: k_masso_partial, vol per step or shared -------------------------------------------
MASSO_N3 = (1, 255, 257, 2049, 1793 * 2048 - 5)  # the last: 1793 partials a row, the blocks stride


def _masso_case(n3, vol_per_step, nt=3, dead_step=None):
    rng = np.random.default_rng(n3 + vol_per_step)
    rho_i = rng.integers(1000, 1100, (nt, n3), dtype=np.int64)
    vol_i = rng.integers(1, 1 << 16, (nt, n3) if vol_per_step else (n3,), dtype=np.int64)
    rho_nan, vol_nan = rng.random(rho_i.shape) < 0.05, rng.random(vol_i.shape) < 0.05
    if dead_step is not None:
        (vol_nan if vol_per_step else rho_nan)[dead_step] = True
    terms = rho_i * vol_i
    terms[rho_nan | vol_nan] = 0
    assert int(np.abs(terms).sum(axis=1).max()) < EXACT
    rho, vol = rho_i.astype(F64), vol_i.astype(F64)
    rho[rho_nan], vol[vol_nan] = NAN, NAN
    return rho, vol, terms.sum(axis=1, dtype=np.int64)


@pytest.mark.parametrize("vol_per_step", [False, True], ids=["vol-shared", "vol-per-step"])
@pytest.mark.parametrize("n3", MASSO_N3)
def test_masso_is_the_integer_sum(n3, vol_per_step):
    rho, vol, want = _masso_case(n3, vol_per_step)
    got = core.masso(_dev(rho), _dev(vol)).cpu().numpy()
    assert_bit_equal(got, want.astype(F64), f"masso n3={n3}")
    assert n3 == 1 or (np.all(want > 0) and len(set(want.tolist())) == 3)


@pytest.mark.parametrize("vol_per_step", [False, True], ids=["vol-shared", "vol-per-step"])
@pytest.mark.parametrize("n3", [257, 2049])
def test_masso_of_an_all_nan_step_is_zero(n3, vol_per_step):
    """step 1 is NaN throughout -- in rho under a shared vol, in vol when it has steps"""
    rho, vol, want = _masso_case(n3, vol_per_step, dead_step=1)
    assert want[1] == 0 and want[0] > 0 and want[2] > 0
    got = core.masso(_dev(rho), _dev(vol)).cpu().numpy()
    assert_bit_equal(got, want.astype(F64), f"masso n3={n3}, step 1 all NaN")


# ---- 3. K1 on a tall column: a row of 2049 partials, one per level --------------------------------------
# (nz, ny, nx) = (2049, 1, nx): one block covers the plane, so gx = 1 and level z owns partial slot z
# of each row k_reduce_rows adds.  nx = 4 holds whole packs at either dtype: the fast kernels;
# nx = 3 the generic twin.
COL_NT, COL_NZ = 3, 2049
HOT_LEVELS = (0, 255, 256, 1791, 1792, 2047, 2048)
_columns = {}


def _column(nx, dtype):
    """(T, S, pres, [rho steric, rho with S held, rho with theta held]) of the column, from the
    oracle on the fields as stored"""
    if (nx, dtype) not in _columns:
        shape = (COL_NT, COL_NZ, 1, nx)
        r = np.random.default_rng(COL_NZ + nx)
        T, S = r.uniform(-2, 32, shape).astype(dtype), r.uniform(30, 40, shape).astype(dtype)
        pres = o.pressure_from_depth(np.linspace(1.0, 5000.0, COL_NZ))
        pb = pres[:, None, None]
        rho = [np.broadcast_to(o.wright_density(a, b, pb), shape)
               for a, b in ((T, S), (T, S[0]), (T[0], S))]
        assert all(x.dtype == F64 for x in rho)
        _columns[(nx, dtype)] = (T, S, pres, rho)
    return _columns[(nx, dtype)]


def _k1_launches(dT, dS, vol, pres, skip_dry, generic):
    """the all-variants launch and its three single-variant launches -> (rows (4, nt), singles)"""
    kw = dict(skip_dry=skip_dry, arith="exact")
    vol = _dev(vol)
    singles = []
    for a, b in ((dT, dS), (dT, dS[0]), (dT[0], dS)):
        singles.append(core.steric_global_masso(a, b, vol, pres, **kw).cpu().numpy())
        args = _lib.last_kernel().split("<")[1].split(",")
        assert args[5] == ("true" if generic else "false"), _lib.last_kernel()
    rows = core.steric_global_decomp(dT, dS, dT[0], dS[0], vol, pres, **kw).cpu().numpy()
    assert _lib.last_kernel().split("<")[1].split(",")[5] == ("true" if generic else "false")
    assert rows.shape == (4, COL_NT)
    return rows, singles


@pytest.mark.parametrize("skip_dry", [False, True], ids=["all-levels", "skip-dry"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [4, 3], ids=["fast", "generic"])
def test_k1_one_hot_level_comes_through_the_row_reduction(nx, dtype, skip_dry):
    """vol0 is 1.0 in one cell and NaN elsewhere: masso[t] is the oracle's rho of that cell, bit
    for bit, wherever its level's partial sits in the row of 2049 -- the first, the 256th and
    257th, the last the unrolled body takes and the first after it (1792), the row's one-element
    tail (2048).  Every other level is dry: its partial must be 0.0 whether or not the block skipped
    it.  Rows 0-2 of the decomposition are their single launches'; row 3 is theta of the cell."""
    T, S, pres, rho = _column(nx, dtype)
    dT, dS = _dev(T), _dev(S)
    for z in HOT_LEVELS:
        x = z % nx
        hot = np.full((COL_NZ, 1, nx), NAN)
        hot[z, 0, x] = 1.0
        rows, singles = _k1_launches(dT, dS, hot, pres, skip_dry, generic=nx == 3)
        assert_bit_equal(singles[0], rho[0][:, z, 0, x], f"masso, hot level {z}")
        for k, name in enumerate(("steric", "thermosteric", "halosteric")):
            assert_bit_equal(rows[k], singles[k], f"decomposition row {name}, hot level {z}")
            assert_bit_equal(singles[k], rho[k][:, z, 0, x], f"{name} against the oracle, level {z}")
        assert_bit_equal(rows[3], T[:, z, 0, x].astype(F64), f"heat row, hot level {z}")


@pytest.mark.parametrize("skip_dry", [False, True], ids=["all-levels", "skip-dry"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [4, 3], ids=["fast", "generic"])
def test_k1_tall_column_meets_fsum(nx, dtype, skip_dry):
    """a random vol0 with land cells and a band of dry levels: each row against math.fsum of the
    oracle's rho * vol0 terms (row 3: theta * vol0) at 1e-12 relative"""
    T, S, pres, rho = _column(nx, dtype)
    r = np.random.default_rng(7 * nx)
    vol = r.uniform(1e9, 1e12, (COL_NZ, 1, nx))
    vol[r.random(vol.shape) < 0.2] = NAN
    vol[1000:1100] = NAN
    rows, singles = _k1_launches(_dev(T), _dev(S), vol, pres, skip_dry, generic=nx == 3)
    wet = ~np.isnan(vol)
    worst = 0.0
    for k, field in enumerate(rho + [T.astype(F64)]):
        ref = np.array([math.fsum((field[t] * vol)[wet].tolist()) for t in range(COL_NT)])
        err = float(np.max(np.abs(rows[k] - ref) / np.abs(ref)))
        worst = max(worst, err)
        if k < 3:
            assert_bit_equal(rows[k], singles[k], f"decomposition row {k}")
    print(f"K1 column nx={nx} {np.dtype(dtype).name} skip_dry={skip_dry}: worst relative error "
          f"against fsum {worst:.3e} (gate 1e-12)")
    assert worst <= 1e-12


# ---- 4. core.area_mean past 256 tiles: k_area_finish's second and third step -----------------------------
@pytest.mark.parametrize("slots", [False, True], ids=["global", "three-slots"])
@pytest.mark.parametrize("vdt", [F64, F32], ids=["v64", "v32"])
def test_area_mean_over_513_tiles_is_the_integer_quotient(vdt, slots):
    """plane = 512 tiles and one cell: thread 0 of the finish adds tiles 0, 256 and 512, the last a
    tile of one (valid) cell.  v in [-1000, 1000] and area in [1, 1000] are integers, exact in
    float32 too: wsum is the int64 weight sum, the mean float64(num) / float64(den)."""
    tile = core.area_tile(vdt)
    nrec, plane = 2, 512 * tile + 1
    rng = np.random.default_rng(plane + slots)
    v_i = rng.integers(-1000, 1001, (nrec, plane), dtype=np.int64)
    a_i = rng.integers(1, 1001, plane, dtype=np.int64)
    v_nan = (rng.random((nrec, plane)) < 0.05) | (rng.random(plane) < 0.3)  # its own and land
    a_nan = rng.random(plane) < 0.05
    v_nan[:, -1], a_nan[-1] = False, False
    if slots:
        slot = rng.integers(-1, 3, plane).astype(np.int32)  # -1: in no region
        slot[-1] = 1
        v_nan[0, slot == 2] = True  # slot 2 has no valid cell in record 0
        regions = [slot == k for k in range(3)]
        assert (slot == -1).sum() > plane // 8
    else:
        v_nan[1] = True  # the second record is all NaN
        regions = [np.ones(plane, bool)]
    num, den = np.zeros((nrec, len(regions)), np.int64), np.zeros((nrec, len(regions)), np.int64)
    for k, inside in enumerate(regions):
        valid = ~v_nan & ~a_nan & inside
        num[:, k] = np.where(valid, v_i * a_i, 0).sum(axis=1)
        den[:, k] = np.where(valid, a_i, 0).sum(axis=1)
        assert int(np.where(valid, np.abs(v_i) * a_i, 0).sum(axis=1).max()) < EXACT
    with np.errstate(invalid="ignore"):
        mean = num.astype(F64) / np.where(den != 0, den, np.nan).astype(F64)
    nothing = (1, 0) if not slots else (0, 2)
    assert den[nothing] == 0 and np.isnan(mean[nothing]) and (den == 0).sum() == 1
    v = v_i.astype(vdt)
    v[v_nan] = NAN
    vd = _dev(v)
    sd = _dev(slot) if slots else None
    for adt in (F64, F32):
        area = a_i.astype(adt)
        area[a_nan] = NAN
        got_mean, got_den = core.area_mean(vd, _dev(area), sd, len(regions))
        what = f"{np.dtype(vdt).name} v, {np.dtype(adt).name} area, {len(regions)} slot(s)"
        assert_bit_equal(got_den.cpu().numpy(), den.astype(F64), "wsum, " + what)
        assert_bit_equal(got_mean.cpu().numpy(), mean, "mean, " + what)


# ---- 5. core.group_weighted_mean: the packed twin, its guard and its store --------------------------------
# mlx_group_weighted_mean takes k_group_weighted_mean<2> (a thread owns cells 2i, 2i + 1; 512 cells
# a block) when n is even and x and out sit on 16-byte boundaries, k_group_weighted_mean<1> (256
# cells a block) otherwise.  Of the sizes below 2, 512, 514, 1026, 1030 are even: one thread; one
# full block; two blocks, the second of one thread; three blocks, the last of one and of three
# threads.  1, 511, 513 are odd: the one-cell twin over one, two and three blocks.  An even n with x
# or out one element into a padded buffer is the one-cell twin on the same values.
GWM_N = (1, 2, 511, 512, 513, 514, 1026, 1030)


def _gwm_reference(x, w, group_len):
    """util.annual_average's arithmetic in the kernel's order: ascending j, the product rounded,
    then the sum (no np.sum over the axis: its order is another for a one-column array)"""
    ngroups = x.shape[0] // group_len
    out = np.empty((ngroups,) + x.shape[1:])
    for g in range(ngroups):
        num, den = np.zeros(x.shape[1:]), np.zeros(x.shape[1:])
        for j in range(g * group_len, (g + 1) * group_len):
            num += np.where(np.isnan(x[j]), 0.0, x[j]) * w[j]
            den += np.where(np.isnan(x[j]), 0.0, 1.0) * w[j]
        with np.errstate(invalid="ignore"):
            out[g] = num / np.where(den != 0.0, den, np.nan)
    return out


@pytest.mark.parametrize("n", GWM_N)
@pytest.mark.parametrize("ngroups", [1, 3])
@pytest.mark.parametrize("group_len", [1, 12, 13])
def test_group_weighted_mean_in_the_kernels_order(group_len, ngroups, n):
    """real-valued x with 10 % NaN, the last cell NaN throughout the first group, weights from
    {28, 29, 30, 31} and, when there are three groups, the second with weights of 0 (NaN: no
    weight at all)"""
    nt = group_len * ngroups
    rng = np.random.default_rng(1000 * group_len + 10 * ngroups + n)
    x = rng.normal(20.0, 5.0, (nt, n))
    x[rng.random((nt, n)) < 0.1] = NAN
    x[:group_len, n - 1] = NAN
    w = rng.choice([28.0, 29.0, 30.0, 31.0], nt)
    if ngroups == 3:
        w[group_len:2 * group_len] = 0.0
    want = _gwm_reference(x, w, group_len)
    assert np.isnan(want[0, n - 1]) and (ngroups == 1 or np.isnan(want[1]).all())
    xd, wd = _dev(x), _dev(w)
    assert xd.data_ptr() % 16 == 0
    out = torch.full((ngroups, n + 2), -7.0, dtype=torch.float64, device=DEV).reshape(-1)
    got = core.group_weighted_mean(xd, wd, group_len, out=out[:ngroups * n].view(ngroups, n))
    assert got.data_ptr() == out.data_ptr() and got.data_ptr() % 16 == 0
    assert bool((out[ngroups * n:] == -7.0).all()), "a store past the output"
    got = got.cpu().numpy()
    assert_bit_equal(got, want, f"L={group_len} G={ngroups} n={n}")
    if n % 2 == 0:  # the one-cell twin on the same values: x, then out, off the 16-byte boundary
        moved = core.group_weighted_mean(_shifted(xd), wd, group_len).cpu().numpy()
        assert_bit_equal(moved, got, "x one element into a padded buffer")
        buf = torch.full((ngroups * n + 2,), -7.0, dtype=torch.float64, device=DEV)
        into = buf[1:1 + ngroups * n].view(ngroups, n)
        assert into.data_ptr() % 16 == 8
        moved = core.group_weighted_mean(xd, wd, group_len, out=into).cpu().numpy()
        assert_bit_equal(moved, got, "out one element into a padded buffer")
        assert buf[0].item() == -7.0 and buf[-1].item() == -7.0, "a store beside the output"


# ---- 6. core.gauge_gather: more than one block of rows, more gauges than grid rows ------------------------
GATHER_N = 300
GATHER_CASES = [(1, 5), (255, 5), (256, 5), (257, 5), (600, 5), (3, 65535), (3, 65536), (3, 65539)]
CANONICAL = {F64: (np.uint64, 0x7FF8000000000000), F32: (np.uint32, 0x7FC00000)}


def _nan_payloads(rng, count, dtype):
    """``count`` NaN bit patterns of ``dtype``: quiet and signalling, either sign, random payloads"""
    uint, _ = CANONICAL[dtype]
    mant = 52 if dtype is F64 else 23
    width = 8 * uint().nbytes
    expo = ((1 << (width - 1 - mant)) - 1) << mant  # all exponent bits
    payload = rng.integers(1, 1 << (mant - 1), count, dtype=np.int64).astype(uint)
    quiet = (rng.integers(0, 2, count, dtype=np.int64).astype(uint)) << uint(mant - 1)
    sign = (rng.integers(0, 2, count, dtype=np.int64).astype(uint)) << uint(width - 1)
    return uint(expo) | payload | quiet | sign


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("nrest, ng", GATHER_CASES)
def test_gather_copies_bits_past_one_block_and_one_grid(nrest, ng, dtype):
    """out[g, r] = y[r, index[g]] on integer views (NaN payloads count); an index outside [0, n)
    -- -1, n, 2**40, also at positions 0, 65535, 65536 and the last -- gives a canonical NaN row.
    ng = 65536 and 65539 are past the 65535 rows of the grid: blocks walk on by gridDim.y."""
    uint, canonical = CANONICAL[dtype]
    rng = np.random.default_rng(nrest * 100003 + ng)
    y = rng.normal(0.0, 1.0, (nrest, GATHER_N)).astype(dtype)
    bits = y.view(uint)
    where = rng.random(bits.shape) < 0.1
    bits[where] = _nan_payloads(rng, int(where.sum()), dtype)
    assert np.isnan(y[where]).all() and not np.isnan(y[~where]).any()
    assert where.any() or nrest == 1
    index = rng.integers(0, GATHER_N, ng, dtype=np.int64)
    bad = rng.random(ng) < 0.05
    bad[[k for k in (0, 65535, 65536, ng - 1) if k < ng]] = True
    bad[1] = False  # (one valid row at the least)
    index[bad] = np.resize(np.array([-1, GATHER_N, 1 << 40], dtype=np.int64), int(bad.sum()))
    want = np.full((ng, nrest), canonical, dtype=uint)
    want[~bad] = bits[:, index[~bad]].T
    got = core.gauge_gather(_dev(y), index)
    assert got.shape == (ng, nrest)
    assert got.dtype == (torch.float64 if dtype is F64 else torch.float32)
    got = got.cpu().numpy().view(uint)
    differ = got != want
    assert not differ.any(), (f"{int(differ.sum())} of {want.size} elements differ, first at "
                              f"(gauge, row) {tuple(np.argwhere(differ)[0])}")
