"""GPU: the remap past one block of destinations (k_regrid, csrc/momlevel_regrid.hip) against
tests/regrid_numpy.py, BIT FOR BIT.  The other regrid suites stay below three slices of
destinations -- ``blockIdx.x == 0`` -- in every dtype, mode and min_frac but one.

A block of 256 threads is four waves, a wave owns one slice of S = core.regrid_slice() destinations:
BLOCK = 4 S destinations a block.  The shapes are chosen with that width -- no path of the code
depends on it: ndst = S (one slice, whole), 4 S (one block, whole), 4 S + 1 (a second block of one
slice of one destination) and 9 S + 1 (three blocks, the last of one slice of one destination).

The tables start from test_gpu_regrid.make_table.  Each gets an empty row at the first destination,
a row of 100 entries in a slice of the second block where there is one, and at its end both of
what the last slice is there to show -- on two tables where one destination cannot be both:
  * "empty": the last destination has no entry; the row of 40 entries sits as far back as it can
    while in the last slice (the destination before the last, or the slice before where the last
    slice holds one destination only);
  * "long": (ndst = 4 S + 1 and 9 S + 1 only) the last destination, alone in its partial slice,
    holds the long row -- 40 entries, or the 100 of the second block at ndst = 4 S + 1."""

import functools

import numpy as np
import pytest

import regrid_numpy as rn
from momlevel_amd import core
from test_gpu_regrid import F32, F64, NSRC, assert_same_bits, make_record, make_table, run

pytestmark = pytest.mark.gpu

S = core.regrid_slice()
BLOCK = 4 * S  # destinations of a block: four waves of one slice each
NREC = core.regrid_record_window() + 1
TABLES = [(S, "empty"), (BLOCK, "empty"), (BLOCK + 1, "empty"), (BLOCK + 1, "long"),
          (2 * BLOCK + S + 1, "empty"), (2 * BLOCK + S + 1, "long")]
MODES = {"skipna": 0, "no_renorm": rn.NO_RENORM, "propagate": rn.PROPAGATE}


@functools.lru_cache(maxsize=None)
def block_table(ndst, tail):
    """rows (indptr, col, S) and the places of the rows put in: {what: destination}"""
    indptr, col, w = make_table(ndst)
    rows = [(col[indptr[d]:indptr[d + 1]], w[indptr[d]:indptr[d + 1]]) for d in range(ndst)]
    rng = np.random.default_rng(1000 + ndst)

    def row(n):
        return np.sort(rng.choice(NSRC, n, replace=False)).astype(np.int32), rng.uniform(0.25, 4.0, n)

    empty = (np.zeros(0, dtype=np.int32), np.zeros(0))
    last, alone = ndst - 1, ndst % S == 1  # (alone: the last slice holds the last destination only)
    where = {"empty first": 0}
    rows[0] = empty
    if tail == "long":
        assert alone
        where["row of 40"] = last
        rows[last] = row(100 if last // BLOCK == 1 else 40)
    else:
        where["empty last"] = last
        rows[last] = empty
        where["row of 40"] = last - 1
        rows[last - 1] = row(40)
    if ndst > BLOCK + S:  # a slice of the second block that is not the last one
        where["row of 100"] = BLOCK + S + 5
        rows[BLOCK + S + 5] = row(100)
    elif tail == "long" and last // BLOCK == 1:
        where["row of 100"] = last
    table = (np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64),
             np.concatenate([c for c, _ in rows]).astype(np.int32), np.concatenate([x for _, x in rows]))
    for a in table:
        a.setflags(write=False)
    return table, where


def test_the_tables_hold_what_they_claim():
    assert sorted({n for n, _ in TABLES}) == [S, 4 * S, 4 * S + 1, 9 * S + 1]
    assert NREC == core.regrid_record_window() + 1 and core.regrid_window_rows(NREC) == 2
    for ndst, tail in TABLES:
        (indptr, col, w), where = block_table(ndst, tail)
        length = np.diff(indptr)
        assert length.shape == (ndst,) and length[0] == 0
        last_slice = (ndst - 1) // S
        d40 = where["row of 40"]
        assert length[d40] >= 40
        if tail == "long":
            assert d40 == ndst - 1 and ndst % S == 1  # in the last, partial slice
        else:
            assert length[ndst - 1] == 0
            assert d40 // S == (last_slice if ndst % S != 1 else last_slice - 1)
        if ndst > BLOCK:
            d100 = where["row of 100"] if "row of 100" in where else None
            if d100 is None:  # 4 S + 1, "empty": the second block is its one, empty destination
                assert (ndst, tail) == (BLOCK + 1, "empty")
            else:
                assert length[d100] >= 100 and d100 // BLOCK == 1
        for d in range(ndst):  # ascending cols, as a well-formed table has them
            assert np.all(np.diff(col[indptr[d]:indptr[d + 1]]) > 0)
    assert any("row of 100" in block_table(n, t)[1] for n, t in TABLES if n == BLOCK + 1)
    assert all("row of 100" in block_table(n, t)[1] for n, t in TABLES if n > BLOCK + S)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("odt", (F64, F32), ids=("o64", "o32"))
@pytest.mark.parametrize("vdt", (F64, F32), ids=("v64", "v32"))
def test_every_dtype_mode_and_min_frac_past_one_block(vdt, odt, mode):
    flags = MODES[mode]
    v = make_record(NREC, vdt)
    ran = 0
    for ndst, tail in TABLES:
        table, where = block_table(ndst, tail)
        for min_frac in (0.0, 0.5):
            what = f"ndst={ndst} ({tail}) {vdt.__name__} -> {odt.__name__} {mode} min_frac={min_frac}"
            want = rn.apply_csr(v, *table, ndst, min_frac, flags, odt)
            finite = np.isfinite(want)
            assert np.isnan(want).any() and finite.any() and finite.mean() > 0.5, what
            got = run(v, table, ndst, min_frac, propagate=mode == "propagate",
                      renorm=mode != "no_renorm", out_dtype=odt)
            assert got.dtype == odt
            assert_same_bits(got, want, what)
            assert np.isnan(got[:, 0]).all()
            if "empty last" in where:
                assert np.isnan(got[:, ndst - 1]).all()
            if mode != "propagate":
                assert np.isfinite(got[:, where["row of 40"]]).all(), what
            ran += 1
    print(f"{ran} (table, min_frac) cases of {2 * len(TABLES)}: {vdt.__name__} -> {odt.__name__}, {mode}")
    assert ran == 2 * len(TABLES)
