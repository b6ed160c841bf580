"""GPU: core.column_crossing (csrc/momlevel_column.hip) against the numpy restatement
tests/column_numpy.py -- the only yardstick: the function is an extension, the reference has no
counterpart.  Everything is BIT FOR BIT (NaN placement included): both sources, the three modes,
relative and absolute targets, both miss policies, every dtype pairing, the pack path and its
cell-by-cell twin.  The shapes come from the library's own launch queries."""

import numpy as np
import pytest
import torch

import column_numpy as cn
from momlevel_amd import core

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
P_REF = 0.0 * 1.0e4 + 101325
Z7 = np.array([2.5, 10.0, 20.0, 32.5, 51.25, 75.0, 120.0])
MODES = {cn.RISE: "rise", cn.FALL: "fall", cn.DEPART: "depart"}
MISS = {cn.MISS_NAN: "nan", cn.MISS_FLOOR: "floor"}
# source -> (dtype of a, dtype of b or None)
SOURCES = {"field64": (F64, None), "field32": (F32, None), "sigma64": (F64, F64),
           "sigma32": (F32, F32), "sigma_t32_s64": (F32, F64), "sigma_t64_s32": (F64, F32)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64),
                                                 np.ascontiguousarray(b).view(np.int64))


def equals_restatement(got, ref, what=""):
    """bit equality of every number, NaN exactly where the restatement has NaN"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == F64 and got.shape == ref.shape, f"{what}: {got.dtype} {got.shape} vs {ref.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN placement"
    m = ~np.isnan(ref)
    bad = got[m] != ref[m]
    assert not bad.any(), f"{what}: {int(bad.sum())} of {int(m.sum())} values differ"


def planes(adt, bdt):
    """1, 3, one block of packs, one block + one pack + an odd tail (the generic twin), two blocks + 3"""
    block = core.column_block_cells(adt, bdt)
    vec = block // core.column_block_cells(adt, bdt, generic=True)
    assert vec in (2, 4)
    return (1, 3, block, block + vec + 1, 2 * block + 3)


def columns(source, nrec, nz, plane, seed, falling=False):
    """(a, b, x): the operands in their dtypes and the float64 column value the kernel must see.
    Crossing levels are drawn per column over the whole range (a slope per column), the columns
    wiggle (they un-cross), one in ten is land, three in ten end at a floor drawn over every level."""
    adt, bdt = SOURCES[source]
    rng = np.random.default_rng(seed)
    k = np.arange(nz).reshape(1, nz, 1)
    slope = rng.uniform(0.0, 1.6, (nrec, 1, plane)) ** 2
    x = 0.5 + k * slope + rng.normal(0.0, 0.15, (nrec, nz, plane))
    if falling:
        x = 10.0 - x
    kind = rng.random((nrec, plane))
    floor_at = np.where(kind < 0.1, 0, np.where(kind < 0.4, rng.integers(1, nz + 1, (nrec, plane)), nz))
    wet = k < floor_at[:, None, :]
    if bdt is None:
        a = np.where(wet, x, np.nan).astype(adt)
        return a, None, a.astype(F64)
    theta = np.where(wet, 28.0 - 2.5 * x, np.nan).astype(adt)
    so = (34.0 + 0.1 * x + rng.normal(0.0, 0.01, x.shape)).astype(bdt)
    so[(~wet) & (rng.random(x.shape) < 0.5)] = np.nan  # (a NaN in either field is a NaN)
    return theta, so, None


def targets_of(source, mode, relative, n, falling):
    if SOURCES[source][1] is None:
        lo, hi = (0.2, 6.0) if relative else ((3.0, 9.8) if falling else (0.2, 7.0))
    else:
        lo, hi = (0.03, 3.0) if relative else (1019.5, 1026.5)
    return np.linspace(lo, hi, n) if n > 1 else np.array([0.5 * (lo + hi)])


# (mode, relative, miss, with a floor field, kref, targets)
CONFIGS = [
    (cn.RISE, False, cn.MISS_NAN, False, 0, 3),
    (cn.RISE, True, cn.MISS_FLOOR, False, 1, 1),
    (cn.RISE, True, cn.MISS_FLOOR, True, 2, 8),
    (cn.FALL, False, cn.MISS_FLOOR, True, 0, 8),
    (cn.FALL, True, cn.MISS_NAN, False, 1, 3),
    (cn.DEPART, True, cn.MISS_FLOOR, False, 2, 3),
    (cn.DEPART, True, cn.MISS_NAN, True, 0, 1),
]


def run_kernel(a, b, z, tg, kref, mode, relative, miss, floor, eos="wright", out=None):
    return core.column_crossing(dev(a) if isinstance(a, np.ndarray) else a, dev(z), tg,
                                b=None if b is None else (dev(b) if isinstance(b, np.ndarray) else b),
                                kref=kref, mode=MODES[mode], relative=relative, miss=MISS[miss],
                                floor=None if floor is None else dev(floor), eos=eos, p_ref=P_REF,
                                out=out)


@pytest.mark.parametrize("which", range(5), ids=["1", "3", "block", "block+pack+1", "2blocks+3"])
@pytest.mark.parametrize("source", list(SOURCES))
def test_kernel_equals_the_restatement(source, which):
    adt, bdt = SOURCES[source]
    plane = planes(adt, bdt)[which]
    seen = {"hit": 0, "miss": 0, "nan": 0}
    for nz in (1, 2, 7):
        z = Z7[:nz]
        for nrec in (1, 5):
            for ic, (mode, relative, miss, with_floor, kref, nt) in enumerate(CONFIGS):
                kref = min(kref, nz - 1)
                falling = mode == cn.FALL
                a, b, x = columns(source, nrec, nz, plane, 1000 * which + 100 * nz + 10 * nrec + ic, falling)
                eos = "linear" if (bdt is not None and ic % 3 == 2) else "wright"
                if x is None:
                    x = cn.sigma(a, b, P_REF, eos)
                rng = np.random.default_rng(ic)
                floor = None
                if with_floor:
                    floor = rng.uniform(1.0, 200.0, plane)
                    floor[rng.random(plane) < 0.2] = np.nan
                tg = targets_of(source, mode, relative, nt, falling)
                got = run_kernel(a, b, z, tg, kref, mode, relative, miss, floor, eos)
                assert got.is_cuda and tuple(got.shape) == (nrec, nt, plane)
                ref = cn.column_crossing(x, z, kref, mode, relative, miss, tg, floor=floor)
                equals_restatement(got, ref, f"{source} plane={plane} nz={nz} nrec={nrec} config {ic}")
                if nz == 7 and floor is None:
                    interior = ~np.isnan(ref) & ~np.isin(ref, z)
                    seen["hit"] += int(interior.sum())
                    seen["miss"] += int(np.isin(ref, z).sum())
                    seen["nan"] += int(np.isnan(ref).sum())
    # the columns exercise the paths: crossings between levels, misses at a level, NaN
    assert seen["hit"] > 0 and seen["nan"] > 0 and (plane < 3 or seen["miss"] > 0), seen


@pytest.mark.parametrize("source", ["field64", "sigma32"])
def test_every_lane_gets_its_own_trip_count(source):
    """the lanes of one wave finish at different levels; the crossing levels cover the range"""
    adt, bdt = SOURCES[source]
    plane = planes(adt, bdt)[2]
    a, b, x = columns(source, 2, 7, plane, 5)
    if x is None:
        x = cn.sigma(a, b, P_REF)
    tg = targets_of(source, cn.RISE, True, 1, False)
    ref = cn.column_crossing(x, Z7, 0, cn.RISE, True, cn.MISS_NAN, tg)
    level = np.searchsorted(Z7, ref[0, 0, :64])  # of the first wave of the pack path
    assert len(set(level[~np.isnan(ref[0, 0, :64])].tolist())) >= 4
    got = run_kernel(a, b, Z7, tg, 0, cn.RISE, True, cn.MISS_NAN, None)
    equals_restatement(got, ref, source)
