"""Host: the operands of tests/eos_extremes.py have the properties their docstring lists, the
committed fixture tests/golden/wright_extremes.npz (the REFERENCE's density on them,
tests/golden/make_golden.py section (11)) holds exactly these operands, and the oracle agrees with
the fixture bit for bit -- NaN placement, infinities and the sign of zero included."""

import os

import numpy as np
import pytest

import eos_extremes as ex
from conftest import GOLDEN
from oracle import momlevel_numpy as o

PRECS = ["f64", "f32"]
FORMS = ["prof", "p3d", "p4d"]


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "wright_extremes.npz")))


def _pressure(case, form):
    return {"prof": case["pz"][:, None, None], "p3d": case["p3d"], "p4d": case["p4d"]}[form]


@pytest.mark.parametrize("prec", PRECS)
def test_the_builder_asserts_its_properties(prec):
    case = ex.build_case(prec)
    ex.check_case(case)  # (build_case ran it already: once more on the cached record)
    kinds = [k for k, _, _, _ in case["plants"]]
    for b in ex.LADDER:
        assert f"b{b}+" in kinds and f"b{b}-" in kinds
    assert {"inf+", "inf-", "zero"} <= set(kinds)
    assert ("tiny" in kinds) == (prec == "f64")
    assert case["T"].shape == (2, len(case["levels"]), 8, 64)
    rep = ex.placement_report(case)
    print(prec, len(case["levels"]), "levels,", len(kinds), "planted cells;",
          {v: {k: sorted(s) for k, s in r.items() if k != "lanes"} for v, r in rep.items()})


@pytest.mark.parametrize("prec", PRECS)
def test_den_classes_reach_both_sides_of_every_threshold(prec):
    """what the guards see: cells outside the window of both signs, cells just inside it, pressures
    either side of 2^-200 and 2^800 (ExactFastF32Ops::p_ok)"""
    case = ex.build_case(prec)
    _, den, _ = ex.den_of(case)
    a = np.abs(den[np.isfinite(den) & (den != 0)])
    for sign in (1, -1):
        d = den[np.isfinite(den) & (np.sign(den) == sign)]
        b = set(ex.binade(d).tolist())
        assert set(ex.LADDER) <= b, (sign, sorted(set(ex.LADDER) - b))
    assert (a < 2.0 ** 1000).any() and (a >= 2.0 ** 1000).any()
    assert np.isposinf(den).any() and np.isneginf(den).any() and (den == 0).any() and np.isnan(den).any()
    pz = np.abs(case["pz"])
    for lo, hi in ((0.0, 0.0), (5e-324, 2.0 ** -201), (2.0 ** -200, 2.0 ** 800), (2.0 ** 801, np.inf)):
        assert ((pz >= lo) & (pz <= hi)).any(), (lo, hi)
    assert {2.0 ** -200, 2.0 ** 800, 2.0 ** -201, 2.0 ** 801} <= set(pz.tolist())


def test_the_search_for_a_pressure_lands_in_the_binade_it_was_asked_for():
    for dtype in (np.float64, np.float32):
        T, S = np.array([11.5], dtype=dtype), np.array([34.25], dtype=dtype)
        for want in (1.5 * 2.0 ** 990, -1.5 * 2.0 ** 1001, 1.0 * 2.0 ** 1012, -1.99 * 2.0 ** 700, 3.0e5):
            p = ex.pressure_for(T, S, want)
            d = ex.restate(T, S, p)[4][0]
            assert np.isfinite(p) and ex.binade(d) == ex.binade(want) and (d < 0) == (want < 0)
    # ordinary T and S cannot reach the top binades: al0 = 2^-10.5 and p < 2^1024
    T, S = np.array([11.5]), np.array([34.25])
    with np.errstate(all="ignore"):
        top = ex.restate(T, S, np.finfo(np.float64).max)[4][0]
    assert ex.binade(top) <= 1013


@pytest.mark.parametrize("prec", PRECS)
def test_fixture_holds_the_builders_operands(fixture, prec):
    case = ex.build_case(prec)
    for k in ("T", "S", "pz", "p3d", "p4d"):
        got, want = fixture[f"{prec}_{k}"], case[k]
        assert got.dtype == want.dtype and got.shape == want.shape
        assert got.tobytes() == want.tobytes(), k  # (NaN pressures and -0.0 by their bits)
    for k in ("c0", "c1", "planted"):
        assert np.array_equal(fixture[f"{prec}_{k}"], case[k])
    assert [str(k) for k in fixture[f"{prec}_plant_kinds"]] == [k for k, _, _, _ in case["plants"]]
    assert fixture[f"{prec}_plant_cells"].tolist() == [[t, z, c] for _, t, z, c in case["plants"]]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("prec", PRECS)
def test_oracle_equals_fixture_bit_for_bit(fixture, prec, form):
    case = ex.build_case(prec)
    T, S, p = case["T"], case["S"], _pressure(case, form)
    mixes = {"": (T, S)}
    if prec == "f32":
        mixes.update(upcast=(T.astype(np.float64), S.astype(np.float64)),
                     mixT32=(T, S.astype(np.float64)), mixS32=(T.astype(np.float64), S))
    for tag, (a, b) in mixes.items():
        ref = fixture[f"{prec}_rho_{form}" + (f"_{tag}" if tag else "")]
        with np.errstate(all="ignore"):
            got = o.wright_density(a, b, p)
        assert got.dtype == np.float64 and ex.same_bits(got, ref) == 0, (prec, form, tag)
        if not tag:  # and the restatement that returns den: the same bits
            assert ex.same_bits(ex.restate(a, b, np.broadcast_to(p, T.shape))[5].reshape(T.shape), ref) == 0
            assert np.isinf(ref).any() and np.isnan(ref).any() and (form != "prof" or (ref == 0).any())


def test_fixture_is_no_larger_than_the_wright_vectors():
    assert (os.path.getsize(os.path.join(GOLDEN, "wright_extremes.npz"))
            <= os.path.getsize(os.path.join(GOLDEN, "wright_vectors.npz")))
