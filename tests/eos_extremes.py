"""Operands at which the guard of the kernels' reciprocal must object, checkable on the CPU.

csrc/eos_device.hpp computes 1/den of the Wright density with a scale-free sequence and falls back
to the IEEE division when a lane of the wave objects: |den| outside (2^-1000, 2^1000) on float64
operands (ExactFastOps), the class of the seed plus the level's pressure (p == 0 or
2^-200 <= |p| <= 2^800) on numpy's float32 polynomial (ExactFastF32Ops).  This module builds, per
precision ("f64", "f32"), one record of (nt, nz, ny, nx) = (2, nz, 8, 64) whose denominators sit
in chosen binades either side of those thresholds, and asserts what it built with a numpy
restatement of eos/wright.py:44-48 that also returns al0, p0, lam, num and den.

LEVELS (one pressure each; ``case["levels"]`` names them):
  ladder, both signs of the pressure, four planted cells a level:
      top  den in the binades 1023, 1022, 1021 and a den that overflows to +-inf
      mid  den in the binades 1020, 1019, 1010, 1001
      low  den in the binades 1000, 999, 990 (and one slot left ordinary)
    The level's pressure is pressure_for() of its first cell (T = 4e6: al0 = 1.39); the other
    cells get the al0 that puts THEIR den into the wanted binade under that pressure
    (temperature_for(): al0 is linear in T).  Ordinary T and S give al0 = 2^-10.5, so on the
    "low" levels the ordinary cells stay inside the window and the cell of binade 1000 is the only
    objector of its wave; on "mid" and "top" every cell of the level is outside it.
  zero     den == 0.0 exactly with a finite non-zero num (numpy: +-inf), found by stepping the
           pressure of an ordinary cell near -(lam / al0) - p0
  tiny     (float64 only) a non-zero |den| < 2^-1000 CAN be produced from float64 operands: a
           salinity S* with fl(C4 * S*) == -C0 exactly makes C0 + C4*S vanish, lam = T * (...) is
           then as small as T is, and p = -p0 makes num, hence al0 * num, zero: den = lam.  Planted
           with T = 2^-1015 (|den| = 2^-1004.5, rho = -0.0) and T = 2^-1070 (den denormal, 1/den
           infinite, rho = 0 * inf = NaN).  A tiny den with a non-zero num cannot be produced: with
           num != 0, |al0 * num| >= 2^-34 unless al0 vanishes too, and al0 = A0 + A2*S* does not.
           On float32 fields al0, p0 and lam are float32 values and a non-zero den is >= 2^-462
           (eos_device.hpp): nothing to plant, the float32 record has no such level.
  pressure +-0.0, 5e-324, 2^-201, 2^-200, 2^-199, 2^799, 2^800, 2^801, the largest double, +-inf,
           NaN, and 2e5 (ordinary); theta and S ordinary on the whole level.

PLACEMENT.  Level z plants at the two cells c0[z] < 256 <= c1[z] of its (y, x) plane, at both time
steps: four slots (t, c).  A wave of a kernel that takes V cells a lane covers 64 V consecutive
cells, V = 1 (generic), 2 (float64 packs, K2 float32) or 4 (float32 packs), so for every V a planted
cell is alone in its wave: its other 63 lanes hold ordinary theta and S.  Over the levels c0 / c1
run through lane 0 and lane 63, every slot of a 2-cell and of a 4-cell pack, and the first and the
last wave of the plane's block (placement_report() counts them; the cells whose scale-free
quotient can differ from the IEEE one -- binades 1022 and 1023, the overflow, the zero -- sit at
odd cells: never in slot 0 of a pack).

PRESSURE-FIELD TWIN.  ``p3d`` (z, y, x): the level's pressure at c0 and c1, 2e5 everywhere else;
``p4d`` (t, z, y, x): at (t=0, c0) and (t=1, c1) only.  Exactly one lane of a wave carries an
objectionable pressure.

Ordinary cells: theta in [-2, 32], S in [30, 40], one random plane per time step, rolled by five
cells per level (the fixture then compresses; the pressure differs from level to level anyway).
``T_plain`` / ``S_plain``: the same record without the planted cells.
"""

import numpy as np

from oracle import momlevel_numpy as o

NT, NY, NX = 2, 8, 64
PLANE = NY * NX
P_ORDINARY = 2.0e5
DTYPES = {"f64": np.float64, "f32": np.float32}
LADDER = (990, 999, 1000, 1001, 1010, 1019, 1020, 1021, 1022, 1023)
# c0 / c1 of level z: entry z % 12
C0 = (1, 3, 2, 0, 127, 126, 253, 255, 254, 252, 65, 131)
C1 = (511, 509, 510, 508, 385, 384, 257, 259, 258, 256, 447, 386)
PRESSURE_LEVELS = (0.0, -0.0, 5e-324, 2.0 ** -201, 2.0 ** -200, 2.0 ** -199, 2.0 ** 799, 2.0 ** 800,
                   2.0 ** 801, np.finfo(np.float64).max, np.inf, -np.inf, np.nan, P_ORDINARY)
T_ANCHOR = 4.0e6  # al0 = 1.39, lam and p0 finite in float32 too


def restate(T, S, p):
    """eos/wright.py:44-48, operator for operator, on arrays (float64, or numpy's mixed precision for
    float32 T / S: the python-float constants are weak) -> al0, p0, lam, num, den, rho"""
    T, S = np.atleast_1d(T), np.atleast_1d(S)
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    with np.errstate(all="ignore"):
        al0 = o.A0 + o.A1 * T + o.A2 * S
        p0 = o.B0 + o.B4 * S + T * (o.B1 + T * (o.B2 + o.B3 * T) + o.B5 * S)
        lam = o.C0 + o.C4 * S + T * (o.C1 + T * (o.C2 + o.C3 * T) + o.C5 * S)
        num = p + p0
        den = lam + al0 * num
        rho = num * (1.0 / den)
    return al0, p0, lam, num, den, rho


def binade(x):
    """floor(log2 |x|) of finite non-zero values (denormals included)"""
    return np.frexp(np.asarray(x, dtype=np.float64))[1] - 1


def _den(T, S, p):
    return float(restate(T, S, p)[4][0])


def _in_binade(d, want):
    return bool(np.isfinite(d) and d != 0.0 and (d < 0) == (want < 0) and binade(d) == binade(want))


def pressure_for(T, S, want, max_steps=4096):
    """The pressure at which the cell (T, S) -- one-element arrays of the record's dtype -- has a
    den of ``want``'s sign and binade; ``want == 0.0``: a den of exactly zero, or None when no
    pressure within 64 ulp of the estimate gives one.  Starts from (want - lam) / al0 - p0 and steps
    with np.nextafter."""
    al0, p0, lam = (float(v[0]) for v in restate(T, S, 0.0)[:3])
    p = (want - lam) / al0 - p0
    if want == 0.0:
        lo = hi = p
        for _ in range(65):
            for q in (lo, hi):
                num = float(restate(T, S, q)[3][0])
                if _den(T, S, q) == 0.0 and np.isfinite(num) and num != 0.0:
                    return q
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        return None
    for _ in range(max_steps):
        d = _den(T, S, p)
        if _in_binade(d, want):
            return float(p)
        assert not np.isnan(d), (T, S, p)
        p = np.nextafter(p, np.inf if (d < want) == (al0 > 0) else -np.inf)  # d den / d p = al0
    raise AssertionError(f"no pressure gives a den in the binade of {want!r} for T={T}, S={S}")


def temperature_for(S, p, want, dtype, max_steps=1 << 16):
    """The temperature (of ``dtype``) at which the cell (T, S) has a den of ``want``'s sign and
    binade under the pressure ``p`` (|p| huge: den = al0 * p to many digits, al0 linear in T).
    Starts from the T whose al0 is want / p and steps with np.nextafter."""
    s = float(S[0])
    T = np.array([(want / p - o.A0 - o.A2 * s) / o.A1], dtype=dtype)
    for _ in range(max_steps):
        d = _den(T, S, p)
        if _in_binade(d, want):
            return T
        assert not np.isnan(d), (T, S, p)
        T = np.nextafter(T, dtype(np.inf if (d < want) == (p > 0) else -np.inf))  # d den / d T = A1 p
    raise AssertionError(f"no temperature gives a den in the binade of {want!r} at p={p}")


def _salinity_without_c04():
    """a float64 S* with C0 + C4 * S* == 0.0 exactly (the products step by less than an ulp of C0,
    so one exists next to -C0 / C4)"""
    s = np.float64(-o.C0 / o.C4)
    lo = hi = s
    for _ in range(4096):
        for q in (lo, hi):
            if o.C0 + o.C4 * q == 0.0:
                return q
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    raise AssertionError("no salinity cancels C0 + C4*S")


def wave_of(c, vec):
    """(wave, lane, slot) of cell c of a plane in a kernel that takes ``vec`` adjacent cells a lane
    (csrc/momlevel_hip.hip: cell = (unroll * 256 + thread) * vec + slot; 512 cells need one unroll
    step for every vec here)"""
    return c // (64 * vec), (c // vec) % 64, c % vec


_cases = {}


def build_case(prec):
    """The record of ``prec`` ("f64" | "f32"), built once: a dict of
    T, S (nt, nz, ny, nx); T_plain, S_plain; pz (nz,); p3d (nz, ny, nx); p4d (nt, nz, ny, nx);
    c0, c1 (nz,); levels: names; plants: [(kind, t, z, c)] with kind such as "b1022+", "inf-",
    "zero", "tiny", "tiny_denormal"; planted (nt, nz, ny, nx) bool.
    Every property the module docstring lists is asserted here."""
    if prec in _cases:
        return _cases[prec]
    dtype = DTYPES[prec]
    rng = np.random.default_rng(20261021)
    base_T = rng.uniform(-2.0, 32.0, (NT, PLANE)).astype(dtype)
    base_S = rng.uniform(30.0, 40.0, (NT, PLANE)).astype(dtype)

    def ordinary(t, z, c):
        """the unplanted (T, S) of cell c of level z at step t"""
        return (np.roll(base_T[t], 5 * z)[c:c + 1].copy(), np.roll(base_S[t], 5 * z)[c:c + 1].copy())

    levels, pz, plants, values = [], [], [], {}

    def plant(kind, t, z, c, T, S):
        plants.append((kind, t, z, c))
        values[t, z, c] = (dtype(T[0]), dtype(S[0]))

    anchor_T = np.array([T_ANCHOR], dtype=dtype)
    for name, binades in (("top", (1023, 1022, "inf", 1021)), ("mid", (1020, 1019, 1010, 1001)),
                          ("low", (1000, 999, 990, None))):
        for sign, sname in ((1.0, "+"), (-1.0, "-")):
            z = len(levels)
            c0, c1 = C0[z % 12], C1[z % 12]
            slots = [(0, c0), (1, c0), (0, c1), (1, c1)]
            S0 = ordinary(0, z, c0)[1]
            p = pressure_for(anchor_T, S0, sign * 1.5 * 2.0 ** binades[0])
            levels.append(f"{name}{sname}")
            pz.append(p)
            plant(f"b{binades[0]}{sname}", 0, z, c0, anchor_T, S0)
            for b, (t, c) in zip(binades[1:], slots[1:]):
                Sc = ordinary(t, z, c)[1]
                if b is None:
                    continue
                if b == "inf":  # three times the anchor's al0: al0 * num overflows, T, S, p finite
                    plant(f"inf{sname}", t, z, c, np.array([3.0 * T_ANCHOR], dtype=dtype), Sc)
                else:
                    plant(f"b{b}{sname}", t, z, c, temperature_for(Sc, p, sign * 1.5 * 2.0 ** b, dtype), Sc)

    z = len(levels)  # den == 0.0 exactly
    for c in [C0[z % 12]] + [c for c in range(1, 256, 2)]:  # (odd cells: never slot 0 of a pack)
        Tc, Sc = ordinary(0, z, c)
        p = pressure_for(Tc, Sc, 0.0)
        if p is not None:
            break
    assert p is not None, "no ordinary cell of the level reaches den == 0.0"
    levels.append("zero")
    pz.append(p)
    zero_c = c
    plant("zero", 0, z, c, Tc, Sc)

    if prec == "f64":
        z = len(levels)
        s_star = np.array([_salinity_without_c04()])
        levels.append("tiny")
        pz.append(-float(restate(np.array([0.0]), s_star, 0.0)[1][0]))  # -p0 = -(B0 + B4 * S*)
        plant("tiny", 0, z, C0[z % 12], np.array([2.0 ** -1015]), s_star)
        plant("tiny_denormal", 1, z, C1[z % 12], np.array([2.0 ** -1070]), s_star)

    for p in PRESSURE_LEVELS:
        levels.append(f"p={p!r}")
        pz.append(p)
    nz = len(levels)
    pz = np.array(pz, dtype=np.float64)
    c0 = np.array([C0[z % 12] for z in range(nz)])
    c1 = np.array([C1[z % 12] for z in range(nz)])
    c0[levels.index("zero")] = zero_c

    T = np.empty((NT, nz, PLANE), dtype=dtype)
    S = np.empty((NT, nz, PLANE), dtype=dtype)
    for t in range(NT):
        for z in range(nz):
            T[t, z], S[t, z] = np.roll(base_T[t], 5 * z), np.roll(base_S[t], 5 * z)
    T_plain, S_plain = T.copy(), S.copy()
    planted = np.zeros((NT, nz, PLANE), dtype=bool)
    for (t, z, c), (tv, sv) in values.items():
        T[t, z, c], S[t, z, c], planted[t, z, c] = tv, sv, True
    p3d = np.full((nz, PLANE), P_ORDINARY)
    p4d = np.full((NT, nz, PLANE), P_ORDINARY)
    for z in range(nz):
        p3d[z, c0[z]] = p3d[z, c1[z]] = pz[z]
        p4d[0, z, c0[z]] = p4d[1, z, c1[z]] = pz[z]

    shape = (NT, nz, NY, NX)
    case = dict(prec=prec, T=T.reshape(shape), S=S.reshape(shape), T_plain=T_plain.reshape(shape),
                S_plain=S_plain.reshape(shape), pz=pz, p3d=p3d.reshape(shape[1:]),
                p4d=p4d.reshape(shape), c0=c0, c1=c1, levels=levels, plants=plants,
                planted=planted.reshape(shape))
    check_case(case)
    _cases[prec] = case
    return case


def den_of(case, p=None):
    """den (and num, rho) of every cell under the profile (or the pressure field ``p``)"""
    p = case["pz"][:, None, None] if p is None else p
    return restate(case["T"], case["S"], np.broadcast_to(p, case["T"].shape))[3:]


def check_case(case):
    """every property of the module docstring, asserted on the CPU"""
    T, S, pz, plants = case["T"], case["S"], case["pz"], case["plants"]
    nt, nz = T.shape[:2]
    assert T.shape == (NT, nz, NY, NX) and T.dtype == DTYPES[case["prec"]] == S.dtype
    assert np.isfinite(T).all() and np.isfinite(S).all()
    o_T, o_S = case["T_plain"], case["S_plain"]
    assert (o_T >= -2).all() and (o_T <= 32).all() and (o_S >= 30).all() and (o_S <= 40).all()
    assert np.array_equal(T != o_T, case["planted"] & (T != o_T)) and not (S != o_S)[~case["planted"]].any()
    # the restatement is the oracle's density, bit for bit, on every cell and pressure form
    with np.errstate(all="ignore"):
        for p in (pz[:, None, None], case["p3d"], case["p4d"]):
            for a, b in ((T, S), (o_T, o_S)):
                rho = restate(a, b, np.broadcast_to(p, T.shape))[5].reshape(T.shape)
                ref = o.wright_density(a, b, p)
                assert rho.dtype == ref.dtype == np.float64
                assert np.array_equal(np.isnan(rho), np.isnan(ref))
                assert np.array_equal(rho.view(np.int64)[~np.isnan(ref)], ref.view(np.int64)[~np.isnan(ref)])
    num, den, rho = (v.reshape(NT, nz, PLANE) for v in den_of(case))
    kinds = {k: (t, z, c) for k, t, z, c in plants}
    assert len(kinds) == len(plants)
    for sname, neg in (("+", False), ("-", True)):
        for b in LADDER:  # finite den of both signs in every binade of the ladder
            d = den[kinds[f"b{b}{sname}"]]
            assert np.isfinite(d) and binade(d) == b and (d < 0) == neg, (b, sname, d)
        t, z, c = kinds[f"inf{sname}"]
        assert np.isinf(den[t, z, c]) and (den[t, z, c] < 0) == neg and np.isfinite(pz[z])
    t, z, c = kinds["zero"]
    assert den[t, z, c] == 0.0 and np.isfinite(num[t, z, c]) and num[t, z, c] != 0.0 and pz[z] < 0
    assert np.isinf(rho[t, z, c])
    if case["prec"] == "f64":
        d = den[kinds["tiny"]]
        assert d != 0.0 and abs(d) < 2.0 ** -1000 and abs(d) >= 2.0 ** -1022
        assert rho[kinds["tiny"]] == 0.0 and np.signbit(rho[kinds["tiny"]])
        d = den[kinds["tiny_denormal"]]
        assert d != 0.0 and abs(d) < 2.0 ** -1022 and np.isnan(rho[kinds["tiny_denormal"]])
    else:
        assert "tiny" not in kinds
    for p in PRESSURE_LEVELS:  # (NaN: by its bits)
        assert any(np.array(p).tobytes() == np.array(q).tobytes() for q in pz), p
    # on the "low" levels the cell of binade 1000 is the only cell outside the window
    for sname in "+-":
        z = case["levels"].index(f"low{sname}")
        out = ~(np.abs(den[:, z]) < 2.0 ** 1000)
        assert out.sum() == 1 and out[kinds[f"b1000{sname}"][0], kinds[f"b1000{sname}"][2]]
    # placement: alone in its wave for every pack width; c0 in the first half, c1 in the second
    planted = case["planted"].reshape(NT, nz, PLANE)
    assert planted.sum() == len(plants)
    for vec in (1, 2, 4):
        per_wave = planted.reshape(NT, nz, PLANE // (64 * vec), 64 * vec).sum(axis=-1)
        assert per_wave.max() == 1, vec
    assert (case["c0"] < 256).all() and (case["c1"] >= 256).all()
    rep = placement_report(case)
    for vec in (2, 4):
        r = rep[vec]
        assert r["slots"] == set(range(vec)) and {0, 63} <= r["lanes"], (vec, r)
        assert {0, PLANE // (64 * vec) - 1} <= r["waves"], (vec, r)
    assert {0, 63} <= rep[1]["lanes"]
    for k in ("b1022+", "b1022-", "b1023+", "b1023-", "inf+", "inf-", "zero"):
        assert kinds[k][2] % 2 == 1, k  # an odd cell: slot 1 of a 2-pack, 1 or 3 of a 4-pack
    # the pressure fields: one objectionable lane a wave, 2e5 elsewhere
    p3 = case["p3d"].reshape(nz, PLANE)
    p4 = case["p4d"].reshape(NT, nz, PLANE)
    for z in range(nz):
        odd3 = np.flatnonzero(p3[z].view(np.int64) != np.float64(P_ORDINARY).view(np.int64))
        assert set(odd3) <= {case["c0"][z], case["c1"][z]}
        for c in (case["c0"][z], case["c1"][z]):
            assert p3[z, c:c + 1].tobytes() == pz[z:z + 1].tobytes()
        assert p4[0, z, case["c0"][z]:][:1].tobytes() == pz[z:z + 1].tobytes()
        assert p4[1, z, case["c1"][z]:][:1].tobytes() == pz[z:z + 1].tobytes()
        assert (p4[0, z, np.arange(PLANE) != case["c0"][z]] == P_ORDINARY).all()
        assert (p4[1, z, np.arange(PLANE) != case["c1"][z]] == P_ORDINARY).all()


def placement_report(case):
    """{vec: {"slots", "lanes", "waves"}}: where the planted cells and the cells c0 / c1 of the
    pressure fields sit in a kernel of ``vec`` cells a lane"""
    cells = {c for _, _, _, c in case["plants"]} | set(case["c0"].tolist()) | set(case["c1"].tolist())
    rep = {}
    for vec in (1, 2, 4):
        w = [wave_of(c, vec) for c in cells]
        rep[vec] = {"waves": {a for a, _, _ in w}, "lanes": {b for _, b, _ in w},
                    "slots": {c for _, _, c in w}}
    return rep


def guard_classes(den):
    """the class of every den for the fused policy's report: "window" (2^-1000 < |den| < 2^1000),
    "huge" (finite, >= 2^1000), "tiny" (non-zero normal, <= 2^-1000), "denormal", "zero", "inf",
    "nan" -> an array of strings"""
    a = np.abs(den)
    cls = np.full(den.shape, "window", dtype=object)
    cls[np.isfinite(den) & (a >= 2.0 ** 1000)] = "huge"
    cls[(a <= 2.0 ** -1000) & (a >= 2.0 ** -1022)] = "tiny"
    cls[(a < 2.0 ** -1022) & (a > 0)] = "denormal"
    cls[den == 0.0] = "zero"
    cls[np.isinf(den)] = "inf"
    cls[np.isnan(den)] = "nan"
    return cls


def same_bits(got, ref):
    """number of cells whose bits differ: NaN must sit on NaN (any payload), everything else is
    compared as integers -- infinities and the sign of zero included"""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float64, (got.shape, ref.shape)
    nan = np.isnan(ref)
    return int((np.isnan(got) != nan).sum() + (got.view(np.int64)[~nan] != ref.view(np.int64)[~nan]).sum())
