"""GPU: K0, the promote map, K2 and the exact K1 sums where the guard of the scale-free reciprocal
(csrc/eos_device.hpp: the window on den, the class of the seed, p_ok, the OR over the wave and the
redo of the whole batch in quotients<>) must object -- on the operands of tests/eos_extremes.py,
against the REFERENCE's density on them (tests/golden/wright_extremes.npz; the host file
test_eos_extremes_host.py holds the oracle to it).

Every exact comparison is equality of bits (eos_extremes.same_bits: NaN on NaN, integer views
elsewhere: infinities and the sign of zero count).  The paths are asked of the library
(core.eos_map_path, i.e. core.k0_path on the arguments of the very call) before anything is
compared.  Every call on the planted record is followed by the same call on the record WITHOUT the
planted cells (and, for a pressure field, without the lane that carries the level's pressure): the
ordinary cells must have the same bits in both.

Mutations of the guard (DESIGN.md has the table): redoing only element 0 of a batch fails 21 tests
here; raising the window's upper bound to 2^1023, dropping the p_unsafe_lanes OR and widening p_ok
change no bit on this hardware at these operands (binades 1022 / 1023 come out of the scale-free
sequence with the IEEE bits; den = 0 / inf reach the class test whatever the pressure).

The fused policy is unguarded: its test holds the project's 1e-10 gate inside the window and pins,
per class of den outside it, what was measured on an MI355X (see test_fused_policy_per_class_of_den).
"""

import os

import numpy as np
import pytest
import torch

import eos_extremes as ex
from conftest import GOLDEN
from momlevel_amd import core
from oracle import momlevel_numpy as o

pytestmark = pytest.mark.gpu

FORMS = ["prof", "p3d", "p4d"]
# dtype codes of mlx_eos_map: (record, f32_mode, fixture tag); the two mixed theta / so codes run on
# mlx_eos_map_promote through core.eos_map
CODES = {"f64": ("f64", "faithful", ""), "faithful": ("f32", "faithful", ""),
         "upcast": ("f32", "upcast", "upcast"), "mixT32": ("f32", "faithful", "mixT32"),
         "mixS32": ("f32", "faithful", "mixS32")}
# offT / offS / offP: that operand one element into a padded buffer (offP: the pressure FIELD; a
# profile has no alignment beyond its elements' and runs aligned there)
LAYOUTS = ["aligned", "nx63", "offT", "offS", "offP"]


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "wright_extremes.npz")))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _off16(a):
    """the same values one element into a padded buffer: off a 16-byte line"""
    a = np.ascontiguousarray(a)
    buf = torch.zeros(a.size + 1, dtype=torch.from_numpy(a).dtype, device="cuda")
    view = buf[1:].view(a.shape)
    view.copy_(_dev(a))
    assert view.data_ptr() % 16 != 0
    return view


def _pressures(case, form, plain=False):
    """(host pressure as numpy broadcasts it, what core takes).  ``plain``: without the lanes that
    carry the level's pressure (a field of 2e5); the profile has no plain twin"""
    if form == "prof":
        return case["pz"][:, None, None], case["pz"]
    p = case[form]
    if plain:
        p = np.full_like(p, ex.P_ORDINARY)
    return p, p


def _operands(code, case, plain=False):
    T, S = (case["T_plain"], case["S_plain"]) if plain else (case["T"], case["S"])
    if code == "mixT32":
        S = S.astype(np.float64)
    if code == "mixS32":
        T = T.astype(np.float64)
    return T, S


def _reference(code, T, S, p):
    """numpy on the operands as the dtype code defines them"""
    if code == "upcast":
        T, S = T.astype(np.float64), S.astype(np.float64)
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(o.wright_density(T, S, p))


def _differ(got, ref, what, case=None):
    """the number of cells whose bits differ, printed; the first of them by index, level and value"""
    n = ex.same_bits(got, ref)
    print(f"{what}: {n} of {ref.size} cells differ")
    if n:
        bad = ~((got.view(np.int64) == ref.view(np.int64)) | (np.isnan(got) & np.isnan(ref)))
        for idx in list(zip(*np.nonzero(bad)))[:8]:
            level = case["levels"][idx[1]] if case is not None and len(idx) == 4 else ""
            print(f"    {tuple(int(i) for i in idx)} {level}: got {float(got[idx]).hex()}, want {float(ref[idx]).hex()}")
    return n


# ---- K0 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("code", list(CODES))
def test_k0_density_on_every_dtype_path_and_pressure_form(fixture, code, form, layout):
    prec, f32_mode, tag = CODES[code]
    case = ex.build_case(prec)
    ref = fixture[f"{prec}_rho_{form}" + (f"_{tag}" if tag else "")]
    # nx63: 7 rows of 63 cells, a plane of 441 cells -- no whole packs, the generic kernel
    cut = (Ellipsis, slice(0, 7), slice(0, 63)) if layout == "nx63" else (Ellipsis,)
    results = {}
    for plain in (False, True):
        T, S = (a[cut] for a in _operands(code, case, plain))
        hp, p = _pressures(case, form, plain)
        if form != "prof":
            hp = p = np.ascontiguousarray(p[cut])
        offp = layout == "offP" and form != "prof"
        dT = _off16(T) if layout == "offT" else _dev(T)
        dS = _off16(S) if layout == "offS" else _dev(S)
        dp = _off16(p) if offp else _dev(p)
        if code.startswith("mix"):
            # theta / so of different dtypes run on mlx_eos_map_promote over the broadcast operands:
            # the width of a lane and the result dtype, asked for the flat views core.eos_map hands it
            full = T.shape
            flat = [x.expand(full).reshape(-1) for x in (dT, dS)]
            flat_p = (dp.reshape(1, -1, 1, 1) if form == "prof" else dp).expand(full).reshape(-1)
            width, rdtype = core.eos_map_promote_path(*flat, flat_p)
            print(f"K0 {code} {form} {layout}: promote, {width} cells a lane")
            # (two cells a lane with a float64 operand, one as soon as a flat operand is off a 16-byte
            #  line; a broadcast pressure is materialised, hence aligned, whatever its source was)
            off = any(x.data_ptr() % 16 for x in (*flat, flat_p))
            assert rdtype == torch.float64 and width == (1 if off else 2), (code, form, layout, width)
            assert off == (layout in ("offT", "offS") or (offp and form == "p4d")), (code, form, layout)
        else:
            path = core.eos_map_path(dT, dS, dp, f32_mode=f32_mode)
            generic = layout in ("nx63", "offT", "offS") or offp or form == "p4d"
            want = "generic" if generic else ("fast_p3d" if form == "p3d" else "fast")
            assert path[0] == want, (code, form, layout, path)
        got = core.eos_map(dT, dS, dp, f32_mode=f32_mode).cpu().numpy()
        results[plain] = got
        what = f"K0 {code} {form} {layout}{' plain twin' if plain else ''}"
        if not plain:
            assert _differ(got, np.ascontiguousarray(ref[cut]), what + " vs the fixture", case) == 0
        assert _differ(got, _reference(code, T, S, hp), what + " vs the oracle", case) == 0
    # neighbours: the ordinary cells have the bits of the call without the planted cells
    keep = ~case["planted"][cut]
    if form != "prof":
        keep &= np.broadcast_to(case[form][cut] == ex.P_ORDINARY, keep.shape)
    assert keep.sum() > keep.size - 3 * len(case["levels"]) * ex.NT
    assert ex.same_bits(results[False][keep], results[True][keep]) == 0


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("code", ["f64", "faithful", "upcast"])
def test_k0_other_functions_on_the_same_operands(code, form):
    """drho_dtemp, drho_dsal, alpha and beta divide with the IEEE division everywhere (no guard):
    against the oracle, which make_golden.py held to the reference on these operands"""
    prec, f32_mode, _ = CODES[code]
    case = ex.build_case(prec)
    keep = ~case["planted"]
    if form != "prof":
        keep = keep & np.broadcast_to(case[form] == ex.P_ORDINARY, keep.shape)
    results = {}
    for plain in (False, True):
        T, S = _operands(code, case, plain)
        hp, p = _pressures(case, form, plain)
        dT, dS, dp = _dev(T), _dev(S), _dev(p)
        hT, hS = (T.astype(np.float64), S.astype(np.float64)) if code == "upcast" else (T, S)
        for func in ("drho_dtemp", "drho_dsal", "alpha", "beta"):
            path = core.eos_map_path(dT, dS, dp, func=func, f32_mode=f32_mode)
            assert path[0] == ("fast" if (code == "f64" and form == "prof") else "generic"), (func, path)
            got = core.eos_map(dT, dS, dp, func=func, f32_mode=f32_mode).cpu().numpy()
            with np.errstate(all="ignore"):
                want = np.ascontiguousarray(o.eos_func_from_str("wright", func)(hT, hS, hp))
            assert _differ(got, want, f"K0 {func} {code} {form}{' plain twin' if plain else ''}", case) == 0
            results[plain, func] = got
    for func in ("drho_dtemp", "drho_dsal", "alpha", "beta"):  # neighbours
        assert ex.same_bits(results[False, func][keep], results[True, func][keep]) == 0, func


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_promote_map_gives_the_bits_of_k0(fixture, prec, form):
    """mlx_eos_map_promote on float64 operands and on float32 fields with a float64 pressure"""
    case = ex.build_case(prec)
    shape = case["T"].shape
    results = {}
    for plain in (False, True):
        T, S = _operands(prec, case, plain)
        hp, p = _pressures(case, form, plain)
        dT, dS = _dev(T), _dev(S)
        k0 = core.eos_map(dT, dS, _dev(p)).cpu().numpy()
        flat_p = _dev(np.broadcast_to(hp, shape).reshape(-1))
        width, rdtype = core.eos_map_promote_path(dT.reshape(-1), dS.reshape(-1), flat_p)
        assert rdtype == torch.float64 and width in (2, 4)
        got = core.eos_map_promote(dT.reshape(-1), dS.reshape(-1), flat_p).cpu().numpy().reshape(shape)
        what = f"promote {prec} {form}{' plain twin' if plain else ''}"
        assert _differ(got, k0, what + " vs K0", case) == 0
        if not plain:
            assert _differ(got, fixture[f"{prec}_rho_{form}"], what + " vs the fixture", case) == 0
        results[plain] = got
    keep = ~case["planted"]  # neighbours
    if form != "prof":
        keep = keep & np.broadcast_to(case[form] == ex.P_ORDINARY, keep.shape)
    assert ex.same_bits(results[False][keep], results[True][keep]) == 0


# ---- K2 ---------------------------------------------------------------------------------------------
def _k2(T, S, rho0, p, nz):
    vol = torch.ones((nz, ex.NY, ex.NX), dtype=torch.float64, device="cuda")
    drho, _ = core.steric_local(T, S, core.fold_mask(_dev(rho0), vol), vol[0], p, -1.0 / 1035.0,
                                z_i=np.arange(nz + 1) * 10.0, deptho=np.full((ex.NY, ex.NX), 1e4))
    return drho.cpu().numpy()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_k2_delta_rho_is_fixture_minus_rho0(fixture, prec, form):
    """steric: both fields stream.  thermosteric (S held) and halosteric (theta held), one time step
    a call with the other field's slab of that step held: the planted temperatures are the varying
    field in the first and the held field in the second (the planted salinity the other way round),
    and the fixture applies as it is."""
    case = ex.build_case(prec)
    ref = fixture[f"{prec}_rho_{form}"]
    nz = len(case["levels"])
    with np.errstate(all="ignore"):
        rho0 = o.wright_density(case["T_plain"][0].astype(np.float64),
                                case["S_plain"][0].astype(np.float64), ex.P_ORDINARY)
        dref = ref - rho0
    assert np.isfinite(rho0).all()
    hp, p = _pressures(case, form)
    dT, dS, dp = _dev(case["T"]), _dev(case["S"]), _dev(p)
    got = _k2(dT, dS, rho0, dp, nz)
    assert _differ(got, dref, f"K2 steric {prec} {form}") == 0
    for t in range(ex.NT):
        pt = dp[t:t + 1] if form == "p4d" else dp
        thermo = _k2(dT[t:t + 1], dS[t], rho0, pt, nz)
        halo = _k2(dT[t], dS[t:t + 1], rho0, pt, nz)
        assert _differ(thermo, dref[t:t + 1], f"K2 thermosteric {prec} {form} t={t}") == 0
        assert _differ(halo, dref[t:t + 1], f"K2 halosteric {prec} {form} t={t}") == 0
    # neighbours
    _, pp = _pressures(case, form, plain=True)
    plain = _k2(_dev(case["T_plain"]), _dev(case["S_plain"]), rho0, _dev(pp), nz)
    keep = ~case["planted"]
    if form != "prof":
        keep = keep & np.broadcast_to(case[form] == ex.P_ORDINARY, keep.shape)
    assert ex.same_bits(got[keep], plain[keep]) == 0


# ---- K1, exact ----------------------------------------------------------------------------------------
def _skipna(v):
    return np.where(np.isnan(v), 0.0, v)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_k1_exact_one_hot_sums_at_every_kind_of_planted_cell(fixture, prec):
    """volcello = 1 at one planted cell, NaN elsewhere: masso(t) is rho there, or 0 where rho is
    NaN (skipna).  The single-variant launches divide under the guard, profile and (z,y,x) pressure
    field alike; the all-variants launch (core.steric_global_decomp) divides without it and must
    give the same three sums as they do."""
    case = ex.build_case(prec)
    T, S = case["T"], case["S"]
    nz = len(case["levels"])
    dT, dS, dpz, dp3 = _dev(T), _dev(S), _dev(case["pz"]), _dev(case["p3d"])
    cells = [(k, z, c) for k, _, z, c in case["plants"]]
    # and the cells that carry an objectionable PRESSURE only: the pressure levels' c0
    cells += [(case["levels"][z], z, int(case["c0"][z])) for z in range(nz) if case["levels"][z].startswith("p=")]
    bad = 0
    for kind, z, c in cells:
        y, x = divmod(c, ex.NX)
        hot = np.full((nz, ex.NY, ex.NX), np.nan)
        hot[z, y, x] = 1.0
        dhot = _dev(hot)
        for form, dp, hp in (("prof", dpz, case["pz"][z]), ("p3d", dp3, case["p3d"][z, y, x])):
            assert hp.tobytes() == case["pz"][z].tobytes()  # (the lane carries the level's pressure)
            want = _skipna(fixture[f"{prec}_rho_{form}"][:, z, y, x])
            with np.errstate(all="ignore"):
                want_thermo = _skipna(o.wright_density(T[:, z, y, x], S[0, z, y, x], hp))
                want_halo = _skipna(o.wright_density(T[0, z, y, x], S[:, z, y, x], hp))
            one = core.steric_global_masso(dT, dS, dhot, dp, arith="exact").cpu().numpy()
            thermo = core.steric_global_masso(dT, dS[0], dhot, dp, arith="exact").cpu().numpy()
            halo = core.steric_global_masso(dT[0], dS, dhot, dp, arith="exact").cpu().numpy()
            rows = [(f"{form} steric", one, want), (f"{form} thermosteric", thermo, want_thermo),
                    (f"{form} halosteric", halo, want_halo)]
            if form == "prof":
                dec = core.steric_global_decomp(dT, dS, dT[0], dS[0], dhot, dp, arith="exact").cpu().numpy()
                rows += [("decomp steric", dec[0], want), ("decomp thermosteric", dec[1], want_thermo),
                         ("decomp halosteric", dec[2], want_halo)]
            for name, got, w in rows:
                if not np.array_equal(got, w):
                    bad += 1
                    print(f"K1 {prec} {kind} (z={z}, c={c}) {name}: got {got}, want {w}")
    print(f"K1 {prec}: {len(cells)} cells, {bad} sums differ")
    assert bad == 0


# ---- the fused policy -----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["prof", "p3d"])
def test_fused_policy_per_class_of_den(fixture, form):
    """K0 arith="fused" on the float64 record.  Inside the window 2^-1000 < |den| < 2^1000 the
    project's gate holds: NaN where numpy has NaN, 1e-10 relative elsewhere.  Outside it the policy
    documents what it returns (eos_device.hpp FusedOps, core.arith_default): pinned per class."""
    case = ex.build_case("f64")
    ref = fixture[f"f64_rho_{form}"]
    hp, p = _pressures(case, form)
    _, den, _ = ex.den_of(case, None if form == "prof" else hp)
    den = den.reshape(ref.shape)
    cls = ex.guard_classes(den)
    got = core.eos_map(_dev(case["T"]), _dev(case["S"]), _dev(p), arith="fused").cpu().numpy()
    table = {}
    for c in ("huge", "tiny", "denormal", "zero", "inf", "nan"):
        m = cls == c
        g, r = got[m], ref[m]
        kinds = lambda v: {"nan": int(np.isnan(v).sum()), "inf": int(np.isinf(v).sum()),  # noqa: E731
                           "zero": int((v == 0).sum()),
                           "finite": int((np.isfinite(v) & (v != 0)).sum())}
        fin = np.isfinite(g) & np.isfinite(r) & (r != 0)
        rel = float(np.max(np.abs(g[fin] - r[fin]) / np.abs(r[fin]))) if fin.any() else 0.0
        table[c] = (int(m.sum()), kinds(g), kinds(r), rel)
        print(f"fused {form} den {c}: {m.sum()} cells; fused returns {kinds(g)}, numpy {kinds(r)}; "
              f"max rel where both are finite {rel:.2e}")
    w = cls == "window"
    assert np.array_equal(np.isnan(got[w]), np.isnan(ref[w])), "NaN mask differs inside the window"
    k = w & ~np.isnan(ref)
    assert np.isfinite(ref[k]).all()
    err = np.max(np.abs(got[k] - ref[k]) / np.abs(ref[k]))
    print(f"fused {form} inside the window: {int(k.sum())} cells, max rel {err:.2e} (gate 1e-10)")
    assert err <= 1e-10
    _pin_fused(table, got, ref, cls)


def _pin_fused(table, got, ref, cls):
    """What was MEASURED on an MI355X outside the window (classes of numpy's den; the counts are
    those of the profile record), pinned:
      huge      finite |den| >= 2^1000, up to the top binade (5120 cells): finite, within 1.5e-14 of
                numpy -- v_rcp_f64 hands back a denormal seed unflushed and the cubic correction
                works on it; the 1e-10 gate holds there too
      inf       (2050 cells, two of them overflows from finite operands where numpy has 0.0): NaN
      nan       NaN
      zero, tiny, denormal (one cell each): numpy's den vanishes there by CANCELLATION, and the fused
                policy rounds another den (the pressure folded into B0, lam + al0 * num one fma), which
                does not vanish: a finite value, not NaN.  A den that is 0 or denormal in the fused
                arithmetic itself gives NaN by that arithmetic (r0 = inf, e = -+inf or NaN); no
                operand here reaches one."""
    m = cls == "huge"
    assert np.isfinite(got[m]).all() and np.isfinite(ref[m]).all()
    assert np.max(np.abs(got[m] - ref[m]) / np.abs(ref[m])) <= 1e-10
    assert np.isnan(got[cls == "inf"]).all() and (cls == "inf").sum() >= 10
    assert (ref[cls == "inf"] == 0).sum() == 2  # numpy: num * (1 / +-inf) at the two overflows
    assert np.isnan(got[cls == "nan"]).all()
    for c in ("zero", "tiny", "denormal"):
        assert (cls == c).sum() == 1 and np.isfinite(got[cls == c]).all(), c
        print(f"fused at numpy's {c} den: {float(got[cls == c][0])!r} (numpy {float(ref[cls == c][0])!r})")
