"""GPU: steric / halosteric / thermosteric through the public, labelled API.

First the reference's own tests (tests/test_steric.py) almost verbatim, then parity with
the oracle: pointwise outputs (rho, delta_rho, local eta) bit for bit, masks bit-exact,
reductions over (z,y,x) to <= 1e-10 relative (north_star; observed ~1e-16).
"""

import numpy as np
import pytest
import torch

from momlevel_amd import steric, thermosteric, halosteric, reference as reference_mod, util
from momlevel_amd.eos import wright
from momlevel_amd.labeled import DataArray, Dataset
from momlevel_amd.test_data import generate_test_data
from oracle import momlevel_numpy as o
from conftest import assert_bit_equal, assert_rel

pytestmark = pytest.mark.gpu

dset = generate_test_data()
dset2 = generate_test_data(seed=999)
dset3 = generate_test_data(start_year=1983, nyears=2, calendar="julian")

RTOL_SUM = 1e-10  # north_star tolerance for fp64 reductions


# =================== the reference's tests/test_steric.py =======================================
def test_steric_broadcast():
    result, reference = steric(dset)
    reference = float(reference["rho"][1, 2, 3])
    patm = 101325.0
    rho = wright.density(
        float(dset["thetao"][0, 1, 2, 3]),
        float(dset["so"][0, 1, 2, 3]),
        (float(dset["z_l"][1]) * 1.0e4) + patm,
    )
    assert np.allclose(reference, rho)
    assert reference == rho  # same kernel arithmetic: exactly equal


def test_steric_incorrect_area():
    _dset = dset.copy()
    _dset["areacello"] = _dset["areacello"] * 1.3
    with pytest.raises(Exception):
        _ = steric(_dset)
    with pytest.warns(UserWarning):
        _ = steric(_dset, strict=False)


def _check_reference_sums(reference, g):
    assert np.allclose(reference["thetao"], g["reference_thetao"])
    assert np.allclose(reference["so"], g["reference_so"])
    assert np.allclose(reference["volcello"], g["reference_vol"])
    assert np.allclose(reference["rho"], g["reference_rho"])


@pytest.mark.parametrize("func,variant", [(halosteric, "halosteric"), (steric, "steric"),
                                          (thermosteric, "thermosteric")])
def test_local_values(goldens, func, variant):
    g = goldens["steric_local"]
    result, reference = func(dset)
    result = result.sum()
    reference = reference.sum()
    _check_reference_sums(reference, g)
    assert np.allclose(result[variant], g[variant])
    assert np.allclose(result["delta_rho"], g[f"{variant}_delta_rho"])


@pytest.mark.parametrize("func,variant", [(halosteric, "halosteric"), (steric, "steric"),
                                          (thermosteric, "thermosteric")])
def test_global_values(goldens, steric_cases, func, variant):
    result, reference = func(dset, domain="global")
    assert result[variant].dims == ("time",)
    assert float(result[variant][0]) == 0.0  # self-generated reference
    # the reference's goldens for these 1e-13 values are vacuous (atol-dominated);
    # pinned here by the oracle, as an expansion coefficient with abs tol 1e-12
    href = float(result["reference_height"])
    assert np.isclose(href, steric_cases["global_reference_height"], rtol=1e-13)
    assert np.allclose(result[variant].values / href,
                       steric_cases[f"global_{variant}"] / href, rtol=0, atol=1e-12)
    rsum = reference.sum()
    _check_reference_sums(rsum, goldens["steric_local"])
    assert np.allclose(rsum["volo"], goldens["steric_global"]["global_reference_vol"])
    assert np.allclose(rsum["rhoga"], goldens["steric_global"]["global_reference_rho"])


def test_steric_read_reference(goldens, capsys):
    g = goldens["steric_read_reference"]
    _, reference = steric(dset2)
    result, reference = steric(dset, verbose=True, reference=reference)
    assert "Using supplied reference state" in capsys.readouterr().out
    result = result.sum()
    reference = reference.sum()
    _check_reference_sums(reference, g)
    assert np.allclose(result["steric"], g["steric"])


def test_verbose_generated_reference(capsys):
    steric(dset, verbose=True)
    assert "Generating reference state from first timestep" in capsys.readouterr().out


def test_encoding_1():
    result, reference = steric(dset)
    assert result["delta_rho"].encoding["dtype"] == "float32"
    assert result["steric"].encoding["dtype"] == "float32"
    result, reference = steric(dset, dtype="float64")
    assert result["delta_rho"].encoding["dtype"] == "float64"
    assert result["steric"].encoding["dtype"] == "float64"


def test_encoding_2():
    result, reference = steric(dset, domain="global")
    assert result["reference_height"].encoding["dtype"] == "float32"
    assert result["steric"].encoding["dtype"] == "float32"
    result, reference = steric(dset, domain="global", dtype="float64")
    assert result["reference_height"].encoding["dtype"] == "float64"
    assert result["steric"].encoding["dtype"] == "float64"


def test_steric_annual_average(goldens):
    g = goldens["steric_annual"]
    result, reference = steric(dset3, annual=True)
    assert len(result["time"]) == 2
    result = result.sum()
    assert np.allclose(result["steric"], g["steric"])
    assert np.allclose(result["delta_rho"], g["delta_rho"])


# =================== reference tests/test_reference.py, test_util.py:103-116 ====================
def test_setup_reference_state():
    result = reference_mod.setup_reference_state(dset, eos="Wright")
    expected = ["thetao", "so", "volcello", "rho", "volo", "masso", "rhoga", "areacello"]
    assert len(set(expected) - set(result.variables)) == 0
    util.validate_dataset(result, reference=True)
    with pytest.raises(ValueError):
        util.validate_dataset(result.drop_vars(["rhoga"]), reference=True)


# =================== parity with the oracle =====================================================
def _oracle(d, **kw):
    return o.steric(d["thetao"].values, d["so"].values, d["volcello"].values,
                    d["areacello"].values, d["z_l"].values, d["z_i"].values,
                    d["deptho"].values, **kw)


@pytest.mark.parametrize("variant", ["steric", "thermosteric", "halosteric"])
def test_local_bit_exact_vs_oracle(variant):
    res, ref = steric(dset, variant=variant, dtype="float64")
    ores, oref = _oracle(dset, variant=variant)
    assert res["delta_rho"].dims == ("time", "z_l", "yh", "xh")
    assert res[variant].dims == ("time", "yh", "xh")
    assert_bit_equal(ref["rho"].values, oref["rho"], "rho0")
    assert_bit_equal(res["delta_rho"].values, ores["delta_rho"], "delta_rho")
    assert_bit_equal(res[variant].values, ores[variant], variant)
    assert_rel(ref["volo"].values, oref["volo"], RTOL_SUM, "volo")
    assert_rel(ref["masso"].values, oref["masso"], RTOL_SUM, "masso")
    assert_rel(ref["rhoga"].values, oref["rhoga"], RTOL_SUM, "rhoga")
    assert res[variant].attrs == {"long_name": f"{variant.capitalize()} height adjustment",
                                  "units": "m"}
    assert res["delta_rho"].attrs["units"] == "kg m-3"
    assert res["time"].attrs["cartesian_axis"] == "T"  # coordinate attrs copied from dset


def _masked_dataset(nt=6, nz=9, ny=14, nx=20, seed=7, dtype=np.float64):
    """MOM6-like case with land / below-bottom NaNs everywhere the reference tests have none."""
    from momlevel_amd import synthetic

    g = synthetic.make_grid(ny, nx, nz)
    r = np.random.default_rng(seed)
    mask = np.isnan(g["volcello"])
    T = np.where(mask[None], np.nan, r.normal(12.0, 6.0, (nt, nz, ny, nx)))
    S = np.where(mask[None], np.nan, r.normal(35.0, 1.0, (nt, nz, ny, nx)))
    vol = np.broadcast_to(g["volcello"], T.shape).copy()
    d = Dataset()
    d["time"] = DataArray(np.arange(nt, dtype=float), ("time",), None, {"cartesian_axis": "T"})
    d["z_l"] = DataArray(g["z_l"], ("z_l",))
    d["z_i"] = DataArray(g["z_i"], ("z_i",))
    d["yh"] = DataArray(np.arange(ny, dtype=float), ("yh",))
    d["xh"] = DataArray(np.arange(nx, dtype=float), ("xh",))
    dims = ("time", "z_l", "yh", "xh")
    d["thetao"] = DataArray(T.astype(dtype), dims)
    d["so"] = DataArray(S.astype(dtype), dims)
    d["volcello"] = DataArray(vol, dims)
    d["areacello"] = DataArray(g["areacello"], ("yh", "xh"))
    d["deptho"] = DataArray(g["deptho"], ("yh", "xh"))
    return d


def test_float32_volumes_and_areas_take_numpys_result_dtypes():
    """MOM6 writes volcello and areacello as float32 too.  numpy then sums them in float32
    (derived.py:789 ``volcello.sum()``, steric.py:138 ``areacello.sum()``): ``volo`` is a float32,
    ``reference_height = volo / areacello.sum()`` a float32 division, masso / rhoga stay float64 (rho
    is float64) and the height series float64.  momlevel_amd returns the same dtypes; ``volo`` is
    the float64 device sum of the same float32 values rounded ONCE -- closer to the exact sum than
    numpy's own float32 accumulation (sequential over 8192-element blocks), hence a tolerance, not
    bit equality: 2e-6 relative, at the OM4 1-degree size of BASELINE.json configs[1]."""
    from momlevel_amd import derived, synthetic

    nt, nz, ny, nx = 4, 75, 576, 360
    g = synthetic.make_grid(ny, nx, nz)
    mask = np.isnan(g["volcello"])
    kw = dict(seed=synthetic.SEED, mask3d=g["volcello"])
    d = Dataset()
    d["time"] = DataArray(np.arange(nt, dtype=float), ("time",))
    d["z_l"] = DataArray(g["z_l"], ("z_l",))
    d["z_i"] = DataArray(g["z_i"], ("z_i",))
    dims = ("time", "z_l", "yh", "xh")
    d["thetao"] = DataArray(synthetic.field_numpy((nt, nz, ny, nx), field_id=1, lo=-2.0, scale=34.0,
                                                  **kw).astype(np.float32), dims)
    d["so"] = DataArray(synthetic.field_numpy((nt, nz, ny, nx), field_id=2, lo=30.0, scale=10.0,
                                              **kw).astype(np.float32), dims)
    vol32 = g["volcello"].astype(np.float32)
    d["volcello"] = DataArray(np.broadcast_to(vol32, (nt, nz, ny, nx)), dims)
    d["areacello"] = DataArray(g["areacello"].astype(np.float32), ("yh", "xh"))
    d["deptho"] = DataArray(g["deptho"], ("yh", "xh"))
    assert not mask.all()

    gres, gref = steric(d, domain="global")
    ores, oref = _oracle(d, domain="global")  # numpy on the same float32 arrays
    # dtypes: what numpy gives
    assert oref["volo"].dtype == np.float32 and ores["reference_height"].dtype == np.float32
    assert gref["volo"].values.dtype == np.float32
    assert gres["reference_height"].values.dtype == np.float32
    for name in ("masso", "rhoga"):
        assert gref[name].values.dtype == oref[name].dtype == np.float64
    assert gres["steric"].values.dtype == ores["steric"].dtype == np.float64
    assert derived.calc_volo(gref["volcello"]).values.dtype == np.float32
    assert derived.calc_volo(gref["volcello"]).values == gref["volo"].values
    # values: float64 sum rounded once vs numpy's float32 accumulation
    exact = np.nansum(vol32.astype(np.float64))
    assert gref["volo"].values == np.float32(exact)  # the correctly rounded sum
    assert abs(float(gref["volo"].values) - float(oref["volo"])) <= 2e-6 * exact
    assert_rel(gres["reference_height"].values, ores["reference_height"], 2e-6, "reference_height")
    assert_rel(gref["masso"].values, oref["masso"], RTOL_SUM, "masso")  # float64 in both
    assert_rel(gref["rhoga"].values, oref["rhoga"], 2e-6, "rhoga")
    assert float(gres["steric"][0]) == 0.0 and float(ores["steric"][0]) == 0.0
    scale = np.max(np.abs(ores["steric"]))
    assert scale > 0 and np.max(np.abs(gres["steric"].values - ores["steric"])) <= 2e-6 * scale
    # the local results do not depend on the volumes' values (the volume only masks): bit-identical
    sub = d.isel({"time": slice(0, 2)})
    res, _ = steric(sub)
    lres, _ = _oracle(sub)
    assert_bit_equal(res["steric"].values, lres["steric"], "local eta, float32 volcello")
    assert_bit_equal(res["delta_rho"].values, lres["delta_rho"], "delta_rho, float32 volcello")
    # float64 volumes with a float32 areacello (and the other way round): numpy's promotion
    d64 = d.copy()
    d64["volcello"] = DataArray(np.broadcast_to(g["volcello"], (nt, nz, ny, nx)), dims)
    r64, ref64 = steric(d64.isel({"time": slice(0, 2)}), domain="global")
    assert ref64["volo"].values.dtype == np.float64
    assert r64["reference_height"].values.dtype == np.float64  # float64 / float32 -> float64


@pytest.mark.parametrize("variant", ["steric", "thermosteric", "halosteric"])
@pytest.mark.parametrize("shape", [(6, 9, 14, 20), (3, 5, 7, 9), (17, 4, 6, 16)])
def test_land_masked_local_and_global(variant, shape):
    """even planes take the dwordx4 kernels, the odd 7x9 plane the scalar ones; nt=17 is a
    ragged K2 time chunk (8+8+1)."""
    d = _masked_dataset(*shape)
    res, ref = steric(d, variant=variant)
    ores, oref = _oracle(d, variant=variant)
    assert_bit_equal(res["delta_rho"].values, ores["delta_rho"], "delta_rho")
    assert_bit_equal(res[variant].values, ores[variant], variant)
    assert np.isnan(res[variant].values).any() and not np.isnan(res[variant].values).all()
    gres, gref = steric(d, variant=variant, domain="global")
    ogres, ogref = _oracle(d, variant=variant, domain="global")
    assert float(gres[variant][0]) == 0.0
    href = float(gres["reference_height"])
    assert_rel(href, ogres["reference_height"], RTOL_SUM, "reference_height")
    assert np.allclose(gres[variant].values / href, ogres["expansion_coeff"], rtol=0, atol=1e-12)
    assert_rel(gref["masso"].values, ogref["masso"], RTOL_SUM, "masso0")


@pytest.mark.parametrize("f32_mode", ["faithful", "upcast"])
@pytest.mark.parametrize("shape", [(6, 9, 14, 20), (5, 4, 7, 9)])
@pytest.mark.parametrize("variant", ["steric", "thermosteric", "halosteric"])
def test_float32_inputs_match_numpy_mixed_precision(variant, shape, f32_mode, monkeypatch):
    """float32 theta/S (the reference's usual input dtype), every variant, local AND global.
    faithful: numpy's mixed precision on float32 arrays (eos/wright.py:44-48 with weak python-float
    constants) -- bit for bit; upcast: float64 arithmetic on the float32 values.  The 14x20 plane
    takes the float4 kernels (held-field hoisting in float32, eos_device.hpp), 7x9 the scalar ones."""
    monkeypatch.setenv("MOMLEVEL_AMD_F32_MODE", f32_mode)
    d = _masked_dataset(*shape, dtype=np.float32)
    od = d
    if f32_mode == "upcast":
        od = d.copy()
        for k in ("thetao", "so"):
            od[k] = DataArray(d[k].values.astype(np.float64), d[k].dims)
    res, ref = steric(d, variant=variant)
    ores, oref = _oracle(od, variant=variant)
    assert_bit_equal(ref["rho"].values, oref["rho"], "rho0 from float32")
    assert_bit_equal(res["delta_rho"].values, ores["delta_rho"], "delta_rho from float32")
    assert_bit_equal(res[variant].values, ores[variant], "eta from float32")
    gres, gref = steric(d, variant=variant, domain="global")
    ogres, ogref = _oracle(od, variant=variant, domain="global")
    assert float(gres[variant][0]) == 0.0
    assert_rel(gref["masso"].values, ogref["masso"], RTOL_SUM, "masso0 from float32")
    href = float(gres["reference_height"])
    assert np.allclose(gres[variant].values / href, ogres["expansion_coeff"], rtol=0, atol=1e-12)
    # masso(t) itself, not only its logarithm
    from momlevel_amd import core

    T, S = d["thetao"].values, d["so"].values
    Tv = torch.from_numpy(T if variant != "halosteric" else T[0]).cuda()
    Sv = torch.from_numpy(S if variant != "thermosteric" else S[0]).cuda()
    masso = core.steric_global_masso(Tv, Sv, torch.from_numpy(d["volcello"].values[0]).cuda(),
                                     o.pressure_from_depth(d["z_l"].values),
                                     f32_mode=f32_mode).cpu().numpy()
    assert_rel(masso, ogres["masso"], RTOL_SUM, f"masso(t) float32 {variant}")


@pytest.mark.parametrize("dtypes", [(np.float32, np.float64), (np.float64, np.float32)])
@pytest.mark.parametrize("shape", [(6, 9, 14, 20), (5, 4, 7, 9)])
@pytest.mark.parametrize("variant", ["steric", "thermosteric", "halosteric"])
def test_thetao_and_so_of_different_dtypes(variant, shape, dtypes):
    """A dataset whose thetao and so were written with different precisions.  The reference hands
    both to numpy as they are, so every sub-expression of the EOS takes the dtype numpy's promotion
    gives it (one field's part float32, the other's float64, joined in float64): rho0, delta_rho
    and eta bit for bit, the global sums to 1e-10, local and global, every variant."""
    d = _masked_dataset(*shape)
    for k, dt in zip(("thetao", "so"), dtypes):
        d[k] = DataArray(d[k].values.astype(dt), d[k].dims)
    res, ref = steric(d, variant=variant)
    ores, oref = _oracle(d, variant=variant)
    assert_bit_equal(ref["rho"].values, oref["rho"], "rho0, mixed dtypes")
    assert_bit_equal(res["delta_rho"].values, ores["delta_rho"], "delta_rho, mixed dtypes")
    assert_bit_equal(res[variant].values, ores[variant], "eta, mixed dtypes")
    from momlevel_amd import _lib

    gres, gref = steric(d, variant=variant, domain="global")
    # even planes run on the 16-byte-load kernels since round 4 (the float32 field in 8-byte loads),
    # odd ones on the scalar twins: <type, cells per pack, packs, variant, mode, GENERIC, ...>
    args = _lib.last_kernel().split("<")[1].split(",")
    assert args[4] in ("3", "4") and args[5] == ("false" if (shape[2] * shape[3]) % 2 == 0 else "true")
    ogres, ogref = _oracle(d, variant=variant, domain="global")
    assert float(gres[variant][0]) == 0.0
    assert_rel(gref["masso"].values, ogref["masso"], RTOL_SUM, "masso0, mixed dtypes")
    href = float(gres["reference_height"])
    assert np.allclose(gres[variant].values / href, ogres["expansion_coeff"], rtol=0, atol=1e-12)


def test_mixed_dtypes_refuse_the_fused_policy_in_every_kernel():
    """theta and so of different dtypes have exact kernels only: an explicit arith="fused" raises the
    same ValueError from K0 (eos_map, which routes them to the promote kernel) as from K1 and K2 --
    it used to be ignored silently there"""
    from momlevel_amd import core

    d = _masked_dataset(3, 4, 6, 8)
    T = torch.from_numpy(d["thetao"].values.astype(np.float32)).cuda()
    S = torch.from_numpy(d["so"].values).cuda()
    vol0 = torch.from_numpy(d["volcello"].values[0]).cuda()
    pres = o.pressure_from_depth(d["z_l"].values)
    with pytest.raises(ValueError, match="different dtypes"):
        core.eos_map(T, S, pres, arith="fused")
    with pytest.raises(ValueError, match="different dtypes"):
        core.steric_global_masso(T, S, vol0, pres, arith="fused")
    rho = core.eos_map(T, S, pres)  # the default policy falls back to exact: numpy's bits
    assert_bit_equal(rho.cpu().numpy(),
                     o.wright_density(d["thetao"].values.astype(np.float32), d["so"].values,
                                      pres[:, None, None]), "mixed dtypes, default policy")


def test_cpu_torch_tensors_are_staged_like_numpy_arrays():
    """A CPU torch.Tensor field is host memory like any numpy array: engine.TimeChunks moves it
    through hostio's page-locked staging on the copy stream, with an event, allocated under the
    consumer's stream (it used to take a bare `.to(device)` in the worker thread) --
    same bits as the numpy input, also under a caller's non-default stream"""
    from momlevel_amd import engine

    d = _masked_dataset(nt=7, nz=6, ny=32, nx=48)
    T, S = d["thetao"].values, d["so"].values
    vol0 = torch.from_numpy(d["volcello"].values[0]).cuda()
    pres = o.pressure_from_depth(d["z_l"].values)
    want = engine.global_masso(T, S, vol0, pres, steps=3).cpu().numpy()
    seen = []
    import momlevel_amd.hostio as hostio

    real = hostio.upload

    def spy(host, dev, stream=None, ring=None, mask=None):
        seen.append((host.numel() * host.element_size(), stream is not None))
        return real(host, dev, stream=stream, ring=ring, mask=mask)

    hostio.upload, saved = spy, hostio.upload
    try:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            got = engine.global_masso(torch.from_numpy(T.copy()), torch.from_numpy(S.copy()), vol0,
                                      pres, steps=3)
        side.synchronize()
    finally:
        hostio.upload = saved
    assert np.array_equal(got.cpu().numpy(), want)
    chunk = 3 * T[0].size * 8
    assert sum(1 for n, on_stream in seen if n >= chunk // 2 and on_stream) >= 4  # theta and S chunks


@pytest.mark.parametrize("domain", ["local", "global"])
def test_reference_state_of_another_precision(domain):
    """steric(dset, reference=...) with a float64 reference state and float32 fields (a reference
    written by an earlier run): thermosteric pairs float32 theta with the float64 reference
    salinity, halosteric the other way round, steric is all float32 -- numpy promotes per variant.
    Single calls and the one-pass extension (which then takes one launch per variant)."""
    from momlevel_amd import steric_variants

    d64 = _masked_dataset(5, 6, 14, 20)
    _, ref64 = steric(d64)
    d32 = d64.copy()
    for k in ("thetao", "so"):
        d32[k] = DataArray(d64[k].values.astype(np.float32), d64[k].dims)
    oref = o.setup_reference_state(d64["thetao"].values, d64["so"].values, d64["volcello"].values,
                                   d64["areacello"].values, d64["z_l"].values)
    many, _ = steric_variants(d32, reference=ref64, domain=domain)
    for variant in ("steric", "thermosteric", "halosteric"):
        res, _ = steric(d32, reference=ref64, variant=variant, domain=domain)
        ores, _ = _oracle(d32, reference=oref, variant=variant, domain=domain)
        if domain == "local":
            assert_bit_equal(res["delta_rho"].values, ores["delta_rho"], f"delta_rho {variant}")
            assert_bit_equal(res[variant].values, ores[variant], f"eta {variant}")
        else:
            href = float(res["reference_height"])
            assert np.allclose(res[variant].values / href, ores["expansion_coeff"], rtol=0, atol=1e-12)
        assert_bit_equal(np.asarray(many[variant][variant].values), np.asarray(res[variant].values),
                         f"one-pass extension, {variant}")


def test_mixed_dtypes_in_the_one_pass_extension(monkeypatch):
    from momlevel_amd import steric_variants

    d = _masked_dataset(6, 5, 14, 20)
    d["thetao"] = DataArray(d["thetao"].values.astype(np.float32), d["thetao"].dims)
    for domain in ("local", "global"):
        results, _ = steric_variants(d, domain=domain)
        for variant in ("steric", "thermosteric", "halosteric"):
            single, _ = steric(d, variant=variant, domain=domain)
            assert_bit_equal(np.asarray(results[variant][variant].values),
                             np.asarray(single[variant].values), f"{domain} {variant}")


def test_device_resident_inputs_give_device_outputs():
    d = _masked_dataset()
    dd = d.copy()
    for k in ("thetao", "so", "volcello"):
        dd[k] = DataArray(torch.from_numpy(d[k].values).cuda(), d[k].dims)
    res, ref = steric(dd)
    assert res["delta_rho"].is_device and res["steric"].is_device and ref["rho"].is_device
    ores, _ = _oracle(d)
    assert_bit_equal(res["delta_rho"].values, ores["delta_rho"])
    assert_bit_equal(res["steric"].values, ores["steric"])


def test_time_chunk_streaming_is_invisible(monkeypatch):
    """host inputs larger than the HBM budget go through TimeChunks: force 2-step chunks."""
    from momlevel_amd import engine

    d = _masked_dataset(nt=7)
    whole, _ = steric(d)
    gwhole, _ = steric(d, domain="global")
    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 2)
    res, _ = steric(d)
    gres, _ = steric(d, domain="global")
    assert_bit_equal(res["delta_rho"].values, whole["delta_rho"].values)
    assert_bit_equal(res["steric"].values, whole["steric"].values)
    assert_bit_equal(gres["steric"].values, gwhole["steric"].values)


def test_coord_names_and_varname_map():
    d = _masked_dataset()
    ren = d.rename({"time": "TIME", "z_l": "lev", "z_i": "lev_bnds", "thetao": "temp",
                    "so": "salt"})
    res, ref = steric(ren, coord_names={"t": "TIME", "z": "lev", "zbounds": "lev_bnds"},
                      varname_map={"temp": "thetao", "salt": "so"})
    base, _ = steric(d)
    assert res["steric"].dims == ("TIME", "yh", "xh")
    assert_bit_equal(res["steric"].values, base["steric"].values)
    assert_bit_equal(res["delta_rho"].values, base["delta_rho"].values)


def test_transposed_input_is_handled_by_name():
    d = _masked_dataset()
    dt = d.copy()
    for k in ("thetao", "so", "volcello"):
        tr = d[k].transpose("time", "yh", "xh", "z_l")
        dt[k] = DataArray(np.ascontiguousarray(tr.values), tr.dims)
    res, _ = steric(dt)
    base, _ = steric(d)
    a = res["steric"].transpose("time", "yh", "xh").values
    assert_bit_equal(a, base["steric"].values)
    assert_bit_equal(res["delta_rho"].transpose("time", "z_l", "yh", "xh").values,
                     base["delta_rho"].values)


def test_patm_as_dataarray():
    d = _masked_dataset()
    r = np.random.default_rng(3)
    patm2d = 101325.0 + r.normal(0.0, 500.0, d["areacello"].shape)
    res, ref = steric(d, patm=DataArray(patm2d, ("yh", "xh")))
    T, S = d["thetao"].values, d["so"].values
    pres = d["z_l"].values[:, None, None] * 1.0e4 + patm2d[None]
    rho0 = o.wright_density(T[0], S[0], pres)
    assert_bit_equal(ref["rho"].values, rho0, "rho0 with 2-D patm")
    rho = o.wright_density(T, S, pres[None])
    drho = np.where(~np.isnan(d["volcello"].values[0]), rho - rho0, np.nan)
    assert_bit_equal(res["delta_rho"].values, drho, "delta_rho with 2-D patm")


@pytest.mark.parametrize("domain", ["local", "global"])
def test_patm_with_a_time_dimension(domain, monkeypatch, capsys):
    """patm may be any DataArray (steric.py:58-60,96).  With a time dimension the pressure is 4-D:
    rho(t) = rho(theta(t), S(t), z*1e4 + patm(t)); given a reference state (here from a scalar
    patm) momlevel computes that.  WITHOUT one, its self-made reference is time dependent too
    (reference.py:54,71) and fails validate_dataset (rho 4-D, masso/rhoga not scalar) -- same here."""
    from momlevel_amd import engine

    d = _masked_dataset(nt=5)
    r = np.random.default_rng(4)
    patm = 101325.0 + r.normal(0.0, 600.0, (5,) + d["areacello"].shape)
    patm_da = DataArray(patm, ("time", "yh", "xh"))
    _, ref = steric(d, domain=domain)  # reference state from a scalar patm
    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 2)
    res, _ = steric(d, reference=ref, patm=patm_da, domain=domain)
    T, S, vol0 = d["thetao"].values, d["so"].values, d["volcello"].values[0]
    pres = d["z_l"].values[None, :, None, None] * 1.0e4 + patm[:, None]
    rho = o.wright_density(T, S, pres)
    if domain == "local":
        drho = np.where(~np.isnan(vol0), rho - ref["rho"].values, np.nan)
        assert_bit_equal(res["delta_rho"].values, drho, "delta_rho, patm(time,yh,xh)")
        dz = o.calc_dz(d["z_l"].values, d["z_i"].values, d["deptho"].values)
        eta = np.where(~np.isnan(vol0[0]), (-1.0 / 1035.0) * np.nansum(dz * drho, axis=1), np.nan)
        assert_bit_equal(res["steric"].values, eta, "eta, patm(time,yh,xh)")
    else:
        masso = np.nansum(rho * vol0, axis=(1, 2, 3))
        expansion = np.log(float(ref["rhoga"]) / (masso / float(ref["volo"])))
        h = float(res["reference_height"])
        assert np.allclose(res["steric"].values / h, expansion, rtol=0, atol=1e-12)
    capsys.readouterr()
    with pytest.raises(ValueError, match="Errors found in dataset."):
        steric(d, patm=patm_da, domain=domain)
    out = capsys.readouterr().out
    assert "Variable masso must be a scalar" in out and "Variable rhoga must be a scalar" in out
    # setup_reference_state itself returns the time-dependent state, as momlevel's does
    tref = reference_mod.setup_reference_state(d, patm=patm_da)
    assert tref["rho"].dims == ("time", "z_l", "yh", "xh") and tref["masso"].dims == ("time",)
    rho0_t = o.wright_density(T[0], S[0], pres)
    assert_bit_equal(tref["rho"].values, rho0_t, "time-dependent rho0")
    assert_rel(tref["masso"].values, np.nansum(rho0_t * vol0, axis=(1, 2, 3)), RTOL_SUM)


def test_linear_equation_of_state():
    d = _masked_dataset()
    res, ref = steric(d, equation_of_state="linear")
    ores, oref = _oracle(d, equation_of_state="linear")
    assert_bit_equal(res["delta_rho"].values, ores["delta_rho"])
    assert_bit_equal(res["steric"].values, ores["steric"])


def test_errors():
    with pytest.raises(ValueError):
        steric(dset, variant="bogus")
    with pytest.raises(ValueError):
        steric(dset, equation_of_state="teos10")
    with pytest.raises(AssertionError):
        steric(dset, reference={"not": "a dataset"})
    with pytest.raises(ValueError):  # local needs z_i and deptho
        steric(dset.drop_vars(["deptho"]))
    steric(dset.drop_vars(["deptho"]), domain="global")  # global does not
    bad = dset.copy()
    dep = dset["deptho"].values.copy()
    dep[4, 4] = -200.0
    bad["deptho"] = DataArray(dep, ("yh", "xh"))
    with pytest.raises(AssertionError):
        steric(bad)


def test_xarray_round_trip_if_available():
    xr = pytest.importorskip("xarray")
    from momlevel_amd.adapters import to_xarray

    xd = to_xarray(dset)
    res, ref = steric(xd)
    assert isinstance(res, xr.Dataset) and isinstance(ref, xr.Dataset)
    base, _ = steric(dset)
    assert_bit_equal(res["steric"].values, base["steric"].values)


def test_memory_mapped_inputs_stream_from_disk(tmp_path, monkeypatch):
    """theta/S larger than host RAM live in .npy files: np.load(mmap_mode='r') arrays are sliced
    chunk by chunk by engine.TimeChunks, so only one time chunk is ever resident on the host."""
    from momlevel_amd import engine

    d = _masked_dataset(nt=9)
    base, _ = steric(d)
    gbase, _ = steric(d, domain="global")
    dm = d.copy()
    for k in ("thetao", "so"):
        path = tmp_path / f"{k}.npy"
        np.save(path, d[k].values)
        mm = np.load(path, mmap_mode="r")
        dm[k] = DataArray(mm, d[k].dims)
        assert isinstance(mm, np.memmap) and np.shares_memory(dm[k].data, mm)  # a view, not a copy
    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 4)
    res, _ = steric(dm)
    gres, _ = steric(dm, domain="global")
    assert_bit_equal(res["steric"].values, base["steric"].values)
    assert_bit_equal(res["delta_rho"].values, base["delta_rho"].values)
    assert_bit_equal(gres["steric"].values, gbase["steric"].values)


def test_uploads_and_downloads_go_through_owned_staging(monkeypatch):
    """Round 3: no GPU mapping of caller memory, ever (hostio.py) -- host chunks are copied into a
    ring of page-locked staging buffers of our own and DMA'd from there, results come back through
    the ring into ordinary numpy arrays (round 4's default) or, opt-in, land in page-locked arrays
    of our own.  Forced here through many small pieces (ring wrap-around, ragged last piece) and
    through both result paths; same bits as the plain path every time."""
    from momlevel_amd import engine, hostio

    d = _masked_dataset(nt=6, nz=12, ny=64, nx=96)  # 590 KB per step and field
    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 2)
    base, _ = steric(d)
    gbase, _ = steric(d, domain="global")
    assert hostio._rings, "the staging ring was never used"

    acquired = []
    real_acquire = hostio._Ring.acquire

    def spy(self):
        out = real_acquire(self)
        acquired.append(out[0])
        return out

    monkeypatch.setattr(hostio._Ring, "acquire", spy)
    monkeypatch.setattr(hostio, "PIECE_BYTES", 200_000)  # 1.18 MB chunks -> 6 pieces, last ragged
    res, _ = steric(d)
    assert len(acquired) >= 2 * 3 * 6 and set(acquired) >= {0, 1, 2}  # (the result ring has 4)
    assert_bit_equal(res["steric"].values, base["steric"].values)
    assert_bit_equal(res["delta_rho"].values, base["delta_rho"].values)
    gres, _ = steric(d, domain="global")
    assert_bit_equal(gres["steric"].values, gbase["steric"].values)
    # the default: results come back through the same ring into ordinary numpy arrays ...
    assert hostio.PINNED_RESULT_LIMIT == 0
    assert not torch.from_numpy(res["delta_rho"].values).is_pinned()
    # ... page-locked result arrays are opt-in (MOMLEVEL_AMD_PINNED_RESULT_MIB): one DMA each
    monkeypatch.setattr(hostio, "PINNED_RESULT_LIMIT", 1 << 30)
    acquired.clear()
    big, _ = steric(d)
    assert acquired  # (the uploads)
    assert torch.from_numpy(big["delta_rho"].values).is_pinned()
    assert_bit_equal(big["steric"].values, base["steric"].values)
    assert_bit_equal(big["delta_rho"].values, base["delta_rho"].values)
    # the staging buffers are page-locked memory of torch's allocator, never the caller's array
    ring = next(iter(hostio._rings.values()))
    assert all(b is None or b.is_pinned() for b in ring.bufs)
    assert not torch.from_numpy(d["thetao"].values).is_pinned()


def test_product_moves_bulk_data_through_owned_pinned_memory_only(monkeypatch):
    """The stock transfer path, instrumented: inside this test torch's own ``.cpu()`` / ``.cuda()``
    are in place (the session fixture's rerouting is off) and every host<->device move that goes
    through a Python-level tensor method -- ``copy_``, ``cpu``, ``cuda``, ``to`` -- is recorded.
    steric() on host numpy inputs of 88 MiB per field, both domains, several time chunks: every
    transfer of 256 KiB or more must have page-locked memory OF OURS on its host side (the product
    never hands the runtime a pageable source or destination it would have to map on the fly), and
    the caller's arrays are never page-locked.  A spy, run once -- not an attempt to provoke the
    round-3 fault."""
    import conftest
    from momlevel_amd import engine, hostio

    stock_cpu, stock_cuda = conftest.stock_transfers()
    real_copy, real_to = torch.Tensor.copy_, torch.Tensor.to
    seen = []  # (method, bytes, host side page-locked?)

    def note(method, host):
        seen.append((method, host.numel() * host.element_size(), bool(host.is_pinned())))

    def copy_(self, src, *a, **k):
        if isinstance(src, torch.Tensor) and self.is_cuda != src.is_cuda:
            note("copy_", src if self.is_cuda else self)
        return real_copy(self, src, *a, **k)

    def cpu(self, *a, **k):
        if self.is_cuda:
            seen.append(("cpu", self.numel() * self.element_size(), False))  # pageable result
        return stock_cpu(self, *a, **k)

    def cuda(self, *a, **k):
        if not self.is_cuda:
            note("cuda", self)
        return stock_cuda(self, *a, **k)

    def to(self, *a, **k):
        out = real_to(self, *a, **k)
        if out.is_cuda != self.is_cuda:
            if self.is_cuda:
                seen.append(("to", self.numel() * self.element_size(), False))
            else:
                note("to", self)
        return out

    for name, fn in (("copy_", copy_), ("cpu", cpu), ("cuda", cuda), ("to", to)):
        monkeypatch.setattr(torch.Tensor, name, fn)
    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 3)

    d = _masked_dataset(nt=8, nz=20, ny=240, nx=288)  # 88 MiB per field
    assert d["thetao"].values.nbytes >= 64 << 20
    res, ref = steric(d)
    gres, _ = steric(d, domain="global")
    torch.cuda.synchronize()
    monkeypatch.undo()
    big = [(m, n, pinned) for m, n, pinned in seen if n >= hostio.SMALL_BYTES]
    assert len(big) >= 8, seen  # uploads in 64 MiB pieces + result downloads: the spy saw them
    assert all(pinned for _, _, pinned in big), [b for b in big if not b[2]]
    assert sum(n for _, n, _ in big) >= 2 * 2 * d["thetao"].values.nbytes  # theta and S, twice
    for k in ("thetao", "so", "volcello"):
        assert not torch.from_numpy(np.ascontiguousarray(d[k].values)).is_pinned()
    # and the numbers are the reference's
    ores, _ = _oracle(d)
    assert_bit_equal(res["steric"].values, ores["steric"], "local eta")
    assert_bit_equal(res["delta_rho"].values, ores["delta_rho"], "delta_rho")
    assert float(gres["steric"][0]) == 0.0


def test_leading_one_pressure_with_several_time_chunks():
    """a (1,nz,1,1) pressure (calc_rho's 4-D broadcast of a z profile) must give the same
    result whatever the number of time chunks -- it used to be sliced like a time-dependent field
    and came out empty from the second chunk on"""
    from momlevel_amd import engine

    d = _masked_dataset(nt=5)
    T = np.ascontiguousarray(d["thetao"].values)
    S = np.ascontiguousarray(d["so"].values)
    vol0 = np.ascontiguousarray(d["volcello"].values[0])
    nz = T.shape[1]
    pres = o.pressure_from_depth(np.asarray(d["z_l"].values)).reshape(1, nz, 1, 1)
    one = engine.global_masso(T, S, vol0, pres).cpu().numpy()
    many = engine.global_masso(T, S, vol0, pres, steps=2).cpu().numpy()
    assert np.array_equal(one, many)
    ref = engine.global_masso(T, S, vol0, pres.reshape(nz), steps=2).cpu().numpy()
    assert np.array_equal(ref, many)


def test_hostio_round_trip_ragged_sizes(monkeypatch):
    """upload / download_into on sizes around the piece and small-transfer boundaries, float32
    and float64, pinned and pageable destinations"""
    from momlevel_amd import hostio

    monkeypatch.setattr(hostio, "PIECE_BYTES", 1 << 20)
    r = np.random.default_rng(5)
    for dtype in (np.float64, np.float32):
        for n in (1, 1000, (256 << 10) // 8, (1 << 20) // 8 + 3, 3 * (1 << 20) // 8 + 17, 1234567):
            a = r.standard_normal(n).astype(dtype)
            t = hostio.to_device(a, "cuda")
            assert t.dtype == (torch.float64 if dtype == np.float64 else torch.float32)
            assert np.array_equal(t.cpu().numpy(), a)
            pinned = torch.empty(n, dtype=t.dtype, pin_memory=True).numpy()
            for out in (pinned, hostio.pinned_array((n,), dtype), np.empty(n, dtype)):
                hostio.download_into(out, t)
                torch.cuda.synchronize()
                assert np.array_equal(out, a)
            assert np.array_equal(hostio.to_host(t), a)
    b = r.standard_normal((7, 300, 301))
    assert np.array_equal(hostio.to_host(hostio.to_device(b[:, ::2], "cuda")), b[:, ::2])


def test_pipelined_result_downloads(monkeypatch):
    """hostio.Downloader (round 4): the result arrays of consecutive time chunks leave through ONE
    pipeline of staging pieces on a worker thread -- pieces of one array still in flight while the
    next array's are enqueued, at most `depth` chunks outstanding.  Ragged sizes, float64 results
    into pageable and page-locked arrays, many small pieces (ring wrap-around); a failure in the
    worker reaches the caller."""
    from momlevel_amd import hostio

    monkeypatch.setattr(hostio, "PIECE_BYTES", 1 << 20)
    r = np.random.default_rng(11)
    sizes = [(3, 40, 50, 60), (2, 50, 60), (1, 7), (5, 300, 301), (1 << 17,), ((3 << 20) // 8 + 5,)]
    truth = [r.standard_normal(sz) for sz in sizes]
    dev = [hostio.to_device(a, "cuda") for a in truth]
    outs = [np.full(sz, np.nan) for sz in sizes]
    outs[3] = torch.empty(sizes[3], dtype=torch.float64, pin_memory=True).numpy()
    acquired = []
    real_acquire = hostio._Ring.acquire
    monkeypatch.setattr(hostio._Ring, "acquire",
                        lambda self: acquired.append(self) or real_acquire(self))
    with hostio.Downloader(dev[0].device, depth=2) as results:
        ring = results._ring
        results.submit([(outs[0], dev[0]), (outs[1], dev[1])])
        results.submit([(outs[2], dev[2])])
        # a non-contiguous device tensor is packed on the download stream
        results.submit([(outs[3], dev[3]), (outs[4], dev[4])])
        results.submit([(outs[5], dev[5])])
        assert len(results._jobs) <= 2
    for a, out in zip(truth, outs):
        assert_bit_equal(out, a)
    assert acquired and all(x is ring for x in acquired) and ring.depth == 4
    assert not results._pending and all(e is None for e in ring.events)
    t = hostio.to_device(truth[0], "cuda")
    with pytest.raises(ValueError):  # 4 values more than the array holds: the worker refuses
        with hostio.Downloader(t.device) as results:
            results.submit([(np.empty(truth[0].size - 4), t.reshape(-1))])
    with pytest.raises(ZeroDivisionError):  # the caller's own failure is the one reported
        with hostio.Downloader(t.device) as results:
            results.submit([(outs[0], t)])
            1 / 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("domain", ["local", "global"])
def test_steric_variants_extension_matches_single_calls(domain, monkeypatch):
    """One upload of theta/S, three variants: each bit-identical to its own steric() call."""
    from momlevel_amd import engine, steric_variants

    d = _masked_dataset(nt=7)
    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 3)
    results, reference = steric_variants(d, domain=domain)
    assert set(results) == {"steric", "thermosteric", "halosteric"}
    for variant, res in results.items():
        single, ref1 = steric(d, variant=variant, domain=domain)
        assert_bit_equal(res[variant].values, single[variant].values, variant)
        if domain == "local":
            assert_bit_equal(res["delta_rho"].values, single["delta_rho"].values)
        else:
            assert float(res[variant][0]) == 0.0
            assert float(reference["masso"]) == float(ref1["masso"])
    with pytest.raises(ValueError):
        steric_variants(d, variants=("steric", "bogus"))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_global_decomposition_and_heat_content_in_one_pass(dtype, monkeypatch):
    """steric_variants(domain="global") runs the all-variants kernel (theta/S read ONCE); every
    variant stays bit-identical to its own steric() call; heat_content=True adds the OHC row
    (extension; own numpy oracle, parity unpinned -- momlevel has no such function)."""
    from momlevel_amd import core, engine, steric_variants

    d = _masked_dataset(nt=7, dtype=dtype)
    calls = {"decomp": 0, "single": 0}
    real_decomp, real_single = core.steric_global_decomp, core.steric_global_masso

    def count_decomp(*a, **k):
        calls["decomp"] += 1
        return real_decomp(*a, **k)

    def count_single(*a, **k):
        calls["single"] += 1
        return real_single(*a, **k)

    monkeypatch.setattr(core, "steric_global_decomp", count_decomp)
    monkeypatch.setattr(core, "steric_global_masso", count_single)
    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 4)
    results, reference = steric_variants(d, domain="global", heat_content=True)
    assert calls == {"decomp": 2, "single": 0}  # two time chunks, one launch each
    assert set(results) == {"steric", "thermosteric", "halosteric", "heat"}
    ohc = o.ocean_heat_content(d["thetao"].values, d["volcello"].values[0])
    assert_rel(results["heat"]["ohc"].values, ohc, 1e-12, "ocean heat content")
    assert results["heat"]["ohc"].attrs["units"] == "J"
    for variant in ("steric", "thermosteric", "halosteric"):
        single, ref1 = steric(d, variant=variant, domain="global")
        assert_bit_equal(results[variant][variant].values, single[variant].values, variant)
        assert float(results[variant][variant][0]) == 0.0
        assert float(reference["masso"]) == float(ref1["masso"])
    with pytest.raises(ValueError):
        steric_variants(d, domain="local", heat_content=True)


def test_fused_arithmetic_through_the_public_api(monkeypatch):
    """MOMLEVEL_AMD_ARITH=fused: the whole path (reference rho0, K1, K2) switches together, so
    the exact zeros at t=0 survive, and results stay within north_star's 1e-10 of the oracle."""
    d = _masked_dataset(nt=5)
    exact, _ = steric(d)
    gexact, _ = steric(d, domain="global")
    monkeypatch.setenv("MOMLEVEL_AMD_ARITH", "fused")
    for variant in ("steric", "thermosteric", "halosteric"):
        res, ref = steric(d, variant=variant)
        ores, oref = _oracle(d, variant=variant)
        wet = ~np.isnan(ores["delta_rho"][0])
        assert np.all(res["delta_rho"].values[0][wet] == 0.0)
        err = np.nanmax(np.abs(res["delta_rho"].values - ores["delta_rho"]))
        assert err <= 1e-10 * np.nanmax(np.abs(ores["delta_rho"])) and err > 0.0
        err = np.nanmax(np.abs(res[variant].values - ores[variant]))
        assert err <= 1e-10 * np.nanmax(np.abs(ores[variant]))
        assert_rel(ref["rho"].values, oref["rho"], 1e-10, "fused rho0")
        gres, gref = steric(d, variant=variant, domain="global")
        ogres, ogref = _oracle(d, variant=variant, domain="global")
        assert float(gres[variant][0]) == 0.0
        assert_rel(gref["masso"].values, ogref["masso"], RTOL_SUM, "fused masso0")
        h = float(gres["reference_height"])
        assert np.allclose(gres[variant].values / h, ogres["expansion_coeff"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("domain", ["local", "global"])
@pytest.mark.parametrize("order", [("time", "z_l", "yh", "xh"), ("time", "yh", "xh", "z_l")])
def test_lazy_inputs_are_read_one_time_chunk_at_a_time(domain, order, monkeypatch):
    """momlevel's real inputs are dask-chunked float32 files (examples/example.ipynb cell 4).  A
    lazy theta/S/volcello (tests/lazy_array.py counts every read) goes through steric() without
    EVER being materialised whole: reads are the reference slab and one time chunk at a time, also
    when the dims need a transpose; results equal the numpy-backed run bit for bit."""
    from lazy_array import CountingLazy
    from momlevel_amd import engine

    d = _masked_dataset(nt=7, dtype=np.float32)
    base, bref = steric(d, domain=domain)
    lazies = {}
    dl = d.copy()
    for k in ("thetao", "so", "volcello"):
        arr = d[k].transpose(*order).values
        lazies[k] = CountingLazy(np.ascontiguousarray(arr))
        dl[k] = DataArray(lazies[k], order)
    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 2)
    res, ref = steric(dl, domain=domain)
    step_bytes = d["thetao"].values[0].nbytes
    for k in ("thetao", "so"):
        assert lazies[k].largest_read <= 2 * step_bytes, (k, lazies[k].reads)
        assert sum(lazies[k].reads) <= (7 + 2) * step_bytes  # every step once + the reference slab
    assert lazies["volcello"].largest_read <= d["volcello"].values[0].nbytes
    assert_bit_equal(res["steric"].values, base["steric"].values, "lazy vs numpy inputs")
    if domain == "local":
        assert_bit_equal(res["delta_rho"].values, base["delta_rho"].values)
    assert_bit_equal(ref["rho"].transpose(*bref["rho"].dims).values, bref["rho"].values)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("domain", ["local", "global"])
@pytest.mark.parametrize("container", ["masked", "masked_deferred", "masked_deferred_transposed",
                                       "lazy_masked", "lazy_masked_transposed"])
def test_masked_arrays_mean_nan(container, domain, dtype, monkeypatch):
    """What netCDF4 hands over where a file declares ``_FillValue``: numpy masked arrays holding
    1e20 under the mask -- for a whole in-memory variable ("masked") and for every slice of a lazily
    read one ("lazy_masked").  The reference never sees them: xarray has turned the mask into NaN
    (``xr.DataArray(masked)``; ``open_mfdataset``, examples/example.ipynb cell 4; steric.py:84-96).
    steric() on theta/S/volcello/areacello/deptho given so returns the bits of the same call on the
    NaN-filled plain arrays -- and those are the oracle's."""
    from lazy_array import FILL, MaskedLazy, as_masked
    from momlevel_amd import engine

    from momlevel_amd import hostio, labeled

    d = _masked_dataset(nt=7, dtype=dtype)
    assert np.isnan(d["thetao"].values).any()
    base, bref = steric(d, domain=domain)
    dm = d.copy()
    dims = d["thetao"].dims
    order = ("time", "yh", "xh", "z_l") if container.endswith("transposed") else dims
    deferred = container.startswith("masked_deferred")
    if deferred:
        # "masked_deferred": the in-memory masked array is big enough (here: the threshold is made
        # small enough) to be kept as data + mask -- labeled.MaskedSource -- and NaN-filled only
        # while its time chunks are copied into the staging ring
        monkeypatch.setattr(labeled, "_NATIVE_FILL_BYTES", 1 << 10)
        monkeypatch.setattr(hostio, "SMALL_BYTES", 1 << 10)
        fused = []
        real = hostio._host_copy_masked
        monkeypatch.setattr(hostio, "_host_copy_masked",
                            lambda dst, src, mask, elem: fused.append(dst.numel()) or real(dst, src, mask, elem))
    for k in ("thetao", "so", "volcello"):
        arr = np.ascontiguousarray(d[k].transpose(*order).values)
        held = as_masked(arr) if container.startswith("masked") else MaskedLazy(arr)
        if container.startswith("masked"):
            assert held.data[np.isnan(arr)][0] == arr.dtype.type(FILL)
        dm[k] = DataArray(held, order)
        assert isinstance(dm[k].data, labeled.MaskedSource) == deferred
    for k in ("areacello", "deptho"):
        dm[k] = DataArray(as_masked(d[k].values), d[k].dims)
    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 2)
    res, ref = steric(dm, domain=domain)
    if container == "masked_deferred":
        assert fused, "the chunks of a MaskedSource must be NaN-filled by the staging copy"
    assert_bit_equal(res["steric"].values, base["steric"].values, "masked vs NaN-filled inputs")
    assert_bit_equal(ref["rho"].transpose(*bref["rho"].dims).values, bref["rho"].values)
    assert float(ref["volo"]) == float(bref["volo"]) and float(ref["masso"]) == float(bref["masso"])
    if domain == "local":
        assert_bit_equal(res["delta_rho"].transpose(*dims).values, base["delta_rho"].values)
        if dtype == np.float64:
            ores, oref = _oracle(d)
            assert_bit_equal(res["steric"].values, ores["steric"], "masked inputs vs the oracle")
            assert_bit_equal(res["delta_rho"].transpose(*dims).values, ores["delta_rho"])
    else:
        assert float(res["reference_height"]) == float(base["reference_height"])
        assert np.abs(res["steric"].values).max() < 1.0  # (1e20 fill values would give ~1e17 m)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("domain", ["local", "global"])
def test_masked_slices_are_nan_filled_on_their_way_into_the_staging_ring(domain, dtype, monkeypatch):
    """The masked slices of a lazily read field above hostio.SMALL_BYTES are not NaN-filled into an
    array of their own: they travel as data + mask and mlx_host_copy_masked writes NaN under the mask
    while each piece is copied into the page-locked staging buffer (hostio.split_masked / upload).
    Here with thresholds small enough that the test grid takes that path, in several pieces per
    chunk with piece edges inside rows: bit-identical to the NaN-filled plain arrays."""
    from lazy_array import PrebuiltMaskedLazy
    from momlevel_amd import engine, hostio

    d = _masked_dataset(nt=7, nz=9, ny=28, nx=40, dtype=dtype)
    base, bref = steric(d, domain=domain)
    calls = []
    real = hostio._host_copy_masked
    monkeypatch.setattr(hostio, "_host_copy_masked",
                        lambda dst, src, mask, elem: calls.append((dst.numel(), elem)) or real(dst, src, mask, elem))
    monkeypatch.setattr(hostio, "SMALL_BYTES", 1 << 10)
    monkeypatch.setattr(hostio, "PIECE_BYTES", 12344)  # (a multiple of 8, not of a row)
    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 3)
    dm = d.copy()
    for k in ("thetao", "so"):
        dm[k] = DataArray(PrebuiltMaskedLazy(np.ascontiguousarray(d[k].values)), d[k].dims)
    res, ref = steric(dm, domain=domain)
    assert calls and {e for _, e in calls} == {np.dtype(dtype).itemsize}
    assert max(n for n, _ in calls) <= 12344 and len(calls) >= 2 * 3 * 3  # fields x chunks x pieces
    assert_bit_equal(res["steric"].values, base["steric"].values, "fused NaN fill vs NaN-filled inputs")
    assert_bit_equal(ref["rho"].values, bref["rho"].values)
    if domain == "local":
        assert_bit_equal(res["delta_rho"].values, base["delta_rho"].values)


@pytest.mark.parametrize("domain", ["local", "global"])
def test_float16_fields_are_refused_on_the_steric_path_too(domain):
    """numpy evaluates eos/wright.py on float16 arrays in float16; a silent float64 upcast would
    answer in other bits.  The EOS functions refused such operands already; steric() now does too."""
    d = _masked_dataset(nt=3)
    d16 = d.copy()
    d16["thetao"] = DataArray(d["thetao"].values.astype(np.float16), d["thetao"].dims)
    with pytest.raises(TypeError, match="float16"):
        steric(d16, domain=domain)
    steric(d, domain=domain)  # (and the next call works)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("domain", ["local", "global"])
def test_steric_from_a_netcdf3_file(domain, dtype, tmp_path, monkeypatch):
    """The advertised lazy route with a REAL reader: the dataset is written as a NetCDF-3 file (NaN
    cells as _FillValue 1e20, what MOM6 writes on land) and read back through scipy.io.netcdf_file
    with ``maskandscale=True`` -- every read is a BIG-ENDIAN numpy masked array.  The 4-D fields stay
    on disk and are read one time chunk at a time; steric() returns the bits of the same call on the
    in-memory NaN-filled arrays (for float32 fields that means numpy's float32 polynomial, not a
    silent float64 upcast of ">f4"), i.e. the oracle's."""
    from scipy.io import netcdf_file

    from lazy_array import NetCDFVar, write_netcdf3
    from momlevel_amd import engine

    d = _masked_dataset(nt=7, dtype=dtype)
    base, bref = steric(d, domain=domain)
    path = str(tmp_path / "ocean.nc")
    write_netcdf3(path, d)
    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 2)
    f = netcdf_file(path, "r", mmap=False, maskandscale=True)
    try:
        dl = Dataset()
        lazies = {}
        for name, var in f.variables.items():
            if len(var.shape) == 4 and name == "so":
                dl[name] = DataArray(var, tuple(var.dimensions))  # the scipy variable as it is
                assert dl[name].is_lazy and dl[name].dtype == np.dtype(dtype)
            elif len(var.shape) == 4:
                lazies[name] = NetCDFVar(var)  # (counts the reads)
                dl[name] = DataArray(lazies[name], tuple(var.dimensions))
            else:
                dl[name] = DataArray(var[:], tuple(var.dimensions))  # a masked array or a plain one
        assert str(lazies["thetao"].dtype) == (">f4" if dtype == np.float32 else ">f8")
        assert dl["thetao"].dtype == np.dtype(dtype) and dl["thetao"].is_lazy
        assert isinstance(lazies["thetao"][0:1], np.ma.MaskedArray)
        res, ref = steric(dl, domain=domain)
        step = d["thetao"].values[0].nbytes
        assert max(lazies["thetao"].reads) <= 2 * step  # never more than one time chunk
    finally:
        f.close()
    assert_bit_equal(res["steric"].values, base["steric"].values, "NetCDF-3 file vs in-memory arrays")
    assert_bit_equal(ref["rho"].values, bref["rho"].values)
    assert float(ref["volo"]) == float(bref["volo"])
    if domain == "local":
        assert_bit_equal(res["delta_rho"].values, base["delta_rho"].values)
        ores, _ = _oracle(d)
        if dtype == np.float64:
            assert_bit_equal(res["steric"].values, ores["steric"])


@pytest.mark.parametrize("domain", ["local", "global"])
def test_a_failing_source_raises_from_steric_and_leaves_no_thread_behind(domain, monkeypatch):
    """Uploads are staged by a worker thread (engine.TimeChunks): a source that fails in the middle
    of the record -- an I/O error of a lazily read file -- must surface as THAT exception from
    steric(), promptly, and the worker must be gone afterwards; a following call works."""
    import threading

    from lazy_array import CountingLazy
    from momlevel_amd import engine

    class Flaky(CountingLazy):
        def __getitem__(self, key):
            if isinstance(key, slice) and (key.start or 0) >= 4:
                raise OSError("simulated read error in the third time chunk")
            return super().__getitem__(key)

    d = _masked_dataset(nt=7, dtype=np.float32)
    dl = d.copy()
    dl["thetao"] = DataArray(Flaky(np.ascontiguousarray(d["thetao"].values)), d["thetao"].dims)
    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 2)
    with pytest.raises(OSError, match="simulated read error"):
        steric(dl, domain=domain)
    assert not [t for t in threading.enumerate() if t.name.startswith(("mlx-upload", "mlx-download"))]
    good, _ = steric(d, domain=domain)  # the streams and the staging ring are still usable
    base, _ = steric(d, domain=domain)
    assert_bit_equal(good["steric"].values, base["steric"].values)


@pytest.mark.parametrize("domain", ["local", "global"])
def test_host_inputs_under_a_callers_stream(domain, monkeypatch):
    """the caller may run steric() with a stream of its own current: uploads (worker thread, copy
    stream), kernels (the caller's stream) and downloads order themselves against THAT stream"""
    from momlevel_amd import engine

    d = _masked_dataset(nt=7)
    base, _ = steric(d, domain=domain)
    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 2)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        res, _ = steric(d, domain=domain)
    side.synchronize()
    assert_bit_equal(res["steric"].values, base["steric"].values)
    if domain == "local":
        assert_bit_equal(res["delta_rho"].values, base["delta_rho"].values)


def test_concurrent_calls_from_a_thread_pool(monkeypatch):
    """The reference's functions are called from dask's thread pool (examples/example.ipynb runs on
    a LocalCluster with threads): several steric() / thermosteric() calls at once, host inputs, both
    domains, float64 and float32 -- each with its own upload and download workers, all sharing the
    library's copy team and the device's default stream -- give the bits of the same calls made one
    after the other, and leave no worker thread behind."""
    import threading
    from concurrent.futures import ThreadPoolExecutor

    from momlevel_amd import engine, hostio, thermosteric

    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 2)
    monkeypatch.setattr(hostio, "PIECE_BYTES", 1 << 20)  # several staging pieces per chunk
    jobs = []
    for i, (fn, domain, dtype) in enumerate([(steric, "local", np.float64), (steric, "global", np.float64),
                                             (thermosteric, "local", np.float32), (steric, "local", np.float32),
                                             (thermosteric, "global", np.float64), (steric, "global", np.float32)]):
        jobs.append((fn, _masked_dataset(nt=7, nz=12, ny=64, nx=96, seed=40 + i, dtype=dtype), domain))

    def call(job):
        fn, d, domain = job
        res, ref = fn(d, domain=domain)
        return {k: np.asarray(res[k].values) for k in res.data_vars}

    expected = [call(j) for j in jobs]
    with ThreadPoolExecutor(4) as pool:
        for _ in range(2):
            got = list(pool.map(call, jobs))
            for e, g_ in zip(expected, got):
                assert set(e) == set(g_)
                for k in e:
                    assert_bit_equal(g_[k], e[k], k)
    assert not [t for t in threading.enumerate() if t.name.startswith(("mlx-upload", "mlx-download"))]


def test_time_chunks_stop_early_without_hanging(monkeypatch):
    """a consumer that leaves the chunk loop early (an exception of its own, a `return`) shuts the
    upload worker down with the generator"""
    import threading

    from momlevel_amd import engine

    r = np.random.default_rng(3)
    T = r.uniform(0, 30, (9, 4, 64, 96))
    S = r.uniform(30, 40, (9, 4, 64, 96))
    chunks = engine.TimeChunks(T, S, torch.device("cuda", 0), steps=2)
    seen = []
    for t0, t1, Tc, Sc in chunks:
        seen.append((t0, t1))
        assert np.array_equal(Tc.cpu().numpy(), T[t0:t1])
        if len(seen) == 2:
            break
    del chunks
    import gc

    gc.collect()
    assert seen == [(0, 2), (2, 4)]
    assert not [t for t in threading.enumerate() if t.name.startswith("mlx-upload")]


@pytest.mark.parametrize("resident", [False, True])
def test_local_variants_come_from_one_pass(resident, monkeypatch):
    """steric_variants(domain="local") with all three variants: one launch of the all-variants K2
    per time chunk, no single-variant launch; results == the three steric() calls"""
    from momlevel_amd import core, engine, steric_variants

    d = _masked_dataset(nt=7)
    if resident:
        dd = d.copy()
        for k in ("thetao", "so", "volcello"):
            dd[k] = DataArray(torch.from_numpy(d[k].values).cuda(), d[k].dims)
    else:
        dd = d
    calls = {"decomp": 0, "single": 0}
    real_decomp, real_single = core.steric_local_decomp, core.steric_local

    def count_decomp(*a, **k):
        calls["decomp"] += 1
        return real_decomp(*a, **k)

    def count_single(*a, **k):
        calls["single"] += 1
        return real_single(*a, **k)

    monkeypatch.setattr(core, "steric_local_decomp", count_decomp)
    monkeypatch.setattr(core, "steric_local", count_single)
    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 3)
    results, _ = steric_variants(dd, domain="local")
    assert calls["single"] == 0 and calls["decomp"] == (1 if resident else 3)
    monkeypatch.setattr(core, "steric_local", real_single)
    for variant in ("steric", "thermosteric", "halosteric"):
        single, _ = steric(d, variant=variant)
        assert_bit_equal(results[variant][variant].values, single[variant].values, variant)
        assert_bit_equal(results[variant]["delta_rho"].values, single["delta_rho"].values)


def test_delta_rho_can_be_elided(monkeypatch):
    d = _masked_dataset()
    base, _ = steric(d)
    monkeypatch.setenv("MOMLEVEL_AMD_DELTA_RHO", "0")
    res, _ = steric(d)
    assert "delta_rho" not in res
    assert_bit_equal(res["steric"].values, base["steric"].values)


def test_annual_means_fused_on_device_match_the_oracle(monkeypatch):
    """annual=True, domain='local': the days-in-month weighted means are taken on the device behind
    K2 (mlx_group_weighted_mean), 12-step chunks; bit-identical to the host formula."""
    from momlevel_amd import engine

    od = o.generate_test_data(start_year=1983, nyears=2, calendar="julian")
    ores, _ = o.steric(od["thetao"], od["so"], od["volcello"], od["areacello"], od["z_l"],
                       od["z_i"], od["deptho"])
    st = o.annual_average(ores["steric"], od["time_year"], od["time_days_in_month"])
    dr = o.annual_average(ores["delta_rho"], od["time_year"], od["time_days_in_month"])
    from momlevel_amd import core

    calls = []
    real = core.group_weighted_mean

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(core, "group_weighted_mean", spy)
    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 12)
    res, _ = steric(dset3, annual=True)
    assert calls, "the fused device epilogue was not used"
    assert len(res["time"]) == 2 and res["time"].values[1].year == 1984
    assert_bit_equal(res["steric"].values, st, "annual steric")
    assert_bit_equal(res["delta_rho"].values, dr, "annual delta_rho")
    assert res["steric"].dims == ("time", "yh", "xh")
    gres, _ = steric(dset3, annual=True, domain="global")  # tiny: host formula
    assert len(gres["time"]) == 2 and gres["steric"].dims == ("time",)


def test_annual_average_of_device_resident_results():
    d = dset3.copy()
    for k in ("thetao", "so", "volcello"):
        d[k] = DataArray(torch.from_numpy(dset3[k].values).cuda(), dset3[k].dims)
    res, _ = steric(d, annual=True)
    base, _ = steric(dset3, annual=True)
    assert res["steric"].is_device
    assert_bit_equal(res["steric"].values, base["steric"].values)
    assert_bit_equal(res["delta_rho"].values, base["delta_rho"].values)
    monthly, _ = steric(d)  # util.annual_average on device-backed monthly results
    ann = util.annual_average(monthly)
    assert ann["steric"].is_device
    assert_bit_equal(ann["steric"].values, base["steric"].values)


@pytest.mark.parametrize("domain", ["local", "global"])
def test_a_float32_depth_coordinate_is_followed_or_refused_never_widened(domain, wright_vectors):
    """steric.py:96 / reference.py:53-54: ``pres = dset[zcoord] * 1e4 + patm`` has the COORDINATE's
    dtype.  float32 z_l against float64 theta / S: numpy widens the float32 pressure exactly where it
    meets them -- followed bit for bit.  float32 z_l against float32 theta AND S: numpy evaluates the
    whole equation of state in float32 -- refused on the steric path (no kernel restates it), and
    followed by derived.calc_rho (mlx_eos_map_promote), pinned to the REFERENCE module's own output
    (tests/golden/wright_vectors.npz f32z_*).  Rounds 3-5 widened the coordinate silently
    (VERDICT r5 item 5)."""
    from momlevel_amd import derived

    setup_reference_state = reference_mod.setup_reference_state

    d = _masked_dataset(nt=4)
    z32 = d["z_l"].values.astype(np.float32)
    assert not np.array_equal(z32.astype(np.float64) * 1.0e4 + 101325.0,
                              (z32 * 1.0e4 + 101325.0).astype(np.float64))  # float32 rounding shows
    d32z = d.copy()
    d32z["z_l"] = DataArray(z32, ("z_l",))
    # float64 fields: followed -- the oracle on the same float32 coordinate, bit for bit
    res, ref = steric(d32z, domain=domain)
    pres32 = o.pressure_from_depth(z32)
    assert pres32.dtype == np.float32
    rho0 = o.calc_rho(d["thetao"].values[0], d["so"].values[0], pres32)
    assert rho0.dtype == np.float64
    assert_bit_equal(ref["rho"].values, rho0, "rho0 with a float32 depth coordinate")
    wide, wref = steric(d, domain=domain)
    assert not np.array_equal(ref["rho"].values, wref["rho"].values, equal_nan=True)
    if domain == "local":
        ores, _ = o.steric(d["thetao"].values, d["so"].values, d["volcello"].values,
                           d["areacello"].values, z32, d["z_i"].values, d["deptho"].values)
        assert_bit_equal(res["delta_rho"].values, ores["delta_rho"], "delta_rho, float32 z_l")
        assert_bit_equal(res["steric"].values, ores["steric"], "eta, float32 z_l")
    # float32 fields too: refused, with a message that says what numpy would do
    f32 = d32z.copy()
    for k in ("thetao", "so"):
        f32[k] = DataArray(d[k].values.astype(np.float32), d[k].dims)
    with pytest.raises(TypeError, match="float32.*whole equation of state in float32"):
        steric(f32, domain=domain)
    with pytest.raises(TypeError, match="convert the coordinate to float64"):
        setup_reference_state(f32)
    # ... one float64 field, or a float64 patm DataArray, and numpy promotes: accepted
    mixed = f32.copy()
    mixed["so"] = d["so"]
    steric(mixed, domain=domain)
    steric(f32, domain=domain, patm=DataArray(np.float64(101325.0), ()))
    # calc_rho FOLLOWS: float32 throughout, the reference module's own bits
    v = wright_vectors
    T32, S32 = v["f32_T"], v["f32_S"]
    dims = ("time", "z_l", "yh", "xh")
    coords = {"z_l": DataArray(v["f32z_z"], ("z_l",))}
    pres = DataArray(v["f32z_pres"], ("z_l",), coords)
    rho = derived.calc_rho(DataArray(T32, dims, coords), DataArray(S32, dims, coords), pres)
    assert rho.values.dtype == np.float32
    assert_bit_equal(rho.values, v["f32z_density"], "calc_rho, float32 fields and pressure")
    rho = derived.calc_rho(DataArray(v["blk_T"], dims, coords), DataArray(v["blk_S"], dims, coords), pres)
    assert_bit_equal(rho.values, v["f32z_density_f64fields"], "calc_rho, float64 fields, float32 pressure")


def test_steric_inside_an_except_block_completes_the_reference_density(monkeypatch):
    """a host-input steric() that SUCCEEDS while its caller is handling an
    exception of its own finishes the deferred rho0 download like any other call (it used to be
    treated as failed: jobs cancelled, errors swallowed) -- reference["rho"] bit for bit the plain
    call's, on the deferred path (the threshold is made small enough for the test grid)."""
    from momlevel_amd import hostio

    monkeypatch.setattr(hostio, "SMALL_BYTES", 1 << 10)
    d = _masked_dataset(nt=5, nz=9, ny=28, nx=40)
    deferred = []
    real = hostio.Downloader.finish
    monkeypatch.setattr(hostio.Downloader, "finish", lambda self: deferred.append(1) or real(self))
    base, bref = steric(d, domain="global")  # (global: the ONLY Downloader is the pending rho0's)
    assert len(deferred) == 1, "the test grid must take the deferred rho0 path"
    try:
        raise KeyError("the caller's own, handled")
    except KeyError:
        res, ref = steric(d, domain="global")
        lres, lref = steric(d)
    assert len(deferred) >= 3
    assert_bit_equal(ref["rho"].values, bref["rho"].values)
    assert_bit_equal(lref["rho"].values, bref["rho"].values)
    assert not np.isnan(ref["rho"].values).all()
    assert_bit_equal(res["steric"].values, base["steric"].values)
