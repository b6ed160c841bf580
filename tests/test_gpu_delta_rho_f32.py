"""GPU: the opt-in float32 ``delta_rho`` (MOMLEVEL_AMD_DELTA_RHO_DTYPE=encoding,
``steric_variants(delta_rho_dtype="encoding")``, ``core.steric_local(delta_rho_dtype=torch.float32)``).

Expected value everywhere: ``oracle delta_rho (float64).astype(np.float32)``, to the last bit, and
the array IS float32.  No tolerance: the float64 field is bit-identical to numpy under the exact
policy, and one IEEE round-to-nearest-even conversion (what ``astype`` does, what v_cvt_f32_f64
does) is deterministic.  The device's float32 denormal mode cannot enter: rho is about 1e3, so a
non-zero ``rho - rho0`` is at least one ulp of that, ~1e-13, thirty orders of magnitude above the
float32 subnormals (1e-38), and never near the float32 maximum -- ``_expected`` asserts that the
narrowed expectation holds no subnormal, no infinity and no -0.0.  Time level 0 of a self-made
reference state is exactly +0.0 and part of every case (the helper checks the sign of zero); every
NaN must come out as the float32 quiet NaN 0x7FC00000.  The height field and the reference density
must be bit-equal to the same call WITHOUT the switch: eta sums the unrounded float64 terms.
"""

import numpy as np
import pytest
import torch

from momlevel_amd import _lib, core, engine, halosteric, steric, steric_variants, synthetic, thermosteric
from momlevel_amd.labeled import DataArray, Dataset
from momlevel_amd.test_data import generate_test_data
from oracle import momlevel_numpy as o
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

SWITCH = "MOMLEVEL_AMD_DELTA_RHO_DTYPE"
FUNCS = {"steric": steric, "thermosteric": thermosteric, "halosteric": halosteric}
VARIANTS = ("steric", "thermosteric", "halosteric")
# (17, 2, 2, 2052): the float32-egress shapes (16 steps, or 6 in the all-in-one pass, by 2 columns
# per thread) on 9 column blocks and 2 or 3 time blocks, both ragged; the other planes fit one block
SHAPES = [(6, 9, 14, 20), (3, 5, 7, 9), (5, 4, 7, 9), (17, 4, 6, 16), (17, 2, 2, 2052)]
# (thetao dtype, so dtype, MOMLEVEL_AMD_F32_MODE)
KINDS = {
    "f64": (np.float64, np.float64, None),
    "f32": (np.float32, np.float32, "faithful"),
    "f32_upcast": (np.float32, np.float32, "upcast"),
    "t32_s64": (np.float32, np.float64, None),
    "t64_s32": (np.float64, np.float32, None),
}


def _masked_dataset(nt=6, nz=9, ny=14, nx=20, seed=7, dtypes=(np.float64, np.float64)):
    """MOM6-like case with land / below-bottom NaNs (as tests/test_gpu_steric.py builds it)"""
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
    d["thetao"] = DataArray(T.astype(dtypes[0]), dims)
    d["so"] = DataArray(S.astype(dtypes[1]), dims)
    d["volcello"] = DataArray(vol, dims)
    d["areacello"] = DataArray(g["areacello"], ("yh", "xh"))
    d["deptho"] = DataArray(g["deptho"], ("yh", "xh"))
    return d


def _oracle(d, upcast=False, **kw):
    T, S = d["thetao"].values, d["so"].values
    if upcast:  # MOMLEVEL_AMD_F32_MODE=upcast: float64 arithmetic on the float32 values
        T, S = T.astype(np.float64), S.astype(np.float64)
    return o.steric(T, S, d["volcello"].values, d["areacello"].values, d["z_l"].values,
                    d["z_i"].values, d["deptho"].values, **kw)


def _expected(delta_rho64):
    """float32(oracle's float64 delta_rho), and the facts the module docstring relies on"""
    assert delta_rho64.dtype == np.float64
    e = delta_rho64.astype(np.float32)
    finite = e[~np.isnan(e)]
    assert not np.isinf(finite).any()
    nz64 = delta_rho64[~np.isnan(delta_rho64)] != 0.0
    assert (finite[nz64] != 0.0).all(), "a non-zero value was flushed to zero"
    assert (np.abs(finite[finite != 0.0]) >= np.finfo(np.float32).tiny).all(), "subnormal"
    assert not np.signbit(finite[finite == 0.0]).any(), "-0.0"
    assert (finite == 0.0).any(), "time level 0 holds exact zeros"
    return e


def _check_field(got, delta_rho64, what):
    got = np.asarray(got)
    assert got.dtype == np.float32, f"{what}: {got.dtype}"
    assert_bit_equal(got, _expected(delta_rho64), what)
    nan_bits = got.view(np.uint32)[np.isnan(got)]
    assert nan_bits.size and (nan_bits == 0x7FC00000).all(), f"{what}: NaN payload"


def _kernel_args():
    name = _lib.last_kernel()
    assert name.startswith("k_steric_local<") and name.endswith(">")
    return name[len("k_steric_local<"):-1].split(",")


# 5 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_public_api_with_the_environment_switch(variant, shape, kind, monkeypatch):
    """steric / thermosteric / halosteric, every theta/S dtype family; even planes take the fast
    kernels, the odd 7x9 plane the generic twin, nt=17 a ragged time block"""
    dt_T, dt_S, f32_mode = KINDS[kind]
    if f32_mode:
        monkeypatch.setenv("MOMLEVEL_AMD_F32_MODE", f32_mode)
    d = _masked_dataset(*shape, dtypes=(dt_T, dt_S))
    monkeypatch.delenv(SWITCH, raising=False)
    base, bref = FUNCS[variant](d)
    assert base["delta_rho"].values.dtype == np.float64
    assert "f32out" not in _lib.last_kernel()
    monkeypatch.setenv(SWITCH, "encoding")
    res, ref = FUNCS[variant](d)
    args = _kernel_args()
    assert args[-1] == "f32out", _lib.last_kernel()
    assert args[5] == ("false" if (shape[2] * shape[3]) % 4 == 0 else "true"), _lib.last_kernel()
    ores, _ = _oracle(d, upcast=f32_mode == "upcast", variant=variant)
    _check_field(res["delta_rho"].values, ores["delta_rho"], f"delta_rho {variant} {kind}")
    # eta is summed from the UNROUNDED terms; the reference state has nothing to do with the switch
    assert res[variant].values.dtype == np.float64
    assert_bit_equal(res[variant].values, base[variant].values, f"eta {variant} {kind}")
    assert_bit_equal(res[variant].values, ores[variant], f"eta vs oracle {variant} {kind}")
    assert_bit_equal(ref["rho"].values, bref["rho"].values, "reference rho")
    # metadata as ever
    assert res["delta_rho"].encoding["dtype"] == "float32"
    assert res["delta_rho"].attrs == base["delta_rho"].attrs
    assert res["delta_rho"].dims == base["delta_rho"].dims


# 6 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_all_variants_in_one_pass(resident, dtype, monkeypatch):
    """steric_variants(delta_rho_dtype="encoding"): one launch of the all-variants, float32-out K2
    per time chunk; each field equals its single-call field; device inputs give float32 device
    tensors"""
    monkeypatch.delenv(SWITCH, raising=False)
    d = _masked_dataset(nt=7, dtypes=(dtype, dtype))
    dd = d
    if resident:
        dd = d.copy()
        for k in ("thetao", "so", "volcello"):
            dd[k] = DataArray(torch.from_numpy(d[k].values).cuda(), d[k].dims)
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
    results, _ = steric_variants(dd, domain="local", delta_rho_dtype="encoding")
    assert calls["single"] == 0 and calls["decomp"] == (1 if resident else 3)
    args = _kernel_args()
    assert args[3] == "3" and args[-1] == "f32out", _lib.last_kernel()
    monkeypatch.setattr(core, "steric_local", real_single)
    monkeypatch.setenv(SWITCH, "encoding")
    for variant in VARIANTS:
        field = results[variant]["delta_rho"]
        if resident:
            assert field.is_device and field.data.dtype == torch.float32
            assert results[variant][variant].is_device
            assert results[variant][variant].data.dtype == torch.float64
        single, _ = steric(d, variant=variant)
        ores, _ = _oracle(d, variant=variant)
        _check_field(field.values, ores["delta_rho"], f"one pass {variant}")
        assert single["delta_rho"].values.dtype == np.float32
        assert_bit_equal(field.values, single["delta_rho"].values, f"one pass vs single {variant}")
        assert_bit_equal(results[variant][variant].values, single[variant].values, variant)
        assert_bit_equal(results[variant][variant].values, ores[variant], f"eta {variant}")
    # the keyword wins over the environment, both ways
    off, _ = steric_variants(dd, domain="local", delta_rho_dtype="float64")
    assert np.asarray(off["steric"]["delta_rho"].values).dtype == np.float64
    assert "f32out" not in _lib.last_kernel()
    with pytest.raises(ValueError, match="delta_rho_dtype"):
        steric_variants(dd, domain="local", delta_rho_dtype="float32")


# 7 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_several_time_chunks_equal_one(dtype, monkeypatch):
    monkeypatch.setenv(SWITCH, "encoding")
    d = _masked_dataset(nt=7, dtypes=(dtype, dtype))
    whole = {v: FUNCS[v](d)[0] for v in VARIANTS}
    many_whole, _ = steric_variants(d, domain="local")
    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 2)
    for v in VARIANTS:
        res, _ = FUNCS[v](d)
        assert res["delta_rho"].values.dtype == np.float32
        assert_bit_equal(res["delta_rho"].values, whole[v]["delta_rho"].values, f"chunked {v}")
        assert_bit_equal(res[v].values, whole[v][v].values, f"chunked eta {v}")
    many, _ = steric_variants(d, domain="local")
    for v in VARIANTS:
        assert many[v]["delta_rho"].values.dtype == np.float32
        assert_bit_equal(many[v]["delta_rho"].values, whole[v]["delta_rho"].values, f"one pass {v}")
        assert_bit_equal(many_whole[v]["delta_rho"].values, whole[v]["delta_rho"].values)
    ores, _ = _oracle(d)
    _check_field(whole["steric"]["delta_rho"].values, ores["delta_rho"], "whole")


def test_chunks_get_longer(monkeypatch):
    """the bytes-per-step estimate that sizes the time chunks follows the dtype: 4 B instead of 8
    per cell of a host result"""
    seen = []
    real = engine.TimeChunks

    def spy(*a, **k):
        seen.append(k["extra_bytes_per_step"])
        return real(*a, **k)

    monkeypatch.setattr(engine, "TimeChunks", spy)
    d = _masked_dataset()
    monkeypatch.delenv(SWITCH, raising=False)
    steric(d)
    monkeypatch.setenv(SWITCH, "encoding")
    steric(d)
    cells = 9 * 14 * 20
    assert seen == [8 * cells, 4 * cells]


# 8 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [False, True])
def test_annual_means_are_narrowed_after_the_mean(resident, monkeypatch):
    """annual=True: float32(float64 annual mean of the float64 field), never a mean of rounded
    values"""
    od = o.generate_test_data(start_year=1983, nyears=2, calendar="julian")
    ores, _ = o.steric(od["thetao"], od["so"], od["volcello"], od["areacello"], od["z_l"],
                       od["z_i"], od["deptho"])
    st = o.annual_average(ores["steric"], od["time_year"], od["time_days_in_month"])
    dr = o.annual_average(ores["delta_rho"], od["time_year"], od["time_days_in_month"])
    rounded_first = o.annual_average(ores["delta_rho"].astype(np.float32).astype(np.float64),
                                     od["time_year"], od["time_days_in_month"]).astype(np.float32)
    assert (rounded_first != dr.astype(np.float32)).any()  # (the two orders do differ on this data)
    d = generate_test_data(start_year=1983, nyears=2, calendar="julian")
    if resident:
        host = d
        d = host.copy()
        for k in ("thetao", "so", "volcello"):
            d[k] = DataArray(torch.from_numpy(host[k].values).cuda(), host[k].dims)
    monkeypatch.setenv(SWITCH, "encoding")
    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 12)
    res, _ = steric(d, annual=True)
    got = res["delta_rho"].values
    assert got.dtype == np.float32 and got.shape[0] == 2
    assert res["delta_rho"].is_device == resident
    assert_bit_equal(got, dr.astype(np.float32), "annual delta_rho")
    assert res["steric"].values.dtype == np.float64
    assert_bit_equal(res["steric"].values, st, "annual steric")


# 9 ---------------------------------------------------------------------------------------------
def test_float64_encoding_and_elided_field_are_untouched(monkeypatch):
    d = _masked_dataset()
    monkeypatch.delenv(SWITCH, raising=False)
    base, _ = steric(d, dtype="float64")
    monkeypatch.setenv(SWITCH, "encoding")
    res, _ = steric(d, dtype="float64")
    assert "f32out" not in _lib.last_kernel()
    assert res["delta_rho"].values.dtype == np.float64
    assert res["delta_rho"].encoding["dtype"] == "float64"
    assert_bit_equal(res["delta_rho"].values, base["delta_rho"].values)
    assert_bit_equal(res["steric"].values, base["steric"].values)
    monkeypatch.setenv("MOMLEVEL_AMD_DELTA_RHO", "0")
    res, _ = steric(d)
    assert "delta_rho" not in res and "f32out" not in _lib.last_kernel()
    assert_bit_equal(res["steric"].values, base["steric"].values)
    monkeypatch.delenv("MOMLEVEL_AMD_DELTA_RHO")
    # the global domain has no such field and ignores the switch
    g_on, _ = steric(d, domain="global")
    monkeypatch.delenv(SWITCH)
    g_off, _ = steric(d, domain="global")
    assert_bit_equal(g_on["steric"].values, g_off["steric"].values)
    monkeypatch.setenv(SWITCH, "float32")
    with pytest.raises(ValueError, match=SWITCH):
        steric(d)


# 10 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fused_arithmetic_is_narrowed_the_same_way(dtype, monkeypatch):
    """MOMLEVEL_AMD_ARITH=fused has no numpy twin: this pins only the conversion -- float32 of the
    fused float64 field of the same build"""
    monkeypatch.setenv("MOMLEVEL_AMD_ARITH", "fused")
    d = _masked_dataset(nt=5, dtypes=(dtype, dtype))
    for variant in VARIANTS:
        monkeypatch.delenv(SWITCH, raising=False)
        base, _ = FUNCS[variant](d)
        args64 = _kernel_args()
        monkeypatch.setenv(SWITCH, "encoding")
        res, _ = FUNCS[variant](d)
        args = _kernel_args()
        assert args[7] == "true" and args[:-1] == args64, _lib.last_kernel()  # MLX_FLAG_FMA, same shape
        _check_field(res["delta_rho"].values, base["delta_rho"].values, f"fused {variant}")
        assert_bit_equal(res[variant].values, base[variant].values, f"fused eta {variant}")


# 11 --------------------------------------------------------------------------------------------
def test_core_refuses_an_output_of_the_other_dtype():
    d = _masked_dataset()
    T = torch.from_numpy(d["thetao"].values).cuda()
    S = torch.from_numpy(d["so"].values).cuda()
    vol0 = torch.from_numpy(d["volcello"].values[0]).cuda()
    pres = o.pressure_from_depth(d["z_l"].values)
    rho0m = core.fold_mask(core.eos_map(T[0], S[0], pres), vol0)
    kw = dict(z_i=d["z_i"].values, deptho=d["deptho"].values)
    ops = (T, S, rho0m, vol0[0], pres, -1.0 / 1035.0)
    out32 = torch.empty(T.shape, dtype=torch.float32, device="cuda")
    out64 = torch.empty(T.shape, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="delta_rho_out"):
        core.steric_local(*ops, delta_rho_out=out32, **kw)
    with pytest.raises(ValueError, match="delta_rho_out"):
        core.steric_local(*ops, delta_rho_out=out64, delta_rho_dtype=torch.float32, **kw)
    with pytest.raises(ValueError, match="delta_rho_dtype"):
        core.steric_local(*ops, delta_rho_dtype=torch.float16, **kw)
    all32 = torch.empty((3,) + tuple(T.shape), dtype=torch.float32, device="cuda")
    all64 = torch.empty((3,) + tuple(T.shape), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="float64"):
        core.steric_local_decomp(T, S, T[0], S[0], *ops[2:], delta_rho_out=all32, **kw)
    with pytest.raises(ValueError, match="float32"):
        core.steric_local_decomp(T, S, T[0], S[0], *ops[2:], delta_rho_out=all64,
                                 delta_rho_dtype=torch.float32, **kw)
    # and what it accepts: caller-provided outputs of the right dtype, filled in place
    d64, e64 = core.steric_local(*ops, delta_rho_out=out64, **kw)
    d32, e32 = core.steric_local(*ops, delta_rho_out=out32, delta_rho_dtype=torch.float32, **kw)
    assert d32 is out32 and d64 is out64
    _check_field(d32.cpu().numpy(), d64.cpu().numpy(), "caller-provided output")
    assert_bit_equal(e32.cpu().numpy(), e64.cpu().numpy(), "eta")
    a32, f32 = core.steric_local_decomp(T, S, T[0], S[0], *ops[2:], delta_rho_out=all32,
                                        delta_rho_dtype=torch.float32, **kw)
    assert a32 is all32
    _check_field(a32[0].cpu().numpy(), d64.cpu().numpy(), "all-variants output, steric row")
    assert_bit_equal(f32[0].cpu().numpy(), e64.cpu().numpy(), "all-variants eta")
    # a 4- but not 16-byte aligned float32 output takes the generic twin: same bits
    buf = torch.empty(T.numel() + 1, dtype=torch.float32, device="cuda")
    odd = buf[1:].view(T.shape)
    assert odd.data_ptr() % 8 == 4
    core.steric_local(*ops, delta_rho_out=odd, delta_rho_dtype=torch.float32, **kw)
    args = _kernel_args()
    assert args[5] == "true" and args[-1] == "f32out", _lib.last_kernel()
    assert torch.equal(odd.view(torch.int32), out32.view(torch.int32))


# 12 --------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_full_size_plane_float32_fields_thermosteric():
    """the 0.25-degree plane (1080 x 1440 x 75), float32 theta/S, thermosteric (S held at the
    reference slab), float32 egress against oracle slabs held one at a time"""
    nt, nz, ny, nx = 5, 75, 1080, 1440
    g = synthetic.make_grid(ny, nx, nz)
    vol0 = torch.from_numpy(g["volcello"]).cuda()
    kw = dict(seed=synthetic.SEED, mask3d=vol0)
    T = core.synth_field((nt, nz, ny, nx), torch.float32, field_id=1, lo=-2.0, scale=34.0, **kw)
    S0 = core.synth_field((1, nz, ny, nx), torch.float32, field_id=2, lo=30.0, scale=10.0, **kw)[0]
    pres = o.pressure_from_depth(g["z_l"])
    rho0 = core.eos_map(T[0], S0, pres)
    rho0m = core.fold_mask(rho0, vol0)
    ops = (T, S0, rho0m, vol0[0], pres, -1.0 / 1035.0)
    drho, eta = core.steric_local(*ops, z_i=g["z_i"], deptho=g["deptho"],
                                  delta_rho_dtype=torch.float32)
    args = _kernel_args()
    assert args[0] == "float" and args[3] == "2" and args[5] == "false" and args[-1] == "f32out"
    assert drho.dtype == torch.float32 and eta.dtype == torch.float64
    _, eta64 = core.steric_local(*ops, z_i=g["z_i"], deptho=g["deptho"], want_delta_rho=False)
    assert torch.equal(eta.view(torch.int64), eta64.view(torch.int64))
    wet3 = ~np.isnan(g["volcello"])
    hk = dict(seed=synthetic.SEED, mask3d=g["volcello"], dtype=np.float32)
    Sn = synthetic.field_numpy((1, nz, ny, nx), field_id=2, lo=30.0, scale=10.0, t0=0, **hk)[0]
    rho0_ref = None
    for t in range(nt):
        Tn = synthetic.field_numpy((1, nz, ny, nx), field_id=1, lo=-2.0, scale=34.0, t0=t, **hk)[0]
        rho = o.calc_rho(Tn, Sn, pres)
        if t == 0:
            rho0_ref = rho
        d = np.where(wet3, rho - rho0_ref, np.nan)
        got = drho[t].cpu().numpy()
        assert got.dtype == np.float32
        e = d.astype(np.float32)
        assert_bit_equal(got, e, f"delta_rho t={t}")
        nan_bits = got.view(np.uint32)[np.isnan(got)]
        assert (nan_bits == 0x7FC00000).all()
        nonzero = e[~np.isnan(e) & (d != 0.0)]
        assert (np.abs(nonzero) >= np.finfo(np.float32).tiny).all()  # (no subnormal, none flushed)
