"""GPU: WHERE the entry points of momlevel_amd/core.py write -- the result-buffer contract
("Result buffers") over every entry point that takes a caller's buffer.

One table, ROWS: a row builds small valid operands for a case, names its result argument(s) and
the operands the kernel reads, and carries the numpy restatement its kernel's own suite compares
with (taken as it stands, with that suite's gate: bit equality wherever that is the standing gate).

(1) REFUSALS AND OVERLAP.  ``core._call`` is replaced by a spy that records the entry name and
    returns: no test of this part launches anything, and a check that is missing shows up as "the
    spy was called", never as a kernel writing through a bad pointer.  For every row a result of
    the other float dtype, one element short along each axis, of the same numel in another shape,
    a non-contiguous view of the right shape, a host tensor, each named operand itself, a result
    that shares the LAST element of an operand, and two results of one call that share an element
    are each a ``ValueError`` with no spy call; a result that only touches an operand, carved from
    one buffer with it, reaches the spy once per expected launch.

(2) GUARD BANDS, valid buffers only.  The result is a view inside a buffer filled with a
    sentinel NaN (tests/out_contract.py), GUARD elements before and after it, starting 16-byte
    aligned and one element past an aligned address: the packed path and the cell-by-cell path
    where the row has both (asked of the library where it has a query: eos_map_path,
    eos_map_promote_path, vort_records_per_launch).  After the call: the entry point returned the
    view itself; every guard element and every element of a stride gap still holds the sentinel
    bits; no element of the view does; the view meets the restatement.
    Shapes: the smallest that end mid-pack, on a pack boundary with a partial block, and at one
    cell.  The two stream probes take whole 16-byte packs on 16-byte boundaries only (their
    header): every other case must be refused by the library with the buffer left as it was.
"""

import numpy as np
import pytest
import torch

import area_numpy as an
import clim_numpy as cn
import column_numpy as col
import filter_numpy as fn
import layer_numpy as ln
import out_contract as oc
import quantile_numpy as qn
import spice_numpy as sn
import vort_numpy as vn
from conftest import assert_bit_equal
from momlevel_amd import _lib, core, synthetic
from oracle import momlevel_numpy as o

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = np.float64, np.float32
TD = {F64: torch.float64, F32: torch.float32}
NAN = float("nan")
FLAT = (1, 5, 1028, 1029)  # one cell; mid-pack; whole packs past one block of 256 lanes; + a tail
NT = 13  # the time records: 13 steps -- one group of 13, or a group of 12 and a group of 1
PROF = np.array([101325.0, 1.23456789e7, 4.0e7 + 0.125])  # the pressure of the 3 levels
P_WEAK, G = 2.0e7 + 0.5, 9.81
NEG_INV = -1.0 / 1035.0
Z_LAYER = np.array([0.0, 5.0, 15.0, 40.0, 90.0, 200.0, 350.0, 600.0])  # 7 levels' interfaces
Z_COLUMN = np.array([2.5, 10.0, 20.0, 32.5, 51.25, 75.0, 120.0])  # 7 level depths
W64, _W32, H, _BANDS = (_lib.VORT_TILE_LANES * 2, _lib.VORT_TILE_LANES * 4, _lib.VORT_TILE_H,
                        _lib.VORT_TILE_BANDS)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _name(dtype):
    return np.dtype(dtype).name


def _equal_values(got, ref, what):
    """the gate of the layer and column suites: bit equality, NaN placement included; +0.0 == -0.0"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, f"{what}: {got.dtype} {got.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN placement"
    m = ~np.isnan(ref)
    bad = got[m] != ref[m]
    assert not bad.any(), f"{what}: {int(bad.sum())} of {int(m.sum())} values differ"


def _same_bits(got, ref, what):
    """the gate of the vorticity and gather suites: the integer views agree"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, f"{what}: {got.dtype} {got.shape}"
    view = np.int64 if ref.dtype == F64 else np.int32
    differ = np.ascontiguousarray(got).view(view) != np.ascontiguousarray(ref).view(view)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {ref.size} elements differ in bits"


class Row:
    """One entry point on one case.  ``ops``: name -> device tensor, the operands whose pointers
    go to the launch; ``call(ops, **results)`` runs the entry point on them; ``outs``: result
    argument -> (shape, torch dtype); ``check(got)``: the restatement's gate on {argument: numpy
    array}; ``entry`` / ``launches``: what the spy must see for valid buffers; ``strides``: result
    argument -> strides of its guarded view (default contiguous); ``path(ops, views, offset)``:
    asserts the path from the library's query; ``refused(offset)``: the library itself refuses the
    case (MomlevelHipError) and must leave the buffer alone."""

    def __init__(self, entry, ops, call, outs, check, launches=1, strides=None, path=None,
                 refused=None, unpack=None):
        self.entry, self.ops, self.call, self.outs, self.check = entry, ops, call, outs, check
        self.launches, self.strides, self.path = launches, strides or {}, path
        self.refused = refused or (lambda offset: False)
        self.unpack = unpack or (lambda ret: {next(iter(outs)): ret})


ROWS = {}  # name -> (builder(case) -> Row, the guard-band cases, the case of the refusal tests)


def row(name, cases, refuse):
    def register(builder):
        ROWS[name] = (builder, list(cases), refuse)
        return builder
    return register


def _ids(case):
    return "-".join(_name(c) if isinstance(c, type) else str(c).replace(" ", "") for c in case)


# ---- the EOS maps -----------------------------------------------------------------------------------
def _eos_fields(n, dtype):
    rng = np.random.default_rng(100 + n)
    shape = (2, 3, 1, n)
    T, S = rng.uniform(-2.0, 32.0, shape).astype(dtype), rng.uniform(30.0, 40.0, shape).astype(dtype)
    T[0, 1, 0, n // 2], S[1, 2, 0, n - 1] = NAN, NAN
    return shape, T, S


def _k0_row(n, dtype, ibh):
    shape, T, S = _eos_fields(n, dtype)
    with np.errstate(all="ignore"):
        if ibh:
            ref = o.inverse_barometer(T, S, PROF[:, None, None], gravity=G, equation_of_state="wright")
        else:
            ref = o.eos_func_from_str("wright", "density")(T, S, PROF[:, None, None])
    ref = np.ascontiguousarray(np.broadcast_to(np.asarray(ref).astype(F64), shape))
    ops = {"thetao": _dev(T), "so": _dev(S), "p": _dev(PROF)}

    def call(ops, **res):
        if ibh:
            return core.inverse_barometer(ops["thetao"], ops["so"], ops["p"], gravity=G, **res)
        return core.eos_map(ops["thetao"], ops["so"], ops["p"], **res)

    def path(ops, views, offset):
        kind = core.eos_map_path(ops["thetao"], ops["so"], ops["p"],
                                 func="inverse_barometer" if ibh else "density", out=views["out"])[0]
        # whole packs of either dtype on aligned pointers: the fast kernel of the density with a
        # level profile; everything else, and the inverse barometer always, cell by cell
        assert kind == ("fast" if not ibh and offset == 0 and n == 1028 else "generic"), kind

    return Row("mlx_inverse_barometer" if ibh else "mlx_eos_map", ops, call,
               {"out": (shape, torch.float64)},
               lambda got: assert_bit_equal(got["out"], ref, f"K0 n={n} {_name(dtype)}"), path=path)


@row("eos_map", [(n, dt) for dt in (F64, F32) for n in FLAT], (6, F64))
def _eos_map(case):
    return _k0_row(case[0], case[1], False)


@row("inverse_barometer", [(n, F64) for n in FLAT], (6, F64))
def _inverse_barometer(case):
    return _k0_row(case[0], case[1], True)


@row("eos_map_promote", [(n,) for n in FLAT], (6,))
def _eos_map_promote(case):
    """T float64, S float32, p a python float: numpy's promotion gives float64"""
    n, = case
    rng = np.random.default_rng(200 + n)
    T, S = rng.uniform(-2.0, 32.0, n), rng.uniform(30.0, 40.0, n).astype(F32)
    T[n // 2] = NAN
    with np.errstate(all="ignore"):
        ref = np.asarray(o.wright_density(T, S, P_WEAK))
    assert ref.dtype == F64

    def path(ops, views, offset):
        width, dtype = core.eos_map_promote_path(ops["T"], ops["S"], P_WEAK, out=views["out"])
        full = core.promote_path("dfw")[0]
        # (one-element OPERANDS count as aligned, include/momlevel_path.h; the result never does)
        assert dtype == torch.float64 and width == (full if offset == 0 else 1), width

    return Row("mlx_eos_map_promote", {"T": _dev(T), "S": _dev(S)},
               lambda ops, **res: core.eos_map_promote(ops["T"], ops["S"], P_WEAK, **res),
               {"out": ((n,), torch.float64)},
               lambda got: assert_bit_equal(got["out"], ref, f"promote n={n}"), path=path)


# ---- K2 -----------------------------------------------------------------------------------------------
def _steric_case(nx, seed):
    nt, nz, ny = 2, 3, 3
    rng = np.random.default_rng(seed)
    shape = (nt, nz, ny, nx)
    T, S = rng.uniform(-2.0, 32.0, shape), rng.uniform(30.0, 40.0, shape)
    vol = rng.uniform(1.0, 2.0, (nz, ny, nx))
    vol[:, 1, 1] = NAN  # land
    vol[2, 0, 2] = NAN  # a shallower column
    dz = rng.uniform(1.0, 50.0, (nz, ny, nx))
    with np.errstate(all="ignore"):
        rho0 = o.wright_density(T[0], S[0], PROF[:, None, None])
    rho0m = np.where(np.isnan(vol), NAN, rho0)
    return shape, T, S, vol, dz, rho0m


def _steric_reference(Tv, Sv, shape, vol, dz, rho0m, ddt):
    with np.errstate(all="ignore"):
        rho = np.broadcast_to(o.wright_density(Tv, Sv, PROF[:, None, None]), shape)
        d = np.where(~np.isnan(vol), rho - rho0m, NAN)  # test_gpu_kernels.py, "band delta_rho"
        eta = np.stack([np.where(~np.isnan(vol[0]), NEG_INV * np.nansum(dz * d[t], axis=0), NAN)
                        for t in range(shape[0])])
    return d.astype(ddt), eta


@row("steric_local", [(4, F64), (3, F64)], (4, F64))
@row("steric_local_drho32", [(4, F32), (3, F32)], (4, F32))
def _steric_local(case):
    """(2, 3, 3, 4): whole packs, the fast kernel; (2, 3, 3, 3): the generic one"""
    nx, ddt = case
    shape, T, S, vol, dz, rho0m = _steric_case(nx, 300 + nx)
    d_ref, e_ref = _steric_reference(T, S, shape, vol, dz, rho0m, ddt)
    ops = {"thetao": _dev(T), "so": _dev(S), "rho0m": _dev(rho0m), "vol0_surface": _dev(vol[0]),
           "dz": _dev(dz), "p": _dev(PROF)}

    def call(ops, **res):
        return core.steric_local(ops["thetao"], ops["so"], ops["rho0m"], ops["vol0_surface"], ops["p"],
                                 NEG_INV, dz=ops["dz"], delta_rho_dtype=TD[ddt], **res)

    def check(got):
        assert_bit_equal(got["delta_rho_out"], d_ref, f"delta_rho nx={nx} {_name(ddt)}")
        assert_bit_equal(got["eta_out"], e_ref, f"eta nx={nx}")

    return Row("mlx_steric_local", ops, call,
               {"delta_rho_out": (shape, TD[ddt]), "eta_out": ((shape[0],) + shape[2:], torch.float64)},
               check, unpack=lambda ret: {"delta_rho_out": ret[0], "eta_out": ret[1]})


STEPS_AROUND = (1, 5)  # the decomposition's results are full[:, 1:3] of five steps


@row("steric_local_decomp", [(4, F64), (3, F64)], (4, F64))
@row("steric_local_decomp_drho32", [(4, F32), (3, F32)], (4, F32))
def _steric_local_decomp(case):
    nx, ddt = case
    shape, T, S, vol, dz, rho0m = _steric_case(nx, 400 + nx)
    T0, S0 = T[0].copy(), S[0].copy()
    refs = [_steric_reference(Tv, Sv, shape, vol, dz, rho0m, ddt)
            for Tv, Sv in ((T, S), (T, S0), (T0, S))]
    d_ref, e_ref = np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs])
    ops = {"thetao": _dev(T), "so": _dev(S), "T0": _dev(T0), "S0": _dev(S0), "rho0m": _dev(rho0m),
           "vol0_surface": _dev(vol[0]), "dz": _dev(dz), "p": _dev(PROF)}

    def call(ops, **res):
        return core.steric_local_decomp(ops["thetao"], ops["so"], ops["T0"], ops["S0"], ops["rho0m"],
                                        ops["vol0_surface"], ops["p"], NEG_INV, dz=ops["dz"],
                                        delta_rho_dtype=TD[ddt], **res)

    def check(got):
        assert_bit_equal(got["delta_rho_out"], d_ref, f"decomp delta_rho nx={nx} {_name(ddt)}")
        assert_bit_equal(got["eta_out"], e_ref, f"decomp eta nx={nx}")

    nt, steps = shape[0], STEPS_AROUND[1]
    outs = {"delta_rho_out": ((3,) + shape, TD[ddt]),
            "eta_out": ((3, nt) + shape[2:], torch.float64)}
    strides = {}
    for name, (full, _) in outs.items():  # full[:, t0:t1] of (3, steps, ...): the variant axis strided
        inner = oc.strides_of(full[1:])
        strides[name] = (steps * inner[0],) + inner
    return Row("mlx_steric_local_decomp", ops, call, outs, check, strides=strides,
               unpack=lambda ret: {"delta_rho_out": ret[0], "eta_out": ret[1]})


# ---- the time records -------------------------------------------------------------------------------
def _record(n, dtype, seed):
    rng = np.random.default_rng(seed)
    y = rng.normal(20.0, 5.0, (NT, n))
    y[rng.random((NT, n)) < 0.1] = NAN
    y[:, n - 1] = rng.normal(20.0, 5.0, NT)  # the last cell holds data throughout ...
    y[NT // 2, n - 1] = NAN  # ... but for one step
    if n >= 5:
        y[:, 2] = NAN  # an all-NaN cell
    return y.astype(dtype)


def _gwm_reference(x, w, group_len):
    """test_gpu_sums_edges.py's: ascending j, the product rounded, then the sum"""
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


@row("group_weighted_mean", [(n,) for n in FLAT], (6,))
def _group_weighted_mean(case):
    n, = case
    x = _record(n, F64, 500 + n)
    w = np.random.default_rng(n).choice([28.0, 29.0, 30.0, 31.0], NT)
    ref = _gwm_reference(x, w, NT)
    return Row("mlx_group_weighted_mean", {"x": _dev(x), "w": _dev(w)},
               lambda ops, **res: core.group_weighted_mean(ops["x"], ops["w"], NT, **res),
               {"out": ((1, n), torch.float64)},
               lambda got: assert_bit_equal(got["out"], ref, f"group mean n={n}"))


@row("time_apply_remove", [(n, dt) for dt in (F64, F32) for n in FLAT], (6, F64))
def _time_apply_remove(case):
    n, dtype = case
    y = _record(n, dtype, 600 + n)
    rng = np.random.default_rng(601 + n)
    x, m, b = np.arange(NT, dtype=F64) * 0.25 + 3.0, rng.normal(0.0, 1.0, n), rng.normal(5.0, 2.0, n)
    ref = y.astype(F64) - (m * x[:, None] + b)  # test_gpu_trend_edges.py _line("remove")
    ops = {"y": _dev(y), "xm": _dev(x), "a": _dev(m), "b": _dev(b)}
    return Row("mlx_time_apply", ops,
               lambda ops, **res: core.time_apply(ops["y"], "remove", ops["xm"], ops["a"], ops["b"], **res),
               {"out": ((NT, n), torch.float64)},
               lambda got: assert_bit_equal(got["out"], ref, f"remove n={n} {_name(dtype)}"))


@row("time_apply_model_resid", [(n, dt) for dt in (F64, F32) for n in FLAT], (6, F64))
def _time_apply_model(case):
    n, dtype = case
    K = 4
    y = _record(n, dtype, 700 + n)
    rng = np.random.default_rng(701 + n)
    M, c = rng.normal(0.0, 1.0, (K, NT)), rng.normal(0.0, 1.0, (K, n))
    r = M[0][:, None] * c[0][None, :]
    for k in range(1, K):  # test_gpu_trend_edges.py: the ascending-k loop
        r = r + M[k][:, None] * c[k][None, :]
    ref = y.astype(F64) - r
    ops = {"y": _dev(y), "xm": _dev(M), "a": _dev(c)}
    return Row("mlx_time_apply", ops,
               lambda ops, **res: core.time_apply(ops["y"], "model_resid", ops["xm"], ops["a"], **res),
               {"out": ((NT, n), torch.float64)},
               lambda got: assert_bit_equal(got["out"], ref, f"model_resid n={n} {_name(dtype)}"))


GROUP_STEPS, GROUP_OFFSETS = list(range(NT)), [0, 12, NT]  # a group of 12 and a group of 1


@row("time_group_stat", [(n, dt) for dt in (F64, F32) for n in FLAT], (6, F64))
def _time_group_stat(case):
    n, dtype = case
    y = _record(n, dtype, 800 + n)
    ref = cn.grouped(y, GROUP_STEPS, GROUP_OFFSETS, "mean").astype(dtype)
    groups = core.upload_groups(GROUP_STEPS, GROUP_OFFSETS, NT, DEV)
    ops = {"y": _dev(y), "steps": groups.steps, "offsets": groups.offsets}

    def call(ops, **res):
        g = core.upload_groups(GROUP_STEPS, GROUP_OFFSETS, NT, DEV)
        g.steps, g.offsets = ops["steps"], ops["offsets"]
        return core.time_group_stat(ops["y"], g, stat="mean", **res)

    return Row("mlx_clim_group_stat", ops, call, {"out": ((2, n), TD[dtype])},
               lambda got: assert_bit_equal(got["out"], ref, f"group mean n={n} {_name(dtype)}"))


@row("time_filter", [(n, dt) for dt in (F64, F32) for n in FLAT], (6, F64))
def _time_filter(case):
    n, dtype = case
    y = _record(n, dtype, 900 + n)
    w = np.array([-0.6, 0.25, 1.0, 0.25, 0.7])
    ref = fn.time_filter(y, w, 2, 3, True).astype(dtype)
    return Row("mlx_filter_apply", {"y": _dev(y), "w": _dev(w)},
               lambda ops, **res: core.time_filter(ops["y"], ops["w"], 2, 3, True, **res),
               {"out": ((NT, n), TD[dtype])},
               lambda got: assert_bit_equal(got["out"], ref, f"filter n={n} {_name(dtype)}"))


@row("time_quantile", [(n, dt) for dt in (F64, F32) for n in FLAT], (6, F64))
def _time_quantile(case):
    n, dtype = case
    y = _record(n, dtype, 1000 + n)
    q = [0.25, 0.5, 1.0]
    ref = qn.time_quantile(y, q)
    ref = qn.rounded_once(ref) if dtype == F32 else ref
    return Row("mlx_quantile_select", {"y": _dev(y)},
               lambda ops, **res: core.time_quantile(ops["y"], q, **res),
               {"out": ((3, 1, n), TD[dtype])},
               lambda got: qn.assert_values(got["out"], ref, f"quantile n={n} {_name(dtype)}"))


# ---- gather, spice ---------------------------------------------------------------------------------------
@row("gauge_gather", [(F64,), (F32,)], (F64,))
def _gauge_gather(case):
    dtype, = case
    nrest, ng, n = 7, 5, 300
    rng = np.random.default_rng(1100)
    y = rng.normal(0.0, 1.0, (nrest, n)).astype(dtype)
    y[3, 17] = NAN
    index = np.array([17, 299, -1, 0, 300], dtype=np.int64)
    ok = (index >= 0) & (index < n)
    ref = np.full((ng, nrest), NAN, dtype=dtype)  # (numpy's NaN is the canonical quiet NaN)
    ref[ok] = y[:, index[ok]].T
    return Row("mlx_gauge_gather", {"y": _dev(y), "index": _dev(index)},
               lambda ops, **res: core.gauge_gather(ops["y"], ops["index"], **res),
               {"out": ((ng, nrest), TD[dtype])},
               lambda got: _same_bits(got["out"], ref, f"gather {_name(dtype)}"))


@row("spice_map", [(n, dt) for dt in (F64, F32) for n in FLAT], (6, F64))
def _spice_map(case):
    n, dtype = case
    vectors, _ = sn.fixture()
    T, S, ref = (np.array(a[:n]) for a in vectors["uni_f64" if dtype == F64 else "uni_f32"])
    assert T.dtype == dtype and S.dtype == dtype and len(T) == n

    def check(got):  # test_gpu_spice.py _gate: the bound of DESIGN.md 3.11, cell by cell
        assert got["out"].dtype == F64 and not np.isnan(got["out"]).any()
        assert np.all(np.abs(got["out"] - ref) <= sn.bound(T, S)), f"spice n={n} {_name(dtype)}"

    return Row("mlx_spice_map", {"theta": _dev(T), "so": _dev(S)},
               lambda ops, **res: core.spice_map(ops["theta"], ops["so"], **res),
               {"out": ((n,), torch.float64)}, check)


# ---- the stencils and the Rossby radius ---------------------------------------------------------------
def _plane(nx, dtype, seed):
    ny = H + 1
    rng = np.random.default_rng(seed)
    return ny, {"u": rng.normal(0.0061, 0.08, (2, ny, nx)).astype(dtype),
                "v": rng.normal(0.00077, 0.04, (2, ny, nx)).astype(dtype),
                "dx": rng.uniform(2.0e4, 3.0e4, (ny, nx)).astype(dtype),
                "dy": rng.uniform(1.0e4, 3.0e4, (ny, nx)).astype(dtype),
                "area": rng.uniform(4.0e8, 9.0e8, (ny, nx)).astype(dtype),
                "zeta": rng.normal(0.0, 1.0e-5, (2, ny, nx)).astype(dtype),
                "coriolis": rng.normal(1.21e-5, 1.1e-4, (ny, nx)).astype(dtype),
                "n2": rng.normal(1.0e-5, 2.0e-5, (2, ny, nx)).astype(dtype)}


def _vort_path(ny, nx, dtype):
    def path(ops, views, offset):
        """nx = W64 + 2 holds whole float64 packs (the packed path, when every pointer is aligned);
        W64 + 1 and every float32 plane of these widths go cell by cell"""
        step = core.vort_records_per_launch(ny, nx, TD[dtype])
        assert (step > 0) == (dtype == F64 and nx == W64 + 2), step
    return path


VORT_CASES = [(nx, dt) for dt in (F64, F32) for nx in (W64 + 2, W64 + 1)]


@row("rel_vort", VORT_CASES, (6, F64))
def _rel_vort(case):
    nx, dtype = case
    ny, h = _plane(nx, dtype, 1200 + nx)
    names = ("u", "v", "dx", "dy", "area")
    ref = vn.rel_vort(*(h[k] for k in names))
    return Row("mlx_vort_rel_vort", {k: _dev(h[k]) for k in names},
               lambda ops, **res: core.rel_vort(*(ops[k] for k in names), **res),
               {"out": ((2, ny, nx), TD[dtype])},
               lambda got: _same_bits(got["out"], ref, f"zeta nx={nx} {_name(dtype)}"),
               path=_vort_path(ny, nx, dtype))


@row("potential_vorticity", VORT_CASES, (6, F64))
def _potential_vorticity(case):
    nx, dtype = case
    ny, h = _plane(nx, dtype, 1300 + nx)
    names = ("zeta", "coriolis", "n2")
    ref = vn.pv(*(h[k] for k in names), gravity=9.8, symmetric=False, units="m", interp=True)
    return Row("mlx_vort_pv", {k: _dev(h[k]) for k in names},
               lambda ops, **res: core.potential_vorticity(*(ops[k] for k in names), gravity=9.8, **res),
               {"out": ((2, ny, nx), TD[dtype])},
               lambda got: _same_bits(got["out"], ref, f"pv nx={nx} {_name(dtype)}"),
               path=_vort_path(ny, nx, dtype))


@row("rossby_radius", [(n, dt) for dt in (F64, F32) for n in FLAT], (6, F64))
def _rossby_radius(case):
    n, dtype = case
    rng = np.random.default_rng(1400 + n)
    c = rng.uniform(0.5, 3.0, (2, n, 3)).astype(dtype)
    f = rng.normal(1.21e-5, 1.1e-4, n).astype(dtype)
    f[n // 2] = 0.0  # numpy's +inf
    ref = vn.rossby_rd(c, f[None, :, None])
    return Row("mlx_vort_rossby", {"c": _dev(c), "f": _dev(f)},
               lambda ops, **res: core.rossby_radius(ops["c"], ops["f"], **res),
               {"out": ((2, n, 3), TD[dtype])},
               lambda got: _same_bits(got["out"], ref, f"rossby n={n} {_name(dtype)}"))


@row("area_anomaly", [(n, dt) for dt in (F64, F32) for n in FLAT], (6, F64))
def _area_anomaly(case):
    n, dtype = case
    rng = np.random.default_rng(1500 + n)
    v = rng.normal(0.0, 1.0, (2, n)).astype(dtype)
    v[1, n // 2] = NAN
    mean = rng.normal(0.0, 0.1, (2, 3))
    slot = rng.integers(-1, 3, n).astype(np.int32)
    slot[n - 1] = 1
    # the plane as one row of n cells, the slots as the labels 0, 1, 2 (test_gpu_area.py: its bits)
    ref = an.area_anomaly(v.reshape(2, 1, n), mean, slot.reshape(1, n), [0, 1, 2]).reshape(2, n)
    return Row("mlx_area_anomaly", {"v": _dev(v), "mean": _dev(mean), "slot": _dev(slot)},
               lambda ops, **res: core.area_anomaly(ops["v"], ops["mean"], ops["slot"], **res),
               {"out": ((2, n), torch.float64)},
               lambda got: _same_bits(got["out"], ref, f"anomaly n={n} {_name(dtype)}"))


# ---- the column kernels ---------------------------------------------------------------------------------
COLUMN_PLANES = (1, 1041, 1044)


@row("layer_integral", [(p,) for p in COLUMN_PLANES], (6,))
def _layer_integral(case):
    plane, = case
    rng = np.random.default_rng(1600 + plane)
    x = rng.normal(0.5, 3.0, (2, 7, plane))
    x[rng.random(x.shape) < 0.05] = NAN
    depth = rng.uniform(1.0, 330.0, plane)
    depth[rng.random(plane) < 0.25] = NAN
    depth[0] = 27.5
    surface = np.where(np.isnan(depth), NAN, 1.0)
    surface[plane - 1] = NAN
    tops, bottoms = [0.0, 27.0, 3.0], [27.0, np.inf, 16.0]
    ref = ln.layer_integral(x, Z_LAYER, depth, tops, bottoms, surface=surface, scale=2.5)
    ops = {"x": _dev(x), "z_i": _dev(Z_LAYER), "depth": _dev(depth), "surface": _dev(surface)}
    return Row("mlx_layer_integral", ops,
               lambda ops, **res: core.layer_integral(ops["x"], ops["z_i"], ops["depth"], tops, bottoms,
                                                      surface=ops["surface"], scale=2.5, **res),
               {"out": ((2, 3, plane), torch.float64)},
               lambda got: _equal_values(got["out"], ref, f"layers plane={plane}"))


@row("column_crossing", [(p,) for p in COLUMN_PLANES], (6,))
def _column_crossing(case):
    plane, = case
    rng = np.random.default_rng(1700 + plane)
    x = np.cumsum(rng.uniform(0.0, 1.0, (2, 7, plane)), axis=1)  # rises with depth
    x[1, 4:, plane // 2] = NAN  # a shallow column
    if plane > 2:
        x[:, :, 1] = NAN  # land
    floor = rng.uniform(100.0, 130.0, plane)
    targets = [1.0, 2.5]
    ref = col.column_crossing(x, Z_COLUMN, 0, col.RISE, False, col.MISS_FLOOR, targets, floor)
    ops = {"a": _dev(x), "z": _dev(Z_COLUMN), "floor": _dev(floor)}
    return Row("mlx_column_crossing", ops,
               lambda ops, **res: core.column_crossing(ops["a"], ops["z"], targets, kref=0, mode="rise",
                                                       miss="floor", floor=ops["floor"], **res),
               {"out": ((2, 2, plane), torch.float64)},
               lambda got: _equal_values(got["out"], ref, f"crossing plane={plane}"))


# ---- the generator and the probes ----------------------------------------------------------------------
@row("synth_field", [(n, dt) for dt in (F64, F32) for n in FLAT], (6, F64))
def _synth_field(case):
    n, dtype = case
    shape = (2, 3, 1, n)
    mask = np.ones((3, 1, n))
    mask[1, 0, n // 2] = NAN
    kw = dict(seed=synthetic.SEED, field_id=1, lo=-2.0, scale=34.0)
    ref = synthetic.field_numpy(shape, mask3d=mask, dtype=dtype, **kw)
    return Row("mlx_synth_field", {"mask3d": _dev(mask)},
               lambda ops, **res: core.synth_field(shape, TD[dtype], mask3d=ops["mask3d"], **kw, **res),
               {"out": (shape, TD[dtype])},
               lambda got: assert_bit_equal(got["out"], ref, f"synth n={n} {_name(dtype)}"))


def _streams(n, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 1.0, n).astype(dtype), rng.normal(0.0, 1.0, n).astype(dtype)


@row("stream_probe", [(n,) for n in FLAT], (6,))
def _stream_probe(case):
    n, = case
    a, b = _streams(n, F64, 1800 + n)
    return Row("mlx_stream_probe", {"a": _dev(a), "b": _dev(b)},
               lambda ops, **res: core.stream_probe(ops["a"], ops["b"], **res),
               {"out": ((n,), torch.float64)},
               lambda got: assert_bit_equal(got["out"], a + b, f"probe n={n}"),
               refused=lambda offset: n % 2 != 0 or offset != 0)  # whole aligned packs only


@row("stream_probe_mix", [(n, dt) for dt in (F64, F32) for n in FLAT], (8, F64))
def _stream_probe_mix(case):
    n, dtype = case
    a, b = _streams(n, dtype, 1900 + n)
    return Row("mlx_stream_probe_mix", {"a": _dev(a), "b": _dev(b)},
               lambda ops, **res: core.stream_probe_mix(ops["a"], ops["b"], **res),
               {"out": ((n,), torch.float64)},
               lambda got: assert_bit_equal(got["out"], a.astype(F64) + b.astype(F64), f"mix n={n}"),
               refused=lambda offset: n % (16 // np.dtype(dtype).itemsize) != 0 or offset != 0)


ROW_NAMES = list(ROWS)
TWO_RESULTS = [name for name in ROW_NAMES if name.startswith("steric_local")]


def test_the_table_covers_every_entry_point_that_takes_a_buffer():
    """every function of core.py with an ``out`` / ``*_out`` argument has a row (the path queries
    take ``out`` to ask about it and write nothing)"""
    import inspect

    takers = {name for name, f in inspect.getmembers(core, inspect.isfunction)
              if not name.startswith("_") and not name.endswith("_path")
              and any(p == "out" or p.endswith("_out") for p in inspect.signature(f).parameters)}
    covered = {name.replace("_remove", "").replace("_model_resid", "").replace("_drho32", "")
               for name in ROW_NAMES}
    assert takers == covered, takers ^ covered


def _refusal_row(name):
    builder, _, case = ROWS[name]
    return builder(case)


# ---- (1) refusals and overlap: nothing is launched --------------------------------------------------------
@pytest.fixture
def spy(monkeypatch):
    """core._call replaced: the entry names it was asked to launch, and nothing launched"""
    calls = []
    monkeypatch.setattr(core, "_call", lambda lib, name, device, *args: calls.append(name))
    return calls


def _refused(r, spy, results, ops=None, match=None):
    with pytest.raises(ValueError, match=match):
        r.call(r.ops if ops is None else ops, **results)
    assert spy == [], f"{spy} reached the launch with {list(results)} that must be refused"


def _other(dtype):
    return torch.float32 if dtype == torch.float64 else torch.float64


def _bad_results(shape, dtype):
    """(label, tensor) for every refusal that is a property of the result alone"""
    yield "the other float dtype", torch.empty(shape, dtype=_other(dtype), device=DEV)
    for axis in range(len(shape)):
        short = shape[:axis] + (shape[axis] - 1,) + shape[axis + 1:]
        yield f"one short along axis {axis}", torch.empty(short, dtype=dtype, device=DEV)
        long = shape[:axis] + (shape[axis] + 1,) + shape[axis + 1:]
        yield f"one long along axis {axis}", torch.empty(long, dtype=dtype, device=DEV)
    numel = int(np.prod(shape))
    other = shape[::-1] if shape[::-1] != shape else (1,) + shape
    assert int(np.prod(other)) == numel and other != shape
    yield "the same numel in another shape", torch.empty(other, dtype=dtype, device=DEV)
    yield "the same numel, flat and one axis more", torch.empty((numel, 1) if len(shape) == 1
                                                                 else (numel,), dtype=dtype, device=DEV)
    assert shape[-1] >= 2
    wide = torch.empty(shape[:-1] + (2 * shape[-1],), dtype=dtype, device=DEV)
    view = wide[..., ::2]
    assert tuple(view.shape) == shape and not view.is_contiguous()
    yield "every other element of a wider tensor", view
    if len(shape) >= 2 and min(shape[-2:]) >= 2:  # (a transposed (1, n) is contiguous)
        view =torch.empty(shape[:-2] + (shape[-1], shape[-2]), dtype=dtype, device=DEV).transpose(-1, -2)
        assert tuple(view.shape) == shape and not view.is_contiguous()
        yield "a transposed tensor", view
    yield "a host tensor", torch.empty(shape, dtype=dtype)


@pytest.mark.parametrize("name", ROW_NAMES)
def test_a_result_of_the_wrong_kind_is_refused_before_the_launch(name, spy):
    r = _refusal_row(name)
    count = 0
    for arg, (shape, dtype) in r.outs.items():
        for label, bad in _bad_results(tuple(shape), dtype):
            try:
                _refused(r, spy, {arg: bad})
            except BaseException as exc:
                raise AssertionError(f"{name}, {arg}: {label}: {exc!r}") from exc
            count += 1
    assert count >= 7 * len(r.outs)  # (a 1-D result: dtype, short, long, two shapes, strided, host)


@pytest.mark.parametrize("name", ROW_NAMES)
def test_a_result_that_is_an_operand_is_refused_before_the_launch(name, spy):
    r = _refusal_row(name)
    aliased = 0
    for arg, (shape, dtype) in r.outs.items():
        for opname, x in r.ops.items():
            fits = tuple(x.shape) == tuple(shape) and x.dtype == dtype
            # where shape and dtype allow, it is the overlap check that must refuse, by both names
            _refused(r, spy, {arg: x}, match=f"{arg} overlaps {opname}" if fits else None)
            aliased += fits
    print(f"{name}: {aliased} operand(s) fit a result's shape and dtype")


def _carve(x, outs, touch):
    """One buffer holding a copy of the operand ``x`` and, behind it, the results ``outs`` [(shape,
    dtype)]: the first result starts ON x's last element (``touch`` False) or right behind it
    (True), every further one right behind its predecessor (rounded up to its element size).
    -> (the copy of x, [results])."""
    xbytes = x.numel() * x.element_size()
    pad = (-xbytes) % 8  # x ends on an 8-byte boundary, where a result of either dtype may start
    sizes = [(int(np.prod(s)), torch.empty((), dtype=d).element_size()) for s, d in outs]
    buf = torch.zeros(pad + xbytes + sum(n * e + 8 for n, e in sizes), dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    copy = buf[pad:pad + xbytes].view(x.dtype).view(x.shape)
    copy.copy_(x)
    at = pad + xbytes - (0 if touch else sizes[0][1])
    results = []
    for (shape, dtype), (n, e) in zip(outs, sizes):
        at = -(-at // e) * e
        results.append(buf[at:at + n * e].view(dtype).view(tuple(shape)))
        at += n * e
    return copy, results


def _last_byte(t):
    return t.data_ptr() + t.numel() * t.element_size()


@pytest.mark.parametrize("name", ROW_NAMES)
def test_a_result_on_an_operands_last_element_is_refused_before_the_launch(name, spy):
    r = _refusal_row(name)
    for arg, spec in r.outs.items():
        for opname, x in r.ops.items():
            copy, (res,) = _carve(x, [spec], touch=False)
            assert res.is_contiguous() and tuple(res.shape) == tuple(spec[0]) and res.dtype == spec[1]
            assert _last_byte(copy) - res.element_size() == res.data_ptr()  # one element is shared
            _refused(r, spy, {arg: res}, ops={**r.ops, opname: copy}, match=f"{arg} overlaps {opname}")


@pytest.mark.parametrize("name", TWO_RESULTS)
def test_two_results_that_share_an_element_are_refused_before_the_launch(name, spy):
    r = _refusal_row(name)
    (drho, dspec), (eta, espec) = r.outs.items()
    for first, fspec, second, sspec in ((drho, dspec, eta, espec), (eta, espec, drho, dspec)):
        base = torch.empty(fspec[0], dtype=fspec[1], device=DEV)
        one, (two,) = _carve(base, [sspec], touch=False)
        assert one.data_ptr() < two.data_ptr() < _last_byte(one)
        _refused(r, spy, {first: one, second: two}, match="overlaps")


@pytest.mark.parametrize("name", ROW_NAMES)
def test_a_result_that_touches_an_operand_reaches_the_launch(name, spy):
    """the operand and, right behind its last byte, the result(s): accepted, and launched once per
    expected launch (by the spy: nothing runs)"""
    r = _refusal_row(name)
    specs = sorted(r.outs.items(), key=lambda kv: -torch.empty((), dtype=kv[1][1]).element_size())
    for opname, x in r.ops.items():
        copy, results = _carve(x, [spec for _, spec in specs], touch=True)
        assert results[0].data_ptr() == _last_byte(copy)
        given = {arg: res for (arg, _), res in zip(specs, results)}
        del spy[:]
        ret = r.call({**r.ops, opname: copy}, **given)
        assert spy == [r.entry] * r.launches, f"{name}, results behind {opname}: {spy}"
        for arg, t in r.unpack(ret).items():
            assert t is given[arg]
    del spy[:]


# ---- (2) guard bands: valid buffers, real launches -----------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_the_guard_sees_a_device_store_beside_the_view(dtype):
    """the helper on device memory (test_out_contract_host.py has it on the host): one element
    before the view, one in a stride gap and one behind it, stored by the device, are reported"""
    g = oc.Guarded((3, 2, 5), dtype, DEV, offset=1, strides=(30, 5, 1))
    g.view.fill_(1.5)
    assert g.changed() == [] and g.unwritten() == 0
    for k in (-1, 10, g.span):
        g.buf[g.start + k] = 1.5
    assert g.changed() == [-1, 10, g.span]


GUARD_CASES = [(name, case, offset) for name in ROW_NAMES for case in ROWS[name][1] for offset in (0, 1)]


@pytest.mark.parametrize("name, case, offset", GUARD_CASES,
                         ids=[f"{n}-{_ids(c)}-{'aligned' if off == 0 else 'one-in'}"
                              for n, c, off in GUARD_CASES])
def test_nothing_is_written_beside_the_result(name, case, offset):
    r = ROWS[name][0](case)
    guards = {arg: oc.Guarded(shape, dtype, DEV, offset=offset, strides=r.strides.get(arg))
              for arg, (shape, dtype) in r.outs.items()}
    views = {arg: g.view for arg, g in guards.items()}
    for arg, g in guards.items():
        assert g.view.data_ptr() % 16 == offset * g.view.element_size(), arg
        assert g.view.is_contiguous() == (arg not in r.strides)
    what = f"{name} {_ids(case)} offset={offset}"
    if r.refused(offset):  # the library's own refusal: nothing may have been written at all
        with pytest.raises(core.MomlevelHipError):
            r.call(r.ops, **views)
        torch.cuda.synchronize()
        for arg, g in guards.items():
            g.assert_intact(f"{what}, {arg}, refused by the library")
            assert g.unwritten() == g.view.numel()
        return
    if r.path is not None:
        r.path(r.ops, views, offset)
    ret = r.call(r.ops, **views)
    torch.cuda.synchronize()
    for arg, t in r.unpack(ret).items():
        assert t is views[arg], f"{what}: {arg} is not the buffer that was passed"
    for arg, g in guards.items():
        g.assert_intact(f"{what}, {arg}")
        assert g.unwritten() == 0, f"{what}, {arg}: {g.unwritten()} element(s) were never written"
    r.check({arg: v.cpu().numpy() for arg, v in views.items()})
