"""GPU: the stratification kernels (csrc/momlevel_strat.hip: k_stratification, k_adjust_n2,
k_speed_where_time0) on the paths that test_gpu_stratification.py reaches only at toy sizes, only
through the angle's tolerance, or not at all:

* a pressure that varies from cell to cell -- (nz, plane) and (nt, nz, plane) -- held to N^2's BITS,
  past one block of cells, on the two-cell kernel (1026 = 2 x 513 cells: three blocks, the last of
  one thread) and on its one-cell twin (513 cells: three blocks, the last of one cell), for
  float64 fields and both float32 modes;
* the linear EOS: N^2 and the Turner angle, float64 fields and float32 fields upcast;
* exact zeros in the Turner ratio (columns of constant theta, S or both);
* fields with two dimensions before z ((member, time, z, y, x): ``lead0_rows`` = 3 in the
  adjustment), on the device path and through the host pipeline;
* the adjustment's groups of 8 levels: forward fills that cross a group boundary and run through a
  whole group, level counts at and around the group size;
* the alignment fallback (an even plane off its 16-byte boundary takes the one-cell twin) past one
  block, for every operand the entry points test.

The reference is the numpy oracle throughout (oracle/momlevel_numpy.py), called as the reference
package calls numpy.  N^2, its adjustment and the wave speed are held to bit equality, the angle
to identical NaN placement and test_gpu_stratification.py's gate (1e-12 of a right angle: the
device's arctan against libm's); every case asserts that its reference holds NaN and finite values.
The draws are shared between the cases that use them and never written to.
"""

import functools

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal
from momlevel_amd import core, derived
from momlevel_amd.labeled import DataArray
from oracle import momlevel_numpy as o

pytestmark = pytest.mark.gpu

GATE = 90.0 * 1e-12  # test_gpu_stratification.py's
NT, NZ = 2, 5
PLANES = {1026: (2, 513), 513: (1, 513)}  # cells: (ny, nx)
DIMS4 = ("time", "z_l", "yh", "xh")
DIMS5 = ("member", "time", "z_l", "yh", "xh")
MODES = {"f64": (np.float64, "faithful"), "f32": (np.float32, "faithful"),
         "f32_upcast": (np.float32, "upcast")}


def _levels(nz, even=False):
    """test_gpu_stratification.py's "mom6_like" (uneven) and "uniform" levels"""
    return 5.0 + 10.0 * np.arange(nz) if even else np.cumsum(2.0 * 1.075 ** np.arange(nz)) - 1.0


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared draws are read-only)


def _host(t):
    return t.cpu().numpy()


def _offset(a):
    """the host array ``a`` on the device, one element into a flat buffer: contiguous, so nothing
    realigns it, and off its 16-byte boundary (test_gpu_pack_widths._placements)"""
    flat = _cuda(np.ascontiguousarray(a).reshape(-1))
    n = flat.numel()
    buf = torch.zeros(n + 4, dtype=flat.dtype, device=flat.device)
    buf[1:1 + n] = flat
    view = buf[1:1 + n].view(a.shape)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + flat.element_size()
    assert view.data_ptr() % 16 != 0 and view.data_ptr() % flat.element_size() == 0
    return view


def _draw(shape, dtype, seed):
    """theta / S of shape (..., nz, ny, nx) as test_gpu_stratification._fields draws them: a fifth
    of the columns land (NaN at every level), three tenths of the rest NaN below a bottom of their
    own (level 3 at the shallowest, so that the levels above keep a finite derivative).  Pinned:
    cell 0 and the cells about the seam of the two-cell kernel's blocks (511 | 512) are wet at
    every level; the last pack holds a land column (plane-2) and one that lacks its last level
    (plane-1) -- which at 513 cells ARE 511 and 512."""
    r = np.random.default_rng(seed)
    nz, cells = shape[-3], shape[-2:]
    plane = cells[0] * cells[1]
    T = r.uniform(-2.0, 30.0, shape).astype(dtype)
    S = r.uniform(30.0, 40.0, shape).astype(dtype)
    bottom = np.where(r.random(plane) < 0.3, r.integers(3, nz + 1, plane), nz)
    bottom[r.random(plane) < 0.2] = 0
    bottom[[c for c in (0, 511, 512) if c < plane - 2]] = nz
    bottom[plane - 2], bottom[plane - 1] = 0, nz - 1
    dry = (np.arange(nz)[:, None] >= bottom[None, :]).reshape((nz,) + cells)
    T[..., dry], S[..., dry] = np.nan, np.nan
    return T, S


@functools.lru_cache(maxsize=None)
def _fields(plane, dtype):
    """the (NT, NZ, ny, nx) draw of a plane, shared by the cases and read-only"""
    T, S = _draw((NT, NZ) + PLANES[plane], dtype, seed=plane + (dtype == np.float32))
    T.setflags(write=False)
    S.setflags(write=False)
    return T, S


def _rows(a, nt=None):
    """a (..., nz, ny, nx) host array on the device as the kernels see it: (nt, nz, plane)"""
    nz, plane = a.shape[-3], a.shape[-2] * a.shape[-1]
    return _cuda(a).reshape(-1 if nt is None else nt, nz, plane)


def _alpha_beta(T, S, p, eos):
    if eos == "linear":
        return o.linear_alpha(T, S, p), o.linear_beta(T, S, p)
    return o.wright_alpha(T, S, p), o.wright_beta(T, S, p)


def _n2_ref(T, S, p, z, eos="wright", gravity=-9.8):
    """derived.py:401 of the reference at an arbitrary pressure, from the oracle's parts: alpha and
    beta at (T, S, p), numpy.gradient along z.  float32 fields against a float64 pressure ARRAY:
    float64 alpha / beta, float32 derivatives -- the kernel's ``faithful`` mode."""
    alpha, beta = _alpha_beta(T, S, p, eos)
    dTdz = o.differentiate_z(T, z, -3)
    dSdz = o.differentiate_z(S, z, -3)
    assert dTdz.dtype == T.dtype and dSdz.dtype == S.dtype
    if eos == "wright":
        assert alpha.dtype == np.float64 and beta.dtype == np.float64
    return gravity * ((alpha * dTdz) - (beta * dSdz))


def _mixed(ref, what):
    assert np.isnan(ref).any() and np.isfinite(ref).any(), f"{what}: the reference is one-sided"


def _check_bits(got, ref, what):
    _mixed(ref, what)
    assert got.dtype == np.float64 and ref.dtype == np.float64
    assert_bit_equal(got, ref, what)


def _check_angle(got, ref, what):
    """identical NaN placement, every finite value within the gate; prints the measured maximum"""
    _mixed(ref, what)
    assert got.shape == ref.shape and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN placement differs"
    worst = np.nanmax(np.abs(got - ref))
    print(f"{what}: max |angle - numpy| = {worst:.3e} degrees (gate {GATE:.1e})")
    assert worst <= GATE, f"{what}: {worst:.3e} > {GATE:.1e}"


# ---------------------------------------------------------------------------------------------
# 1. per-cell pressure
# ---------------------------------------------------------------------------------------------
P_SHAPES = {"scalar": lambda nt, nz, plane: (), "z": lambda nt, nz, plane: (nz,),
            "z_cell": lambda nt, nz, plane: (nz, plane), "t_z_cell": lambda nt, nz, plane: (nt, nz, plane)}


def _pressure(kind, nt, nz, plane, seed):
    """drawn independently per element: a value read from the wrong cell, level or step is another
    value"""
    return np.asarray(np.random.default_rng(seed).uniform(1e5, 5e7, P_SHAPES[kind](nt, nz, plane)))


def _pressure_full(p, shape):
    """``p`` as the (nt, nz, ny, nx) array the kernel's strides stand for (a view: every time step
    of a (nz, plane) pressure IS the same memory)"""
    nt, nz, ny, nx = shape
    if p.ndim == 1:
        p = p[:, None, None]
    elif p.ndim == 2:
        p = p.reshape(nz, ny, nx)
    elif p.ndim == 3:
        p = p.reshape(shape)
    return np.broadcast_to(p, shape)


@pytest.mark.parametrize("kind", sorted(P_SHAPES))
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("plane", sorted(PLANES))
def test_pressure_by_cell_level_and_step(plane, mode, kind):
    """core.stratification with each pressure layout it takes, N^2 to the bit and the Turner angle
    to the gate.  A (nz, plane) pressure serves both time steps (the reference is evaluated with
    the broadcast array: time stride 0), a (nt, nz, plane) one each its own; the block, the cell of
    the pack (``v``), the level and the step all enter the address."""
    dtype, f32_mode = MODES[mode]
    T, S = _fields(plane, dtype)
    z = _levels(NZ)
    p = _pressure(kind, NT, NZ, plane, seed=7 * plane + len(kind))
    pf = _pressure_full(p, T.shape)
    if kind != "scalar":
        assert len(np.unique(p)) == p.size
    Tr, Sr = (T.astype(np.float64), S.astype(np.float64)) if f32_mode == "upcast" else (T, S)
    Td, Sd, pd = _rows(T), _rows(S), _cuda(p)
    what = f"plane {plane} {mode} p{p.shape}"
    got = core.stratification(Td, Sd, pd, z, func="n2", f32_mode=f32_mode)
    assert tuple(got.shape) == (NT, NZ, plane)
    _check_bits(_host(got).reshape(T.shape), _n2_ref(Tr, Sr, pf, z), f"N^2, {what}")
    got = core.stratification(Td, Sd, pd, z, func="turner", f32_mode=f32_mode)
    _check_angle(_host(got).reshape(T.shape), o.calc_stability_angle(Tr, Sr, pf, z), f"Turner, {what}")


# ---------------------------------------------------------------------------------------------
# 2. the linear EOS
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f64", "f32_upcast"])
@pytest.mark.parametrize("plane", sorted(PLANES))
def test_linear_eos(plane, mode):
    """N^2 and the Turner angle of the linear EOS (no pressure operand): float64 fields, and
    float32 fields upcast -- the combination the C ABI allows beside the refused float32-throughout
    one (test_gpu_stratification.test_errors).  The reference: the float64 conversions."""
    dtype, f32_mode = MODES[mode]
    T, S = _fields(plane, dtype)
    z = _levels(NZ)
    Tr, Sr = T.astype(np.float64), S.astype(np.float64)
    Td, Sd = _rows(T), _rows(S)
    what = f"linear EOS, plane {plane} {mode}"
    n2 = core.stratification(Td, Sd, None, z, func="n2", eos="linear", f32_mode=f32_mode)
    _check_bits(_host(n2).reshape(T.shape), _n2_ref(Tr, Sr, None, z, eos="linear"), f"N^2, {what}")
    if mode == "f64":
        assert_bit_equal(_host(n2).reshape(T.shape), o.calc_n2(T, S, z, eos="linear"))
    tu = core.stratification(Td, Sd, None, z, func="turner", eos="linear", f32_mode=f32_mode)
    _check_angle(_host(tu).reshape(T.shape), o.calc_stability_angle(Tr, Sr, 0.0, z, eos="linear"),
                 f"Turner, {what}")


def test_linear_stability_angle_by_name():
    T, S = _fields(1026, np.float64)
    z = _levels(NZ)
    coords = {"z_l": DataArray(z, ("z_l",))}
    pres = z * 1.0e4 + 101325.0
    tu = derived.calc_stability_angle(DataArray(T, DIMS4, coords), DataArray(S, DIMS4, coords),
                                      DataArray(pres, ("z_l",)), eos="linear")
    _check_angle(tu.values, o.calc_stability_angle(T, S, pres, z, eos="linear"),
                 "calc_stability_angle(eos='linear'), plane 1026")


# ---------------------------------------------------------------------------------------------
# 3. exact zeros in the Turner ratio
# ---------------------------------------------------------------------------------------------
def _constant_columns(plane, dtype):
    """the plane's draw with wet columns of constant theta, constant S and both: the first cell,
    the seams of the blocks (255 | 256 for the one-cell kernel, 511 | 512 for the two-cell one) and
    the last cell (which at 513 cells IS cell 512).  A different constant per step."""
    T, S = (a.copy() for a in _fields(plane, dtype))
    r = np.random.default_rng(plane + 3)
    cells = {0: "T", 255: "S", 256: "TS", 511: "S", 512: "TS"}
    cells.setdefault(plane - 1, "T")
    for cell, which in cells.items():
        j, i = divmod(cell, T.shape[-1])
        T[:, :, j, i] = r.uniform(-2.0, 30.0, T.shape[:2]).astype(dtype)
        S[:, :, j, i] = r.uniform(30.0, 40.0, S.shape[:2]).astype(dtype)
        for t in range(T.shape[0]):
            if "T" in which:
                T[t, :, j, i] = dtype(12.5 + t)
            if "S" in which:
                S[t, :, j, i] = dtype(34.25 + t)
    return T, S, cells


@pytest.mark.parametrize("even", [True, False], ids=["even_levels", "uneven_levels"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("plane", sorted(PLANES))
def test_constant_columns_in_the_turner_ratio(plane, dtype, even):
    """dT/dz or dS/dz exactly zero (evenly spaced levels) or rounding noise about zero (uneven
    ones): R is then +-inf, 0/0, 0 or huge.  Whatever numpy makes of each -- NaN, +-45 degrees --
    the kernel makes the same of it: nothing here assumes which."""
    T, S, cells = _constant_columns(plane, dtype)
    z = _levels(NZ, even)
    pres = z * 1.0e4 + 101325.0
    ref = o.calc_stability_angle(T, S, pres, z)  # (under errstate(divide, invalid = "ignore"))
    flat = ref.reshape(NT, NZ, plane)
    for cell, which in cells.items():
        print(f"constant {which} at cell {cell}: numpy gives {flat[:, :, cell].ravel()}")
    what = f"constant columns, plane {plane} {np.dtype(dtype).name} {'even' if even else 'uneven'} levels"
    got = core.stratification(_rows(T), _rows(S), _cuda(pres), z, func="turner")
    _check_angle(_host(got).reshape(T.shape), ref, what)
    got = core.stratification(_rows(T), _rows(S), _cuda(pres), z, func="n2")
    _check_bits(_host(got).reshape(T.shape), o.calc_n2(T, S, z), f"N^2, {what}")


# ---------------------------------------------------------------------------------------------
# 4. two dimensions before z
# ---------------------------------------------------------------------------------------------
def _fields5(dtype, cells=(1, 6), seed=56):
    shape = (2, 3, NZ) + cells
    T, S = _draw(shape, dtype, seed)
    z = _levels(NZ)
    coords = {"z_l": DataArray(z, ("z_l",))}
    return T, S, z, DataArray(T, DIMS5, coords), DataArray(S, DIMS5, coords)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_member_time_fields_n2(dtype):
    T, S, z, Td, Sd = _fields5(dtype)
    n2 = derived.calc_n2(Td, Sd)
    assert n2.dims == DIMS5
    _check_bits(n2.values, o.calc_n2(T, S, z), f"calc_n2 of (member, time, z, y, x) {np.dtype(dtype).name}")


def test_member_time_fields_stability_angle():
    """a pressure that varies with (time, z) only -- every member reads the same values -- and one
    of the field's full dims"""
    T, S, z, Td, Sd = _fields5(np.float64)
    r = np.random.default_rng(57)
    p = r.uniform(1e5, 5e7, (3, NZ))
    tu = derived.calc_stability_angle(Td, Sd, DataArray(p, ("time", "z_l")))
    assert tu.dims == DIMS5
    ref = o.calc_stability_angle(T, S, np.broadcast_to(p[None, :, :, None, None], T.shape), z)
    _check_angle(tu.values, ref, "5-D field, pressure (time, z_l)")
    p = r.uniform(1e5, 5e7, T.shape)
    tu = derived.calc_stability_angle(Td, Sd, DataArray(p, DIMS5))
    _check_angle(tu.values, o.calc_stability_angle(T, S, p, z), "5-D field, pressure of the field's dims")


def test_time_z_pressure_on_a_plane_of_three_blocks():
    T, S = _fields(1026, np.float64)
    z = _levels(NZ)
    coords = {"z_l": DataArray(z, ("z_l",))}
    p = np.random.default_rng(58).uniform(1e5, 5e7, (NT, NZ))
    tu = derived.calc_stability_angle(DataArray(T, DIMS4, coords), DataArray(S, DIMS4, coords),
                                      DataArray(p, ("time", "z_l")))
    ref = o.calc_stability_angle(T, S, np.broadcast_to(p[:, :, None, None], T.shape), z)
    _check_angle(tu.values, ref, "4-D field of 1026 cells, pressure (time, z_l)")


def test_member_time_fields_adjustment():
    """adjust_negative_n2 of a drawn (member, time, z, y, x) field: the reference's ``adjusted[0]``
    is member 0 -- three of the six rows (``lead0_rows`` = 3) -- so a column that starts
    non-positive reads 1e-8 in every row of member 0 and NaN in every row of member 1.  18 levels:
    three load groups."""
    nz, cells = 18, 6
    r = np.random.default_rng(59)
    n2 = r.normal(1.0e-5, 2.0e-5, (2, 3, nz, 1, cells))
    n2[..., 0] = np.nan                       # land
    n2[:, :, 9:, :, 5] = np.nan               # sub-bottom
    n2[..., 1] = -np.abs(n2[..., 1])          # non-positive at every level of every row
    n2[:, :, ::3, :, 1] = 0.0
    n2[:, :, :9, :, 2] = -np.abs(n2[:, :, :9, :, 2])  # non-positive down to level 8, positive at 9
    n2[:, :, 9, :, 2] = np.abs(n2[:, :, 9, :, 2])
    assert (n2[..., 1] <= 0.0).all() and (n2[:, :, 9, :, 2] > 0.0).all()
    ref = o.adjust_negative_n2(n2)
    # not vacuous: the reference tells the rows of member 0 from the others
    assert (ref[0, :, :, 0, 1] == 1.0e-8).all() and np.isnan(ref[1, :, :, 0, 1]).all()
    assert (ref[0, :, :9, 0, 2] == 1.0e-8).all() and np.isnan(ref[1, :, :9, 0, 2]).all()
    assert_bit_equal(ref[:, :, 9, 0, 2], n2[:, :, 9, 0, 2])
    field = DataArray(n2, DIMS5)
    got = derived.adjust_negative_n2(field)
    assert got.dims == DIMS5
    _check_bits(got.values, ref, "adjust_negative_n2 of (member, time, z, y, x)")
    dz = DataArray(np.abs(r.normal(10.0, 3.0, (nz, 1, cells))), DIMS5[2:])
    with pytest.raises(NotImplementedError):
        derived.calc_wave_speed(field, dz)


# ---------------------------------------------------------------------------------------------
# 5. the adjustment's groups of 8 levels
# ---------------------------------------------------------------------------------------------
GROUP = 8  # MLX_TUNE_ADJUST_DEPTH of csrc/momlevel_strat.hip (not exported)
FILL, LATE, BOTTOM = "fill", "late", "bottom"


def _column(kind, nt, nz):
    """(nt, nz) deterministic columns, cut to nz levels.  FILL: positive down to level 7,
    non-positive (negative or zero) at 8..16 -- the forward fill crosses one group boundary, then
    runs through a whole group -- positive at 17.  LATE: non-positive at 0..7, positive at 8 and 17,
    non-positive between.  BOTTOM: finite at the last level only."""
    k = np.arange(18, dtype=np.float64)[None, :]
    t = np.arange(nt, dtype=np.float64)[:, None]
    nonpos = np.where(k % 2 == 0, 0.0, -1.0e-6 * (1.0 + k + t))
    if kind == FILL:
        col = np.where((k <= 7) | (k == 17), 1.0e-5 * (1.0 + k + 2.0 * t), nonpos)
    elif kind == LATE:
        col = np.where((k == 8) | (k == 17), 2.0e-5 * (1.0 + k + 3.0 * t), nonpos)
    else:
        col = np.full((nt, 18), np.nan)
        col[:, nz - 1] = 4.0e-5 * (1.0 + t[:, 0])
    return col[:, :nz]


@functools.lru_cache(maxsize=None)
def _adjust_case(nt, nz, plane):
    """(n2 (nt, nz, plane), dz (nz, plane), {cell: column kind}): a drawn field -- a third of its
    values non-positive, land columns, sub-bottom NaN, a NaN surface above valid levels -- with the
    deterministic columns at the first pack (FILL, LATE: the two cells of one thread), about the
    seams of the blocks (BOTTOM | FILL at 255 | 256, the one-cell kernel's, and at 511 | 512, the
    two-cell one's) and at the last pack (LATE, BOTTOM)."""
    r = np.random.default_rng(100 * nz + nt + plane)
    n2 = r.normal(1.0e-5, 2.0e-5, (nt, nz, plane))
    n2[:, :, r.random(plane) < 0.2] = np.nan
    n2[:, (nz + 1) // 2:, r.random(plane) < 0.3] = np.nan
    n2[:, 0, r.random(plane) < 0.1] = np.nan
    cells = {0: FILL, 1: LATE, 255: BOTTOM, 256: FILL, 511: BOTTOM, 512: FILL}
    cells[plane - 2], cells[plane - 1] = LATE, BOTTOM  # (at 513 cells these ARE 511 and 512)
    for cell, kind in cells.items():
        n2[:, :, cell] = _column(kind, nt, nz)
    dz = np.abs(r.normal(10.0, 3.0, (nz, plane)))
    dz[np.isnan(n2[0])] = np.nan
    dz[:, list(cells)] = np.abs(r.normal(10.0, 3.0, (nz, len(cells))))
    n2.setflags(write=False)
    dz.setflags(write=False)
    return n2, dz, cells


def _adjust_refs(n2, dz, lead0_rows, cells):
    """(adjusted (nt, nz, plane), speed (nt, plane), quirk or None) of the oracle: ``n2`` as the
    (z, y, x) field it stands for when z leads, as the (time, z, y, x) one otherwise"""
    nt, nz, plane = n2.shape
    dz3 = dz.reshape((nz,) + cells)
    if lead0_rows == 0:
        field = n2.reshape((nz,) + cells)
        return (o.adjust_negative_n2(field).reshape(n2.shape),
                o.calc_wave_speed(field, dz3).reshape(1, plane), None)
    field = n2.reshape((nt, nz) + cells)
    adjusted = o.adjust_negative_n2(field)
    with np.errstate(invalid="ignore"):  # the (time, y, x) intermediate of calc_wave_speed_4d_quirk
        speed = o.nansum(np.sqrt(adjusted) * dz3, axis=-3) / np.pi
    quirk = o.calc_wave_speed_4d_quirk(field, dz3)
    return adjusted.reshape(n2.shape), speed.reshape(nt, plane), quirk.reshape(nz, plane, nt)


@pytest.mark.parametrize("rows", [(1, 0), (3, 1)], ids=["z_leads", "time_leads"])
@pytest.mark.parametrize("plane", sorted(PLANES))
@pytest.mark.parametrize("nz", [1, 2, 7, 8, 9, 16, 17, 18])
def test_adjustment_across_level_groups(nz, plane, rows):
    """core.adjust_negative_n2 with dz (adjusted and speed) and without it, on level counts below,
    at and past one and two groups of 8; ``carried`` and ``sum`` must survive from group to group.
    The filled value is looked for in a row past ``lead0_rows``: in a lead-0 row the non-positive
    levels read 1e-8, whatever was carried."""
    nt, lead0_rows = rows
    n2, dz, cells = _adjust_case(nt, nz, plane)
    ref, speed_ref, quirk = _adjust_refs(n2, dz, lead0_rows, PLANES[plane])
    last = nt - 1
    if nz > GROUP:  # the reference shows the fill across the group boundary and the late start
        filled = ref[last, GROUP:min(nz, 17), 0]
        assert (filled == n2[last, GROUP - 1, 0]).all() and n2[last, GROUP - 1, 0] > 0.0
        assert (ref[0, :GROUP, 1] == 1.0e-8).all() and ref[0, GROUP, 1] == n2[0, GROUP, 1]
        if lead0_rows:
            assert (ref[0, GROUP:min(nz, 17), 0] == 1.0e-8).all()
            assert np.isnan(ref[last, :GROUP, 1]).all() and ref[last, GROUP, 1] == n2[last, GROUP, 1]
    assert np.isnan(ref[:, :nz - 1, plane - 1]).all() and (ref[:, nz - 1, plane - 1] > 0.0).all()
    what = f"nz {nz} plane {plane} nt {nt} lead0_rows {lead0_rows}"
    x, dzd = _cuda(n2), _cuda(dz)
    adjusted, speed = core.adjust_negative_n2(x, lead0_rows, dz=dzd)
    _check_bits(_host(adjusted), ref, f"adjusted (with dz), {what}")
    assert tuple(speed.shape) == (nt, plane) and np.isfinite(speed_ref).any()
    assert_bit_equal(_host(speed), speed_ref, f"speed, {what}")
    alone, none = core.adjust_negative_n2(x, lead0_rows)
    assert none is None
    _check_bits(_host(alone), ref, f"adjusted (no dz), {what}")
    only, speed2 = core.adjust_negative_n2(x, lead0_rows, dz=dzd, want_adjusted=False)
    assert only is None
    assert_bit_equal(_host(speed2), speed_ref, f"speed alone, {what}")
    if lead0_rows:
        out = core.wave_speed_where_time0(x[0], speed)
        _check_bits(_host(out), quirk, f"wave_speed_where_time0, {what}")


# ---------------------------------------------------------------------------------------------
# 6. the alignment fallback past one block
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_stratification_off_the_16_byte_boundary(dtype):
    """1026 cells with theta, S or both one element off their boundary: the one-cell twin (five
    blocks) over the values the two-cell kernel (three) had -- the same bits, N^2 and angle"""
    plane = 1026
    T, S = _fields(plane, dtype)
    z = _levels(NZ)
    p = _pressure("t_z_cell", NT, NZ, plane, seed=61)
    pd = _cuda(p)
    shape3 = (NT, NZ, plane)
    aligned = {f: _host(core.stratification(_rows(T), _rows(S), pd, z, func=f)) for f in ("n2", "turner")}
    _check_bits(aligned["n2"].reshape(T.shape), _n2_ref(T, S, p.reshape(T.shape), z), "N^2, aligned")
    _check_angle(aligned["turner"].reshape(T.shape), o.calc_stability_angle(T, S, p.reshape(T.shape), z),
                 f"Turner, aligned, {np.dtype(dtype).name}")
    for which in ("T", "S", "TS"):
        Td = _offset(T.reshape(shape3)) if "T" in which else _rows(T)
        Sd = _offset(S.reshape(shape3)) if "S" in which else _rows(S)
        for f in ("n2", "turner"):
            got = _host(core.stratification(Td, Sd, pd, z, func=f))
            assert_bit_equal(got, aligned[f], f"{f}, {which} offset against aligned")


@pytest.mark.parametrize("which", ["n2", "dz"])
def test_adjustment_off_the_16_byte_boundary(which):
    nt, nz, plane, lead0_rows = 3, 9, 1026, 1
    n2, dz, cells = _adjust_case(nt, nz, plane)
    ref, speed_ref, _ = _adjust_refs(n2, dz, lead0_rows, PLANES[plane])
    adjusted, speed = core.adjust_negative_n2(_cuda(n2), lead0_rows, dz=_cuda(dz))
    adjusted, speed = _host(adjusted), _host(speed)
    _check_bits(adjusted, ref, "adjusted, aligned")
    assert_bit_equal(speed, speed_ref, "speed, aligned")
    x = _offset(n2) if which == "n2" else _cuda(n2)
    w = _offset(dz) if which == "dz" else _cuda(dz)
    got, got_speed = core.adjust_negative_n2(x, lead0_rows, dz=w)
    assert_bit_equal(_host(got), adjusted, f"adjusted, {which} offset against aligned")
    assert_bit_equal(_host(got_speed), speed, f"speed, {which} offset against aligned")
    if which == "n2":  # without dz the field's alignment alone decides
        got, _ = core.adjust_negative_n2(x, lead0_rows)
        assert_bit_equal(_host(got), adjusted, "adjusted (no dz), n2 offset against aligned")


# ---------------------------------------------------------------------------------------------
# 7. the host pipeline for fields with two dimensions before z
# ---------------------------------------------------------------------------------------------
def test_host_pipeline_of_member_time_fields(monkeypatch):
    """Host (member, time, z, y, x) fields above the pipeline limit are walked as (nt, nz, plane)
    rows, two to a group; a pressure of the field's dims is sliced with its rows.  Same bits as
    the call that is not pipelined, and the reference's."""
    from momlevel_amd import hostio

    cells = (2, 513)
    shape = (2, 3, NZ) + cells
    z = _levels(NZ)
    coords = {"z_l": DataArray(z, ("z_l",))}
    fields = {dtype: _draw(shape, dtype, 71) for dtype in (np.float64, np.float32)}
    p = np.random.default_rng(72).uniform(1e5, 5e7, shape)

    def run():
        out = {}
        for dtype, (T, S) in fields.items():
            out[dtype] = derived.calc_n2(DataArray(T, DIMS5, coords), DataArray(S, DIMS5, coords)).values
        T, S = fields[np.float64]
        out["tu"] = derived.calc_stability_angle(DataArray(T, DIMS5, coords), DataArray(S, DIMS5, coords),
                                                 DataArray(p, DIMS5)).values
        return out

    used = []
    real = hostio._enqueue_download
    monkeypatch.setattr(hostio, "_enqueue_download",
                        lambda out, dev, *a: used.append(out.shape) or real(out, dev, *a))
    plane = cells[0] * cells[1]
    whole = run()
    assert (2, NZ, plane) not in used  # nothing went group by group
    monkeypatch.setattr(hostio, "PIPELINE_ELEMS", 1000)
    monkeypatch.setattr(hostio, "PIECE_ELEMS", 2 * NZ * plane)  # two rows a group
    used.clear()
    piped = run()
    assert used == [(2, NZ, plane)] * 9  # three calls, six rows each, in groups of two
    for dtype, (T, S) in fields.items():
        name = np.dtype(dtype).name
        _check_bits(piped[dtype], o.calc_n2(T, S, z), f"pipelined calc_n2, 5-D {name}")
        assert_bit_equal(piped[dtype], whole[dtype], f"pipelined calc_n2 against the whole call, {name}")
    T, S = fields[np.float64]
    _check_angle(piped["tu"], o.calc_stability_angle(T, S, p, z), "pipelined angle, 5-D, full-dims pressure")
    _check_angle(whole["tu"], o.calc_stability_angle(T, S, p, z), "whole angle, 5-D, full-dims pressure")
    assert_bit_equal(piped["tu"], whole["tu"], "pipelined angle against the whole call")
