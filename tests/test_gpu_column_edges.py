"""GPU: the edges of core.column_crossing and the public functions on top of it
(derived.calc_mld / calc_isosurface_depth / calc_isopycnal_depth): waves whose lanes finish far
apart, records past the grid's rows, independence of records, targets and alignment, the fused
sigma against core.eos_map, labels, host / masked / lazy inputs, refusals.  BIT FOR BIT against
tests/column_numpy.py throughout."""

import numpy as np
import pytest
import torch

import column_numpy as cn
from momlevel_amd import _lib, core, derived, hostio
from momlevel_amd.labeled import DataArray
from test_gpu_column import (F32, F64, P_REF, SOURCES, Z7, columns, dev, equals_restatement, planes,
                             run_kernel, same_bits, targets_of)

pytestmark = pytest.mark.gpu


# ---- 1. one lane against 63 ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("late", [True, False], ids=["one_late", "one_early"])
def test_a_searching_lane_is_never_cut_off_by_finished_neighbours(dtype, late):
    """every column of a block crosses between levels 0 and 1 but a few, which cross between the
    last two (and the reverse): on the pack path and cell by cell"""
    block = core.column_block_cells(dtype)
    vec = block // 256
    nz = 7
    for plane in (block, block + 1):  # whole packs; the generic twin
        x = np.empty((2, nz, plane))
        x[:] = (np.arange(nz) * 0.01).reshape(1, nz, 1)  # 0, 0.01, ...: never reaches 1
        odd = np.zeros(plane, bool)
        odd[[37 * vec, 64 * vec + 1, plane - 1]] = True  # one cell of one lane of waves 0, 1 and the last
        early, last = (~odd, odd) if late else (odd, ~odd)
        x[:, 1:, early] += 5.0  # crosses 1.0 between levels 0 and 1
        x[:, nz - 1, last] += 5.0  # ... between the last two levels
        x = x.astype(dtype)
        ref = cn.column_crossing(x, Z7, 0, cn.RISE, False, cn.MISS_NAN, [1.0, 2.5])
        assert np.all(ref[:, :, early] < Z7[1]) and np.all(ref[:, :, last] > Z7[nz - 2])
        got = run_kernel(x, None, Z7, [1.0, 2.5], 0, cn.RISE, False, cn.MISS_NAN, None)
        equals_restatement(got, ref, f"plane={plane}")


def test_records_past_the_rows_of_the_grid():
    cap = core.column_record_rows(1 << 30)
    nrec = cap + 3
    assert core.column_record_rows(nrec) == cap < nrec
    rng = np.random.default_rng(3)
    x = np.stack([rng.uniform(0.0, 1.0, nrec), rng.uniform(0.5, 2.0, nrec)], axis=1).reshape(nrec, 2, 1)
    x[::17, 1, 0] = np.nan
    z = Z7[:2]
    ref = cn.column_crossing(x, z, 0, cn.RISE, False, cn.MISS_FLOOR, [1.0])
    got = run_kernel(x, None, z, [1.0], 0, cn.RISE, False, cn.MISS_FLOOR, None)
    equals_restatement(got, ref, "strided records")
    assert np.isfinite(ref[cap:]).any() and (ref == z[0]).any() and ((ref > z[0]) & (ref < z[1])).any()


# ---- 2. independence ---------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["field32", "sigma64", "sigma_t32_s64"])
def test_a_result_depends_on_its_own_column_and_target_only(source):
    adt, bdt = SOURCES[source]
    plane = planes(adt, bdt)[2] + 8  # whole packs
    nrec, nz, kref = 5, 7, 1
    a, b, x = columns(source, nrec, nz, plane, 42)
    if x is None:
        x = cn.sigma(a, b, P_REF)
    ad, bd, zd = dev(a), None if b is None else dev(b), dev(Z7)
    tg9 = targets_of(source, cn.RISE, True, 9, False)
    kw = dict(kref=kref, mode="rise", relative=True, miss="floor", p_ref=P_REF)
    full = core.column_crossing(ad, zd, tg9[:8], b=bd, **kw)
    equals_restatement(full, cn.column_crossing(x, Z7, kref, cn.RISE, True, cn.MISS_FLOOR, tg9[:8]), source)
    assert same_bits(full, core.column_crossing(ad, zd, tg9[:8], b=bd, **kw))  # run to run
    for r in (0, 2, nrec - 1):  # a record alone and among others
        alone = core.column_crossing(ad[r:r + 1], zd, tg9[:8], b=None if bd is None else bd[r:r + 1], **kw)
        assert same_bits(alone[0], full[r]), f"record {r}"
    for j in range(8):  # a target alone and among eight
        alone = core.column_crossing(ad, zd, tg9[j:j + 1], b=bd, **kw)
        assert same_bits(alone[:, 0], full[:, j]), f"target {j}"
    three = core.column_crossing(ad, zd, tg9[[1, 4, 6]], b=bd, **kw)
    assert same_bits(three, full[:, [1, 4, 6]])
    nine = core.column_crossing(ad, zd, tg9, b=bd, **kw)  # two launches
    assert same_bits(nine[:, :8], full)
    assert same_bits(nine[:, 8], core.column_crossing(ad, zd, tg9[8:], b=bd, **kw)[:, 0])
    # a, b and out at an odd element offset of a larger buffer: the generic twin
    def shifted(t):
        buf = torch.zeros(t.numel() + 3, dtype=t.dtype, device="cuda")
        buf[1:1 + t.numel()] = t.reshape(-1)
        return buf[1:1 + t.numel()].reshape(t.shape)

    obuf = torch.full((full.numel() + 3,), 7.0, dtype=torch.float64, device="cuda")
    out = obuf[1:1 + full.numel()].reshape(full.shape)
    got = core.column_crossing(shifted(ad), zd, tg9[:8], b=None if bd is None else shifted(bd), out=out, **kw)
    assert got.data_ptr() == out.data_ptr() and got.data_ptr() % 16 != 0
    assert same_bits(got, full)
    assert obuf[0].item() == 7.0 and torch.all(obuf[1 + full.numel():] == 7.0).item()  # nothing beside it
    # ... and each operand on its own
    assert same_bits(core.column_crossing(shifted(ad), zd, tg9[:8], b=bd, **kw), full)
    if bd is not None:
        assert same_bits(core.column_crossing(ad, zd, tg9[:8], b=shifted(bd), **kw), full)


# ---- 3. the fused sigma is eos_map's sigma -----------------------------------------------------------
@pytest.mark.parametrize("eos", ["wright", "linear"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_sigma_source_is_field_source_on_eos_map(dtype, eos):
    source = "sigma64" if dtype is F64 else "sigma32"
    plane = planes(dtype, dtype)[3]
    nrec, nz = 3, 7
    a, b, _ = columns(source, nrec, nz, plane, 9)
    t64, s64 = dev(a.astype(F64)), dev(b.astype(F64))
    rho = core.eos_map(t64.reshape(nrec, nz, 1, plane), s64.reshape(nrec, nz, 1, plane), P_REF, eos=eos)
    assert rho.dtype == torch.float64
    rho = rho.reshape(nrec, nz, plane)
    equals_restatement(rho, cn.sigma(a, b, P_REF, eos), "eos_map against the restatement's sigma")
    for mode, relative, miss, tg in (("rise", True, "floor", [0.03, 0.125]),
                                     ("rise", False, "nan", [1023.0, 1025.0, 1026.5]),
                                     ("depart", True, "nan", [0.03])):
        kw = dict(kref=1, mode=mode, relative=relative, miss=miss)
        fused = core.column_crossing(dev(a), Z7, tg, b=dev(b), eos=eos, p_ref=P_REF, **kw)
        assert same_bits(fused, core.column_crossing(rho, Z7, tg, **kw)), (mode, relative)
        assert np.isfinite(fused.cpu().numpy()).any()


# ---- 4. the public functions ---------------------------------------------------------------------------
DIMS = ("time", "z_l", "yh", "xh")
ZL = DataArray(Z7, ("z_l",))


def _ocean(dtype=F64, nt=5, ny=3, nx=347, seed=21):
    theta, so, _ = columns("sigma64", nt, 7, ny * nx, seed)
    coords = {"z_l": ZL, "time": DataArray(np.arange(nt, dtype=float), ("time",))}
    return (theta.astype(dtype).reshape(nt, 7, ny, nx), so.astype(dtype).reshape(nt, 7, ny, nx), coords)


def test_calc_mld_labels_and_bits():
    T, S, coords = _ocean()
    nt, nz, ny, nx = T.shape
    x = cn.sigma(T, S, P_REF).reshape(nt, nz, -1)
    kref = cn.nearest_level(Z7, 10.0)
    assert kref == 1
    mld = derived.calc_mld(DataArray(dev(T), DIMS, coords), DataArray(dev(S), DIMS, coords))
    assert mld.is_device and mld.dims == ("time", "yh", "xh") and mld.shape == (nt, ny, nx)
    assert mld.attrs["units"] == "m" and "sigma_theta" in mld.attrs["standard_name"]
    assert "time" in mld.coords and "z_l" not in mld.coords
    ref = cn.column_crossing(x, Z7, kref, cn.RISE, True, cn.MISS_FLOOR, [0.03])
    equals_restatement(mld.values, ref[:, 0].reshape(mld.shape), "density criterion")
    # a list of thresholds, a reference depth between two levels (ties: the shallower), a deptho
    deptho = np.random.default_rng(1).uniform(5.0, 150.0, (ny, nx))
    two = derived.calc_mld(DataArray(dev(T), DIMS, coords), DataArray(dev(S), DIMS, coords),
                           threshold=[0.03, 0.125], ref_depth=15.0, deptho=DataArray(deptho, ("yh", "xh")))
    assert two.dims == ("time", "threshold", "yh", "xh") and two.coords["threshold"].values.tolist() == [0.03, 0.125]
    ref = cn.column_crossing(x, Z7, 1, cn.RISE, True, cn.MISS_FLOOR, [0.03, 0.125], floor=deptho.reshape(-1))
    equals_restatement(two.values, ref.reshape(two.shape), "two thresholds")
    # calc_mld(deptho=) equals deptho where nothing crosses
    none = derived.calc_mld(DataArray(dev(T), DIMS, coords), DataArray(dev(S), DIMS, coords),
                            threshold=50.0, deptho=deptho).values
    wet = ~np.isnan(x[:, 0]).reshape(nt, ny, nx)
    assert wet.any() and np.array_equal(none[wet], np.broadcast_to(deptho, none.shape)[wet])
    assert np.isnan(none[~wet]).all()
    # the temperature criterion: FIELD source, DEPART, 0.2 degC; float32; linear EOS for density
    t32 = DataArray(dev(T.astype(F32)), DIMS, coords)
    mt = derived.calc_mld(t32, criterion="temperature")
    assert mt.attrs["standard_name"].endswith("defined_by_temperature") and mt.dims == ("time", "yh", "xh")
    ref = cn.column_crossing(T.astype(F32).reshape(nt, nz, -1), Z7, 1, cn.DEPART, True, cn.MISS_FLOOR, [0.2])
    equals_restatement(mt.values, ref[:, 0].reshape(mt.shape), "temperature criterion")
    ml = derived.calc_mld(t32, DataArray(dev(S), DIMS, coords), eos="linear", level=2000.0, ref_depth=0.0)
    ref = cn.column_crossing(cn.sigma(T.astype(F32), S, 0.0, "linear").reshape(nt, nz, -1), Z7, 0, cn.RISE,
                             True, cn.MISS_FLOOR, [0.03])
    equals_restatement(ml.values, ref[:, 0].reshape(ml.shape), "linear, theta32 / S64")


def test_isopycnal_and_isosurface_depths_labels_and_bits():
    T, S, coords = _ocean(F32)
    nt, nz, ny, nx = T.shape
    theta = DataArray(dev(T), DIMS, coords, {"standard_name": "sea_water_potential_temperature", "units": "degC"})
    so = DataArray(dev(S), DIMS, coords)
    vals = [1023.0, 1025.0, 1026.5]
    iso = derived.calc_isopycnal_depth(theta, so, vals, level=2000.0)
    assert iso.is_device and iso.dims == ("time", "rhopot", "yh", "xh") and iso.shape == (nt, 3, ny, nx)
    assert iso.coords["rhopot"].values.tolist() == vals and iso.attrs["units"] == "m"
    assert iso.coords["rhopot"].attrs["units"] == "kg m-3" and "2000.0 m" in iso.attrs["long_name"]
    x = cn.sigma(T, S, 2000.0 * 1.0e4 + 101325).reshape(nt, nz, -1)
    ref = cn.column_crossing(x, Z7, 0, cn.RISE, False, cn.MISS_NAN, [v + 9.0 for v in vals])
    got = derived.calc_isopycnal_depth(theta, so, [v + 9.0 for v in vals], level=2000.0)
    equals_restatement(got.values, ref.reshape(got.shape), "sigma2")
    one = derived.calc_isopycnal_depth(theta, so, 1025.0)
    assert one.dims == ("time", "yh", "xh") and "rhopot" not in one.coords
    ref = cn.column_crossing(cn.sigma(T, S, P_REF).reshape(nt, nz, -1), Z7, 0, cn.RISE, False, cn.MISS_NAN, [1025.0])
    equals_restatement(one.values, ref[:, 0].reshape(one.shape), "sigma0 = 25")
    assert np.isfinite(ref).any() and np.isnan(ref).any()
    # the 20 degC isotherm: FALL, absolute
    xt = T.reshape(nt, nz, -1)
    d20 = derived.calc_isosurface_depth(theta, 20.0, direction="decreasing")
    assert d20.dims == ("time", "yh", "xh") and d20.attrs["units"] == "m"
    assert d20.attrs["standard_name"] == "depth_of_isosurface_of_sea_water_potential_temperature"
    ref = cn.column_crossing(xt, Z7, 0, cn.FALL, False, cn.MISS_NAN, [20.0, 12.0])
    equals_restatement(d20.values, ref[:, 0].reshape(d20.shape), "20 degC")
    assert np.isfinite(ref[:, 0]).any()
    auto = derived.calc_isosurface_depth(theta, [20.0, 12.0])  # "auto": temperature falls with depth
    assert auto.dims == ("time", "value", "yh", "xh") and auto.coords["value"].values.tolist() == [20.0, 12.0]
    assert auto.coords["value"].attrs["units"] == "degC"
    equals_restatement(auto.values, ref.reshape(auto.shape), "auto -> decreasing")
    up = derived.calc_isosurface_depth(DataArray(dev(x.reshape(nt, nz, ny, nx)), DIMS, coords), [1025.5],
                                       missing="floor", deptho=np.full((ny, nx), 77.0))
    ref = cn.column_crossing(x, Z7, 0, cn.RISE, False, cn.MISS_FLOOR, [1025.5], floor=np.full(ny * nx, 77.0))
    equals_restatement(up.values, ref.reshape(up.shape), "auto -> increasing, floor")
    with pytest.raises(ValueError, match="cannot tell"):
        derived.calc_isosurface_depth(DataArray(torch.ones((1, 7, 2, 2), device="cuda"), DIMS, {"z_l": ZL}), 1.0)


def test_z_first_and_a_5d_field():
    T, S, coords = _ocean(F64, nt=6)
    x = cn.sigma(T, S, P_REF).reshape(6, 7, -1)
    zc = {"z_l": ZL}
    first = derived.calc_mld(DataArray(dev(T[0]), DIMS[1:], zc), DataArray(dev(S[0]), DIMS[1:], zc))
    assert first.dims == ("yh", "xh") and first.is_device
    ref = cn.column_crossing(x[:1], Z7, 1, cn.RISE, True, cn.MISS_FLOOR, [0.03])
    equals_restatement(first.values, ref[0, 0].reshape(first.shape), "z first")
    T5, S5 = T.reshape(2, 3, 7, 3, 347), S.reshape(2, 3, 7, 3, 347)
    five = derived.calc_isopycnal_depth(DataArray(dev(T5), ("member",) + DIMS, zc),
                                        DataArray(dev(S5), ("member",) + DIMS, zc), [1024.0, 1026.0])
    assert five.dims == ("member", "time", "rhopot", "yh", "xh") and five.shape == (2, 3, 2, 3, 347)
    ref = cn.column_crossing(x, Z7, 0, cn.RISE, False, cn.MISS_NAN, [1024.0, 1026.0])
    equals_restatement(five.values, ref.reshape(five.shape), "5-D")


def test_host_masked_and_lazy_fields_give_the_device_calls_bits(monkeypatch):
    from lazy_array import CountingLazy, as_masked

    T, S, coords = _ocean(F64)
    S = S.astype(F32)
    nt, nz, ny, nx = T.shape
    want = derived.calc_mld(DataArray(dev(T), DIMS, coords), DataArray(dev(S), DIMS, coords),
                            threshold=[0.03, 0.125])
    small = derived.calc_mld(DataArray(T, DIMS, coords), DataArray(S, DIMS, coords), threshold=[0.03, 0.125])
    assert type(small.values) is np.ndarray and not small.is_device and same_bits(small.values, want.values)
    pieces = []
    real = hostio.Uploader.submit

    def counting(self, arrays):
        pieces.append([tuple(a.shape) for a in arrays])
        return real(self, arrays)

    monkeypatch.setattr(hostio.Uploader, "submit", counting)
    monkeypatch.setattr(hostio, "PIPELINE_ELEMS", 100)
    monkeypatch.setattr(hostio, "PIECE_ELEMS", 2 * nz * ny * nx)  # two steps a group
    for wrap in (lambda v: v, as_masked, CountingLazy):
        pieces.clear()
        got = derived.calc_mld(DataArray(wrap(T), DIMS, coords), DataArray(wrap(S), DIMS, coords),
                               threshold=[0.03, 0.125])
        assert pieces == [[(2, nz, ny, nx)] * 2] * 2 + [[(1, nz, ny, nx)] * 2]
        assert type(got.values) is np.ndarray and got.shape == (nt, 2, ny, nx)
        assert same_bits(got.values, want.values)
    lazy = CountingLazy(T)
    d = derived.calc_isosurface_depth(DataArray(lazy, DIMS, coords), 20.0)  # "auto" reads one record more
    assert lazy.largest_read == 2 * nz * ny * nx * 8 and len(lazy.reads) == 4  # never whole
    assert same_bits(d.values, derived.calc_isosurface_depth(DataArray(dev(T), DIMS, coords), 20.0,
                                                             direction="decreasing").values)


# ---- 5. status codes ---------------------------------------------------------------------------------------
def test_refusals_return_their_code_and_launch_nothing():
    from test_column_host import REFUSALS, column_call

    lib = _lib.load_column()
    nrec, nz, plane = 2, 3, 10
    a = torch.ones((nrec, nz, plane), dtype=torch.float64, device="cuda")
    a[:, 1] = 20.0
    a[:, 2] = 7.0
    b = torch.full((nrec, nz, plane), 35.0, dtype=torch.float32, device="cuda")
    z = dev(np.array([5.0, 15.0, 25.0]))
    floor = torch.full((plane,), 30.0, dtype=torch.float64, device="cuda")
    out = torch.full((nrec, 2, plane), 7.0, dtype=torch.float64, device="cuda")
    real = dict(a=a.data_ptr(), b=b.data_ptr(), z=z.data_ptr(), floor=floor.data_ptr(), out=out.data_ptr())
    for kw, code in REFUSALS:  # (the table's pointers are offsets from 1 << 20: here from real ones)
        args = dict(real)
        args.update({k: (v if v is None or k not in real else real[k] + (v - (1 << 20)))
                     for k, v in kw.items()})
        assert column_call(lib, **args) == code and _lib.last_error(), kw
    assert column_call(lib, nrec=0, **real) == 0
    torch.cuda.synchronize()
    assert torch.all(out == 7.0).item()  # nothing was launched
    assert column_call(lib, **real) == 0  # the same arguments, unrefused: it runs
    torch.cuda.synchronize()
    x = cn.sigma(a.cpu().numpy(), b.cpu().numpy(), 101325.0)
    ref = cn.column_crossing(x, [5.0, 15.0, 25.0], 1, cn.RISE, False, cn.MISS_FLOOR, [1027.0, 1027.5],
                             floor=np.full(plane, 30.0))
    equals_restatement(out, ref, "the unrefused call")
    assert np.isfinite(ref[:, 0]).all() and (ref[:, 1] == 30.0).all()
    with pytest.raises(ValueError):
        core.column_crossing(a, z, [1.0], mode="up")
    with pytest.raises(ValueError):
        core.column_crossing(a, z[:2], [1.0])
    with pytest.raises(ValueError):
        core.column_crossing(a, z, [1.0], b=b[:1])
    with pytest.raises(_lib.MomlevelHipError, match="relative"):
        core.column_crossing(a, z, [-1.0], relative=True)
    with pytest.raises(_lib.MomlevelHipError, match="kref"):
        core.column_crossing(a, z, [1.0], kref=3)
    empty = core.column_crossing(a[:0], z, [1.0])
    assert tuple(empty.shape) == (0, 1, plane)
