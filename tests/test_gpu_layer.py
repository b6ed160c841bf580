"""GPU: core.layer_integral (csrc/momlevel_layer.hip), derived.calc_layer_integral /
calc_heat_content and steric_layers against the numpy restatement tests/layer_numpy.py -- the only
yardstick: the functions are an extension, the reference has no counterpart.

Everything is BIT FOR BIT.  Against the restatement +0.0 and -0.0 count as equal (numpy's
``where`` form of the skipna sum and the kernel's agree on every value; the sign of a zero sum
that saw a -0.0 term is left open there); between two device results the bits are the same."""

import numpy as np
import pytest
import torch

import layer_numpy as ln
from momlevel_amd import _lib, core, derived, engine, hostio, steric_layers, synthetic
from momlevel_amd.labeled import DataArray, Dataset
from momlevel_amd.steric import OHC_CP, steric, steric_variants

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
INF = np.inf
# an uneven vertical grid; the deepest floor of the test columns is 330 (inside the last cell but one)
Z7 = np.array([0.0, 5.0, 15.0, 40.0, 90.0, 200.0, 350.0, 600.0])
Z1 = np.array([0.0, 350.0])
PLANES = (1, 3, 512, 1041, 2 * 1024 + 3)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _equals_restatement(got, ref, what=""):
    """bit equality, NaN placement included; +0.0 == -0.0"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == F64 and got.shape == ref.shape, f"{what}: {got.dtype} {got.shape} vs {ref.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN placement"
    m = ~np.isnan(ref)
    bad = got[m] != ref[m]
    assert not bad.any(), f"{what}: {int(bad.sum())} of {int(m.sum())} values differ"


def _layer_sets(z_i):
    """name -> (tops, bottoms) on the grid ``z_i``: cuts inside cells, on interfaces, overlaps"""
    zb = float(z_i[-1])
    if z_i.size == 2:  # one level: every cut is inside the cell or on its faces
        edges = [0.0, 100.0, zb, None]
        eight = [(k * 40.0, (k + 1) * 40.0 + 10.0) for k in range(7)] + [(300.0, None)]
    else:
        edges = [0.0, 27.0, float(z_i[4]), None]  # one edge inside a cell, one on an interface
        eight = [(0.0, 5.0), (5.0, 27.0), (27.0, 90.0), (90.0, 120.0), (120.0, 350.0), (350.0, None),
                 (0.0, 340.0), (3.0, 16.0)]
    nine = eight + [(0.0, None)]
    sets = {
        "whole": [(0.0, None)],
        "edges": edges,
        "overlap": [(0.0, 100.0), (0.0, 300.0)],
        # (top in a cell below every floor's: where top and the floor cut the SAME cell calc_dz gives
        #  min(zbot - top, depth - ztop), not 0)
        "below": [(0.0, 100.0), (zb, None) if z_i.size == 2 else (float(z_i[-2]), None)],
        "eight": eight,
        "nine": nine,
    }
    return {k: derived.layer_bounds(v) for k, v in sets.items()}


def _case(nrec, nz, plane, dtype, seed):
    """a field with scattered NaN, one all-NaN wet column, one +inf and one -inf; a depth with land
    (NaN), a floor inside a cell and one on an interface; a surface map with NaN on land and in one
    wet cell"""
    rng = np.random.default_rng(seed)
    z_i = Z7 if nz == 7 else Z1
    x = rng.normal(0.5, 3.0, (nrec, nz, plane))
    x[rng.random(x.shape) < 0.05] = np.nan
    depth = rng.uniform(1.0, 330.0, plane)
    depth[rng.random(plane) < 0.25] = np.nan
    if plane >= 3:
        depth[0], depth[1], depth[2] = 27.5, float(z_i[min(3, nz)]), 330.0
        x[:, :, 1] = np.nan  # an all-NaN wet column
        x[0, 0, 2], x[-1, nz - 1, 0] = np.inf, -np.inf
    else:
        depth[0] = 27.5
    surface = np.where(np.isnan(depth), np.nan, 1.0)
    if plane >= 3:
        surface[2] = np.nan
    return x.astype(dtype), z_i, depth, surface


# ---- 1. the kernel against the restatement ----------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("nz", [1, 7])
@pytest.mark.parametrize("plane", PLANES)
def test_kernel_equals_the_restatement(dtype, nz, plane):
    S = core.LAYER_STEPS
    for nrec in (1, S, S + 1, 2 * S + 3):
        x, z_i, depth, surface = _case(nrec, nz, plane, dtype, 1000 * plane + 10 * nrec + nz)
        xd, zd, dd, sd = _dev(x), _dev(z_i), _dev(depth), _dev(surface)
        for name, (tops, bottoms) in _layer_sets(z_i).items():
            for surf_np, surf_d, scale in ((None, None, 1.0), (surface, sd, -1.0 / 1035.0)):
                got = core.layer_integral(xd, zd, dd, tops, bottoms, surface=surf_d, scale=scale)
                assert got.is_cuda and tuple(got.shape) == (nrec, len(tops), plane)
                ref = ln.layer_integral(x, z_i, depth, tops, bottoms, surface=surf_np, scale=scale)
                _equals_restatement(got, ref, f"{dtype.__name__} nz={nz} plane={plane} nrec={nrec} "
                                              f"{name} surface={surf_np is not None}")
                if name == "below":  # nothing of the column lies in the layer: a zero, not a NaN
                    wet = np.ones(plane, bool) if surf_np is None else ~np.isnan(surf_np)
                    assert np.all(got.cpu().numpy()[:, 1, wet] == 0.0)


# ---- 2. independence ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("plane", [1041, 1044])  # the cell-by-cell twin, and whole packs
def test_a_result_depends_on_its_own_record_and_layer_only(dtype, plane):
    S = core.LAYER_STEPS
    nrec, nz = 2 * S + 3, 7
    x, z_i, depth, surface = _case(nrec, nz, plane, dtype, 77 + plane)
    tops, bottoms = _layer_sets(z_i)["eight"]
    xd, zd, dd, sd = _dev(x), _dev(z_i), _dev(depth), _dev(surface)
    kw = dict(surface=sd, scale=-1.0 / 1035.0)
    full = core.layer_integral(xd, zd, dd, tops, bottoms, **kw)
    assert _same_bits(full, core.layer_integral(xd, zd, dd, tops, bottoms, **kw))  # run to run
    for r in (0, 1, S, nrec - 1):  # a record alone and inside a longer run
        alone = core.layer_integral(xd[r:r + 1], zd, dd, tops, bottoms, **kw)
        assert _same_bits(alone[0], full[r]), f"record {r}"
    part = core.layer_integral(xd[3:S + 2], zd, dd, tops, bottoms, **kw)
    assert _same_bits(part, full[3:S + 2])
    for l in range(8):  # a layer alone and among eight
        alone = core.layer_integral(xd, zd, dd, tops[l:l + 1], bottoms[l:l + 1], **kw)
        assert _same_bits(alone[:, 0], full[:, l]), f"layer {l}"
    t9, b9 = _layer_sets(z_i)["nine"]  # two launches: the ninth layer is the whole column
    nine = core.layer_integral(xd, zd, dd, t9, b9, **kw)
    assert _same_bits(nine[:, :8], full)
    assert _same_bits(nine[:, 8], core.layer_integral(xd, zd, dd, [0.0], [INF], **kw)[:, 0])
    # x and out at an odd element offset of a larger buffer
    xbuf = torch.zeros(x.size + 3, dtype=xd.dtype, device="cuda")
    xbuf[1:1 + x.size] = xd.reshape(-1)
    obuf = torch.full((full.numel() + 3,), 7.0, dtype=torch.float64, device="cuda")
    out = obuf[1:1 + full.numel()].reshape(full.shape)
    got = core.layer_integral(xbuf[1:1 + x.size].reshape(x.shape), zd, dd, tops, bottoms, out=out, **kw)
    assert got.data_ptr() == out.data_ptr() and got.data_ptr() % 16 != 0
    assert _same_bits(got, full)
    assert obuf[0].item() == 7.0 and torch.all(obuf[1 + full.numel():] == 7.0).item()  # nothing beside it


# ---- 3. the tie to K2 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(5, 6, 7, 33), (3, 4, 2, 2052)])
def test_whole_column_of_k2s_delta_rho_is_k2s_eta(dtype, shape):
    nt, nz, ny, nx = shape
    g = synthetic.make_grid(ny, nx, nz)
    r = np.random.default_rng(3)
    mask = np.isnan(g["volcello"])
    T = np.where(mask[None], np.nan, r.uniform(-2, 32, shape)).astype(dtype)
    S = np.where(mask[None], np.nan, r.uniform(30, 40, shape)).astype(dtype)
    vol0 = _dev(g["volcello"])
    pres = g["z_l"] * 1.0e4 + 101325.0
    rho0 = core.eos_map(_dev(T[0]), _dev(S[0]), pres)
    rho0m = core.fold_mask(rho0, vol0)
    neg_inv = -1.0 / 1035.0
    drho, eta = core.steric_local(_dev(T), _dev(S), rho0m, vol0[0], pres, neg_inv, z_i=g["z_i"],
                                  deptho=g["deptho"])
    assert drho.dtype == torch.float64
    got = core.layer_integral(drho.reshape(nt, nz, ny * nx), g["z_i"], _dev(g["deptho"]).reshape(-1),
                              [0.0], [INF], surface=vol0[0].reshape(-1), scale=neg_inv)
    assert _same_bits(got.reshape(nt, ny, nx), eta)  # every bit, zero signs included
    assert np.isfinite(eta.cpu().numpy()).any()


# ---- 4. layers add up ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_consecutive_layers_add_up_to_the_whole_column(dtype):
    """|sum_l out_l - out_whole| <= 2 (nz + nl + 3) 2^-53 |scale| sum_z |dz x| per column, where no
    cell is cut twice: the two parts of a cut cell are each one rounding away from its thickness,
    every product is one rounding, each sum has fewer than nz roundings"""
    nrec, nz, plane = 5, 7, 2 * 1024 + 3
    rng = np.random.default_rng(5)
    x = rng.normal(0.5, 3.0, (nrec, nz, plane))
    x[rng.random(x.shape) < 0.05] = np.nan
    x = x.astype(dtype)
    depth = rng.uniform(1.0, 600.0, plane)
    depth[rng.random(plane) < 0.2] = np.nan
    edges = [0.0, 27.0, 90.0, 260.0, None]  # at most one cut per cell ...
    tops, bottoms = derived.layer_bounds(edges)
    nl = len(tops)
    cuts = np.array([27.0, 260.0])  # ... and the floor must not share a cell with a cut
    d0 = np.nan_to_num(depth, nan=0.0)
    cell_of = lambda v: np.searchsorted(Z7, v, side="right") - 1
    twice = np.zeros(plane, bool)
    for c in cuts:
        twice |= (cell_of(d0) == cell_of(c)) & (d0 > Z7[cell_of(c)]) & (d0 < Z7[cell_of(c) + 1])
    assert twice.any() and (~twice).sum() > plane // 2
    scale = -1.0 / 1035.0
    xd, zd, dd = _dev(x), _dev(Z7), _dev(depth)
    parts = core.layer_integral(xd, zd, dd, tops, bottoms, scale=scale).cpu().numpy()
    whole = core.layer_integral(xd, zd, dd, [0.0], [INF], scale=scale).cpu().numpy()[:, 0]
    bound = 2 * (nz + nl + 3) * 2.0 ** -53 * abs(scale) * ln.abs_sum(x, Z7, depth)
    err = np.abs(parts.sum(axis=1) - whole)
    worst = float(np.max(err[:, ~twice] / np.maximum(bound[:, ~twice], 1e-300)))
    print(f"{dtype.__name__}: worst |sum of layers - whole| / bound = {worst:.3f}")
    assert np.all(err[:, ~twice] <= bound[:, ~twice])


# ---- 5. calc_layer_integral ---------------------------------------------------------------------------------
DIMS = ("time", "z_l", "yh", "xh")


def _labelled_case(dtype=F64, nt=5, ny=3, nx=347, seed=21):
    x, z_i, depth, surface = _case(nt, 7, ny * nx, dtype, seed)
    x = x.reshape(nt, 7, ny, nx)
    zl = DataArray(0.5 * (Z7[1:] + Z7[:-1]), ("z_l",))
    coords = {"z_l": zl, "time": DataArray(np.arange(nt, dtype=float), ("time",))}
    return (x, DataArray(Z7, ("z_i",)), DataArray(depth.reshape(ny, nx), ("yh", "xh")),
            DataArray(surface.reshape(ny, nx), ("yh", "xh")), coords)


def test_calc_layer_integral_device_in_device_out_and_labels():
    x, zi, dep, wet, coords = _labelled_case()
    layers = [0, 27, 90, None]
    tops, bottoms = derived.layer_bounds(layers)
    out = derived.calc_layer_integral(DataArray(_dev(x), DIMS, coords), zi, dep, layers, wet=wet,
                                      scale=2.5)
    assert out.is_device and out.dims == ("time", "layer", "yh", "xh") and out.shape == (5, 3, 3, 347)
    assert out.coords["layer"].values.tolist() == [0, 1, 2]
    assert out.coords["layer_top"].values.tolist() == [0.0, 27.0, 90.0]
    lb = out.coords["layer_bottom"].values
    assert lb[:2].tolist() == [27.0, 90.0] and np.isnan(lb[2])
    assert "time" in out.coords and "z_l" not in out.coords
    ref = ln.layer_integral(x.reshape(5, 7, -1), Z7, dep.values.reshape(-1), tops, bottoms,
                            surface=wet.values.reshape(-1), scale=2.5).reshape(out.shape)
    _equals_restatement(out.values, ref, "device")
    # a device depth and wet map, pairs instead of edges: the same bits
    again = derived.calc_layer_integral(DataArray(_dev(x), DIMS, coords), zi,
                                        DataArray(_dev(dep.values), dep.dims),
                                        [(0, 27), (27, 90), (90, None)], wet=_dev(wet.values), scale=2.5)
    assert _same_bits(again.values, out.values)
    # a small host field: host out
    host = derived.calc_layer_integral(DataArray(x, DIMS, coords), zi, dep, layers, wet=wet, scale=2.5)
    assert type(host.values) is np.ndarray and not host.is_device
    assert _same_bits(host.values, out.values)


def test_z_first_and_a_5d_field():
    x, zi, dep, wet, _ = _labelled_case(F32, nt=6)
    layers = [(0, 100), (0, 300)]
    tops, bottoms = derived.layer_bounds(layers)
    z_first = derived.calc_layer_integral(DataArray(_dev(x[0]), DIMS[1:]), zi, dep, layers)
    assert z_first.dims == ("layer", "yh", "xh") and z_first.is_device
    ref = ln.layer_integral(x[:1].reshape(1, 7, -1), Z7, dep.values.reshape(-1), tops, bottoms)
    _equals_restatement(z_first.values, ref.reshape(z_first.shape), "z first")
    x5 = x.reshape(2, 3, 7, 3, 347)
    five = derived.calc_layer_integral(DataArray(_dev(x5), ("member",) + DIMS), zi, dep, layers)
    assert five.dims == ("member", "time", "layer", "yh", "xh") and five.shape == (2, 3, 2, 3, 347)
    ref = ln.layer_integral(x.reshape(6, 7, -1), Z7, dep.values.reshape(-1), tops, bottoms)
    _equals_restatement(five.values, ref.reshape(five.shape), "5-D")


def test_host_masked_and_lazy_fields_give_the_device_calls_bits(monkeypatch):
    from lazy_array import CountingLazy, as_masked

    x, zi, dep, wet, coords = _labelled_case(F64)
    nt, nz, ny, nx = x.shape
    layers = [0, 27, 90, None]
    want = derived.calc_layer_integral(DataArray(_dev(x), DIMS, coords), zi, dep, layers, wet=wet)
    pieces = []
    real = hostio.Uploader.submit

    def counting(self, arrays):
        pieces.append([tuple(a.shape) for a in arrays])
        return real(self, arrays)

    monkeypatch.setattr(hostio.Uploader, "submit", counting)
    monkeypatch.setattr(hostio, "PIPELINE_ELEMS", 100)
    monkeypatch.setattr(hostio, "PIECE_ELEMS", 2 * nz * ny * nx)  # two steps a group
    for src in (x, as_masked(x), CountingLazy(x)):
        pieces.clear()
        got = derived.calc_layer_integral(DataArray(src, DIMS, coords), zi, dep, layers, wet=wet)
        assert pieces == [[(2, nz, ny, nx)]] * 2 + [[(1, nz, ny, nx)]]
        assert type(got.values) is np.ndarray and got.shape == (nt, 3, ny, nx)
        assert _same_bits(got.values, want.values)
    lazy = CountingLazy(x)
    derived.calc_layer_integral(DataArray(lazy, DIMS, coords), zi, dep, layers)
    assert len(lazy.reads) == 3 and lazy.largest_read == 2 * nz * ny * nx * 8  # never whole
    # a 5-D host field goes in groups of its leading rows too
    x5 = x[:4].reshape(2, 2, nz, ny, nx)
    monkeypatch.setattr(hostio, "PIECE_ELEMS", 2 * nz * ny * nx)
    got = derived.calc_layer_integral(DataArray(x5, ("member",) + DIMS), zi, dep, layers, wet=wet)
    assert _same_bits(got.values, want.values[:4].reshape(got.shape))


# ---- 6. calc_heat_content ---------------------------------------------------------------------------------------
def test_heat_content_is_the_scaled_layer_integral():
    x, zi, dep, wet, coords = _labelled_case(F32)
    theta = DataArray(_dev(x), DIMS, coords)
    layers = [0, 27, 90, None]
    tops, bottoms = derived.layer_bounds(layers)
    scale = float(np.float64(1035.0) * np.float64(OHC_CP))
    ohc = derived.calc_heat_content(theta, zi, dep, layers, wet=wet)
    assert ohc.dims == ("time", "layer", "yh", "xh") and ohc.attrs["units"] == "J m-2"
    assert "rhozero=1035.0" in ohc.attrs["comment"] and "cp=3992.0" in ohc.attrs["comment"]
    ref = ln.layer_integral(x.reshape(5, 7, -1), Z7, dep.values.reshape(-1), tops, bottoms,
                            surface=wet.values.reshape(-1), scale=scale)
    _equals_restatement(ohc.values, ref.reshape(ohc.shape), "heat content")
    whole = derived.calc_heat_content(theta, zi, dep, wet=wet, rhozero=1030.0, cp=4000.0)
    assert whole.dims == ("time", "yh", "xh") and "layer" not in whole.coords
    assert "layer_top" not in whole.coords and whole.attrs["units"] == "J m-2"
    one = derived.calc_heat_content(theta, zi, dep, [(0, None)], wet=wet, rhozero=1030.0, cp=4000.0)
    assert one.dims == ("time", "layer", "yh", "xh") and one.shape[1] == 1
    assert _same_bits(whole.values, one.values[:, 0])
    ref = ln.layer_integral(x.reshape(5, 7, -1), Z7, dep.values.reshape(-1), [0.0], [INF],
                            surface=wet.values.reshape(-1),
                            scale=float(np.float64(1030.0) * np.float64(4000.0)))
    _equals_restatement(whole.values, ref[:, 0].reshape(whole.shape), "whole column")


# ---- 7. steric_layers end to end ------------------------------------------------------------------------------------
def _dataset(dtype, nt=5, nz=6, ny=3, nx=347, seed=7):
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
    d["thetao"] = DataArray(T.astype(dtype), DIMS)
    d["so"] = DataArray(S.astype(dtype), DIMS)
    d["volcello"] = DataArray(vol, DIMS)
    d["areacello"] = DataArray(g["areacello"], ("yh", "xh"))
    d["deptho"] = DataArray(g["deptho"], ("yh", "xh"))
    return d


def _steric_layer_edges(d):
    """consecutive layers: one edge inside a cell, one on an interface, the sea floor"""
    z = d["z_i"].values
    return [0.0, float(0.5 * (z[1] + z[2])), float(z[4]), None]


def _check_steric_layers(d, res, variants, layers, truth):
    tops, bottoms = derived.layer_bounds(layers)
    nt, nz, ny, nx = d["thetao"].shape
    surface = d["volcello"].values[0, 0].reshape(-1)
    for v in variants:
        r = res[v]
        assert "delta_rho" not in r.variables and sorted(r.data_vars) == sorted([v, v + "_layers"])
        eta, lay = r[v], r[v + "_layers"]
        assert eta.dims == ("time", "yh", "xh") and lay.dims == ("time", "layer", "yh", "xh")
        assert lay.shape == (nt, len(tops), ny, nx)
        assert eta.attrs["units"] == lay.attrs["units"] == "m"
        assert lay.attrs["long_name"] == f"{v.capitalize()} height adjustment by depth layer"
        assert eta.encoding["dtype"] == lay.encoding["dtype"] == "float32"
        assert lay.coords["layer"].values.tolist() == list(range(len(tops)))
        assert lay.coords["layer_top"].values.tolist() == tops.tolist()
        assert np.array_equal(lay.coords["layer_bottom"].values,
                              np.where(np.isinf(bottoms), np.nan, bottoms), equal_nan=True)
        assert np.isnan(lay.coords["layer_bottom"].values).sum() == 1  # (the sea floor)
        assert _same_bits(eta.values, truth[v][v].values), v  # steric()'s own bits
        drho = truth[v]["delta_rho"].values
        assert drho.dtype == F64
        ref = ln.layer_integral(drho.reshape(nt, nz, -1), d["z_i"].values,
                                d["deptho"].values.reshape(-1), tops, bottoms, surface=surface,
                                scale=-1.0 / 1035.0)
        _equals_restatement(lay.values, ref.reshape(lay.shape), v + "_layers")


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_steric_layers_end_to_end(dtype, monkeypatch):
    d = _dataset(dtype)
    layers = _steric_layer_edges(d)
    all3 = ("steric", "thermosteric", "halosteric")
    truth, ref0 = steric_variants(d, domain="local")
    for v in all3:
        single, _ = steric(d, variant=v)
        assert _same_bits(single[v].values, truth[v][v].values)
    monkeypatch.setattr(engine, "chunk_steps", lambda nt, b, dev, budget_bytes=None: 2)
    res, ref = steric_layers(d, layers, variants=all3)  # host inputs, several time chunks
    assert type(res["steric"]["steric_layers"].values) is np.ndarray
    assert _same_bits(ref["rho"].values, ref0["rho"].values)
    _check_steric_layers(d, res, all3, layers, truth)
    one, _ = steric_layers(d, layers, variants=("thermosteric",))
    assert list(one) == ["thermosteric"]
    _check_steric_layers(d, one, ("thermosteric",), layers, truth)
    two, _ = steric_layers(d, [(0, None), (0.0, float(d["z_i"].values[2]))], variants=("halosteric", "steric"),
                           reference=ref0)  # a supplied reference; overlapping pairs; per-variant launches
    _check_steric_layers(d, two, ("halosteric", "steric"), [(0, None), (0.0, float(d["z_i"].values[2]))], truth)
    assert _same_bits(two["steric"]["steric_layers"].values[:, 0], two["steric"]["steric"].values)
    # device-resident inputs: the same bits, as device tensors
    dd = d.copy()
    for k in ("thetao", "so", "volcello"):
        dd[k] = DataArray(_dev(d[k].values), d[k].dims)
    for variants in (all3, ("thermosteric",)):
        dres, _ = steric_layers(dd, layers, variants=variants)
        for v in variants:
            assert dres[v][v].is_device and dres[v][v + "_layers"].is_device
            assert _same_bits(dres[v][v].values, res[v][v].values)
            assert _same_bits(dres[v][v + "_layers"].values, res[v][v + "_layers"].values)
    default, _ = steric_layers(d, layers)
    assert list(default) == ["steric"]
    assert _same_bits(default["steric"]["steric_layers"].values, res["steric"]["steric_layers"].values)


def test_steric_layers_refusals():
    d = _dataset(F64, nt=2)
    z = d["z_i"].values
    with pytest.raises(ValueError, match="strictly inside one model cell"):
        steric_layers(d, [(z[1] + 0.1 * (z[2] - z[1]), z[1] + 0.9 * (z[2] - z[1]))])
    with pytest.raises(ValueError):
        steric_layers(d, [])
    with pytest.raises(ValueError, match="Unknown variant"):
        steric_layers(d, [0, None], variants=("heat",))


# ---- 8. status codes ---------------------------------------------------------------------------------------------------------
def test_refusals_return_their_code_and_launch_nothing():
    from test_layer_host import REFUSALS, layer_call

    lib = _lib.load_layer()
    nrec, nz, plane = 2, 3, 10
    x = torch.ones((nrec, nz, plane), dtype=torch.float64, device="cuda")
    z_i = _dev(np.array([0.0, 3.0, 6.0, 9.0]))
    depth = torch.full((plane,), 9.0, dtype=torch.float64, device="cuda")
    out = torch.full((nrec, 2, plane), 7.0, dtype=torch.float64, device="cuda")
    real = dict(x=x.data_ptr(), z_i=z_i.data_ptr(), depth=depth.data_ptr(),
                surface=depth.data_ptr(), out=out.data_ptr())
    for kw, code in REFUSALS:  # (the table's pointers are offsets from 1 << 20: here from real ones)
        a = dict(real)
        a.update({k: (v if v is None or k not in real else real[k] + (v - (1 << 20)))
                  for k, v in kw.items()})
        assert layer_call(lib, **a) == code and _lib.last_error(), kw
    assert layer_call(lib, nrec=0, **real) == 0
    torch.cuda.synchronize()
    assert torch.all(out == 7.0).item()  # nothing was launched
    assert layer_call(lib, **real) == 0  # the same arguments, unrefused: it runs
    torch.cuda.synchronize()
    assert out[:, 0].cpu().numpy().tolist() == [[5.0] * plane] * nrec
    assert out[:, 1].cpu().numpy().tolist() == [[4.0] * plane] * nrec
    with pytest.raises(ValueError):
        core.layer_integral(x, z_i, depth, [0.0], [1.0, 2.0])
    with pytest.raises(_lib.MomlevelHipError, match="bottom"):
        core.layer_integral(x, z_i, depth, [5.0], [2.0])
    empty = core.layer_integral(x[:0], z_i, depth, [0.0], [INF])
    assert tuple(empty.shape) == (0, 1, plane)
