"""GPU: the data edges of the census -- 64 lanes on one bin and 64 lanes on 64 bins, values exactly on
every edge, NaN, +-inf and -0.0, records with nothing in range, NaN weights and values, static
against per-record weights, the labeled results of ``histogram`` and the end-to-end ``ts_census`` on
the package's small test grid.  Against tests/census_numpy.py: counts always exactly, integer-valued
sums exactly, real-valued ones inside 1e-10 * sum |w|."""

import numpy as np
import pytest
import torch

import census_numpy as cn
from momlevel_amd import _lib, census, core, test_data
from momlevel_amd.labeled import DataArray
from test_gpu_census import (E3, E5, E7, F32, F64, GATE, _dev, _host, assert_same, exact, gpu_sums,
                             make_fields, make_int_operands)

pytestmark = pytest.mark.gpu


def _n():
    return 2 * core.census_tile() + 65  # two whole tiles and a wave and a lane of a third


def test_every_cell_in_one_bin():
    """64 lanes collide on one bin at every step: one trip of the leader loop"""
    n = _n()
    f = np.full((2, n), 0.5)
    w, v = make_int_operands(2, n, 1)
    got = gpu_sums([f], [E7], w, v)
    assert_same(got, exact([f], [E7], w, v), "one bin")
    assert got[0][:, 3].tolist() == [n, n] and got[0].sum() == 2 * n


def test_every_lane_of_a_wave_in_its_own_bin():
    """thread t owns cells 4t .. 4t + 3, so cell c belongs to lane (c // 4) % 64: 64 bins a step"""
    n = _n()
    lane = (np.arange(n) // 4) % 64
    f = np.stack([lane + 0.5, 63.5 - lane]).astype(F32)
    edges = np.arange(65.0)
    w, v = make_int_operands(2, n, 2, F32, F64)
    got = gpu_sums([f], [edges], w, v)
    assert_same(got, exact([f], [edges], w, v), "64 bins a step")
    assert (got[0] > 0).all()
    # and in two dims: 8 x 8 classes, every lane its own
    f2 = [np.stack([lane // 8 + 0.5] * 2), np.stack([lane % 8 + 0.5] * 2)]
    e2 = [np.arange(9.0), np.arange(9.0)]
    assert_same(gpu_sums(f2, e2, w, v), exact(f2, e2, w, v), "8 x 8 bins a step")


@pytest.mark.parametrize("dt", (F64, F32))
def test_values_on_every_edge_and_the_special_values(dt):
    """every edge (the last is closed), the neighbours of every edge, NaN, +-inf, -0.0 against the
    edge at 0.0 -- numpy.histogram's own answers (the host tests hold the restatement to them)"""
    e = E7
    near = np.concatenate([np.nextafter(e.astype(dt), dt(-np.inf)), np.nextafter(e.astype(dt), dt(np.inf))])
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e300 if dt is F64 else 1e38, -1e30])
    row = np.concatenate([e, near.astype(np.float64), special, e[::-1]]).astype(dt)
    f = np.stack([row, row[::-1]])
    got = gpu_sums([f], [e])
    want = cn.census([f], [e])
    assert_same(got, want, "edges")
    np_count = np.histogram(row[np.isfinite(row)].astype(np.float64), bins=e)[0]
    assert np.array_equal(got[0][0], np_count) and np.array_equal(got[0][1], np_count)
    assert got[0][0][-1] >= 2 and got[0][0][2] >= 4  # the last edge twice; 0.0, -0.0 and the edge
    # the same values as the second field of a 2-D table
    g = np.full_like(f, 1.0)
    assert_same(gpu_sums([g, f], [E3, e]), cn.census([g, f], [E3, e]), "edges, 2-D")


def test_nothing_in_range_gives_zeros():
    n = _n()
    f = np.concatenate([np.full(n // 2, -5.0), np.full(n - n // 2, 50.0)])[None]
    f[0, ::9] = np.nan
    w = np.ones(n)
    got = gpu_sums([f], [E7], w, f)
    assert all(not x.any() and x.shape == (1, 7) for x in got)
    assert not np.signbit(got[1]).any() and not np.signbit(got[2]).any()
    res, count = census.histogram(_dev(f), bins=E7, weights=_dev(w), values=_dev(f), tcoord="dim_0",
                                  return_count=True)
    assert torch.isnan(res).all() and not count.any()  # the class mean of an empty bin


def test_nan_weights_and_values_leave_their_cells_out():
    n = _n()
    f = make_fields(2, n, 5)
    w, v = make_int_operands(2, n, 5)
    w[:, 3::11] = np.nan
    v[:, 5::13] = np.nan
    w[1, :70] = np.nan  # a whole wave and more
    for fields, edges in (([f[0]], [E7]), (f, [E3, E5])):
        got = gpu_sums(fields, edges, w, v)
        assert_same(got, exact(fields, edges, w, v), "NaN weights and values")
        assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
        only_w = gpu_sums(fields, edges, w)
        assert_same(only_w, exact(fields, edges, w), "NaN weights")
        assert (only_w[0] >= got[0]).all() and (only_w[0] > got[0]).any()
        left = cn.left_out(fields, edges, w, v)
        assert np.array_equal(got[0].reshape(2, -1).sum(axis=1) + left, [n, n])
    ws = w[0].astype(F32)  # static
    assert_same(gpu_sums(f, [E3, E5], ws, v), exact(f, [E3, E5], ws, v), "static NaN weights")


def test_static_weights_are_the_per_record_weights_repeated():
    n = _n()
    rng = np.random.default_rng(8)
    f = make_fields(3, n, 8)
    w = rng.uniform(0.5, 2.0, n)
    v = rng.normal(0.0, 1.0, (3, n))
    a = gpu_sums(f, [E3, E5], w, v)
    b = gpu_sums(f, [E3, E5], np.broadcast_to(w, (3, n)).copy(), v)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))


def test_core_census_refusals_and_empty_shapes():
    e = _dev(E7)
    f = _dev(np.zeros((2, 10)))
    with pytest.raises(ValueError, match="bin groups"):
        core.census([f], [_dev(np.arange(core.census_max_bins(1) + 2.0))])
    with pytest.raises(ValueError, match="values need weights"):
        core.census([f], [e], None, f)
    with pytest.raises(ValueError, match="weights must be"):
        core.census([f], [e], _dev(np.ones(9)))
    with pytest.raises(ValueError, match="one or two fields"):
        core.census([f, f, f], [e, e, e])
    with pytest.raises(TypeError):
        core.census([np.zeros((2, 10))], [e])
    with pytest.raises(TypeError):
        core.census([f.to(torch.float16)], [e])
    c, w, v = core.census([f[:0]], [e], f[0], f[:0])
    assert c.shape == (0, 7) and w.shape == (0, 7) and v.shape == (0, 7)
    c, w, v = core.census([f[:, :0].contiguous()], [e], f[0, :0])
    assert c.shape == (2, 7) and not c.any() and not w.any() and v is None
    # the library itself: a workspace one byte short
    lib = _lib.load_census()
    need = core.census_workspace_bytes(2, 10, 7)
    ws = torch.empty(need // 8, dtype=torch.int64, device="cuda")
    out = torch.empty((2, 7), dtype=torch.int64, device="cuda")
    rc = lib.mlx_census_histogram(f.data_ptr(), 0, None, 0, 1, e.data_ptr(), 7, None, 1, 3, None, 0, 0,
                                  None, 0, 2, 10, out.data_ptr(), None, None, ws.data_ptr(), need - 1,
                                  None)
    assert rc == -4 and "workspace" in _lib.last_error()


# ---- the labeled layer --------------------------------------------------------------------------------
def test_histogram_labels_and_lives_where_the_fields_live():
    rng = np.random.default_rng(9)
    shape = (3, 4, 6, 7)
    th = rng.normal(10.0, 6.0, shape)
    so = rng.normal(35.0, 1.0, shape).astype(F32)
    vol = rng.uniform(1.0, 2.0, shape[1:])
    vol[0, 0, :3] = np.nan  # land
    tb, sb = census.bin_edges(-2.0, 30.0, 8), census.bin_edges(32.0, 38.0, 4)
    time = DataArray(np.arange(3.0), ("time",))
    dims = ("time", "z_l", "yh", "xh")
    mk = lambda a, name, dev: DataArray(_dev(a) if dev else a, dims[-a.ndim:], {"time": time} if a.ndim == 4
                                        else None, {"units": "m3"} if name == "volcello" else None, name)
    flat = lambda a: a.reshape(a.shape[0], -1)
    rc, rw, rv = cn.census([flat(th), flat(so)], [tb, sb], vol.reshape(-1), flat(th))
    for dev in (True, False):
        out, cnt = census.histogram(mk(th, "thetao", dev), mk(so, "so", dev), bins=(tb, sb),
                                    weights=mk(vol, "volcello", dev), return_count=True)
        assert out.dims == ("time", "thetao_bin", "so_bin") and out.shape == (3, 8, 4)
        assert out.is_device == dev and cnt.is_device == dev
        assert np.array_equal(out.coords["thetao_bin"].values, 0.5 * (tb[:-1] + tb[1:]))
        assert np.array_equal(out.attrs["so_bin_edges"], sb) and out.attrs["units"] == "m3"
        assert np.array_equal(out.coords["time"].values, np.arange(3.0))
        assert np.array_equal(cnt.values, rc) and cnt.values.dtype == np.int64
        aw, _ = cn.abs_sums([flat(th), flat(so)], [tb, sb], vol.reshape(-1))
        assert (np.abs(out.values - rw) <= GATE * aw).all()
        mean = census.histogram(mk(th, "thetao", dev), mk(so, "so", dev), bins=(tb, sb),
                                weights=mk(vol, "volcello", dev), values=mk(th, "thetao", dev))
        want = np.where(rc > 0, rv / np.where(rc > 0, rw, 1.0), np.nan)
        assert np.array_equal(np.isnan(mean.values), rc == 0)
        assert np.allclose(mean.values[rc > 0], want[rc > 0], rtol=1e-9, atol=0)
        one = census.histogram(mk(th, "thetao", dev)[0], bins=tb)  # no time dim: one table
        assert one.dims == ("thetao_bin",) and np.array_equal(one.values, cn.census([th[0].reshape(1, -1)], [tb])[0][0])


def test_ts_census_on_the_small_test_grid():
    """the sum over the classes is the in-range volume, computed on the host, within the gate"""
    ds = test_data.generate_test_data()
    th, so, vol = ds["thetao"], ds["so"], ds["volcello"]
    tb, sb = census.bin_edges(5.0, 25.0, 10), census.bin_edges(32.0, 38.0, 6)
    out = census.ts_census(th, so, vol, tb, sb)
    assert out.dims == ("time", "thetao_bin", "so_bin") and out.shape == (5, 10, 6)
    assert out.attrs["units"] == "m3" and not out.is_device
    t, s, v = (np.asarray(x.values).reshape(5, -1) for x in (th, so, vol))
    inside = (t >= tb[0]) & (t <= tb[-1]) & (s >= sb[0]) & (s <= sb[-1])
    assert 0 < inside.sum() < inside.size
    want = np.where(inside, v, 0.0).sum(axis=1)
    scale = np.where(inside, np.abs(v), 0.0).sum(axis=1)
    got = out.values.reshape(5, -1).sum(axis=1)
    print(f"worst |sum bins - in-range volume| / (1e-10 sum|v|) = {np.max(np.abs(got - want) / (GATE * scale)):.3e}")
    assert (np.abs(got - want) <= GATE * scale).all()
    rc, rw, _ = cn.census([t, s], [tb, sb], v)
    aw, _ = cn.abs_sums([t, s], [tb, sb], v)
    assert (np.abs(out.values - rw) <= GATE * aw).all()
    dev = census.ts_census(DataArray(_dev(th.values), th.dims, None, None, "thetao"),
                           DataArray(_dev(so.values), so.dims, None, None, "so"),
                           DataArray(_dev(vol.values), vol.dims), tb, sb, return_count=True)
    assert dev[0].is_device and np.array_equal(_host(dev[0].data).view(np.int64), out.values.view(np.int64))
    assert np.array_equal(_host(dev[1].data), rc)
