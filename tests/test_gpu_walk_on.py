"""GPU: the code a block or a launch reaches only when it WALKS ON -- a second tile of work for a
block, a second launch for a call -- at the smallest sizes that get there, against the same numpy
restatements as the suites of each kernel.  The other suites stop short of all of these: their
records fit one tile a block and one launch a call.

  * k_time_filter (csrc/momlevel_filter.hip), ``for (b = b0; b < b1; ++b)``: several time tiles a
    block, once the launch has its blocks without cutting time further.  Long records of one block
    of cells (core.filter_tiles_per_block >= 2 and >= 3) and one wide, short record.  The per-tile
    reset of the sums, the per-tile rows of a (nt, W) weight table and the clamp of the last block
    are what this loop adds.  Gate: bit-identical to filter_numpy.time_filter_taps, NaN mask
    included; a float32 result is that one rounded once.
  * k_layer_integral (csrc/momlevel_layer.hip), ``for (rb = blockIdx.y; rb < nrb; rb += gridDim.y)``:
    more groups of records than block rows (core.layer_record_blocks at its cap).  Gates:
    layer_numpy.layer_integral, and the records around the stride run on their own.
  * zeta_launch / pv_launch (csrc/momlevel_vort.hip), ``for (r0 = 0; r0 < nrec; r0 += step)``: a
    call of more records than one launch takes (core.vort_records_per_launch), so that a second
    launch starts at offsets of r0 whole planes.  Gates: vort_numpy on the records around the seam,
    and each side of it as a call of its own.
  * eos_map_impl (csrc/momlevel_hip.hip), ``for (tb = 0; tb < nt; tb += L)`` with
    ``t = t_base + blockIdx.z`` in k_eos_map: a record of more steps than one launch of the pointwise
    EOS map takes (core.k0_path).  That walk-on is in test_gpu_eos_matrix.py
    (test_k0_past_one_launch), beside the rest of that entry point's dispatch.
  * k_smooth_cells (csrc/momlevel_smooth.hip), ``for (rec = blockIdx.y; rec < nrec; rec += gridDim.y)``:
    more records than block rows (core.smooth_record_rows at its cap) on the cell-by-cell path, a
    plane of four cells.  Gates: smooth_numpy.plane_smooth, and the records around the stride as
    calls of their own.
  * k_regrid (csrc/momlevel_regrid.hip), ``for (win = blockIdx.y; win < nwin; win += gridDim.y)``:
    more windows of records than block rows (core.regrid_window_rows at its cap), the last window
    of one record.  Gates: regrid_numpy.apply_csr, and the records around the stride as calls of
    their own.

Every size comes from the library's queries at run time, every test asserts from the query that
the path was taken and prints the geometry.  Each result is written into a buffer that was filled
with a sentinel first: a step that is skipped leaves the sentinel, whatever the allocator handed
out.  (The fit windows longer than 256 steps of csrc/momlevel_trend.hip are in
test_gpu_trend_edges.py.)

OUT OF REACH, with the size at which each would first run; no test here gets there:
  * k_spice_map's tile stride: past 2^23 tiles of a launch;
  * the cell-by-cell vorticity kernels' grid stride: past 2^31 cells (2^23 blocks of 256);
  * K2's 2-D grid fallback: past 2^24 - 1 blocks;
  * the filter's cap of 65535 blocks along time: the target of 8192 blocks a launch never lets the
    time axis have that many;
  * k_gauge_nearest's ``part += gridDim.y``: mlx_gauge_nearest_split keeps the parts to one pass.
The horizontal filter and the remap have no other such loop: k_smooth_tiled takes one block per
(tile, record window) and k_regrid one per four slices along blockIdx.x, and the 2^38 cells a call
may hold keep both below the 2^31 blocks of gridDim.x (2^30 at the most).
"""

import numpy as np
import pytest
import torch

import filter_numpy as fn
import layer_numpy as ln
import regrid_numpy as rn
import smooth_numpy as sn
import vort_numpy as vn
from conftest import assert_bit_equal
from momlevel_amd import core, regrid
from test_gpu_filter_edges import _modes
from test_gpu_layer import _equals_restatement, _same_bits
from test_gpu_regrid_edges import _abi as _regrid_abi
from test_gpu_smooth import assert_same_bits
from test_gpu_smooth_edges import _abi as _smooth_abi

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
DEV = "cuda"
SENTINEL = 7.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _torch_dtype(dtype):
    return torch.float64 if dtype == F64 else torch.float32


# ---- the time filter: several time tiles a block ------------------------------------------------------
LAND, ONE_VALID, NEG_ZERO, ENDS_NAN = 0, 1, 2, 3  # special cells (every record here has >= 5)
# (dtype, cells, cells a lane when the pointers are aligned): one block of cells each
FILTER_CELLS = [(F64, 6, 2), (F64, 5, 1), (F32, 8, 4), (F32, 6, 2)]
FILTER_CELL_IDS = [f"{np.dtype(d).name}-{n}" for d, n, _ in FILTER_CELLS]
# 1, the edges of the kernel's walk over a window with the lengths beside them, and 25
WINDOW_ROLES = ["1", "edge0-1", "edge0", "edge0+1", "edge1-1", "edge1", "edge1+1", "25"]
_fields = {}


def _window(role):
    if not role.startswith("edge"):
        return int(role)
    return core.filter_window_edges()[int(role[4])] + int(role[5:] or 0)


def _long_nt(per):
    """by doubling: the smallest nt = tile * k + 1 that gives a block of (nt, 6) float64 ``per``
    tiles; the last tile holds one step"""
    tile, k = core.filter_tile(), 1
    while core.filter_tiles_per_block(tile * k + 1, 6, 2) < per:
        k *= 2
        assert k <= 1 << 20, "no record length gives a block that many tiles"
    return tile * k + 1


def _field(nt, n, dtype, keep=True):
    """test_gpu_filter_edges._record for a handful of cells: a land cell, 5 % scattered NaN, a cell
    with one valid step, a column of -0.0, a cell that is NaN on the first and on the last step;
    the last cell holds data"""
    key = (nt, n, np.dtype(dtype).name)
    if key in _fields:
        return _fields[key]
    assert n >= 5
    rng = np.random.default_rng(7 * nt + n)
    y = rng.normal(0.0, 1.0, (nt, n))
    y[rng.random((nt, n)) < 0.05] = np.nan
    y[:, LAND] = np.nan
    y[:, ONE_VALID] = np.nan
    y[nt // 2, ONE_VALID] = 1.5
    y[:, NEG_ZERO] = -0.0
    y[:, ENDS_NAN] = rng.normal(0.0, 1.0, nt)
    y[[0, nt - 1], ENDS_NAN] = np.nan
    y[:, n - 1] = rng.normal(0.0, 1.0, nt)
    y = y.astype(dtype)
    if keep:
        _fields[key] = y
    return y


def _filter_geometry(nt, n, v):
    tile = core.filter_tile()
    ntiles = -(-nt // tile)
    per = core.filter_tiles_per_block(nt, n, v)
    assert per >= 1
    blocks = -(-ntiles // per)
    return ntiles, per, blocks, ntiles - (blocks - 1) * per


def _filter_calls(y, yd, dtype, window, leads, modes):
    """every lead x mode on the device record ``yd`` against the tap loop on the host record ``y``;
    the weights go up once, the sums of one weight table serve every mode that uses it"""
    nt, n = y.shape
    weights = {id(w): _dev(np.asarray(w, dtype=F64)) for _l, w, _m, _n in modes}
    calls = 0
    for lead in leads:
        sums = {}
        for label, w, mc, norm in modes:
            if id(w) not in sums:
                sums[id(w)] = fn.tap_sums(y, w, lead)
            want = fn.finish(*sums[id(w)], mc, norm).astype(dtype)  # float32: rounded once
            out = torch.full((nt, n), SENTINEL, dtype=_torch_dtype(dtype), device=DEV)
            got = core.time_filter(yd, weights[id(w)], lead, mc, norm, out=out)
            assert got.data_ptr() == out.data_ptr()
            assert_bit_equal(got.cpu().numpy(), want,
                             f"W={window} lead={lead} {label} nt={nt} n={n} {np.dtype(dtype).name}")
            calls += 1
        assert np.isnan(want[:, LAND]).all()
    return calls


@pytest.mark.parametrize("role", WINDOW_ROLES)
@pytest.mark.parametrize("per", [2, 3])
@pytest.mark.parametrize("dtype, n, v", FILTER_CELLS, ids=FILTER_CELL_IDS)
def test_filter_long_records_give_a_block_several_tiles(dtype, n, v, per, role):
    assert len(core.filter_window_edges()) == 2, "WINDOW_ROLES names two edges: add the new ones"
    nt = _long_nt(per)
    # a retuned target must make this fail, not grow (today 65537 and 131073)
    assert nt <= (2 ** 17 if per == 2 else 2 ** 18), nt
    ntiles, got_per, blocks, last = _filter_geometry(nt, n, v)
    window = _window(role)
    print(f"filter nt={nt} n={n} {np.dtype(dtype).name} ({v} a lane): {ntiles} tiles, {got_per} a "
          f"block, {blocks} blocks along time, the last of {last}; W={window}")
    assert got_per >= per and 1 <= last <= got_per and nt % core.filter_tile() == 1
    y = _field(nt, n, dtype)
    yd = _dev(y)
    assert yd.data_ptr() % 16 == 0  # (so that the lanes are as wide as n allows: v)
    leads = sorted({window // 2, window - 1, (window - 1) // 3})  # centred, trailing, one other
    modes = _modes(window, np.random.default_rng(1000 * window + n), nt)
    assert sum(np.ndim(w) == 2 for _l, w, _m, _n in modes) == 2  # both tables: a row per tile
    calls = _filter_calls(y, yd, dtype, window, leads, modes)
    print(f"  {calls} calls bit-identical to the tap loop")


def test_filter_wide_short_record_gives_a_block_several_tiles():
    """float32, one cell a lane, nt <= 96: so many blocks of cells that the launch stops cutting
    time; n is the smallest odd count the query reports two tiles a block for"""
    dtype, nt, window = F32, 96, 13
    lo, hi = 1, 1 << 20  # per(lo) == 1 < per(hi): bisect
    assert core.filter_tiles_per_block(nt, lo, 1) == 1 and core.filter_tiles_per_block(nt, hi, 1) >= 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if core.filter_tiles_per_block(nt, mid, 1) >= 2 else (mid, hi)
    n = hi | 1
    assert n <= 300_000, n  # (about 191 000 today: 73 MB in and out; a retuned target fails here)
    ntiles, per, blocks, last = _filter_geometry(nt, n, 1)
    print(f"filter nt={nt} n={n} float32 (1 a lane): {ntiles} tiles, {per} a block, {blocks} "
          f"blocks along time, the last of {last}; W={window}")
    assert per >= 2 and n % 2 == 1
    y = _field(nt, n, dtype, keep=False)
    rng = np.random.default_rng(n)
    modes = [("mean mc=1", np.ones(window), 1, True),
             ("table mc=W", rng.normal(0.0, 1.0, (nt, window)), window, False)]
    calls = _filter_calls(y, _dev(y), dtype, window, [window // 2], modes)
    print(f"  {calls} calls bit-identical to the tap loop")


# ---- the layer integral: more groups of records than block rows ---------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("cells", ["cell by cell", "one pack"])
def test_layer_record_blocks_stride_past_the_cap(dtype, cells):
    S = core.LAYER_STEPS
    cap = core.layer_record_blocks(10 ** 9)
    nrec = S * cap + S + 1  # the first block row takes a second group, the second one of ONE record
    assert nrec <= 2 ** 19, nrec  # (262 145 today)
    groups = -(-nrec // S)
    plane = 3 if cells == "cell by cell" else 16 // np.dtype(dtype).itemsize
    print(f"layer {np.dtype(dtype).name} plane={plane}: {nrec} records, {groups} groups of {S} on "
          f"{core.layer_record_blocks(nrec)} block rows (the cap: {cap})")
    assert core.layer_record_blocks(nrec) == cap == groups - 2
    z_i = np.array([0.0, 10.0, 30.0])
    tops, bottoms = np.array([0.0, 17.0]), np.array([17.0, np.inf])  # a cut inside a cell; no bottom
    depth = np.array([25.0, np.nan, 30.0, 7.0])[:plane]  # a floor inside a cell, land
    surface = np.where(np.isnan(depth), np.nan, 1.0)
    rng = np.random.default_rng(nrec + plane)
    x = rng.normal(0.5, 3.0, (nrec, 2, plane))
    x[rng.random(x.shape) < 0.05] = np.nan
    x = x.astype(dtype)
    xd, zd, dd, sd = _dev(x), _dev(z_i), _dev(depth), _dev(surface)
    first = S * cap - 1  # the last record of the last block row's first group, then the strided ones
    tail = xd[first:]
    assert tail.is_contiguous() and tail.shape[0] == S + 2
    assert core.layer_record_blocks(S + 2) == -(-(S + 2) // S) < cap  # one block row a group
    for surf_np, surf_d, scale in ((None, None, 1.0), (surface, sd, -1.0 / 1035.0)):
        out = torch.full((nrec, 2, plane), SENTINEL, dtype=torch.float64, device=DEV)
        got = core.layer_integral(xd, zd, dd, tops, bottoms, surface=surf_d, scale=scale, out=out)
        assert got.data_ptr() == out.data_ptr()
        ref = ln.layer_integral(x, z_i, depth, tops, bottoms, surface=surf_np, scale=scale)
        what = f"{np.dtype(dtype).name} plane={plane} surface={surf_np is not None}"
        _equals_restatement(got, ref, what)
        alone = core.layer_integral(tail, zd, dd, tops, bottoms, surface=surf_d, scale=scale)
        assert _same_bits(alone, got[first:]), f"{what}: records [{first}, {nrec}) on their own"
    assert np.isfinite(ref[first:, :, 0]).all() and (ref[first:, :, 0] != 0.0).any()


# ---- the vorticity stencils: a call of more records than one launch takes -----------------------------
def _vort_geometry(dtype):
    """(P, step, nrec, records to download): a plane of two rows of one pack, three records more
    than a launch takes.  (With one row an offset of r0 * nx would be r0 * plane.)"""
    P = 16 // np.dtype(dtype).itemsize
    step = core.vort_records_per_launch(2, P, dtype)
    nrec = step + 3
    assert 0 < step < nrec <= 2 * step and nrec * 2 * P * np.dtype(dtype).itemsize <= 300 << 20
    print(f"vort {np.dtype(dtype).name}: plane (2, {P}), {step} records a launch, {nrec} records: "
          f"launches of {step} and {nrec - step}")
    sample = torch.tensor(list(range(3)) + list(range(step - 2, step + 3)), device=DEV)
    assert int(sample[-1]) == nrec - 1
    return P, step, nrec, sample


def _randn(gen, shape, dtype, mean, sd):
    t = torch.randn(shape, generator=gen, dtype=_torch_dtype(dtype), device=DEV)
    return t.mul_(sd).add_(mean)


def _uniform(gen, shape, dtype, lo, hi):
    t = torch.rand(shape, generator=gen, dtype=_torch_dtype(dtype), device=DEV)
    return t.mul_(hi - lo).add_(lo)


def _same_as_numpy(got, ref, what):
    got = got.cpu().numpy()
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    assert not np.isnan(ref).any() and not np.isnan(got).any(), f"{what}: a record was not written"
    view = np.int64 if ref.dtype == F64 else np.int32
    assert np.array_equal(got.view(view), np.ascontiguousarray(ref).view(view)), f"{what}: bits differ"


def _check_both_sides(call, whole, step, fields, what):
    """``whole[:step]`` and ``whole[step - 1:]`` are the calls on those views: one launch each"""
    for lo, hi in ((0, step), (step - 1, whole.shape[0])):
        assert hi - lo <= step
        views = [f[lo:hi] for f in fields]
        assert all(v.is_contiguous() and v.data_ptr() % 16 == 0 for v in views)
        part = call(*views)
        assert torch.equal(part, whole[lo:hi]), f"{what}: records [{lo}, {hi}) as a call of their own"
        del part


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_rel_vort_second_launch_starts_whole_planes_in(dtype):
    P, step, nrec, sample = _vort_geometry(dtype)
    gen = torch.Generator(device=DEV).manual_seed(20020187 + P)
    u = _randn(gen, (nrec, 2, P), dtype, 0.0061, 0.08)
    v = _randn(gen, (nrec, 2, P), dtype, 0.00077, 0.04)
    dx = _uniform(gen, (2, P), dtype, 2.0e4, 3.0e4)
    dy = _uniform(gen, (2, P), dtype, 1.0e4, 3.0e4)
    area = _uniform(gen, (2, P), dtype, 4.0e8, 9.0e8)
    out = torch.full((nrec, 2, P), float("nan"), dtype=_torch_dtype(dtype), device=DEV)
    assert all(t.data_ptr() % 16 == 0 for t in (u, v, dx, dy, area, out))  # the packed path
    whole = core.rel_vort(u, v, dx, dy, area, out=out)
    assert whole.data_ptr() == out.data_ptr()
    ref = vn.rel_vort(u[sample].cpu().numpy(), v[sample].cpu().numpy(), dx.cpu().numpy(),
                      dy.cpu().numpy(), area.cpu().numpy())
    _same_as_numpy(whole[sample], ref, f"zeta {np.dtype(dtype).name}, records {sample.tolist()}")
    _check_both_sides(lambda a, b: core.rel_vort(a, b, dx, dy, area), whole, step, (u, v),
                      f"zeta {np.dtype(dtype).name}")
    del u, v, out, whole
    torch.cuda.empty_cache()


@pytest.mark.parametrize("interp, units", [(True, "cm"), (False, "m")], ids=["interp-cm", "plain-m"])
def test_pv_second_launch_starts_whole_planes_in(interp, units):
    dtype = F64
    P, step, nrec, sample = _vort_geometry(dtype)
    gen = torch.Generator(device=DEV).manual_seed(20020187 + int(interp))
    zeta = _randn(gen, (nrec, 2, P), dtype, 0.0, 1.0e-5)
    n2 = _randn(gen, (nrec, 2, P), dtype, 1.0e-5, 2.0e-5)
    f = _randn(gen, (2, P), dtype, 1.21e-5, 1.1e-4)
    out = torch.full((nrec, 2, P), float("nan"), dtype=torch.float64, device=DEV)
    assert all(t.data_ptr() % 16 == 0 for t in (zeta, n2, f, out))  # the packed path
    kw = dict(gravity=9.8, interp=interp, units=units)
    whole = core.potential_vorticity(zeta, f, n2, out=out, **kw)
    assert whole.data_ptr() == out.data_ptr()
    ref = vn.pv(zeta[sample].cpu().numpy(), f.cpu().numpy(), n2[sample].cpu().numpy(), **kw)
    _same_as_numpy(whole[sample], ref, f"pv interp={interp} {units}, records {sample.tolist()}")
    _check_both_sides(lambda z, n: core.potential_vorticity(z, f, n, **kw), whole, step, (zeta, n2),
                      f"pv interp={interp} {units}")
    del zeta, n2, out, whole
    torch.cuda.empty_cache()


# ---- the horizontal filter, cell by cell: more records than block rows --------------------------------
@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "closed"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_smooth_cells_record_rows_stride_past_the_cap(dtype, periodic):
    cap = core.smooth_record_rows(1 << 30)
    nrec = cap + 3  # the first three block rows take a second record
    assert nrec <= 2 ** 17, nrec  # (65 538 today)
    ny, nx, Wx, Wy = 1, 4, 3, 1
    print(f"smooth {np.dtype(dtype).name} plane=({ny}, {nx}) window {Wy}x{Wx} periodic={periodic}: "
          f"{nrec} records on {core.smooth_record_rows(nrec)} block rows (the cap: {cap})")
    assert core.smooth_tiled(Wx, Wy, ny, nx) == 0  # cell by cell
    assert core.smooth_record_rows(nrec) == cap == nrec - 3
    rng = np.random.default_rng(nrec + int(periodic))
    v = rng.normal(0.2, 1.0, (nrec, ny, nx))
    v[rng.random(v.shape) < 0.1] = np.nan  # so that the records differ
    v = v.astype(dtype)
    area = np.array([[4.0e8, 9.0e8, 5.5e8, 7.0e8]])
    wx, wy = np.array([0.25, 0.5, 0.3]), np.array([1.0])
    want = sn.plane_smooth(v, area, wx, wy, 1, 0, periodic, 1, False, False, dtype)
    assert np.isnan(want).any() and np.isfinite(want).mean() > 0.5
    vd, ad, wxd, wyd = _dev(v), _dev(area), _dev(wx), _dev(wy)
    out = torch.full((nrec, ny, nx), SENTINEL, dtype=_torch_dtype(dtype), device=DEV)
    _smooth_abi(vd, ad, wxd, wyd, 1, 0, periodic, 1, 0, out)
    what = f"smooth {np.dtype(dtype).name} periodic={periodic}"
    assert_same_bits(out, want, what)
    for rec in (cap - 1, cap, cap + 2):  # the last first record of a row, the first and last strided
        one = torch.full((1, ny, nx), SENTINEL, dtype=_torch_dtype(dtype), device=DEV)
        _smooth_abi(vd[rec:rec + 1], ad, wxd, wyd, 1, 0, periodic, 1, 0, one)
        assert_same_bits(one, out[rec:rec + 1], f"{what}: record {rec} on its own")


# ---- the remap: more windows of records than block rows -----------------------------------------------
def test_regrid_window_rows_stride_past_the_cap():
    R = core.regrid_record_window()
    cap = core.regrid_window_rows(1 << 30)
    nrec = R * cap + R + 1  # the first block row takes a second window, the second one of ONE record
    assert nrec <= 2 ** 20, nrec  # (524 289 today: 21 MB in)
    nwin = -(-nrec // R)
    nsrc, ndst = 5, 3
    print(f"regrid float64 nsrc={nsrc} ndst={ndst}: {nrec} records, {nwin} windows of {R} on "
          f"{core.regrid_window_rows(nrec)} block rows (the cap: {cap})")
    assert core.regrid_window_rows(nrec) == cap == nwin - 2
    indptr = np.array([0, 2, 2, 5], dtype=np.int64)  # the second row is empty
    col = np.array([0, 1, 2, 3, 4], dtype=np.int32)
    S = np.array([1.25, 3.0, 2.5, 0.75, 4.0])
    rng = np.random.default_rng(nrec)
    v = rng.normal(0.2, 1.0, (nrec, nsrc))
    v[rng.random(v.shape) < 0.1] = np.nan
    want = rn.apply_csr(v, indptr, col, S, ndst)
    assert np.isnan(want[:, 1]).all() and np.isnan(want[:, 0]).any() and np.isfinite(want).mean() > 0.5
    vd = _dev(v)
    packed = [_dev(a) for a in regrid.pack_rows(indptr, col, S, core.regrid_slice())]
    out = torch.full((nrec, ndst), SENTINEL, dtype=torch.float64, device=DEV)
    _regrid_abi(vd, packed, ndst, out)
    assert_same_bits(out, want, "regrid float64")
    for rec in (R * cap - 1, R * cap, nrec - 1):  # the last record before the stride, the first past
        one = torch.full((1, ndst), SENTINEL, dtype=torch.float64, device=DEV)  # it, the last
        _regrid_abi(vd[rec:rec + 1], packed, ndst, one)
        assert_same_bits(one, out[rec:rec + 1], f"regrid: record {rec} on its own")
    del vd, out
    torch.cuda.empty_cache()
