"""GPU: the edges of the horizontal filter -- the same plane through the packed and the generic
path, result buffers with guard bands (tests/out_contract.py), and the public layer
momlevel_amd.spatial on numpy, device and Dataset input.  Everything against
tests/smooth_numpy.py, bit for bit."""

import numpy as np
import pytest
import torch

import smooth_numpy as sn
from momlevel_amd import _lib, core, hostio, spatial
from momlevel_amd.labeled import DataArray, Dataset
from out_contract import Guarded
from test_gpu_smooth import F32, F64, TORCH, _dev, _plane, _weights, assert_same_bits, make_case, run

pytestmark = pytest.mark.gpu


def _abi(v, area, wx, wy, lx, ly, periodic, mc, flags, out):
    """mlx_smooth_apply itself, into ``out`` (any device tensor of the result's shape)"""
    code = {torch.float64: _lib.DTYPE_F64, torch.float32: _lib.DTYPE_F32}
    nrec, ny, nx = v.shape
    core._call(_lib.load_smooth(), "mlx_smooth_apply", v.device, v.data_ptr(), code[v.dtype],
               area.data_ptr(), code[area.dtype], wx.data_ptr(), wx.shape[-1],
               wx.shape[-1] if wx.dim() == 2 else 0, lx, wy.data_ptr(), wy.shape[0], ly,
               int(periodic), mc, flags, nrec, ny, nx, out.data_ptr(), code[out.dtype])
    torch.cuda.synchronize()


def _offset_by_one(a):
    """the same values in a device tensor that starts one element past a 16-byte boundary"""
    buf = torch.empty(a.size + 1, dtype=TORCH[a.dtype.type], device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


# ---- the same plane through both paths --------------------------------------------------------------
@pytest.mark.parametrize("vdt", (F64, F32), ids=("v64", "v32"))
@pytest.mark.parametrize("window", ((3, 3), (9, 5), (33, 33)), ids=("3x3", "9x5", "33x33"))
def test_an_offset_pointer_takes_the_generic_path_to_the_same_bits(window, vdt):
    Wx, Wy = window
    ny, nx = _plane(Wy, vdt)
    v, area = make_case(2, ny, nx, vdt, seed=60 + Wx)
    wx, wy = _weights(Wx, 1), _weights(Wy, 2)
    for periodic in (True, False):
        packed = run(v, area, wx, wy, Wx // 2, Wy // 2, periodic, fill=True)
        off = core.plane_smooth(_offset_by_one(v), _dev(area), wx, wy, Wx // 2, Wy // 2, periodic, 1,
                                fill=True)
        assert_same_bits(off, packed, f"v offset by one element, periodic={periodic}")
        off_area = core.plane_smooth(_dev(v), _offset_by_one(area), wx, wy, Wx // 2, Wy // 2,
                                     periodic, 1, fill=True)  # (the maps are read cell by cell)
        assert_same_bits(off_area, packed, f"area offset by one element, periodic={periodic}")
        want = sn.plane_smooth(v, area, wx, wy, Wx // 2, Wy // 2, periodic, 1, True, False, vdt)
        assert_same_bits(packed, want, "the restatement")


@pytest.mark.parametrize("vdt", (F64, F32), ids=("v64", "v32"))
@pytest.mark.parametrize("window", ((3, 3), (9, 5), (33, 33)), ids=("3x3", "9x5", "33x33"))
def test_an_odd_nx_takes_the_generic_path_to_the_same_bits(window, vdt):
    """closed x edges: the plane without its last column (nx odd: no whole packs) against the plane
    whose last column carries no weight -- a cell outside the plane and a cell that is not valid
    add the same nothing, so every other column has the same bits"""
    Wx, Wy = window
    ny, nx = _plane(Wy, vdt)
    v, area = make_case(2, ny, nx, vdt, seed=70 + Wx)
    area[:, -1] = 0.0
    wx, wy = _weights(Wx, 3), _weights(Wy, 4)
    packed = run(v, area, wx, wy, Wx // 2, Wy // 2, False, fill=True)
    odd = run(v[:, :, :-1], area[:, :-1], wx, wy, Wx // 2, Wy // 2, False, fill=True)
    assert (nx - 1) % 2 == 1
    assert_same_bits(odd, packed[:, :, :-1], "nx - 1 columns")
    want = sn.plane_smooth(v[:, :, :-1], area[:, :-1], wx, wy, Wx // 2, Wy // 2, False, 1, True,
                           False, vdt)
    assert_same_bits(odd, want, "the restatement")
    for periodic in (True, False):  # and the odd plane on its own, wrapped too
        got = run(v[:, :, :-1], area[:, :-1], wx, wy, Wx // 2, Wy // 2, periodic, mc=2)
        want = sn.plane_smooth(v[:, :, :-1], area[:, :-1], wx, wy, Wx // 2, Wy // 2, periodic, 2,
                               False, False, vdt)
        assert_same_bits(got, want, f"odd nx, periodic={periodic}")


def test_planes_smaller_than_a_tile():
    th, tw = core.smooth_tile(F64)
    for ny, nx in ((1, 1), (1, 8), (3, 5), (th - 1, tw + 4), (th + 1, tw - 4), (2, tw + 4)):
        v, area = make_case(2, ny, nx, seed=ny * 100 + nx, land=False)
        Wx, Wy = min(3, nx), min(3, ny)
        for periodic in (True, False):
            got = run(v, area, _weights(Wx, 1), _weights(Wy, 2), Wx // 2, Wy // 2, periodic)
            want = sn.plane_smooth(v, area, _weights(Wx, 1), _weights(Wy, 2), Wx // 2, Wy // 2,
                                   periodic, 1)
            assert_same_bits(got, want, f"{ny} x {nx} periodic={periodic}")


# ---- result buffers with guard bands ----------------------------------------------------------------
@pytest.mark.parametrize("odt", (F64, F32), ids=("o64", "o32"))
@pytest.mark.parametrize("offset", (0, 1), ids=("aligned", "offset"))
@pytest.mark.parametrize("window", ((3, 3), (33, 33), (35, 3)), ids=("3x3", "33x33", "35x3"))
def test_the_result_is_written_inside_its_buffer_and_nowhere_else(window, offset, odt):
    """every tile of the last row and column is partial; offset 1 is the generic path"""
    Wx, Wy = window
    ny, nx = _plane(Wy)
    v, area = make_case(3, ny, nx, seed=80 + Wx)
    wx, wy = _weights(Wx, 5), _weights(Wy, 6)
    for flags, (fill, residual) in ((0, (False, False)), (3, (True, True))):
        g = Guarded((3, ny, nx), TORCH[odt], "cuda", offset=offset)
        _abi(_dev(v), _dev(area), _dev(wx), _dev(wy), Wx // 2, Wy // 2, True, 1, flags, g.view)
        g.assert_intact(f"{Wx}x{Wy} offset={offset} flags={flags}")
        assert g.unwritten() == 0
        want = sn.plane_smooth(v, area, wx, wy, Wx // 2, Wy // 2, True, 1, fill, residual, odt)
        assert_same_bits(g.view, want, f"guarded {Wx}x{Wy} offset={offset} flags={flags}")


def test_an_out_that_overlaps_an_operand_is_refused_by_the_library():
    ny, nx = _plane()
    v, area = make_case(2, ny, nx, seed=90)
    dv, da, wx, wy = _dev(v), _dev(area), _dev(_weights(3, 1)), _dev(_weights(3, 2))
    with pytest.raises(_lib.MomlevelHipError, match="overlaps"):
        _abi(dv, da, wx, wy, 1, 1, True, 1, 0, dv)
    with pytest.raises(_lib.MomlevelHipError, match="overlaps"):
        _abi(dv, da, wx, wy, 1, 1, True, 1, 0, dv[1:])
    assert_same_bits(dv, v, "the record is untouched")


# ---- the public layer ---------------------------------------------------------------------------------
def _labelled(vdt, nt=3, seed=95):
    ny, nx = _plane()
    v, area = make_case(nt, ny, nx, vdt, seed=seed)
    time = DataArray(np.arange(float(nt)), ("time",), None, {"axis": "T"}, "time")
    yh = DataArray(np.linspace(-60.0, 60.0, ny), ("yh",), None, {"units": "degrees_north"}, "yh")
    eta = DataArray(v, ("time", "yh", "xh"), {"time": time, "yh": yh},
                    {"units": "m", "long_name": "sea level"}, "zos")
    cell = DataArray(area, ("yh", "xh"), {"yh": yh}, {"units": "m2"}, "areacello")
    return eta, cell, v, area


@pytest.mark.parametrize("vdt", (F64, F32), ids=("v64", "v32"))
def test_numpy_in_numpy_out_device_in_device_out(vdt):
    eta, cell, v, area = _labelled(vdt)
    w = spatial.gaussian_weights(1.0)
    assert w.size == 7
    want_s = sn.plane_smooth(v, area, w, w, 3, 3, True, 1, False, False, vdt)
    want_h = sn.plane_smooth(v, area, w, w, 3, 3, True, 1, False, True, vdt)
    for fn, want in ((spatial.smooth, want_s), (spatial.highpass, want_h)):
        host = fn(v, area, w)
        assert isinstance(host, np.ndarray) and host.dtype == vdt
        assert_same_bits(host, want, f"{fn.__name__}: numpy in")
        dev = fn(_dev(v), _dev(area), w)
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == TORCH[vdt]
        assert_same_bits(dev, want, f"{fn.__name__}: device in")
        lab = fn(eta, cell, w)
        assert isinstance(lab, DataArray) and lab.dims == eta.dims and lab.name == "zos"
        assert lab.attrs == eta.attrs and set(lab.coords) == set(eta.coords)
        assert lab.dtype == vdt and not lab.is_device
        assert_same_bits(lab.values, want, f"{fn.__name__}: DataArray in")
        resident = fn(DataArray(_dev(v), eta.dims, eta.coords, eta.attrs, "zos"), cell, w)
        assert resident.is_device and resident.dims == eta.dims
        assert_same_bits(resident.data, want, f"{fn.__name__}: resident DataArray")
    # a 4-D record: every leading index is a record of its own
    four = spatial.smooth(np.stack([v, v[::-1]]), area, w)
    assert four.shape == (2,) + v.shape
    assert_same_bits(four[1], want_s[::-1], "leading dims are records")
    # other keywords reach the kernel
    closed = spatial.smooth(v, area, spatial.boxcar_weights(3), spatial.boxcar_weights(5),
                            periodic_x=False, min_count=4, fill=True)
    b3, b5 = spatial.boxcar_weights(3), spatial.boxcar_weights(5)
    assert_same_bits(closed, sn.plane_smooth(v, area, b3, b5, 1, 2, False, 4, True, False, vdt), "keywords")
    trailing = spatial.smooth(v, area, [1.0, 2.0], [1.0, 1.0, 1.0, 3.0], center=False)
    assert_same_bits(trailing, sn.plane_smooth(v, area, [1.0, 2.0], [1.0, 1.0, 1.0, 3.0], 1, 3, True, 1,
                                               False, False, vdt), "center=False")


def test_smooth_plus_highpass_is_the_record():
    """float64.  RESIDUAL is one subtraction, so highpass == v - smooth to the bit for any record.
    Adding the smooth back is exact where the subtraction was (Sterbenz: smooth / 2 <= v <= 2
    smooth): a record in [1, 1.5] under positive weights has its smooth in [1, 1.5] too, so there
    smooth + highpass == v to the bit."""
    eta, cell, v, area = _labelled(F64)
    w = spatial.gaussian_weights(1.5)
    s, h = spatial.smooth(v, area, w), spatial.highpass(v, area, w)
    both = ~np.isnan(s)
    assert both.any() and np.array_equal(both, ~np.isnan(h))
    assert_same_bits(h[both], v[both] - s[both], "highpass == v - smooth")
    near = np.where(np.isnan(v), np.nan, 1.0 + 0.5 * np.random.default_rng(1).random(v.shape))
    s, h = spatial.smooth(near, area, w), spatial.highpass(near, area, w)
    both = ~np.isnan(s)
    assert both.sum() > near.size // 2 and np.array_equal(both, ~np.isnan(h))
    assert_same_bits(s[both] + h[both], near[both], "smooth + highpass == v")
    # float32: both are rounded once from float64, so the identity holds to float32 rounding only
    s32 = spatial.smooth(near.astype(F32), area, w)
    h32 = spatial.highpass(near.astype(F32), area, w)
    assert s32.dtype == h32.dtype == F32
    err = np.abs((s32[both].astype(F64) + h32[both]) - near.astype(F32)[both])
    assert err.max() <= 2.0 ** -23 * 1.5  # half an ulp of each rounding at values below 2


def test_a_dataset_and_a_length_scale_table():
    eta, cell, v, area = _labelled(F64)
    ny = v.shape[1]
    dx = 100.0 * np.cos(np.deg2rad(eta.coords["yh"].values))
    table = spatial.length_scale_weights(120.0, dx, "gaussian")
    assert table.shape[0] == ny and table.shape[1] > 7
    wy = spatial.gaussian_weights(1.2)
    ds = Dataset({"zos": eta, "steps": DataArray(np.arange(3.0), ("time",)), "areacello": cell})
    out = spatial.smooth(ds, cell, table, wy, min_count=3)
    assert isinstance(out, Dataset) and set(out.data_vars) == {"zos", "steps", "areacello"}
    assert out["zos"].dims == eta.dims and out["zos"].attrs == eta.attrs
    assert np.array_equal(out["steps"].values, np.arange(3.0))
    want = sn.plane_smooth(v, area, table, wy, table.shape[1] // 2, wy.size // 2, True, 3)
    assert_same_bits(out["zos"].values, want, "Dataset: zos")
    want_a = sn.plane_smooth(area[None], area, table, wy, table.shape[1] // 2, wy.size // 2, True, 3)
    assert_same_bits(out["areacello"].values, want_a[0], "Dataset: a 2-D variable is one record")


def test_a_large_host_record_goes_in_groups_of_leading_rows(monkeypatch):
    eta, cell, v, area = _labelled(F32, nt=5)
    w = spatial.boxcar_weights(3)
    whole = spatial.highpass(eta, cell, w).values
    monkeypatch.setattr(hostio, "PIPELINE_ELEMS", 100)
    monkeypatch.setattr(hostio, "PIECE_ELEMS", 2 * v.shape[1] * v.shape[2])  # two steps a group
    grouped = spatial.highpass(eta, cell, w)
    assert grouped.dims == eta.dims and grouped.dtype == F32
    assert_same_bits(grouped.values, whole, "groups of two leading rows")
    assert_same_bits(whole, sn.plane_smooth(v, area, w, w, 1, 1, True, 1, False, True, F32), "highpass")
