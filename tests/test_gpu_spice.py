"""GPU: spice.flament.spice, derived.calc_spice and mlx_spice_map (csrc/momlevel_spice.hip) against
the reference's vectors (tests/golden/spice_vectors.npz) within the parity bounds of
tests/spice_numpy.py, and the kernel's own invariants bit for bit: a cell's value depends on its
two operands only -- not on its position, the alignment of the pointers, the vector path or n."""

import numpy as np
import pytest
import torch

import spice_numpy as sn
from conftest import assert_bit_equal
from momlevel_amd import _lib, core, derived
from momlevel_amd.labeled import DataArray
from momlevel_amd.spice.flament import spice
from momlevel_amd.test_data import generate_test_data

pytestmark = pytest.mark.gpu

DTYPES = {"f64": (torch.float64, torch.float64), "f32": (torch.float32, torch.float32),
          "t32s64": (torch.float32, torch.float64), "t64s32": (torch.float64, torch.float32)}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.view(torch.int64), b.view(torch.int64)))


def _gate(name, got, T, S, ref):
    """print the worst error of a vector in units of its bound, then assert the bound cell by cell"""
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == ref.shape, name
    ok = ~np.isnan(ref)
    assert np.array_equal(np.isnan(got), ~ok), f"{name}: NaN placement"
    lim = sn.bound(T, S)
    err = np.abs(got[ok] - ref[ok])
    print(f"{name:24s} worst |kernel - reference| / bound = {np.max(err / lim[ok]):.4f}   "
          f"(bound {'10 * 2^-24' if np.float32 in (T.dtype, S.dtype) else '64 * 2^-53'} A, "
          f"{int(ok.sum())} cells)")
    assert np.all(err <= lim[ok]), name


# ---- values ---------------------------------------------------------------------------------------
def test_every_vector_within_the_bounds():
    vec, gold = sn.fixture()
    for name, (T, S, ref) in vec.items():
        got = spice(T, S)
        assert type(got) is np.ndarray
        _gate(f"spice() {name}", got, T, S, ref)
        Td, Sd = (_dev(x.astype(np.float64) if x.dtype.kind in "iu" else x).reshape(-1) for x in (T, S))
        raw = core.spice_map(Td, Sd)
        assert raw.dtype == torch.float64 and raw.is_cuda and raw.shape == (T.size,)
        _gate(f"core.spice_map {name}", raw.cpu().numpy().reshape(T.shape), T, S, ref)
        assert_bit_equal(raw.cpu().numpy().reshape(T.shape), got, name)
    T, S, ref = vec["grid"]
    total = spice(T, S).sum()
    tol = sn.bound(T, S).sum() + 2.0 * (np.log2(ref.size) + 8.0) * 2.0 ** -53 * np.abs(ref).sum()
    print("sum over the reference's grid:", repr(total), "pinned:", repr(gold["grid_sum"]),
          "difference", abs(total - gold["grid_sum"]), "tolerance", tol)
    assert np.allclose(total, gold["grid_sum"])  # the reference's own assertion
    assert abs(total - gold["grid_sum"]) <= tol  # the cells' bounds and two pairwise sums


def test_nan_placement_and_the_finite_cells_beside_them():
    vec, _ = sn.fixture()
    for name in ("nan", "nan_f32"):
        T, S, ref = vec[name]
        got = spice(T, S)
        assert np.array_equal(np.isnan(got), np.isnan(T) | np.isnan(S))
        ok = ~np.isnan(ref)
        # the finite cells are the cells of a call that never saw a NaN
        alone = spice(np.ascontiguousarray(T[ok]), np.ascontiguousarray(S[ok]))
        assert_bit_equal(got[ok], alone, name)
        _gate(name, got, T, S, ref)


# ---- position independence, exact -----------------------------------------------------------------
N_BIG = (1 << 20) + 3
SIZES = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 4099)


@pytest.fixture(scope="module")
def big():
    """one random vector of 2^20 + 3 cells in float64 and rounded to float32, evaluated once per
    dtype pairing: {pairing: (theta, S, pi)} on the device"""
    rng = np.random.default_rng(54493501)
    T64, S64 = rng.uniform(-2.0, 32.0, N_BIG), rng.uniform(0.0, 42.0, N_BIG)
    out = {}
    for name, (dt, ds) in DTYPES.items():
        T, S = _dev(T64).to(dt), _dev(S64).to(ds)
        out[name] = (T, S, core.spice_map(T, S))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("pairing", list(DTYPES))
def test_views_and_prefixes_are_slices_of_the_whole(big, pairing):
    T, S, whole = big[pairing]
    assert whole.dtype == torch.float64 and not bool(torch.isnan(whole).any())
    m = max(SIZES)
    shifted = torch.empty(m + 4, dtype=S.dtype, device="cuda")
    outbuf = torch.empty(m + 2, dtype=torch.float64, device="cuda")
    bad = []
    for oT in range(4):
        for oS in range(4):
            shifted[oS:oS + m] = S[oT:oT + m]  # S of the cells oT.. at an offset of its own
            for oO in range(2):
                for n in SIZES:
                    out = outbuf[oO:oO + n]
                    got = core.spice_map(T[oT:oT + n], shifted[oS:oS + n], out=out)
                    assert got.data_ptr() == out.data_ptr()
                    if not _same_bits(got, whole[oT:oT + n]):
                        bad.append((oT, oS, oO, n))
    print(f"{pairing}: {4 * 4 * 2 * len(SIZES)} offset views (theta, S, out offsets x n), "
          f"{len(bad)} differ from the slice of the whole")
    assert not bad, bad[:8]
    for n in SIZES + (N_BIG - 1, N_BIG - 2, N_BIG - 3):  # prefixes
        assert _same_bits(core.spice_map(T[:n], S[:n]), whole[:n]), n


@pytest.mark.parametrize("pairing", list(DTYPES))
def test_thousands_of_tiles_give_the_same_cells(big, pairing):
    """six copies of the vector in a row -- 3073 to 12289 tiles with a ragged last one -- on the
    cell-by-cell path (theta one element into its allocation) and on the packed one"""
    T, S, whole = big[pairing]
    T6 = torch.cat([T[:1]] + [T] * 6)[1:]  # a view that starts one element into its allocation
    S6 = torch.cat([S] * 6)
    for theta in (T6, T6.clone()):
        got = core.spice_map(theta, S6)
        assert _same_bits(got, torch.cat([whole] * 6))


def test_two_runs_agree_and_nothing_is_empty(big):
    for name, (T, S, whole) in big.items():
        assert _same_bits(core.spice_map(T, S), whole), name
    empty = core.spice_map(torch.empty(0, dtype=torch.float32, device="cuda"),
                           torch.empty(0, dtype=torch.float64, device="cuda"))
    assert empty.shape == (0,) and empty.dtype == torch.float64
    got = spice(np.empty((0, 3)), np.empty((0, 3), dtype=np.float32))
    assert type(got) is np.ndarray and got.shape == (0, 3) and got.dtype == np.float64


def test_argument_errors_launch_nothing():
    lib = _lib.load_spice()
    T = torch.ones(16, dtype=torch.float64, device="cuda")
    S = torch.full((16,), 35.0, dtype=torch.float64, device="cuda")
    out = torch.full((16,), -7.0, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    F64, F32 = _lib.DTYPE_F64, _lib.DTYPE_F32
    t, s, o = T.data_ptr(), S.data_ptr(), out.data_ptr()
    calls = {
        "theta NULL": ((None, F64, s, F64, 16, o), -1), "so NULL": ((t, F64, None, F64, 16, o), -1),
        "out NULL": ((t, F64, s, F64, 16, None), -1), "n < 0": ((t, F64, s, F64, -16, o), -2),
        "n too large": ((t, F64, s, F64, (1 << 38) + 1, o), -2),
        "theta dtype": ((t, 2, s, F64, 16, o), -3), "so dtype": ((t, F64, s, 9, 16, o), -3),
        "theta alignment": ((t + 4, F64, s, F64, 8, o), -5),
        "so alignment": ((t, F64, s + 2, F32, 8, o), -5), "out alignment": ((t, F64, s, F64, 8, o + 4), -5),
    }
    for what, (args, code) in calls.items():
        rc = lib.mlx_spice_map(*args, st)
        print(f"{what:16s} -> {rc}: {_lib.last_error()}")
        assert rc == code and _lib.last_error(), what
    assert lib.mlx_spice_map(t, F64, s, F64, 0, o, st) == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())  # nothing ran
    for bad in (dict(theta=T.cpu()), dict(so=S.half()), dict(theta=T.reshape(4, 4)), dict(so=S[:8]),
                dict(theta=T[::2], so=S[::2]), dict(out=out.float()), dict(out=out[:8])):
        kw = dict(theta=T, so=S, out=None)
        kw.update(bad)
        with pytest.raises((TypeError, ValueError)):
            core.spice_map(**kw)


# ---- placement and shapes -------------------------------------------------------------------------
def test_placement_shapes_and_dtypes():
    rng = np.random.default_rng(7)
    T = rng.uniform(-2.0, 32.0, (3, 4, 5, 7))
    S = rng.uniform(30.0, 40.0, (3, 4, 5, 7))
    ref = spice(T, S)
    assert type(ref) is np.ndarray and ref.shape == T.shape and ref.dtype == np.float64
    _gate("4-D host", ref, T, S, sn.horner(T, S))  # (the restatement is within 20 u A of the kernel)
    dev = spice(_dev(T), _dev(S))
    assert isinstance(dev, torch.Tensor) and dev.device == torch.device("cuda", torch.cuda.current_device())
    assert dev.shape == T.shape and dev.dtype == torch.float64
    assert_bit_equal(dev.cpu().numpy(), ref)
    mixed = spice(_dev(T), S)  # one operand on the device: the result stays there
    assert isinstance(mixed, torch.Tensor) and mixed.is_cuda
    assert_bit_equal(mixed.cpu().numpy(), ref)
    f32 = spice(_dev(T.astype(np.float32)), _dev(S.astype(np.float32)))
    assert f32.dtype == torch.float64
    assert_bit_equal(f32.cpu().numpy(), spice(T.astype(np.float32).astype(np.float64),
                                              S.astype(np.float32).astype(np.float64)))
    # python scalars (np.float64 is a float): shape (1,)
    for a, b in ((10.0, 35.0), (10, 35), (np.float64(10.0), 35), (True, 35.5)):
        one = spice(a, b)
        assert type(one) is np.ndarray and one.shape == (1,) and one.dtype == np.float64
        assert_bit_equal(one, spice(np.array([float(a)]), np.array([float(b)])))
    # no broadcasting at this level
    for a, b in ((T, S[0]), (T, S[..., :1]), (T.reshape(-1), S), (10.0, S), (_dev(T), _dev(S[0]))):
        with pytest.raises(AssertionError, match="thetao and so must have the same shape"):
            spice(a, b)
    for a, b in ((T.astype(np.float16), S), (T, S.astype(np.longdouble)), (_dev(T).half(), _dev(S))):
        with pytest.raises(TypeError):
            spice(a, b)
    # a masked array means NaN where it is masked; integers and booleans compute as float64
    from lazy_array import as_masked

    Tn, Sn = T.copy(), S.copy()
    Tn[0, 1, 2, :] = np.nan
    Sn[2, :, 0, 3] = np.nan
    filled = spice(Tn, Sn)
    assert np.isnan(filled).sum() == 7 + 4
    assert_bit_equal(spice(as_masked(Tn), as_masked(Sn)), filled)
    assert_bit_equal(spice(as_masked(Tn.astype(np.float32)), Sn), spice(Tn.astype(np.float32), Sn))
    Ti = rng.integers(-2, 33, T.shape).astype(np.int32)
    assert_bit_equal(spice(Ti, S), spice(Ti.astype(np.float64), S))
    assert_bit_equal(spice(_dev(Ti), _dev(S)).cpu().numpy(), spice(Ti.astype(np.float64), S))
    Sb = S > 35.0
    assert_bit_equal(spice(T, Sb), spice(T, Sb.astype(np.float64)))
    assert_bit_equal(spice(np.asfortranarray(T), S[::-1][::-1]), ref)  # any memory layout


def test_the_host_pipeline_walks_pieces(monkeypatch):
    from lazy_array import CountingLazy, MaskedLazy
    from momlevel_amd import hostio

    rng = np.random.default_rng(11)
    shape = (6, 5, 9, 11)
    T = rng.uniform(-2.0, 32.0, shape)
    S = rng.uniform(30.0, 40.0, shape).astype(np.float32)
    T[1, 2, 3, :] = np.nan
    whole = spice(T, S)
    lazyT = CountingLazy(T)
    assert_bit_equal(spice(lazyT, S), whole)  # small: read in one piece
    assert len(lazyT.reads) == 1

    pieces = []
    real = hostio.Uploader.submit

    def counting(self, arrays):
        pieces.append([tuple(a.shape) for a in arrays])
        return real(self, arrays)

    monkeypatch.setattr(hostio.Uploader, "submit", counting)
    monkeypatch.setattr(hostio, "PIPELINE_ELEMS", 1000)
    monkeypatch.setattr(hostio, "PIECE_ELEMS", 2 * 5 * 9 * 11)  # two rows of the leading axis a piece
    got = spice(T, S)
    assert type(got) is np.ndarray and got.dtype == np.float64
    assert_bit_equal(got, whole)
    assert pieces == [[(2, 5, 9, 11)] * 2] * 3
    pieces.clear()
    lazyT, lazyS = MaskedLazy(T), CountingLazy(S)
    assert_bit_equal(spice(lazyT, lazyS), whole)
    assert len(pieces) == 3 and len(lazyT.reads) == 3 and len(lazyS.reads) == 3
    assert lazyT.largest_read == 2 * 5 * 9 * 11 * 8 and lazyS.largest_read == 2 * 5 * 9 * 11 * 4
    pieces.clear()
    Ti = np.nan_to_num(T).astype(np.int32)  # integers travel as float64
    assert_bit_equal(spice(Ti, S), spice(Ti.astype(np.float64), S))
    assert len(pieces) == 6


# ---- calc_spice on labelled arrays ----------------------------------------------------------------
dset1 = generate_test_data()
ATTRS = {"long_name": "Sea water spiciness", "comment": "calculated based on Flament 2002 methodology",
         "units": "1"}


def test_calc_spice():
    pi = derived.calc_spice(dset1.thetao, dset1.so)
    assert isinstance(pi, DataArray) and pi.dims == dset1.thetao.dims == ("time", "z_l", "yh", "xh")
    assert pi.attrs == ATTRS and list(pi.attrs) == list(ATTRS)
    assert set(pi.coords) == set(dset1.thetao.coords)
    assert pi.values.dtype == np.float64
    assert_bit_equal(pi.values, spice(dset1.thetao.values, dset1.so.values))
    _gate("calc_spice", pi.values, dset1.thetao.values, dset1.so.values,
          sn.horner(dset1.thetao.values, dset1.so.values))


def test_calc_spice_broadcasts_by_dimension_name():
    so3 = dset1.so.isel(time=0)
    assert so3.dims == ("z_l", "yh", "xh")
    pi = derived.calc_spice(dset1.thetao, so3)
    assert pi.dims == ("time", "z_l", "yh", "xh") and pi.shape == dset1.thetao.shape
    assert pi.attrs == ATTRS
    for name in ("time", "z_l", "yh", "xh"):
        assert np.array_equal(np.asarray(pi.coords[name].values), np.asarray(dset1.thetao.coords[name].values))
    expanded = np.ascontiguousarray(np.broadcast_to(so3.values, dset1.thetao.shape))
    assert_bit_equal(pi.values, spice(dset1.thetao.values, expanded))
    # output dims in first-appearance order: the 3-D field first, then time
    rev = derived.calc_spice(so3, dset1.thetao)
    assert rev.dims == ("z_l", "yh", "xh", "time")
    assert_bit_equal(rev.values, spice(np.ascontiguousarray(np.broadcast_to(so3.values[..., None], rev.shape)),
                                       np.ascontiguousarray(np.moveaxis(dset1.thetao.values, 0, -1))))
    # device-resident fields stay on the device
    devT = DataArray(_dev(dset1.thetao.values), dset1.thetao.dims, dict(dset1.thetao.coords))
    devS = DataArray(_dev(so3.values), so3.dims, dict(so3.coords))
    dpi = derived.calc_spice(devT, devS)
    assert dpi.is_device and dpi.dims == pi.dims
    assert_bit_equal(dpi.values, pi.values)


def test_calc_spice_on_lazy_fields(monkeypatch):
    from lazy_array import CountingLazy
    from momlevel_amd import hostio

    ref = derived.calc_spice(dset1.thetao, dset1.so).values
    monkeypatch.setattr(hostio, "PIPELINE_ELEMS", 100)
    monkeypatch.setattr(hostio, "PIECE_ELEMS", 2 * 125)  # two time steps a piece
    lazy = CountingLazy(dset1.thetao.values)
    pi = derived.calc_spice(DataArray(lazy, dset1.thetao.dims, dict(dset1.thetao.coords)), dset1.so)
    assert_bit_equal(pi.values, ref)
    assert lazy.largest_read == 2 * 125 * 8 and len(lazy.reads) == 3
    so3 = dset1.so.isel(time=0)
    lazy = CountingLazy(dset1.thetao.values)
    pi = derived.calc_spice(DataArray(lazy, dset1.thetao.dims, dict(dset1.thetao.coords)), so3)
    assert_bit_equal(pi.values, derived.calc_spice(dset1.thetao, so3).values)
    assert lazy.largest_read == 2 * 125 * 8


def test_calc_spice_answers_xarray_in_kind(monkeypatch):
    import fake_xarray
    from momlevel_amd import adapters

    monkeypatch.setattr(adapters, "xr", fake_xarray)
    x = adapters.to_xarray(dset1)
    pi = derived.calc_spice(x["thetao"], x["so"])
    assert isinstance(pi, fake_xarray.DataArray) and pi.dims == ("time", "z_l", "yh", "xh")
    assert dict(pi.attrs) == ATTRS and "z_l" in pi.coords
    assert_bit_equal(np.asarray(pi.values), derived.calc_spice(dset1.thetao, dset1.so).values)
