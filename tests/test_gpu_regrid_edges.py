"""GPU: the edges of the remap -- result buffers with guard bands (tests/out_contract.py) through
the ctypes call, pointers one element off the 16-byte grid, tables whose entries point outside the
source plane or outside the table (ordinary inputs of the contract: they carry no weight), every
refusal's code and text, empty shapes.  Everything against tests/regrid_numpy.py, bit for bit."""

import numpy as np
import pytest
import torch

import regrid_numpy as rn
from momlevel_amd import _lib, core, regrid
from out_contract import Guarded
from test_gpu_regrid import (F32, F64, NSRC, TORCH, _dev, _shape, _want, assert_same_bits, make_record,
                             make_table)

pytestmark = pytest.mark.gpu

CODE = {torch.float64: _lib.DTYPE_F64, torch.float32: _lib.DTYPE_F32}


def _abi(v, packed, ndst, out, min_frac=0.0, flags=0, nsrc=None, nrec=None, out_ptr=None, odt=None):
    """mlx_regrid_apply itself, into ``out`` (any device tensor of the result's shape) or to the
    raw address ``out_ptr``"""
    sp, ln, col, S = packed
    core._call(_lib.load_regrid(), "mlx_regrid_apply", v.device, v.data_ptr(), CODE[v.dtype],
               sp.data_ptr(), ln.data_ptr(), col.data_ptr(), S.data_ptr(), S.shape[0], min_frac, flags,
               v.shape[0] if nrec is None else nrec, v.shape[1] if nsrc is None else nsrc, ndst,
               out.data_ptr() if out_ptr is None else out_ptr,
               CODE[out.dtype] if odt is None else odt)
    torch.cuda.synchronize()


def _packed(ndst):
    return regrid.pack_rows(*make_table(ndst), core.regrid_slice())


def _offset_by_one(a):
    """the same values in a device tensor that starts one element past a 16-byte boundary"""
    buf = torch.empty(a.size + 1, dtype=TORCH[a.dtype.type], device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a, order="C")))  # (a copy: the shared cases are read-only)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


# ---- result buffers with guard bands ----------------------------------------------------------------
@pytest.mark.parametrize("odt", (F64, F32), ids=("o64", "o32"))
@pytest.mark.parametrize("offset", (0, 1), ids=("aligned", "offset"))
@pytest.mark.parametrize("flags", (0, rn.PROPAGATE, rn.NO_RENORM))
def test_the_result_is_written_inside_its_buffer_and_nowhere_else(flags, offset, odt):
    """the second slice holds one destination and the second record window one record"""
    ndst, nrec = _shape()
    g = Guarded((nrec, ndst), TORCH[odt], "cuda", offset=offset)
    _abi(_dev(make_record(nrec)), [_dev(a) for a in _packed(ndst)], ndst, g.view, 0.25, flags)
    g.assert_intact(f"offset={offset} flags={flags}")
    assert g.unwritten() == 0
    assert_same_bits(g.view, _want(ndst, nrec, F64, odt, 0.25, flags), f"guarded, flags={flags}")


# ---- alignment ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odt", (F64, F32), ids=("o64", "o32"))
@pytest.mark.parametrize("vdt", (F64, F32), ids=("v64", "v32"))
def test_pointers_off_the_sixteen_byte_grid_give_the_same_bits(vdt, odt):
    ndst, nrec = _shape()
    packed = [_dev(a) for a in _packed(ndst)]
    want = _want(ndst, nrec, vdt, odt)
    v = _offset_by_one(make_record(nrec, vdt))
    out = _offset_by_one(np.zeros((nrec, ndst), dtype=odt))
    _abi(v, packed, ndst, out)
    assert_same_bits(out, want, "v and out one element off")
    aligned = torch.empty((nrec, ndst), dtype=TORCH[odt], device="cuda")
    _abi(_dev(make_record(nrec, vdt)), packed, ndst, aligned)
    assert_same_bits(aligned, want, "v and out aligned")
    # the table off the grid too: col and len by one int32, S and slice_ptr by one 8-byte element
    moved = [_offset_by_one_int(a) if a.dtype.kind == "i" else _offset_by_one(a) for a in _packed(ndst)]
    _abi(v, moved, ndst, out.zero_())
    assert_same_bits(out, want, "the table one element off")


def _offset_by_one_int(a):
    t = torch.empty(a.size + 1, dtype=torch.int64 if a.dtype == np.int64 else torch.int32, device="cuda")
    view = t[1:]
    view.copy_(torch.from_numpy(a))
    return view


# ---- entries that point outside ---------------------------------------------------------------------------
def _position(packed, d, k):
    L = core.regrid_slice()
    return int(packed[0][d // L]) + k * L + d % L


@pytest.mark.parametrize("vdt", (F64, F32), ids=("v64", "v32"))
@pytest.mark.parametrize("flags", (0, rn.PROPAGATE))
def test_entries_out_of_range_carry_no_weight(flags, vdt):
    """a col of -1, a col of nsrc and beyond, a len that runs into the next slice and one that runs
    past the table, a negative len: results by the contract (tests/regrid_numpy.py restates the
    packed table position by position), and the kernel reads nothing outside its buffers"""
    ndst, nrec = _shape()
    L = core.regrid_slice()
    sp, ln, col, S = (a.copy() for a in _packed(ndst))
    nentries = col.size
    col[_position((sp,), 3, 2)] = -1
    col[_position((sp,), 3, 5)] = NSRC
    col[_position((sp,), 3, 39)] = NSRC + 1000
    col[_position((sp,), 2, 0)] = np.iinfo(np.int32).max
    col[_position((sp,), 1, 0)] = np.iinfo(np.int32).min
    ln[10] = 41                     # one step past the first slice: an entry of the second slice
    ln[ndst - 1] = 1000             # the second slice's only row: far past the table
    ln[12] = -3
    ln[20] = np.iinfo(np.int32).max
    assert _position((sp,), ndst - 1, 999) > nentries and _position((sp,), 10, 40) < nentries
    v = make_record(nrec, vdt)
    want = rn.apply_packed(v, sp, ln, col, S, ndst, L, 0.0, flags)
    out = torch.empty((nrec, ndst), dtype=TORCH[vdt], device="cuda")
    _abi(_dev(v), [_dev(a) for a in (sp, ln, col, S)], ndst, out, 0.0, flags)
    assert_same_bits(out, want, "entries out of range")
    clean = _want(ndst, nrec, vdt, vdt, 0.0, flags)
    touched = [1, 2, 3, 10, 12, 20, ndst - 1]
    rest = np.setdiff1d(np.arange(ndst), touched)
    assert_same_bits(out[:, rest], clean[:, rest], "the other rows")
    assert np.isnan(want[:, 12]).all()
    if not flags:  # row 1's only entry and row 2's first are gone; row 3 lost three of forty
        assert np.isnan(want[:, 1]).all() and not np.isnan(want[:, 3]).any()
        assert (_bits_differ(want[:, 3], clean[:, 3])).any()
    # min_frac sees the whole weight of the entries in range only
    strict = torch.empty_like(out)
    _abi(_dev(v), [_dev(a) for a in (sp, ln, col, S)], ndst, strict, 1.0, flags)
    assert_same_bits(strict, rn.apply_packed(v, sp, ln, col, S, ndst, L, 1.0, flags), "min_frac = 1")


def _bits_differ(a, b):
    return np.ascontiguousarray(a).view(np.uint8) != np.ascontiguousarray(b).view(np.uint8)


@pytest.mark.parametrize("where", ("negative", "past the table", "the last entry"))
def test_a_slice_that_starts_outside_the_table_has_no_entries(where):
    ndst, nrec = _shape()
    L = core.regrid_slice()
    sp, ln, col, S = (a.copy() for a in _packed(ndst))
    sp[0] = {"negative": -L, "past the table": col.size, "the last entry": col.size - 1}[where]
    v = make_record(nrec)
    want = rn.apply_packed(v, sp, ln, col, S, ndst, L)
    out = torch.empty((nrec, ndst), dtype=torch.float64, device="cuda")
    _abi(_dev(v), [_dev(a) for a in (sp, ln, col, S)], ndst, out)
    assert_same_bits(out, want, where)
    assert_same_bits(out[:, L:], _want(ndst, nrec, F64, F64)[:, L:], "the other slice")
    if where != "the last entry":
        assert np.isnan(want[:, :L]).all()


# ---- refusals ------------------------------------------------------------------------------------------
def test_every_refusal_has_its_code_and_text():
    ndst, nrec = _shape()
    v = _dev(make_record(nrec))
    packed = [_dev(a) for a in _packed(ndst)]
    out = torch.full((nrec, ndst), 7.0, dtype=torch.float64, device="cuda")
    cases = [
        (dict(odt=2), "argument error -3", "dtype"),
        (dict(flags=4), "argument error -3", "flags"),
        (dict(nrec=-1), "argument error -2", "negative"),
        (dict(nsrc=1 << 31), "argument error -2", "2\\^31"),
        (dict(nrec=1 << 30, nsrc=1 << 10), "argument error -2", "2\\^38"),
        (dict(min_frac=1.5), "argument error -2", "min_frac"),
        (dict(min_frac=-0.5), "argument error -2", "min_frac"),
        (dict(min_frac=float("nan")), "argument error -2", "min_frac"),
        (dict(out_ptr=0), "argument error -1", "NULL"),
        (dict(out_ptr=out.data_ptr() + 4), "argument error -5", "aligned"),
        # an out that overlaps an operand: the record, the weights, the indices
        (dict(out_ptr=v.data_ptr()), "argument error -2", "overlaps"),
        (dict(out_ptr=v.data_ptr() + 8 * (nrec * NSRC - 1)), "argument error -2", "overlaps"),
        (dict(out_ptr=packed[3].data_ptr()), "argument error -2", "overlaps"),
        (dict(out_ptr=packed[2].data_ptr()), "argument error -2", "overlaps"),
        (dict(out_ptr=packed[1].data_ptr()), "argument error -2", "overlaps"),
        (dict(out_ptr=packed[0].data_ptr()), "argument error -2", "overlaps"),
    ]
    before = [t.clone() for t in [v] + packed]
    for kw, code, text in cases:
        with pytest.raises(_lib.MomlevelHipError, match=f"{code}.*{text}"):
            _abi(v, packed, ndst, out, **kw)
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    for t, b in zip([v] + packed, before):
        assert torch.equal(t.view(torch.int64) if t.dtype == torch.float64 else t,
                           b.view(torch.int64) if b.dtype == torch.float64 else b)
    # the Python layer refuses before the library does
    for kw in (dict(min_frac=2.0), dict(min_frac=float("nan"))):
        with pytest.raises(ValueError, match="min_frac"):
            core.regrid_apply(v, tuple(packed), NSRC, ndst, **kw)
    with pytest.raises(ValueError, match="slice_ptr"):
        core.regrid_apply(v, tuple(packed), NSRC, ndst + 64)
    with pytest.raises(ValueError, match="must be .nrec"):
        core.regrid_apply(v, tuple(packed), NSRC + 1, ndst)
    with pytest.raises(ValueError, match="col must be"):
        core.regrid_apply(v, (packed[0], packed[1], packed[2].to(torch.int64), packed[3]), NSRC, ndst)
    with pytest.raises(ValueError, match="plan_tensors"):
        core.regrid_apply(v, tuple(packed[:3]), NSRC, ndst)
    with pytest.raises(TypeError, match="out_dtype"):
        core.regrid_apply(v, tuple(packed), NSRC, ndst, out_dtype=torch.float16)
    with pytest.raises(TypeError):
        core.regrid_apply(v.to(torch.float16), tuple(packed), NSRC, ndst)
    with pytest.raises(ValueError, match="contiguous"):
        core.regrid_apply(v.t().contiguous().t(), tuple(packed), NSRC, ndst)


def test_an_out_that_only_touches_the_record_is_accepted():
    ndst, nrec = _shape()
    buf = torch.empty(nrec * NSRC + nrec * ndst, dtype=torch.float64, device="cuda")
    v, out = buf[:nrec * NSRC].view(nrec, NSRC), buf[nrec * NSRC:].view(nrec, ndst)
    v.copy_(_dev(make_record(nrec)))
    _abi(v, [_dev(a) for a in _packed(ndst)], ndst, out)
    assert_same_bits(out, _want(ndst, nrec, F64, F64), "out directly behind v")
    assert_same_bits(v, make_record(nrec), "the record is untouched")


# ---- empty shapes ------------------------------------------------------------------------------------------
def test_empty_shapes():
    ndst, nrec = _shape()
    packed = tuple(_dev(a) for a in _packed(ndst))
    none = core.regrid_apply(torch.empty((0, NSRC), dtype=torch.float32, device="cuda"), packed, NSRC, ndst)
    assert none.shape == (0, ndst) and none.dtype == torch.float32 and none.is_cuda
    empty = tuple(_dev(a) for a in regrid.pack_rows(np.zeros(1, dtype=np.int64), [], [], 64))
    v = _dev(make_record(nrec))
    nothing = core.regrid_apply(v, empty, NSRC, 0, out_dtype=torch.float32)
    assert nothing.shape == (nrec, 0) and nothing.dtype == torch.float32
    # the library itself: 0 without a launch, whatever the pointers
    lib = _lib.load_regrid()
    for kw in (dict(nrec=0), dict(ndst=0)):
        a = dict(dict(nrec=nrec, ndst=ndst), **kw)
        assert lib.mlx_regrid_apply(None, _lib.DTYPE_F64, None, None, None, None, 0, 0.0, 0, a["nrec"],
                                    NSRC, a["ndst"], None, _lib.DTYPE_F64, None) == 0
    # a table without a single entry: every destination NaN
    bare = tuple(_dev(a) for a in regrid.pack_rows(np.zeros(ndst + 1, dtype=np.int64), [], [], 64))
    got = core.regrid_apply(v, bare, NSRC, ndst)
    assert_same_bits(got, np.full((nrec, ndst), rn.NAN64), "no entries")
    # and a record on an empty source plane
    hollow = core.regrid_apply(torch.empty((nrec, 0), dtype=torch.float64, device="cuda"),
                               tuple(_dev(a) for a in _packed(ndst)), 0, ndst)
    assert_same_bits(hollow, np.full((nrec, ndst), rn.NAN64), "nsrc == 0: every col is out of range")
