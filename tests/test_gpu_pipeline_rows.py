"""GPU: hostio.pipeline_rows, the one loop behind the piecewise EOS / spice, stratification,
vorticity and area paths, on its own.  The "kernel" is a torch expression on small whole numbers,
so every expected value is exact in float64 and every comparison is bit for bit."""

import threading

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal
from lazy_array import CountingLazy, MaskedLazy
from momlevel_amd import hostio

pytestmark = pytest.mark.gpu

TAIL = (3, 7)  # 21 elements a leading row
PER_ROW = 21
A = np.arange(5 * PER_ROW, dtype=np.float64).reshape((5,) + TAIL)
STARTS = np.array([0, 0, 2, 2, 4], dtype=np.float64)[:, None, None]  # i0 of the group of every row


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _run(sources, kernel, nlead=5, per_row=PER_ROW, out=None):
    out = np.empty((nlead,) + TAIL, dtype=np.float64) if out is None else out
    return hostio.pipeline_rows(hostio.row_bounds(nlead, per_row), _device(),
                                hostio.leading_slices(sources), kernel, out)


@pytest.fixture
def submits(monkeypatch):
    """the shapes of every group the Uploader is handed"""
    seen = []
    real = hostio.Uploader.submit

    def counting(self, arrays):
        arrays = list(arrays)
        seen.append([tuple(a.shape) for a in arrays])
        return real(self, arrays)

    monkeypatch.setattr(hostio.Uploader, "submit", counting)
    return seen


def _workers():
    """the transfer worker threads alive now (an earlier test's steric call may have left its own)"""
    return {t.ident for t in threading.enumerate() if t.name.startswith(("mlx-upload", "mlx-download"))}


def test_ragged_tail_of_groups(monkeypatch, submits):
    monkeypatch.setattr(hostio, "PIECE_ELEMS", 2 * PER_ROW)  # two rows a group
    calls, before = [], _workers()

    def kernel(tensors, i0, i1):
        calls.append((i0, i1, tuple(tensors[0].shape), tensors[0].is_cuda))
        return 2 * tensors[0] + i0

    out = np.empty(A.shape, dtype=np.float64)
    got = _run([A], kernel, out=out)
    assert got is out
    assert calls == [(0, 2, (2,) + TAIL, True), (2, 4, (2,) + TAIL, True), (4, 5, (1,) + TAIL, True)]
    assert submits == [[(2,) + TAIL], [(2,) + TAIL], [(1,) + TAIL]]
    assert_bit_equal(got, 2 * A + STARTS)
    assert _workers() <= before


@pytest.mark.parametrize("piece", [5 * PER_ROW, 5 * PER_ROW + 1, 1 << 25])
def test_one_group_submits_one_upload(monkeypatch, submits, piece):
    monkeypatch.setattr(hostio, "PIECE_ELEMS", piece)  # at or above the leading count
    calls = []
    got = _run([A], lambda t, i0, i1: calls.append((i0, i1)) or 2 * t[0] + i0)
    assert calls == [(0, 5)] and submits == [[(5,) + TAIL]]
    assert_bit_equal(got, 2 * A)


def test_a_row_larger_than_a_piece_goes_alone(monkeypatch, submits):
    monkeypatch.setattr(hostio, "PIECE_ELEMS", PER_ROW - 1)
    calls = []
    got = _run([A], lambda t, i0, i1: calls.append((i0, i1)) or 2 * t[0] + i0)
    assert calls == [(i, i + 1) for i in range(5)] and len(submits) == 5
    assert_bit_equal(got, 2 * A + np.arange(5.0)[:, None, None])


def test_sources_arrive_in_order_in_the_uploaders_dtypes(monkeypatch):
    monkeypatch.setattr(hostio, "PIECE_ELEMS", 2 * PER_ROW)
    a32, a64, i16 = A.astype(np.float32), A + 1000.0, (A % 7).astype(np.int16)
    dtypes, asked = [], []

    def kernel(tensors, i0, i1):
        dtypes.append([t.dtype for t in tensors])
        return tensors[0] + tensors[1] + 3 * tensors[2]  # (float32 + float64: float64)

    def allocate(dtype):  # `out` from the first result's dtype, once
        asked.append(dtype)
        return np.empty(A.shape, dtype=np.float64)

    got = _run([a32, a64, i16], kernel, out=allocate)
    assert dtypes == [[torch.float32, torch.float64, torch.float64]] * 3  # (integers travel as float64)
    assert asked == [torch.float64]
    assert got.dtype == np.float64
    assert_bit_equal(got, A + (A + 1000.0) + 3 * (A % 7))
    # a float32 result lands in a float32 array
    got = _run([a32], lambda t, i0, i1: 2 * t[0],
               out=lambda dtype: np.empty(A.shape, dtype=np.float32 if dtype == torch.float32 else np.float64))
    assert got.dtype == np.float32
    assert_bit_equal(got, (2 * A).astype(np.float32))


def test_a_lazy_source_is_read_group_by_group(monkeypatch):
    monkeypatch.setattr(hostio, "PIECE_ELEMS", 2 * PER_ROW)
    lazy = CountingLazy(A)
    got = _run([lazy], lambda t, i0, i1: 2 * t[0] + i0)
    assert_bit_equal(got, 2 * A + STARTS)
    assert len(lazy.reads) == 3 and lazy.largest_read == 2 * PER_ROW * 8


def test_masked_cells_of_a_lazy_source_arrive_as_nan(monkeypatch):
    monkeypatch.setattr(hostio, "PIECE_ELEMS", 2 * PER_ROW)
    holes = A.copy()
    holes[0, 1, 2] = holes[3, 0, :] = holes[4, 2, 6] = np.nan
    lazy = MaskedLazy(holes)  # (its slices hold the fill value, 1e20, under the mask -- never NaN)
    got = _run([lazy], lambda t, i0, i1: 2 * t[0] + i0)
    assert_bit_equal(got, 2 * holes + STARTS)
    assert int(np.isnan(got).sum()) == 1 + TAIL[1] + 1 and len(lazy.reads) == 3


def _check_an_ordinary_call_after(before):
    assert _workers() <= before  # the failed call's workers are gone
    assert_bit_equal(_run([A], lambda t, i0, i1: 2 * t[0] + i0), 2 * A + STARTS)


def test_a_kernel_that_raises_on_the_host_ends_the_call(monkeypatch):
    """a python exception in ``kernel`` on the second of three groups, before anything is launched
    for that group: it comes out of the call as it is, the workers are shut down, and the next call
    is an ordinary one"""
    monkeypatch.setattr(hostio, "PIECE_ELEMS", 2 * PER_ROW)
    calls, before = [], _workers()

    def kernel(tensors, i0, i1):
        calls.append(i0)
        if i0 == 2:
            raise ValueError("the caller's kernel refuses rows 2..3")
        return 2 * tensors[0] + i0

    with pytest.raises(ValueError, match="refuses rows"):
        _run([A], kernel)
    assert calls == [0, 2]
    _check_an_ordinary_call_after(before)


class _FailingLazy(CountingLazy):
    def __getitem__(self, key):
        if len(self.reads) == 1:
            self.reads.append(0)
            raise OSError("the file went away under the second read")
        return super().__getitem__(key)


def test_a_read_that_raises_in_the_upload_worker_ends_the_call(monkeypatch):
    """the same for a lazy source whose SECOND read fails: the error travels from the upload worker
    to the caller through the group's future"""
    monkeypatch.setattr(hostio, "PIECE_ELEMS", 2 * PER_ROW)
    lazy = _FailingLazy(A)
    calls, before = [], _workers()
    with pytest.raises(OSError, match="second read"):
        _run([lazy], lambda t, i0, i1: calls.append(i0) or 2 * t[0] + i0)
    assert calls == [0] and len(lazy.reads) == 2
    _check_an_ordinary_call_after(before)
