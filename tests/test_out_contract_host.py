"""The result-buffer contract of momlevel_amd/core.py on the host: ``_out_like`` and
``_no_overlap`` are pure functions of tensor metadata (shape, dtype, device, strides, data_ptr),
so CPU tensors exercise every branch; and the guard-band helper of tests/out_contract.py must
report a flipped element before the view, after it and in a stride gap, each with its offset.
No GPU, no library."""

import pytest
import torch

import out_contract as oc
from momlevel_amd import core

F64, F32 = torch.float64, torch.float32


def _refused(outputs, operands=(), names=()):
    with pytest.raises(ValueError) as err:
        core._no_overlap(outputs, operands)
    for name in names:
        assert name in str(err.value), str(err.value)


# ---- _no_overlap ----------------------------------------------------------------------------------
def test_identical_tensor_is_refused_and_both_arguments_are_named():
    x = torch.zeros(8, dtype=F64)
    _refused([("out", x)], [("u", x)], names=("out", "u"))
    _refused([("eta_out", x)], [("thetao", torch.zeros(3)), ("so", x.view(2, 4))],
             names=("eta_out", "so"))


def test_one_shared_element_at_either_end_is_refused():
    buf = torch.zeros(32, dtype=F64)
    operand = buf[8:16]
    _refused([("out", buf[15:23])], [("x", operand)])  # starts on the operand's last element
    _refused([("out", buf[1:9])], [("x", operand)])  # ends on the operand's first element
    _refused([("out", buf[10:12])], [("x", operand)])  # inside it
    _refused([("out", buf[0:32])], [("x", operand)])  # around it


def test_touching_and_disjoint_ranges_are_accepted():
    buf = torch.zeros(32, dtype=F64)
    operand = buf[8:16]
    core._no_overlap([("out", buf[16:24])], [("x", operand)])  # touches its end
    core._no_overlap([("out", buf[0:8])], [("x", operand)])  # touches its start
    core._no_overlap([("out", buf[20:24])], [("x", operand)])
    core._no_overlap([("out", torch.zeros(8, dtype=F64))], [("x", operand), ("none", None)])


def test_views_of_one_storage_in_two_dtypes_compare_in_bytes():
    buf = torch.zeros(16, dtype=F64)
    as32 = buf.view(F32)  # 32 float32
    _refused([("out", buf[4:8])], [("x", as32[15:16])])  # the second half of buf[7]
    _refused([("out", as32[8:9])], [("x", buf[4:8])])  # the first half of buf[4]
    core._no_overlap([("out", buf[4:8])], [("x", as32[16:20])])  # from byte 64 on: touching
    core._no_overlap([("out", buf[4:8])], [("x", as32[0:8])])  # up to byte 32: touching


def test_an_empty_tensor_overlaps_nothing():
    buf = torch.zeros(16, dtype=F64)
    core._no_overlap([("out", buf[4:4])], [("x", buf)])
    core._no_overlap([("out", buf)], [("x", buf[4:4])])
    core._no_overlap([("out", buf[:0]), ("eta_out", buf[:0])])


def test_two_outputs_of_one_call_are_checked_against_each_other():
    buf = torch.zeros(32, dtype=F64)
    _refused([("delta_rho_out", buf[0:16]), ("eta_out", buf[15:20])],
             names=("delta_rho_out", "eta_out"))
    core._no_overlap([("delta_rho_out", buf[0:16]), ("eta_out", buf[16:20])])


def test_a_strided_variant_view_covers_its_gaps():
    """full[:, t0:t1] of a (3, nt, field) tensor: the kernel addresses (3 - 1) * stride(0) + field
    elements from the first, so an operand in the gap between two variants is refused, and one
    just past the last variant's field is not"""
    nt, field = 6, 5
    full = torch.zeros(3 * nt * field + 10, dtype=F64)
    variants = full[:3 * nt * field].view(3, nt, field)
    out = variants[:, 1:3]
    assert not out.is_contiguous() and out.stride(0) == nt * field
    first = out.data_ptr()
    last = first + ((3 - 1) * out.stride(0) + 2 * field) * 8
    assert core._extent(out) == (first, last)
    gap = variants[0, 4]  # between variant 0's and variant 1's steps 1:3
    _refused([("eta_out", out)], [("rho0m", gap)], names=("eta_out", "rho0m"))
    _refused([("out", gap)], [("x", out)])  # and as the operand of another output
    core._no_overlap([("eta_out", out)], [("rho0m", variants[2, 3])])  # past the last field
    core._no_overlap([("eta_out", out)], [("rho0m", variants[0, 0])])  # before the first
    assert core._extent(torch.zeros(4, 6, dtype=F32)[1:3]) is not None
    x = torch.zeros(4, 6, dtype=F32)
    assert core._extent(x) == (x.data_ptr(), x.data_ptr() + 4 * 6 * 4)  # contiguous: numel


# ---- _out_like --------------------------------------------------------------------------------------
CPU = torch.device("cpu")


def test_out_like_returns_a_matching_buffer_itself_and_allocates_for_none():
    out = torch.zeros(2, 3, 4, dtype=F64)
    assert core._out_like(out, (2, 3, 4), F64, CPU) is out
    new = core._out_like(None, (2, 3, 4), F32, "cpu")
    assert tuple(new.shape) == (2, 3, 4) and new.dtype == F32 and new.is_contiguous()


@pytest.mark.parametrize("shape", [(2, 3, 3), (2, 2, 4), (1, 3, 4), (2, 3, 5), (3, 2, 4), (4, 3, 2),
                                   (24,), (2, 12), (2, 3, 4, 1), ()])
def test_out_like_refuses_every_other_shape(shape):
    """one short or long along each axis, and the same numel in another shape or rank"""
    with pytest.raises(ValueError, match="out must be a contiguous"):
        core._out_like(torch.zeros(shape, dtype=F64), (2, 3, 4), F64, CPU)


def test_out_like_refuses_the_other_dtype_and_names_the_argument():
    with pytest.raises(ValueError, match="eta_out must be a contiguous float64"):
        core._out_like(torch.zeros(2, 3, dtype=F32), (2, 3), F64, CPU, "float64", name="eta_out")
    with pytest.raises(ValueError):
        core._out_like(torch.zeros(2, 3, dtype=F64), (2, 3), F32, CPU)
    with pytest.raises(ValueError):
        core._out_like(torch.zeros(2, 3, dtype=torch.int64), (2, 3), F64, CPU)
    with pytest.raises(ValueError):
        core._out_like([[0.0] * 3] * 2, (2, 3), F64, CPU)  # not a tensor at all


def test_out_like_refuses_non_contiguous_views_of_the_right_shape():
    wide = torch.zeros(4, 6, dtype=F64)
    for view in (wide[:, ::2], torch.zeros(3, 4, dtype=F64).T, wide[:, :3]):
        assert tuple(view.shape) == (4, 3) and not view.is_contiguous()
        with pytest.raises(ValueError):
            core._out_like(view, (4, 3), F64, CPU)


def test_out_like_refuses_a_tensor_of_another_device():
    host = torch.zeros(2, 3, dtype=F64)
    with pytest.raises(ValueError, match="cuda:0"):
        core._out_like(host, (2, 3), F64, torch.device("cuda", 0))
    with pytest.raises(ValueError):
        core._out_like(torch.zeros(2, 3, dtype=F64, device="meta"), (2, 3), F64, CPU)


# ---- the guard-band helper ------------------------------------------------------------------------------
def _flip(g, offset):
    """one element of the buffer, ``offset`` elements from the view's first, gets another value"""
    g.buf[g.start + offset] = 1.0


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("offset", [0, 1])
def test_guard_reports_an_element_before_and_after_the_view(dtype, offset):
    g = oc.Guarded((3, 5), dtype, offset=offset)
    assert g.view.is_contiguous() and tuple(g.view.shape) == (3, 5) and g.span == 15
    assert g.view.data_ptr() % 16 == offset * g.view.element_size()
    assert g.buf.numel() == 2 * oc.GUARD + offset + 15
    assert g.changed() == [] and g.unwritten() == 15
    g.view.fill_(2.0)  # a full, in-bounds result leaves every guard alone
    assert g.changed() == [] and g.unwritten() == 0
    g.assert_intact()
    _flip(g, -1)
    assert g.changed() == [-1]
    _flip(g, 15)
    assert g.changed() == [-1, 15]
    _flip(g, -oc.GUARD - offset)  # the buffer's first and last elements
    _flip(g, 15 + oc.GUARD - 1)
    assert g.changed() == [-oc.GUARD - offset, -1, 15, 15 + oc.GUARD - 1]
    with pytest.raises(AssertionError, match=r"4 element\(s\).*-1, 15"):
        g.assert_intact("case")


def test_guard_reports_an_element_in_a_stride_gap():
    """the (3, nt, field) variants' steps 1:3: the steps outside belong to the guard"""
    nt, field = 6, 5
    g = oc.Guarded((3, 2, field), F64, strides=(nt * field, field, 1))
    assert g.span == 2 * nt * field + 2 * field and not g.view.is_contiguous()
    g.view.fill_(3.0)
    assert g.changed() == [] and g.unwritten() == 0
    _flip(g, 2 * field)  # the first element past variant 0's steps
    _flip(g, nt * field - 1)  # the last element before variant 1's
    _flip(g, nt * field + 2 * field + 3)
    assert g.changed() == [2 * field, nt * field - 1, nt * field + 2 * field + 3]
    g.view[1, 0, 0] = float("nan")  # a NaN the kernel stored is not the sentinel
    assert g.unwritten() == 0


def test_the_sentinel_is_a_quiet_nan_with_a_payload():
    for dtype, canonical in ((F64, 0x7FF8000000000000), (F32, 0x7FC00000)):
        g = oc.Guarded((1,), dtype, guard=4)
        assert torch.isnan(g.buf).all()
        assert oc.SENTINEL[dtype] & canonical == canonical and oc.SENTINEL[dtype] != canonical
        assert g.unwritten() == 1
        g.view.fill_(float("nan"))
        assert g.unwritten() == 0 and g.changed() == []
