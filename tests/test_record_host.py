"""CPU: momlevel_amd.record driven directly -- the layout rule, the block walk and the ranges it
hands to its callback, the axis views, the per-device upload cache, the walk over a Dataset's
variables with the three fates of the time coordinate, and the slope-unit rule.  Host records go
through stubs of engine.device_of and hostio (as tests/test_quantile_host.py); no GPU."""

import numpy as np
import pytest
import torch

from momlevel_amd import core, engine, hostio, record, trend
from momlevel_amd.labeled import DataArray, Dataset

DIMS = ("a", "b", "c")
SHAPE = (4, 3, 5)


@pytest.fixture
def stubbed(monkeypatch):
    monkeypatch.setattr(engine, "device_of", lambda *a, **k: torch.device("cpu"))
    monkeypatch.setattr(hostio, "to_device", lambda x, device, dtype=None: torch.from_numpy(
        np.ascontiguousarray(x)) if dtype is None else torch.from_numpy(
        np.ascontiguousarray(x)).to(dtype))
    monkeypatch.setattr(hostio, "to_host", lambda t: t.numpy())


def _source(dtype):
    v = np.arange(60).reshape(SHAPE) % 7 - 3
    return (v > 0) if dtype == "bool" else v.astype(dtype)


# ---- layout ---------------------------------------------------------------------------------------
DTYPES = ("float64", "float32", ">f4", "int16", "bool")


@pytest.mark.parametrize("axis", (0, 1, 2))
@pytest.mark.parametrize("dtype, tensor", [(d, False) for d in DTYPES]
                         + [(d, True) for d in DTYPES if d != ">f4"])  # (no big-endian tensors)
def test_layout(stubbed, monkeypatch, axis, dtype, tensor):
    src = _source(dtype)
    nt, n = SHAPE[axis], 60 // SHAPE[axis]
    want = np.moveaxis(src, axis, 0).reshape(nt, n)
    is_f32 = dtype in ("float32", ">f4")
    if tensor:  # a CPU tensor standing in for a device record
        monkeypatch.setattr(DataArray, "is_device", property(lambda self: torch.is_tensor(self.data)))
        src = torch.from_numpy(src)
    rec = record.Record(DataArray(src, DIMS), DIMS[axis])
    assert (rec.nt, rec.n, rec.axis) == (nt, n, axis) and rec.device == tensor
    assert rec.rest_dims == tuple(d for d in DIMS if d != DIMS[axis])
    y = rec.y
    if tensor:
        assert torch.is_tensor(y) and y.is_contiguous()
        assert y.dtype == (torch.float32 if is_f32 else torch.float64)
        y = y.numpy()
    else:
        # (C-contiguous unless the rule's reshape could stay a view: a trailing time dim merges
        #  into a strided (nt, n) view of the source, which hostio packs block by block)
        assert isinstance(y, np.ndarray) and (y.flags["C_CONTIGUOUS"] or axis == 2)
        assert y.dtype.itemsize == (4 if is_f32 else 8) and y.dtype.kind == "f"
    assert y.shape == (nt, n) and np.array_equal(y, want.astype(np.float64))
    same = record.layout(DataArray(src, DIMS), DIMS[axis])
    assert type(same) is type(rec.y) and same.dtype == rec.y.dtype
    assert np.array_equal(np.asarray(same), y)


# ---- walk -----------------------------------------------------------------------------------------
def _walked(rec, out_dtype=torch.float64):
    seen = []

    def fn(y, cells):
        seen.append((cells.start, cells.stop, tuple(y.shape), y.dtype))
        total = y[0] * 0.5  # (cell by cell: a sum whose rounding does not depend on the width)
        for t in range(1, y.shape[0]):
            total = total + y[t]
        return total.to(out_dtype), y.to(out_dtype) + 1.0

    return seen, rec.walk(fn, 1, 1)


@pytest.mark.parametrize("block", (1, 7, 34, 35, 36))
@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("float64", "float32"))
def test_walk_in_blocks(stubbed, monkeypatch, block, dtype):
    rng = np.random.default_rng(3)
    da = DataArray(rng.normal(0.0, 1.0, (5, 6, 7)).astype(dtype), ("y", "t", "x"))
    out_dtype = torch.float32 if dtype == np.float32 else torch.float64
    monkeypatch.setattr(record, "BLOCK_CELLS", 35)
    seen, (cell0, step0) = _walked(record.Record(da, "t"), out_dtype)
    assert [s[:3] for s in seen] == [(0, 35, (6, 35))]
    monkeypatch.setattr(record, "BLOCK_CELLS", block)
    seen, (cell, step) = _walked(record.Record(da, "t"), out_dtype)
    edges = list(range(0, 35, block)) + [35]
    assert [s[:2] for s in seen] == list(zip(edges[:-1], edges[1:]))  # ascending, no gaps
    assert all(s[2] == (6, s[1] - s[0]) and s[3] == out_dtype for s in seen)
    assert cell.shape == (5, 7) and step.shape == (6, 5, 7)
    assert cell.dtype == step.dtype == dtype  # (the first block's results decide)
    assert cell.tobytes() == cell0.tobytes() and step.tobytes() == step0.tobytes()
    want = np.moveaxis(da.values, 1, 0)
    assert np.array_equal(step, want + dtype(1.0))


def test_walk_of_a_record_without_cells(stubbed, monkeypatch):
    monkeypatch.setattr(record, "BLOCK_CELLS", 7)
    rec = record.Record(DataArray(np.zeros((6, 0, 3), dtype=np.float32), ("t", "y", "x")), "t")
    seen, (cell, step) = _walked(rec)
    assert seen == [(0, 0, (6, 0), torch.float64)]
    assert cell.shape == (0, 3) and step.shape == (6, 0, 3)


def test_a_float32_output_of_a_float64_record_stays_float32(stubbed, monkeypatch):
    monkeypatch.setattr(record, "BLOCK_CELLS", 4)
    rec = record.Record(DataArray(np.ones((3, 10)), ("t", "x")), "t")
    (out,) = rec.walk(lambda y, cells: (y.sum(0).to(torch.float32),), 0, 1)
    assert out.dtype == np.float32 and out.tolist() == [3.0] * 10


# ---- axis views -----------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", (0, 1, 2))
def test_back_and_to_end_are_views_where_moveaxis_puts_them(stubbed, axis):
    rec = record.Record(DataArray(np.zeros(SHAPE), DIMS), DIMS[axis])
    rest = tuple(s for i, s in enumerate(SHAPE) if i != axis)
    steps = np.arange(60.0).reshape((SHAPE[axis],) + rest)
    lead = np.arange(120.0).reshape((2, SHAPE[axis]) + rest)
    for s in (steps, torch.from_numpy(steps)):
        for got, want in ((rec.back(s), np.moveaxis(steps, 0, axis)),
                          (record.to_end(s), np.moveaxis(steps, 0, -1))):
            assert type(got) is type(s) and np.array_equal(np.asarray(got), want)
            assert np.shares_memory(np.asarray(got), steps)
    for s in (lead, torch.from_numpy(lead)):
        got = rec.back(s, 1)
        assert np.array_equal(np.asarray(got), np.moveaxis(lead, 1, 1 + axis))
        assert np.shares_memory(np.asarray(got), lead)


# ---- operands uploaded once per device -------------------------------------------------------------
class _Plan:
    steps = np.array([0, 2, 1], dtype=np.int32)
    offsets = np.array([0, 2, 3], dtype=np.int64)


def test_an_operand_goes_up_once_for_five_blocks(stubbed, monkeypatch):
    uploads = []
    monkeypatch.setattr(core, "upload_groups",
                        lambda steps, offsets, nt, device: uploads.append((nt, device)) or "groups")
    monkeypatch.setattr(record, "BLOCK_CELLS", 7)
    rec = record.Record(DataArray(np.zeros((3, 35)), ("t", "x")), "t")
    for plan, want in ((_Plan, "groups"), (None, None)):
        groups, got = record.plan_groups(plan, rec.nt), []
        rec.walk(lambda y, cells: (got.append(groups(y.device)), y.sum(0))[1:], 0, 0)
        assert got == [want] * 5
    assert uploads == [(3, torch.device("cpu"))]
    made = []
    on = record.per_device(lambda device: made.append(device) or len(made))
    assert [on("a"), on("b"), on("a"), on("b")] == [1, 2, 1, 2] and made == ["a", "b"]


# ---- the walk over a Dataset ----------------------------------------------------------------------
def _dataset():
    coords = {"time": DataArray(np.arange(4.0), ("time",), None, None, "time"),
              "month": DataArray(np.arange(4) % 12, ("time",), None, None, "month"),
              "x": DataArray(np.arange(3.0), ("x",), None, None, "x")}
    return Dataset({"eta": DataArray(np.ones((4, 3)), ("time", "x")),
                    "depth": DataArray(np.ones(3), ("x",)),
                    "label": DataArray(np.array(["a"] * 4), ("time",))}, coords)


def test_over_a_dataset_and_the_fate_of_the_time_coordinate():
    ds, seen = _dataset(), []

    def one(da):
        seen.append((da.name, sorted(da.coords)))
        return DataArray(np.zeros(3), ("x",), None, None, da.name)

    kept = record.over(ds, "time", one)
    assert seen == [("eta", ["month", "time", "x"])]  # (the coordinates of its dims ride along)
    assert list(kept.data_vars) == ["eta"] and sorted(kept.coords) == ["month", "time", "x"]
    assert kept["time"].values.tolist() == [0.0, 1.0, 2.0, 3.0]
    gone = record.over(ds, "time", one, None)
    assert list(gone.data_vars) == ["eta"] and sorted(gone.coords) == ["x"]
    axis = DataArray(np.array([10.0, 20.0]), ("time",), None, None, "time")
    q = DataArray(np.float64(0.5), (), None, None, "quantile")
    new = record.over(ds, "time", one, axis, {"quantile": q})
    assert list(new.data_vars) == ["eta"] and sorted(new.coords) == ["quantile", "time", "x"]
    assert new["time"].values.tolist() == [10.0, 20.0] and float(new["quantile"].values) == 0.5
    assert record.KEEP is not None and seen == [("eta", ["month", "time", "x"])] * 3


def test_over_stores_a_result_under_its_own_name():
    def one(da):
        return DataArray(np.zeros(3), ("x",), None, None, f"{da.name}_slope")

    assert list(record.over(_dataset(), "time", one).data_vars) == ["eta_slope"]
    nameless = record.over(_dataset(), "time", lambda da: DataArray(np.zeros(3), ("x",)))
    assert list(nameless.data_vars) == ["eta"]


def test_over_refusals():
    ds, da = _dataset(), _dataset()["eta"]
    with pytest.raises(ValueError, match="no variable of the dataset"):
        record.over(ds, "t", lambda v: v)
    empty = record.over(ds, "t", lambda v: v, None, required=False)
    assert list(empty.data_vars) == [] and sorted(empty.coords) == ["month", "time", "x"]
    for required in (True, False):
        with pytest.raises(ValueError, match="the array has no dimension"):
            record.over(da, "t", lambda v: v, required=required)
    assert record.over(da, "time", lambda v: v.name) == "eta"
    with pytest.raises(TypeError):
        record.over(np.ones((4, 3)), "time", lambda v: v)


def test_labeled_places_the_time_axis(stubbed):
    da = _dataset()["eta"].transpose("x", "time")
    da.attrs, da.encoding = {"units": "m"}, {"dtype": "float32"}
    rec = record.Record(da, "time")
    same = rec.labeled(np.zeros((4, 3)))
    assert same.dims == ("x", "time") and same.shape == (3, 4)
    assert sorted(same.coords) == ["month", "time", "x"] and same.name == "eta"
    assert same.attrs == {"units": "m"} and same.attrs is not da.attrs
    assert same.encoding == {"dtype": "float32"} and same.encoding is not da.encoding
    axis = DataArray(np.array([10.0, 20.0]), ("time",), None, None, "time")
    new = rec.labeled(np.zeros((5, 2, 3)), axis, ("q",), attrs={"a": 1}, name="p")
    assert new.dims == ("q", "x", "time") and new.shape == (5, 3, 2)
    assert sorted(new.coords) == ["time", "x"] and new.coords["time"] is axis
    assert new.attrs == {"a": 1} and new.name == "p"
    gone = rec.labeled(np.zeros(3), None, (), {"quantile": DataArray(0.5, ())})
    assert gone.dims == ("x",) and sorted(gone.coords) == ["quantile", "x"]


# ---- slope units ----------------------------------------------------------------------------------
@pytest.mark.parametrize("attrs, time_units, units", [
    ({"units": "m"}, None, "m  ns-1"), ({"units": "m"}, "yr", "m  yr-1"),
    ({}, None, " ns-1"), ({"long_name": "sea level"}, "yr", " yr-1")])
def test_slope_units(attrs, time_units, units):
    before = dict(attrs)
    factor, got = record.slope_units(attrs, time_units)
    assert got == units and attrs == before
    assert factor == 1.0 / trend.time_conversion_factor("ns", time_units or "ns")
    assert factor == (1.0 if time_units is None else 1.0 / (1.0 / (1.0e9 * 60.0 * 60.0 * 24.0 * 365.0)))


def test_the_block_size_lives_here_alone():
    # (a leftover alias in trend would make a stale patch of it pass without walking in blocks)
    assert record.BLOCK_CELLS is None and "BLOCK_CELLS" not in vars(trend)
