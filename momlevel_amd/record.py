"""record - what the labeled time-axis features share: the ``(time, cells)`` record and its walk in
blocks, operands uploaded once per device, the walk over a Dataset's variables, the relabelling of
a result and the small rules of the time axis.

``trend``, ``climatology``, ``filters`` and ``extremes`` do one job around one kernel call each: the
time dimension of a labeled array moves to the front, the rest is flattened into cells, a core
kernel runs on the ``(nt, cells)`` record and the result is unflattened and relabelled.  A new
time-axis feature starts from here and holds only what is particular to it.

Placement: a device tensor in gives a device tensor out and nothing crosses the host link.  Host
(or lazily read) arrays go up and the results come down through ``hostio``, a block of cells at a
time when record and result do not fit the device together.  The kernels behind a record treat
every cell on its own, so the block size never changes a bit of the result.

torch, ``core``, ``engine`` and ``hostio`` are imported where they are used.
"""

import numpy as np

from .labeled import _UNSUPPORTED, DataArray, Dataset, dtype_name, np_dtype

# Cells per block when a host-resident record is walked in blocks; None = sized from free device
# memory (engine.chunk_steps).  The result does not depend on it.
BLOCK_CELLS = None

# the fate of the time coordinate in ``over`` and ``Record.labeled``: KEEP leaves every coordinate
# as it is, a DataArray (a plan's axis) replaces it, None removes it -- and in the last two cases
# every other coordinate on the time dimension goes too
KEEP = "keep"


# ---------------------------------------------------------------------------------------
# the record: time first, every other axis flattened into cells
# ---------------------------------------------------------------------------------------
def layout(arr, dim):
    """``arr`` as a contiguous ``(nt, n)`` record with ``dim`` first: float32 stays float32 (in
    either byte order), anything else becomes float64.  A device tensor stays on the device
    (torch's movedim().contiguous()); everything else gives a host array."""
    nt = arr.sizes[dim]
    n = int(np.prod([arr.sizes[d] for d in arr.dims if d != dim], dtype=np.int64))
    if arr.is_device:
        import torch

        y = arr.data.movedim(arr.dims.index(dim), 0)
        if y.dtype not in (torch.float32, torch.float64):
            y = y.to(torch.float64)
        return y.contiguous().reshape(nt, n)
    host = np.asarray(arr.transpose(dim, ...).values)
    if np_dtype(host.dtype) != np.dtype(np.float32):
        host = host.astype(np.float64, copy=False)
    return host.reshape(nt, n)


class Record:
    """``arr`` laid out by ``layout``: a device tensor (nothing leaves the device) or a host array
    to be walked in blocks of cells."""

    def __init__(self, arr, dim):
        assert dim in arr.dims, f"Dimension {dim} not found in array"
        self.arr, self.dim, self.axis = arr, dim, arr.dims.index(dim)
        self.rest_dims = tuple(d for d in arr.dims if d != dim)
        self.rest_shape = tuple(arr.sizes[d] for d in self.rest_dims)
        self.device = arr.is_device
        self.y = layout(arr, dim)
        self.nt, self.n = (int(s) for s in self.y.shape)

    def walk(self, fn, step_outputs, cell_rows):
        """Run ``fn(device block (nt, cells), cells) -> tuple of device tensors (..., cells)`` over
        the record, ``cells`` being the slice of the record's cells that the block holds, and
        return the outputs with the cells unflattened.  Device records: one call.  Host records: a
        block of cells at a time through hostio, in ascending order, sized so that a block, its
        ``step_outputs`` (nt, cells) results and ``cell_rows`` per-cell rows fit the device."""
        if self.device:
            return tuple(o.reshape(tuple(o.shape[:-1]) + self.rest_shape)
                         for o in fn(self.y, slice(0, self.n)))
        from . import engine, hostio

        device = engine.device_of()
        per_cell = self.nt * (self.y.dtype.itemsize + 8 * step_outputs) + 8 * cell_rows
        block = BLOCK_CELLS or engine.chunk_steps(self.n, per_cell, device)
        block = max(1, min(int(block), max(self.n, 1)))
        outs = None
        for c0 in range(0, self.n, block):
            cells = slice(c0, min(c0 + block, self.n))
            res = fn(hostio.to_device(self.y[:, cells], device), cells)
            if outs is None:
                outs = [np.empty(tuple(r.shape[:-1]) + (self.n,), dtype=np_dtype(r.dtype))
                        for r in res]  # (float64 for every fit; a grouped statistic keeps float32)
            for o, r in zip(outs, res):
                o[..., cells] = hostio.to_host(r)
        if outs is None:  # no cells at all
            import torch

            empty = torch.empty((self.nt, 0), dtype=torch.float64, device=device)
            outs = [hostio.to_host(r) for r in fn(empty, slice(0, 0))]
        return tuple(o.reshape(o.shape[:-1] + self.rest_shape) for o in outs)

    def back(self, steps, lead=0):
        """a (lead dims..., nt, ...) result with the time axis back where the input had it among
        its own dims (a view)"""
        if self.axis == 0:
            return steps
        if hasattr(steps, "movedim"):
            return steps.movedim(lead, lead + self.axis)
        return np.moveaxis(steps, lead, lead + self.axis)

    def labeled(self, data, time=KEEP, lead_dims=(), coords=None, attrs=None, name=None):
        """``data`` (lead dims..., steps or groups, cells...) as a DataArray labelled like the
        input: the time axis goes back where the input had it, with every coordinate (``time``
        KEEP) or with ``time`` (a plan's axis) in place of the coordinates on it.  ``time`` None:
        ``data`` is (lead dims..., cells...) and the time dimension is gone.  ``coords`` are added;
        attrs are copied unless given; name (unless given) and encoding are carried."""
        arr, lead_dims = self.arr, tuple(lead_dims)
        if time is KEEP:
            cs = dict(arr.coords)
        else:
            cs = {k: v for k, v in arr.coords.items() if self.dim not in v.dims}
        if time is None:
            dims = lead_dims + self.rest_dims
        else:
            dims, data = lead_dims + tuple(arr.dims), self.back(data, len(lead_dims))
            if time is not KEEP:
                cs[self.dim] = time
        cs.update(coords or {})
        out = DataArray(data, dims, cs, dict(arr.attrs) if attrs is None else attrs,
                        arr.name if name is None else name)
        out.encoding = dict(arr.encoding)
        return out


def to_end(steps):
    """(nt, ...) -> (..., nt), a view: the dims of xarray's ``slope * index`` (trend.py:105)"""
    if hasattr(steps, "movedim"):
        return steps.movedim(0, -1)
    return np.moveaxis(steps, 0, -1)


def per_device(make):
    """``on(device)``: a host operand on that device, made by ``make(device)`` the first time it is
    asked for there -- once per variable and device, not once per block"""
    made = {}

    def on(device):
        if device not in made:
            made[device] = make(device)
        return made[device]

    return on


def plan_groups(plan, nt):
    """``per_device`` for the group lists of ``plan`` (``core.upload_groups``); a plan of None
    means no groups: None on every device, nothing uploaded"""
    def make(device):
        from . import core

        return None if plan is None else core.upload_groups(plan.steps, plan.offsets, nt, device)

    return per_device(make)


# ---------------------------------------------------------------------------------------
# labels: which variables take part, and where a Dataset's coordinates go
# ---------------------------------------------------------------------------------------
def check_record_dtype(da):
    name = dtype_name(da.data.dtype)
    if name in _UNSUPPORTED:
        raise TypeError(f"{name} records are not supported: convert '{da.name}' to float32 or "
                        "float64")
    return name


def is_numeric(da):
    """float, integer and boolean variables take part; strings, objects, times are skipped"""
    if dtype_name(da.data.dtype) in _UNSUPPORTED:
        return True  # (and refused, loudly, by check_record_dtype)
    try:
        return np_dtype(da.data.dtype).kind in "fiub"
    except TypeError:
        return False


def over(xobj, tcoord, one, time=KEEP, coords=None, required=True):
    """``one(DataArray)`` for a DataArray, or for every numeric variable of a Dataset that has
    ``tcoord``: non-numeric variables are skipped, variables without ``tcoord`` are left out (a
    groupby over time drops them), and ``one`` gets ``xobj[name]``, which carries the coordinates of
    its dims.  A result is stored under its own name when it has one.  The Dataset's coordinates
    follow ``time`` (see KEEP) and ``coords`` are added.  A DataArray without ``tcoord`` is a
    ``ValueError``; so is, when ``required``, a Dataset none of whose variables has it."""
    if isinstance(xobj, DataArray):
        if tcoord not in xobj.dims:
            raise ValueError(f"the array has no dimension '{tcoord}'")
        return one(xobj)
    if not isinstance(xobj, Dataset):
        raise TypeError("Input must be a DataArray or a Dataset")
    if required and not any(tcoord in v.dims for v in xobj.data_vars.values()):
        raise ValueError(f"no variable of the dataset has a dimension '{tcoord}'")
    result = Dataset()
    for name, c in xobj.coords.items():
        if time is KEEP or tcoord not in c.dims:
            result._set(name, c, is_coord=True)
    if time is not KEEP and time is not None:
        result._set(tcoord, time, is_coord=True)
    for name, c in (coords or {}).items():
        result._set(name, c, is_coord=True)
    for name, var in xobj.data_vars.items():
        if tcoord in var.dims and is_numeric(var):
            res = one(xobj[name])
            result[res.name if res.name is not None else name] = res
    return result


# ---------------------------------------------------------------------------------------
# the time axis
# ---------------------------------------------------------------------------------------
def axis_values(arr, dim):
    """the coordinate of ``dim`` (its objects / numbers), or 0..n-1 when there is none"""
    if dim in arr.coords:
        return np.asarray(arr.coords[dim].values)
    if arr.dims == (dim,) and arr.name == dim:
        return np.asarray(arr.values)
    return np.arange(arr.sizes[dim], dtype=np.float64)


def rest_coords(arr, dims):
    """the coordinates of ``arr`` that live on ``dims`` alone"""
    return {k: v for k, v in arr.coords.items() if set(v.dims) <= set(dims)}


def slope_units(attrs, time_units):
    """``(factor, units)`` of a slope along a calendar axis: the factor takes a slope per
    nanosecond to ``time_units`` ("ns", "s", "min", "hr", "day", "mon", "yr"; None: "ns") and
    ``units`` is the reference's attribute (trend.py:268-285), ``"<units>  <time_units>-1"`` or
    ``" <time_units>-1"`` when ``attrs`` has no units"""
    from .trend import time_conversion_factor

    time_units = "ns" if time_units is None else time_units
    units = attrs["units"] + " " if "units" in attrs else ""
    return 1.0 / time_conversion_factor("ns", time_units), f"{units} {time_units}-1"
