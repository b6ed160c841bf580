"""census - weighted histograms of a record by value class on the GPU: how much ocean lies in
every (theta, S), (sigma, pi) or sigma class, per time step.

EXTENSION: momlevel has no such functions.  A water-mass view is a volumetric census -- the m^3 of
ocean per class of ``calc_pdens`` against ``calc_spice``, the volume warmer than 20 degC, the area
per class of steric trend, the PDF of eta by month, the heat content by density class -- and each
of them is a histogram of a record, weighted by a map the package already holds (``volcello``,
``areacello``), whose bin depends on the DATA.  The answer is ``nbins`` numbers per record against
75 x 1080 x 1440 cells, so it is formed where the fields were computed and only the table leaves
the device.  In numpy this is ``numpy.histogramdd`` with explicit edges (or xhistogram); the
specification is its restatement tests/census_numpy.py, which the kernels
(csrc/momlevel_census.hip, ``core.census``; include/momlevel_census.h states the contract) are
gated against: counts bit for bit, sums inside the summation-order bound.

For one record, ``D`` = 1 or 2 binning fields widened exactly to float64, ``e_d`` the ``n_d + 1``
strictly increasing edges of field d::

    i_d   = searchsorted(e_d, f_d, side="right") - 1      # the last edge belongs to the last bin
    valid = every 0 <= i_d < n_d, and ~isnan(weight) & ~isnan(value)
    count[bin] = number of valid cells      wsum[bin] = sum w      vsum[bin] = sum w * v

A value below the first edge, above the last, +-inf or NaN leaves its cell out; ``-0.0`` lies in the
bin that starts at ``0.0``.  NOTE the one difference from numpy: a cell whose weight or value is NaN
is left out of all three outputs (numpy would poison the bin).  There are no atomics: the order of
summation is a function of the record's size alone, so reruns, split calls, bin groups and host or
device input agree to the bit.

Binning by a STATIC map needs none of this: zonal bands of ``geolat`` or basins are a sparse table
for ``regrid.from_triplets`` or a label map for ``regional.area_mean``.

NOT BUILT: more than two binning fields; the density evaluated inside the census (as the column
search does); a census spread over several ranks (the partial tables are additive over tiles); a
table in global memory for very large ``nbins`` -- a table larger than one launch holds (``core.
census_max_bins``) is launched in bin groups instead, the fields re-read once per group.
"""

import numpy as np
import torch

from . import core, engine, hostio
from .adapters import accepts_xarray
from .labeled import DataArray, check_field_dtype

__all__ = ["histogram", "ts_census", "bin_edges"]

WORKSPACE_BOUND = 256 << 20  # bytes of partials one launch may ask for
RECORD_WINDOW = 256          # the most records of one launch
_MAX_ELEMS = 1 << 40         # records x cells of one launch (include/momlevel_census.h)


def bin_edges(lo, hi, n):
    """``n`` equal bins from ``lo`` to ``hi``: ``numpy.linspace(lo, hi, n + 1)`` as float64."""
    if int(n) != n or int(n) < 1:
        raise ValueError(f"a table has a whole number of bins >= 1, got {n}")
    return np.linspace(float(lo), float(hi), int(n) + 1, dtype=np.float64)


# ---------------------------------------------------------------------------------------
# planning: pure functions, on the host
# ---------------------------------------------------------------------------------------
def check_edges(bins, nfields):
    """``bins`` -> one float64 edge array per field: strictly increasing, finite, two edges at least"""
    if nfields == 1 and not (isinstance(bins, (list, tuple)) and len(bins) == 1
                             and np.ndim(bins[0]) == 1):
        bins = [bins]
    if not isinstance(bins, (list, tuple)) or len(bins) != nfields:
        raise ValueError(f"bins must hold one edge array per field ({nfields}): pass "
                         "bins=(edges0, edges1), made with bin_edges or by hand")
    out = []
    for d, e in enumerate(bins):
        if isinstance(e, torch.Tensor):
            e = e.detach().cpu().numpy()
        e = np.array(e, dtype=np.float64)
        if e.ndim != 1 or e.size < 2:
            raise ValueError(f"bins[{d}] must be a 1-D array of at least two edges (one bin): an "
                             "integer number of bins is not taken, use bin_edges(lo, hi, n)")
        if not np.all(np.isfinite(e)):
            raise ValueError(f"bins[{d}] holds NaN or infinite edges: use finite edges, values "
                             "outside them are left out")
        if not np.all(np.diff(e) > 0):
            raise ValueError(f"bins[{d}] must increase strictly (monotonic edges): sort them and "
                             "drop duplicates")
        out.append(e)
    return out


def plan_bin_groups(shape, cap):
    """The table of ``shape`` (n0,) or (n0, n1) bins in launches of at most ``cap`` bins:
    ``[((a0, b0), ...)]``, one half-open index range per field, rectangles that tile the table --
    every bin lies in exactly one.  A 2-D table is cut into bands of whole rows, a row longer than
    ``cap`` into pieces."""
    shape = tuple(int(n) for n in shape)
    cap = int(cap)
    if cap < 1 or len(shape) not in (1, 2) or min(shape) < 1:
        raise ValueError("a table has one or two dims of at least one bin, and a launch holds one")
    if len(shape) == 1:
        return [((a, min(a + cap, shape[0])),) for a in range(0, shape[0], cap)]
    n0, n1 = shape
    if n1 <= cap:
        rows = cap // n1
        return [((a, min(a + rows, n0)), (0, n1)) for a in range(0, n0, rows)]
    return [((i, i + 1), (a, min(a + cap, n1))) for i in range(n0) for a in range(0, n1, cap)]


def group_closed(group, shape):
    """mlx_census_histogram's ``closed`` of one group: bit d when the group ends field d's table"""
    return sum(1 << d for d, ((_, b), n) in enumerate(zip(group, shape)) if b == n)


def plan_record_windows(nrec, ncells, bytes_per_record, bound=None, cap=None):
    """``[(i0, i1)]``: the records in launches whose partials stay under ``bound`` bytes (one
    record at least; default WORKSPACE_BOUND), of at most ``cap`` records (default RECORD_WINDOW)
    and 2^40 elements."""
    bound = WORKSPACE_BOUND if bound is None else bound
    cap = RECORD_WINDOW if cap is None else cap
    rows = max(1, min(int(cap), int(bound) // max(1, int(bytes_per_record)),
                      _MAX_ELEMS // max(1, int(ncells))))
    return [(i0, min(i0 + rows, int(nrec))) for i0 in range(0, int(nrec), rows)]


# ---------------------------------------------------------------------------------------
# one call's plan: checked on the host before any device work
# ---------------------------------------------------------------------------------------
def _float_name(x, what):
    name = check_field_dtype(x.dtype, what)
    if name not in ("float32", "float64"):
        raise TypeError(f"{what} must be float32 or float64, not {name}: convert with "
                        ".astype(float32 / float64) (classes of an integer field need edges "
                        "between the integers)")
    return name


def _wrap(x, what):
    if isinstance(x, DataArray):
        return x
    if isinstance(x, (list, tuple)) or np.isscalar(x):
        raise TypeError(f"{what} must be a DataArray, a numpy array, a device tensor or a lazy "
                        "array")
    return DataArray(x)


class _Plan:
    def __init__(self, fields, bins, weights, values, tcoord):
        if not 1 <= len(fields) <= 2:
            raise ValueError(f"the census bins by one or two fields, got {len(fields)}: more than "
                             "two binning fields are not built -- fold one into the records")
        self.labeled = all(isinstance(f, DataArray) for f in fields)
        self.fields = [_wrap(f, "a field") for f in fields]
        f0 = self.fields[0]
        self.names = [_float_name(f, "binning fields") for f in self.fields]
        for f in self.fields[1:]:
            if tuple(f.shape) != tuple(f0.shape):
                raise ValueError(f"the fields' shapes {tuple(f0.shape)} and {tuple(f.shape)} differ: "
                                 "bring them to one grid and one shape first")
        self.edges = check_edges(bins, len(self.fields))
        if tcoord in f0.dims and f0.dims.index(tcoord) != 0:
            raise ValueError(f"'{tcoord}' must be the first dim of {f0.dims}: the reduced dims are "
                             "trailing and contiguous -- transpose the record")
        self.lead = 1 if tcoord in f0.dims else 0
        self.lead_shape = tuple(int(n) for n in f0.shape[:self.lead])
        self.red_shape = tuple(int(n) for n in f0.shape[self.lead:])
        self.nrec = int(np.prod(self.lead_shape, dtype=np.int64))
        self.ncells = int(np.prod(self.red_shape, dtype=np.int64))
        if values is not None and weights is None:
            raise ValueError("values need weights: the class mean is sum(w * v) / sum(w) -- pass "
                             "weights (ones for a plain mean)")
        self.weights = self.values = None
        self.w_per_record = False
        if weights is not None:
            self.weights = _wrap(weights, "weights")
            self.wname = _float_name(self.weights, "weights")
            ws = tuple(int(n) for n in self.weights.shape)
            if ws == tuple(f0.shape) and self.lead:
                self.w_per_record = True
            elif ws != self.red_shape:
                raise ValueError(f"weights of shape {ws} fit neither the reduced dims "
                                 f"{self.red_shape} nor the whole field {tuple(f0.shape)}: "
                                 "broadcast them to one of the two")
        if values is not None:
            self.values = _wrap(values, "values")
            self.vname = _float_name(self.values, "values")
            if tuple(self.values.shape) != tuple(f0.shape):
                raise ValueError(f"values of shape {tuple(self.values.shape)} must have the "
                                 f"fields' shape {tuple(f0.shape)}")
        self.shape = tuple(e.size - 1 for e in self.edges)

    # what travels per record, in the order the launches take it
    def per_record(self):
        ops = list(self.fields)
        if self.w_per_record:
            ops.append(self.weights)
        if self.values is not None:
            ops.append(self.values)
        return ops


def _tdt(da):
    return torch.float32 if check_field_dtype(da.dtype) == "float32" else torch.float64


def _launch(plan, dev, edges_dev, fields, weights, values):
    """(count, wsum, vsum), each (rows, nbins) -- wsum / vsum None without weights / values -- of
    the (rows, ncells) device operands: record windows x bin groups of ``core.census``."""
    rows = int(fields[0].shape[0])
    hw, hv = weights is not None, values is not None
    D, shape = len(fields), plan.shape
    nbins = int(np.prod(shape))
    groups = plan_bin_groups(shape, core.census_max_bins(D, hw, hv))
    widest = max(int(np.prod([b - a for a, b in g])) for g in groups)
    per_rec = core.census_blocks(plan.ncells) * widest * (1 + hw + hv) * 8
    count = torch.empty((rows,) + shape, dtype=torch.int64, device=dev)
    wsum = torch.empty((rows,) + shape, dtype=torch.float64, device=dev) if hw else None
    vsum = torch.empty((rows,) + shape, dtype=torch.float64, device=dev) if hv else None
    if plan.ncells == 0:
        for t in (count, wsum, vsum):
            if t is not None:
                t.zero_()
        return count.reshape(rows, nbins), wsum, vsum
    for i0, i1 in plan_record_windows(rows, plan.ncells, per_rec):
        f = [x[i0:i1] for x in fields]
        w = weights[i0:i1] if hw and weights.dim() == 2 else weights
        v = values[i0:i1] if hv else None
        for g in groups:
            e = [edges_dev[d][a:b + 1] for d, (a, b) in enumerate(g)]
            c, sw, sv = core.census(f, e, w, v, closed=group_closed(g, shape))
            box = (slice(i0, i1),) + tuple(slice(a, b) for a, b in g)
            gshape = (i1 - i0,) + tuple(b - a for a, b in g)
            count[box] = c.reshape(gshape)
            if hw:
                wsum[box] = sw.reshape(gshape)
            if hv:
                vsum[box] = sv.reshape(gshape)
    return count, wsum, vsum


def _run(plan):
    """(count, wsum, vsum) as raw arrays of shape lead + table: on the device when the first field
    lives there, on the host otherwise"""
    f0 = plan.fields[0]
    data = [x.data for x in plan.fields + [plan.weights, plan.values] if x is not None]
    dev = engine.device_of(*data)
    on_device = f0.is_device
    hw, hv = plan.weights is not None, plan.values is not None
    K = 1 + hw + hv
    nrec, ncells, shape = plan.nrec, plan.ncells, plan.shape
    edges_dev = [hostio.to_device(e, dev, torch.float64).contiguous() for e in plan.edges]

    def on_dev(da, rows):
        t = da.data.to(_tdt(da)) if da.is_device else engine.to_device(da.values, dev, _tdt(da))
        return t.reshape(rows, ncells).contiguous()

    static_w = None
    if hw and not plan.w_per_record:
        static_w = on_dev(plan.weights, 1).reshape(ncells)
    ops = plan.per_record()

    if (not any(x.is_device for x in ops) and plan.lead and nrec > 0
            and hostio.wants_pipeline(nrec, nrec * ncells)):
        # a large host / lazy record: groups of whole leading rows; a lazy record is never
        # materialised whole.  A record's table depends on that record alone.  The counts travel as
        # float64 (exact: a count is at most 2^38).
        sources = [x.data if x.is_lazy else x.values for x in ops]

        def kernel(tensors, i0, i1):
            t = [x.to(_tdt(o)).reshape(i1 - i0, ncells) for x, o in zip(tensors, ops)]
            f = t[:len(plan.fields)]
            w = t[len(plan.fields)] if plan.w_per_record else static_w
            v = t[-1] if hv else None
            c, sw, sv = _launch(plan, dev, edges_dev, f, w, v)
            parts = [c.to(torch.float64)] + [s for s in (sw, sv) if s is not None]
            return torch.stack([p.reshape((i1 - i0,) + shape) for p in parts], dim=1)

        both = hostio.pipeline_rows(hostio.row_bounds(nrec, ncells), dev,
                                    hostio.leading_slices(sources), kernel,
                                    np.empty((nrec, K) + shape, dtype=np.float64))
        count = both[:, 0].astype(np.int64)
        return count, both[:, 1].copy() if hw else None, both[:, 2].copy() if hv else None

    rows = max(nrec, 1) if not plan.lead else nrec
    t = [on_dev(x, rows) for x in ops]
    f = t[:len(plan.fields)]
    w = t[len(plan.fields)] if plan.w_per_record else static_w
    v = t[-1] if hv else None
    count, wsum, vsum = _launch(plan, dev, edges_dev, f, w, v)
    full = plan.lead_shape + shape
    out = [None if x is None else x.reshape(full) for x in (count, wsum, vsum)]
    if not on_device:
        out = [None if x is None else hostio.to_host(x) for x in out]
    return tuple(out)


def _class_mean(count, wsum, vsum):
    """sum(w v) / sum(w); NaN where the bin is empty"""
    if isinstance(count, torch.Tensor):
        nan = torch.full_like(vsum, float("nan"))
        return torch.where(count > 0, vsum / wsum, nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(count > 0, vsum / wsum, np.nan)


def _bin_names(fields):
    names = [f.name if f.name else f"field{d}" for d, f in enumerate(fields)]
    if len(names) == 2 and names[0] == names[1]:
        names = [f"{names[0]}_0", f"{names[1]}_1"]
    return names


def sums(*fields, bins, weights=None, values=None, tcoord="time"):
    """The three raw tables behind ``histogram``: ``(count, wsum, vsum)`` of shape lead + table --
    int64 counts, float64 ``sum w`` (None without weights) and ``sum w * v`` (None without values)
    -- as raw arrays, on the device when the first field lives there.  What a caller needs to
    combine tiles or ranks: the three are additive."""
    return _run(_Plan(fields, bins, weights, values, tcoord))


@accepts_xarray
def histogram(*fields, bins, weights=None, values=None, tcoord="time", return_count=False):
    """The census of one or two fields (EXTENSION: not in momlevel; ``numpy.histogramdd`` with
    explicit edges, per record -- the specification is the module docstring and
    tests/census_numpy.py).

    ``fields``: one or two DataArrays of one shape -- or numpy arrays, device tensors, lazy or
    masked arrays, answered in kind -- float32 or float64 each (float16 and integers are refused:
    convert them).  Every dim but ``tcoord`` is reduced; ``tcoord``, when present, must come first
    and gives one table per step.  ``bins``: one array of strictly increasing finite edges per
    field (``bin_edges(lo, hi, n)``); a value on the last edge belongs to the last bin, values
    outside the edges, +-inf and NaN leave their cell out.

    ``weights``: of the reduced shape (a static ``volcello(z, y, x)``, ``areacello(y, x)`` under a
    ``(time, y, x)`` record) or of the fields' whole shape; ``values``: of the fields' shape, and
    only with weights.  float32 or float64 each.  UNLIKE numpy, a cell whose weight or value is NaN
    is left out (numpy would make its bin NaN): land needs no masking.

    Returns a DataArray ``(tcoord, <name>_bin[, <name2>_bin])`` with the bin centres as
    coordinates and the edges in ``attrs["<name>_bin_edges"]``: int64 counts without weights,
    float64 ``sum w`` with weights, the class mean ``sum(w v) / sum(w)`` with values (NaN where a
    bin is empty).  ``return_count=True`` returns ``(result, count)``.  The result lives on the
    device when the first field does; a large host or lazy record goes up in groups of whole steps.

    A table larger than one launch holds is launched in bin groups (the fields re-read once per
    group): 100 x 100 classes are a few passes.  No atomics: the order of summation is fixed, so
    reruns, split records, bin groups and host or device input agree to the bit.  Binning by a
    static map (latitude bands, basins) is ``regrid.from_triplets`` / ``regional.area_mean``."""
    plan = _Plan(fields, bins, weights, values, tcoord)
    count, wsum, vsum = _run(plan)
    if values is not None:
        result = _class_mean(count, wsum, vsum)
    else:
        result = count if weights is None else wsum
    if not plan.labeled:
        return (result, count) if return_count else result
    f0 = plan.fields[0]
    names = _bin_names(plan.fields)
    lead_dims = tuple(f0.dims[:plan.lead])
    dims = lead_dims + tuple(f"{n}_bin" for n in names)
    coords = {k: c for k, c in f0.coords.items() if set(c.dims) <= set(lead_dims)}
    attrs = {}
    for n, e, f in zip(names, plan.edges, plan.fields):
        centre = 0.5 * (e[:-1] + e[1:])
        cattrs = {k: f.attrs[k] for k in ("units", "long_name") if k in f.attrs}
        coords[f"{n}_bin"] = DataArray(centre, (f"{n}_bin",), None, cattrs, f"{n}_bin")
        attrs[f"{n}_bin_edges"] = e.copy()
    src = plan.values if values is not None else plan.weights
    if src is not None and isinstance(src, DataArray) and "units" in src.attrs:
        attrs["units"] = src.attrs["units"]
    attrs["cell_methods"] = ("census: count" if weights is None else
                             "census: sum" if values is None else "census: mean")
    name = (src.name if src is not None and src.name else "count")
    out = DataArray(result, dims, coords, attrs, name)
    if not return_count:
        return out
    return out, DataArray(count, dims, coords, {**attrs, "cell_methods": "census: count",
                                                "units": "1"}, "count")


@accepts_xarray
def ts_census(thetao, so, volcello, theta_bins, salt_bins, tcoord="time", return_count=False):
    """The volumetric theta-S census in one call (EXTENSION, see ``histogram``): the m^3 of ocean
    in every (theta, S) class per step, ``(time, thetao_bin, so_bin)``.  ``volcello``: the static
    ``(z, y, x)`` cell volumes or a ``(time, z, y, x)`` record of them; NaN volumes (land) are left
    out.  The sigma-pi form of the same view, without theta and S leaving the device::

        census.histogram(derived.calc_pdens(thetao, so), derived.calc_spice(thetao, so),
                         weights=volcello, bins=(sigma_edges, spice_edges))
    """
    def named(x, name):
        if isinstance(x, DataArray) and not x.name:
            x = DataArray(x.data, x.dims, x.coords, x.attrs, name)
        return x

    return histogram(named(thetao, "thetao"), named(so, "so"), bins=(theta_bins, salt_bins),
                     weights=named(volcello, "volcello"), tcoord=tcoord,
                     return_count=return_count)
