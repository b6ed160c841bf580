"""regional.py -- area-weighted global and regional means of a ``(..., yh, xh)`` record, and the
anomalies from them, on the MI355X.

AN EXTENSION, in the sense of ``steric_variants``: momlevel has no such function.  It is the first
thing its documentation does with a local field -- "represent the local steric changes as
anomalies from the global mean" (docs/source/steric.rst), ``zos`` "reported as a deviation from the
global mean" (docs/source/inverse_barometer.rst) -- and a ``(time, yh, xh)`` record that lives on
the device reaches its global-mean curve, its per-basin series or its anomaly field here without a
download.  In xarray the mean is spelled ``xobj.weighted(areacello.fillna(0)).mean((ydim, xdim))``;
xarray is not importable where the tests run, so parity with it is UNPINNED: the specification is
the numpy restatement tests/area_numpy.py, which the kernels (csrc/momlevel_area.hip) are gated
against.

For every leading index ``rec`` and region ``r``, with the operands widened exactly to float64::

    valid = ~isnan(v[rec]) & ~isnan(area) & (label == r)
    w     = where(valid, area, 0.0)
    den   = sum(w)
    mean  = sum(w * where(valid, v[rec], 0.0)) / den        # NaN where nothing is valid
    anomaly[rec, c] = v[rec, c] - mean[rec, region(c)]      # NaN outside every region
"""

import numpy as np
import torch

from . import core, derived, engine, hostio
from .adapters import accepts_xarray
from .labeled import DataArray, Dataset, check_field_dtype

__all__ = ["area_anomaly", "area_mean"]


# ---------------------------------------------------------------------------------------
# region planning: pure functions of the 2-D label map (host, numpy)
# ---------------------------------------------------------------------------------------
def region_labels(regions):
    """The label map as int64: integers as they are, a float map of whole numbers and NaN cast
    (NaN -> 0, no region); anything else is refused."""
    lab = np.asarray(regions)
    if lab.dtype.kind in "iub":
        return lab.astype(np.int64)
    if lab.dtype.kind != "f":
        raise TypeError(f"regions must be an integer label map, not {lab.dtype}")
    nan = np.isnan(lab)
    whole = np.where(nan, 0.0, lab)
    if not np.all(np.isfinite(whole)) or np.any(whole != np.rint(whole)):
        raise ValueError("a float regions map must hold whole numbers and NaN only")
    return whole.astype(np.int64)


def plan_regions(regions, region_ids=None):
    """``(ids, slot)``: the region ids (int64, in result order) and the int32 map of the same
    shape as ``regions`` that holds every cell's position in ``ids``, -1 for cells of no region
    (labels <= 0, NaN, labels that are not in ``ids``).  ``region_ids=None``: the sorted unique
    positive labels present; an explicit sequence fixes the order, may name absent labels (their
    rows are NaN), and must hold positive integers without duplicates."""
    lab = region_labels(regions)
    if region_ids is None:
        ids = np.unique(lab[lab > 0])
    else:
        raw = np.asarray(list(region_ids))
        if raw.size and (raw.dtype.kind not in "iuf" or np.any(raw != np.rint(raw))):
            raise ValueError("region_ids must be integers")
        ids = raw.astype(np.int64).reshape(-1)
        if np.unique(ids).size != ids.size:
            raise ValueError("region_ids holds duplicates")
        if np.any(ids <= 0):
            raise ValueError("region_ids must be positive: labels <= 0 belong to no region")
    slot = np.full(lab.shape, -1, dtype=np.int32)
    if ids.size:
        order = np.argsort(ids, kind="stable")
        pos = np.minimum(np.searchsorted(ids[order], lab), ids.size - 1)
        hit = (ids[order][pos] == lab) & (lab > 0)
        slot[hit] = order[pos[hit]].astype(np.int32)
    return ids, slot


def slot_groups(nids, cap=core.AREA_MAX_SLOTS):
    """``[(start, count)]``: the ids in launches of at most ``cap`` slots"""
    return [(s, min(cap, nids - s)) for s in range(0, nids, cap)]


def group_slot_map(slot, start, count):
    """The slot map of one launch: slots ``start .. start+count-1`` renumbered from 0, every other
    cell -1 (no region)."""
    inside = (slot >= start) & (slot < start + count)
    return np.where(inside, slot - start, -1).astype(np.int32)


# ---------------------------------------------------------------------------------------
# the maps of one call: checked once on the host, uploaded once per device
# ---------------------------------------------------------------------------------------
def _int32_on(a, dev):
    """a host int32 map -> device tensor, through the staging ring like every other upload"""
    host = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
    out = torch.empty(host.shape, dtype=torch.int32, device=dev)
    hostio.upload(host, out)
    return out


class _Maps:
    def __init__(self, areacello, regions, region_ids):
        if not isinstance(areacello, DataArray):
            areacello = DataArray(areacello)
        if areacello.ndim != 2:
            raise ValueError(f"areacello has dims {areacello.dims}: a 2-D (ydim, xdim) field is "
                             "expected")
        self.src = areacello
        self.dims = tuple(areacello.dims)
        self.shape = tuple(int(n) for n in areacello.shape)
        name = derived.float_name(areacello, "areacello", allow_other=True)
        # (a device-resident map is small: downloaded for the check)
        area = np.ascontiguousarray(areacello.values,
                                    dtype=np.float32 if name == "float32" else np.float64)
        if np.any(area < 0):  # (NaN compares False: it carries no weight)
            raise ValueError("areacello holds negative areas")
        self.area = area.reshape(-1)
        self.ids = self.slot = None
        if regions is None:
            if region_ids is not None:
                raise ValueError("region_ids needs a regions map")
        else:
            if isinstance(regions, DataArray):
                if tuple(regions.dims) != self.dims:
                    raise ValueError(f"regions has dims {regions.dims}: expected {self.dims}")
                regions = regions.values
            elif isinstance(regions, torch.Tensor):
                regions = regions.detach().cpu().numpy()
            if tuple(np.shape(regions)) != self.shape:
                raise ValueError(f"regions {tuple(np.shape(regions))} does not cover areacello's "
                                 f"plane {self.shape}")
            self.ids, slot = plan_regions(regions, region_ids)
            self.slot = slot.reshape(-1)
        self._on = {}

    @property
    def nslots(self):
        return 1 if self.ids is None else int(self.ids.size)

    def on(self, dev):
        """(area, slot map of every id or None, [(start, count, slot map of the launch)]) on
        ``dev``"""
        key = str(dev)
        if key not in self._on:
            if self.src.is_device and self.src.data.device == dev:
                area = self.src.data.to(torch.float32 if self.area.dtype == np.float32
                                        else torch.float64).contiguous().reshape(-1)
            else:
                area = engine.to_device(self.area, dev)
            full, launches = None, []
            if self.ids is not None:
                full = _int32_on(self.slot, dev)
                groups = slot_groups(self.nslots)
                launches = [(s, n, full if len(groups) == 1 else
                             _int32_on(group_slot_map(self.slot, s, n), dev))
                            for s, n in groups]
            self._on[key] = (area, full, launches)
        return self._on[key]

    def mean(self, v, dev):
        """(mean, den) of the records ``v`` (nrec, plane): (nrec, nslots) device tensors"""
        area, full, launches = self.on(dev)
        if self.ids is None:
            return core.area_mean(v, area)
        if len(launches) == 1:
            return core.area_mean(v, area, full, self.nslots)
        mean = torch.empty((v.shape[0], self.nslots), dtype=torch.float64, device=dev)
        den = torch.empty_like(mean)
        for start, count, slot in launches:  # (none for an empty list of ids)
            m, d = core.area_mean(v, area, slot, count)
            mean[:, start:start + count] = m
            den[:, start:start + count] = d
        return mean, den

    def anomaly(self, v, mean, dev):
        _, full, _ = self.on(dev)
        if self.ids is None:
            return core.area_anomaly(v, mean)
        if self.nslots == 0:  # no region at all: every cell is outside
            return torch.full(tuple(v.shape), float("nan"), dtype=torch.float64, device=dev)
        return core.area_anomaly(v, mean, full)


# ---------------------------------------------------------------------------------------
# one variable
# ---------------------------------------------------------------------------------------
def _records(da, maps, want_anomaly):
    """(mean, den, anomaly or None) of one DataArray as raw arrays -- (lead..., nslots) and the
    input's shape -- on the device for a device record, on the host otherwise."""
    ydim, xdim = maps.dims
    derived.check_trailing(da, ydim, xdim, da.name or "the record")
    if tuple(int(n) for n in da.shape[-2:]) != maps.shape:
        raise ValueError(f"the record's plane {tuple(da.shape[-2:])} is not areacello's {maps.shape}")
    name = check_field_dtype(da.dtype, "records")
    tdt = torch.float32 if name == "float32" else torch.float64  # (integers compute as float64)
    lead = tuple(int(n) for n in da.shape[:-2])
    nrec = int(np.prod(lead, dtype=np.int64))
    plane = maps.shape[0] * maps.shape[1]
    ns = maps.nslots
    dev = engine.device_of(da.data, maps.src.data)
    on_device = da.is_device

    if not on_device and len(lead) >= 1 and hostio.wants_pipeline(lead[0], nrec * plane):
        # a large host / lazy record: groups of whole leading rows, uploads, kernels and downloads
        # overlapping; a lazy record is never materialised whole.  A record's means depend on that
        # record alone, so the grouping cannot show in the result.
        inner = nrec // lead[0]
        source = da.data if da.is_lazy else da.values

        def groups(kernel, out):
            return hostio.pipeline_rows(hostio.row_bounds(lead[0], inner * plane), dev,
                                        hostio.leading_slices([source]), kernel, out)

        def stats(tensors, i0, i1):
            v = tensors[0].to(tdt).reshape((i1 - i0) * inner, plane)
            return (v,) + maps.mean(v, dev)

        if want_anomaly:
            mean_d = torch.empty((nrec, ns), dtype=torch.float64, device=dev)
            den_d = torch.empty_like(mean_d)

            def kernel(tensors, i0, i1):
                v, m, d = stats(tensors, i0, i1)
                mean_d[i0 * inner:i1 * inner] = m
                den_d[i0 * inner:i1 * inner] = d
                return maps.anomaly(v, m, dev)

            anom = groups(kernel, np.empty(lead + maps.shape, dtype=np.float64))
            mean, den = hostio.to_host(mean_d), hostio.to_host(den_d)
        else:
            def kernel(tensors, i0, i1):
                _, m, d = stats(tensors, i0, i1)
                return torch.stack([m.reshape(i1 - i0, inner, ns), d.reshape(i1 - i0, inner, ns)],
                                   dim=1)

            both = groups(kernel, np.empty((lead[0], 2, inner, ns), dtype=np.float64))
            mean, den, anom = both[:, 0], both[:, 1], None
        return mean.reshape(lead + (ns,)), den.reshape(lead + (ns,)), anom

    # (a device record is read where it lives; only a host record goes through hostio)
    v = da.data.to(tdt) if on_device else engine.to_device(da.values, dev, tdt)
    v = v.reshape(nrec, plane).contiguous()
    mean, den = maps.mean(v, dev)
    anom = maps.anomaly(v, mean, dev).reshape(lead + maps.shape) if want_anomaly else None
    mean, den = mean.reshape(lead + (ns,)), den.reshape(lead + (ns,))
    if not on_device:
        mean, den = hostio.to_host(mean), hostio.to_host(den)
        anom = None if anom is None else hostio.to_host(anom)
    return mean, den, anom


def _labelled(da, maps, want_anomaly):
    """(mean, den, anomaly or None) of one DataArray as DataArrays"""
    mean, den, anom = _records(da, maps, want_anomaly)
    lead_dims = tuple(da.dims[:-2])
    coords = {k: c for k, c in da.coords.items() if set(c.dims) <= set(lead_dims)}
    if maps.ids is None:
        dims, mean, den = lead_dims, mean[..., 0], den[..., 0]
    else:
        dims = lead_dims + ("region",)
        coords["region"] = DataArray(maps.ids.copy(), ("region",), None, None, "region")
    attrs = {}
    if "long_name" in da.attrs:
        attrs["long_name"] = "Area-weighted mean of " + str(da.attrs["long_name"])
    if "units" in da.attrs:
        attrs["units"] = da.attrs["units"]
    attrs["cell_methods"] = "area: mean"
    m = DataArray(mean, dims, coords, attrs, da.name)
    m.encoding = dict(da.encoding)
    dattrs = {"long_name": "Valid area under the area-weighted mean"}
    if "units" in maps.src.attrs:
        dattrs["units"] = maps.src.attrs["units"]
    d = DataArray(den, dims, coords, dattrs, da.name)
    a = None
    if want_anomaly:
        aattrs = dict(da.attrs)
        if "long_name" in aattrs:
            aattrs["long_name"] = "Anomaly from the area-weighted mean of " + str(aattrs["long_name"])
        a = DataArray(anom, da.dims, dict(da.coords), aattrs, da.name)
        a.encoding = dict(da.encoding)
    return m, d, a


def _has_plane(da, maps):
    return all(d in da.dims for d in maps.dims)


def _numeric(da):
    return da.dtype.kind in "fiub"


@accepts_xarray
def area_mean(xobj, areacello, regions=None, region_ids=None, return_area=False):
    """Area-weighted, NaN-aware mean over the horizontal plane (EXTENSION: not in momlevel; in
    xarray ``xobj.weighted(areacello.fillna(0)).mean((ydim, xdim))``, parity unpinned -- the
    specification is the numpy restatement in the module docstring).

    ``areacello`` is the 2-D ``(ydim, xdim)`` cell area (float32 / float64, NaN = no weight,
    negative values a ``ValueError``); ``xobj`` a DataArray whose LAST two dims are those, with any
    leading dims, or a Dataset: every numeric variable with the two trailing dims is reduced, the
    others are left out.  float32 / float64 records are read as they are, integers as float64,
    float16 / long double refused; the result is float64.

    ``regions=None`` is one region of every cell.  Otherwise ``regions`` is an integer
    ``(ydim, xdim)`` label map (MOM6's ``basin``; a float map of whole numbers and NaN is cast):
    labels <= 0 and NaN belong to no region, and the result gains a trailing dim ``"region"`` whose
    coordinate holds ``region_ids`` -- default the sorted positive labels present; an explicit
    sequence fixes the order and may name absent labels (NaN rows); duplicates are a ``ValueError``.

    ``return_area=True`` returns ``(mean, den)``: ``den`` is the valid area each mean was taken
    over -- what a caller needs to combine tiles or regions: the combined mean is
    ``sum(mean * den) / sum(den)``.

    A device record gives device results and nothing crosses the host link; a large host or lazy
    record is uploaded in groups of whole leading rows.  The order of summation is fixed (no
    atomics): a record's means do not depend on the records around it or on that grouping."""
    maps = _Maps(areacello, regions, region_ids)
    if isinstance(xobj, DataArray):
        m, d, _ = _labelled(xobj, maps, False)
        return (m, d) if return_area else m
    if isinstance(xobj, Dataset):
        means, dens = Dataset(attrs=xobj.attrs), Dataset(attrs=xobj.attrs)
        for name, c in xobj.coords.items():
            if not set(c.dims) & set(maps.dims):
                means._set(name, c, is_coord=True)
                dens._set(name, c, is_coord=True)
        for name, var in xobj.data_vars.items():
            if _numeric(var) and _has_plane(var, maps):
                means[name], dens[name], _ = _labelled(var, maps, False)
        return (means, dens) if return_area else means
    raise TypeError("Input must be a DataArray or a Dataset")


@accepts_xarray
def area_anomaly(xobj, areacello, regions=None, region_ids=None, return_mean=False):
    """``xobj`` minus its area-weighted mean (EXTENSION, see area_mean): every cell minus the mean
    of ITS region and record, float64 (numpy's promotion of a float32 field minus a float64 mean),
    NaN in cells that belong to no region; the input's dims and coords.  The mean that is
    subtracted is bit for bit the one ``area_mean`` returns; ``return_mean=True`` returns
    ``(anomaly, mean)``.  In a Dataset, variables without the two trailing dims pass through and
    non-numeric ones are skipped.  A large host or lazy record goes up and comes back in groups of
    whole leading rows."""
    maps = _Maps(areacello, regions, region_ids)
    if isinstance(xobj, DataArray):
        m, _, a = _labelled(xobj, maps, True)
        return (a, m) if return_mean else a
    if isinstance(xobj, Dataset):
        anoms, means = Dataset(attrs=xobj.attrs), Dataset(attrs=xobj.attrs)
        for name, c in xobj.coords.items():
            anoms._set(name, c, is_coord=True)
            if not set(c.dims) & set(maps.dims):
                means._set(name, c, is_coord=True)
        for name, var in xobj.data_vars.items():
            if not _numeric(var):
                continue
            if _has_plane(var, maps):
                means[name], _, anoms[name] = _labelled(var, maps, True)
            else:
                anoms[name] = var
        return (anoms, means) if return_mean else anoms
    raise TypeError("Input must be a DataArray or a Dataset")
