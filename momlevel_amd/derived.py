"""derived.py -- the reference's ``momlevel.derived`` hot subset on the MI355X.

Same signatures as src/momlevel/derived.py: ``calc_rho`` (:597-639), ``calc_masso``
(:414-444), ``calc_volo`` (:769-795), ``calc_rhoga`` (:642-666), ``calc_dz``
(:249-325), plus ``calc_alpha`` / ``calc_beta`` (:74-159) which reuse the EOS
kernel, and their consumers: ``calc_n2`` (:328-411),
``calc_stability_angle`` (:714-766), ``adjust_negative_n2`` (:30-71) and
``calc_wave_speed`` (:798-831), each ONE pass of a HIP kernel of its own
(csrc/momlevel_strat.hip) over what the reference evaluates as dozens of numpy passes; and the
C-grid group ``calc_rel_vort`` (:187-246), ``calc_pv`` (:489-565), ``calc_rossby_rd`` (:568-594)
on the stencil kernels of csrc/momlevel_vort.hip, with ``calc_coriolis`` (:162-184).  Inputs and outputs are labelled arrays (momlevel_amd.labeled, or xarray
objects when xarray is installed -- see adapters.py); every number comes from a
HIP kernel.
"""

import numpy as np
import torch

from . import core, engine, hostio, spice, util
from .adapters import accepts_xarray
from .labeled import DataArray, as_plain, check_field_dtype, is_lazy
from .steric import OHC_CP

__all__ = [
    "adjust_negative_n2",
    "calc_alpha",
    "calc_beta",
    "calc_coriolis",
    "calc_dz",
    "calc_heat_content",
    "calc_isopycnal_depth",
    "calc_isosurface_depth",
    "calc_layer_integral",
    "calc_masso",
    "calc_mld",
    "calc_n2",
    "calc_pdens",
    "calc_pv",
    "calc_rel_vort",
    "calc_rho",
    "calc_rhoga",
    "calc_rossby_rd",
    "calc_spice",
    "calc_stability_angle",
    "calc_volo",
    "calc_wave_speed",
    "layer_bounds",
]


def _broadcast_dims(*arrays):
    """Union of dims in first-appearance order (xarray's apply_ufunc rule)."""
    dims = []
    for a in arrays:
        for d in a.dims:
            if d not in dims:
                dims.append(d)
    return tuple(dims)


def _expand_to(da, dims, sizes):
    """Raw data of ``da`` reshaped/transposed so it broadcasts against ``dims``."""
    data = da.data
    order = [d for d in dims if d in da.dims]
    perm = [da.dims.index(d) for d in order]
    if da.is_lazy:  # a dask / netCDF4-like field
        if tuple(da.dims) == tuple(dims):
            return data  # already laid out like the result: read piece by piece (eos/_dispatch.py)
        data = da.values  # (reads all of it; masked elements of a netCDF4 read become NaN)
    if perm != list(range(len(perm))):
        data = data.permute(*perm) if isinstance(data, torch.Tensor) else data.transpose(perm)
    shape = [sizes[d] if d in da.dims else 1 for d in dims]
    return data.reshape(shape)


def _apply_eos(func_name, thetao, so, pres, eos, eos_func=None):
    """xr.apply_ufunc(eos_func, thetao, so, pres) restated: broadcast by dim name."""
    if eos_func is None:
        eos_func = util.eos_func_from_str(eos, func_name=func_name)
    # python floats / ints stay python scalars (xr.apply_ufunc hands them through): numpy lets them
    # take the dtype of the arrays they meet -- calc_pdens' pressure on float32 fields
    weak = [isinstance(a, (bool, int, float)) and not isinstance(a, np.generic)
            for a in (thetao, so, pres)]
    args = [a if (isinstance(a, DataArray) or w) else DataArray(np.asarray(a), ())
            for a, w in zip((thetao, so, pres), weak)]
    arrays = [a for a, w in zip(args, weak) if not w]
    dims = _broadcast_dims(*arrays)
    sizes = {}
    for a in arrays:
        sizes.update(a.sizes)
    raw = [a if w else _expand_to(a, dims, sizes) for a, w in zip(args, weak)]
    out = eos_func(*raw)
    if not arrays:  # python scalars only: a 0-d result
        return DataArray(np.asarray(out), ())
    coords = {}
    for a in arrays:
        coords.update(a.coords)
    return DataArray(out, dims, {k: v for k, v in coords.items() if set(v.dims) <= set(dims)})


@accepts_xarray
def calc_rho(thetao, so, pres, eos="Wright"):
    """In situ density from potential temperature, salinity and pressure (derived.py:597-639)."""
    rho = _apply_eos("density", thetao, so, pres, eos)
    rho.attrs = {
        "standard_name": "sea_water_density",
        "long_name": "In situ sea water density",
        "comment": f"calculated with the {eos} equation of state",
        "units": "kg m-3",
    }
    return rho


@accepts_xarray
def calc_pdens(thetao, so, level=0.0, patm=101325, eos="Wright"):
    """Potential density referenced to depth ``level`` (p = level*1e4 + patm) (derived.py:447-486)."""
    assert 0.0 <= level <= 7500.0, "specified level must be between 0 and 7500 m"
    rhopot = _apply_eos("density", thetao, so, (level * 1.0e4) + patm, eos)
    rhopot.attrs = {
        "standard_name": "sea_water_potential_density",
        "long_name": f"Sea water potential density referenced to {level} m",
        "comment": f"calculated with the {eos} equation of state",
        "units": "kg m-3",
    }
    return rhopot


def _broadcast_full(raw, shape):
    """``raw`` (an array, tensor or lazy source that broadcasts against ``shape``) at ``shape``"""
    if tuple(raw.shape) == tuple(shape):
        return raw
    return raw.expand(shape) if isinstance(raw, torch.Tensor) else np.broadcast_to(raw, shape)


@accepts_xarray
def calc_spice(thetao, so):
    """Sea water spiciness after Flament (2002) (derived.py:669-711): thetao in deg C, so in PSU,
    broadcast against each other by dimension name."""
    args = [a if isinstance(a, DataArray) else DataArray(np.asarray(a), ()) for a in (thetao, so)]
    dims = _broadcast_dims(*args)
    sizes = {}
    for a in args:
        sizes.update(a.sizes)
    shape = tuple(sizes[d] for d in dims)
    # spice.flament.spice takes equal shapes only: each field is expanded to the common one
    raw = [_broadcast_full(_expand_to(a, dims, sizes), shape) for a in args]
    out = spice.flament.spice(*raw)
    coords = {}
    for a in args:
        coords.update(a.coords)
    pi = DataArray(out, dims, {k: v for k, v in coords.items() if set(v.dims) <= set(dims)})
    pi.attrs = {
        "long_name": "Sea water spiciness",
        "comment": "calculated based on Flament 2002 methodology",
        "units": "1",
    }
    return pi


@accepts_xarray
def calc_alpha(thetao, so, pres, eos="Wright"):
    """Thermal expansion coefficient (derived.py:74-115)."""
    alpha = _apply_eos("alpha", thetao, so, pres, eos)
    alpha.attrs = {
        "long_name": "Thermal expansion coefficient",
        "comment": f"calculated with the {eos} equation of state",
        "units": "degC-1",
    }
    return alpha


@accepts_xarray
def calc_beta(thetao, so, pres, eos="Wright"):
    """Haline contraction coefficient (derived.py:118-159)."""
    beta = _apply_eos("beta", thetao, so, pres, eos)
    beta.attrs = {
        "long_name": "Haline contraction coefficient",
        "comment": f"calculated with the {eos} equation of state",
        "units": "PSU-1",
    }
    return beta


@accepts_xarray
def calc_masso(rho, volcello, tcoord="time"):
    """Total ocean mass: sum(rho*volcello) over every non-time dim, skipna (derived.py:414-444)."""
    dims = _broadcast_dims(rho, volcello)
    sizes = dict(volcello.sizes)
    sizes.update(rho.sizes)
    has_t = tcoord in dims
    inner_dims = tuple(d for d in dims if d != tcoord)
    inner = tuple(sizes[d] for d in inner_dims)
    nt = sizes[tcoord] if has_t else 1
    dev = engine.device_of(rho.data, volcello.data)

    def canon(da, with_time):
        order = ((tcoord,) if with_time else ()) + inner_dims
        raw = _expand_to(da, order, sizes)
        raw = engine.to_device(raw, dev, torch.float64)
        full = ((nt,) if with_time else ()) + inner
        return raw.expand(full).contiguous().reshape((nt, -1) if with_time else (-1,))

    r = canon(rho, has_t)
    if not has_t:
        r = r.reshape(1, -1)
    v = canon(volcello, tcoord in volcello.dims)
    out = core.masso(r, v)
    data = out if has_t else out[0]
    if not (rho.is_device or volcello.is_device):
        data = hostio.to_host(data)
    masso = DataArray(data, (tcoord,) if has_t else (),
                      {tcoord: rho.coords[tcoord]} if has_t and tcoord in rho.coords else None)
    masso.attrs = {
        "standard_name": "sea_water_mass",
        "long_name": "Sea Water Mass",
        "units": "kg",
    }
    return masso


@accepts_xarray
def calc_volo(volcello):
    """Total ocean volume: skipna sum of a 3-D volcello (derived.py:769-795)."""
    assert len(volcello.dims) == 3, "Expecting only 3 dimensions for volcello"
    dev = engine.device_of(volcello.data)
    total = core.nansum(engine.to_device(volcello.data, dev, torch.float64))
    # numpy's sum of a float32 field is a float32: the float64 sum of the same values (mlx_nansum),
    # rounded ONCE -- closer to the exact sum than numpy's own float32 accumulation
    if engine.sum_dtype(volcello.data) == np.float32:
        total = total.to(torch.float32)
    volo = DataArray(total if volcello.is_device else hostio.to_host(total), ())
    volo.attrs = {
        "standard_name": "sea_water_volume",
        "long_name": "Sea Water Volume",
        "units": "m3",
    }
    return volo


@accepts_xarray
def calc_rhoga(masso, volo):
    """Global average ocean density masso/volo (derived.py:642-666); host scalars."""
    rhoga = masso / volo
    rhoga.attrs = {
        "long_name": "Global Average Sea Water Density",
        "units": "kg m-3",
    }
    return rhoga


@accepts_xarray
def calc_dz(levels, interfaces, depth, top=0.0, bottom=None, fraction=False):
    """dz with partial bottom cells (derived.py:249-325); dims (z, y, x)."""
    # sign checks stay on the host (derived.py:284-292)
    assert bool(np.all(np.nan_to_num(depth.values, nan=0.0) >= 0)), (
        "Depth values must all be positive-definite"
    )
    assert bool(np.all(levels.values >= 0)), (
        "Vertical coordinate levels must all be positive-definite"
    )
    assert bool(np.all(interfaces.values >= 0)), (
        "Vertical coordinate interfaces must all be positive-definite"
    )
    dev = engine.device_of(depth.data)
    out = core.calc_dz(
        engine.to_device(interfaces.data, dev, torch.float64),
        engine.to_device(depth.data, dev, torch.float64).contiguous(),
        top=top, bottom=bottom, fraction=fraction,
    )
    zdim = levels.dims[0]
    coords = dict(depth.coords)
    coords[zdim] = levels.coords.get(zdim, levels)
    return DataArray(out if depth.is_device else hostio.to_host(out), (zdim,) + depth.dims, coords)


# ---------------------------------------------------------------------------------------
# stratification: the consumers of alpha / beta (csrc/momlevel_strat.hip)
# ---------------------------------------------------------------------------------------
def _z_layout(da, zcoord):
    """(index of zcoord, nt, nz, plane): the field seen as (nt, nz, plane), z the middle axis."""
    if zcoord not in da.dims:
        raise ValueError(f"{zcoord!r} is not a dimension of the field (dims {da.dims})")
    zi = da.dims.index(zcoord)
    shape = tuple(int(v) for v in da.shape)
    return zi, int(np.prod(shape[:zi], dtype=np.int64)), shape[zi], int(np.prod(shape[zi + 1:], dtype=np.int64))


def _level_values(da, zcoord):
    if zcoord not in da.coords:
        raise ValueError(f"the field has no coordinate values for {zcoord!r}")
    return np.asarray(da.coords[zcoord].values)


def _strat_pressure(pres, like, zcoord, dev, f32_fields):
    """The pressure operand of alpha / beta as core.stratification takes it.  float32 fields need
    a float64 pressure ARRAY: with a python float or a float32 array numpy evaluates alpha in
    float32 (eos/_dispatch.py), which this kernel does not restate."""
    if isinstance(pres, DataArray):
        if f32_fields and str(pres.dtype) != "float64":
            raise TypeError("float32 thetao/so need a float64 pressure (numpy evaluates alpha and "
                            f"beta in float32 against a {pres.dtype} one): convert it")
        if not set(pres.dims) <= set(like.dims):
            raise ValueError(f"pressure dims {pres.dims} are not dims of the field {like.dims}")
        zi, nt, nz, plane = _z_layout(like, zcoord)
        if pres.dims == (zcoord,):
            return engine.to_device(pres.data, dev, torch.float64).reshape(nz)
        if pres.dims == ():
            return engine.to_device(pres.data, dev, torch.float64).reshape(1)
        sizes = dict(like.sizes)
        raw = engine.to_device(_expand_to(pres, like.dims, sizes), dev, torch.float64)
        if zi > 0 and all(d not in pres.dims for d in like.dims[:zi]):  # no leading (time) dims
            return raw.reshape(raw.shape[zi:]).expand(tuple(like.shape[zi:])).contiguous().reshape(nz, plane)
        return raw.expand(tuple(like.shape)).contiguous().reshape(nt, nz, plane)
    if f32_fields:
        raise TypeError("float32 thetao/so need a float64 pressure array (numpy evaluates alpha and "
                        "beta in float32 against a python float): pass a DataArray")
    return float(pres)


def _stratification(func, thetao, so, pres, eos, zcoord, gravity=-9.8):
    if tuple(so.dims) != tuple(thetao.dims) or tuple(so.shape) != tuple(thetao.shape):
        raise ValueError(f"thetao {thetao.dims}{tuple(thetao.shape)} and so {so.dims}{tuple(so.shape)} "
                         "must share dims and shape")
    if str(thetao.dtype) != str(so.dtype):
        raise TypeError("thetao and so of different dtypes: convert one of them")
    if str(thetao.dtype) not in ("float32", "float64"):
        raise TypeError(f"thetao/so must be float32 or float64, not {thetao.dtype}")
    f32 = str(thetao.dtype) == "float32"
    if f32 and eos.lower() == "linear":
        raise TypeError("the linear EOS on float32 fields is float32 throughout in numpy: "
                        "convert the fields to float64")
    util.eos_func_from_str(eos, func_name="alpha")  # unknown EOS: the reference's ValueError
    zi, nt, nz, plane = _z_layout(thetao, zcoord)
    z = _level_values(thetao, zcoord)
    if f32 and str(z.dtype) == "float32":
        # numpy.gradient takes its coefficients from the coordinate IN THE COORDINATE'S dtype: with a
        # float32 z and float32 fields the edge rows (every row of an uneven grid) are float32
        # arithmetic, and calc_n2's own pressure `thetao[zcoord] * 1e4 + patm` is float32 too, so
        # that numpy evaluates alpha, beta and N^2 in float32 throughout.  The kernel forms the
        # derivative in float64 and rounds once: not numpy's bits -- refused, like a
        # float32 pressure on float32 fields.
        raise TypeError(f"float32 thetao/so with a float32 {zcoord!r} coordinate: numpy would "
                        "differentiate (and calc_n2 build its pressure) in float32, which no kernel "
                        "here restates; convert the coordinate to float64")
    dev = engine.device_of(thetao.data, so.data)
    dt = torch.float32 if f32 else torch.float64
    p = None if eos.lower() == "linear" else _strat_pressure(pres, thetao, zcoord, dev, f32)
    kw = dict(func=func, eos=eos.lower(), gravity=gravity)
    on_device = thetao.is_device or so.is_device
    if not on_device and hostio.wants_pipeline(nt, nt * nz * plane):
        out = _stratification_host_rows(thetao.data, so.data, p, z, nt, nz, plane, dev,
                                        lead=nt if zi == 1 else None, **kw)
        return DataArray(out.reshape(tuple(thetao.shape)), thetao.dims, dict(thetao.coords))
    T = engine.to_device(thetao.data, dev, dt).reshape(nt, nz, plane)
    S = engine.to_device(so.data, dev, dt).reshape(nt, nz, plane)
    out = core.stratification(T, S, p, z, **kw).reshape(tuple(thetao.shape))
    return DataArray(out if on_device else hostio.to_host(out), thetao.dims, dict(thetao.coords))


def _stratification_host_rows(T, S, p, z, nt, nz, plane, dev, lead=None, **kw):
    """core.stratification on host fields seen as (nt, nz, plane), group of rows by group
    (hostio.pipeline_rows: rows are independent, the derivative runs along z).  ``lead``: the
    fields are (lead, nz, ...) with ONE dimension before z (the usual (time, z, y, x)): they are
    then sliced along it as they are -- a lazy field is read group by group and never materialised
    whole.  (A pressure that varies from row to row -- ``p`` of shape (nt, nz, plane) -- IS
    resident whole: _strat_pressure expanded it before the groups start; only theta/S and the
    result are streamed.)"""
    if lead is not None:
        Tn, Sn = T, S  # sliced along their own leading axis
    else:
        Tn = hostio.as_plain(T[...] if is_lazy(T) else T).reshape(nt, nz, plane)
        Sn = hostio.as_plain(S[...] if is_lazy(S) else S).reshape(nt, nz, plane)
    p_rows = isinstance(p, torch.Tensor) and p.dim() == 3  # a pressure that varies from row to row

    def kernel(tensors, i0, i1):
        Td, Sd = tensors
        return core.stratification(Td.reshape(i1 - i0, nz, plane), Sd.reshape(i1 - i0, nz, plane),
                                   p[i0:i1] if p_rows else p, z, **kw)

    return hostio.pipeline_rows(hostio.row_bounds(nt, nz * plane), dev, hostio.leading_slices([Tn, Sn]),
                                kernel, np.empty((nt, nz, plane), dtype=np.float64))


@accepts_xarray
def calc_n2(thetao, so, eos="Wright", gravity=-9.8, patm=101325.0, zcoord="z_l", interfaces=None,
            adjust_negative=False):
    """Buoyancy frequency N^2 at the cell centres (derived.py:328-411):
    ``gravity * ((alpha * dT/dz) - (beta * dS/dz))`` with alpha, beta at
    ``p = thetao[zcoord] * 1e4 + patm`` and d/dz = ``differentiate(zcoord, edge_order=2)``.
    ``interfaces`` (the cell-edge variant) interpolates with xgcm's ``Grid.transform`` in the
    reference: not built.  Deviations, deliberate: ``adjust_negative=True`` forwards ``zcoord``
    (the reference calls ``adjust_negative_n2(n2)`` with its default "z_l", derived.py:409, and so
    fails on any other name); float32 fields need a float64 coordinate (TypeError otherwise, see
    _stratification)."""
    if interfaces is not None:
        raise NotImplementedError("calc_n2(interfaces=...) needs xgcm's linear vertical transform "
                                  "(derived.py:389-394): not built; pass interfaces=None")
    z = DataArray(_level_values(thetao, zcoord).astype(np.float64), (zcoord,))
    pres = (z * 1.0e4) + patm  # derived.py:396
    n2 = _stratification("n2", thetao, so, pres, eos, zcoord, gravity=gravity)
    n2.attrs = {
        "standard_name": "square_of_brunt_vaisala_frequency_in_sea_water",
        "long_name": "Square of seawater buoyancy frequency",
        "units": "s-2",
    }
    return adjust_negative_n2(n2, zcoord=zcoord) if adjust_negative else n2


@accepts_xarray
def calc_stability_angle(thetao, so, pres, eos="Wright", zcoord="z_l"):
    """Stability (Turner) angle in degrees (derived.py:714-766)."""
    result = _stratification("turner", thetao, so, pres, eos, zcoord)
    result.name = "tu_angle"
    result.attrs = {
        "long_name": "Stability angle",
        "units": "degrees",
    }
    return result


def _adjust(n2, zcoord, dz=None, want_adjusted=True):
    zi, nt, nz, plane = _z_layout(n2, zcoord)
    # `adjusted[0]` (derived.py:62) indexes the LEADING dimension: the rows of the (nt, nz, plane)
    # view whose index along it is 0 -- all nt // size0 of them -- unless z leads
    lead0_rows = 0 if zi == 0 else nt // int(n2.shape[0])
    dev = engine.device_of(n2.data)
    x = engine.to_device(n2.data, dev, torch.float64).reshape(nt, nz, plane)
    dzt = None
    if dz is not None:
        if tuple(dz.dims) != tuple(n2.dims[zi:]) or tuple(dz.shape) != tuple(n2.shape[zi:]):
            raise ValueError(f"dz {dz.dims}{tuple(dz.shape)} must cover the field's "
                             f"{n2.dims[zi:]}{tuple(n2.shape[zi:])}")
        dzt = engine.to_device(dz.data, dev, torch.float64).reshape(nz, plane)
    adjusted, speed = core.adjust_negative_n2(x, lead0_rows, dz=dzt, want_adjusted=want_adjusted)
    return adjusted, speed, (zi, nt, nz, plane), x


@accepts_xarray
def adjust_negative_n2(n2, zcoord="z_l"):
    """Remove negative N^2 after Chelton et al. 1998 (derived.py:30-71): non-positive values
    become NaN, NaN at index 0 OF THE LEADING DIMENSION becomes 1e-8 (the reference writes
    ``adjusted[0]``: the first time step of a (time, z, y, x) field, the surface of a (z, y, x)
    one), the rest is forward-filled down the column, the original NaN mask is put back.
    Deviation: the result is float64 whatever ``n2``'s dtype (the reference keeps a float32 n2
    float32 and writes float32(1e-8)); ``zcoord`` is an addition (the reference ffills "z_l")."""
    adjusted, _, _, _ = _adjust(n2, zcoord)
    adjusted = adjusted.reshape(tuple(n2.shape))
    out = DataArray(adjusted if n2.is_device else hostio.to_host(adjusted), n2.dims, dict(n2.coords))
    out.attrs = {**n2.attrs, "comment": "adjustment applied for negative values"}
    return out


@accepts_xarray
def calc_wave_speed(n2, dz, zcoord="z_l"):
    """Gravity wave speed of the first baroclinic mode (derived.py:798-831):
    ``(sqrt(adjust_negative_n2(n2)) * dz).sum(zcoord) / pi``, NaN where ``n2[0]`` is null.  As in
    the reference ``n2[0]`` indexes the leading dimension: for a (z, y, x) field it is the surface
    and the result has dims (y, x); for a (time, z, y, x) field it is the first TIME STEP, dims
    (z, y, x), which xarray broadcasts against the (time, y, x) speeds into (z, y, x, time) -- the
    array whose sum the reference's own test holds (tests/test_derived.py:147-151).  float64 out
    whatever the dtype of ``n2`` (see adjust_negative_n2)."""
    _, speed, (zi, nt, nz, plane), x = _adjust(n2, zcoord, dz=dz, want_adjusted=False)
    trail_dims, trail_shape = tuple(n2.dims[zi + 1:]), tuple(n2.shape[zi + 1:])
    host = not n2.is_device
    if zi == 0:
        data = speed.reshape(trail_shape)
        result = DataArray(hostio.to_host(data) if host else data, trail_dims,
                           {k: v for k, v in n2.coords.items() if set(v.dims) <= set(trail_dims)})
    elif zi == 1:
        data = core.wave_speed_where_time0(x[0], speed).reshape((nz,) + trail_shape + (nt,))
        dims = (zcoord,) + trail_dims + (n2.dims[0],)
        result = DataArray(hostio.to_host(data) if host else data, dims, dict(n2.coords))
    else:
        raise NotImplementedError("calc_wave_speed: more than one dimension before "
                                  f"{zcoord!r} (dims {n2.dims})")
    result.attrs = {
        "long name": "Ocean gravity wave speed of the first baroclinic mode",
        "units": "m s-1",
    }
    return result


# ---------------------------------------------------------------------------------------
# vorticity on the staggered (C) grid: the stencils of csrc/momlevel_vort.hip
# ---------------------------------------------------------------------------------------
_COORD_KEYS = ("xcenter", "ycenter", "xcorner", "ycorner")


def _coord_names(coord_dict):
    """the four dimension names of util.get_xgcm_grid (util.py:424-430); the grid object itself is
    not built (no xgcm): the names say which dimension is which"""
    if coord_dict is None:
        return {"xcenter": "xh", "ycenter": "yh", "xcorner": "xq", "ycorner": "yq"}
    missing = [k for k in _COORD_KEYS if k not in coord_dict]
    if missing:
        raise ValueError(f"coord_dict is missing the keys {missing}")
    return {k: coord_dict[k] for k in _COORD_KEYS}


def float_name(da, what, allow_other=False):
    """"float32" / "float64"; float16, long double (check_field_dtype) and, unless
    ``allow_other``, everything that is not a float are refused"""
    name = check_field_dtype(da.dtype, what)
    if name not in ("float32", "float64"):
        if not allow_other:
            raise TypeError(f"{what} must be float32 or float64, not {name}")
        name = "float64"
    return name


def check_trailing(da, ydim, xdim, what):
    if len(da.dims) < 2 or tuple(da.dims[-2:]) != (ydim, xdim):
        raise ValueError(f"{what} has dims {da.dims}: its last two must be ({ydim!r}, {xdim!r}), "
                         "in that order")


def _corner_extents(sizes, names, symmetric, what):
    """(ny, nx) of the corner plane after checking centre against corner lengths"""
    s = int(bool(symmetric))
    for c, q in (("ycenter", "ycorner"), ("xcenter", "xcorner")):
        nc, nq = sizes.get(names[c]), sizes.get(names[q])
        if nc is not None and nq is not None and nq != nc + s:
            raise ValueError(
                f"{what}: {names[q]!r} has {nq} points and {names[c]!r} has {nc}; a "
                f"{'symmetric' if s else 'non-symmetric'} grid needs {nc + s} corner points "
                f"(symmetric={bool(symmetric)})")
    return sizes[names["ycorner"]], sizes[names["xcorner"]]


def _raw(da):
    """numpy (a lazy source is read whole) or the device tensor"""
    return da.data if da.is_device else da.values


def _records(x, dev, dtype, nrec, tail):
    return engine.to_device(x, dev, dtype).reshape((nrec,) + tuple(tail)).contiguous()


def _stencil(fields, lead_shape, out_tail, out_np_dtype, dev, on_device, kernel):
    """``kernel(tensors)`` on the (nrec, y, x) views of ``fields`` (labelled arrays that share
    ``lead_shape``), whole or -- large host / lazy fields with more than one leading row -- in
    groups of whole leading rows (hostio.pipeline_rows).  Returns the raw result at
    lead_shape + out_tail: host in, host out."""
    shape = tuple(lead_shape) + tuple(out_tail)
    nrec = int(np.prod(lead_shape, dtype=np.int64))
    tdt = [torch.float32 if str(f.dtype) == "float32" else torch.float64 for f in fields]

    def views(tensors, n):
        return [t.reshape((n,) + tuple(f.shape[-2:])) for t, f in zip(tensors, fields)]

    if (not on_device and len(lead_shape) >= 1
            and hostio.wants_pipeline(lead_shape[0], int(np.prod(shape, dtype=np.int64)))):
        inner = int(np.prod(lead_shape[1:], dtype=np.int64))
        bounds = hostio.row_bounds(lead_shape[0], int(np.prod(shape[1:], dtype=np.int64)))
        sources = [f.data if f.is_lazy else f.values for f in fields]
        return hostio.pipeline_rows(
            bounds, dev, hostio.leading_slices(sources),
            lambda tensors, i0, i1: kernel(views([t.to(d) for t, d in zip(tensors, tdt)],
                                                 (i1 - i0) * inner)),
            np.empty(shape, dtype=out_np_dtype))
    tensors = [_records(_raw(f), dev, d, nrec, f.shape[-2:]) for f, d in zip(fields, tdt)]
    res = kernel(tensors).reshape(shape)
    return res if on_device else hostio.to_host(res)


@accepts_xarray
def calc_coriolis(lat):
    """Coriolis parameter ``2 (2 pi / 86400) sin(lat pi / 180)`` (derived.py:162-184).  Evaluated
    by numpy ON THE HOST: a 2-D field computed once per grid, and the bits of libm's ``sin`` cannot
    be pinned on the device.  A device-resident ``lat`` is downloaded and the result returned on
    its device."""
    if not isinstance(lat, DataArray):
        lat = DataArray(np.asarray(lat))
    values = lat.values
    coriolis = 2.0 * (2.0 * np.pi / (60.0 * 60.0 * 24.0)) * np.sin(values * np.pi / 180.0)
    data = engine.to_device(coriolis, lat.data.device) if lat.is_device else coriolis
    return DataArray(data, lat.dims, dict(lat.coords), {
        "standard_name": "coriolis_parameter",
        "long_name": "Coriolis parameter",
        "units": "s-1",
    }, None)


@accepts_xarray
def calc_rel_vort(dset, varname_map=None, coord_dict=None, symmetric=False):
    """Vertical component of the relative vorticity on the corner points (derived.py:187-246):
    ``( -diff_y(uo * dxCu) + diff_x(vo * dyCv) ) / areacello_bu`` with xgcm's zero-filled
    differences, ONE pass of core.rel_vort.  ``coord_dict`` names the four horizontal dimensions
    (the keys of util.get_xgcm_grid).  The two horizontal dimensions must be the last two of each
    field, y then x; ``uo`` and ``vo`` share a dtype (float32 or float64), the three metrics too."""
    if varname_map is None:
        varname_map = {"u": "uo", "v": "vo", "dx": "dxCu", "dy": "dyCv", "area": "areacello_bu"}
    missing = list(set(varname_map.values()) - set(dset.variables))
    if len(missing) > 0:
        raise ValueError(f"Input dataset missing fields: {missing}")
    names = _coord_names(coord_dict)
    u, v, dx, dy, area = (dset[varname_map[k]] for k in ("u", "v", "dx", "dy", "area"))
    yc, xc, yq, xq = names["ycenter"], names["xcenter"], names["ycorner"], names["xcorner"]
    check_trailing(u, yc, xq, varname_map["u"])
    check_trailing(v, yq, xc, varname_map["v"])
    for m, dims, what in ((dx, (yc, xq), varname_map["dx"]), (dy, (yq, xc), varname_map["dy"]),
                          (area, (yq, xq), varname_map["area"])):
        if tuple(m.dims) != dims:
            raise ValueError(f"{what} has dims {m.dims}: expected {dims}")
    if tuple(u.dims[:-2]) != tuple(v.dims[:-2]) or tuple(u.shape[:-2]) != tuple(v.shape[:-2]):
        raise ValueError(f"{varname_map['u']} {u.dims}{tuple(u.shape)} and {varname_map['v']} "
                         f"{v.dims}{tuple(v.shape)} must share their leading dims")
    sizes = {}
    for a in (u, v, dx, dy, area):
        for d, n in zip(a.dims[-2:], a.shape[-2:]):
            if sizes.setdefault(d, n) != n:
                raise ValueError(f"{d!r} has {n} points in one field and {sizes[d]} in another")
    ny, nx = _corner_extents(sizes, names, symmetric, "calc_rel_vort")
    fdt = float_name(u, "velocity fields")
    if float_name(v, "velocity fields") != fdt:
        raise TypeError(f"{varname_map['u']} is {u.dtype} and {varname_map['v']} is {v.dtype}: "
                        "convert one of them")
    mdts = {float_name(m, "grid metrics") for m in (dx, dy, area)}
    if len(mdts) != 1:
        raise TypeError(f"{varname_map['dx']}, {varname_map['dy']} and {varname_map['area']} must "
                        f"share one dtype, not {sorted(mdts)}")
    mdt = mdts.pop()
    dev = engine.device_of(u.data, v.data, dx.data, dy.data, area.data)
    on_device = u.is_device or v.is_device
    mt = torch.float32 if mdt == "float32" else torch.float64
    dxd, dyd, aread = (engine.to_device(_raw(m), dev, mt).contiguous() for m in (dx, dy, area))
    out_dtype = np.float32 if (fdt, mdt) == ("float32", "float32") else np.float64
    out = _stencil([u, v], tuple(u.shape[:-2]), (ny, nx), out_dtype, dev, on_device,
                   lambda t: core.rel_vort(t[0], t[1], dxd, dyd, aread, symmetric=symmetric))
    dims = tuple(u.dims[:-2]) + (yq, xq)
    coords = {k: c for k, c in dset.coords.items() if set(c.dims) <= set(dims)}
    return DataArray(out, dims, coords, {
        "standard_name": "ocean_relative_vorticity",
        "long_name": "Ocean relative vorticity",
        "units": "s-1",
    })


@accepts_xarray
def calc_pv(zeta, coriolis, n2, gravity=9.8, coord_dict=None, symmetric=False, units="m",
            interp_n2=True):
    """Ocean potential vorticity ``(zeta + coriolis) * (n2 / gravity)`` (derived.py:489-565), N^2
    averaged to the corner points first (``interp_n2``: along x, then along y, zero-filled --
    xgcm's ``grid.interp(n2, axis=["X", "Y"], boundary="fill")``) inside the same pass of
    core.potential_vorticity.  ``units="cm"`` gives ``abs((pv / 100) * 1e14)``.  ``zeta`` and
    ``n2`` share their leading dims; ``gravity`` is a python float (it takes N^2's dtype)."""
    if units not in core.VORT_UNITS:
        raise ValueError(f"unknown units option `{units}`")
    names = _coord_names(coord_dict)
    yc, xc, yq, xq = names["ycenter"], names["xcenter"], names["ycorner"], names["xcorner"]
    interp = bool(interp_n2)
    if interp:
        check_trailing(zeta, yq, xq, "zeta")
        check_trailing(n2, yc, xc, "n2")
        if tuple(coriolis.dims) != (yq, xq):
            raise ValueError(f"coriolis has dims {coriolis.dims}: expected {(yq, xq)}")
    else:
        if len(zeta.dims) < 2 or tuple(n2.dims[-2:]) != tuple(zeta.dims[-2:]):
            raise ValueError(f"without interp_n2, n2 {n2.dims} must lie on the points of zeta "
                             f"{zeta.dims}")
        if tuple(coriolis.dims) != tuple(zeta.dims[-2:]):
            raise ValueError(f"coriolis has dims {coriolis.dims}: expected {tuple(zeta.dims[-2:])}")
    if tuple(zeta.dims[:-2]) != tuple(n2.dims[:-2]) or tuple(zeta.shape[:-2]) != tuple(n2.shape[:-2]):
        raise ValueError(f"zeta {zeta.dims}{tuple(zeta.shape)} and n2 {n2.dims}{tuple(n2.shape)} "
                         "must share their leading dims")
    if tuple(coriolis.shape) != tuple(zeta.shape[-2:]):
        raise ValueError(f"coriolis {tuple(coriolis.shape)} does not cover zeta's plane "
                         f"{tuple(zeta.shape[-2:])}")
    ny, nx = (int(n) for n in zeta.shape[-2:])
    if interp:
        sizes = {yq: ny, xq: nx, yc: int(n2.shape[-2]), xc: int(n2.shape[-1])}
        _corner_extents(sizes, names, symmetric, "calc_pv")
    elif tuple(n2.shape[-2:]) != (ny, nx):
        raise ValueError(f"n2 {tuple(n2.shape)} and zeta {tuple(zeta.shape)} differ in shape")
    zdt, ndt = float_name(zeta, "zeta"), float_name(n2, "n2")
    cdt = float_name(coriolis, "coriolis", allow_other=True)
    dev = engine.device_of(zeta.data, n2.data, coriolis.data)
    on_device = zeta.is_device or n2.is_device
    fd = engine.to_device(_raw(coriolis), dev,
                          torch.float32 if cdt == "float32" else torch.float64).contiguous()
    out_dtype = np.float32 if (zdt, cdt, ndt) == ("float32",) * 3 else np.float64
    out = _stencil([zeta, n2], tuple(zeta.shape[:-2]), (ny, nx), out_dtype, dev, on_device,
                   lambda t: core.potential_vorticity(t[0], fd, t[1], gravity=float(gravity),
                                                      interp=interp, symmetric=symmetric,
                                                      units=units))
    coords = dict(coriolis.coords)
    coords.update(zeta.coords)
    pv = DataArray(out, zeta.dims, {k: c for k, c in coords.items() if set(c.dims) <= set(zeta.dims)})
    pv.attrs = {
        "long_name": "Ocean potential vorticity",
        "units": "m-1 s-1" if units == "m" else "10^14 cm-1 s-1",
    }
    return pv


@accepts_xarray
def calc_rossby_rd(wave_speed, coriolis):
    """Rossby radius of deformation ``wave_speed / abs(coriolis)`` (derived.py:568-594), the
    Coriolis parameter broadcast by dimension name: its dims must be a contiguous run of
    ``wave_speed``'s -- (yh, xh) of (yh, xh), of (time, yh, xh) or of the (z_l, yh, xh, time) array
    calc_wave_speed returns for 4-D input.  IEEE division: at the equator the result is the
    ``inf`` / NaN numpy gives."""
    nd = len(coriolis.dims)
    start = None
    for k in range(len(wave_speed.dims) - nd + 1):
        if tuple(wave_speed.dims[k:k + nd]) == tuple(coriolis.dims):
            start = k
            break
    if start is None:
        raise ValueError(f"coriolis dims {coriolis.dims} are not a contiguous run of wave_speed's "
                         f"{wave_speed.dims}")
    if tuple(wave_speed.shape[start:start + nd]) != tuple(coriolis.shape):
        raise ValueError(f"coriolis {coriolis.dims}{tuple(coriolis.shape)} does not fit wave_speed "
                         f"{wave_speed.dims}{tuple(wave_speed.shape)}")
    shape = tuple(int(n) for n in wave_speed.shape)
    outer = int(np.prod(shape[:start], dtype=np.int64))
    plane = int(np.prod(shape[start:start + nd], dtype=np.int64))
    inner = int(np.prod(shape[start + nd:], dtype=np.int64))
    wdt = float_name(wave_speed, "wave_speed", allow_other=True)
    cdt = float_name(coriolis, "coriolis", allow_other=True)
    dev = engine.device_of(wave_speed.data, coriolis.data)
    c = engine.to_device(_raw(wave_speed), dev, torch.float32 if wdt == "float32" else torch.float64)
    f = engine.to_device(_raw(coriolis), dev, torch.float32 if cdt == "float32" else torch.float64)
    out = core.rossby_radius(c.contiguous().reshape(outer, plane, inner),
                             f.contiguous().reshape(plane)).reshape(shape)
    on_device = wave_speed.is_device or coriolis.is_device
    coords = dict(coriolis.coords)
    coords.update(wave_speed.coords)
    return DataArray(out if on_device else hostio.to_host(out), wave_speed.dims,
                     {k: v for k, v in coords.items() if set(v.dims) <= set(wave_speed.dims)},
                     {"long name": "Rossby radius of deformation", "units": "m"}, None)


# ---------------------------------------------------------------------------------------
# (..., z, y, x) fields seen as (records, z, plane): shared by the depth-layer sums and the column
# search
# ---------------------------------------------------------------------------------------
def _z_plane(field, zcoord, zi, depth=None):
    """(dims, shape) of the two horizontal dims behind ``zcoord``; with ``depth``: its plane"""
    hdims, hshape = tuple(field.dims[zi + 1:]), tuple(int(n) for n in field.shape[zi + 1:])
    if depth is not None:
        if len(hdims) != 2 or hshape != tuple(int(n) for n in depth.shape):
            raise ValueError(f"the field's dims behind {zcoord!r} are {hdims}{hshape}: expected "
                             f"depth's plane {tuple(depth.shape)}")
    elif len(hdims) != 2:
        raise ValueError(f"the field's dims behind {zcoord!r} are {hdims}{hshape}: two horizontal "
                         "dims are expected")
    return hdims, hshape


def _over_z_records(fields, zi, nout, dev, kernel):
    """``kernel(tensors)`` on the (records, nz, plane) device views of ``fields`` -- labelled
    float32 / float64 arrays of one shape ``lead + (nz, y, x)``, each kept in its own dtype (other
    dtypes compute as float64) -- where it returns ``(records, nout, plane)``  ->  the raw result of
    shape ``lead + (nout, y, x)``: a device tensor when a field lives on the device, else a host
    array.  A large host or lazy field goes up in groups of whole leading rows and is never
    materialised whole: a record's result depends on that record alone, so the grouping cannot show."""
    first = fields[0]
    shape_in = tuple(int(n) for n in first.shape)
    lead, nz, hshape = shape_in[:zi], shape_in[zi], shape_in[zi + 1:]
    nrec = int(np.prod(lead, dtype=np.int64))
    plane = int(np.prod(hshape, dtype=np.int64))
    shape = lead + (nout,) + hshape
    on_device = any(f.is_device for f in fields)
    dts = [torch.float32 if str(f.dtype) == "float32" else torch.float64 for f in fields]

    def run(tensors, n):
        return kernel([x.to(dt).reshape(n, nz, plane) for x, dt in zip(tensors, dts)])

    if not on_device and len(lead) >= 1 and hostio.wants_pipeline(lead[0], nrec * nz * plane):
        inner = nrec // lead[0]
        sources = [f.data if f.is_lazy else f.values for f in fields]
        return hostio.pipeline_rows(
            hostio.row_bounds(lead[0], inner * nz * plane), dev, hostio.leading_slices(sources),
            lambda tensors, i0, i1: run(tensors, (i1 - i0) * inner),
            np.empty(shape, dtype=np.float64))
    xs = [f.data if f.is_device else engine.to_device(f.values, dev, dt)
          for f, dt in zip(fields, dts)]
    out = run([x.contiguous() for x in xs], nrec).reshape(shape)
    return out if on_device else hostio.to_host(out)


# ---------------------------------------------------------------------------------------
# depth-layer sums (EXTENSION; csrc/momlevel_layer.hip)
# ---------------------------------------------------------------------------------------
def layer_bounds(layers):
    """The public spelling of depth layers -> ``(tops, bottoms)`` float64 arrays, a bottom of +inf
    meaning the sea floor.  Two spellings: a sequence of ``(top, bottom)`` pairs in the units of
    ``depth`` (``bottom=None``: the sea floor; pairs may overlap -- ``(0, 700)`` beside
    ``(0, 2000)``), or a flat sequence of edges ``[0, 700, 2000, None]``: consecutive layers.
    ``ValueError`` for negative or NaN bounds, ``bottom <= top``, a ``None`` anywhere but a last
    bottom, and an empty list."""
    items = list(layers) if layers is not None else []
    if not items:
        raise ValueError("layers is empty")

    def is_pair(item):
        return (not isinstance(item, (str, bytes)) and item is not None and np.ndim(item) == 1
                and len(item) == 2)

    if all(is_pair(item) for item in items):
        pairs = [(item[0], item[1]) for item in items]
    elif all(item is None or np.ndim(item) == 0 for item in items):
        if len(items) < 2:
            raise ValueError("a list of edges needs two entries at least")
        if any(e is None for e in items[:-1]):
            raise ValueError("None (the sea floor) can only be the last edge")
        pairs = list(zip(items[:-1], items[1:]))
    else:
        raise ValueError("layers must be (top, bottom) pairs or a flat sequence of edges")
    tops = np.empty(len(pairs), dtype=np.float64)
    bottoms = np.empty(len(pairs), dtype=np.float64)
    for l, (top, bottom) in enumerate(pairs):
        if top is None:
            raise ValueError(f"layer {l}: None (the sea floor) can only be a bottom")
        top = float(top)
        bottom = np.inf if bottom is None else float(bottom)
        if np.isnan(top) or np.isnan(bottom):
            raise ValueError(f"layer {l}: a bound is NaN")
        if top < 0 or bottom < 0:
            raise ValueError(f"layer {l}: bounds must not be negative")
        if bottom <= top:
            raise ValueError(f"layer {l}: bottom {bottom} is not below top {top}")
        tops[l], bottoms[l] = top, bottom
    return tops, bottoms


def _check_layers_in_cells(tops, bottoms, z_i):
    """calc_dz gives min(zbot - top, bottom - ztop), not bottom - top, where top and bottom both
    lie strictly inside ONE model cell (derived.py:311-318): refused, certainly not what was meant"""
    z = np.asarray(z_i, dtype=np.float64).reshape(-1)
    for l, (top, bottom) in enumerate(zip(tops, bottoms)):
        inside = (z[:-1] < top) & (top < z[1:]) & (z[:-1] < bottom) & (bottom < z[1:])
        if np.any(inside):
            k = int(np.argmax(inside))
            raise ValueError(f"layer {l} ({top}, {bottom}) lies strictly inside one model cell "
                             f"({z[k]}, {z[k + 1]}): calc_dz does not give bottom - top there")


def _layer_coords(tops, bottoms):
    nl = len(tops)
    return {
        "layer": DataArray(np.arange(nl, dtype=np.int64), ("layer",), None, None, "layer"),
        "layer_top": DataArray(np.asarray(tops, dtype=np.float64).copy(), ("layer",), None,
                               {"long_name": "Top of the depth layer"}, "layer_top"),
        "layer_bottom": DataArray(np.where(np.isinf(bottoms), np.nan, bottoms), ("layer",), None,
                                  {"long_name": "Bottom of the depth layer (NaN: the sea floor)"},
                                  "layer_bottom"),
    }


@accepts_xarray
def calc_layer_integral(field, interfaces, depth, layers, zcoord="z_l", scale=1.0, wet=None):
    """EXTENSION (not in momlevel): ``scale * (calc_dz(top, bottom) * field).sum(zcoord)`` for
    every depth layer of ``layers`` (see layer_bounds), NaN terms skipped, in one pass over the
    field -- the specification is the numpy restatement tests/layer_numpy.py.

    ``field``: a float32 / float64 DataArray (not a Dataset) with ``zcoord`` and the two horizontal
    dims of ``depth`` right behind it, any dims before; ``interfaces``: the nz+1 interface depths;
    ``depth`` ``(y, x)``, NaN = land (contributes 0); ``wet``: an optional ``(y, x)`` array, the
    result is NaN where it is NaN.  Returns float64 with dims ``lead... + ("layer", y, x)`` and the
    coordinates ``layer`` (0 .. nl-1), ``layer_top`` and ``layer_bottom`` (NaN: the sea floor).
    Device input gives device output; a large host or lazy field goes up in groups of whole
    leading rows and is never materialised whole.

    The layer thickness per cell is calc_dz's, bit for bit.  A layer whose top and bottom both lie
    strictly inside one model cell is a ``ValueError``: calc_dz returns
    ``min(zbot - top, bottom - ztop)`` there, not ``bottom - top``.  Where the SEA FLOOR and ``top``
    cut the same cell calc_dz does the same (``min(zbot - top, depth - ztop)``); that depends on
    the cell and cannot be refused -- parity with calc_dz is the contract."""
    if not isinstance(field, DataArray):
        raise TypeError("field must be a DataArray (a Dataset is not accepted)")
    float_name(field, "field")
    tops, bottoms = layer_bounds(layers)
    if not isinstance(depth, DataArray):
        depth = DataArray(depth)
    if depth.ndim != 2:
        raise ValueError(f"depth has dims {depth.dims}: a 2-D (y, x) field is expected")
    zi, nrec, nz, plane = _z_layout(field, zcoord)
    hdims, hshape = _z_plane(field, zcoord, zi, depth)
    z_i = np.asarray(interfaces.values if isinstance(interfaces, DataArray) else interfaces,
                     dtype=np.float64).reshape(-1)
    if z_i.size != nz + 1:
        raise ValueError(f"interfaces holds {z_i.size} values: {nz + 1} expected")
    depth_np = np.asarray(depth.values, dtype=np.float64)
    # calc_dz's sign checks stay on the host (derived.py:284-292)
    assert bool(np.all(np.nan_to_num(depth_np, nan=0.0) >= 0)), (
        "Depth values must all be positive-definite"
    )
    if zcoord in field.coords:
        assert bool(np.all(np.asarray(field.coords[zcoord].values) >= 0)), (
            "Vertical coordinate levels must all be positive-definite"
        )
    assert bool(np.all(z_i >= 0)), "Vertical coordinate interfaces must all be positive-definite"
    _check_layers_in_cells(tops, bottoms, z_i)
    if wet is not None:
        wet = wet.data if isinstance(wet, DataArray) else wet
        if tuple(int(n) for n in wet.shape) != hshape:
            raise ValueError(f"wet {tuple(wet.shape)} does not cover the plane {hshape}")

    dev = engine.device_of(field.data, depth.data)
    z_d = engine.to_device(z_i, dev, torch.float64)
    depth_d = engine.to_device(depth.data, dev, torch.float64).contiguous().reshape(-1)
    wet_d = None if wet is None else engine.to_device(wet, dev, torch.float64).contiguous().reshape(-1)
    nl = len(tops)
    out = _over_z_records(
        [field], zi, nl, dev,
        lambda xs: core.layer_integral(xs[0], z_d, depth_d, tops, bottoms, surface=wet_d, scale=scale))
    coords = {k: c for k, c in field.coords.items() if zcoord not in c.dims}
    coords.update(_layer_coords(tops, bottoms))
    return DataArray(out, tuple(field.dims[:zi]) + ("layer",) + hdims, coords, None, field.name)


@accepts_xarray
def calc_heat_content(thetao, interfaces, depth, layers=None, rhozero=1035.0, cp=OHC_CP,
                      zcoord="z_l", wet=None):
    """EXTENSION (not in momlevel): ocean heat content per unit area and depth layer relative to
    0 degC, ``rhozero * cp * sum_z(thetao * dz_l)`` in J m-2: calc_layer_integral with
    ``scale = float64(rhozero) * float64(cp)``.  ``layers=None`` is the whole column and the result
    has no ``layer`` dim."""
    whole = layers is None
    scale = float(np.float64(rhozero) * np.float64(cp))
    out = calc_layer_integral(thetao, interfaces, depth, [(0.0, None)] if whole else layers,
                              zcoord=zcoord, scale=scale, wet=wet)
    if whole:
        ax = out.dims.index("layer")
        data = out.data.reshape(out.shape[:ax] + out.shape[ax + 1:])
        coords = {k: c for k, c in out.coords.items() if "layer" not in c.dims}
        out = DataArray(data, out.dims[:ax] + out.dims[ax + 1:], coords, None, out.name)
    out.attrs.update({
        "long_name": "Ocean heat content per unit area relative to 0 degC (momlevel_amd extension)",
        "units": "J m-2",
        "comment": f"rhozero={rhozero} kg m-3 * cp={cp} J kg-1 K-1 * sum_z(thetao*dz)",
    })
    return out


# ---------------------------------------------------------------------------------------
# the column search: mixed layer, isotherm and isopycnal depths (EXTENSION; csrc/momlevel_column.hip)
# ---------------------------------------------------------------------------------------
def _first_record_level_means(field, zi, dev):
    """NaN-skipping mean of every level of the FIRST record of ``field``, on the host: one small
    device reduction (core.area_mean with unit areas over the (nz, plane) record)"""
    shape = tuple(int(n) for n in field.shape)
    nz, plane = shape[zi], int(np.prod(shape[zi + 1:], dtype=np.int64))
    dt = torch.float32 if str(field.dtype) == "float32" else torch.float64
    if field.is_device:
        rec = field.data.reshape((-1, nz, plane))[0].to(dt).contiguous()
    else:
        src = field.data if field.is_lazy else field.values
        rec = as_plain(src[(slice(0, 1),) * zi]) if zi else field.values  # one record is read
        rec = engine.to_device(np.ascontiguousarray(rec).reshape(nz, plane), dev, dt)
    mean, _ = core.area_mean(rec, torch.ones(plane, dtype=torch.float64, device=dev))
    return mean.reshape(-1).cpu().numpy()


def _column_depth(fields, values, zcoord, kref, mode, relative, miss, deptho, value_dim, attrs,
                  value_attrs=None, eos="wright", p_ref=0.0):
    """core.column_crossing on labelled ``fields`` ([field], or [thetao, so]: SIGMA source) ->
    a labelled float64 depth of dims ``lead + (value_dim, y, x)`` (``values`` a sequence) or
    ``lead + (y, x)`` (a scalar).  ``kref``: a level index, or a function of the level depths;
    ``mode``: "rise" | "fall" | "depart" | "auto" (rise or fall, from the first record)."""
    first = fields[0]
    for f, what in zip(fields, ("field", "so") if len(fields) == 1 else ("thetao", "so")):
        if not isinstance(f, DataArray):
            raise TypeError(f"{what} must be a DataArray (a Dataset is not accepted)")
        float_name(f, what, allow_other=True)
        if tuple(f.dims) != tuple(first.dims) or tuple(f.shape) != tuple(first.shape):
            raise ValueError(f"thetao {first.dims}{tuple(first.shape)} and so {f.dims}"
                             f"{tuple(f.shape)} must agree in dims and shape")
    zi, nrec, nz, plane = _z_layout(first, zcoord)
    if deptho is not None and not isinstance(deptho, DataArray):
        deptho = DataArray(deptho)
    if deptho is not None and deptho.ndim != 2:
        raise ValueError(f"deptho has dims {deptho.dims}: a 2-D (y, x) field is expected")
    hdims, _ = _z_plane(first, zcoord, zi, deptho)
    z = np.asarray(_level_values(first, zcoord), dtype=np.float64).reshape(-1)
    if z.size != nz or np.isnan(z).any() or not np.all(np.diff(z) > 0):
        raise ValueError(f"the levels of {zcoord!r} must increase strictly (depth, positive down)")
    scalar = np.ndim(values) == 0
    vals = np.atleast_1d(np.asarray(values, dtype=np.float64)).reshape(-1)
    if vals.size < 1 or np.isnan(vals).any():
        raise ValueError("values must hold one number at least and no NaN")
    if relative and not np.all(vals > 0):
        raise ValueError("a threshold relative to the reference level must be > 0")
    kref = int(kref(z)) if callable(kref) else int(kref)

    dev = engine.device_of(*[f.data for f in fields], *([] if deptho is None else [deptho.data]))
    if mode == "auto":
        m = _first_record_level_means(first, zi, dev)
        m = m[~np.isnan(m)]
        if m.size < 2 or m[-1] == m[0]:
            raise ValueError("direction='auto' cannot tell: the first record's level means do not "
                             "differ between its shallowest and deepest level; pass a direction")
        mode = "rise" if m[-1] > m[0] else "fall"
    z_d = engine.to_device(z, dev, torch.float64)
    floor_d = None if deptho is None else (
        engine.to_device(deptho.data, dev, torch.float64).contiguous().reshape(-1))
    out = _over_z_records(
        fields, zi, vals.size, dev,
        lambda xs: core.column_crossing(xs[0], z_d, vals, b=xs[1] if len(xs) > 1 else None,
                                        kref=kref, mode=mode, relative=relative, miss=miss,
                                        floor=floor_d, eos=eos, p_ref=p_ref))
    lead_dims = tuple(first.dims[:zi])
    coords = {k: c for k, c in first.coords.items() if zcoord not in c.dims}
    if scalar:
        out = out.reshape(tuple(out.shape[:zi]) + tuple(out.shape[zi + 1:]))
        return DataArray(out, lead_dims + hdims, coords, dict(attrs), None)
    coords[value_dim] = DataArray(vals.copy(), (value_dim,), None, dict(value_attrs or {}), value_dim)
    return DataArray(out, lead_dims + (value_dim,) + hdims, coords, dict(attrs), None)


_DIRECTIONS = {"increasing": "rise", "decreasing": "fall", "auto": "auto"}


@accepts_xarray
def calc_isosurface_depth(field, values, zcoord="z_l", direction="auto", missing="nan",
                          deptho=None):
    """EXTENSION (not in momlevel): the depth at which ``field`` (``(..., z, y, x)``) first reaches
    each of ``values`` going down from the surface, linearly interpolated between the two levels
    around the crossing -- the specification is the numpy restatement tests/column_numpy.py.

    ``direction``: "increasing" (the field grows with depth: the first level with
    ``field >= value``), "decreasing" (``field <= value``: the 20 degC isotherm of a temperature
    field) or "auto".  "auto" decides ONCE, from the first record alone: the NaN-skipping
    horizontal mean of every level is taken on the device (one small reduction, nothing of the
    field is downloaded) and the deepest level's mean is compared with the shallowest's --
    greater: "increasing", smaller: "decreasing", equal or a single level: ``ValueError``.
    ``missing``: what a column that never reaches a value gets -- "nan", or "floor": ``deptho``
    where given, else the depth of the column's deepest level with a value.  A value the surface
    level has already reached (an outcrop) and land give NaN.

    A list of ``values`` gives dims ``lead + ("value", y, x)`` with the coordinate ``value``; a
    scalar drops the dim.  float64 metres; device input gives device output."""
    if direction not in _DIRECTIONS:
        raise ValueError(f"direction must be 'increasing', 'decreasing' or 'auto', got {direction!r}")
    if missing not in core.COLUMN_MISS:
        raise ValueError(f"missing must be 'nan' or 'floor', got {missing!r}")
    attrs = {"long_name": "Depth of the isosurface", "units": "m", "positive": "down"}
    of = field.attrs.get("standard_name") if isinstance(field, DataArray) else None
    if of:
        attrs["standard_name"] = f"depth_of_isosurface_of_{of}"
    value_attrs = {k: field.attrs[k] for k in ("standard_name", "units")
                   if isinstance(field, DataArray) and k in field.attrs}
    return _column_depth([field], values, zcoord, 0, _DIRECTIONS[direction], False, missing,
                         deptho, "value", attrs, value_attrs)


@accepts_xarray
def calc_isopycnal_depth(thetao, so, values, level=0.0, patm=101325, eos="Wright", zcoord="z_l"):
    """EXTENSION (not in momlevel): the depth at which the potential density referenced to
    ``level`` (p = level*1e4 + patm, as calc_pdens) first reaches each of ``values`` (kg m-3, e.g.
    1027.0 for sigma0 = 27) going down from the surface; NaN where it never does, where the surface
    is denser already, and on land.  The density is evaluated inside the search, in float64 on the
    widened values whatever the dtype of ``thetao`` and ``so`` (include/momlevel_column.h says
    why): for float64 fields the bits of calc_pdens, which is never materialised.  Dims
    ``lead + ("rhopot", y, x)`` for a list of values; a scalar drops the dim."""
    assert 0.0 <= level <= 7500.0, "specified level must be between 0 and 7500 m"
    attrs = {
        "standard_name": "depth_of_isosurface_of_sea_water_potential_density",
        "long_name": f"Depth of the isopycnal (potential density referenced to {level} m)",
        "comment": f"calculated with the {eos} equation of state",
        "units": "m",
        "positive": "down",
    }
    value_attrs = {"standard_name": "sea_water_potential_density", "units": "kg m-3"}
    return _column_depth([thetao, so], values, zcoord, 0, "rise", False, "nan", None, "rhopot",
                         attrs, value_attrs, eos=_eos_name(eos), p_ref=(level * 1.0e4) + patm)


def _eos_name(eos):
    name = str(eos).lower()
    if name not in core.EOS_IDS:
        raise ValueError(f"unknown equation of state {eos!r}")
    return name


MLD_THRESHOLDS = {"density": 0.03, "temperature": 0.2}


@accepts_xarray
def calc_mld(thetao, so=None, criterion="density", threshold=None, ref_depth=10.0, level=0.0,
             patm=101325, eos="Wright", zcoord="z_l", deptho=None):
    """EXTENSION (not in momlevel): mixed layer depth by a threshold criterion (de Boyer Montegut
    et al. 2004).

    ``criterion="density"``: the depth at which the potential density (referenced to ``level``, as
    calc_pdens; evaluated in float64 inside the search) exceeds its value at the reference level by
    ``threshold`` (default 0.03 kg m-3); needs ``so``.  ``criterion="temperature"``: the depth at
    which ``thetao`` departs from its value at the reference level by ``threshold`` (default
    0.2 degC) either way.  The reference level is the level nearest ``ref_depth`` (ties to the
    shallower), found on the host from the ``zcoord`` values, which must increase strictly.  The
    depth is linearly interpolated between the two levels around the crossing.  A column in which
    the threshold is never reached is mixed to the bottom: ``deptho`` where given, else the depth
    of its deepest level with a value.  Land is NaN.  float64 metres, dims ``lead + (y, x)``; a
    list of thresholds gives ``lead + ("threshold", y, x)``.  Device input gives device output."""
    if criterion not in MLD_THRESHOLDS:
        raise ValueError(f"criterion must be 'density' or 'temperature', got {criterion!r}")
    if criterion == "density" and so is None:
        raise ValueError("criterion='density' needs so (the salinity)")
    assert 0.0 <= level <= 7500.0, "specified level must be between 0 and 7500 m"
    if threshold is None:
        threshold = MLD_THRESHOLDS[criterion]
    if not np.all(np.asarray(threshold, dtype=np.float64) > 0):
        raise ValueError("threshold must be > 0")
    ref = float(ref_depth)
    kref = lambda z: int(np.argmin(np.abs(z - ref)))  # (argmin: the first, shallower, of a tie)
    density = criterion == "density"
    attrs = {
        "standard_name": ("ocean_mixed_layer_thickness_defined_by_sigma_theta" if density
                          else "ocean_mixed_layer_thickness_defined_by_temperature"),
        "long_name": "Mixed layer depth",
        "units": "m",
        "comment": (f"{criterion} threshold relative to the level nearest {ref} m"
                    + (f"; potential density referenced to {level} m, {eos} equation of state"
                       if density else "")),
    }
    value_attrs = {"units": "kg m-3" if density else "degC"}
    if density:
        return _column_depth([thetao, so], threshold, zcoord, kref, "rise", True, "floor", deptho,
                             "threshold", attrs, value_attrs, eos=_eos_name(eos),
                             p_ref=(level * 1.0e4) + patm)
    return _column_depth([thetao], threshold, zcoord, kref, "depart", True, "floor", deptho,
                         "threshold", attrs, value_attrs)
