""" staggered_data - the reference's velocity test dataset on the staggered (C) grid

Restates ``generate_test_data_uv`` (src/momlevel/test_data/__init__.py:194-315) on the labelled
classes with the same ``numpy.random.default_rng`` draws, beside the generators of test_data.py
whose grid stubs it reuses; published as ``momlevel_amd.test_data.generate_test_data_uv``, where
the reference keeps it.
"""

import numpy as np

from .labeled import DataArray, Dataset
from .test_data import _time_stub, xy_fields, zlevel_fields

__all__ = ["generate_test_data_uv"]


def generate_test_data_uv(start_year=1981, nyears=0, calendar="noleap", seed=123):
    """ntimes x 5 x 5 x 5 velocities on the staggered grid with their metrics
    (test_data/__init__.py:194-315): ``uo`` on (yh, xq), ``vo`` on (yq, xh), ``dxCu``, ``dyCv``,
    ``Coriolis`` and ``areacello_bu`` on (yq, xq) -- a non-symmetric grid, corner and centre
    dimensions of equal length."""
    dset = Dataset()
    if nyears >= 1:
        dset["time"] = _time_stub(start_year, nyears, calendar)
    else:
        dset["time"] = DataArray(
            [1.0, 2.0, 3.0, 4.0, 5.0], ("time",), None,
            {"long_name": "time", "cartesian_axis": "T", "calendar_type": calendar,
             "bounds": "time_bnds"},
        )
    ntimes = len(dset["time"])
    dset = xy_fields(dset)
    dset = zlevel_fields(dset)
    dset["xq"] = DataArray([1.5, 2.5, 3.5, 4.5, 5.5], ("xq",))
    dset["yq"] = DataArray([1.5, 2.5, 3.5, 4.5, 5.5], ("yq",))
    shape = (ntimes, 5, 5, 5)
    tavg = {"time_avg_info": "average_T1,average_T2,average_DT"}
    dset["uo"] = DataArray(
        np.random.default_rng(seed).normal(0.0061, 0.08, shape), ("time", "z_l", "yh", "xq"), None,
        dict(long_name="Sea Water X Velocity", units="m s-1", standard_name="sea_water_x_velocity",
             interp_method="none", cell_methods="z_l:mean yh:mean xq:point time: mean", **tavg),
    )
    dset["vo"] = DataArray(
        np.random.default_rng(seed).normal(0.00077, 0.04, shape), ("time", "z_l", "yq", "xh"), None,
        dict(long_name="Sea Water Y Velocity", units="m s-1", standard_name="sea_water_y_velocity",
             interp_method="none", cell_methods="z_l:mean yq:point xh:mean time: mean", **tavg),
    )
    dset["dxCu"] = DataArray(
        np.ones((5, 5)), ("yh", "xq"), None,
        {"long_name": "Delta(x) at u points (meter)", "units": "m", "cell_methods": "time: point",
         "interp_method": "none"},
    )
    dset["dyCv"] = DataArray(
        np.ones((5, 5)), ("yq", "xh"), None,
        {"long_name": "Delta(y) at v points (meter)", "units": "m", "cell_methods": "time: point",
         "interp_method": "none"},
    )
    dset["Coriolis"] = DataArray(
        np.random.default_rng(seed).normal(1.21e-5, 0.00011, (5, 5)), ("yq", "xq"), None,
        {"long_name": "Coriolis parameter at corner (Bu) points", "units": "s-1",
         "cell_methods": "time: point", "interp_method": "none"},
    )
    areacello_bu = np.random.default_rng(seed).normal(100.0, 10.0, (5, 5))
    areacello_bu = areacello_bu / areacello_bu.sum()
    dset["areacello_bu"] = DataArray(
        areacello_bu * 3.6111092e14, ("yq", "xq"), None,
        {"long_name": "Ocean Grid-Cell Area", "units": "m2",
         "cell_methods": "area:sum yq:sum xq:sum time: point", "standard_name": "cell_area"},
    )
    return dset
