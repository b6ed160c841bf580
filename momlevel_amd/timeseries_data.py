"""Time-series test datasets with a monthly or a daily axis.

``generate_test_data_time`` of the reference (src/momlevel/test_data/__init__.py:143-191) with its
``frequency`` argument: ``"MS"`` gives the monthly mid-point axis (time.py:66-73), ``"D"`` the
daily mid-day axis (time.py:75-94).  Same ``numpy.random.default_rng`` draws as the reference, so
the daily dataset is number for number the one its ``tests/test_trend.py`` runs on.  The package
publishes this function as ``momlevel_amd.test_data.generate_test_data_time`` (the reference's
place for it); with the default ``frequency="MS"`` it returns what that module's own monthly-only
generator returns.
"""

import numpy as np

from .cftime_lite import daily_midpoints, monthly_midpoints
from .labeled import DataArray, Dataset

__all__ = ["generate_test_data_time"]


def _time_stub(start_year, nyears, calendar, frequency):
    if frequency == "MS":
        steps = monthly_midpoints(start_year, nyears, calendar)
    elif frequency == "D":
        steps = daily_midpoints(start_year, nyears, calendar)
    else:  # (time.py:88-89)
        raise ValueError(f"Time frequency '{frequency}' is not currently supported.")
    time = np.empty(len(steps), dtype=object)
    time[:] = steps
    return DataArray(
        time, ("time",), None,
        {"long_name": "time", "cartesian_axis": "T", "calendar_type": calendar,
         "bounds": "time_bnds"},
    )


def generate_test_data_time(start_year=1981, nyears=5, calendar="noleap", seed=123,
                            frequency="MS"):
    """Time-series dataset var_a / var_b on a 5x5 grid (test_data/__init__.py:143-191): monthly
    mid-points (``frequency="MS"``, the default) or daily mid-days (``"D"``)."""
    dset = Dataset()
    dset["time"] = _time_stub(start_year, nyears, calendar, frequency)
    nt = len(dset["time"])
    lon = DataArray([1.0, 2.0, 3.0, 4.0, 5.0], ("lon",))
    lat = DataArray([1.0, 2.0, 3.0, 4.0, 5.0], ("lat",))
    dset["lon"], dset["lat"] = lon, lat
    attrs = {"first_attribute": "foo", "second_attribute": "bar"}
    dset["var_a"] = DataArray(np.random.default_rng(seed).normal(100, 20, (nt, 5, 5)),
                              ("time", "lat", "lon"), None, attrs)
    dset["var_b"] = DataArray(np.random.default_rng(seed * 2).normal(100, 20, (nt, 5, 5)),
                              ("time", "lat", "lon"), None, attrs)
    return dset
