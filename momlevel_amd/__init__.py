""" momlevel_amd - momlevel's steric sea-level hot path on AMD Instinct MI355X (gfx950)

A drop-in for one path of jkrasting/momlevel: the Wright (1997) in-situ density and
the volume-weighted reductions behind ``steric`` / ``halosteric`` / ``thermosteric``
and ``derived.calc_rho`` / ``calc_masso`` / ``calc_volo``, the per-cell trend,
detrend and deseason fits of ``trend``, and the grouped time statistics
``util.monthly_average`` / ``util.annual_cycle``, computed by hand-written HIP kernels behind a
C ABI (include/momlevel_hip.h, include/momlevel_trend.h, include/momlevel_clim.h,
include/momlevel_gauge.h, include/momlevel_spice.h, include/momlevel_vort.h,
include/momlevel_area.h, include/momlevel_layer.h, include/momlevel_filter.h,
include/momlevel_quantile.h, include/momlevel_column.h, include/momlevel_eof.h,
include/momlevel_smooth.h, include/momlevel_regrid.h, include/momlevel_census.h).

``tidegauge.extract_tidegauge`` takes a ``(..., yh, xh)`` record to its tide gauges: the nearest
wet grid point of every gauge by great-circle distance (a brute-force search on the GPU, ties to
the lowest flat index) and the gauges' series, gathered in one launch -- a device-resident record
reaches its gauges without a download.  ``util.geolocate_points`` is the same search on pandas
frames.  The reference's gauge tables are not shipped: pass a CSV path or an in-memory table.

``derived.calc_spice`` / ``spice.flament.spice`` map potential temperature and salinity to Flament's
(2002) spiciness in one pointwise kernel; with ``derived.calc_pdens`` the sigma-pi water-mass view
is computed without the fields leaving the device.

``derived.calc_rel_vort`` / ``calc_pv`` / ``calc_rossby_rd`` (with ``calc_coriolis``) are the
reference's C-grid group: relative and potential vorticity as horizontal stencils on MOM6's
staggered grid, one pass each, consuming the N^2 of ``calc_n2`` and the wave speed of
``calc_wave_speed`` where they were computed.

``regional.area_mean`` / ``regional.area_anomaly`` (an EXTENSION: momlevel has no such function)
reduce a ``(..., yh, xh)`` record to its area-weighted global or per-basin means and to the
anomalies from them -- the first thing done with a local steric field -- where the record lives.

``steric_layers``, ``derived.calc_layer_integral`` and ``derived.calc_heat_content`` (EXTENSIONS as
well) split the local steric height, any ``(..., z, yh, xh)`` field or the heat content into depth
layers -- the upper 700 m, 700-2000 m, below -- with ``calc_dz``'s own partial cells, on a kernel that
runs behind K2 on a device scratch of ``delta_rho`` (include/momlevel_layer.h).

``filters`` (an EXTENSION too) smooths a ``(time, ...)`` record along time where it lives:
``rolling_mean`` / ``rolling_sum`` (xarray's ``.rolling().mean()`` values), ``lowpass`` (Lanczos),
``time_filter`` (any FIR weights) and ``rolling_trend`` (the least-squares rate over sliding windows
against the actual time axis) are one NaN-aware banded operator along time with weight tables made
on the host (include/momlevel_filter.h).

``extremes`` (an EXTENSION too) gives the order statistics of a ``(time, ...)`` record where it
lives: ``time_quantile`` / ``time_median`` (the values of xarray's ``.quantile(q, dim="time")``,
over the whole record, per calendar month or per year) by radix select in registers, and
``exceedance_count``, the steps above a number, a per-cell field or those quantiles
(include/momlevel_quantile.h).

``derived.calc_mld``, ``derived.calc_isosurface_depth`` and ``derived.calc_isopycnal_depth`` (EXTENSIONS
too) answer the vertical questions of a ``(..., z, yh, xh)`` field where it lives: the mixed layer
depth by a density or temperature threshold, the depth of the 20 degC isotherm, the depth of
sigma0 = 27 -- one search down every column that stops reading at the crossing, the potential
density evaluated inside it and never written out (include/momlevel_column.h).

``eof`` (an EXTENSION too) couples all cells of a ``(time, yh, xh)`` record: ``time_covariance``,
``calc_eofs`` (eigenvalues, variance fractions, unit-variance principal components and the EOFs as
covariance maps) and ``project_field``.  The contraction over the cells runs on the float64 matrix
cores with the anomalies formed while the rows are staged, in a fixed order of summation; the
``nt x nt`` eigen-problem is solved on the host (include/momlevel_eof.h).

``spatial`` (an EXTENSION too) is the horizontal filter: ``smooth`` and ``highpass`` apply an
area-weighted, land-aware separable convolution over the ``(yh, xh)`` plane of every record where
it lives -- ``boxcar_weights``, ``gaussian_weights``, or ``length_scale_weights`` for a fixed length
on a converging grid -- with x periodic or closed; the tripolar fold and multi-rank tiles are not
built (include/momlevel_smooth.h).

``regrid`` (an EXTENSION too) moves a ``(..., yh, xh)`` record to another grid where it lives: a
gather through a sparse weight table with the weights of the sources present renormalised --
``coarsen_weights`` (conservative blocks of any grid), ``conservative_weights`` (rectilinear
lat/lon grids), ``nearest_weights`` or any ESMF-style table through ``from_triplets``, then
``apply`` or the one-call ``coarsen``.  Bilinear and curvilinear conservative weights are not
generated, the tripolar fold is not part of the coarsening's periodic option and a table is not
spread over ranks (include/momlevel_regrid.h).

``census`` (an EXTENSION too) is the scatter: ``histogram`` counts, or sums a weight or a weighted
value over, the cells of every class of one or two fields per record -- ``ts_census`` is the
volumetric theta-S census, ``histogram(calc_pdens, calc_spice, weights=volcello)`` the sigma-pi one
-- in a fixed order of summation without atomics; tables larger than one launch go in bin groups;
more than two binning fields, a fused density and multi-rank tables are not built
(include/momlevel_census.h).

Everything else in momlevel (plots, the xgcm grid object itself, ...) is out of scope -- use momlevel.

There is no CPU fallback: without libmomlevel_hip.so and a HIP device the compute
entry points raise ``MomlevelHipError``.
"""

__version__ = "0.1.0"

from . import census
from . import derived
from . import dynamic
from . import eof
from . import eos
from . import extremes
from . import filters
from . import reference
from . import regional
from . import regrid
from . import spatial
from . import spice
from . import staggered_data
from . import test_data
from . import tidegauge
from . import timeseries_data
from . import trend
from . import util
from ._lib import MomlevelHipError
from .dynamic import inverse_barometer
from .labeled import DataArray, Dataset
from .steric import halosteric, steric, steric_layers, steric_variants, thermosteric

# the reference keeps generate_test_data_time in its test_data module; the version with the
# ``frequency`` argument ("MS" | "D") lives in timeseries_data and is published there
test_data.generate_test_data_time = timeseries_data.generate_test_data_time
# generate_test_data_uv (the velocities on the staggered grid) lives in staggered_data and is
# published where the reference keeps it
test_data.generate_test_data_uv = staggered_data.generate_test_data_uv

__all__ = [
    "DataArray",
    "Dataset",
    "MomlevelHipError",
    "census",
    "derived",
    "dynamic",
    "inverse_barometer",
    "eof",
    "eos",
    "extremes",
    "filters",
    "halosteric",
    "reference",
    "regional",
    "regrid",
    "spatial",
    "spice",
    "steric",
    "steric_layers",
    "steric_variants",
    "test_data",
    "thermosteric",
    "tidegauge",
    "trend",
    "util",
]
