"""Generate the committed tide-gauge fixtures under tests/golden/ from the DATA files of a momlevel
checkout (src/momlevel/resources):

    python -B tests/golden/make_tidegauge_golden.py /path/to/momlevel

(-B: nothing is written into the reference tree.)  Only the standard library's csv module and numpy
are used; no reference code is imported and the text of no reference source file is stored --
numbers and site names only.

* ``tidegauge_nwa12.npz`` -- the NWA12 grid of ``NWA12_grid_dataframe.csv`` (the model frame of the
  reference's tests/test_util.py:216-231): ``geolat`` / ``geolon`` (146, 100) float64 as parsed (empty cells are NaN),
  ``mask`` (146, 100) uint8 (8509 wet points), and the frame's index levels ``yh`` (146) / ``xh``
  (100).
* ``tidegauge_goldens.json`` -- ``gauges``: name, lat, lon of the 117 rows of
  ``us_tide_gauges.csv``; ``reference``: name, distance (km), mod_index of the 16 rows of
  ``geolocate_points_reference.csv`` (what ``util.geolocate_points(..., threshold=13.75)`` returned
  with scikit-learn's BallTree); ``threshold`` and ``rad_earth`` of that call.

``NWA12_sample_grid_data.nc`` (``ssh_max`` and the 16 sums of the reference's
tests/test_tidegauge.py:23-38) is a netCDF-4 / HDF5 file: scipy.io.netcdf_file reads netCDF-3 only
and no HDF5 reader is installed where the fixtures are made, so those sums are NOT part of the
fixtures.
"""

import csv
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))


def rows(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def number(text):
    """a CSV cell as pandas.read_csv parses it: an empty cell is NaN"""
    return float(text) if text.strip() else float("nan")


def main(reference):
    res = os.path.join(reference, "src", "momlevel", "resources")

    grid = rows(os.path.join(res, "NWA12_grid_dataframe.csv"))
    yh = np.array([float(r["yh"]) for r in grid])
    xh = np.array([float(r["xh"]) for r in grid])
    ny = len(np.unique(yh))
    nx = len(grid) // ny
    assert (ny, nx) == (146, 100) and ny * nx == len(grid)
    yh2, xh2 = yh.reshape(ny, nx), xh.reshape(ny, nx)
    assert np.all(yh2 == yh2[:, :1]) and np.all(xh2 == xh2[:1, :])  # C order: yh outer, xh inner
    mask = np.array([number(r["mask"]) for r in grid]).reshape(ny, nx)
    assert set(np.unique(mask)) <= {0.0, 1.0} and int(mask.sum()) == 8509
    np.savez_compressed(
        os.path.join(HERE, "tidegauge_nwa12.npz"),
        geolat=np.array([number(r["geolat"]) for r in grid]).reshape(ny, nx),
        geolon=np.array([number(r["geolon"]) for r in grid]).reshape(ny, nx),
        mask=mask.astype(np.uint8), yh=yh2[:, 0].copy(), xh=xh2[0, :].copy())

    gauges = rows(os.path.join(res, "us_tide_gauges.csv"))
    assert len(gauges) == 117
    ref = rows(os.path.join(res, "geolocate_points_reference.csv"))
    assert len(ref) == 16
    out = {
        "source": "momlevel src/momlevel/resources: us_tide_gauges.csv, "
                  "geolocate_points_reference.csv (tests/test_util.py:216-231)",
        "threshold": 13.75,
        "rad_earth": 6.378e03,
        "gauges": {"name": [r["PSMSL_site"] for r in gauges],
                   "lat": [float(r["lat"]) for r in gauges],
                   "lon": [float(r["lon"]) for r in gauges]},
        "reference": {"name": [r["name"] for r in ref],
                      "distance": [float(r["distance"]) for r in ref],
                      "mod_index": [int(r["mod_index"]) for r in ref]},
    }
    with open(os.path.join(HERE, "tidegauge_goldens.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
