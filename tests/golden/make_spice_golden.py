"""Generate the committed spiciness fixtures under tests/golden/ from a momlevel checkout:

    python -B tests/golden/make_spice_golden.py /path/to/momlevel

(-B: nothing is written into the reference tree.)  The reference's ``src/momlevel/spice/flament.py``
is loaded standalone with importlib (it imports numpy only; the package itself needs xarray), the
way make_golden.py loads ``wright.py``.  The text of no reference source file is stored: numbers
only.

* ``spice_vectors.npz`` -- inputs and the outputs of the reference's ``spice``:
    grid_*     the grid of the reference's tests/test_flament.py (theta = 0..30, S = arange(33.0, 37.1, 0.1));
    uni_T/S    4096 draws of theta ~ U[-2, 32], S ~ U[0, 42] (float64);
    nrm_T/S    4096 draws of theta ~ N(15, 5), S ~ N(35, 1.5) (float64);
    {uni,nrm}_{f64,f32,t32s64,t64s32}_pi
               the reference on those draws as float64, as float32 (the draws rounded:
               ``astype(float32)``) and with one of the two fields rounded -- the float32 inputs are
               not stored, the tests round the draws the same way;
    int_*      an int32 theta against a float64 S;
    nan_*      a block with NaNs in theta only, in S only and in both (float64, and rounded to
               float32: nan_f32_pi).
* ``spice_goldens.json`` -- the sum over the grid that tests/test_flament.py pins, and the
  reference's own sum to every digit.
"""

import importlib.util
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

GRID_SUM = 3283.680384169385  # tests/test_flament.py:13
VARIANTS = {"f64": (np.float64, np.float64), "f32": (np.float32, np.float32),
            "t32s64": (np.float32, np.float64), "t64s32": (np.float64, np.float32)}


def load_reference(root):
    path = os.path.join(root, "src", "momlevel", "spice", "flament.py")
    spec = importlib.util.spec_from_file_location("ref_flament", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(root):
    ref = load_reference(root)
    out = {}

    S = np.arange(33.0, 37.1, 0.1)
    T = np.arange(0.0, 31.0, 1.0)
    out["grid_S"] = np.tile(S[None, :], (len(T), 1))
    out["grid_T"] = np.tile(T[:, None], (1, len(S)))
    out["grid_pi"] = ref.spice(out["grid_T"], out["grid_S"])
    # (numpy's arange(33.0, 37.1, 0.1) has 42 elements, the last one 37.1: the grid is what the
    # reference's test builds, and the pinned sum belongs to it)
    assert out["grid_pi"].shape == (len(T), len(S)) and out["grid_pi"].dtype == np.float64
    assert np.allclose(out["grid_pi"].sum(), GRID_SUM)

    rng = np.random.default_rng(20020054)
    n = 4096
    out["uni_T"], out["uni_S"] = rng.uniform(-2.0, 32.0, n), rng.uniform(0.0, 42.0, n)
    out["nrm_T"], out["nrm_S"] = rng.normal(15.0, 5.0, n), rng.normal(35.0, 1.5, n)
    for draw in ("uni", "nrm"):
        for name, (dt, ds) in VARIANTS.items():
            pi = ref.spice(out[f"{draw}_T"].astype(dt), out[f"{draw}_S"].astype(ds))
            assert pi.dtype == np.float64 and np.isfinite(pi).all()
            out[f"{draw}_{name}_pi"] = pi

    out["int_T"] = rng.integers(-2, 33, 257).astype(np.int32)
    out["int_S"] = rng.uniform(0.0, 42.0, 257)
    out["int_pi"] = ref.spice(out["int_T"], out["int_S"])
    assert out["int_pi"].dtype == np.float64

    T, S = rng.uniform(-2.0, 32.0, 96), rng.uniform(0.0, 42.0, 96)
    T[[0, 5, 17, 63, 64]] = np.nan   # theta only
    S[[1, 6, 18, 65, 95]] = np.nan   # S only
    T[[2, 7, 40]] = np.nan           # both
    S[[2, 7, 40]] = np.nan
    out["nan_T"], out["nan_S"] = T, S
    out["nan_pi"] = ref.spice(T, S)
    out["nan_f32_pi"] = ref.spice(T.astype(np.float32), S.astype(np.float32))
    assert np.array_equal(np.isnan(out["nan_pi"]), np.isnan(T) | np.isnan(S))
    assert np.array_equal(np.isnan(out["nan_f32_pi"]), np.isnan(T) | np.isnan(S))

    np.savez_compressed(os.path.join(HERE, "spice_vectors.npz"), **out)
    goldens = {
        "source": "momlevel src/momlevel/spice/flament.py on the grid of tests/test_flament.py",
        "grid_shape": list(out["grid_pi"].shape),
        "grid_sum": GRID_SUM,
        "grid_sum_reference": float(out["grid_pi"].sum()),
    }
    with open(os.path.join(HERE, "spice_goldens.json"), "w") as f:
        json.dump(goldens, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
