"""numpy restatement of the spiciness map (include/momlevel_spice.h): the nested evaluation of
Flament's (2002) polynomial in float64, and the magnitude sum A the parity bounds are stated in.
Shared by tests/test_spice_host.py and tests/test_gpu_spice.py; a test helper, not part of the
product.

numpy has no fused multiply-add, so ``horner`` rounds twice where the kernel rounds once: it is
within the bounds below of the kernel and of the reference, not bit-identical to either.

The bounds, u = 2^-53, A = sum_jk |b[j][k] theta^j (S - 35)^k|:
  * float64 inputs: |kernel - reference| <= 64 u A.  A term of the reference carries <= 10 u (two
    powers at <= 1 ulp each, up to four roundings of s carried into s^k, two products); its
    30-term sum adds <= 30 u, the nested evaluation <= 20 u.
  * any float32 input: |kernel - reference| <= 10 * 2^-24 * A -- the reference's own float32
    roundings by the same count; the kernel, float64 on the widened operands, adds nothing at
    that scale.
"""

import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Flament (2002), table 1: B[j][k] multiplies theta^j (S - 35)^k
B = np.array([
    [0.0,        7.7442e-1,  -5.85e-3,   -9.84e-4,   -2.06e-4],
    [5.1655e-2,  2.034e-3,   -2.742e-4,  -8.5e-6,    1.36e-5],
    [6.64783e-3, -2.4681e-4, -1.428e-5,  3.337e-5,   7.894e-6],
    [-5.4023e-5, 7.326e-6,   7.0036e-6,  -3.0412e-6, -1.0853e-6],
    [3.949e-7,   -3.029e-8,  -3.8209e-7, 1.0012e-7,  4.7133e-8],
    [-6.36e-10,  -1.309e-9,  6.048e-9,   -1.1409e-9, -6.676e-10],
])

BOUND_F64 = 64.0 * 2.0 ** -53
BOUND_F32 = 10.0 * 2.0 ** -24

# the dtype variants of the random vectors: name -> (dtype of theta, dtype of S)
VARIANTS = {"f64": (np.float64, np.float64), "f32": (np.float32, np.float32),
            "t32s64": (np.float32, np.float64), "t64s32": (np.float64, np.float32)}


def horner(theta, so):
    """pi in float64 on the exactly widened operands: inner in theta for each power of s = S - 35,
    outer in s -- the order of the kernel"""
    t = np.asarray(theta).astype(np.float64)
    s = np.asarray(so).astype(np.float64) - 35.0
    q = []
    for k in range(5):
        a = np.full(t.shape, B[5][k])
        for j in range(4, -1, -1):
            a = a * t + B[j][k]
        q.append(a)
    pi = q[4]
    for k in range(3, -1, -1):
        pi = pi * s + q[k]
    return pi


def magnitude(theta, so):
    """A = sum_jk |b[j][k] theta^j (S - 35)^k| in float64"""
    t = np.abs(np.asarray(theta).astype(np.float64))
    s = np.abs(np.asarray(so).astype(np.float64) - 35.0)
    A = np.zeros(t.shape)
    tj = np.ones(t.shape)
    for j in range(6):
        sk = np.ones(t.shape)
        for k in range(5):
            A = A + np.abs(B[j][k]) * tj * sk
            sk = sk * s
        tj = tj * t
    return A


def bound(theta, so):
    """the gate of a vector, per cell: by the dtypes of its operands (integers count as float64:
    numpy takes their powers exactly and the products in float64)"""
    f32 = any(np.asarray(x).dtype == np.float32 for x in (theta, so))
    return (BOUND_F32 if f32 else BOUND_F64) * magnitude(theta, so)


_cache = {}


def fixture():
    """the committed vectors (tests/golden/make_spice_golden.py), loaded once, read-only:
    {name: (theta, S, reference pi)} and the goldens of spice_goldens.json"""
    if not _cache:
        z = np.load(os.path.join(GOLDEN, "spice_vectors.npz"))
        vec = {"grid": (z["grid_T"], z["grid_S"], z["grid_pi"]),
               "int32": (z["int_T"], z["int_S"], z["int_pi"]),
               "nan": (z["nan_T"], z["nan_S"], z["nan_pi"]),
               "nan_f32": (z["nan_T"].astype(np.float32), z["nan_S"].astype(np.float32), z["nan_f32_pi"])}
        for draw in ("uni", "nrm"):
            for name, (dt, ds) in VARIANTS.items():  # (the float32 operands are the rounded draws)
                vec[f"{draw}_{name}"] = (z[f"{draw}_T"].astype(dt), z[f"{draw}_S"].astype(ds),
                                         z[f"{draw}_{name}_pi"])
        for arrs in vec.values():
            for a in arrs:
                a.setflags(write=False)
        with open(os.path.join(GOLDEN, "spice_goldens.json")) as f:
            _cache["goldens"] = json.load(f)
        _cache["vectors"] = vec
    return _cache["vectors"], _cache["goldens"]
