"""Time the spiciness map (csrc/momlevel_spice.hip) on one 0.25-degree step, (75, 1080, 1440), resident
on the device, for float64 and for float32 theta / S:

    python scripts/bench_spice.py [--nz 75 --ny 1080 --nx 1440] [--window-ms 300] [--rounds 5]

Each case is timed with device events around enough calls to fill ``--window-ms``; the median over
the rounds is reported with the spread (min .. max).  Per input dtype, on the same tensors in the
same process:

* ``core.spice_map`` -- with its algorithmic bytes (16 B in + 8 B out per cell at float64, 8 + 8 at
  float32), the rate they imply and its fraction of the 8 TB/s HBM peak;
* ``core.stream_probe_mix(a, b, out, write=True)`` -- two streams in, one float64 stream out, no
  arithmetic to speak of: the box's ceiling for this read:write mix -- and the ratio of the map
  to it;
* ``core.eos_map(..., func="density")`` -- the Wright density (K0) with a z-profile pressure: the
  same streams, more arithmetic and a divide.

The last line states the acceptance condition: the float64 spiciness map takes no longer than the
float64 density map, the margin being the spread (max - min) of the density map's own rounds.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from momlevel_amd import _lib, core  # noqa: E402
from momlevel_amd.csrc.build import source_sha, spice_source_sha  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, MI355X


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def measure(name, fn, a, nbytes, extra=None):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    calls = max(1, int(np.ceil(a.window_ms / max(timed(fn, 1), 1e-3))))
    ms = [timed(fn, calls) for _ in range(a.rounds)]
    med = float(np.median(ms))
    row = {"case": name, "calls_per_window": calls, "ms": round(med, 4), "ms_min": round(min(ms), 4),
           "ms_max": round(max(ms), 4), "bytes": nbytes, "TB/s": round(nbytes / med / 1e9, 3),
           "fraction_of_8TBs_peak": round(nbytes / med * 1e3 / HBM_PEAK, 3)}
    row.update(extra(med) if extra else {})
    print(json.dumps(row), flush=True)
    return med, min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nz", type=int, default=75)
    ap.add_argument("--ny", type=int, default=1080)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    core.require_device()
    _lib.load_spice()
    n = a.nz * a.ny * a.nx
    print(json.dumps({"spice_source_sha": spice_source_sha(), "timed_source_sha": source_sha(),
                      "step": [a.nz, a.ny, a.nx], "cells": n, "window_ms": a.window_ms,
                      "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}), flush=True)

    gen = torch.Generator(device="cuda").manual_seed(2002)
    T64 = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) * 34.0 - 2.0
    S64 = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) * 10.0 + 30.0
    p = torch.linspace(1.0e4, 6.0e7, a.nz, dtype=torch.float64, device="cuda")  # a z profile
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    results = {}
    for label, T, S in (("float64", T64, S64), ("float32", T64.float(), S64.float())):
        nbytes = n * (2 * T.element_size() + 8)
        probe, _, _ = measure(f"stream probe, 2 x {label} in, 1 x float64 out",
                              lambda: core.stream_probe_mix(T, S, out, write=True), a, nbytes)
        spice = measure(f"spice_map, {label} theta / S", lambda: core.spice_map(T, S, out=out), a, nbytes,
                        lambda ms: {"ratio_to_stream_probe": round(ms / probe, 3)})
        T4, S4 = T.reshape(1, a.nz, a.ny, a.nx), S.reshape(1, a.nz, a.ny, a.nx)
        dens = measure(f"eos_map density (Wright, z-profile pressure), {label} theta / S",
                       lambda: core.eos_map(T4, S4, p, eos="wright", func="density"), a, nbytes,
                       lambda ms: {"ratio_to_stream_probe": round(ms / probe, 3)})
        results[label] = (spice, dens)
        del T4, S4
    (sp, _, _), (de, de_min, de_max) = results["float64"]
    margin = de_max - de_min
    print(json.dumps({"condition": "float64 spice_map takes no longer than float64 eos_map density",
                      "spice_ms": round(sp, 4), "density_ms": round(de, 4),
                      "margin_ms (spread of the density map's rounds)": round(margin, 4),
                      "met": bool(sp <= de + margin)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
