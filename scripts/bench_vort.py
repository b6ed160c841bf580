"""Time the two C-grid stencils (csrc/momlevel_vort.hip) on one 0.25-degree step, (75, 1080, 1440),
resident on the device, for float64 and for float32 operands:

    python scripts/bench_vort.py [--nz 75 --ny 1080 --nx 1440] [--window-ms 300] [--rounds 5]

Each case is timed with device events around enough calls to fill ``--window-ms``; the median over
the rounds is reported with the spread (min .. max).  Per dtype, on the same tensors in the same
process:

* ``core.stream_probe_mix(u, v, out, write=True)`` -- two streams in, one float64 stream out, no
  arithmetic to speak of: the box's ceiling for this read:write mix;
* ``core.rel_vort`` and ``core.potential_vorticity`` (interp, both units) -- with their algorithmic
  bytes (two fields in, one out: 24 B per cell at float64, 12 at float32; the 2-D metrics are read
  from cache), the rate they imply and the ratio to the probe.

After the two dtypes, one case per mixed-dtype instantiation of the packed kernels (fields of one
dtype and metrics of the other; zeta, coriolis and n2 in every combination that is not uniform).

The last lines state the acceptance condition per float64 pass: it takes no longer than the probe's
time x the algorithmic byte ratio of the tiling, (24 + 8 / H) / 24 -- the halo row, nothing else --
plus the spread (max - min) of the probe's own rounds.

``--counters`` runs each float64 pass a few times and exits: the body of a counter-only
``rocprofv3 --pmc FETCH_SIZE WRITE_SIZE`` run; ``--summarise DIR`` then reads the csv files that run
left under DIR and prints the traffic per kernel beside the algorithmic bytes.
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s, MI355X


def timed(fn, calls):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def measure(name, fn, a, nbytes, extra=None):
    import torch

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


def summarise(directory, cells):
    """FETCH_SIZE / WRITE_SIZE per kernel from the csv files of a counter-only rocprofv3 run"""
    rows = {}
    for base, _, files in os.walk(directory):
        for name in files:
            if not name.endswith(".csv"):
                continue
            with open(os.path.join(base, name), newline="") as f:
                for r in csv.DictReader(f):
                    kernel, counter, value = r.get("Kernel_Name"), r.get("Counter_Name"), r.get("Counter_Value")
                    if kernel and counter in ("FETCH_SIZE", "WRITE_SIZE") and "k_vort" in kernel:
                        rows.setdefault((kernel.split("(")[0][:60], counter), []).append(float(value))
    if not rows:
        print(json.dumps({"counters": "no k_vort rows found under " + directory}), flush=True)
        return 1
    for (kernel, counter), values in sorted(rows.items()):
        med = float(np.median(values))
        print(json.dumps({"kernel": kernel, "counter": counter, "dispatches": len(values),
                          "median_KB": round(med, 1), "bytes_per_cell": round(med * 1024.0 / cells, 3),
                          "algorithmic_bytes_per_cell": 16 if counter == "FETCH_SIZE" else 8,
                          "note": "gfx950 tallies a wide streaming read at half its bytes: double "
                                  "FETCH_SIZE before comparing" if counter == "FETCH_SIZE" else
                                  "16-byte streaming stores are counted exactly"}), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nz", type=int, default=75)
    ap.add_argument("--ny", type=int, default=1080)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--counters", action="store_true")
    ap.add_argument("--summarise", metavar="DIR")
    a = ap.parse_args()
    n = a.nz * a.ny * a.nx
    if a.summarise:
        return summarise(a.summarise, n)

    import torch

    from momlevel_amd import _lib, core
    from momlevel_amd.csrc.build import source_sha, vort_source_sha

    core.require_device()
    _lib.load_vort()
    w64, w32, h, bands = core.vort_tile()
    byte_ratio = (24.0 + 8.0 / h) / 24.0
    print(json.dumps({"vort_source_sha": vort_source_sha(), "timed_source_sha": source_sha(),
                      "step": [a.nz, a.ny, a.nx], "cells": n, "window_ms": a.window_ms,
                      "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
                      "tile": {"W_float64": w64, "W_float32": w32, "H": h, "bands_per_block": bands},
                      "algorithmic_byte_ratio (24 + 8 / H) / 24": round(byte_ratio, 5)}), flush=True)

    gen = torch.Generator(device="cuda").manual_seed(1872)
    shape = (a.nz, a.ny, a.nx)

    def rand(shp, lo, hi, dtype=torch.float64):
        return (torch.rand(shp, dtype=torch.float64, device="cuda", generator=gen) * (hi - lo) + lo).to(dtype)

    u64, v64 = rand(shape, -0.5, 0.5), rand(shape, -0.3, 0.3)
    n264 = rand(shape, -1e-5, 4e-5)
    m64 = [rand(shape[1:], 1.0e4, 3.0e4), rand(shape[1:], 1.0e4, 3.0e4), rand(shape[1:], 4.0e8, 9.0e8)]
    f64 = rand(shape[1:], -1.4e-4, 1.4e-4)
    probe_out = torch.empty(n, dtype=torch.float64, device="cuda")

    if a.counters:
        zeta = core.rel_vort(u64, v64, *m64)
        for _ in range(3):
            core.rel_vort(u64, v64, *m64, out=zeta)
            core.potential_vorticity(zeta, f64, n264, out=probe_out.view(shape))
        torch.cuda.synchronize()
        return 0

    met = []
    for label, dt in (("float64", torch.float64), ("float32", torch.float32)):
        u, v, n2, f = u64.to(dt), v64.to(dt), n264.to(dt), f64.to(dt)
        dx, dy, area = (m.to(dt) for m in m64)
        out = torch.empty(shape, dtype=dt, device="cuda")
        zeta = core.rel_vort(u, v, dx, dy, area)
        nbytes = n * 3 * u.element_size()
        probe, pmin, pmax = measure(f"stream probe, 2 x {label} in, 1 x float64 out",
                                    lambda: core.stream_probe_mix(u.view(-1), v.view(-1), probe_out, write=True),
                                    a, n * (2 * u.element_size() + 8))
        ratio = lambda ms: {"ratio_to_stream_probe": round(ms / probe, 3)}  # noqa: E731
        cases = [
            (f"rel_vort, {label} fields and metrics",
             lambda: core.rel_vort(u, v, dx, dy, area, out=out)),
            (f"potential_vorticity (interp, m), {label}",
             lambda: core.potential_vorticity(zeta, f, n2, out=out)),
            (f"potential_vorticity (interp, cm), {label}",
             lambda: core.potential_vorticity(zeta, f, n2, units="cm", out=out)),
            (f"potential_vorticity (no interp), {label}",
             lambda: core.potential_vorticity(zeta, f, n2, interp=False, out=out)),
        ]
        for name, fn in cases:
            ms, _, _ = measure(name, fn, a, nbytes, ratio)
            if label == "float64" and "no interp" not in name:
                limit = probe * byte_ratio + (pmax - pmin)
                met.append({"condition": f"{name}: no longer than probe x {byte_ratio:.5f} + the "
                                         "spread of the probe's rounds",
                            "ms": round(ms, 4), "probe_ms": round(probe, 4),
                            "probe_spread_ms": round(pmax - pmin, 4), "limit_ms": round(limit, 4),
                            "met": bool(ms <= limit)})
        del u, v, n2, f, dx, dy, area, out, zeta
    # operands of both dtypes in one call (the result is float64): the packed kernels' other
    # instantiations, one case each
    kinds = {"float64": torch.float64, "float32": torch.float32}
    out = torch.empty(shape, dtype=torch.float64, device="cuda")
    zeta64 = core.rel_vort(u64, v64, *m64)
    for tf, tm in (("float64", "float32"), ("float32", "float64")):
        u, v = u64.to(kinds[tf]), v64.to(kinds[tf])
        dx, dy, area = (m.to(kinds[tm]) for m in m64)
        measure(f"rel_vort, {tf} fields, {tm} metrics",
                lambda: core.rel_vort(u, v, dx, dy, area, out=out), a, n * (2 * u.element_size() + 8))
    for tz in kinds:
        for tc in kinds:
            for tn in kinds:
                if tz == tc == tn:
                    continue
                zeta, f, n2 = zeta64.to(kinds[tz]), f64.to(kinds[tc]), n264.to(kinds[tn])
                for interp in (True, False):
                    measure(f"potential_vorticity ({'interp' if interp else 'no interp'}, m), zeta {tz}, "
                            f"coriolis {tc}, n2 {tn}",
                            lambda: core.potential_vorticity(zeta, f, n2, interp=interp, out=out), a,
                            n * (zeta.element_size() + n2.element_size() + 8))
    for row in met:
        print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
