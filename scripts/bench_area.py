"""Time the area-mean kernels (csrc/momlevel_area.hip) on a resident (1200, 1080, 1440) eta record --
a century of monthly 0.25-degree fields -- for float64 and for float32:

    python scripts/bench_area.py [--nt 1200 --ny 1080 --nx 1440] [--window-ms 300] [--rounds 5]

Each case is timed with device events around enough calls to fill ``--window-ms``; the median over
the rounds is reported with the spread (min .. max).  Per dtype, on the same tensor in the same
process:

* ``core.stream_probe_mix(record, write=False)`` -- the record read once, nothing written: the
  box's ceiling for the global and the regional mean (``vs_probe`` = probe time / kernel time);
* ``core.stream_probe_mix(record, out=..., write=True)`` -- one stream in, one float64 stream out:
  the ceiling for the anomaly pass;
* ``core.area_mean`` without regions, with 12 regions, and ``core.area_anomaly`` against the 12
  regional means, with their algorithmic bytes: the record once (and 8 B per cell out for the
  anomaly); the 2-D maps and the partials are left out of the byte count, so the rates are what a
  caller sees;
* ``core.group_weighted_mean`` (float64 only: it takes nothing else), the existing one-read
  reduction over time, for comparison.

These are call times: the workspace of the partials comes from torch's caching allocator inside the
timed region, as a caller pays for it.

``--counters`` runs each float64 pass a few times and exits: the body of a counter-only
``rocprofv3 --pmc FETCH_SIZE`` run and of a second one with ``--pmc WRITE_SIZE`` (ONE counter a run:
the two together are more than the hardware collects in a pass, and rocprofv3 aborts at the first
dispatch); ``--summarise DIR`` then reads the csv files those runs left under DIR and prints the
traffic per kernel beside the algorithmic bytes.
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
NREGIONS = 12


def timed(fn, calls):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def measure(name, fn, a, nbytes, probe_ms=None):
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
    if probe_ms is not None:
        row["vs_probe"] = round(probe_ms / med, 4)
    print(json.dumps(row), flush=True)
    return med


def summarise(directory, cells, plane):
    """FETCH_SIZE / WRITE_SIZE per kernel from the csv files of a counter-only rocprofv3 run"""
    rows = {}
    for base, _, files in os.walk(directory):
        for name in files:
            if not name.endswith(".csv"):
                continue
            with open(os.path.join(base, name), newline="") as f:
                for r in csv.DictReader(f):
                    kernel, counter, value = r.get("Kernel_Name"), r.get("Counter_Name"), r.get("Counter_Value")
                    if kernel and counter in ("FETCH_SIZE", "WRITE_SIZE") and "k_area" in kernel:
                        rows.setdefault((kernel.split("(")[0][:70], counter), []).append(float(value))
    if not rows:
        print(json.dumps({"counters": "no k_area rows found under " + directory}), flush=True)
        return 1
    for (kernel, counter), values in sorted(rows.items()):
        med = float(np.median(values))
        print(json.dumps({"kernel": kernel, "counter": counter, "dispatches": len(values),
                          "median_KB": round(med, 1), "bytes_per_cell": round(med * 1024.0 / cells, 3),
                          "record_plus_maps_once_bytes_per_cell (float64 record)":
                              round(8.0 + 12.0 * plane / cells, 3),
                          "note": "gfx950 tallies a wide streaming read at half its bytes: double "
                                  "FETCH_SIZE before comparing" if counter == "FETCH_SIZE" else
                                  "16-byte streaming stores are counted exactly"}), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nt", type=int, default=1200)
    ap.add_argument("--ny", type=int, default=1080)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--counters", action="store_true")
    ap.add_argument("--summarise", metavar="DIR")
    a = ap.parse_args()
    plane = a.ny * a.nx
    n = a.nt * plane
    if a.summarise:
        return summarise(a.summarise, n, plane)

    import torch

    from momlevel_amd import _lib, core
    from momlevel_amd.csrc.build import area_source_sha, source_sha

    core.require_device()
    _lib.load_area()
    print(json.dumps({"area_source_sha": area_source_sha(), "timed_source_sha": source_sha(),
                      "record": [a.nt, a.ny, a.nx], "cells": n, "window_ms": a.window_ms,
                      "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
                      "tile": {"float64": core.area_tile(torch.float64),
                               "float32": core.area_tile(torch.float32)},
                      "records_per_window": core.AREA_WINDOW, "regions": NREGIONS}), flush=True)

    gen = torch.Generator(device="cuda").manual_seed(1872)
    rec64 = torch.empty((a.nt, plane), dtype=torch.float64, device="cuda")
    land = torch.rand(plane, dtype=torch.float64, device="cuda", generator=gen) < 0.3
    for t in range(a.nt):  # (step by step: no second copy of the record while it is drawn)
        row = torch.rand(plane, dtype=torch.float64, device="cuda", generator=gen) - 0.5
        row[land] = float("nan")
        rec64[t] = row
    area = torch.rand(plane, dtype=torch.float64, device="cuda", generator=gen) * 5.0e8 + 4.0e8
    # twelve basins as bands of latitude, land in none
    slot = (torch.arange(plane, device="cuda") // a.nx * NREGIONS // a.ny).to(torch.int32)
    slot[land] = -1
    out = torch.empty((a.nt, plane), dtype=torch.float64, device="cuda")

    if a.counters:
        for _ in range(3):
            core.area_mean(rec64, area)
            mean, _ = core.area_mean(rec64, area, slot, NREGIONS)
            core.area_anomaly(rec64, mean, slot, out=out)
        torch.cuda.synchronize()
        return 0

    for label, dt in (("float64", torch.float64), ("float32", torch.float32)):
        rec = rec64 if dt == torch.float64 else rec64.to(dt)
        item = rec.element_size()
        flat = rec.view(-1)
        read = measure(f"stream probe, {label} read", lambda: core.stream_probe_mix(flat, write=False),
                       a, n * item)
        both = measure(f"stream probe, {label} read + float64 write",
                       lambda: core.stream_probe_mix(flat, out=out.view(-1), write=True), a, n * (item + 8))
        measure(f"area_mean, global, {label}", lambda: core.area_mean(rec, area), a, n * item, read)
        measure(f"area_mean, {NREGIONS} regions, {label}",
                lambda: core.area_mean(rec, area, slot, NREGIONS), a, n * item, read)
        mean, _ = core.area_mean(rec, area, slot, NREGIONS)
        measure(f"area_anomaly, {NREGIONS} regions, {label}",
                lambda: core.area_anomaly(rec, mean, slot, out=out), a, n * (item + 8), both)
        if dt == torch.float64 and a.nt % 12 == 0:
            w = torch.rand(a.nt, dtype=torch.float64, device="cuda", generator=gen) + 28.0
            gwm = torch.empty((a.nt // 12, plane), dtype=torch.float64, device="cuda")
            measure("group_weighted_mean (12 steps a group), float64",
                    lambda: core.group_weighted_mean(rec, w, 12, out=gwm), a, n * item, read)
            del gwm
        del rec, flat, mean
    return 0


if __name__ == "__main__":
    sys.exit(main())
