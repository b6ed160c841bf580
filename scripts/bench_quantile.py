"""Time the quantile kernels (csrc/momlevel_quantile.hip) on a device-generated eta-shaped record,
beside the read-only streaming probe on the same tensor, torch.sort along time on a slab of it and
numpy.nanquantile on one host thread on a smaller slab.

    python scripts/bench_quantile.py [--nt 1200 --ny 1080 --nx 1440] [--window-ms 600] [--rounds 3]
                                     [--sort-rows 135] [--numpy-rows 16]
                                     [--log profiles/quantile_kernels.log]

Per dtype (float64, float32) the cases run ALTERNATING, round after round, in one process; each is
timed with device events around enough calls to fill ``--window-ms``; the median over the rounds is
reported with the spread (min .. max) beside it.  A selection reads its rows once a pass: 16 digit
passes and the closing pass at float64 (17), 8 + 1 at float32, per (group, q); ``bytes`` is the
record's (or the groups') bytes times those passes, ``TB/s`` what that comes to and ``vs_probe`` its
ratio to the rate of ``core.stream_probe_mix(write=False)`` on the same tensor.  ``ms_per_pass`` of
a selection beside the time of ``exceed_count`` -- one pass of the same walk -- says whether the
later passes of a lane over its own rows run faster than a first one.  torch.sort and
numpy.nanquantile are timed on slabs and EXTRAPOLATED to the record by the ratio of the cells.
Every JSON line is also appended to ``--log``.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from momlevel_amd import climatology, core, hostio, synthetic  # noqa: E402
from momlevel_amd.cftime_lite import DatetimeLite  # noqa: E402
from momlevel_amd.csrc.build import quantile_source_sha  # noqa: E402
from momlevel_amd.labeled import DataArray  # noqa: E402

_log = None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if _log is not None:
        _log.write(line + "\n")
        _log.flush()


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def run_cases(label, name, cases, a):
    """cases: (case name, bytes the algorithm reads, passes over the rows, fn)"""
    calls = {}
    for cname, _b, _p, fn in cases:  # warm-up: code objects, the allocator's blocks
        fn()
        torch.cuda.synchronize()
        calls[cname] = max(1, int(np.ceil(a.window_ms / timed(fn, 1))))
    ms = {c[0]: [] for c in cases}
    for _ in range(a.rounds):
        for cname, _b, _p, fn in cases:
            ms[cname].append(timed(fn, calls[cname]))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    tbs = {c[0]: c[1] / med[c[0]] / 1e9 for c in cases}
    for cname, nbytes, passes, _fn in cases:
        row = {"record": label, "dtype": name, "case": cname, "passes": passes,
               "GB_read": round(nbytes / 1e9, 2), "calls_per_window": calls[cname],
               "ms": round(med[cname], 3), "ms_min": round(min(ms[cname]), 3),
               "ms_max": round(max(ms[cname]), 3), "ms_per_pass": round(med[cname] / passes, 3),
               "TB/s": round(tbs[cname], 3)}
        if cname != "probe_read":
            row["vs_passes_x_probe"] = round(tbs[cname] / tbs["probe_read"], 4)
        emit(row)
    return med


def monthly_axis(nt):
    return DataArray(np.array([DatetimeLite(1900 + m // 12, m % 12 + 1, 16, calendar="noleap")
                               for m in range(nt)], dtype=object), ("time",), None, None, "time")


def main():
    global _log
    ap = argparse.ArgumentParser()
    ap.add_argument("--nt", type=int, default=1200)
    ap.add_argument("--ny", type=int, default=1080)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--gauge-nt", type=int, default=15000)
    ap.add_argument("--gauge-n", type=int, default=128)
    ap.add_argument("--sort-rows", type=int, default=135)
    ap.add_argument("--numpy-rows", type=int, default=16)
    ap.add_argument("--window-ms", type=float, default=600.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    core.require_device()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        _log = open(a.log, "w")
    emit({"quantile_source_sha": quantile_source_sha(), "window_ms": a.window_ms,
          "rounds": a.rounds, "unroll": core.quantile_unroll(),
          "block_cells": [core.quantile_block_cells(torch.float64),
                          core.quantile_block_cells(torch.float32)],
          "device": torch.cuda.get_device_name(0)})
    nt, ny, nx = a.nt, a.ny, a.nx
    cells = ny * nx
    g = synthetic.make_grid(ny, nx, 2)
    mask = hostio.to_device(np.ascontiguousarray(g["volcello"][:1]), "cuda")
    plan = climatology.annual_cycle_plan(monthly_axis(nt), "time") if nt >= 12 else None

    for name, dt, item in (("float64", torch.float64, 8), ("float32", torch.float32, 4)):
        y = core.synth_field((nt, 1, ny, nx), dt, seed=synthetic.SEED, field_id=7, lo=-1.0,
                             scale=2.0, mask3d=mask).reshape(nt, ny, nx)
        passes = 2 * item + 1  # 4-bit digits of the key, and the closing pass
        record_bytes = nt * cells * item
        out1 = torch.empty((1, 1, ny, nx), dtype=dt, device="cuda")
        out3 = torch.empty((3, 1, ny, nx), dtype=dt, device="cuda")
        thr = core.time_quantile(y, 0.9)[0].to(torch.float64)
        flat = y.reshape(-1)
        cases = [
            ("probe_read", record_bytes, 1, lambda: core.stream_probe_mix(flat, write=False)),
            ("quantile q=0.5", record_bytes * passes, passes,
             lambda: core.time_quantile(y, 0.5, out=out1)),
            ("quantile q=(0.05,0.5,0.95)", 3 * record_bytes * passes, 3 * passes,
             lambda: core.time_quantile(y, [0.05, 0.5, 0.95], out=out3)),
            ("exceed_count per-cell thr", record_bytes, 1, lambda: core.time_exceed_count(y, thr)),
        ]
        if plan is not None:
            groups = core.upload_groups(plan.steps, plan.offsets, nt, y.device)
            out12 = torch.empty((1, 12, ny, nx), dtype=dt, device="cuda")
            cases.insert(3, ("quantile q=0.99 by=month", record_bytes * passes, passes,
                             lambda: core.time_quantile(y, 0.99, groups, out=out12)))
        med = run_cases(["eta", nt, ny, nx], name, cases, a)
        emit({"record": ["eta", nt, ny, nx], "dtype": name, "case": "later passes against a first one",
              "select_ms_per_pass": round(med["quantile q=0.5"] / passes, 3),
              "one_pass_ms (exceed_count)": round(med["exceed_count per-cell thr"], 3),
              "probe_read_ms": round(med["probe_read"], 3)})
        del cases, out3, thr
        torch.cuda.empty_cache()

        # torch.sort along time on a slab: what a user would otherwise do on the device (NaN sorts
        # last; values and int64 indices come back, 3 slabs' worth of memory and more)
        rows = min(a.sort_rows, ny)
        slab = y[:, :rows].contiguous()
        torch.sort(slab, dim=0)
        torch.cuda.synchronize()
        ms_sort = float(np.median([timed(lambda: torch.sort(slab, dim=0), 1) for _ in range(a.rounds)]))
        emit({"record": ["eta slab", nt, rows, nx], "dtype": name, "case": "torch.sort(dim=0)",
              "ms": round(ms_sort, 3),
              "ms_extrapolated_to_record": round(ms_sort * ny / rows, 1),
              "vs_quantile_q=0.5": round(ms_sort * ny / rows / med["quantile q=0.5"], 2)})
        del slab
        torch.cuda.empty_cache()

        # numpy.nanquantile on one host thread on a smaller slab
        rows = min(a.numpy_rows, ny)
        host = y[:, :rows].cpu().numpy()
        t0 = time.perf_counter()
        ref = np.nanquantile(host, 0.5, axis=0)
        sec = time.perf_counter() - t0
        same = np.array_equal(ref.astype(np.float64) if item == 8 else
                              np.nanquantile(host.astype(np.float64), 0.5, axis=0).astype(np.float32),
                              out1[0, 0, :rows].cpu().numpy(), equal_nan=True)
        emit({"record": ["eta slab", nt, rows, nx], "dtype": name,
              "case": "numpy.nanquantile q=0.5, one host thread", "s": round(sec, 3),
              "s_extrapolated_to_record": round(sec * ny / rows, 1),
              "vs_quantile_q=0.5": round(sec * ny / rows * 1e3 / med["quantile q=0.5"], 1),
              "values_equal_the_kernel's": bool(same)})
        del y, out1, host
        torch.cuda.empty_cache()

        # few cells, many steps (gauge series): one lane per pack, no parallelism over time
        gy = core.synth_field((a.gauge_nt, 1, 1, a.gauge_n), dt, seed=synthetic.SEED, field_id=7,
                              lo=-1.0, scale=2.0).reshape(a.gauge_nt, a.gauge_n)
        core.time_quantile(gy, 0.5)
        torch.cuda.synchronize()
        ms_g = float(np.median([timed(lambda: core.time_quantile(gy, 0.5), 3) for _ in range(a.rounds)]))
        emit({"record": ["gauges", a.gauge_nt, a.gauge_n], "dtype": name, "case": "quantile q=0.5",
              "passes": passes, "ms": round(ms_g, 3),
              "TB/s": round(a.gauge_nt * a.gauge_n * item * passes / ms_g / 1e9, 5)})
        del gy
    return 0


if __name__ == "__main__":
    sys.exit(main())
