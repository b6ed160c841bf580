"""Time the trend kernels (csrc/momlevel_trend.hip) on a device-generated eta-shaped record, beside
the streaming probes with the matching byte mix and beside k_group_weighted_mean, the existing
kernel with the same time-strided access pattern.

    python scripts/bench_trend.py [--nt 1200 --ny 1080 --nx 1440] [--window-ms 600] [--rounds 3]
                                  [--no-polyfit] [--stats-dir DIR]

Per dtype (float64, float32) the cases run ALTERNATING, round after round, in one process; each
case is timed with device events around enough calls to fill ``--window-ms``; the median over the
rounds is reported with the spread (min .. max) beside it.  Bytes are what the algorithm has to
move: fit / projection read the record once (8 or 4 B per cell-step), the apply pass (the straight
line removed, and the residual of the 6-term seasonal model) reads it and writes float64 (16 or
12 B). ``frac_of_8TBs`` is bytes / time over the 8 TB/s peak; ``vs_probe``
the probe's time over the kernel's.  These are call times (workspace allocation from torch's
cache and the small finishing kernel included); kernel times come from a separate
``rocprofv3 --kernel-trace --stats`` run of this script, condensed with ``--stats-dir``.
np.polyfit on a 1/64 slab of the same record on the host is printed as a stated baseline.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from momlevel_amd import core, hostio, synthetic, trend  # noqa: E402
from momlevel_amd.csrc.build import trend_source_sha  # noqa: E402

PEAK_GBS = 8000.0


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def condense_stats(stats_dir):
    """kernel times of a rocprofv3 --kernel-trace --stats run of this script, one line per kernel"""
    hits = sorted(glob.glob(os.path.join(stats_dir, "**", "*_kernel_stats.csv"), recursive=True))
    if not hits:
        print(json.dumps({"kernel_stats": "no *_kernel_stats.csv under " + stats_dir}))
        return 1
    for r in csv.DictReader(open(hits[0])):
        name = r["Name"]
        if any(k in name for k in ("k_time_", "k_linfit", "k_project", "k_group_weighted",
                                   "k_stream_probe", "probe")):
            print(json.dumps({"kernel": name[:150], "calls": int(r["Calls"]),
                              "avg_us": round(float(r["AverageNs"]) / 1e3, 1),
                              "min_us": round(float(r["MinNs"]) / 1e3, 1),
                              "max_us": round(float(r["MaxNs"]) / 1e3, 1)}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nt", type=int, default=1200)
    ap.add_argument("--ny", type=int, default=1080)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--window-ms", type=float, default=600.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-polyfit", action="store_true")
    ap.add_argument("--stats-dir", default=None)
    a = ap.parse_args()
    if a.stats_dir:
        return condense_stats(a.stats_dir)
    core.require_device()
    nt, ny, nx = a.nt, a.ny, a.nx
    nt -= nt % 12  # whole groups for k_group_weighted_mean
    cells = ny * nx
    g = synthetic.make_grid(ny, nx, 2)
    mask = hostio.to_device(np.ascontiguousarray(g["volcello"][:1]), "cuda")
    x = np.arange(nt, dtype=np.float64) * 30.4 * 86400e9 + 3.5e17  # a monthly axis, in ns
    xt, s, xmean = trend.fit_axis(x)
    model, pmodel = trend.seasonal_model_matrix(np.arange(nt) / 12.0)
    xd, xtd = hostio.to_device(x, "cuda"), hostio.to_device(xt, "cuda")
    Md, Pd = hostio.to_device(model, "cuda"), hostio.to_device(pmodel, "cuda")
    w = hostio.to_device(np.tile([31., 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31], nt // 12), "cuda")
    print(json.dumps({"record": [nt, ny, nx], "trend_source_sha": trend_source_sha(),
                      "window_ms": a.window_ms, "rounds": a.rounds,
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    out = torch.empty((nt, ny, nx), dtype=torch.float64, device="cuda")
    for name, dt, item in (("float64", torch.float64, 8), ("float32", torch.float32, 4)):
        y = core.synth_field((nt, 1, ny, nx), dt, seed=synthetic.SEED, field_id=7, lo=-1.0,
                             scale=2.0, mask3d=mask).reshape(nt, ny, nx)
        flat = y.reshape(-1)
        slope, icpt = core.time_linfit(y, xtd, s, xmean)
        coef = core.time_project(y, Pd)
        gwm_out = torch.empty((nt // 12, ny, nx), dtype=torch.float64, device="cuda")
        cases = [
            ("k_time_linfit", item, lambda: core.time_linfit(y, xtd, s, xmean), "probe_read"),
            ("k_time_project<6>", item, lambda: core.time_project(y, Pd), "probe_read"),
            ("probe_read", item, lambda: core.stream_probe_mix(flat, write=False), None),
            ("k_time_apply remove", item + 8,
             lambda: core.time_apply(y, "remove", xd, slope, icpt, out=out), "probe_read_write"),
            ("k_time_apply model_resid<6>", item + 8,
             lambda: core.time_apply(y, "model_resid", Md, coef, out=out), "probe_read_write"),
            ("probe_read_write", item + 8,
             lambda: core.stream_probe_mix(flat, out=out.reshape(-1), write=True), None),
        ]
        if dt == torch.float64:
            cases.append(("k_group_weighted_mean", item,
                          lambda: core.group_weighted_mean(y, w, 12, out=gwm_out), "probe_read"))
        calls = {}
        for cname, _b, fn, _p in cases:  # warm-up: code objects, the allocator's blocks
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            calls[cname] = max(1, int(np.ceil(a.window_ms / timed(fn, 1))))
        ms = {cname: [] for cname, *_ in cases}
        for _ in range(a.rounds):
            for cname, _b, fn, _p in cases:
                ms[cname].append(timed(fn, calls[cname]))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for cname, bpc, _fn, probe in cases:
            gbs = bpc * nt * cells / med[cname] / 1e6
            row = {"dtype": name, "case": cname, "bytes_per_cell_step": bpc,
                   "calls_per_window": calls[cname], "ms": round(med[cname], 3),
                   "ms_min": round(min(ms[cname]), 3), "ms_max": round(max(ms[cname]), 3),
                   "GB/s": round(gbs, 1), "frac_of_8TBs": round(gbs / PEAK_GBS, 4)}
            if probe:
                row["vs_probe"] = round(med[probe] / med[cname], 4)
            if cname in ("k_time_linfit", "k_time_project<6>") and "k_group_weighted_mean" in med:
                row["vs_group_weighted_mean"] = round(med["k_group_weighted_mean"] / med[cname], 4)
            print(json.dumps(row), flush=True)
        if not a.no_polyfit and dt == torch.float64:
            slab = hostio.to_host(y.reshape(nt, cells)[:, : cells // 64].contiguous())
            ocean = slab[:, ~np.isnan(slab).any(axis=0)]
            t0 = time.perf_counter()
            np.polyfit(x, ocean, 1)
            dt_s = time.perf_counter() - t0
            print(json.dumps({"baseline": "np.polyfit on the host, 1/64 slab (ocean columns only)",
                              "columns": int(ocean.shape[1]), "wall_s": round(dt_s, 3),
                              "whole_record_s_extrapolated": round(dt_s * 64, 1)}), flush=True)
        del y, flat, slope, icpt, coef, gwm_out, cases
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
