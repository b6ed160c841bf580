"""Time the grouped time statistic (csrc/momlevel_clim.hip) on device-generated eta-shaped records,
beside the read-only streaming probe with the matching byte count and beside
k_group_weighted_mean, the existing kernel that reads the same bytes of the same tensor.

    python scripts/bench_clim.py [--nt 1200 --ny 1080 --nx 1440] [--daily-nt 3650 --daily-ny 540
                                 --daily-nx 720] [--window-ms 600] [--rounds 3] [--stats-dir DIR]

Per dtype (float64, float32) and record the cases run ALTERNATING, round after round, in one
process; each case is timed with device events around enough calls to fill ``--window-ms``; the
median over the rounds is reported with the spread (min .. max) beside it.  Bytes are what the
algorithm has to move: 8 or 4 B per cell-step, twice that for "std", which reads the record twice;
the result is ngroups / nt of the input and is not counted.  ``frac_of_8TBs`` is bytes / time over
the 8 TB/s peak; ``vs_probe`` the probe's time over the kernel's (for "std": of two probe passes);
``vs_group_weighted_mean`` that kernel's time over this one's.  The group lists are uploaded once,
outside the timed window (``core.upload_groups``): these are call times of the kernel launch.
Kernel times come from a separate ``rocprofv3 --kernel-trace --stats`` run of this script,
condensed with ``--stats-dir``.
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from momlevel_amd import cftime_lite, climatology, core, hostio, synthetic  # noqa: E402
from momlevel_amd.csrc.build import clim_source_sha  # noqa: E402
from momlevel_amd.labeled import DataArray  # noqa: E402

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
        if any(k in name for k in ("k_group_stat", "k_group_weighted", "probe")):
            print(json.dumps({"kernel": name[:150], "calls": int(r["Calls"]),
                              "avg_us": round(float(r["AverageNs"]) / 1e3, 1),
                              "min_us": round(float(r["MinNs"]) / 1e3, 1),
                              "max_us": round(float(r["MaxNs"]) / 1e3, 1)}))
    return 0


def _axis(values):
    a = np.empty(len(values), dtype=object)
    a[:] = list(values)
    return DataArray(a, ("time",), None, None, "time")


def run_cases(label, name, cases, nt, cells, a):
    """cases: (case name, bytes per cell-step, fn, probe case or None, probe passes)"""
    calls = {}
    for cname, _b, fn, _p, _k in cases:  # warm-up: code objects, the allocator's blocks
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        calls[cname] = max(1, int(np.ceil(a.window_ms / timed(fn, 1))))
    ms = {c[0]: [] for c in cases}
    for _ in range(a.rounds):
        for cname, _b, fn, _p, _k in cases:
            ms[cname].append(timed(fn, calls[cname]))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    for cname, bpc, _fn, probe, passes in cases:
        gbs = bpc * nt * cells / med[cname] / 1e6
        row = {"record": label, "dtype": name, "case": cname, "bytes_per_cell_step": bpc,
               "calls_per_window": calls[cname], "ms": round(med[cname], 3),
               "ms_min": round(min(ms[cname]), 3), "ms_max": round(max(ms[cname]), 3),
               "GB/s": round(gbs, 1), "frac_of_8TBs": round(gbs / PEAK_GBS, 4)}
        if probe:
            row["vs_probe"] = round(passes * med[probe] / med[cname], 4)
        if cname.startswith("annual_cycle") and "k_group_weighted_mean" in med:
            row["vs_group_weighted_mean"] = round(passes * med["k_group_weighted_mean"] / med[cname], 4)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nt", type=int, default=1200)
    ap.add_argument("--ny", type=int, default=1080)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--daily-nt", type=int, default=3650)
    ap.add_argument("--daily-ny", type=int, default=540)
    ap.add_argument("--daily-nx", type=int, default=720)
    ap.add_argument("--window-ms", type=float, default=600.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--stats-dir", default=None)
    a = ap.parse_args()
    if a.stats_dir:
        return condense_stats(a.stats_dir)
    core.require_device()
    print(json.dumps({"clim_source_sha": clim_source_sha(), "window_ms": a.window_ms,
                      "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}), flush=True)

    def record(nt, ny, nx, dt):
        g = synthetic.make_grid(ny, nx, 2)
        mask = hostio.to_device(np.ascontiguousarray(g["volcello"][:1]), "cuda")
        return core.synth_field((nt, 1, ny, nx), dt, seed=synthetic.SEED, field_id=7, lo=-1.0,
                                scale=2.0, mask3d=mask).reshape(nt, ny, nx)

    for name, dt, item in (("float64", torch.float64, 8), ("float32", torch.float32, 4)):
        # ---- monthly record: annual_cycle, all four statistics ------------------------------
        nt, ny, nx = a.nt - a.nt % 12, a.ny, a.nx
        plan = climatology.annual_cycle_plan(_axis(cftime_lite.monthly_midpoints(1900, nt // 12, "noleap")))
        y = record(nt, ny, nx, dt)
        flat = y.reshape(-1)
        groups = core.upload_groups(plan.steps, plan.offsets, nt, y.device)
        out = torch.empty((12, ny, nx), dtype=dt, device="cuda")
        cases = [(f"annual_cycle {s}", item * (2 if s == "std" else 1),
                  (lambda s=s: core.time_group_stat(y, groups, stat=s, out=out)), "probe_read",
                  2 if s == "std" else 1) for s in climatology.STATS]
        cases.append(("probe_read", item, lambda: core.stream_probe_mix(flat, write=False), None, 1))
        if dt == torch.float64:
            w = hostio.to_device(np.tile([31., 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31], nt // 12), "cuda")
            gwm_out = torch.empty((nt // 12, ny, nx), dtype=torch.float64, device="cuda")
            cases.append(("k_group_weighted_mean", item,
                          lambda: core.group_weighted_mean(y, w, 12, out=gwm_out), "probe_read", 1))
        run_cases([nt, ny, nx], name, cases, nt, ny * nx, a)
        del y, flat, out, cases
        if dt == torch.float64:
            del gwm_out
        torch.cuda.empty_cache()
        # ---- daily record: monthly_average ---------------------------------------------------
        nyears = max(1, a.daily_nt // 365)
        nt, ny, nx = nyears * 365, a.daily_ny, a.daily_nx
        plan = climatology.monthly_plan(_axis(cftime_lite.daily_midpoints(1900, nyears, "noleap")))
        y = record(nt, ny, nx, dt)
        flat = y.reshape(-1)
        groups = core.upload_groups(plan.steps, plan.offsets, nt, y.device)
        out = torch.empty((plan.ngroups, ny, nx), dtype=dt, device="cuda")
        cases = [("monthly_average", item, lambda: core.time_group_stat(y, groups, stat="mean", out=out),
                  "probe_read", 1),
                 ("probe_read", item, lambda: core.stream_probe_mix(flat, write=False), None, 1)]
        run_cases([nt, ny, nx], name, cases, nt, ny * nx, a)
        del y, flat, out, cases
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
