"""Time the time filter (csrc/momlevel_filter.hip) on device-generated eta-shaped records, beside
the read+write streaming probe on the same tensors and beside core.time_group_stat with one W-step
group per output step -- how a running mean had to be done before the kernel existed.

    python scripts/bench_filter.py [--nt 1200 --ny 1080 --nx 1440] [--daily-nt 3650 --daily-ny 540
                                   --daily-nx 720] [--window-ms 600] [--rounds 3]
                                   [--log profiles/filter_kernels.log]

Per dtype (float64, float32) and record the cases run ALTERNATING, round after round, in one
process; each case is timed with device events around enough calls to fill ``--window-ms``; the
median over the rounds is reported with the spread (min .. max) beside it.  Bytes are what the
algorithm has to move: the record once in, the result once out (16 B per cell-step at float64, 8 B
at float32; rolling_trend writes float64).  ``vs_probe`` is the kernel's GB/s over the GB/s of
``core.stream_probe_mix(write=True)`` on the same record (the probe always writes float64: 16 B per
element at float64, 12 B at float32 -- hence the comparison of rates, not of times);
``vs_group_stat`` is the time of ``core.time_group_stat`` over the kernel's.  Weights and group
lists are uploaded once, outside the timed window.  Every JSON line is also appended to ``--log``.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from momlevel_amd import core, filters, hostio, synthetic  # noqa: E402
from momlevel_amd.csrc.build import filter_source_sha  # noqa: E402

PEAK_GBS = 8000.0
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


def run_cases(label, name, cases, nt, cells, a):
    """cases: (case name, bytes per cell-step, fn, baseline case or None)"""
    calls = {}
    for cname, _b, fn, _base in cases:  # warm-up: code objects, the allocator's blocks
        fn()
        torch.cuda.synchronize()
        calls[cname] = max(1, int(np.ceil(a.window_ms / timed(fn, 1))))
    ms = {c[0]: [] for c in cases}
    for _ in range(a.rounds):
        for cname, _b, fn, _base in cases:
            ms[cname].append(timed(fn, calls[cname]))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    gbs = {c[0]: c[1] * nt * cells / med[c[0]] / 1e6 for c in cases}
    for cname, bpc, _fn, base in cases:
        row = {"record": label, "dtype": name, "case": cname, "bytes_per_cell_step": bpc,
               "calls_per_window": calls[cname], "ms": round(med[cname], 3),
               "ms_min": round(min(ms[cname]), 3), "ms_max": round(max(ms[cname]), 3),
               "GB/s": round(gbs[cname], 1), "frac_of_8TBs": round(gbs[cname] / PEAK_GBS, 4)}
        if cname != "probe_read_write" and not cname.startswith("group_stat"):
            row["vs_probe"] = round(gbs[cname] / gbs["probe_read_write"], 4)
        if base:
            row["vs_group_stat"] = round(med[base] / med[cname], 3)
        emit(row)


def window_groups(nt, window):
    lead = filters.window_lead(window, True)
    members = [np.arange(max(t - lead, 0), min(t - lead + window, nt)) for t in range(nt)]
    return np.concatenate(members), np.concatenate([[0], np.cumsum([len(m) for m in members])])


def main():
    global _log
    ap = argparse.ArgumentParser()
    ap.add_argument("--nt", type=int, default=1200)
    ap.add_argument("--ny", type=int, default=1080)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--daily-nt", type=int, default=3650)
    ap.add_argument("--daily-ny", type=int, default=540)
    ap.add_argument("--daily-nx", type=int, default=720)
    ap.add_argument("--window-ms", type=float, default=600.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    core.require_device()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        _log = open(a.log, "w")
    emit({"filter_source_sha": filter_source_sha(), "window_ms": a.window_ms, "rounds": a.rounds,
          "tile": core.filter_tile(), "window_edges": list(core.filter_window_edges()),
          "device": torch.cuda.get_device_name(0)})

    def record(nt, ny, nx, dt):
        g = synthetic.make_grid(ny, nx, 2)
        mask = hostio.to_device(np.ascontiguousarray(g["volcello"][:1]), "cuda")
        return core.synth_field((nt, 1, ny, nx), dt, seed=synthetic.SEED, field_id=7, lo=-1.0,
                                scale=2.0, mask3d=mask).reshape(nt, ny, nx)

    def dev(w):
        return hostio.to_device(np.ascontiguousarray(w, dtype=np.float64), "cuda", torch.float64)

    def filter_cases(y, out, out64, item, windows, with_trend, nt):
        cases = []
        for W in windows:
            lead = W // 2
            ones = dev(np.ones(W))
            lan = dev(filters.lanczos_weights(W, W / 3.0))
            groups = core.upload_groups(*window_groups(nt, W), nt, y.device)
            cases.append((f"rolling_mean W={W}", 2 * item,
                          lambda ones=ones, lead=lead, W=W: core.time_filter(y, ones, lead, W, True, out=out),
                          f"group_stat W={W}"))
            cases.append((f"lowpass W={W}", 2 * item,
                          lambda lan=lan, lead=lead, W=W: core.time_filter(y, lan, lead, W, False, out=out),
                          None))
            cases.append((f"group_stat W={W}", 2 * item,
                          lambda groups=groups: core.time_group_stat(y, groups, stat="mean", out=out), None))
        if with_trend:
            W = with_trend
            x = np.cumsum(np.tile([31., 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31], nt // 12 + 1)[:nt])
            table = dev(filters.trend_table(x, W, W // 2))
            cases.append((f"rolling_trend W={W}", item + 8,
                          lambda: core.time_filter(y, table, W // 2, W, False, out=out64,
                                                   out_dtype=torch.float64), None))
        flat = y.reshape(-1)
        cases.append(("probe_read_write", item + 8,
                      lambda: core.stream_probe_mix(flat, out=out64.reshape(-1), write=True), None))
        return cases

    for name, dt, item in (("float64", torch.float64, 8), ("float32", torch.float32, 4)):
        for label, (nt, ny, nx), windows, with_trend in (
                ("monthly", (a.nt, a.ny, a.nx), (13, 61, 241), 241),
                ("daily", (a.daily_nt, a.daily_ny, a.daily_nx), (31, 365), 0)):
            windows = tuple(w for w in windows if w <= nt)
            y = record(nt, ny, nx, dt)
            out = torch.empty_like(y)
            out64 = out if dt == torch.float64 else torch.empty(y.shape, dtype=torch.float64,
                                                                device="cuda")
            cases = filter_cases(y, out, out64, item, windows,
                                 with_trend if with_trend and with_trend <= nt else 0, nt)
            run_cases([label, nt, ny, nx], name, cases, nt, ny * nx, a)
            del y, out, out64, cases
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
