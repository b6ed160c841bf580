"""Time the column-search kernel (csrc/momlevel_column.hip) on one resident 0.25-degree step:

    python scripts/bench_column.py [--log profiles/column_kernels.log] [--window-ms 300] [--rounds 5]

(the output, one JSON object a line, is what profiles/column_kernels.log holds).

One (1, 75, 1080, 1440) step of theta and S, float64 and then float32, each dtype in a process of
its own that is started under a time limit; nothing more is started after a step that failed.  In
that process, on the same tensors, timed with device events around enough calls to fill
``--window-ms``, median over the rounds with the spread:

  * ``core.stream_probe_mix(theta, so, write=False)``: the two-stream read probe;
  * ``core.eos_map(theta, so, p_ref)``: reads the same 16 (8) B/cell, writes 8 more;
  * ``calc_mld``'s launch (SIGMA source, RISE, relative 0.03, FLOOR) on a field with a shallow
    mixed layer (10 to 70 m of a 6 km column: the wave stops reading at its deepest crossing);
  * the same launch on a field that never crosses (constant theta and S: the whole column is read);
  * three isopycnals (SIGMA source, RISE, absolute) on the mixed-layer field.

What follows from the byte counts is a condition, not a number: the no-crossing search moves no
more bytes than eos_map, so it should not take longer (``nocross_over_eos_map`` <= 1); the shallow
search should take less than the no-crossing one (``shallow_over_nocross`` < 1).  Both ratios, the
achieved fraction of the read probe and the launch shape are written down; a condition that fails
is said so in the summary line (``conditions_hold`` false), not tuned away.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s, MI355X
SHAPE = (1, 75, 1080, 1440)
STEP_LIMIT_S = 300


def timed(fn, calls):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def measure(name, fn, a, nbytes, emit):
    import torch

    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    calls = max(1, int(np.ceil(a.window_ms / max(timed(fn, 1), 1e-3))))
    ms = [timed(fn, calls) for _ in range(a.rounds)]
    med = float(np.median(ms))
    emit({"case": name, "calls_per_window": calls, "ms": round(med, 4), "ms_min": round(min(ms), 4),
          "ms_max": round(max(ms), 4), "input_bytes": nbytes,
          "TB/s_of_the_whole_input": round(nbytes / med / 1e9, 3)})
    return med


def fields(dt, nz, ny, nx):
    """(theta, so) with a shallow mixed layer, (theta, so) that never cross, z_l, deptho: device"""
    import torch

    from momlevel_amd import synthetic

    g = synthetic.make_grid(ny, nx, nz)
    z = torch.from_numpy(g["z_l"]).cuda()
    wet = ~torch.isnan(torch.from_numpy(g["volcello"]).cuda())
    yy = torch.arange(ny, device="cuda", dtype=torch.float64).reshape(ny, 1)
    xx = torch.arange(nx, device="cuda", dtype=torch.float64).reshape(1, nx)
    h = 40.0 + 30.0 * torch.sin(2 * np.pi * xx / nx) * torch.cos(2 * np.pi * yy / ny)  # 10 .. 70 m
    below = torch.clamp(z.reshape(nz, 1, 1) - h, min=0.0)
    theta = 20.0 - 15.0 * (1.0 - torch.exp(-below / 200.0))
    nan = torch.full_like(theta, float("nan"))
    theta = torch.where(wet, theta, nan).to(dt).reshape(1, nz, ny, nx).contiguous()
    so = torch.where(wet, torch.full_like(nan, 35.0), nan).to(dt).reshape(1, nz, ny, nx).contiguous()
    flat_t = torch.where(wet, torch.full_like(nan, 10.0), nan).to(dt).reshape(1, nz, ny, nx).contiguous()
    return (theta, so), (flat_t, so), z, torch.from_numpy(g["deptho"]).cuda().reshape(-1), h


def step(a, label):
    """every measurement of one dtype, in this process, on the same tensors"""
    import torch

    from momlevel_amd import _lib, core
    from momlevel_amd.csrc.build import column_source_sha, source_sha

    core.require_device()  # no GPU: an error, never a CPU timing
    _lib.load_column()

    def emit(row):
        print(json.dumps(row), flush=True)

    dt = torch.float64 if label == "float64" else torch.float32
    nrec, nz, ny, nx = SHAPE[0], a.nz, a.ny, a.nx
    plane = ny * nx
    emit({"step": label, "column_source_sha": column_source_sha(), "timed_source_sha": source_sha(),
          "device": torch.cuda.get_device_name(0), "field": [nrec, nz, ny, nx],
          "window_ms": a.window_ms, "rounds": a.rounds,
          "launch_shape": {"threads_per_block": 256, "cells_per_block": core.column_block_cells(dt, dt),
                           "record_rows": core.column_record_rows(nrec), "records_per_thread": 1},
          "launch_shapes_tried": "this one only"})
    (theta, so), (flat_t, flat_s), z, deptho, h = fields(dt, nz, ny, nx)
    p_ref = 101325.0
    p_dev = torch.tensor([p_ref], dtype=torch.float64, device="cuda")  # (resident: no upload per call)
    kref = int(np.argmin(np.abs(z.cpu().numpy() - 10.0)))
    nbytes = 2 * theta.numel() * theta.element_size()
    t3, s3 = theta.reshape(nrec, nz, plane), so.reshape(nrec, nz, plane)
    f3 = flat_t.reshape(nrec, nz, plane)
    out1 = torch.empty((nrec, 1, plane), dtype=torch.float64, device="cuda")
    out3 = torch.empty((nrec, 3, plane), dtype=torch.float64, device="cuda")
    rho = torch.empty(theta.shape, dtype=torch.float64, device="cuda")
    mld = dict(kref=kref, mode="rise", relative=True, miss="floor", floor=deptho, p_ref=p_ref)

    probe = measure(f"stream_probe_mix, two {label} streams read, no write",
                    lambda: core.stream_probe_mix(theta.view(-1), so.view(-1), write=False), a, nbytes, emit)
    eos = measure(f"eos_map density, {label}", lambda: core.eos_map(theta, so, p_dev, out=rho), a, nbytes, emit)
    shallow = measure(f"mld launch, shallow mixed layer, {label}",
                      lambda: core.column_crossing(t3, z, [0.03], b=s3, out=out1, **mld), a, nbytes, emit)
    got = out1.reshape(ny, nx)
    ok = ~torch.isnan(got)
    emit({"check": "shallow mixed layer", "kref": kref, "wet_cells": int(ok.sum()),
          "mld_min_m": round(float(got[ok].min()), 2), "mld_max_m": round(float(got[ok].max()), 2),
          "levels_above_the_deepest_mld": int((z <= got[ok].max()).sum()), "levels": nz})
    nocross = measure(f"mld launch, never crosses (whole column read), {label}",
                      lambda: core.column_crossing(f3, z, [0.03], b=s3, out=out1, **mld), a, nbytes, emit)
    got = out1.reshape(-1)
    ok = ~torch.isnan(got)
    emit({"check": "never crosses", "all_misses_equal_deptho": bool(torch.equal(got[ok], deptho[ok]))})
    iso = measure(f"three isopycnals (1025.5, 1026.5, 1027.5), {label}",
                  lambda: core.column_crossing(t3, z, [1025.5, 1026.5, 1027.5], b=s3, mode="rise",
                                               p_ref=p_ref, out=out3), a, nbytes, emit)
    emit({"check": "isopycnals", "finite_fraction": [round(float((~torch.isnan(out3[0, j])).double().mean()), 3)
                                                     for j in range(3)]})
    ratios = {"nocross_over_eos_map": round(nocross / eos, 4), "shallow_over_nocross": round(shallow / nocross, 4),
              "nocross_fraction_of_read_probe": round(probe / nocross, 4),
              "isopycnals_over_nocross": round(iso / nocross, 4)}
    ratios["conditions_hold"] = bool(ratios["nocross_over_eos_map"] <= 1.0 and ratios["shallow_over_nocross"] < 1.0)
    emit({"summary": label, **ratios})
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["float64", "float32"], help="(internal) one dtype, in this process")
    ap.add_argument("--log", default=None, help="also write the lines to this file")
    ap.add_argument("--nz", type=int, default=SHAPE[1])
    ap.add_argument("--ny", type=int, default=SHAPE[2])
    ap.add_argument("--nx", type=int, default=SHAPE[3])
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if a.step:
        return step(a, a.step)
    lines = []
    rc = 0
    for label in ("float64", "float32"):  # a fresh process per step, each under its own time limit
        cmd = [sys.executable, os.path.abspath(__file__), "--step", label, "--nz", str(a.nz), "--ny", str(a.ny),
               "--nx", str(a.nx), "--window-ms", str(a.window_ms), "--rounds", str(a.rounds)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
            out, rc = res.stdout, res.returncode
            if rc != 0:
                out += json.dumps({"step": label, "failed": rc, "stderr_tail": res.stderr[-2000:]}) + "\n"
        except subprocess.TimeoutExpired as exc:
            out = (exc.stdout or b"").decode() if isinstance(exc.stdout, bytes) else (exc.stdout or "")
            out += json.dumps({"step": label, "failed": f"time limit of {STEP_LIMIT_S} s"}) + "\n"
            rc = 124
        sys.stdout.write(out)
        sys.stdout.flush()
        lines.append(out)
        if rc != 0:  # nothing more starts after a failed step
            break
    if a.log:
        with open(a.log, "w") as f:
            f.writelines(lines)
    return rc


if __name__ == "__main__":
    sys.exit(main())
