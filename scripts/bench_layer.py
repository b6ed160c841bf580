"""Time the layer-integral kernel (csrc/momlevel_layer.hip) and steric_layers end to end:

    python scripts/bench_layer.py [--kernel] [--end-to-end] [--window-ms 300] [--rounds 5] [--reps 5]

(both parts when neither is named; the output, one JSON object a line, is what
profiles/layer_kernels.log holds).

KERNEL (``--kernel``): a resident (32, 75, 1080, 1440) field, float64 and float32, with 1, 3 and 8
layers -- the whole column; [0, 700, 2000, sea floor]; eight consecutive layers -- timed with device
events around enough calls to fill ``--window-ms``, median over the rounds with the spread, beside
``core.stream_probe_mix(x, write=False)`` over the same bytes in the same process (``vs_probe`` =
probe time / kernel time: the project's other one-stream readers stand at 0.79 (trend fit) to 0.94
(global area mean) of it).  The algorithmic bytes are the field once; the nl planes per record that
are written (8 nl / (nz itemsize) of the read) are left out, so the rate is what a caller sees.

END TO END (``--end-to-end``): the reference's recorded call's shape, 60 x 35 x 1080 x 1440 float32
from host memory (scripts/example_call.py builds it): ``steric_layers(ds, [0, 700, 2000, None],
variants=("thermosteric",))`` against ``thermosteric(ds)`` and against ``thermosteric(ds)`` with
MOMLEVEL_AMD_DELTA_RHO=0, alternating, wall clock around calls that end with host arrays.  Every
repetition is written down; the first two calls of each are the warm-up (the summary line takes
the third on).
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s, MI355X
KERNEL_SHAPE = (32, 75, 1080, 1440)


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


def kernel_part(a):
    import torch

    from momlevel_amd import core, synthetic

    nrec, nz, ny, nx = a.nrec, a.nz, a.ny, a.nx
    plane = ny * nx
    g = synthetic.make_grid(ny, nx, nz)
    z_i = torch.from_numpy(g["z_i"]).cuda()
    depth = torch.from_numpy(g["deptho"]).cuda().reshape(-1)
    surface = torch.from_numpy(g["volcello"][0]).cuda().reshape(-1)
    zb = float(g["z_i"][-1])
    cases = {
        "1 layer (whole column)": ([0.0], [np.inf]),
        "3 layers [0, 700, 2000, floor]": ([0.0, min(700.0, 0.1 * zb), min(2000.0, 0.3 * zb)],
                                           [min(700.0, 0.1 * zb), min(2000.0, 0.3 * zb), np.inf]),
        "8 consecutive layers": ([zb * k / 8 for k in range(8)],
                                 [zb * (k + 1) / 8 for k in range(7)] + [np.inf]),
        "8 overlapping layers (0 .. k/8 of the column)": ([0.0] * 8,
                                                          [zb * (k + 1) / 8 for k in range(7)] + [np.inf]),
    }
    print(json.dumps({"part": "kernel", "field": [nrec, nz, ny, nx], "steps": core.LAYER_STEPS,
                      "layer_max": core.LAYER_MAX, "z_i_last": zb}), flush=True)
    vol0 = torch.from_numpy(g["volcello"]).cuda()
    for label, dt in (("float64", torch.float64), ("float32", torch.float32)):
        x = core.synth_field((nrec, nz, ny, nx), dt, seed=synthetic.SEED, field_id=1, lo=-2.0,
                             scale=34.0, mask3d=vol0).reshape(nrec, nz, plane)
        nbytes = x.numel() * x.element_size()
        flat = x.view(-1)
        probe = measure(f"stream probe, {label} read", lambda: core.stream_probe_mix(flat, write=False),
                        a, nbytes)
        for name, (tops, bottoms) in cases.items():
            out = torch.empty((nrec, len(tops), plane), dtype=torch.float64, device="cuda")
            measure(f"layer_integral, {name}, {label}",
                    lambda: core.layer_integral(x, z_i, depth, tops, bottoms, surface=surface,
                                                scale=-1.0 / 1035.0, out=out), a, nbytes, probe)
            del out
        del x, flat
        torch.cuda.empty_cache()


def end_to_end_part(a):
    import torch

    import momlevel_amd as m
    from momlevel_amd import core, hostio, synthetic
    from momlevel_amd.labeled import DataArray, Dataset

    nt, nz, ny, nx = a.e2e_nt, a.e2e_nz, a.ny, a.nx
    shape = (nt, nz, ny, nx)
    g = synthetic.make_grid(ny, nx, nz)
    vol0 = hostio.to_device(g["volcello"], "cuda")
    host = {}
    for name, fid, lo, sc in (("thetao", 1, -2.0, 34.0), ("so", 2, 30.0, 10.0)):
        dev = core.synth_field(shape, torch.float32, seed=synthetic.SEED, mask3d=vol0, field_id=fid,
                               lo=lo, scale=sc)
        host[name] = hostio.to_host(dev)  # plain (pageable) numpy arrays, as a user has
        del dev
    del vol0
    torch.cuda.empty_cache()
    d = Dataset()
    d["time"] = DataArray(np.arange(nt, dtype=float), ("time",))
    d["z_l"] = DataArray(g["z_l"], ("z_l",))
    d["z_i"] = DataArray(g["z_i"], ("z_i",))
    dims = ("time", "z_l", "yh", "xh")
    d["thetao"] = DataArray(host["thetao"], dims)
    d["so"] = DataArray(host["so"], dims)
    d["volcello"] = DataArray(np.broadcast_to(g["volcello"].astype(np.float32), shape), dims)
    d["areacello"] = DataArray(g["areacello"].astype(np.float32), ("yh", "xh"))
    d["deptho"] = DataArray(g["deptho"], ("yh", "xh"))
    zb = float(g["z_i"][-1])
    layers = [0.0, 700.0, 2000.0, None] if zb > 2000.0 else [0.0, 0.1 * zb, 0.3 * zb, None]
    cells = nt * nz * ny * nx

    def layers_call():
        res, _ = m.steric_layers(d, layers, variants=("thermosteric",))
        return res["thermosteric"]["thermosteric_layers"].values.shape

    def plain_call():
        res, _ = m.thermosteric(d)
        return res["delta_rho"].values.shape

    def no_drho_call():
        os.environ["MOMLEVEL_AMD_DELTA_RHO"] = "0"
        try:
            res, _ = m.thermosteric(d)
        finally:
            del os.environ["MOMLEVEL_AMD_DELTA_RHO"]
        return res["thermosteric"].values.shape

    calls = (("steric_layers(ds, [0, 700, 2000, None], variants=('thermosteric',))", layers_call),
             ("thermosteric(ds)", plain_call),
             ("thermosteric(ds), MOMLEVEL_AMD_DELTA_RHO=0", no_drho_call))
    print(json.dumps({"part": "end to end", "shape_t_z_y_x": list(shape), "cells": cells,
                      "layers": [None if v is None else v for v in layers], "reps": a.reps,
                      "host_bytes_streamed_in_GB": round(cells * 4 / 1e9, 2)}), flush=True)
    walls = {name: [] for name, _ in calls}
    for rep in range(a.reps):  # alternating: a drift of the box shows in all three alike
        for name, fn in calls:
            gc.collect()
            t0 = time.perf_counter()
            shape_out = fn()
            walls[name].append(round(time.perf_counter() - t0, 4))
            print(json.dumps({"call": name, "rep": rep, "wall_s": walls[name][-1],
                              "result": list(shape_out)}), flush=True)
    for name, w in walls.items():
        steady = w[2:]
        print(json.dumps({"call": name, "wall_s_all": w, "from_the_third_call_on": steady,
                          "median_s": round(float(np.median(steady)), 4) if steady else None}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--nrec", type=int, default=KERNEL_SHAPE[0])
    ap.add_argument("--nz", type=int, default=KERNEL_SHAPE[1])
    ap.add_argument("--ny", type=int, default=KERNEL_SHAPE[2])
    ap.add_argument("--nx", type=int, default=KERNEL_SHAPE[3])
    ap.add_argument("--e2e-nt", type=int, default=60)
    ap.add_argument("--e2e-nz", type=int, default=35)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    both = not (a.kernel or a.end_to_end)

    import torch

    from momlevel_amd import _lib, core
    from momlevel_amd.csrc.build import layer_source_sha, source_sha

    core.require_device()  # no GPU: an error, never a CPU timing
    _lib.load_layer()
    print(json.dumps({"layer_source_sha": layer_source_sha(), "timed_source_sha": source_sha(),
                      "window_ms": a.window_ms, "rounds": a.rounds,
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    if a.kernel or both:
        kernel_part(a)
    if a.end_to_end or both:
        end_to_end_part(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
