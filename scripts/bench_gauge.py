"""Time the tide-gauge kernels (csrc/momlevel_gauge.hip) at the 0.25-degree shape: prepare and nearest
on a 1080 x 1440 grid with 1500 gauges, gather out of a (1200, 1080, 1440) float32 record.

    python scripts/bench_gauge.py [--ny 1080 --nx 1440 --gauges 1500 --nt 1200] [--window-ms 300]
                                  [--rounds 3] [--host-gauges 4] [--skip-host]

Each case is timed with device events around enough calls to fill ``--window-ms``; the median over
the rounds is reported with the spread (min .. max).  ``nearest`` is the two launches of
mlx_gauge_nearest (search + combine).  Beside it: the pair count (valid or not, every point is
compared with every gauge), the float64 VALU lane-instructions the search issues per pair (8
arithmetic: 3 subtractions, 3 multiplications, 2 additions; 1 compare; the selects are 32-bit and
not counted) and the rate they imply -- to be read against the float64 issue ceiling mlx_valu_probe
measures on the same box, printed next to it.  The record is shortened (and the line says so) when
it does not fit the free device memory.

On the host, for scale: the numpy restatement's brute force (tests/gauge_numpy.py) on
``--host-gauges`` gauges over the full grid, EXTRAPOLATED linearly to all gauges and labelled so,
and scikit-learn's BallTree (build + query of all gauges) when scikit-learn is importable.
Nothing is gated on these numbers.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gauge_numpy as gn  # noqa: E402
from momlevel_amd import _lib, core  # noqa: E402
from momlevel_amd.csrc.build import gauge_source_sha  # noqa: E402

F64_PER_PAIR = 9  # 3 v_add (sub) + 3 v_mul + 2 v_add + 1 v_cmp, all float64


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def measure(name, fn, a, extra=None):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    calls = max(1, int(np.ceil(a.window_ms / max(timed(fn, 1), 1e-3))))
    ms = [timed(fn, calls) for _ in range(a.rounds)]
    row = {"case": name, "calls_per_window": calls, "ms": round(float(np.median(ms)), 4),
           "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
    row.update(extra(float(np.median(ms))) if extra else {})
    print(json.dumps(row), flush=True)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ny", type=int, default=1080)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--gauges", type=int, default=1500)
    ap.add_argument("--nt", type=int, default=1200)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-gauges", type=int, default=4)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    core.require_device()
    lib = _lib.load_gauge()
    n, ng = a.ny * a.nx, a.gauges
    print(json.dumps({"gauge_source_sha": gauge_source_sha(), "grid": [a.ny, a.nx], "gauges": ng,
                      "window_ms": a.window_ms, "rounds": a.rounds,
                      "device": torch.cuda.get_device_name(0)}), flush=True)

    lat, lon, mask, glat, glon = gn.synthetic_grid(a.ny, a.nx, ng, seed=7)
    dlat, dlon, dmask = (torch.from_numpy(x).cuda() for x in (lat, lon, mask))
    measure("prepare (grid, float64 lat / lon / mask)", lambda: core.gauge_prepare(dlat, dlon, dmask), a,
            lambda ms: {"points": n, "Gpoints/s": round(n / ms / 1e6, 2)})
    points, valid = core.gauge_prepare(dlat, dlon, dmask)
    gauges, _ = core.gauge_prepare(glat, glon)
    split = lib.mlx_gauge_nearest_split(n, ng, 0)
    pairs = n * ng

    def rate(ms):
        return {"pairs": pairs, "split": split, "f64_lane_instructions_per_pair": F64_PER_PAIR,
                "implied_f64_lane_instructions_per_s": float(f"{pairs * F64_PER_PAIR / ms * 1e3:.4g}")}

    measure("nearest (search + combine)", lambda: core.gauge_nearest(points, gauges), a, rate)
    issued = core.valu_probe()  # (v_fma_f64 lane-instructions of one launch)
    measure("float64 VALU issue ceiling (mlx_valu_probe)", core.valu_probe, a,
            lambda ms: {"lane_instructions_per_s": float(f"{issued / ms * 1e3:.4g}")})
    index, angle = core.gauge_nearest(points, gauges)

    free, _total = torch.cuda.mem_get_info()
    nt = int(min(a.nt, max(1, (free * 0.8) // (n * 4))))
    note = "" if nt == a.nt else f" (shortened from {a.nt}: free device memory)"
    y = torch.empty((nt, n), dtype=torch.float32, device="cuda").normal_()
    out = torch.empty((ng, nt), dtype=torch.float32, device="cuda")
    measure(f"gather ({nt}, {a.ny}, {a.nx}) float32 record{note}",
            lambda: core.gauge_gather(y, index, out=out), a,
            lambda ms: {"elements": ng * nt, "record_GB": round(nt * n * 4 / 1e9, 2),
                        "whole_record_download_at_63GBs_ms": round(nt * n * 4 / 63e9 * 1e3, 1)})
    del y, out
    if a.skip_host:
        return 0

    hg = max(1, min(a.host_gauges, ng))
    t0 = time.perf_counter()
    want_index, _angle, _gap = gn.nearest(lat, lon, glat[:hg], glon[:hg], mask)
    dt = time.perf_counter() - t0
    same = bool(np.array_equal(want_index, index[:hg].cpu().numpy()))
    print(json.dumps({"case": f"host: numpy brute force, {hg} of {ng} gauges over the full grid",
                      "s": round(dt, 3), "EXTRAPOLATED_to_all_gauges_s": round(dt / hg * ng, 1),
                      "indices_equal_the_device": same}), flush=True)
    try:
        from sklearn.neighbors import BallTree
    except Exception:
        print(json.dumps({"case": "host: scikit-learn BallTree", "note": "scikit-learn is not importable here"}))
        return 0
    ok = gn.valid_points(lat, lon, mask)
    rad = np.deg2rad(np.stack([lat.reshape(-1)[ok], lon.reshape(-1)[ok]], axis=1))
    t0 = time.perf_counter()
    ball = BallTree(rad, metric="haversine")
    t1 = time.perf_counter()
    _d, nearest = ball.query(np.deg2rad(np.stack([glat, glon], axis=1)), k=1)
    t2 = time.perf_counter()
    flat = np.nonzero(ok)[0][nearest[:, 0]]
    print(json.dumps({"case": "host: scikit-learn BallTree(haversine), all gauges",
                      "build_s": round(t1 - t0, 3), "query_s": round(t2 - t1, 3),
                      "indices_equal_the_device": int(np.sum(flat == index.cpu().numpy())),
                      "of": ng}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
