"""Time the census kernels (csrc/momlevel_census.hip) on one resident 0.25-degree step of theta and
S -- (75, 1080, 1440) cells -- with a static volcello map, for float64 and for float32:

    python scripts/bench_census.py [--nz 75 --ny 1080 --nx 1440] [--window-ms 300] [--rounds 5]

Each case is timed with device events around enough calls to fill ``--window-ms``; the median over
the rounds is reported with the spread (min .. max).  Cases, per dtype, in one process on the same
tensors:

* 1-D, 100 sigma-like classes (a linear density of theta and S), weighted by volume;
* 2-D, 64 x 64 (theta, S) classes;
* 2-D, 100 x 100 (theta, S) classes (several bin groups: the fields are re-read once per group);
* an adversarial field on which every lane of a wave has a bin of its own at every step (64 bins).

Beside each: the read probe of the same bytes (``core.stream_probe_mix(x, write=False)`` over every
operand once) and a torch route -- ``torch.bucketize`` per field, a combined index, a mask and a
weighted ``torch.bincount``.  The log records each case's time, its ratio to the probe and its ratio
to the torch route; the one condition is that the realistic cases are not slower than the torch
route (ratio < 1.0, median against median).  The torch route adds with atomics, so the agreement is
checked inside the summation-order bound |ours - torch| <= 1e-10 * sum_bin |w|, never bit for bit.

These are call times of ``census.sums`` on device tensors: the plan, the upload of the edges and the
workspace from torch's caching allocator are inside the timed region, as a caller pays for them.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
           "ms_max": round(max(ms), 4), "operand_bytes_once": nbytes,
           "TB/s_of_operands_once": round(nbytes / med / 1e9, 3)}
    row.update(extra or {})
    print(json.dumps(row), flush=True)
    return med


def torch_route(fields, edges, w):
    """bucketize per field, a combined index, a mask, a weighted bincount (float64 sums)"""
    import torch

    idx = valid = None
    nbins = 1
    for f, e in zip(fields, edges):
        n = e.numel() - 1
        i = torch.bucketize(f, e.to(f.dtype) if f.dtype != e.dtype else e, right=True) - 1
        i = torch.where(f == e[-1], n - 1, i)
        ok = (i >= 0) & (i < n)
        valid = ok if valid is None else valid & ok
        idx = i if idx is None else idx * n + i
        nbins *= n
    valid = valid & ~torch.isnan(w)
    idx = torch.where(valid, idx, nbins)  # one more bin for what is left out
    ww = torch.where(valid, w, torch.zeros((), dtype=w.dtype, device=w.device)).to(torch.float64)
    return torch.bincount(idx, weights=ww, minlength=nbins + 1)[:nbins]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nz", type=int, default=75)
    ap.add_argument("--ny", type=int, default=1080)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    n = a.nz * a.ny * a.nx

    import torch

    from momlevel_amd import _lib, census, core
    from momlevel_amd.csrc.build import census_source_sha, source_sha

    core.require_device()
    _lib.load_census()
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(1872)
    # a smooth ocean: warm and salty above and in the tropics, eddies on top, land as NaN columns
    k = torch.arange(a.nz, device=dev, dtype=torch.float64).view(-1, 1, 1)
    j = torch.arange(a.ny, device=dev, dtype=torch.float64).view(1, -1, 1)
    i = torch.arange(a.nx, device=dev, dtype=torch.float64).view(1, 1, -1)
    lat = (j / a.ny - 0.5) * np.pi
    theta = 1.0 + 26.0 * torch.exp(-k / 12.0) * torch.cos(lat) ** 2 + 0.8 * torch.sin(i / a.nx * 12 * np.pi) \
        * torch.cos(j / a.ny * 9 * np.pi)
    theta += 0.05 * torch.randn((a.nz, a.ny, a.nx), dtype=torch.float64, device=dev, generator=gen)
    salt = 34.6 + 1.6 * torch.exp(-k / 20.0) * torch.cos(2.0 * lat) + 0.2 * torch.cos(i / a.nx * 8 * np.pi) \
        + 0.0 * theta
    salt += 0.01 * torch.randn((a.nz, a.ny, a.nx), dtype=torch.float64, device=dev, generator=gen)
    land = (torch.rand((1, a.ny, a.nx), dtype=torch.float64, device=dev, generator=gen) < 0.00017)
    land = torch.nn.functional.max_pool2d(land.to(torch.float32), 41, 1, 20) > 0  # islands of 41 cells: about a quarter of the plane
    vol = (1.0e9 * (1.0 + k / 10.0) * torch.cos(lat) + 0.0 * i)
    vol = torch.where(land, torch.full_like(vol, float("nan")), vol)
    theta = torch.where(land, torch.full_like(theta, float("nan")), theta)
    salt = torch.where(land, torch.full_like(salt, float("nan")), salt)
    sigma = 27.0 - 0.2 * (theta - 4.0) + 0.78 * (salt - 35.0)
    lane = ((torch.arange(n, device=dev) // 4) % 64).to(torch.float64) + 0.5

    # (edges that float32 holds exactly: the torch route buckets a float32 field by float32 edges)
    cases = [
        ("1-D, 100 sigma-like classes", ("sigma",), [census.bin_edges(21.0, 28.8125, 100)]),
        ("2-D, 64 x 64 (theta, S) classes", ("theta", "salt"),
         [census.bin_edges(-2.0, 30.0, 64), census.bin_edges(32.0, 37.5, 64)]),
        ("2-D, 100 x 100 (theta, S) classes", ("theta", "salt"),
         [census.bin_edges(-1.0, 30.25, 100), census.bin_edges(32.0, 38.25, 100)]),
        ("adversarial: every lane of a wave in its own bin, 64 classes", ("lane",),
         [np.arange(65.0)]),
    ]
    for e in (e for c in cases for e in c[2]):
        assert np.array_equal(e.astype(np.float32).astype(np.float64), e)
    for label, dt in (("float64", torch.float64), ("float32", torch.float32)):
        ops = {"theta": theta.to(dt).reshape(1, n), "salt": salt.to(dt).reshape(1, n),
               "sigma": sigma.to(dt).reshape(1, n), "lane": lane.to(dt).reshape(1, n)}
        w = vol.to(dt).reshape(n).contiguous()
        item = w.element_size()
        print(json.dumps({"step": label, "census_source_sha": census_source_sha(),
                          "timed_source_sha": source_sha(), "device": torch.cuda.get_device_name(0),
                          "record": [1, a.nz, a.ny, a.nx], "cells": n, "window_ms": a.window_ms,
                          "rounds": a.rounds, "wet_fraction": round(float((~torch.isnan(w)).double().mean()), 4),
                          "launch_shape": {"threads_per_block": 256, "tile": core.census_tile(),
                                           "blocks_per_record": core.census_blocks(n),
                                           "max_bins_with_weights": core.census_max_bins(2, True, False)},
                          "launch_shapes_tried": "this one only"}), flush=True)
        summary = {}
        for name, which, edges in cases:
            fields = [ops[x] for x in which]
            e_dev = [torch.from_numpy(e).to(dev) for e in edges]
            shape = tuple(e.size - 1 for e in edges)
            groups = census.plan_bin_groups(shape, core.census_max_bins(len(shape), True, False))
            nbytes = (len(fields) + 1) * n * item

            def probe():
                for x in fields:
                    core.stream_probe_mix(x.view(-1), write=False)
                core.stream_probe_mix(w, write=False)

            def ours():
                return census.sums(*fields, bins=edges, weights=w, tcoord="dim_0")

            def theirs():
                return torch_route([x.view(-1) for x in fields], e_dev, w)

            count, wsum, _ = ours()
            ref = theirs().reshape(wsum.shape)
            scale = torch_route([x.view(-1) for x in fields], e_dev, w.abs()).reshape(wsum.shape)
            ratio = float(((wsum - ref).abs() / (1e-10 * scale).clamp_min(1e-300)).max())
            distinct = int((count > 0).sum())
            print(json.dumps({"check": f"torch route against the census, {name}",
                              "cells_in_range": int(count.sum()), "classes_occupied": distinct,
                              "max_error_over_bound": ratio, "agree_within_the_bound": ratio <= 1.0}),
                  flush=True)
            p = measure(f"read probe of the same bytes, {name}, {label}", probe, a, nbytes)
            c = measure(f"census {name}, {label}", ours, a, nbytes,
                        {"bin_groups": len(groups), "bins": int(np.prod(shape))})
            t = measure(f"torch route {name}, {label}", theirs, a, nbytes)
            summary[name] = {"census_ms": round(c, 4), "census_over_probe": round(c / p, 3),
                             "census_over_torch": round(c / t, 4), "bin_groups": len(groups)}
            del count, wsum, ref, scale
        real = [v["census_over_torch"] for k2, v in summary.items() if not k2.startswith("adversarial")]
        summary["conditions_hold"] = bool(all(r < 1.0 for r in real))
        if not summary["conditions_hold"]:
            summary["missed"] = [k2 for k2, v in summary.items() if isinstance(v, dict)
                                 and not k2.startswith("adversarial") and v["census_over_torch"] >= 1.0]
        print(json.dumps({"summary": label, **summary}), flush=True)
        del ops, w
    return 0


if __name__ == "__main__":
    sys.exit(main())
