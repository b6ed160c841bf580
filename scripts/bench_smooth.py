"""Time the horizontal filter (csrc/momlevel_smooth.hip) on one resident 0.25-degree record:

    python scripts/bench_smooth.py [--log profiles/smooth_kernels.log] [--window-ms 300] [--rounds 5]

(the output, one JSON object a line, is what profiles/smooth_kernels.log holds).

One (32, 1080, 1440) record with the land mask of ``synthetic.make_grid``, float64 and then float32,
each dtype in a process of its own that is started under a time limit; nothing more is started
after a step that failed.  In that process, on the same tensors, timed with device events around
enough calls to fill ``--window-ms``, median over the rounds with the spread:

  * ``core.stream_probe_mix(v, out=...)``: one stream read, one float64 stream written;
  * ``core.plane_smooth`` at 3 x 3, 9 x 9 and 33 x 33 Gaussian windows with periodic x, and with a
    9-wide per-row table of x weights;
  * a torch route that evaluates the same formulas on the device, as Wx + Wy rolled multiply-adds
    over the (y-padded) record -- after a check that its results agree with the kernel's to a few
    ulp.

What follows from the byte counts is a condition, not a number: the torch route moves at least
Wx + Wy passes over the record and the kernel one plus its halos, so ``smooth_over_torch`` must be
below 1 at every timed window.  The fraction of the stream probe reached (per byte the kernel must
move: the record once in, the result once out), the LDS per block, the waves per SIMD and the halo
overhead of every window are written down beside it; a condition that fails is said so in the
summary line (``conditions_hold`` false), not tuned away.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (32, 1080, 1440)
STEP_LIMIT_S = 420
# static LDS of k_smooth_tiled per window class (largest window it takes -> bytes per block), as
# hipcc -Rpass-analysis=kernel-resource-usage reports them for the sources of smooth_source_sha;
# 160 KiB per CU and 256-thread blocks give the blocks per CU and the waves per SIMD
LDS_PER_BLOCK = {5: 50760, 9: 60168, 33: 127368}
LDS_PER_CU = 160 * 1024


def timed(fn, calls):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def measure(name, fn, a, nbytes, emit, extra=None):
    import torch

    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    calls = max(1, int(np.ceil(a.window_ms / max(timed(fn, 1), 1e-3))))
    ms = [timed(fn, calls) for _ in range(a.rounds)]
    med = float(np.median(ms))
    emit({"case": name, "calls_per_window": calls, "ms": round(med, 4), "ms_min": round(min(ms), 4),
          "ms_max": round(max(ms), 4), "bytes_in_and_out": nbytes,
          "TB/s_of_in_and_out": round(nbytes / med / 1e9, 3), **(extra or {})})
    return med


def torch_route(v, area, wx, wy, lead_x, lead_y):
    """the contract's formulas in torch, periodic x, min_count 1, no fill, no residual: float64"""
    import torch

    v64, a64 = v.double(), area.double()
    valid = ~torch.isnan(v64) & (~torch.isnan(a64) & (a64 > 0))[None]
    zero = torch.zeros((), dtype=torch.float64, device=v.device)
    m = torch.where(valid, a64[None] * v64, zero)
    aa = torch.where(valid, a64[None], zero)
    rn, rd = torch.zeros_like(m), torch.zeros_like(m)
    rc = torch.zeros(m.shape, dtype=torch.int32, device=v.device)
    vi = valid.to(torch.int32)
    table = wx.dim() == 2
    for k in range(wx.shape[-1]):
        x = wx[:, k].reshape(1, -1, 1) if table else wx[k]
        rn += x * torch.roll(m, lead_x - k, dims=-1)
        rd += x * torch.roll(aa, lead_x - k, dims=-1)
        rc += torch.roll(vi, lead_x - k, dims=-1)
    ny, Wy = m.shape[1], wy.shape[0]
    pad = (0, 0, lead_y, Wy - 1 - lead_y)  # closed north and south: rows of zeros
    rn, rd, rc = (torch.nn.functional.pad(t, pad) for t in (rn, rd, rc))
    num, den = torch.zeros_like(m), torch.zeros_like(m)
    cnt = torch.zeros_like(vi)
    for l in range(Wy):  # noqa: E741
        num += wy[l] * rn[:, l:l + ny]
        den += wy[l] * rd[:, l:l + ny]
        cnt += rc[:, l:l + ny]
    nan = torch.full((), float("nan"), dtype=torch.float64, device=v.device)
    return torch.where(valid & (cnt >= 1), num / den, nan)


def ulps_apart(got, want):
    """the largest distance in units of the last place of ``want`` over the cells both hold"""
    import torch

    both = ~torch.isnan(got) & ~torch.isnan(want)
    same_nan = bool(torch.equal(torch.isnan(got), torch.isnan(want)))
    if not bool(both.any()):
        return same_nan, 0.0
    g, w = got[both].double(), want[both].double()
    ulp = torch.clamp(w.abs(), min=2.0 ** -1022) * 2.0 ** -52
    return same_nan, float(((g - w).abs() / ulp).max())


def step(a, label):
    """every measurement of one dtype, in this process, on the same tensors"""
    import torch

    from momlevel_amd import _lib, core, spatial, synthetic
    from momlevel_amd.csrc.build import smooth_source_sha, source_sha

    core.require_device()  # no GPU: an error, never a CPU timing
    _lib.load_smooth()

    def emit(row):
        print(json.dumps(row), flush=True)

    dt = torch.float64 if label == "float64" else torch.float32
    nrec, ny, nx = a.nrec, a.ny, a.nx
    th, tw = core.smooth_tile(dt)
    emit({"step": label, "smooth_source_sha": smooth_source_sha(), "timed_source_sha": source_sha(),
          "device": torch.cuda.get_device_name(0), "record": [nrec, ny, nx],
          "window_ms": a.window_ms, "rounds": a.rounds,
          "launch_shape": {"threads_per_block": 256, "tile": [th, tw],
                           "max_window": core.smooth_max_window(),
                           "record_window": core.smooth_record_window()},
          "launch_shapes_tried": "this one only"})
    g = synthetic.make_grid(ny, nx, 2)
    area = torch.from_numpy(np.ascontiguousarray(g["areacello"])).cuda().to(dt)
    wet = ~torch.isnan(torch.from_numpy(g["deptho"]).cuda())
    gen = torch.Generator(device="cuda").manual_seed(7)
    v = torch.randn((nrec, ny, nx), dtype=torch.float64, device="cuda", generator=gen)
    v = torch.where(wet[None], v, torch.full((), float("nan"), dtype=torch.float64, device="cuda"))
    v = v.to(dt).contiguous()
    emit({"check": "record", "wet_fraction": round(float(wet.double().mean()), 4),
          "area_nan_fraction": round(float(torch.isnan(area).double().mean()), 4)})
    elem = v.element_size()
    nbytes = 2 * v.numel() * elem  # the record once in, the result once out
    out64 = torch.empty(v.shape, dtype=torch.float64, device="cuda")
    probe_bytes = v.numel() * (elem + 8)
    probe = measure(f"stream_probe_mix, one {label} stream read, one float64 stream written",
                    lambda: core.stream_probe_mix(v.view(-1), out=out64.view(-1)), a, probe_bytes, emit)
    probe_tbs = probe_bytes / probe / 1e9

    # a length of 0.4 equatorial cells on a grid that converges to 73 degrees: 3 to 9 cells wide
    table = spatial.length_scale_weights(0.4, np.cos(np.deg2rad(np.linspace(-73.0, 73.0, ny))))
    windows = [("3x3", spatial.gaussian_weights(1.0 / 3.0)),
               ("9x9", spatial.gaussian_weights(4.0 / 3.0)), ("33x33", spatial.gaussian_weights(16.0 / 3.0)),
               ("9x9 per-row table", spatial.gaussian_weights(4.0 / 3.0))]
    summary, hold = {}, True
    for name, w in windows:
        W = int(w.size)
        wx_host = table if "table" in name else w
        assert wx_host.shape[-1] == W, (name, wx_host.shape)
        wx = torch.from_numpy(np.ascontiguousarray(wx_host)).cuda()
        wy = torch.from_numpy(w).cuda()
        lead = W // 2
        cls = min(c for c in LDS_PER_BLOCK if c >= W)
        blocks = LDS_PER_CU // LDS_PER_BLOCK[cls]
        halo = (th + W - 1) * ((tw + W - 1 + 6) // 4 * 4) / (th * tw)  # (columns in whole packs)
        shape = {"window": [W, W], "lds_bytes_per_block": LDS_PER_BLOCK[cls], "blocks_per_cu": blocks,
                 "waves_per_simd": blocks, "halo_overhead_cells_staged_per_output_cell": round(halo, 3)}

        def kernel():
            return core.plane_smooth(v, area, wx, wy, lead, lead, True, 1)

        got = core.plane_smooth(v[:2], area, wx, wy, lead, lead, True, 1, out_dtype=torch.float64)
        want = torch_route(v[:2], area, wx, wy, lead, lead)
        same_nan, ulps = ulps_apart(got, want)
        agree = bool(same_nan and ulps <= 4.0)
        emit({"check": f"torch route against the kernel, {name}", "nan_placement_equal": same_nan,
              "max_ulps_apart": ulps, "agree_to_a_few_ulp": agree})
        del want, got
        ms = measure(f"plane_smooth {name}, {label}", kernel, a, nbytes, emit, shape)
        tms = measure(f"torch route {name}, {label}", lambda: torch_route(v, area, wx, wy, lead, lead),
                      a, nbytes, emit, {"passes_over_the_record_at_least": 2 * W})
        ratio = ms / tms
        summary[name] = {"smooth_over_torch": round(ratio, 4),
                         "fraction_of_stream_probe": round(nbytes / ms / 1e9 / probe_tbs, 4)}
        hold = hold and agree and ratio < 1.0
    emit({"summary": label, **summary, "conditions_hold": bool(hold)})
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["float64", "float32"], help="(internal) one dtype, in this process")
    ap.add_argument("--log", default=None, help="also write the lines to this file")
    ap.add_argument("--nrec", type=int, default=SHAPE[0])
    ap.add_argument("--ny", type=int, default=SHAPE[1])
    ap.add_argument("--nx", type=int, default=SHAPE[2])
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if a.step:
        return step(a, a.step)
    lines = []
    rc = 0
    for label in ("float64", "float32"):  # a fresh process per step, each under its own time limit
        cmd = [sys.executable, os.path.abspath(__file__), "--step", label, "--nrec", str(a.nrec),
               "--ny", str(a.ny), "--nx", str(a.nx), "--window-ms", str(a.window_ms),
               "--rounds", str(a.rounds)]
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
