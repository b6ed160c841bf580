"""Time the Gram kernel (csrc/momlevel_eof.hip) and what stands around it on a resident
(1200, 1080, 1440) record -- a century of monthly 0.25-degree fields -- for float64 and float32, in
one process on the same tensors:

    python scripts/bench_eof.py [--nt 1200 --ny 1080 --nx 1440] [--rounds 7] [--log profiles/eof_kernels.log]

Every row is the median of ``--rounds`` single launches (device events around one call each) with
the scatter (min .. max); the rows are printed and written to ``--log``:

  (a) ``core.time_gram``, symmetric form, with the per-cell time mean as center and sqrt(area) as
      scale: TFLOP/s counts ``nt (nt + 1) n`` flop, TB/s the record's bytes once;
  (b) ``core.stream_probe_mix(record, write=False)``: the record's bytes read once;
  (c) ``core.gram_issue_probe``: independent v_mfma_f64_16x16x4_f64 on registers, at one wave and at
      four waves per SIMD -- the ceiling of (a);
  (d) the torch route: the anomaly pass into a second buffer of the record's size (float64), then
      ``torch.matmul(B, B.T)``, each timed;
  (e) ``numpy.linalg.eigh`` of the nt x nt matrix on the host;
  (f) ``core.time_project`` with 4 columns;
  (g) ``eof.calc_eofs(neofs=4)`` end to end on the device record.

The condition the log reports is (a) <= (d) total, by medians.  ``--only-gram`` prints (a) alone:
for a library built with another LDS image (MOMLEVEL_AMD_LIB, -DMLX_GRAM_LDS_PAD=0).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s, MI355X
LOG = None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if LOG is not None:
        LOG.write(line + "\n")
        LOG.flush()


def once(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(name, fn, rounds, flop=None, nbytes=None, extra=None):
    import torch

    fn()
    torch.cuda.synchronize()
    ms = [once(fn) for _ in range(rounds)]
    med = float(np.median(ms))
    row = {"case": name, "launches": rounds, "ms": round(med, 4), "ms_min": round(min(ms), 4),
           "ms_max": round(max(ms), 4)}
    if flop is not None:
        row["TFLOP/s"] = round(flop / med / 1e9, 2)
    if nbytes is not None:
        row["TB/s"] = round(nbytes / med / 1e9, 3)
    row.update(extra or {})
    emit(row)
    return med


def main():
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--nt", type=int, default=1200)
    ap.add_argument("--ny", type=int, default=1080)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "eof_kernels.log"))
    ap.add_argument("--only-gram", action="store_true")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    n = a.ny * a.nx

    import torch

    from momlevel_amd import _lib, core, eof
    from momlevel_amd.csrc.build import eof_source_sha, source_sha

    core.require_device()
    _lib.load_eof()
    LOG = open(a.log, "a" if a.only_gram else "w")
    cells = core.gram_cells(n)
    emit({"eof_source_sha": eof_source_sha(), "timed_source_sha": source_sha(),
          "library": os.path.relpath(_lib.LIB_PATH, ROOT), "record": [a.nt, a.ny, a.nx],
          "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "tile": core.gram_tile(),
          "cells_per_range": cells, "ranges": -(-n // cells),
          "workspace_MB": round(_lib.load_eof().mlx_gram_matrix_workspace_bytes(a.nt, 0, n) / 1e6, 1)})

    gen = torch.Generator(device="cuda").manual_seed(1872)
    rec64 = torch.empty((a.nt, n), dtype=torch.float64, device="cuda")
    land = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) < 0.3
    for t in range(a.nt):  # (step by step: no second copy of the record while it is drawn)
        row = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) - 0.5
        row[land] = float("nan")
        rec64[t] = row
    area = torch.rand((a.ny, a.nx), dtype=torch.float64, device="cuda", generator=gen) * 5.0e8 + 4.0e8
    scale = core._f64(eof.area_scale(area, (a.ny, a.nx)), rec64.device)
    flop = a.nt * (a.nt + 1) * n

    for label, dt in (("float64", torch.float64), ("float32", torch.float32)):
        rec = rec64 if dt == torch.float64 else rec64.to(dt)
        nbytes = rec.numel() * rec.element_size()
        center = eof.time_mean(rec)
        gram = measure(f"(a) time_gram, symmetric, {label}",
                       lambda: core.time_gram(rec, None, center, None, scale), a.rounds, flop, nbytes)
        if a.only_gram:
            continue
        measure(f"(b) stream probe, {label} read",
                lambda: core.stream_probe_mix(rec.view(-1), write=False), a.rounds, None, nbytes)
        if dt == torch.float64:
            issue = {}
            for blocks, what in ((256, "one wave per SIMD"), (1024, "four waves per SIMD")):
                iters = 1 << 15
                pflop = blocks * 4 * iters * 8 * 2048
                med = measure(f"(c) issue probe, v_mfma_f64_16x16x4_f64, {what}",
                              lambda: core.gram_issue_probe(iters, blocks), a.rounds, pflop)
                issue[what] = pflop / med / 1e9
            peak = max(issue.values())
        # (d) the torch route: a second buffer of the record's size, then a library GEMM
        torch_total = None
        try:
            buf = torch.empty((a.nt, n), dtype=torch.float64, device="cuda")
            m = torch.nan_to_num(center, nan=0.0)
            s = torch.where(torch.isnan(center), torch.zeros_like(scale), scale)  # (land: weight 0)

            def anomaly():
                torch.sub(rec, m, out=buf)
                buf.mul_(s)
                buf.nan_to_num_(nan=0.0)  # (0 * NaN on land)

            t_anom = measure(f"(d1) torch anomaly pass into a float64 buffer, {label}", anomaly,
                             a.rounds, None, nbytes + 5 * buf.numel() * 8)
            t_mm = measure(f"(d2) torch.matmul(B, B.T) float64 (record was {label})",
                           lambda: torch.matmul(buf, buf.T), a.rounds, 2 * a.nt * a.nt * n,
                           buf.numel() * 8)
            torch_total = t_anom + t_mm
            G = core.time_gram(rec, None, center, None, scale)
            ref = torch.matmul(buf, buf.T)
            emit({"case": f"(d) agreement of the two routes, {label}",
                  "max|G - torch| / max|G|": float((G - ref).abs().max() / ref.abs().max())})
            del buf, ref, G
        except Exception as exc:  # (a torch build without a float64 GEMM: say so, go on)
            emit({"case": f"(d) torch route, {label}", "error": repr(exc)[:200]})
        torch.cuda.empty_cache()
        row = {"case": f"condition (a) <= (d1) + (d2), {label}", "gram_ms": round(gram, 3),
               "of_issue_probe": round(flop / gram / 1e9 / peak, 3)}
        if torch_total is not None:
            row.update({"torch_ms": round(torch_total, 3), "gram / torch": round(gram / torch_total, 3),
                        "holds": bool(gram <= torch_total)})
        emit(row)
        if dt == torch.float64:
            cov = core.time_gram(rec, None, center, None, scale).cpu().numpy() / (a.nt - 1)
            secs = []
            for _ in range(5):
                t0 = time.perf_counter()
                np.linalg.eigh(cov)
                secs.append(time.perf_counter() - t0)
            emit({"case": f"(e) numpy.linalg.eigh, {a.nt} x {a.nt}, host", "calls": 5,
                  "s": round(float(np.median(secs)), 4), "s_min": round(min(secs), 4),
                  "s_max": round(max(secs), 4), "threads": os.cpu_count()})
        P = np.random.default_rng(3).normal(size=(a.nt, 4))
        measure(f"(f) time_project, 4 modes, {label}", lambda: core.time_project(rec, P), a.rounds,
                None, nbytes)
        secs = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = eof.calc_eofs(rec.view(a.nt, a.ny, a.nx), area, neofs=4)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        emit({"case": f"(g) calc_eofs(neofs=4) end to end, device record, {label}", "calls": 3,
              "s": round(float(np.median(secs)), 4), "s_min": round(min(secs), 4),
              "s_max": round(max(secs), 4),
              "variance_fraction": [round(float(v), 6) for v in out["variance_fraction"].values]})
        del rec, center, out
        torch.cuda.empty_cache()
    LOG.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
