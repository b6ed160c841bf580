"""Time the grid-to-grid remap (csrc/momlevel_regrid.hip) on one resident 0.25-degree record:

    python scripts/bench_regrid.py [--log profiles/regrid_kernels.log] [--window-ms 300] [--rounds 5]

(the output, one JSON object a line, is what profiles/regrid_kernels.log holds).

One (32, 1080, 1440) record with the land mask of ``synthetic.make_grid``, float64 and then float32,
each dtype in a process of its own that is started under a time limit; nothing more is started
after a step that failed.  Three plans, made once per process:

  (a) ``regrid.coarsen_weights`` 4 x 4 on the grid's own areas (land carries no entry);
  (b) ``regrid.conservative_weights`` from the grid's nominal coordinates (1080 x 1440 cells over
      the sphere) to 1 degree;
  (c) ``regrid.nearest_weights`` to the centres of the 1-degree grid, the time to build the plan
      reported on its own: it is a search, not the gather.

For each plan, on the same tensors in the same process, timed with device events around enough
calls to fill ``--window-ms``, the kernel and the torch route in alternating rounds, median over
the rounds with the spread:

  * ``core.regrid_apply``;
  * the torch route: two ``torch.sparse.mm`` of the table as a CSR tensor, with ``nan_to_num(v)``
    and with the validity mask, and the division -- with the transposes it needs from and to the
    (nrec, nsrc) layout, which are also timed on their own.  Where this torch build refuses the
    sparse product the ``index_select`` + ``index_add_`` form runs instead; the log says which ran;
  * a check that both routes agree: only the order of summation differs, so per destination num
    and den are each within len * 2^-52 * sum |S v| (resp. sum S) of each other, and the quotients
    within (2 len + 2) * 2^-52 * sum |S v| / den.

The one condition is ``regrid_over_torch < 1`` at every plan and dtype, with no margin beyond "not
slower"; a condition that fails is said so in the summary line (``conditions_hold`` false), not
tuned away.  Beside it, not gated: the fraction of the stream probe reached per byte the kernel
must move (every source cell the table names once per record in, the result once out: a gather
of single cells fetches whole cache lines, so the nearest-point plan stays far below the probe by
this count), and the table's bytes against the record's.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (32, 1080, 1440)
STEP_LIMIT_S = 420


def timed(fn, calls):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def calls_for(fn, a):
    import torch

    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    return max(1, int(np.ceil(a.window_ms / max(timed(fn, 1), 1e-3))))


def report(name, ms, calls, nbytes, emit, extra=None):
    med = float(np.median(ms))
    emit({"case": name, "calls_per_window": calls, "ms": round(med, 4), "ms_min": round(min(ms), 4),
          "ms_max": round(max(ms), 4), "bytes_in_and_out": nbytes,
          "TB/s_of_in_and_out": round(nbytes / med / 1e9, 3), **(extra or {})})
    return med


def measure(name, fn, a, nbytes, emit, extra=None):
    calls = calls_for(fn, a)
    return report(name, [timed(fn, calls) for _ in range(a.rounds)], calls, nbytes, emit, extra)


def measure_alternating(names, fns, a, nbytes, emit, extras):
    """the rounds of the two routes interleaved: a drift of the clocks meets both alike"""
    calls = [calls_for(fn, a) for fn in fns]
    ms = [[], []]
    for _ in range(a.rounds):
        for i, fn in enumerate(fns):
            ms[i].append(timed(fn, calls[i]))
    return [report(names[i], ms[i], calls[i], nbytes, emit, extras[i]) for i in range(2)]


class TorchRoute:
    """out = (A @ nan_to_num(v)^T) / (A @ valid^T), NaN where no source is valid: float64"""

    def __init__(self, plan, device):
        import torch

        self.ndst, self.nsrc = plan.ndst, plan.nsrc
        self.indptr = torch.from_numpy(plan.indptr).to(device)
        self.col = torch.from_numpy(plan.col.astype(np.int64)).to(device)
        self.S = torch.from_numpy(plan.S).to(device)
        self.row = torch.repeat_interleave(torch.arange(plan.ndst, device=device),
                                           self.indptr[1:] - self.indptr[:-1])
        self.form = "torch.sparse.mm on a CSR tensor"
        try:
            self.A = torch.sparse_csr_tensor(self.indptr, self.col, self.S, size=(plan.ndst, plan.nsrc))
            probe = torch.zeros((plan.nsrc, 2), dtype=torch.float64, device=device)
            torch.sparse.mm(self.A, probe)
            torch.cuda.synchronize()
        except (RuntimeError, NotImplementedError) as exc:
            self.A = None
            self.form = f"index_select + index_add_ (the sparse product was refused: {str(exc)[:120]})"

    def matmul(self, xT):
        import torch

        if self.A is not None:
            return torch.sparse.mm(self.A, xT)
        out = torch.zeros((self.ndst, xT.shape[1]), dtype=torch.float64, device=xT.device)
        return out.index_add_(0, self.row, self.S[:, None] * xT.index_select(0, self.col))

    def parts(self, v):
        import torch

        v64 = v.double()
        valid = ~torch.isnan(v64)
        num = self.matmul(torch.nan_to_num(v64, nan=0.0).t().contiguous())
        den = self.matmul(valid.double().t().contiguous())
        return num, den

    def __call__(self, v):
        import torch

        num, den = self.parts(v)
        nan = torch.full((), float("nan"), dtype=torch.float64, device=v.device)
        return torch.where(den > 0, num / den, nan).t().contiguous()

    def transposes(self, v, out):
        """the layout changes alone: two (nsrc, nrec) operands in, one (nrec, ndst) result out"""
        v64 = v.double()
        return v64.t().contiguous(), v64.t().contiguous(), out.t().contiguous()


def agreement(route, plan, v, got):
    """(nan placement equal, the largest error in units of the bound of the module docstring)"""
    import torch

    num, den = route.parts(v)
    want = torch.where(den > 0, num / den, torch.full_like(num, float("nan"))).t()
    absS = torch.from_numpy(np.abs(plan.S)).to(v.device)
    keep, route.S = route.S, absS
    A = route.A
    route.A = None  # (|S| through the index form: the CSR tensor holds S)
    scale = route.matmul(torch.nan_to_num(v.double(), nan=0.0).abs().t().contiguous())
    route.S, route.A = keep, A
    length = (route.indptr[1:] - route.indptr[:-1]).double()[:, None]
    bound = ((2.0 * length + 2.0) * 2.0 ** -52 * scale / den).t()
    both = ~torch.isnan(got) & ~torch.isnan(want)
    same_nan = bool(torch.equal(torch.isnan(got), torch.isnan(want)))
    if not bool(both.any()):
        return same_nan, 0.0
    err = (got.double() - want).abs()[both] / torch.clamp(bound[both], min=2.0 ** -1022)
    return same_nan, float(err.max())


def step(a, label):
    """every measurement of one dtype, in this process, on the same tensors"""
    import torch

    from momlevel_amd import _lib, core, regrid, synthetic
    from momlevel_amd.csrc.build import regrid_source_sha, source_sha

    core.require_device()  # no GPU: an error, never a CPU timing
    _lib.load_regrid()

    def emit(row):
        print(json.dumps(row), flush=True)

    dt = torch.float64 if label == "float64" else torch.float32
    nrec, ny, nx = a.nrec, a.ny, a.nx
    emit({"step": label, "regrid_source_sha": regrid_source_sha(), "timed_source_sha": source_sha(),
          "device": torch.cuda.get_device_name(0), "record": [nrec, ny, nx],
          "window_ms": a.window_ms, "rounds": a.rounds,
          "launch_shape": {"threads_per_block": 256, "slice": core.regrid_slice(),
                           "record_window": core.regrid_record_window(),
                           "grid": "slice groups fast, record windows slow"},
          "launch_shapes_tried": "this one only"})
    g = synthetic.make_grid(ny, nx, 2)
    wet_host = ~np.isnan(g["deptho"])
    wet = torch.from_numpy(wet_host).cuda()
    gen = torch.Generator(device="cuda").manual_seed(7)
    v = torch.randn((nrec, ny, nx), dtype=torch.float64, device="cuda", generator=gen)
    v = torch.where(wet[None], v, torch.full((), float("nan"), dtype=torch.float64, device="cuda"))
    v = v.to(dt).reshape(nrec, ny * nx).contiguous()
    emit({"check": "record", "wet_fraction": round(float(wet.double().mean()), 4)})
    elem = v.element_size()
    out64 = torch.empty(v.shape, dtype=torch.float64, device="cuda")
    probe_bytes = v.numel() * (elem + 8)
    probe = measure(f"stream_probe_mix, one {label} stream read, one float64 stream written",
                    lambda: core.stream_probe_mix(v.view(-1), out=out64.view(-1)), a, probe_bytes, emit)
    probe_tbs = probe_bytes / probe / 1e9
    del out64

    lat_b, lon_b = np.linspace(-90.0, 90.0, ny + 1), np.linspace(0.0, 360.0, nx + 1)
    lat_c, lon_c = 0.5 * (lat_b[:-1] + lat_b[1:]), 0.5 * (lon_b[:-1] + lon_b[1:])
    one_b = (np.linspace(-90.0, 90.0, 181), np.linspace(0.0, 360.0, 361))
    plans = []
    t0 = time.perf_counter()
    plans.append(("coarsen 4x4", regrid.coarsen_weights(g["areacello"], 4, 4)))
    t1 = time.perf_counter()
    plans.append(("conservative 0.25 -> 1 degree",
                  regrid.conservative_weights(lat_b, lon_b, *one_b, src_mask=wet_host)))
    t2 = time.perf_counter()
    plans.append(("nearest -> 1 degree",
                  regrid.nearest_weights(lat_c, lon_c, 0.5 * (one_b[0][:-1] + one_b[0][1:]),
                                         0.5 * (one_b[1][:-1] + one_b[1][1:]),
                                         mask=wet_host.astype(np.float64))))
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    emit({"plan_building_s": {"coarsen 4x4 (host)": round(t1 - t0, 3),
                              "conservative (host)": round(t2 - t1, 3),
                              "nearest (the search on the device, the table on the host)": round(t3 - t2, 3)}})

    summary, hold = {}, True
    for name, plan in plans:
        tensors = plan.on(v.device)
        length = np.diff(plan.indptr)
        table_bytes = sum(int(t.numel() * t.element_size()) for t in tensors)
        # what the kernel must move: every source cell some row names once per record (land carries
        # no entry; the nearest-point table names one source per destination), the result once
        touched = int(np.unique(plan.col).size)
        nbytes = nrec * (touched + plan.ndst) * elem
        shape = {"ndst": plan.ndst, "entries": plan.nnz, "padded_entries": int(tensors[2].numel()),
                 "source_cells_named": touched,
                 "source_cells_named_over_plane": round(touched / plan.nsrc, 4),
                 "row_length_median_max": [int(np.median(length)), int(length.max())],
                 "table_bytes": table_bytes,
                 "table_over_record_bytes": round(table_bytes / (v.numel() * elem), 4)}
        route = TorchRoute(plan, v.device)

        def kernel():
            return core.regrid_apply(v, tensors, plan.nsrc, plan.ndst)

        got = core.regrid_apply(v, tensors, plan.nsrc, plan.ndst, out_dtype=torch.float64)
        same_nan, worst = agreement(route, plan, v, got)
        agree = bool(same_nan and worst <= 1.0)
        emit({"check": f"torch route against the kernel, {name}", "torch_route": route.form,
              "nan_placement_equal": same_nan, "max_error_over_bound": worst,
              "agree_within_the_bound": agree})
        del got
        ms, tms = measure_alternating(
            [f"regrid_apply {name}, {label}", f"torch route {name}, {label}"],
            [kernel, lambda: route(v)], a, nbytes, emit, [shape, {"torch_route": route.form}])
        out_t = torch.empty((plan.ndst, nrec), dtype=torch.float64, device=v.device)
        trans = measure(f"the torch route's transposes alone, {name}, {label}",
                        lambda: route.transposes(v, out_t), a, nbytes, emit)
        del out_t
        ratio = ms / tms
        summary[name] = {"regrid_over_torch": round(ratio, 4),
                         "regrid_over_torch_without_its_transposes": round(ms / max(tms - trans, 1e-6), 4),
                         "fraction_of_stream_probe": round(nbytes / ms / 1e9 / probe_tbs, 4),
                         "table_over_record_bytes": shape["table_over_record_bytes"]}
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
