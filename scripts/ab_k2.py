#!/usr/bin/env python3
"""A/B timing of the K2 kernels of whichever library MOMLEVEL_AMD_LIB points at (tuning harness).

    MOMLEVEL_AMD_LIB=scripts/variants/lib_x.so python scripts/ab_k2.py [--nt 32]

One JSON line: best-of-5 ms per case at the 0.25-degree grid, theta/S resident.  Next to every
case that stores delta_rho its float32-egress twin (``..._f32out``: MLX_FLAG_DRHO_F32, same process,
same tensors), and a ``pairs`` table: ms, B/cell, GB/s and the fraction of the 8 TB/s HBM peak of
both, and the time ratio float32 / float64 egress."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from momlevel_amd import core, synthetic  # noqa: E402


def best(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return round(min(out), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nt", type=int, default=32)
    a = ap.parse_args()
    nz, ny, nx = 75, 1080, 1440
    g = synthetic.make_grid(ny, nx, nz)
    vol0 = torch.from_numpy(g["volcello"]).cuda()
    pz = torch.from_numpy(101325.0 + g["z_l"] * 1.0e4).cuda()
    shape = (a.nt, nz, ny, nx)
    res = {"lib": os.environ.get("MOMLEVEL_AMD_LIB", "default"), "nt": a.nt}
    zi, dep = torch.from_numpy(g["z_i"]).cuda(), torch.from_numpy(g["deptho"]).cuda()
    for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        T = core.synth_field(shape, dt, seed=synthetic.SEED, field_id=1, lo=-2.0, scale=34.0, mask3d=vol0)
        S = core.synth_field(shape, dt, seed=synthetic.SEED, field_id=2, lo=30.0, scale=10.0, mask3d=vol0)
        rho0m = core.fold_mask(core.eos_map(T[0], S[0], pz), vol0)
        eta = torch.empty((a.nt, ny, nx), dtype=torch.float64, device="cuda")
        drho = torch.empty(shape, dtype=torch.float64, device="cuda")
        drho32 = torch.empty(shape, dtype=torch.float32, device="cuda")
        kw = dict(z_i=zi, deptho=dep, skip_dry=False)
        kw32 = dict(kw, delta_rho_out=drho32, delta_rho_dtype=torch.float32)
        B = T.element_size()
        pairs = res.setdefault("pairs", {})

        def pair(name, in_bytes, nout=1):
            """the float64 / float32 egress rows of one pass (bytes per cell: fields read + written)"""
            row = {}
            for key, out_b in ((name, 8), (name + "_f32out", 4)):
                ms, bpc = res[key], in_bytes + nout * out_b
                gbs = bpc * T.numel() / ms / 1e6
                row[key] = {"ms": ms, "B/cell": bpc, "GB/s": round(gbs, 1),
                            "of_8TB/s": round(gbs / 8000.0, 3)}
            row["time_ratio_f32out/f64out"] = round(res[name + "_f32out"] / res[name], 3)
            pairs[name] = row

        res[f"{tag}_eta_only"] = best(lambda: core.steric_local(
            T, S, rho0m, vol0[0], pz, -1.0 / 1035.0, want_delta_rho=False, eta_out=eta, **kw))
        res[f"{tag}_with_delta_rho"] = best(lambda: core.steric_local(
            T, S, rho0m, vol0[0], pz, -1.0 / 1035.0, eta_out=eta, delta_rho_out=drho, **kw))
        res[f"{tag}_with_delta_rho_f32out"] = best(lambda: core.steric_local(
            T, S, rho0m, vol0[0], pz, -1.0 / 1035.0, eta_out=eta, **kw32))
        pair(f"{tag}_with_delta_rho", 2 * B)
        res[f"{tag}_thermo_eta_only"] = best(lambda: core.steric_local(
            T, S[0], rho0m, vol0[0], pz, -1.0 / 1035.0, want_delta_rho=False, eta_out=eta, **kw))
        res[f"{tag}_thermo_eta_only_fingerprint"] = "%.17g" % eta.nan_to_num(0.0).sum().item()
        res[f"{tag}_halo_eta_only"] = best(lambda: core.steric_local(
            T[0], S, rho0m, vol0[0], pz, -1.0 / 1035.0, want_delta_rho=False, eta_out=eta, **kw))
        res[f"{tag}_halo_eta_only_fingerprint"] = "%.17g" % eta.nan_to_num(0.0).sum().item()
        res[f"{tag}_thermo_with_delta_rho"] = best(lambda: core.steric_local(
            T, S[0], rho0m, vol0[0], pz, -1.0 / 1035.0, eta_out=eta, delta_rho_out=drho, **kw))
        res[f"{tag}_thermo_with_delta_rho_f32out"] = best(lambda: core.steric_local(
            T, S[0], rho0m, vol0[0], pz, -1.0 / 1035.0, eta_out=eta, **kw32))
        pair(f"{tag}_thermo_with_delta_rho", B)
        res[f"{tag}_halo_with_delta_rho"] = best(lambda: core.steric_local(
            T[0], S, rho0m, vol0[0], pz, -1.0 / 1035.0, eta_out=eta, delta_rho_out=drho, **kw))
        res[f"{tag}_halo_with_delta_rho_f32out"] = best(lambda: core.steric_local(
            T[0], S, rho0m, vol0[0], pz, -1.0 / 1035.0, eta_out=eta, **kw32))
        pair(f"{tag}_halo_with_delta_rho", B)
        res[f"{tag}_eta_only_skip_dry"] = best(lambda: core.steric_local(
            T, S, rho0m, vol0[0], pz, -1.0 / 1035.0, want_delta_rho=False, eta_out=eta,
            z_i=zi, deptho=dep, skip_dry=True))
        # fingerprints of the held-field outputs (equal across libraries: tuning never changes a bit)
        for name, Tv, Sv in (("thermo", T, S[0]), ("halo", T[0], S)):
            core.steric_local(Tv, Sv, rho0m, vol0[0], pz, -1.0 / 1035.0, eta_out=eta,
                              delta_rho_out=drho, **kw)
            res[f"{tag}_{name}_fingerprint"] = "%.17g/%.17g" % (
                eta.nan_to_num(0.0).sum().item(), drho.nan_to_num(0.0).abs().sum().item())
            core.steric_local(Tv, Sv, rho0m, vol0[0], pz, -1.0 / 1035.0, eta_out=eta,
                              delta_rho_out=drho, z_i=zi, deptho=dep, skip_dry=True)
            res[f"{tag}_{name}_fingerprint_skip_dry"] = "%.17g/%.17g" % (
                eta.nan_to_num(0.0).sum().item(), drho.nan_to_num(0.0).abs().sum().item())
        del drho, drho32, kw32
        e3 = torch.empty((3, a.nt, ny, nx), dtype=torch.float64, device="cuda")
        res[f"{tag}_one_pass_eta_only"] = best(lambda: core.steric_local_decomp(
            T, S, T[0], S[0], rho0m, vol0[0], pz, -1.0 / 1035.0, want_delta_rho=False, eta_out=e3, **kw))
        # the all-variants pass with its three delta_rho fields on as many steps as are whole time
        # blocks of BOTH shapes it runs in (8 steps per thread; 6 for the float32-egress kernel of a
        # float64 polynomial): a shorter launch would flatter the shape with more blocks per record
        n3 = (a.nt // 24) * 24 or max(1, a.nt // 3)
        d3 = torch.empty((3, n3) + shape[1:], dtype=torch.float64, device="cuda")
        res[f"{tag}_one_pass_with_delta_rho"] = best(lambda: core.steric_local_decomp(
            T[:n3], S[:n3], T[0], S[0], rho0m, vol0[0], pz, -1.0 / 1035.0, delta_rho_out=d3,
            eta_out=e3[:, :n3], **kw))
        del d3
        d3 = torch.empty((3, n3) + shape[1:], dtype=torch.float32, device="cuda")
        res[f"{tag}_one_pass_with_delta_rho_f32out"] = best(lambda: core.steric_local_decomp(
            T[:n3], S[:n3], T[0], S[0], rho0m, vol0[0], pz, -1.0 / 1035.0, delta_rho_out=d3,
            delta_rho_dtype=torch.float32, eta_out=e3[:, :n3], **kw))
        for key in (f"{tag}_one_pass_with_delta_rho", f"{tag}_one_pass_with_delta_rho_f32out"):
            res[key] = round(res[key] * a.nt / n3, 3)  # (scaled to the record's length, as the other rows)
        res[f"{tag}_one_pass_steps_per_launch"] = n3
        pair(f"{tag}_one_pass_with_delta_rho", 2 * B, nout=3)
        del T, S, rho0m, eta, e3, d3
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
