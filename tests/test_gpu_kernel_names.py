"""GPU: which K1 / K2 instantiation every combination of the dispatch axes launches.

``tests/golden/kernel_names.json`` maps each case to the string ``mlx_last_kernel`` reported for it
when the fixture was recorded; the dispatch (momlevel_hip.hip, steric_global_impl /
steric_local_impl down to k1_launch / k2_launch) must still pick exactly that kernel.  The
shapes are the smallest on which each branch is taken: nt = 3, nz = 2; a 2 x 8 plane is whole packs
at both dtypes (the fast kernels), a 3 x 3 plane is odd (the scalar twins).

Axes -- dtype: float64, float32 faithful, float32 upcast, theta32/S64, theta64/S32; variant: steric,
thermosteric (S held: stride 0), halosteric (theta held), all-in-one (the *_decomp entries);
pressure: a z profile or a 16-byte-aligned (z, y, x) field; skip_dry on / off; arith exact / fused
(fields of different dtypes: exact only, the entries refuse fused); K2 only: no delta_rho, float64
delta_rho, float32 delta_rho.  One test per kernel and dtype; a launch takes microseconds.
"""

import itertools
import json
import os

import pytest
import torch

from momlevel_amd import _lib, core

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_names.json")

NT, NZ = 3, 2
PLANES = {"2x8": (2, 8), "3x3": (3, 3)}
# (theta dtype, salinity dtype, f32_mode)
DTYPES = {
    "f64": (torch.float64, torch.float64, "faithful"),
    "f32": (torch.float32, torch.float32, "faithful"),
    "f32_upcast": (torch.float32, torch.float32, "upcast"),
    "t32_s64": (torch.float32, torch.float64, "faithful"),
    "t64_s32": (torch.float64, torch.float32, "faithful"),
}
VARIANTS = ("steric", "thermosteric", "halosteric", "all")
PRESSURES = ("zprofile", "field")
DELTA_RHO = {"none": None, "f64": torch.float64, "f32": torch.float32}


def cases(kernel, dtype):
    """-> [(case id, (variant, plane, pressure, skip_dry, arith, delta_rho))] of one test"""
    ariths = ("exact",) if dtype in ("t32_s64", "t64_s32") else ("exact", "fused")
    drhos = ("-",) if kernel == "k1" else tuple(DELTA_RHO)
    out = []
    for c in itertools.product(VARIANTS, PLANES, PRESSURES, (False, True), ariths, drhos):
        variant, plane, pressure, skip, arith, drho = c
        cid = f"{kernel}/{dtype}/{variant}/{plane}/{pressure}/{'skip' if skip else 'noskip'}/{arith}"
        out.append((cid if kernel == "k1" else f"{cid}/delta_rho-{drho}", c))
    return out


def collect(kernel, dtype):
    """run every case of (kernel, dtype) through core -> {case id: mlx_last_kernel's name}"""
    dt_T, dt_S, f32_mode = DTYPES[dtype]
    names, fields = {}, {}
    for cid, (variant, plane, pressure, skip, arith, drho) in cases(kernel, dtype):
        ny, nx = PLANES[plane]
        if plane not in fields:  # values do not matter to the dispatch: every cell wet, mid-ocean
            kw = dict(dtype=torch.float64, device="cuda")
            fields[plane] = dict(
                T=torch.full((NT, NZ, ny, nx), 10.0, **kw), S=torch.full((NT, NZ, ny, nx), 35.0, **kw),
                vol0=torch.ones((NZ, ny, nx), **kw), dz=torch.ones((NZ, ny, nx), **kw),
                zprofile=torch.tensor([1.0e5, 2.0e5], **kw),
                field=torch.full((NZ, ny, nx), 1.5e5, **kw))
        f = fields[plane]
        T, S = f["T"].to(dt_T), f["S"].to(dt_S)
        p = f[pressure]
        kw = dict(f32_mode=f32_mode, skip_dry=skip, arith=arith)
        if variant == "thermosteric":
            S = S[0]
        elif variant == "halosteric":
            T = T[0]
        if kernel == "k1":
            if variant == "all":
                core.steric_global_decomp(T, S, T[0], S[0], f["vol0"], p, **kw)
            else:
                core.steric_global_masso(T, S, f["vol0"], p, **kw)
        else:
            kw.update(dz=f["dz"], want_delta_rho=drho != "none", delta_rho_dtype=DELTA_RHO[drho])
            if variant == "all":
                core.steric_local_decomp(T, S, T[0], S[0], f["vol0"], f["vol0"][0], p, -1.0 / 1035.0, **kw)
            else:
                core.steric_local(T, S, f["vol0"], f["vol0"][0], p, -1.0 / 1035.0, **kw)
        names[cid] = _lib.last_kernel()
    torch.cuda.synchronize()
    return names


def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_the_fixture_holds_exactly_the_cases_the_tests_run():
    """no case without a recorded name, no recorded name without its case: 256 K1 + 768 K2 launches
    (320 + 960 less the fused cases of the two mixed dtypes)"""
    ids = [cid for k in ("k1", "k2") for d in DTYPES for cid, _ in cases(k, d)]
    assert len(ids) == len(set(ids)) == 256 + 768
    assert set(ids) == set(_golden())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("kernel", ["k1", "k2"])
def test_every_case_launches_the_recorded_kernel(kernel, dtype):
    want = {k: v for k, v in _golden().items() if k.startswith(f"{kernel}/{dtype}/")}
    got = collect(kernel, dtype)
    assert set(got) == set(want)  # every case ran, nothing else did
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} of {len(want)} cases, e.g. {sorted(wrong.items())[:3]}"


if __name__ == "__main__":  # record the fixture: python tests/test_gpu_kernel_names.py OUT.json
    import sys

    rec = {}
    for k in ("k1", "k2"):
        for d in DTYPES:
            rec.update(collect(k, d))
    with open(sys.argv[1], "w") as fh:
        json.dump(rec, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(len(rec), "cases recorded from", os.path.dirname(os.path.abspath(core.__file__)))
