"""GPU: BASELINE.json configs[3] -- the 0.25-degree grid tiled 2x4 over 8 MI355X, 1200 time steps,
one RCCL all-reduce per time chunk -- as far as ONE GPU can take it (VERDICT r2 missing #1):

* one rank's tile of the 2x4 layout at FULL size (540x360x75 cells x 1200 steps = 279.9 GB
  resident, what `bench.py --gpus 8` holds per GPU) through parallel.steric_global_tile_streamed
  in the bench's 5 chunks, against whole-tile oracle slabs from the first, a middle and the last
  chunk;
* the RCCL leg itself: a world of one rank on the "nccl" backend with the per-chunk exchange
  forced active, so librccl loads and the asynchronous all-reduce / wait / stream ordering runs on
  hardware once before the 8-GPU node sees it.
"""

import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from momlevel_amd import core, parallel, synthetic
from oracle import momlevel_numpy as o

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_hbm():
    import gc

    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.timeout(1500)
def test_configs3_one_rank_tile_at_full_size():
    _free_hbm()
    NY, NX, nz, nt, world, rank, chunks = 1080, 1440, 75, 1200, 8, 3, 5
    tile = synthetic.tile_bounds(NY, NX, rank, world)
    th, tw = tile[1] - tile[0], tile[3] - tile[2]
    assert (th, tw) == (540, 360)
    need = 2 * nt * nz * th * tw * 8
    free, _ = torch.cuda.mem_get_info()
    if free < 290e9:
        pytest.skip(f"needs 290 GB of free HBM for the {need / 1e9:.1f} GB record, have {free / 1e9:.0f}")
    g = synthetic.make_grid(NY, NX, nz, tile=tile)
    vol0 = torch.from_numpy(g["volcello"]).cuda()
    pres = o.pressure_from_depth(g["z_l"])
    kw = dict(seed=synthetic.SEED, mask3d=vol0, global_hw=(NY, NX), origin=g["origin"])
    T = core.synth_field((nt, nz, th, tw), field_id=1, lo=-2.0, scale=34.0, **kw)
    S = core.synth_field((nt, nz, th, tw), field_id=2, lo=30.0, scale=10.0, **kw)
    steps = -(-nt // chunks)
    evs = []
    # validate_area=False: one tile's areacello is an eighth of the ocean (the range check belongs
    # to the all-reduced sum, tests/test_gpu_multirank.py)
    out = parallel.steric_global_tile_streamed((T, S), vol0, g["areacello"], pres, steps=steps,
                                               skip_dry=False, validate_area=False,
                                               events=evs)["steric"]
    assert len(evs) == chunks
    m = out["masso"]
    assert m.shape == (nt,) and out["eta"][0] == 0.0 and out["masso0"] == m[0]
    # chunking changes nothing: ONE launch over the whole 1200-step record gives the same bits
    one = core.steric_global_masso(T, S, vol0, pres, skip_dry=False).cpu().numpy()
    assert np.array_equal(one, m)
    # whole-tile oracle slabs: first / last step of the first, the middle and the last chunk
    hk = dict(seed=synthetic.SEED, mask3d=g["volcello"], global_hw=(NY, NX), origin=g["origin"])
    for t in (0, steps - 1, 2 * steps + 7, nt - steps, nt - 1):
        Tn = synthetic.field_numpy((1, nz, th, tw), field_id=1, lo=-2.0, scale=34.0, t0=t, **hk)[0]
        Sn = synthetic.field_numpy((1, nz, th, tw), field_id=2, lo=30.0, scale=10.0, t0=t, **hk)[0]
        ref = o.calc_masso(o.calc_rho(Tn, Sn, pres), g["volcello"])
        assert abs(m[t] - ref) <= 1e-12 * abs(ref), f"t={t}: {m[t]!r} vs {ref!r}"
    # the device generator and the host replay agree on the last slab, tile origin included
    assert np.array_equal(np.nan_to_num(T[nt - 1].cpu().numpy()), np.nan_to_num(Tn))
    ms = [a.elapsed_time(b) for a, b in evs]
    print(f"configs[3] tile {tw}x{th}x{nz} x {nt} steps: K1 per chunk {ms} ms, "
          f"{nt * nz * th * tw / sum(ms) / 1e6:.1f} Gcells/s")
    del T, S
    _free_hbm()


@pytest.mark.timeout(600)
def test_rccl_leg_runs_in_a_world_of_one(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "nccl.npz")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    env.pop("MOMLEVEL_AMD_DIST_BACKEND", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "nccl_worker.py"), out,
                        "11", "6", "16", "24", "4"], env=env, capture_output=True, text=True,
                       timeout=500)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    r = dict(np.load(out))
    assert bool(r["rccl_loaded"]), "librccl was not mapped into the worker"
    # the chunked exchange: 3 chunks of the forced walk, every one a collective on a device buffer
    assert int(r["chunked_collectives"]) == 3 and int(r["chunked_on_device"]) == 3
    # the labelled front end's exchange: unforced it is the identity and NOTHING runs (the control:
    # this is what the round-5 test mistook for the RCCL leg) ...
    assert int(r["unforced_collectives"]) == 0
    assert np.array_equal(r["unforced_vector"], r["payload"])
    for mode in ("ordered", "allreduce"):
        # ... forced, ONE collective on the "nccl" backend, on a device buffer, world of one
        assert int(r[f"labelled_{mode}_collectives"]) == 1, mode
        assert int(r[f"labelled_{mode}_on_device"]) == 1, mode
        assert str(r[f"labelled_{mode}_backend"]) == "nccl"
        assert str(r[f"labelled_{mode}_device"]).startswith("cuda")
        assert int(r[f"labelled_{mode}_world"]) == 1 and str(r[f"labelled_{mode}_mode"]) == mode
        assert np.array_equal(r[f"labelled_{mode}_vector"], r["payload"]), mode
        # parallel.steric / steric_variants / setup_reference_state on momlevel's 5x5x5x5 dataset
        # through RCCL: a global call is 4 flags + sum(areacello) + the data exchange = 6
        # collectives, all on the device; the numbers are the single-domain call's, bit for bit
        assert int(r[f"api_{mode}_collectives_steric"]) == 6, mode
        assert int(r[f"api_{mode}_collectives"]) == int(r[f"api_{mode}_on_device"]) == 13, mode
        for k, single in (("steric", "single_steric"), ("href", "single_href"),
                          ("masso", "single_masso"), ("volo", "single_volo"),
                          ("thermo", "single_thermo"), ("halo", "single_halo"),
                          ("ohc", "single_ohc"), ("setup_masso", "single_masso"),
                          ("setup_volo", "single_volo")):
            assert np.array_equal(r[f"api_{mode}_{k}"], r[single]), (mode, k)
        assert r[f"api_{mode}_steric"][0] == 0.0
    # reference-pinned invariants of the 5x5x5x5 dataset (tests/golden)
    assert float(r["api_ordered_volo"]) == 125921.15458781991
    assert np.array_equal(r["heat_plain"], r["heat_forced"])
    for v in ("steric", "thermosteric", "halosteric"):
        for k in ("masso", "eta", "volo", "masso0", "area_sum"):
            assert np.array_equal(r[f"{v}_{k}_plain"], r[f"{v}_{k}_forced"]), (v, k)
        assert r[f"{v}_eta_forced"][0] == 0.0


@pytest.mark.timeout(600)
def test_bench_force_collective_on_a_small_grid(tmp_path):
    """`python bench.py --force-collective`: the `--gpus 8` step in a world of one
    rank on the RCCL backend, beside the plain step.  Here on a small grid, as a fresh process: one
    JSON line last on stdout (RCCL prints its banner first), every expected collective run, all on
    device buffers, masso / eta bit-identical to the plain step, the contract keys in place."""
    import json

    env = dict(os.environ)
    env.pop("MOMLEVEL_AMD_DIST_BACKEND", None)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--force-collective",
                        "--grid", "9,48,128", "--nt", "13", "--chunks", "5", "--steps", "3",
                        "--warmup", "1"], env=env, capture_output=True, text=True, timeout=500)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["steps"] == 3 and line["warmup"] == 1
    assert line["config"]["forced_collective"] is True and line["config"]["backend"] == "nccl (RCCL)"
    assert line["config"]["time_chunks"] == 5 and "--force-collective" in line["config"]["workload"]
    fc = line["forced_collective"]
    assert fc["collectives_run"] == fc["collectives_expected"] == fc["collectives_on_device"] == (3 + 1) * 5
    assert fc["last_collective"]["backend"] == "nccl" and fc["last_collective"]["world"] == 1
    assert fc["masso_bit_identical_to_plain_step"] and fc["eta_bit_identical_to_plain_step"]
    assert line["eta_t0_is_zero"] is True and line["roofline"]["launches_per_step"] == 5
    assert line["value"] > 0 and line["cpu_baseline"] is None  # (no CPU leg in this mode)


@pytest.mark.timeout(600)
def test_bench_plain_run_dumps_its_last_step(tmp_path):
    """A plain `python bench.py` (no --full) on a small grid, twice, as fresh processes: the contract
    line alone (no BENCH_DETAIL, no CPU leg), --steps honoured, and --dump-outputs writing the last
    timed step's results -- identical from run to run and equal to the line's own masso(t=0)."""
    import json

    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    lines = []
    for k in range(2):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--grid", "9,48,128",
                            "--nt", "13", "--steps", "3", "--warmup", "1", "--dump-outputs",
                            str(tmp_path / f"out{k}")], env=env, capture_output=True, text=True,
                           timeout=280)
        assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
        assert not any(t.startswith("BENCH_DETAIL") for t in p.stdout.splitlines())
        lines.append(json.loads(p.stdout.strip().splitlines()[-1]))
        assert "detail" not in lines[-1]
    for line in lines:
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert line["unit"] == "Mcells/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert line["cpu_baseline"] is None and line["eta_t0_is_zero"] is True
    names = sorted(os.listdir(tmp_path / "out0"))
    assert names == sorted(os.listdir(tmp_path / "out1"))
    assert {"masso.npy", "eta.npy", "expansion_coeff.npy", "masso0.npy"} <= set(names)
    for name in names:
        a, b = np.load(tmp_path / "out0" / name), np.load(tmp_path / "out1" / name)
        assert a.dtype == np.float64 and np.array_equal(a, b, equal_nan=True), name
    masso = np.load(tmp_path / "out0" / "masso.npy")
    assert masso.shape == (13,) and masso[0] == np.load(tmp_path / "out0" / "masso0.npy")
    assert np.load(tmp_path / "out0" / "eta.npy")[0] == 0.0
