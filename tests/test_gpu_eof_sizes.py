"""GPU: momlevel_amd.eof (time_covariance, calc_eofs, project_field) against the numpy restatement
tests/eof_numpy.py at a size the Gram kernel SPLITS: the record of tests/eof_cases.py, (tile + 5, 9,
7300) -- 65 700 cells in GRAM_MAX_SPLIT grown ranges with a short last one, two tiles of time steps
(three tile pairs), a true 2-D cell shape, maps in two passes of modes.  tests/test_gpu_eof.py runs
the same layer on 35 cells: one range, one tile.

The gates are those tests/test_gpu_eof.py derives (tests/eof_cases.py GATE_*): the two sides differ
in G by a rounding of order n 2^-53 lambda_1 -- 7e-12 lambda_1 at this n, still below 1e-10 -- and an
eigenvector moves by that over its gap, pinned at lambda_1 / 10 or more on the restatement's own
eigenvalues.  tests/test_eof_host.py::test_the_restatement_sits_a_tenth_inside_the_gates_of_the_size_case
shows that the restatement's own rounding on this very record is below a tenth of each.  Every gate
prints the worst observed error as a fraction of it."""

import numpy as np
import pytest
import torch

import eof_cases as ec
import eof_numpy as en
from momlevel_amd import _lib, core, eof
from momlevel_amd.labeled import DataArray, Dataset

pytestmark = pytest.mark.gpu

NY, NX, NEOFS = ec.NY, ec.NX, ec.NEOFS


def _assert_grown(n):
    """the Gram kernel cuts ``n`` cells into GRAM_MAX_SPLIT ranges longer than the minimum one"""
    cells = core.gram_cells(n)
    assert cells > core.gram_cells(1) and -(-n // cells) == _lib.GRAM_MAX_SPLIT, (n, cells)


def _gate(what, err, gate):
    print(f"{what}: worst error / gate = {err / gate:.3e}")
    assert err <= gate, (what, err, gate)


@pytest.fixture(scope="module")
def case():
    nt = core.gram_tile() + 5
    y, area = ec.planted(nt)
    assert y.shape == (nt, NY, NX) and NEOFS > eof.MODES_PER_PASS
    _assert_grown(NY * NX)
    ref = en.calc_eofs(y, area, neofs=NEOFS)
    time = DataArray(np.arange(nt) * 30.0, ("time",), None, {"axis": "T"}, "time")
    yh = DataArray(np.arange(NY, dtype=float), ("yh",), None, None, "yh")
    xh = DataArray(np.arange(NX, dtype=float), ("xh",), None, None, "xh")
    da = DataArray(y, ("time", "yh", "xh"), {"time": time, "yh": yh, "xh": xh}, {"units": "m"}, "zos")
    out = eof.calc_eofs(da, area, neofs=NEOFS)
    return dict(nt=nt, y=y, area=area, da=da, ref=ref, out=out)


def test_the_planted_modes_are_well_separated(case):
    lam = case["ref"]["eigenvalues"]
    for k in range(3):  # (the gaps below modes 1, 2 and 3: a condition on the input)
        assert lam[k] - lam[k + 1] >= lam[0] / 10, (k, lam)


def test_the_record_has_what_the_case_promises(case):
    y, area = case["y"], case["area"]
    land = np.isnan(y).all(axis=0)
    once = np.isnan(y).sum(axis=0) == 1
    assert 0.28 < land.mean() < 0.32 and once.sum() == 7
    assert once.reshape(-1)[np.flatnonzero(~land.reshape(-1))[[0, -3, -2]]].all()
    # the last cell of all carries weight, in the last chunk of the short last range
    assert not np.isnan(y[:, -1, -1]).any() and area[-1, -1] > 0
    assert (NY * NX) % core.gram_cells(NY * NX) % 16 != 0
    assert np.isnan(area).sum() > 100 and (area <= 0).sum() == 1 and not land[area <= 0].any()


def test_time_covariance(case):
    y, area, nt = case["y"], case["area"], case["nt"]
    cov = eof.time_covariance(y, area).values
    ref = en.time_covariance(y, area)
    assert cov.shape == (nt, nt) and cov.dtype == np.float64
    _gate("time_covariance", np.abs(cov - ref).max(), ec.GATE_COV * np.abs(ref).max())
    assert np.array_equal(cov.view(np.int64), cov.T.copy().view(np.int64))
    cov0 = eof.time_covariance(y, area, ddof=0).values
    rel = np.abs(cov0 * nt - cov * (nt - 1)) / np.abs(cov * (nt - 1))
    print(f"ddof=0 against ddof=1: worst relative difference / 2e-15 = {rel.max() / 2e-15:.3e}")
    assert np.allclose(cov0 * nt, cov * (nt - 1), rtol=2e-15, atol=0)  # (two roundings a side)
    # the cells without weight are left out whatever they hold
    missing = np.isnan(y).any(axis=0)
    filled = np.where(np.isnan(y), 7.0, y)
    area2 = area.copy()
    area2[missing] = np.nan
    assert np.array_equal(eof.time_covariance(filled, area2).values, cov)


def test_eigenvalues_and_fractions(case):
    ref, out, nt = case["ref"], case["out"], case["nt"]
    assert isinstance(out, Dataset)
    lam1 = ref["eigenvalues"][0]
    lam = out["eigenvalues"].values
    assert lam.shape == (NEOFS,) and lam.dtype == np.float64 and np.all(np.diff(lam) < 0)
    _gate("eigenvalues", np.abs(lam - ref["eigenvalues"]).max(), ec.GATE_LAMBDA * lam1)
    _gate("variance fractions", np.abs(out["variance_fraction"].values - ref["variance_fraction"]).max(),
          ec.GATE_LAMBDA)
    assert np.array_equal(out["eigenvalue_error"].values, lam * np.sqrt(2.0 / nt))
    assert out["mode"].values.tolist() == list(range(1, NEOFS + 1))
    assert 0.99 < out["variance_fraction"].values[:3].sum() < 1.0


def test_pcs_and_eofs(case):
    y, ref, out, nt = case["y"], case["ref"], case["out"], case["nt"]
    pcs, eofs = out["pcs"].values, out["eofs"].values
    assert out["pcs"].dims == ("time", "mode") and out["eofs"].dims == ("mode", "yh", "xh")
    assert pcs.shape == (nt, NEOFS) and eofs.shape == (NEOFS, NY, NX)  # (two passes of maps)
    for k in range(3):
        _gate(f"pc {k + 1}", np.abs(pcs[:, k] - ref["pcs"][:, k]).max(),
              ec.GATE_MODES * np.abs(ref["pcs"][:, k]).max())
        _gate(f"eof {k + 1}", np.nanmax(np.abs(eofs[k] - ref["eofs"][k])),
              ec.GATE_MODES * np.nanmax(np.abs(ref["eofs"][k])))
    # every map, the second pass included: NaN exactly where the restatement's is -- where a step
    # is missing
    assert np.array_equal(np.isnan(eofs), np.isnan(ref["eofs"]))
    assert np.array_equal(np.isnan(eofs), np.broadcast_to(np.isnan(y).any(axis=0), eofs.shape))
    # the noise modes' eigenvectors are not pinned by the restatement (near-degenerate), their maps
    # are: E_k = pc_k' a / N of the module's OWN pcs, contracted on the host -- both passes of modes
    full = ~np.isnan(y).any(axis=0)
    anom = y[:, full] - en.cell_maps(y)[0].reshape(NY, NX)[full][None, :]
    own = pcs.T @ anom / (nt - 1)
    for k in range(NEOFS):
        _gate(f"eof {k + 1} against the host contraction of its own pc",
              np.abs(eofs[k][full] - own[k]).max(), ec.GATE_MODES * np.abs(own[k]).max())
    unit = np.abs((pcs ** 2).sum(axis=0) / (nt - 1) - 1.0).max()
    _gate("unit variance of the pcs", unit, 1e-12)
    for k in range(NEOFS):  # the sign rule
        assert pcs[np.argmax(np.abs(pcs[:, k])), k] > 0, k


def test_projecting_the_record_returns_its_pcs(case):
    """ppc_k = C pc_k N / (pc_k' C pc_k) in exact arithmetic, and pc_k is an eigenvector of the
    COMPUTED covariance matrix, which differs from C by a rounding of order n 2^-53 lambda_1: the
    pseudo-PC leaves pc_k by that over lambda_k.  For the planted modes (lambda_1 / lambda_3 < 5)
    that is some 3e-11, inside the 1e-10 gate.  The eight noise modes have lambda_1 / lambda_k near
    2e6: their identity holds to n 2^-53 lambda_1 / lambda_k only, which is their gate here; what
    pins them to 1e-10 is the restatement projecting onto the SAME maps."""
    y, area, da, ref, out, nt = (case[k] for k in ("y", "area", "da", "ref", "out", "nt"))
    ppc = eof.project_field(da, out["eofs"], area)
    assert ppc.dims == ("time", "mode") and ppc.values.shape == (nt, NEOFS)
    pcs = out["pcs"].values
    _gate("project_field of the record against its pcs, planted modes",
          np.abs(ppc.values[:, :3] - pcs[:, :3]).max(), ec.GATE_PPC)
    lam = ref["eigenvalues"]
    assert lam[0] / lam[2] < 5 and np.all(lam[0] / lam[3:] > 1e6)
    for k in range(3, NEOFS):
        _gate(f"project_field of the record against its pcs, noise mode {k + 1}",
              np.abs(ppc.values[:, k] - pcs[:, k]).max(),
              NY * NX * 2.0 ** -53 * lam[0] / lam[k] * np.abs(pcs[:, k]).max())
    want = en.project_field(y, out["eofs"].values, area)
    _gate("project_field of the record against the restatement, all modes",
          np.abs(ppc.values - want).max(), ec.GATE_PPC)


def test_projecting_another_period_against_a_center_that_excludes_cells(case):
    y, area, out = case["y"], case["area"], case["out"]
    center = en.cell_maps(y)[0].reshape(NY, NX)  # the climatology: NaN where a step is missing
    assert np.isnan(center).sum() > np.isnan(y).all(axis=0).sum()
    other = y[ec.OTHER_PERIOD] + ec.OTHER_SHIFT
    got = eof.project_field(other, out["eofs"], area, center=center).values
    want = en.project_field(other, out["eofs"].values, area, center=center)
    assert got.shape == (other.shape[0], NEOFS) and np.isfinite(want).all()
    _gate("project_field of another period", np.abs(got - want).max(), ec.GATE_PPC)


def test_device_in_device_out_with_the_values_of_host_in(case):
    y, area, out, nt = case["y"], case["area"], case["out"], case["nt"]
    dev = torch.from_numpy(y).cuda()
    res = eof.calc_eofs(DataArray(dev, ("time", "yh", "xh")), area, neofs=NEOFS)
    for name in ("eigenvalues", "variance_fraction", "eigenvalue_error", "pcs", "eofs"):
        t = res[name].data
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64, name
        assert np.array_equal(t.cpu().numpy(), out[name].values, equal_nan=True), name
    cov = eof.time_covariance(dev, torch.from_numpy(area).cuda())
    assert cov.data.is_cuda and tuple(cov.shape) == (nt, nt)
    assert np.array_equal(cov.data.cpu().numpy(), eof.time_covariance(y, area).values)
    ppc = eof.project_field(dev, res["eofs"], area)
    assert ppc.data.is_cuda
    assert np.array_equal(ppc.data.cpu().numpy(), eof.project_field(y, out["eofs"], area).values)


def test_a_float32_record_against_the_restatement_of_the_same_values(case):
    y, area = case["y"], case["area"]
    y32, area32 = y.astype(np.float32), area.astype(np.float32)
    r32 = eof.calc_eofs(y32, area32, neofs=3)
    want = en.calc_eofs(y32.astype(np.float64), area32.astype(np.float64), neofs=3)
    for name in ("eigenvalues", "pcs", "eofs"):
        v = r32[name].values
        assert v.dtype == np.float64
        _gate(f"float32 record, {name}", np.nanmax(np.abs(v - want[name])),
              1e-9 * np.nanmax(np.abs(want[name])))
    assert np.array_equal(np.isnan(r32["eofs"].values), np.isnan(want["eofs"]))


def test_an_integer_record_gives_the_bits_of_its_float64_copy():
    """integers are read as float64 (momlevel_amd.eof._Prepared)"""
    rng = np.random.default_rng(31)
    yi = rng.integers(-2000, 2001, (12, NY, NX)).astype(np.int32)
    _assert_grown(NY * NX)
    area = rng.uniform(1.0, 3.0, (NY, NX))
    got = eof.time_covariance(yi, area).values
    want = eof.time_covariance(yi.astype(np.float64), area).values
    assert got.dtype == np.float64 and np.isfinite(got).all() and np.abs(got).max() > 0
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    ref = en.time_covariance(yi, area)
    assert np.abs(got - ref).max() <= ec.GATE_COV * np.abs(ref).max()
