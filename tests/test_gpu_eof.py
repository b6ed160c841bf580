"""GPU: momlevel_amd.eof (time_covariance, calc_eofs, project_field) against the numpy restatement
tests/eof_numpy.py on a (24, 5, 7) record with land, one cell that misses a single step, three
planted modes with orthogonal zero-mean time series and small noise.

The gates: eigenvalues and variance fractions within 1e-10 of lambda_1; pcs and eofs of the three
planted modes within 1e-9 of their largest magnitude -- the two sides differ in G by a rounding of
order n 2^-53 lambda_1, and an eigenvector moves by that over its gap, which the test pins at
lambda_1 / 10 or more on the restatement's own eigenvalues; the reconstruction from nt - 1 modes
within 1e-10 of max|a| (the project's gate for sums)."""

import numpy as np
import pytest
import torch

import eof_numpy as en
from momlevel_amd import eof
from momlevel_amd.labeled import DataArray, Dataset

pytestmark = pytest.mark.gpu

NT, NY, NX = 24, 5, 7


def _planted():
    rng = np.random.default_rng(42)
    t = np.arange(NT)
    series = np.stack([np.sin(2 * np.pi * t / NT), np.cos(2 * np.pi * 2 * t / NT),
                       np.sin(2 * np.pi * 3 * t / NT)])  # orthogonal, zero mean
    yy, xx = np.meshgrid(np.linspace(-1, 1, NY), np.linspace(-1, 1, NX), indexing="ij")
    maps = np.stack([np.exp(-(yy ** 2 + xx ** 2)), 0.6 * xx, 0.35 * yy * (1 - xx ** 2)])
    y = 2.0 + 0.3 * yy + np.einsum("kt,kyx->tyx", series * np.array([3.0, 3.2, 4.9])[:, None], maps)
    y += 0.01 * rng.normal(size=y.shape)
    y[:, 0, 0] = y[:, 0, 1] = y[:, 4, 6] = np.nan  # land
    y[7, 2, 3] = np.nan  # one missing step
    area = 1.0e8 * (1.0 + 0.2 * np.cos(yy))
    area[0, 0] = np.nan
    return y, area


@pytest.fixture(scope="module")
def case():
    y, area = _planted()
    ref4 = en.calc_eofs(y, area, neofs=4)
    time = DataArray(np.arange(NT) * 30.0, ("time",), None, {"axis": "T"}, "time")
    yh = DataArray(np.arange(NY, dtype=float), ("yh",), None, None, "yh")
    xh = DataArray(np.arange(NX, dtype=float), ("xh",), None, None, "xh")
    da = DataArray(y, ("time", "yh", "xh"), {"time": time, "yh": yh, "xh": xh}, {"units": "m"}, "zos")
    out4 = eof.calc_eofs(da, area, neofs=4)
    return y, area, da, ref4, out4


def test_the_planted_modes_are_well_separated(case):
    y, area, _, ref, _ = case
    lam = en.calc_eofs(y, area, neofs=5)["eigenvalues"]
    for k in range(3):  # (the gaps below modes 1, 2 and 3)
        assert lam[k] - lam[k + 1] >= lam[0] / 10, (k, lam)


def test_eigenvalues_and_fractions(case):
    _, _, _, ref, out = case
    assert isinstance(out, Dataset)
    assert sorted(out.data_vars.keys()) == ["eigenvalue_error", "eigenvalues", "eofs", "pcs",
                                            "variance_fraction"]
    lam1 = ref["eigenvalues"][0]
    assert out["eigenvalues"].dims == ("mode",) and out["eigenvalues"].values.dtype == np.float64
    assert np.abs(out["eigenvalues"].values - ref["eigenvalues"]).max() <= 1e-10 * lam1
    assert np.abs(out["variance_fraction"].values - ref["variance_fraction"]).max() <= 1e-10
    assert np.array_equal(out["eigenvalue_error"].values,
                          out["eigenvalues"].values * np.sqrt(2.0 / NT))
    assert out["mode"].values.tolist() == [1, 2, 3, 4]
    assert 0.99 < out["variance_fraction"].values[:3].sum() < 1.0


def test_pcs_and_eofs_of_the_planted_modes(case):
    _, _, da, ref, out = case
    pcs, eofs = out["pcs"].values, out["eofs"].values
    assert out["pcs"].dims == ("time", "mode") and out["eofs"].dims == ("mode", "yh", "xh")
    assert pcs.shape == (NT, 4) and eofs.shape == (4, NY, NX)
    assert np.array_equal(out["eofs"].coords["yh"].values, da.coords["yh"].values)
    assert np.array_equal(out["pcs"].coords["time"].values, da.coords["time"].values)
    assert out["eofs"].attrs["units"] == "m"
    for k in range(3):
        assert np.abs(pcs[:, k] - ref["pcs"][:, k]).max() <= 1e-9 * np.abs(ref["pcs"][:, k]).max()
        assert np.array_equal(np.isnan(eofs[k]), np.isnan(ref["eofs"][k]))
        err = np.nanmax(np.abs(eofs[k] - ref["eofs"][k]))
        assert err <= 1e-9 * np.nanmax(np.abs(ref["eofs"][k])), (k, err)
        assert pcs[np.argmax(np.abs(pcs[:, k])), k] > 0
    assert np.abs((pcs ** 2).sum(axis=0) / (NT - 1) - 1.0).max() <= 1e-12  # unit variance


def test_land_and_the_incomplete_cell_are_left_out(case):
    y, area, _, _, out = case
    eofs = out["eofs"].values
    missing = np.isnan(y).any(axis=0)
    assert missing.sum() == 4 and missing[2, 3]
    assert np.isnan(eofs[:, missing]).all() and not np.isnan(eofs[:, ~missing]).any()
    # the covariance is that of the record without those cells, whatever they hold
    cov = eof.time_covariance(y, area).values
    filled = np.where(np.isnan(y), 7.0, y)
    filled[7, 2, 3] = np.nan  # (still incomplete: still out)
    area2 = area.copy()
    area2[missing] = np.nan
    assert np.array_equal(eof.time_covariance(filled, area2).values, cov)
    ref = en.time_covariance(y, area)
    assert cov.shape == (NT, NT) and np.abs(cov - ref).max() <= 1e-10 * np.abs(ref).max()
    assert np.array_equal(cov, cov.T)
    cov0 = eof.time_covariance(y, area, ddof=0).values
    assert np.allclose(cov0 * NT, cov * (NT - 1), rtol=2e-15, atol=0)  # (two roundings a side)


def test_all_modes_reproduce_the_anomalies(case):
    y, area, _, _, _ = case
    out = eof.calc_eofs(y, area, neofs=NT - 1)
    anom = y - y.mean(axis=0)
    rec = np.einsum("tk,kyx->tyx", out["pcs"].values, out["eofs"].values)
    full = ~np.isnan(y).any(axis=0)
    assert np.array_equal(np.isnan(rec), np.broadcast_to(~full, rec.shape))
    assert np.abs(rec[:, full] - anom[:, full]).max() <= 1e-10 * np.abs(anom[:, full]).max()
    assert out["pcs"].dims == ("time", "mode") and out["pcs"].shape == (NT, NT - 1)  # (3 passes of maps)


def test_projecting_the_record_returns_its_pcs(case):
    y, area, da, _, out = case
    ppc = eof.project_field(da, out["eofs"], area)
    assert ppc.dims == ("time", "mode") and ppc.values.shape == (NT, 4)
    assert np.abs(ppc.values - out["pcs"].values).max() <= 1e-10
    assert np.abs(eof.project_field(y, out, area).values - ppc.values).max() == 0.0
    ref = en.project_field(y, out["eofs"].values, area)
    assert np.abs(ppc.values - ref).max() <= 1e-10
    # another period against the first one's climatology
    center = en.cell_maps(y)[0].reshape(NY, NX)  # (NaN where a step is missing)
    shifted = y[5:17] + 0.25
    got = eof.project_field(shifted, out["eofs"], area, center=center).values
    want = en.project_field(shifted, out["eofs"].values, area, center=center)
    assert got.shape == (12, 4) and np.abs(got - want).max() <= 1e-10


def test_device_in_device_out_and_float32(case):
    y, area, _, ref, out = case
    dev = torch.from_numpy(y).cuda()
    res = eof.calc_eofs(DataArray(dev, ("time", "yh", "xh")), area, neofs=4)
    for name in ("eigenvalues", "variance_fraction", "eigenvalue_error", "pcs", "eofs"):
        t = res[name].data
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64, name
        assert np.array_equal(t.cpu().numpy(), out[name].values, equal_nan=True), name
    cov = eof.time_covariance(dev, torch.from_numpy(area).cuda())
    assert cov.data.is_cuda and tuple(cov.shape) == (NT, NT)
    ppc = eof.project_field(dev, res["eofs"], area)
    assert ppc.data.is_cuda and np.abs(ppc.data.cpu().numpy() - out["pcs"].values).max() <= 1e-10
    # float32 in, float64 out: the restatement of the SAME float32 values
    y32 = y.astype(np.float32)
    r32 = eof.calc_eofs(y32, area.astype(np.float32), neofs=3)
    want = en.calc_eofs(y32.astype(np.float64), area.astype(np.float32).astype(np.float64), neofs=3)
    for name in ("eigenvalues", "pcs", "eofs"):
        v = r32[name].values
        assert v.dtype == np.float64
        scale = np.nanmax(np.abs(want[name]))
        assert np.nanmax(np.abs(v - want[name])) <= 1e-9 * scale, name
    d32 = eof.calc_eofs(torch.from_numpy(y32).cuda(), area, neofs=3)
    assert d32["eofs"].data.dtype == torch.float64 and d32["pcs"].data.dtype == torch.float64
