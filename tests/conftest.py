import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu)")


def _have_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


def pytest_collection_modifyitems(config, items):
    if _have_gpu():
        return
    skip = pytest.mark.skip(reason="no HIP device in this container")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


# torch's own .cpu() / .cuda() as imported, before the fixture below reroutes them (a test that wants
# the stock transfer path -- or wants to spy on it -- wraps these)
STOCK_TRANSFERS = {}


def stock_transfers():
    import torch

    if not STOCK_TRANSFERS:
        STOCK_TRANSFERS.update(cpu=torch.Tensor.cpu, cuda=torch.Tensor.cuda)
    return STOCK_TRANSFERS["cpu"], STOCK_TRANSFERS["cuda"]


@pytest.fixture(scope="session", autouse=True)
def _bulk_transfers_through_pinned_memory():
    """On the GPU box the tests' OWN bulk transfers (``tensor.cpu()``, ``tensor.cuda()`` of 256 KiB
    or more) go through page-locked memory, as the product's do (momlevel_amd.hostio).  A
    PRECAUTION on the checker's side of the suite, not a fix of anything established: both aborts
    this project has seen were GPU page faults on malloc-heap addresses while the runtime was moving
    pageable memory (DESIGN.md section 7 -- which mapping went stale was never determined).
    ``MOMLEVEL_TEST_STOCK_TRANSFERS=1`` switches the rerouting off: the suite then uses torch's
    stock pageable transfers everywhere.  tests/test_gpu_steric.py::
    test_product_moves_bulk_data_through_owned_pinned_memory_only runs with the STOCK functions
    (instrumented) regardless, and asserts that the product itself hands no pageable memory of any
    size that matters to the runtime."""
    orig_cpu, orig_cuda = stock_transfers() if _have_gpu() else (None, None)
    if not _have_gpu() or os.environ.get("MOMLEVEL_TEST_STOCK_TRANSFERS") == "1":
        yield
        return
    import torch

    limit = 256 << 10

    def cpu(self, *args, **kwargs):
        if self.is_cuda and not args and not kwargs and self.numel() * self.element_size() >= limit:
            out = torch.empty(self.shape, dtype=self.dtype, pin_memory=True)
            out.copy_(self)
            return out
        return orig_cpu(self, *args, **kwargs)

    def cuda(self, *args, **kwargs):
        if (not self.is_cuda and not args and not kwargs and not self.is_pinned()
                and self.numel() * self.element_size() >= limit):
            staged = torch.empty(self.shape, dtype=self.dtype, pin_memory=True)
            staged.copy_(self)
            return orig_cuda(staged)
        return orig_cuda(self, *args, **kwargs)

    torch.Tensor.cpu, torch.Tensor.cuda = cpu, cuda
    yield
    torch.Tensor.cpu, torch.Tensor.cuda = orig_cpu, orig_cuda


@pytest.fixture(scope="session", autouse=True)
def _transfer_log():
    """Should a GPU run ever abort again, the log must hold what round 3's did not: the address
    range of every staging / result buffer the product allocated and of every host array it was
    asked to upload, so that a fault address can be matched to a transfer.  momlevel_amd.hostio
    appends them to the file MOMLEVEL_AMD_TRANSFER_LOG names (line-buffered: survives an abort);
    scripts/gpu_pytest.sh keeps the file and the head of any gpucore.* when the run fails."""
    if _have_gpu() and "MOMLEVEL_AMD_TRANSFER_LOG" not in os.environ:
        out = os.path.join(ROOT, "gpurun_out")
        os.makedirs(out, exist_ok=True)
        os.environ["MOMLEVEL_AMD_TRANSFER_LOG"] = os.path.join(out, f"transfer_ranges_{os.getpid()}.log")
    yield


@pytest.fixture(scope="session", autouse=True)
def _built_library():
    """Make sure libmomlevel_hip.so exists (hipcc cross-compiles without a GPU)."""
    from momlevel_amd.csrc import build

    build.build()


@pytest.fixture(scope="session")
def goldens():
    with open(os.path.join(GOLDEN, "reference_goldens.json")) as f:
        return json.load(f)


@pytest.fixture(scope="session")
def wright_vectors():
    # two files (the mixed-operand section on its own) so that each stays under 1 MiB
    vectors = dict(np.load(os.path.join(GOLDEN, "wright_vectors.npz")))
    vectors.update(np.load(os.path.join(GOLDEN, "wright_vectors_mixed.npz")))
    return vectors


@pytest.fixture(scope="session")
def steric_cases():
    return dict(np.load(os.path.join(GOLDEN, "steric_cases.npz")))


MIX_KINDS = ["".join(k) for k in __import__("itertools").product("dfw", repeat=3) if k != ("w", "w", "w")]
MIX_FUNCS = ["density", "drho_dtemp", "drho_dsal", "alpha", "beta", "lin_density", "lin_alpha", "lin_beta"]


def mixed_operands(vectors, kinds):
    """(T, S, p) of tests/golden/make_golden.py section (8) for a kinds string such as "ffw": d = the
    float64 array, f = the same array as float32, w = a python float."""
    ops = []
    for i, (k, name) in enumerate(zip(kinds, "TSp")):
        a = vectors[f"mix_{name}"]
        ops.append(float(vectors["mix_weak"][i]) if k == "w"
                   else a.astype(np.float32) if k == "f" else a)
    return ops


def assert_bit_equal(got, ref, what=""):
    """NaN placement identical; every finite value identical to the last bit."""
    got = np.asarray(got)
    ref = np.asarray(ref)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN mask differs"
    m = ~np.isnan(ref)
    bad = got[m] != ref[m]
    assert not bad.any(), (
        f"{what}: {int(bad.sum())} of {int(m.sum())} finite values differ; "
        f"max rel {np.max(np.abs(got[m][bad] - ref[m][bad]) / np.abs(ref[m][bad])):.3e}"
    )
    # +0.0 == -0.0 compares equal: the sign bit is part of "to the last bit"
    sign = np.signbit(got[m]) != np.signbit(ref[m])
    assert not sign.any(), f"{what}: {int(sign.sum())} values differ in the sign of zero"


def assert_rel(got, ref, rtol, what=""):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN mask differs"
    m = ~np.isnan(ref)
    if m.any():
        err = np.max(np.abs(got[m] - ref[m]) / np.maximum(np.abs(ref[m]), 1e-300))
        assert err <= rtol, f"{what}: max rel err {err:.3e} > {rtol:.1e}"
