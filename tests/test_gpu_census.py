"""GPU: the census (momlevel_amd.census, core.census, csrc/momlevel_census.hip) against the numpy
restatement tests/census_numpy.py at every seam of the launch: the sizes at which a wave, a tile or
a block ends (taken from the library's queries), records off the 16-byte grid, every dtype mix, bin
tables up to and past one launch's capacity, record windows, and the five invariants of the order
of summation, bit for bit.

Counts are compared exactly, always.  Integer-valued weights and values make every partial sum an
integer far below 2^53, so the sums are compared exactly too, against int64 arithmetic on the host.
Real-valued operands are held to the project's gate for sums, |sum - ref| <= 1e-10 * sum_bin |w|
(|w v| for vsum); the worst ratio seen is printed."""

import numpy as np
import pytest
import torch

import census_numpy as cn
from momlevel_amd import census, core

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
GATE = 1e-10
E7 = np.array([-2.0, -0.5, 0.0, 0.25, 1.0, 1.5, 4.0, 9.0])   # 7 bins
E3 = np.array([-1.0, 0.0, 2.0, 5.0])                         # 3 bins
E5 = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 8.0])                # 5 bins


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return None if t is None else t.cpu().numpy()


def gpu_sums(fields, edges, w=None, v=None):
    """(count, wsum, vsum) of device copies of the operands, as numpy arrays"""
    out = census.sums(*[_dev(f) for f in fields], bins=list(edges), weights=_dev(w), values=_dev(v),
                      tcoord="dim_0")
    assert out[0].is_cuda and out[0].dtype == torch.int64
    return tuple(_host(t) for t in out)


def make_fields(nrec, ncells, seed, dtypes=(F64, F64), lo=-3.0, hi=10.0):
    """values spread past both ends of E7 / E3 / E5, with some exactly on edges"""
    rng = np.random.default_rng(seed)
    out = []
    for dt in dtypes:
        f = rng.uniform(lo, hi, (nrec, ncells))
        on_edge = rng.random((nrec, ncells)) < 0.2
        f = np.where(on_edge, rng.choice([-2.0, -1.0, 0.0, 0.25, 1.0, 2.0, 4.0, 5.0, 8.0, 9.0],
                                         (nrec, ncells)), f)
        out.append(f.astype(dt))
    return out


def make_int_operands(nrec, ncells, seed, wdt=F64, vdt=F64, per_record=True):
    rng = np.random.default_rng(seed + 1000)
    w = rng.integers(0, 9, (nrec, ncells) if per_record else (ncells,)).astype(wdt)
    v = rng.integers(-8, 9, (nrec, ncells)).astype(vdt)
    return w, v


def exact(fields, edges, w=None, v=None):
    """the census in int64 arithmetic on the host, for integer-valued w and v"""
    nrec, ncells = fields[0].shape
    shape = tuple(e.size - 1 for e in edges)
    nb = int(np.prod(shape))
    count = np.zeros((nrec, nb), dtype=np.int64)
    wsum, vsum = np.zeros_like(count), np.zeros_like(count)
    for r in range(nrec):
        flat, valid = np.zeros(ncells, dtype=np.int64), np.ones(ncells, dtype=bool)
        for d, (f, e) in enumerate(zip(fields, edges)):
            i, inside = cn.bin_index(e, f[r])
            flat, valid = flat * shape[d] + i, valid & inside
        wr = None if w is None else (w[r] if w.ndim == 2 else w)
        if w is not None:
            valid &= ~np.isnan(wr)
        if v is not None:
            valid &= ~np.isnan(v[r])
        np.add.at(count[r], flat[valid], 1)
        if w is not None:
            wi = wr[valid].astype(np.int64)
            assert np.array_equal(wi.astype(np.float64), wr[valid])
            np.add.at(wsum[r], flat[valid], wi)
            if v is not None:
                vi = v[r][valid].astype(np.int64)
                np.add.at(vsum[r], flat[valid], wi * vi)
    assert np.abs(vsum).max(initial=0) < 2 ** 53 and wsum.max(initial=0) < 2 ** 53
    full = (nrec,) + shape
    return (count.reshape(full), None if w is None else wsum.reshape(full).astype(np.float64),
            None if v is None else vsum.reshape(full).astype(np.float64))


def assert_same(got, want, what):
    for name, g, x in zip(("count", "wsum", "vsum"), got, want):
        assert (g is None) == (x is None), f"{what}: {name}"
        if g is not None:
            assert g.shape == x.shape and g.dtype == x.dtype, f"{what}: {name} {g.shape} {g.dtype}"
            assert np.array_equal(g, x), f"{what}: {name} differs in {int((g != x).sum())} bins"
            if g.dtype == np.float64:  # (sums start at +0.0: a zero sum is +0.0)
                assert not (np.signbit(g) & (g == 0)).any(), f"{what}: {name} holds -0.0"


def cell_sizes():
    T = core.census_tile()
    assert T % 64 == 0 and core.census_blocks(8 * T) == 1 and core.census_blocks(8 * T + 1) == 2
    many = 16 * T + 3
    assert core.census_blocks(many) >= 2 and many > core.census_blocks(many) * T
    return [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3, 8 * T + 1, many]


# ---- sizes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(10))
def test_every_seam_of_the_cells(which):
    """nrec = 2: an odd ncells puts the second record off the 16-byte grid (cell-by-cell loads);
    2T + 3 makes one block walk on to a second and third tile, 16T + 3 several blocks several tiles"""
    ncells = cell_sizes()[which]
    f = make_fields(2, ncells, which)
    w, v = make_int_operands(2, ncells, which)
    for fields, edges in (([f[0]], [E7]), (f, [E3, E5])):
        want = exact(fields, edges, w, v)
        assert_same(gpu_sums(fields, edges, w, v), want, f"ncells={ncells} D={len(fields)}")
        assert_same(want, cn.census(fields, edges, w, v), "the restatement")  # (exact sums)
        left = cn.left_out(fields, edges, w, v)
        got = gpu_sums(fields, edges)  # counts alone
        assert_same(got, exact(fields, edges), f"ncells={ncells} counts")
        assert np.array_equal(got[0].reshape(2, -1).sum(axis=1) + left, [ncells, ncells])


@pytest.mark.parametrize("vdt", (None, F64, F32), ids=("nov", "v64", "v32"))
@pytest.mark.parametrize("wdt", (F64, F32), ids=("w64", "w32"))
@pytest.mark.parametrize("fdt", ((F64, F64), (F32, F32), (F64, F32), (F32, F64)),
                         ids=("ff64", "ff32", "f64f32", "f32f64"))
@pytest.mark.parametrize("per_record", (False, True), ids=("static", "perrec"))
def test_every_mix_of_dtypes(per_record, fdt, wdt, vdt):
    T = core.census_tile()
    nrec, ncells = 2, T + 1
    f = make_fields(nrec, ncells, 77, fdt)
    w, v = make_int_operands(nrec, ncells, 77, wdt, vdt or F64, per_record)
    v = None if vdt is None else v
    assert_same(gpu_sums(f, [E3, E5], w, v), exact(f, [E3, E5], w, v), "2-D")
    assert_same(gpu_sums(f[1:], [E7], w, v), exact(f[1:], [E7], w, v), "1-D")


# ---- bins -------------------------------------------------------------------------------------------
def _bin_case(shape_name):
    cap = core.census_max_bins(1, True, True)
    cap2 = core.census_max_bins(2, True, True)
    return {"1": (1,), "2": (2,), "7": (7,), "cap": (cap,), "cap+1": (cap + 1,),
            "2cap+3": (2 * cap + 3,), "1xn": (1, 9), "nx1": (9, 1), "3x5": (3, 5),
            "2xcap2": (2, cap2), "3x(cap2+1)": (3, cap2 + 1), "wide": (cap2 // 9 + 1, 10)}[shape_name]


@pytest.mark.parametrize("name", ("1", "2", "7", "cap", "cap+1", "2cap+3", "1xn", "nx1", "3x5",
                                  "2xcap2", "3x(cap2+1)", "wide"))
def test_tables_up_to_and_past_one_launch(name):
    """the cap, the cap + 1 and 2 cap + 3 bins: the seams of the bin groups; 2-D tables cut into
    bands of rows and rows cut into pieces"""
    shape = _bin_case(name)
    T = core.census_tile()
    nrec, ncells = 2, 3 * T + 5
    rng = np.random.default_rng(len(name) + shape[0])
    edges = [np.linspace(0.0, 1.0, n + 1) for n in shape]
    fields = [rng.uniform(-0.02, 1.02, (nrec, ncells)) for _ in shape]
    for f, e in zip(fields, edges):  # values on edges, the last and the group seams among them
        f[:, ::7] = rng.choice(e, (nrec, f[:, ::7].shape[1]))
        f[:, 5] = e[-1]
    w, v = make_int_operands(nrec, ncells, 5)
    groups = census.plan_bin_groups(shape, core.census_max_bins(len(shape), True, True))
    assert (len(groups) > 1) == (name in ("cap+1", "2cap+3", "2xcap2", "3x(cap2+1)", "wide"))
    assert_same(gpu_sums(fields, edges, w, v), exact(fields, edges, w, v), f"{shape}")
    assert_same(gpu_sums(fields, edges), exact(fields, edges), f"{shape} counts")


# ---- real-valued operands: the gate -------------------------------------------------------------------
@pytest.mark.parametrize("fdt,wdt,vdt", ((F64, F64, F64), (F32, F32, F32), (F64, F32, F64)))
def test_real_valued_sums_stay_inside_the_gate(fdt, wdt, vdt):
    T = core.census_tile()
    nrec, ncells = 2, 16 * T + 3
    rng = np.random.default_rng(11)
    f = make_fields(nrec, ncells, 12, (fdt, fdt))
    w = rng.uniform(0.5, 2.0e3, (ncells,)).astype(wdt)
    v = rng.normal(0.0, 30.0, (nrec, ncells)).astype(vdt)
    worst = 0.0
    for fields, edges in (([f[0]], [E7]), (f, [E3, E5])):
        count, wsum, vsum = gpu_sums(fields, edges, w, v)
        rc, rw, rv = cn.census(fields, edges, w, v)
        aw, av = cn.abs_sums(fields, edges, w, v)
        assert np.array_equal(count, rc)
        for got, ref, scale in ((wsum, rw, np.broadcast_to(aw, rw.shape)), (vsum, rv, av)):
            err = np.abs(got - ref)
            assert (err <= GATE * scale).all()
            worst = max(worst, float(np.max(err / np.maximum(GATE * scale, 1e-300))))
    print(f"worst |sum - ref| / (1e-10 sum|.|) = {worst:.3e}")


# ---- the invariants of the order of summation --------------------------------------------------------
def _real_case(nrec=5, dt=F64):
    T = core.census_tile()
    ncells = 9 * T + 7  # odd: every other record is off the 16-byte grid; two blocks
    rng = np.random.default_rng(21)
    f = make_fields(nrec, ncells, 22, (dt, dt))
    w = rng.uniform(0.1, 3.0, (nrec, ncells)).astype(dt)
    v = rng.normal(0.0, 1.0, (nrec, ncells)).astype(dt)
    return f, w, v


def _same_bits(a, b, what):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and np.array_equal(x.view(np.int64), y.view(np.int64)), what


def test_reruns_and_split_records_agree_to_the_bit():
    f, w, v = _real_case()
    whole = gpu_sums(f, [E3, E5], w, v)
    _same_bits(whole, gpu_sums(f, [E3, E5], w, v), "rerun")
    a = gpu_sums([x[0:2] for x in f], [E3, E5], w[0:2], v[0:2])
    b = gpu_sums([x[2:5] for x in f], [E3, E5], w[2:5], v[2:5])
    _same_bits(whole, [np.concatenate([p, q]) for p, q in zip(a, b)], "records [0:2] + [2:5]")


def test_a_bins_sums_do_not_depend_on_its_bin_group(monkeypatch):
    f, w, v = _real_case(2)

    def grouped(cap, fields, edges):
        with monkeypatch.context() as m:
            m.setattr(core, "census_max_bins", lambda *a, **k: cap)
            return gpu_sums(fields, edges, w, v)

    cap = core.census_max_bins(1, True, True)
    edges = [np.linspace(-2.0, 9.0, cap + 2)]  # cap + 1 bins: two groups, the second of one bin
    assert len(census.plan_bin_groups((cap + 1,), cap)) == 2
    first = gpu_sums(f[:1], edges, w, v)
    _same_bits(first, grouped(100, f[:1], edges), "groups of 100")
    few = [np.linspace(-2.0, 9.0, 6)]
    _same_bits(gpu_sums(f[:1], few, w, v), grouped(1, f[:1], few), "one bin per launch")
    # 2-D: one launch against bands of rows and against rows cut into pieces
    want = gpu_sums(f, [E3, E5], w, v)
    _same_bits(want, grouped(5, f, [E3, E5]), "3 x 5 in rows")
    _same_bits(want, grouped(2, f, [E3, E5]), "3 x 5 in pieces of 2")


def test_weights_of_ones_give_the_count_exactly():
    f, _, _ = _real_case(2, F32)
    for ones in (np.ones(f[0].shape[1], F32), np.ones(f[0].shape, F64)):
        count, wsum, _ = gpu_sums(f, [E3, E5], ones)
        assert np.array_equal(wsum, count.astype(np.float64)) and count.sum() > 0


def test_host_input_gives_the_bits_of_device_input():
    f, w, v = _real_case(3)
    dev = gpu_sums(f, [E3, E5], w, v)
    host = census.sums(*f, bins=[E3, E5], weights=w, values=v, tcoord="dim_0")
    assert all(isinstance(x, np.ndarray) for x in host)
    _same_bits(dev, host, "host arrays")


def test_a_view_one_element_into_a_padded_buffer():
    T = core.census_tile()
    ncells = 2 * T
    f, = make_fields(1, ncells, 31, (F64,))
    w, v = make_int_operands(1, ncells, 31, F32, F32)
    want = exact([f], [E7], w, v)

    def offset(a):
        buf = torch.zeros(a.size + 3, dtype=torch.from_numpy(a).dtype, device="cuda")
        view = buf[1:1 + a.size].view(a.shape)
        view.copy_(torch.from_numpy(a))
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        return view

    got = core.census([offset(f)], [_dev(E7)], offset(w), offset(v))
    assert_same([_host(t) for t in got], [x.reshape(1, -1) for x in want], "offset views")
    got = core.census([_dev(f)], [offset(E7)], _dev(w), _dev(v))  # the edges off the grid too
    assert_same([_host(t) for t in got], [x.reshape(1, -1) for x in want], "offset edges")


# ---- records ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrec", (1, 2, census.RECORD_WINDOW + 1))
def test_records_up_to_and_past_one_window(nrec):
    ncells = 65
    f = make_fields(nrec, ncells, 41)
    w, v = make_int_operands(nrec, ncells, 41, per_record=False)
    per = core.census_blocks(ncells) * 15 * 3 * 8
    assert len(census.plan_record_windows(nrec, ncells, per)) == (2 if nrec > census.RECORD_WINDOW else 1)
    assert_same(gpu_sums(f, [E3, E5], w, v), exact(f, [E3, E5], w, v), f"nrec={nrec}")


def test_a_small_workspace_bound_windows_the_records(monkeypatch):
    f = make_fields(5, 200, 43)
    w, v = make_int_operands(5, 200, 43)
    want = exact(f, [E3, E5], w, v)
    per = core.census_blocks(200) * 15 * 3 * 8
    monkeypatch.setattr(census, "WORKSPACE_BOUND", 2 * per)  # two records' partials
    calls = []
    real = core.census
    monkeypatch.setattr(core, "census",
                        lambda fs, *a, **k: calls.append(int(fs[0].shape[0])) or real(fs, *a, **k))
    assert_same(gpu_sums(f, [E3, E5], w, v), want, "windows of two records")
    assert calls == [2, 2, 1]
