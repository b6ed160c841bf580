"""The planted record of the EOF size tests, shared by tests/test_gpu_eof_sizes.py (the public layer
on the GPU against tests/eof_numpy.py) and tests/test_eof_host.py (the restatement against its own
long-double recomputation): both must see the same record, so it is built here and nowhere else.

(nt, 9, 7300): 65 700 cells, a true 2-D cell shape and more than GRAM_MAX_SPLIT minimum ranges, so
core.time_gram cuts it into 32 grown ranges with a short last one.  Three planted modes with
orthogonal zero-mean series and smooth maps, noise 0.01, about 30 % land (NaN at all steps), seven
cells that miss a single step (the first wet cell and the two before the last among them), an area
with NaNs and one non-positive value.  The last cell of all is wet, whole and has an area: the short
last chunk of the short last range carries weight."""

import numpy as np

NY, NX = 9, 7300
NOISE = 0.01
AMPLITUDES = (3.0, 3.2, 4.9)
NEOFS = 11  # two passes of maps (momlevel_amd.eof.MODES_PER_PASS = 8)
OTHER_PERIOD = slice(40, 100)  # the steps of the record projected as "another period", plus 0.25
OTHER_SHIFT = 0.25

# the gates of tests/test_gpu_eof_sizes.py; the restatement alone must sit within a tenth of each
GATE_COV = 1e-10  # of max|cov|
GATE_LAMBDA = 1e-10  # of lambda_1 (the variance fractions: absolute)
GATE_MODES = 1e-9  # pcs and eofs of the planted modes, of their largest magnitude
GATE_PPC = 1e-10  # pseudo-PCs, absolute (the pcs have unit variance)


def planted(nt, ny=NY, nx=NX):
    """``(y, area)``: the float64 record (nt, ny, nx) and its cell areas (ny, nx)"""
    rng = np.random.default_rng(4242)
    t = np.arange(nt)
    series = np.stack([np.sin(2 * np.pi * t / nt), np.cos(2 * np.pi * 2 * t / nt),
                       np.sin(2 * np.pi * 3 * t / nt)])  # orthogonal, zero mean
    yy, xx = np.meshgrid(np.linspace(-1, 1, ny), np.linspace(-1, 1, nx), indexing="ij")
    maps = np.stack([np.exp(-(yy ** 2 + xx ** 2)), 0.6 * xx, 0.35 * yy * (1 - xx ** 2)])
    y = 2.0 + 0.3 * yy + np.einsum("kt,kyx->tyx", series * np.array(AMPLITUDES)[:, None], maps)
    y += NOISE * rng.normal(size=y.shape)
    land = rng.random((ny, nx)) < 0.3
    land[-1, -1] = False  # the last cell of all carries weight: the last chunk of the last range
    y[:, land] = np.nan
    wet = np.flatnonzero(~land.reshape(-1))
    picks = wet[[0, len(wet) // 7, len(wet) // 3, len(wet) // 2, 2 * len(wet) // 3, -3, -2]]
    flat = y.reshape(nt, -1)  # (a view)
    for k, c in enumerate(picks):
        flat[(7 + 19 * k) % nt, c] = np.nan  # one missing step each
    area = 1.0e8 * (1.0 + 0.2 * np.cos(yy))
    area[rng.random((ny, nx)) < 0.01] = np.nan
    area[-1, -1] = 1.0e8
    area.reshape(-1)[wet[len(wet) // 4]] = np.nan  # (wet cells, so that both count)
    area.reshape(-1)[wet[len(wet) // 5]] = -1.0e8  # one non-positive value: no weight, as NaN
    return y, area
