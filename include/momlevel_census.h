/*
 * momlevel_census.h -- the census of libmomlevel_hip.so (gfx950): weighted histograms of a record by
 * value class.  For every record of a (nrec, ncells) record and every bin of a table over one or two
 * binning fields: the number of cells in the bin, the sum of a weight over them and the sum of
 * weight * value.  A volumetric theta-S (or sigma-pi) census, the area of ocean per class of trend,
 * the PDF of eta: a scatter whose bin depends on the data, with an answer of nbins numbers per
 * record.  Binning by a STATIC map (zonal bands, basins) needs none of this: that is a sparse table
 * for mlx_regrid_apply or a label map for mlx_area_mean.
 *
 * EXTENSION: momlevel has no such function.
 *
 * A header of its own, as include/momlevel_regrid.h: the entry points have no host build.  They live
 * in the same library, follow the same conventions (momlevel_hip.h, "Conventions": int status,
 * MLX_E_* argument errors before any HIP call, caller-owned device buffers, the caller's stream
 * last, text through mlx_last_error) and do not move MLX_ABI_VERSION.
 *
 * The contract (tests/census_numpy.py restates it in numpy; it is numpy.histogramdd with explicit
 * edges).  D = 1 or 2 binning fields f_d, each with n_d + 1 strictly increasing finite float64
 * edges e_d; field values are widened exactly to float64 before any comparison.
 *
 *     i_d = (number of edges e_d[j] <= f_d) - 1          (searchsorted(e_d, f_d, side="right") - 1)
 *     i_d = n_d - 1   when f_d == e_d[n_d] and bit d of `closed` is set
 *     the cell is left out when some i_d is outside 0 .. n_d - 1: a value below the first edge,
 *     above the last, +-inf, NaN.  -0.0 lies in the bin that starts at 0.0.
 *     bin = i_0                (D = 1)        bin = i_0 * n_1 + i_1        (D = 2)
 *
 * `closed` is 3 for a whole table.  A launch over a sub-range of a larger table's edges (a "bin
 * group") clears the bit of a field whose last edge is not the table's last: then the value on it
 * belongs to the next group.  Cells of other groups are left out, not added as zeros.
 *
 * A cell whose weight or value is NaN is left out of all three outputs (this differs from numpy,
 * which would poison the bin; it is the `valid` rule of mlx_area_mean).  Per record and bin, over
 * the cells that are left in:
 *
 *     count = number of cells                                   int64
 *     wsum  = sum w                                             float64, when w is given
 *     vsum  = sum w * v   (each product rounded once, no FMA)   float64, when val is given too
 *
 * Weights and values are widened exactly.  Sums start at +0.0.
 *
 * ORDER OF SUMMATION.  No atomics of any kind, global or LDS.  A record is cut into tiles of
 * mlx_census_tile() cells; mlx_census_blocks(ncells) blocks of four waves work on it, block b on the
 * tiles b, b + blocks, ... in ascending order.  In a tile thread t owns the four cells 4t .. 4t + 3;
 * the wave handles its lanes' cell k together, k = 0 .. 3: the lanes of one bin are added by a fixed
 * 64-lane tree in which every other lane holds +0.0, and the tree's sum is added to the wave's
 * private LDS histogram.  The block then adds its four waves' histograms in ascending wave order and
 * stores one partial per (record, block, bin); a second kernel adds the partials in ascending block
 * order.  The order is a function of (ncells, the cell's place in the record) only: the bits of a
 * bin's sums do not depend on the pointers' alignment (16-byte pack loads and cell-by-cell loads
 * give the same cell to the same lane), on the number of CUs, on nrec, on the other bins of the
 * launch or on the bin group.  Weights of 1.0 give wsum == count exactly.
 *
 * RESOURCES.  mlx_census_max_bins bins per launch: what fits 64 KiB of LDS per block with the edges
 * and four private histograms (4, 12 or 20 bytes per bin and wave).  Larger tables are launched in
 * bin groups by the caller (momlevel_amd/census.py), the fields re-read once per group.  The
 * workspace holds the partials only -- nrec * blocks * nbins words of 8 bytes per output -- and
 * never scales with ncells * nbins.
 *
 * No table content can make the kernel address outside its LDS histogram: the search is bounded by
 * the number of edges, and its result is tested against 0 .. n_d - 1 before it is an address.
 * Edges that are not increasing give wrong bins, never a wild write.
 *
 * NOT BUILT: more than two binning fields; the sigma evaluation fused into the census (as the column
 * search fuses it); a census over several ranks (the partials are additive over tiles); a table in
 * global memory for very large nbins.
 */
#ifndef MOMLEVEL_CENSUS_H
#define MOMLEVEL_CENSUS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Cells of one tile, and the blocks that share a record of ncells cells (0 for ncells <= 0): a pure
 * function of ncells. */
int64_t mlx_census_tile(void);
int64_t mlx_census_blocks(int64_t ncells);

/* The most bins (n_0, or n_0 * n_1) of one launch; 0 for a D outside {1, 2} or values without
 * weights.  has_weights / has_values: 0 or not 0. */
int64_t mlx_census_max_bins(int D, int has_weights, int has_values);

/* Bytes of workspace mlx_census_histogram needs; 0 for sizes it refuses. */
size_t mlx_census_workspace_bytes(int64_t nrec, int64_t ncells, int64_t nbins, int has_weights,
                                  int has_values);

/* f0, f1: (nrec, ncells) C-contiguous, MLX_DTYPE_F64 or MLX_DTYPE_F32 each (f1 is read when D == 2);
 * edges0: (n0 + 1) float64, edges1: (n1 + 1) float64 when D == 2 (n1 must be 1 when D == 1); w: NULL
 * or weights, (ncells) when w_per_record == 0 and (nrec, ncells) otherwise; val: NULL or
 * (nrec, ncells) values, which need w; count: (nrec, nbins) int64; wsum, vsum: (nrec, nbins)
 * float64, wsum required with w and vsum with val (ignored otherwise); nbins = n0 * n1.  All on the
 * device.
 *
 * Refused before any HIP call: an unknown dtype, a closed outside 0 .. 3 (MLX_E_ENUM); D outside
 * {1, 2}, n0 or n1 < 1, nbins over mlx_census_max_bins, nrec or ncells < 0, ncells > 2^38,
 * nrec * ncells > 2^40, nrec * blocks >= 2^31, val without w (MLX_E_SHAPE); a NULL operand or result
 * (MLX_E_NULL); pointers not aligned to their element (MLX_E_ALIGN); a workspace that is too small
 * or not 8-byte aligned (MLX_E_WORKSPACE).  Sizes, dtypes and flags are checked first; then nrec == 0
 * or ncells == 0 returns 0 without a launch and without a look at the pointers (the results are not
 * written). */
int mlx_census_histogram(const void *f0, int f0_dtype, const void *f1, int f1_dtype, int D,
                         const double *edges0, int64_t n0, const double *edges1, int64_t n1,
                         int closed, const void *w, int w_dtype, int w_per_record, const void *val,
                         int val_dtype, int64_t nrec, int64_t ncells, int64_t *count, double *wsum,
                         double *vsum, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MOMLEVEL_CENSUS_H */
