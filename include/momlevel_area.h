/*
 * momlevel_area.h -- area-weighted, NaN-aware means over the horizontal plane of a (record, y, x)
 * field, for one region or many at once, and the anomalies from them, in libmomlevel_hip.so
 * (gfx950).
 *
 * AN EXTENSION: momlevel has no such function.  It is what its documentation does first with a
 * local steric field ("anomalies from the global mean", docs/source/steric.rst), spelled in xarray
 * `xobj.weighted(areacello.fillna(0)).mean((ydim, xdim))`.  The specification is the numpy
 * restatement of tests/area_numpy.py: for every record `rec` and every slot `r`, with v64 and a64
 * the operands widened exactly to float64,
 *
 *     valid = ~isnan(v[rec]) & ~isnan(area) & (slot == r)
 *     w     = where(valid, a64, 0.0)
 *     den   = sum(w)
 *     num   = sum(w * where(valid, v64, 0.0))         one rounding per product, no fma
 *     mean  = num / den                               IEEE: 0 / 0 -> NaN when nothing is valid
 *
 *     anomaly[rec, c] = v64[rec, c] - mean[rec, slot[c]]       NaN where slot[c] < 0
 *
 * THE ORDER OF SUMMATION is fixed and is a function of (plane, v_dtype) only.  The plane is cut
 * into tiles of mlx_area_tile(v_dtype) cells.  Stage 1: one block per tile (and window of
 * MLX_AREA_WINDOW records) -- thread t of the block owns the cells
 * tile * T + (u * 256 + t) * P + k  (P = 16 bytes of the record's dtype, u < T / (256 P), k < P),
 * adds their terms in ascending (u, k) into an accumulator of its own per slot, and the block adds
 * its 256 accumulators per slot as  wave_tree(((c[l] + c[l+64]) + c[l+128]) + c[l+192])  -- the
 * (num, den) partial of that tile, slot and record, stored in the workspace.  Stage 2: one block
 * per (record, slot) adds the tiles' partials, thread t those of the tiles t, t + 256, ... in
 * ascending order, then a binary tree over the 256 threads, and divides.  `num` and `den` go
 * through the SAME tree in the SAME order and `w * v` is one IEEE multiply: a record of ones has
 * num == den bit for bit, so its mean is exactly 1.0 wherever den > 0.  No atomics anywhere: two
 * runs are bit-identical; the result of a record depends neither on nrec, on the records around
 * it, on the alignment of the pointers nor on the path its loads took (16-byte packs where a
 * record's tile is 16-byte aligned and whole, cell by cell elsewhere -- the same cells in the same
 * order).  slot == NULL gives the bits of a slot map that is 0 everywhere.
 *
 * TRAFFIC.  A block keeps its tile's weights and slots in registers across its window of records:
 * the 2-D maps are read once per MLX_AREA_WINDOW records, not once per record.
 *
 * A header of its own, as include/momlevel_spice.h and momlevel_vort.h: the entry points have no
 * host build.  They live in the same library, follow the same conventions (momlevel_hip.h,
 * "Conventions": int status, MLX_E_* argument errors before any HIP call, caller-owned device
 * buffers, the caller's stream last, text through mlx_last_error) and do not move MLX_ABI_VERSION.
 *
 * An infinite area is outside the contract; infinite values propagate as in numpy.  Negative areas
 * are the caller's to refuse (the kernels do not look).
 */
#ifndef MOMLEVEL_AREA_H
#define MOMLEVEL_AREA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the most slots (regions) one launch of mlx_area_mean takes: a thread's accumulators live in LDS,
 * 16 bytes per slot and thread, 64 KiB per block at the cap */
#define MLX_AREA_MAX_SLOTS 16
/* records per block of stage 1 (and of the anomaly pass): how long the maps stay in registers */
#define MLX_AREA_WINDOW 32

/* cells of the plane that one block of stage 1 reduces for a record of `v_dtype` (MLX_DTYPE_F64 or
 * MLX_DTYPE_F32); 0 for any other value */
int64_t mlx_area_tile(int v_dtype);

/* bytes of workspace mlx_area_mean needs: 16 per (record, tile, slot); 0 for arguments the call
 * would refuse */
size_t mlx_area_mean_workspace_bytes(int64_t nrec, int64_t plane, int nslots, int v_dtype);

/* mean[rec, r] and, when `wsum` is not NULL, wsum[rec, r] = den, as defined above.
 *
 *   v:     (nrec, plane)  `v_dtype`             area: (plane)  `area_dtype`
 *   slot:  (plane) int32, the slot 0 .. nslots-1 of every cell, < 0 = no region; NULL = one region
 *          that covers every cell (nslots must then be 1)
 *   mean, wsum: (nrec, nslots) float64          workspace: 8-byte aligned, caller-owned
 * all contiguous on the device.  nrec == 0 or plane == 0 returns 0 without a launch (pointers are
 * not looked at; nothing is written).  A slot value >= nslots is treated as < 0.
 *
 * Refused before any HIP call: a dtype that is not MLX_DTYPE_F64 / MLX_DTYPE_F32 (MLX_E_ENUM);
 * nslots < 1 or > MLX_AREA_MAX_SLOTS, slot == NULL with nslots != 1, nrec or plane < 0,
 * nrec * plane > 2^38 (MLX_E_SHAPE); v, area, mean or workspace NULL with work to do (MLX_E_NULL);
 * workspace_bytes below mlx_area_mean_workspace_bytes or a workspace not 8-byte aligned
 * (MLX_E_WORKSPACE); v / area / slot not aligned to their element, mean / wsum not 8-byte aligned
 * (MLX_E_ALIGN). */
int mlx_area_mean(const void *v, int v_dtype, const void *area, int area_dtype,
                  const int32_t *slot, int nslots, int64_t nrec, int64_t plane, double *mean,
                  double *wsum, void *workspace, size_t workspace_bytes, void *stream);

/* out[rec, c] = (float64) v[rec, c] - mean[rec, slot[c]], NaN where slot[c] is not in
 * 0 .. nslots-1; slot == NULL: out[rec, c] = v[rec, c] - mean[rec] (nslots must be 1).  One IEEE
 * subtraction per cell: bit for bit numpy's `v.astype(float64) - mean`.
 *
 *   v: (nrec, plane) `v_dtype`     slot: (plane) int32 or NULL     mean: (nrec, nslots) float64
 *   out: (nrec, plane) float64
 * nslots is not bounded by MLX_AREA_MAX_SLOTS here (no accumulators): 1 <= nslots <= 2^24.
 *
 * Refused before any HIP call: as above, without the workspace. */
int mlx_area_anomaly(const void *v, int v_dtype, const int32_t *slot, int nslots,
                     const double *mean, int64_t nrec, int64_t plane, double *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MOMLEVEL_AREA_H */
