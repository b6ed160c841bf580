/*
 * momlevel_regrid.h -- the grid-to-grid remap of libmomlevel_hip.so (gfx950): a gather through a
 * sparse weight table, dst[d] = sum_k S[k] * src[col[k]], over the flattened (y, x) plane of every
 * record of a (nrec, nsrc) record, with the NaN-aware renormalisation that land makes necessary.
 * Conservative coarsening, conservative lat/lon remapping, nearest-point sampling and weights from
 * ESMF_RegridWeightGen / xesmf are this operator with different tables made on the host
 * (momlevel_amd/regrid.py).
 *
 * EXTENSION: momlevel has no such function.
 *
 * A header of its own, as include/momlevel_smooth.h: the entry point has no host build.  It lives in
 * the same library, follows the same conventions (momlevel_hip.h, "Conventions": int status,
 * MLX_E_* argument errors before any HIP call, caller-owned device buffers, the caller's stream
 * last, text through mlx_last_error) and does not move MLX_ABI_VERSION.
 *
 * The table.  Destinations come in slices of L = mlx_regrid_slice() rows; slice s owns destinations
 * s*L .. s*L + L - 1 and the entries from slice_ptr[s] on, stored [k][lane]: entry k of
 * destination d = s*L + lane sits at
 *
 *     pos(d, k) = slice_ptr[s] + k*L + lane,          k = 0 .. len[d] - 1
 *
 * A well-formed table pads every slice to its longest row (slice_ptr[s+1] - slice_ptr[s] =
 * L * max len) and keeps a row's entries in ascending order of col; padding holds col = -1, S = 0.
 *
 * The arithmetic contract (tests/regrid_numpy.py restates it in numpy; results agree with it bit
 * for bit).  All arithmetic is float64 on exactly widened operands (v64); every product and every
 * add is rounded on its own (no FMA).  For destination d and record rec, k = 0 .. len[d] - 1
 * ascending, accumulators start at +0.0, p = pos(d, k):
 *
 *     in_range = 0 <= p < nentries && 0 <= col[p] < nsrc
 *     valid    = in_range && !isnan(v[rec, col[p]])
 *     tot += in_range ? S[p] : 0.0
 *   default (skipna):
 *     num += valid ? S[p] * v64 : 0.0;    den += valid ? S[p] : 0.0;    cnt += valid
 *   MLX_REGRID_PROPAGATE:
 *     num += in_range ? S[p] * v64 : 0.0            (a NaN source makes the sum NaN)
 *
 *     out = canonical NaN   when len[d] <= 0, or (skipna) cnt == 0, or (skipna) den < min_frac * tot
 *         = num / den       skipna (IEEE; a NaN that the arithmetic gives is stored canonical)
 *         = num             MLX_REGRID_PROPAGATE (it wins over MLX_REGRID_NO_RENORM), or skipna with
 *                           MLX_REGRID_NO_RENORM
 *
 * min_frac * tot is one product.  An entry that is out of range -- a position outside the table or
 * a col outside the source plane -- carries no weight: NO content of slice_ptr, len, col or S makes
 * the kernel read outside the buffers it was given (a slice_ptr[s] outside [0, nentries) leaves the
 * whole slice without entries in range).  A corrupt table gives NaNs, not a fault.
 *
 * num and den go through the same operations, so a record of ones gives exactly 1.0 wherever it is
 * not NaN.  The bits of out[rec, d] depend on row d of the table and on record rec alone: not on
 * nrec, on ndst, on the rows around d, on the alignment of the pointers nor on the launch.  No
 * atomics: two runs are bit-identical.  A float32 result is the float64 result rounded once, in the
 * store.  Non-finite weights are outside the contract (the Python layer refuses them).
 *
 * A very long row (a global mean has nsrc entries) is correct but slow: one lane walks it.  That is
 * mlx_area_mean's job (include/momlevel_area.h).
 *
 * NOT BUILT: the generation of bilinear or curvilinear conservative weights (bring them as
 * triplets), the tripolar north fold in the coarsening's periodic option, and tables spread over
 * several ranks.
 */
#ifndef MOMLEVEL_REGRID_H
#define MOMLEVEL_REGRID_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mlx_regrid_apply's flags */
#define MLX_REGRID_PROPAGATE 1 /* a NaN source makes the destination NaN; no renormalisation */
#define MLX_REGRID_NO_RENORM 2 /* skipna, but out = num: the weights present are not renormalised */

/* One wave owns one slice of mlx_regrid_slice() destinations, one lane per destination, and walks
 * mlx_regrid_record_window() records on one read of its entries.  The results depend on neither. */
int64_t mlx_regrid_slice(void);
int64_t mlx_regrid_record_window(void);

/* Block rows along the records (gridDim.y) of a call over nrec records:
 * min(ceil(nrec / mlx_regrid_record_window()), cap).  Up to the cap a block row carries one window
 * of records; past it a row goes on to the window cap rows further, and so on.  Host arithmetic
 * only, the rule the launch itself goes by; a record's bits do not depend on it.  0 for nrec <= 0
 * or nrec > 2^38. */
int mlx_regrid_window_rows(int64_t nrec);

/* v: (nrec, nsrc) C-contiguous, MLX_DTYPE_F64 or MLX_DTYPE_F32 (dtype); slice_ptr:
 * (ceil(ndst / mlx_regrid_slice()) + 1) int64; len: (ndst) int32; col: (nentries) int32; S:
 * (nentries) float64; out: (nrec, ndst), MLX_DTYPE_F64 or MLX_DTYPE_F32 (out_dtype).  All on the
 * device.
 *
 * Refused before any HIP call: an unknown dtype, out_dtype or flag (MLX_E_ENUM); nrec, nsrc, ndst
 * or nentries < 0, nsrc >= 2^31, nrec * max(nsrc, ndst) > 2^38, a min_frac outside [0, 1] or NaN
 * (MLX_E_SHAPE); a NULL operand -- v only when nsrc > 0, col and S only when nentries > 0
 * (MLX_E_NULL); v / out not element-aligned, slice_ptr / S not 8-byte, len / col not 4-byte aligned
 * (MLX_E_ALIGN); an out that overlaps an operand (MLX_E_SHAPE).  Sizes and flags are checked first;
 * then nrec == 0 or ndst == 0 returns 0 without a launch. */
int mlx_regrid_apply(const void *v, int dtype, const int64_t *slice_ptr, const int32_t *len,
                     const int32_t *col, const double *S, int64_t nentries, double min_frac,
                     int flags, int64_t nrec, int64_t nsrc, int64_t ndst, void *out, int out_dtype,
                     void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MOMLEVEL_REGRID_H */
