/*
 * momlevel_quantile.h -- the order statistics of libmomlevel_hip.so (gfx950): NaN-skipping
 * quantiles over groups of time steps of a (time, cells) record, one result row per group and
 * quantile, and the count of steps above a per-cell threshold.
 *
 * EXTENSION: momlevel has no such function.  The arithmetic authority is numpy's
 * nanquantile(..., method="linear"), which xarray's .quantile(q, dim="time") calls.
 *
 * A header of its own, as include/momlevel_clim.h: the entry points have no host build.  They live
 * in the same library, follow the same conventions (momlevel_hip.h, "Conventions": int status,
 * MLX_E_* argument errors before any HIP call, caller-owned device buffers, the caller's stream
 * last, text through mlx_last_error) and do not move MLX_ABI_VERSION.
 *
 * The arithmetic contract (tests/quantile_numpy.py restates it with numpy.sort), per cell, group of
 * steps and q:
 *   - c is the number of listed steps whose value is not NaN; a step outside [0, nt) is a NaN
 *     step.  c == 0 (an empty group included) gives canonical NaN;
 *   - vi = (c - 1) * q in float64 (numpy 2.2's virtual index of "linear");
 *   - vi >= c - 1:  lo = hi = c - 1, prev = -1;
 *     vi < 0:       lo = hi = 0,     prev = 0;
 *     otherwise:    lo = floor(vi),  hi = lo + 1, prev = lo;
 *   - g = vi - prev (numpy's gamma);
 *   - a, b are the lo-th and hi-th smallest valid values (0-based);
 *   - d = b - a;  r = a + d * g;  if g >= 0.5 then r = b - d * (1 - g);
 *   - plain float64 operators, no contraction.
 * float64 records give float64 results, value-identical to numpy.nanquantile(y[sel], q, axis=0),
 * numpy's own NaN where a and b are the same infinity included.  The one difference allowed is the
 * sign of a zero result: the selection orders -0.0 before +0.0, numpy's partition leaves either.
 * float32 records are widened exactly, selected and interpolated in float64 and rounded ONCE, in
 * the store (the convention of momlevel_clim.h and momlevel_filter.h; not numpy's float32 lerp).
 * A step listed twice counts twice.  A cell's selection never leaves its lane: the results depend
 * neither on the launch geometry nor on how a caller splits the cells between calls.
 */
#ifndef MOMLEVEL_QUANTILE_H
#define MOMLEVEL_QUANTILE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the most quantiles one mlx_quantile_select call takes */
#define MLX_QUANTILE_MAX_Q 8

/* Cells one block of the pack path covers for a record of dtype (block threads times the cells of
 * a 16-byte pack); 0 for an unknown dtype.  The results do not depend on it. */
int64_t mlx_quantile_block_cells(int dtype);

/* Rows of a group whose loads a lane issues before it consumes the first of them.  The results do
 * not depend on it. */
int64_t mlx_quantile_unroll(void);

/* y: (nt, n) C-contiguous, MLX_DTYPE_F64 or MLX_DTYPE_F32, on the device.
 * steps: (nsel) int32 time indices, offsets: (ngroups + 1) int64, both on the device, as in
 * mlx_clim_group_stat: group g is steps[offsets[g] .. offsets[g + 1]); their CONTENTS are the
 * caller's to validate (momlevel_amd.core.upload_groups does).  The kernel still never reads
 * outside y: it clamps every group to [0, nsel) and treats a step outside [0, nt) as a NaN step.
 * steps == offsets == NULL with ngroups == 1 and nsel == nt: all rows, in order, without the
 * indirection.
 * q: HOST array of nq doubles, 1 <= nq <= MLX_QUANTILE_MAX_Q, each in [0, 1].
 * out: (nq, ngroups, n), the dtype of y, on the device.
 *
 * Refused before any HIP call: y, q or out NULL, one list NULL without the other, both NULL with
 * ngroups != 1 (MLX_E_NULL); nt, n, nsel or ngroups <= 0, nt or nsel >= 2^31, n > 2^38, nt * n or
 * nq * ngroups * n not addressable, nq outside [1, 8], NULL lists with nsel != nt (MLX_E_SHAPE);
 * an unknown dtype, a q outside [0, 1] or NaN (MLX_E_ENUM); y / out not element-aligned, steps not
 * 4-byte or offsets not 8-byte aligned (MLX_E_ALIGN). */
int mlx_quantile_select(const void *y, int dtype, const int32_t *steps, const int64_t *offsets,
                        int64_t nsel, int64_t ngroups, int64_t nt, int64_t n, const double *q,
                        int nq, void *out, void *stream);

/* out[g][cell] = the number of steps of group g with y > thr[g][cell]: strict, compared in
 * float64; a NaN on either side (or a step outside [0, nt)) counts nothing.
 * y, steps, offsets, nsel, ngroups, nt, n: as above.  thr: (ngroups, n) float64, out: (ngroups, n)
 * int64, both on the device.  Refusals as above (thr / out 8-byte aligned). */
int mlx_quantile_exceed_count(const void *y, int dtype, const int32_t *steps,
                              const int64_t *offsets, int64_t nsel, int64_t ngroups, int64_t nt,
                              int64_t n, const double *thr, int64_t *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MOMLEVEL_QUANTILE_H */
