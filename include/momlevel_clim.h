/*
 * momlevel_clim.h -- the grouped time statistic of libmomlevel_hip.so (gfx950): a NaN-skipping
 * mean, standard deviation, minimum or maximum over groups of time steps of a (time, cells) record,
 * one result row per group.
 *
 * It replaces the array arithmetic of momlevel.util.monthly_average (src/momlevel/util.py:454-511:
 * groupby year, then groupby month, .mean) and momlevel.util.annual_cycle (:122-196: groupby
 * month, .mean / .std / .min / .max).  Both are the same computation with different group lists;
 * the lists are made on the host from the calendar (momlevel_amd/climatology.py).
 *
 * A header of its own, as include/momlevel_trend.h: the entry point has no host build.  It lives
 * in the same library, follows the same conventions (momlevel_hip.h, "Conventions": int status,
 * MLX_E_* argument errors before any HIP call, caller-owned device buffers, the caller's stream
 * last, text through mlx_last_error) and does not move MLX_ABI_VERSION.
 *
 * The arithmetic contract -- float64 results are bit-identical to numpy's nanmean / nanstd /
 * nanmin / nanmax over axis 0 of the selected rows:
 *   - per cell, a group's steps are visited in the order steps[] lists them; accumulation is
 *     sequential, in float64, without a tree and without atomics;
 *   - a group is never split between threads: results depend neither on the launch geometry nor
 *     on how a caller blocks the cells between calls;
 *   - MEAN: acc = first value (+0.0 if it is NaN), then acc += value (+0.0 if NaN);
 *     result = acc / count, count the number of non-NaN steps; count == 0 gives canonical NaN;
 *   - STD: population standard deviation (ddof = 0), two passes as numpy: the mean as above, then
 *     d = y - mean, ss += d * d over the valid steps in the same order (no contraction);
 *     result = sqrt(ss / count).  The record is read twice;
 *   - MIN / MAX skip NaN; all-NaN gives NaN;
 *   - an empty group (offsets[g] == offsets[g + 1]) gives a NaN row.
 * float32 records are widened in registers (exact), accumulated in float64 and rounded ONCE, in
 * the store: out = float32(float64 result).  That is not numpy's float32 running sum; it is the
 * correctly rounded statistic (what xarray gives with bottleneck installed).
 */
#ifndef MOMLEVEL_CLIM_H
#define MOMLEVEL_CLIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mlx_clim_group_stat's stat */
#define MLX_STAT_MEAN 0 /* numpy.nanmean(y[sel], axis=0) */
#define MLX_STAT_STD  1 /* numpy.nanstd(y[sel], axis=0), ddof = 0 */
#define MLX_STAT_MIN  2 /* numpy.nanmin(y[sel], axis=0) */
#define MLX_STAT_MAX  3 /* numpy.nanmax(y[sel], axis=0) */

/* y: (nt, n) C-contiguous, MLX_DTYPE_F64 or MLX_DTYPE_F32, on the device.
 * steps: (nsel) int32 time indices in [0, nt), on the device; offsets: (ngroups + 1) int64,
 * non-decreasing, offsets[0] >= 0, offsets[ngroups] <= nsel, on the device: group g is
 * steps[offsets[g] .. offsets[g + 1]).  A step may belong to several groups or to none.
 * out: (ngroups, n), the dtype of y.
 *
 * Any ngroups works: a daily record with one group per step is fine.
 *
 * Refused before any HIP call: a NULL operand (MLX_E_NULL); nt, n, nsel or ngroups <= 0, nt or
 * nsel >= 2^31, nt * n or ngroups * n not addressable (MLX_E_SHAPE); an unknown dtype or stat
 * (MLX_E_ENUM); y / out not element-aligned, steps not 4-byte or offsets not 8-byte aligned
 * (MLX_E_ALIGN).  The CONTENTS of steps and offsets are device
 * memory the entry point cannot read: the caller validates its host-side mirror before upload
 * (momlevel_amd.core.upload_groups does).  The kernel still never reads outside y: it clamps every
 * group to [0, nsel) and treats a step outside [0, nt) as a NaN step. */
int mlx_clim_group_stat(const void *y, int dtype, const int32_t *steps, const int64_t *offsets,
                        int64_t nsel, int64_t ngroups, int64_t nt, int64_t n, int stat, void *out,
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MOMLEVEL_CLIM_H */
