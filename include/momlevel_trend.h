/*
 * momlevel_trend.h -- the trend entry points of libmomlevel_hip.so (gfx950): per-cell fits along
 * the time axis of a (time, cells) record and the elementwise pass that applies them.
 *
 * They replace the array arithmetic of momlevel.trend (src/momlevel/trend.py): xarray's
 * polyfit(dim, 1) behind calc_linear_trend (:252), the fitted line of broadcast_trend /
 * _detrend_array (:105, :190-202), and the pinv / dot model of seasonal_model (:412-431) and
 * seasonal_cycle_model (:523-532).
 *
 * A header of its own: include/momlevel_hip.h is the ABI the host build of the checker restates
 * symbol for symbol, and these entry points have no host build.  They live in the same library,
 * follow the same conventions (momlevel_hip.h, "Conventions": int status, MLX_E_* argument errors
 * before any HIP call, caller-owned device buffers, a *_workspace_bytes() query, the caller's
 * stream last, text through mlx_last_error) and do not move MLX_ABI_VERSION.
 *
 * The record: y[nt][n], float64 (MLX_DTYPE_F64) or float32 (MLX_DTYPE_F32), C-contiguous, time
 * leading, n = every other axis flattened.  float32 is widened in registers (exact); every output
 * is float64, as numpy promotes in polyfit / dot.  The time axis is cut into windows whose length
 * depends on nt alone; the windows' partial sums go to the workspace and are combined in ascending
 * window order by a second kernel: no float atomics, results are bit-identical from run to run and
 * do not depend on how a caller splits the cells between calls.
 */
#ifndef MOMLEVEL_TREND_H
#define MOMLEVEL_TREND_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLX_TREND_MAX_TERMS 8 /* most terms (K) of a projected model */

/* mlx_time_apply's mode.  x[t] is the numeric time axis, M[k][t] the model matrix. */
#define MLX_APPLY_REMOVE      0 /* out = y - (slope * x[t] + intercept)     trend.py:190-202 */
#define MLX_APPLY_CORRECT     1 /* out = y - slope * x[t]                   mode="correct"   */
#define MLX_APPLY_TREND       2 /* out = slope * x[t]            broadcast_trend, trend.py:105 */
#define MLX_APPLY_TREND_ANOM  3 /* out = slope * x[t] - slope * x[0]        trend.py:108-110 */
#define MLX_APPLY_MODEL_RESID 4 /* out = y - sum_k M[k][t] * c[k]           trend.py:431, :532 */
#define MLX_APPLY_MODEL       5 /* out = sum_k M[k][t] * c[k]               trend.py:430, :529 */

/* Bytes of workspace mlx_time_linfit (nterms = 5) or mlx_time_project (nterms = K) needs for a
 * record of nt steps and n cells; 0 for arguments the entry points would refuse. */
size_t mlx_time_fit_workspace_bytes(int64_t nt, int64_t n, int nterms);

/* NaN-skipping straight-line fit per cell (numpy.polyfit(x, y, 1) on the valid steps of each
 * cell; trend.py:252).  xt[nt] = (x - xmean) / s with xmean the mean of the WHOLE axis and
 * s = max|x - xmean| (1 if that is 0), float64, on the device.  Per cell, over its valid steps:
 *   m = (n Sxy - Sx Sy) / (n Sxx - Sx^2),  slope = m / s,  intercept = (Sy - m Sx) / n - slope * xmean.
 * A cell with fewer than 2 valid steps (land: none) or a zero denominator gets canonical NaN in
 * both outputs -- numpy's lstsq would give a minimum-norm answer and a RankWarning there.
 * slope, intercept: (n) float64.  workspace: 16-byte aligned. */
int mlx_time_linfit(const void *y, int dtype, const double *xt, int64_t nt, int64_t n, double s,
                    double xmean, double *slope, double *intercept, void *workspace,
                    size_t workspace_bytes, void *stream);

/* coef[k][cell] = sum_t P[t][k] * y[t][cell], t ascending: the reference's pmodel.dot(ts)
 * (trend.py:428, :526).  P: (nt, K) float64 on the device, 1 <= K <= MLX_TREND_MAX_TERMS.  NaN
 * PROPAGATES: one NaN step makes all K coefficients of that cell NaN, as numpy's dot does.
 * coef: (K, n) float64. */
int mlx_time_project(const void *y, int dtype, const double *P, int K, int64_t nt, int64_t n,
                     double *coef, void *workspace, size_t workspace_bytes, void *stream);

/* The elementwise pass (MLX_APPLY_*).  Straight-line modes: xm = x (nt), a = slope (n),
 * b = intercept (n; MLX_APPLY_REMOVE only), K ignored; the reference's operator order, no
 * contraction: bit-identical to numpy given the same slope and intercept.  Model modes: xm = M
 * (K, nt), a = coef (K, n), b ignored; the sum runs over k ascending.  y may be NULL in the modes
 * that do not read it (TREND, TREND_ANOM, MODEL).  out: (nt, n) float64. */
int mlx_time_apply(const void *y, int dtype, int mode, const double *xm, const double *a,
                   const double *b, int K, int64_t nt, int64_t n, double *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MOMLEVEL_TREND_H */
