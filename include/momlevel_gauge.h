/*
 * momlevel_gauge.h -- tide gauges on the model grid, in libmomlevel_hip.so (gfx950): the nearest
 * valid ("wet") grid point of every gauge by great-circle distance, and the gather of the gauges'
 * series out of a (rest, cells) record.
 *
 * It replaces the array work of momlevel.tidegauge.extract_tidegauge (src/momlevel/tidegauge.py:
 * 40-152): util.geolocate_points (src/momlevel/util.py:252-367: a scikit-learn BallTree with the
 * haversine metric, queried with k = 1) and one arr.sel per gauge (tidegauge.py:14-37,148-150).
 * Here the search is a brute-force, deterministic argmin and the extraction is one gather.
 *
 * A header of its own, as include/momlevel_trend.h and include/momlevel_clim.h: the entry points
 * have no host build.  They live in the same library, follow the same conventions (momlevel_hip.h,
 * "Conventions": int status, MLX_E_* argument errors before any HIP call, caller-owned device
 * buffers, the caller's stream last, text through mlx_last_error) and do not move MLX_ABI_VERSION.
 *
 * The search contract:
 *   - a point is VALID iff its mask value equals 1.0 exactly (util.py:327, after the fillna(0) of
 *     tidegauge.py:109: a NaN mask is dry, 0.5 is dry) and its latitude and longitude are finite;
 *     without a mask every point with finite coordinates is valid;
 *   - phi, lam = degrees * (pi / 180) in float64 (numpy.deg2rad); a point's unit vector is
 *     (cos phi cos lam, cos phi sin lam, sin phi).  An invalid point gets (+inf, +inf, +inf): its
 *     squared chord to any gauge is +inf, which never compares below anything;
 *   - per gauge the winner is the valid point with the smallest squared chord
 *         ((gx - ux)^2 + (gy - uy)^2) + (gz - uz)^2
 *     evaluated in float64, in that association, without contraction: the value of a pair does not
 *     depend on tiling, launch geometry or the split of the points;
 *   - TIES GO TO THE LOWEST FLAT INDEX (numpy's argmin; BallTree leaves ties unspecified);
 *   - no float atomics: the points are split over blocks, every block writes its (chord^2, index)
 *     partial, and a second kernel combines the partials of a gauge with the same rule -- smaller
 *     chord, then lower index: a total order, so the winner does not depend on the order in which
 *     the partials meet.  Index and angle are bit-identical for every split;
 *   - the distance is evaluated once, for the winner: the haversine angle in radians
 *         2 asin(min(1, sqrt(sin^2((phi1 - phi2) / 2) + cos phi1 cos phi2 sin^2((lam1 - lam2) / 2))))
 *     with the gauge as point 1 -- the metric of BallTree(metric="haversine").  The caller
 *     multiplies by the earth's radius;
 *   - a gauge with no valid point (or with a non-finite position) gets index -1 and a NaN angle.
 */
#ifndef MOMLEVEL_GAUGE_H
#define MOMLEVEL_GAUGE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* rows of a prepared point table: (MLX_GAUGE_ROWS, n) float64, C-contiguous */
#define MLX_GAUGE_ROW_X   0 /* cos phi cos lam, +inf for an invalid point */
#define MLX_GAUGE_ROW_Y   1 /* cos phi sin lam, +inf for an invalid point */
#define MLX_GAUGE_ROW_Z   2 /* sin phi,         +inf for an invalid point */
#define MLX_GAUGE_ROW_PHI 3 /* latitude in radians  (NaN for an invalid point) */
#define MLX_GAUGE_ROW_LAM 4 /* longitude in radians (NaN for an invalid point) */
#define MLX_GAUGE_ROWS    5

/* One pass over n points.  lat, lon: (n) degrees, `dtype` MLX_DTYPE_F64 or MLX_DTYPE_F32 (widened
 * exactly); mask: (n) of `mask_dtype` (same two codes), or NULL for all ones (mask_dtype is then
 * ignored).  table: (MLX_GAUGE_ROWS, n) float64; valid: (n) uint8, 1 for a valid point, else 0.
 * Gauges are prepared by the same call, without a mask.
 *
 * Refused before any HIP call: lat, lon, table or valid NULL (MLX_E_NULL); n <= 0 or n > 2^38
 * (MLX_E_SHAPE); an unknown dtype (MLX_E_ENUM); lat / lon / mask not element-aligned, table not
 * 8-byte aligned (MLX_E_ALIGN). */
int mlx_gauge_prepare(const void *lat, const void *lon, int dtype, const void *mask, int mask_dtype,
                      int64_t n, double *table, uint8_t *valid, void *stream);

/* The number of parts the n points are cut into for ng gauges: the library's choice when `split`
 * is 0; otherwise n / ceil(n / split) rounded up -- `split` itself whenever it divides n -- kept
 * between n / 2^30 and min(n, 65535).  0 for arguments mlx_gauge_nearest refuses. */
int64_t mlx_gauge_nearest_split(int64_t n, int64_t ng, int64_t split);

/* Bytes of workspace mlx_gauge_nearest needs: 16 per gauge and part.  0 for n or ng <= 0. */
size_t mlx_gauge_nearest_workspace_bytes(int64_t n, int64_t ng, int64_t split);

/* points: the prepared table of the n grid points; gauges: the prepared table of the ng gauges.
 * index: (ng) int64, the flat index of the winner or -1; angle: (ng) float64 radians or NaN.
 * split: as mlx_gauge_nearest_split; the result does not depend on it.  workspace: at least
 * mlx_gauge_nearest_workspace_bytes(n, ng, split) bytes, 16-byte aligned.
 *
 * Refused before any HIP call: points, gauges, index, angle or workspace NULL (MLX_E_NULL); n or
 * ng <= 0, n > 2^38, ng >= 2^31, split < 0 (MLX_E_SHAPE); a pointer not 8-byte aligned
 * (MLX_E_ALIGN); a workspace too small or not 16-byte aligned (MLX_E_WORKSPACE). */
int mlx_gauge_nearest(const double *points, int64_t n, const double *gauges, int64_t ng,
                      int64_t split, int64_t *index, double *angle, void *workspace,
                      size_t workspace_bytes, void *stream);

/* out[g, r] = y[r, index[g]].  y: (nrest, n) C-contiguous, MLX_DTYPE_F64 or MLX_DTYPE_F32, on the
 * device; index: (ng) int64 on the device; out: (ng, nrest), the dtype of y -- each gauge's series
 * is contiguous.  Bits are copied (NaN payloads included).  An index outside [0, n) gives a series
 * of canonical NaN; the kernel never reads outside y.
 *
 * Refused before any HIP call: y, index or out NULL (MLX_E_NULL); nrest, n or ng <= 0, nrest or
 * ng >= 2^31, n > 2^38, nrest * n or ng * nrest not addressable (MLX_E_SHAPE); an unknown dtype
 * (MLX_E_ENUM); y / out not element-aligned, index not 8-byte aligned (MLX_E_ALIGN). */
int mlx_gauge_gather(const void *y, int dtype, const int64_t *index, int64_t nrest, int64_t n,
                     int64_t ng, void *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MOMLEVEL_GAUGE_H */
