/*
 * momlevel_filter.h -- the time filter of libmomlevel_hip.so (gfx950): a banded linear operator
 * along the time axis of a (time, cells) record,
 *
 *     out[t] = sum_k w[t, k] * y[t - lead + k],   k = 0 .. W-1,
 *
 * NaN-aware, with one weight row for every step or one row per step.  Rolling means and sums,
 * Lanczos low-pass filters, arbitrary FIR weights and running least-squares slopes are this
 * operator with different weight tables made on the host (momlevel_amd/filters.py).
 *
 * EXTENSION: momlevel has no such function.
 *
 * A header of its own, as include/momlevel_clim.h: the entry point has no host build.  It lives in
 * the same library, follows the same conventions (momlevel_hip.h, "Conventions": int status,
 * MLX_E_* argument errors before any HIP call, caller-owned device buffers, the caller's stream
 * last, text through mlx_last_error) and does not move MLX_ABI_VERSION.
 *
 * The arithmetic contract (tests/filter_numpy.py restates it in numpy; float64 results agree with
 * it bit for bit):
 *   - the window of output t is the steps s_k = t - lead + k, k = 0 .. W-1;
 *   - a step is VALID when it lies inside [0, nt) and its value is not NaN;
 *   - per cell and output step, in float64, k ascending, sequentially: no tree, no atomics and no
 *     running add / subtract across outputs.  Every output is summed afresh, so results depend
 *     neither on the launch geometry nor on how a caller blocks the cells between calls;
 *   - acc starts at -0.0, wsum and cnt at +0.0 (0), and for each k
 *         acc  += valid ? w[k] * y : 0.0      (the product is rounded, then the add: no FMA)
 *         wsum += valid ? w[k]     : 0.0
 *         cnt  += valid
 *   - result: canonical NaN when cnt < min_count; otherwise acc / wsum with MLX_FILTER_NORMALISE,
 *     else acc.  A NaN that the arithmetic itself gives (inf - inf, 0 / 0) is stored canonical.
 *   - min_count == W therefore means "any NaN or any step outside the record gives NaN".
 * float32 records are widened in registers (exact); a float32 result is the float64 result rounded
 * ONCE, in the store.
 */
#ifndef MOMLEVEL_FILTER_H
#define MOMLEVEL_FILTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mlx_filter_apply's flags */
#define MLX_FILTER_NORMALISE 1 /* divide by the sum of the weights of the valid steps */

/* Output steps a lane sums together from one pass over W + tile - 1 rows (the tile along time):
 * output blocks start at multiples of it.  The results do not depend on it. */
int64_t mlx_filter_tile(void);

/* The window lengths at which the kernel's walk over a window changes: i = 0, 1, ... gives them in
 * ascending order, 0 past the last.  Below edge 0 every row of a tile's pass serves only some of
 * the tile's outputs; from edge 0 on there are rows that serve all of them; from edge 1 on those
 * rows are loaded in batches. */
int64_t mlx_filter_window_edge(int i);

/* Consecutive time tiles one block walks in the launch of an (nt, n) record whose lanes hold
 * cells_per_lane cells (4, 2 or 1; the widest that divides n and that the alignment of y and out
 * allows -- see mlx_filter_apply): ceil(ceil(nt / tile) / gy), where gy, the blocks along time, is
 * cut down once the launch has enough blocks without them.  1 for short or narrow records.  Host
 * arithmetic only, the rule the launch itself goes by; the results do not depend on it.  0 for
 * extents mlx_filter_apply refuses, a cells_per_lane that is not 1, 2 or 4, or one that does not
 * divide n. */
int64_t mlx_filter_tiles_per_block(int64_t nt, int64_t n, int cells_per_lane);

/* y: (nt, n) C-contiguous, MLX_DTYPE_F64 or MLX_DTYPE_F32 (dtype), on the device.
 * w: float64 on the device; w_stride == 0: one row (W) for every step; w_stride == W: a table
 * (nt, W), row t for output t.  1 <= W <= nt, 0 <= lead < W, 1 <= min_count <= W.
 * out: (nt, n), MLX_DTYPE_F64 or MLX_DTYPE_F32 (out_dtype); must not overlap y.
 *
 * Cells move in packs of 16 bytes of y, narrowed to what n and the two base pointers allow
 * (float64 2 / 1 cells, float32 4 / 2 / 1).
 *
 * Refused before any HIP call: a NULL operand (MLX_E_NULL); nt or n <= 0, nt >= 2^30, n > 2^38,
 * nt * n not addressable, W outside [1, nt], lead outside [0, W), min_count outside [1, W],
 * w_stride not 0 or W (MLX_E_SHAPE); an unknown dtype, out_dtype or flag (MLX_E_ENUM); y / out not
 * element-aligned, w not 8-byte aligned (MLX_E_ALIGN). */
int mlx_filter_apply(const void *y, int dtype, const double *w, int64_t W, int64_t w_stride,
                    int64_t lead, int64_t min_count, int flags, int64_t nt, int64_t n, void *out,
                    int out_dtype, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MOMLEVEL_FILTER_H */
