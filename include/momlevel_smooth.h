/*
 * momlevel_smooth.h -- the horizontal filter of libmomlevel_hip.so (gfx950): a separable,
 * normalised, mask-aware, area-weighted convolution over the two trailing dims of a (nrec, ny, nx)
 * record.  Box and Gaussian smoothers, a fixed length scale on a converging grid (one row of x
 * weights per source row) and the high-pass residual are this operator with different weight tables
 * made on the host (momlevel_amd/spatial.py).
 *
 * EXTENSION: momlevel has no such function.
 *
 * A header of its own, as include/momlevel_filter.h: the entry point has no host build.  It lives in
 * the same library, follows the same conventions (momlevel_hip.h, "Conventions": int status,
 * MLX_E_* argument errors before any HIP call, caller-owned device buffers, the caller's stream
 * last, text through mlx_last_error) and does not move MLX_ABI_VERSION.
 *
 * The arithmetic contract (tests/smooth_numpy.py restates it in numpy; results agree with it bit
 * for bit).  All arithmetic is float64 on exactly widened operands (v64, a64); every product and
 * every add is rounded on its own (no FMA):
 *
 *     valid[r,c] = !isnan(v[rec,r,c]) && !isnan(area[r,c]) && area[r,c] > 0
 *     m[r,c]     = a64[r,c] * v64[rec,r,c]
 *
 *   row pass, source row r, output column i, k = 0 .. Wx-1 ascending, accumulators start at +0.0,
 *   X_r the weights of source row r (wx, or row r of the table):
 *     c = i - lead_x + k;   periodic_x: c mod nx;   otherwise a c outside [0, nx) is not valid
 *     Rn += valid ? X_r[k] * m[r,c]   : 0.0
 *     Rd += valid ? X_r[k] * a64[r,c] : 0.0
 *     Rc += valid                                   (integer)
 *
 *   column pass, output (j, i), l = 0 .. Wy-1 ascending, rows j - lead_y + l outside [0, ny) are
 *   skipped (y is never periodic), accumulators start at +0.0:
 *     num += wy[l] * Rn[j-lead_y+l, i];   den += wy[l] * Rd[..];   cnt += Rc[..]
 *
 *     smooth = num / den        (IEEE; a NaN that the arithmetic gives is stored canonical)
 *     out    = canonical NaN  when cnt < min_count, or when the centre cell (j, i) is not valid and
 *                             MLX_SMOOTH_FILL is not set
 *            = v64 - smooth   with MLX_SMOOTH_RESIDUAL (NaN at a centre that is not valid, with or
 *                             without MLX_SMOOTH_FILL)
 *            = smooth         otherwise
 *
 * Rn[r, i] is a function of (rec, r, i) only: a value recomputed in a neighbouring tile's halo has
 * the same bits, so a cell's result depends neither on the tiling, on nrec, on the records around
 * it, on the alignment of the pointers nor on the path taken.  No atomics and no running sums: two
 * runs are bit-identical.  A float32 result is the float64 result rounded once, in the store.  num
 * and den go through the same operations, so a record of ones gives exactly 1.0 wherever it is not
 * NaN.
 *
 * Non-finite weights and infinite areas are outside the contract (the Python layer refuses them);
 * negative areas carry no weight here (area > 0) and are refused by the Python layer.
 *
 * NOT BUILT: the tripolar north fold (the north and south edges are closed) and tiles spread over
 * several ranks (they need a halo exchange).
 */
#ifndef MOMLEVEL_SMOOTH_H
#define MOMLEVEL_SMOOTH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mlx_smooth_apply's flags */
#define MLX_SMOOTH_FILL 1     /* a centre that is not valid still gets the smooth of its window */
#define MLX_SMOOTH_RESIDUAL 2 /* out = v - smooth: the high-pass form */

/* The tiled path: a block owns mlx_smooth_tile_h() rows by mlx_smooth_tile_w(dtype) columns of
 * output cells (dtype: the record's, MLX_DTYPE_F64 or MLX_DTYPE_F32; 0 for any other value) and
 * walks mlx_smooth_record_window() records while it holds its part of `area` and of the weights in
 * LDS.  It takes windows of up to mlx_smooth_max_window() cells each way.  The results do not
 * depend on any of them. */
int64_t mlx_smooth_tile_h(void);
int64_t mlx_smooth_tile_w(int dtype);
int64_t mlx_smooth_max_window(void);
int64_t mlx_smooth_record_window(void);

/* Block rows along the records (gridDim.y) of a call that goes cell by cell over nrec records:
 * min(nrec, cap).  Up to the cap a block row carries one record; past it a row goes on to the
 * record cap rows further, and so on.  Host arithmetic only, the rule the launch itself goes by; a
 * record's bits do not depend on it.  0 for nrec <= 0 or nrec > 2^38. */
int mlx_smooth_record_rows(int64_t nrec);

/* 1 when a call of these extents takes the tiled path, given v and out on 16-byte boundaries:
 * Wx, Wy <= mlx_smooth_max_window(), nx a multiple of 4, ny >= mlx_smooth_tile_h() and nx >= the
 * tile's width.  0 otherwise, and for extents that mlx_smooth_apply refuses (ny or nx < 1,
 * ny * nx > 2^38, Wx outside [1, nx], Wy outside [1, ny]).  Host arithmetic only, the rule
 * mlx_smooth_apply itself goes by. */
int mlx_smooth_tiled(int64_t Wx, int64_t Wy, int64_t ny, int64_t nx);

/* v: (nrec, ny, nx) C-contiguous, MLX_DTYPE_F64 or MLX_DTYPE_F32 (dtype); area: (ny, nx),
 * MLX_DTYPE_F64 or MLX_DTYPE_F32 (area_dtype); wx: float64, wx_stride == 0: Wx weights for every
 * source row, wx_stride == Wx: a table (ny, Wx), row r for source row r; wy: Wy float64 weights;
 * periodic_x: 0 or 1; out: (nrec, ny, nx), MLX_DTYPE_F64 or MLX_DTYPE_F32 (out_dtype).  All on the
 * device.
 *
 * The tiled path (rows in 16-byte packs, the row pass staged through LDS) takes calls with
 * Wx, Wy <= mlx_smooth_max_window(), nx a multiple of 4, a plane of at least one tile each way and
 * v and out 16-byte aligned; every other call is evaluated cell by cell from global memory, with
 * the same bits.
 *
 * Refused before any HIP call: an unknown dtype, area_dtype, out_dtype or flag, a periodic_x that
 * is not 0 or 1 (MLX_E_ENUM); nrec < 0, ny or nx < 1, nrec * ny * nx > 2^38, Wx outside [1, nx],
 * Wy outside [1, ny], lead_x outside [0, Wx), lead_y outside [0, Wy), min_count outside
 * [1, Wx * Wy], wx_stride not 0 or Wx (MLX_E_SHAPE); a NULL operand (MLX_E_NULL); v / area / out
 * not element-aligned, wx / wy not 8-byte aligned (MLX_E_ALIGN); an out that overlaps an operand
 * (MLX_E_SHAPE).  nrec == 0 returns 0 without a launch. */
int mlx_smooth_apply(const void *v, int dtype, const void *area, int area_dtype, const double *wx,
                     int64_t Wx, int64_t wx_stride, int64_t lead_x, const double *wy, int64_t Wy,
                     int64_t lead_y, int periodic_x, int64_t min_count, int flags, int64_t nrec,
                     int64_t ny, int64_t nx, void *out, int out_dtype, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MOMLEVEL_SMOOTH_H */
