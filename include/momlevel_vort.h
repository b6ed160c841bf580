/*
 * momlevel_vort.h -- relative vorticity, potential vorticity and the Rossby radius on MOM6's
 * staggered (C) grid, in libmomlevel_hip.so (gfx950): two horizontal stencils over
 * (record, y, x) fields and one broadcast division.
 *
 * They replace the array work of momlevel.derived.calc_rel_vort (src/momlevel/derived.py:187-246),
 * calc_pv (:489-565) and calc_rossby_rd (:568-594), which the reference evaluates as a chain of
 * xgcm / xarray passes with padded temporaries (grid.diff and grid.interp with boundary="fill"):
 *
 *     fu = u * dx            on (yh, xq)            fv = v * dy            on (yq, xh)
 *     zeta[j,i] = ( -(fu[j+1,i] - fu[j,i]) + (fv[j,i+1] - fv[j,i]) ) / area[j,i]        on (yq, xq)
 *
 *     ax[j,i]   = 0.5 * (n2[j,i] + n2[j,i+1])       n2c[j,i] = 0.5 * (ax[j,i] + ax[j+1,i])
 *     pv[j,i]   = (zeta[j,i] + f[j,i]) * (n2c[j,i] / gravity)         (n2c = n2 without interp)
 *     "cm":       pv = | (pv / 100) * 1e14 |
 *
 *     rd[o,p,i] = c[o,p,i] / |f[p]|
 *
 * THE GRIDS.  `ny`, `nx` are always the extents of the CORNER (yq, xq) plane, the plane of zeta.
 *   - non-symmetric (symmetric = 0; xgcm "center -> right"): centre and corner dims have equal
 *     lengths; the neighbour of index k is k + 1 and the element past the end is the literal 0.0;
 *   - symmetric (symmetric = 1; "center -> outer"): the corner dims are one longer than the centre
 *     dims, `out[k] = f[k] - f[k-1]` for k = 0..n with both out-of-range elements 0.0, and the
 *     average is built the same way.
 * A term that lies past the edge IS the literal 0.0 (the subtraction / addition is still made);
 * everywhere else a NaN in any operand of a cell gives NaN.
 *
 * ARITHMETIC.  Every operation above is rounded on its own (no contraction) in the dtype numpy
 * would use, float32 operands widened exactly where numpy promotes: the results are BIT-IDENTICAL
 * to numpy's operator-for-operator evaluation.  The value of a cell depends on its own operands
 * only: not on nrec, on the tile it fell in, on the alignment of the pointers or on the path the
 * call took.  No workspace, no atomics: two runs are bit-identical.
 *
 * PATHS.  A non-symmetric call whose rows can all be moved in 16-byte packs (nx a multiple of the
 * pack, every pointer aligned for its pack access) walks tiles: a wave owns MLX_VORT_TILE_LANES
 * packs side by side and MLX_VORT_TILE_H rows, holds the current row of fu (of ax) in registers and
 * loads the next one once -- each row of u (of n2) is read once per tile plus one halo row.  Every
 * other call (odd nx, offset pointers, symmetric grids) is evaluated cell by cell, with the same
 * bits.
 *
 * A header of its own, as include/momlevel_spice.h: the entry points have no host build.  They live
 * in the same library, follow the same conventions (momlevel_hip.h, "Conventions": int status,
 * MLX_E_* argument errors before any HIP call, caller-owned device buffers, the caller's stream
 * last, text through mlx_last_error) and do not move MLX_ABI_VERSION.
 */
#ifndef MOMLEVEL_VORT_H
#define MOMLEVEL_VORT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLX_VORT_UNITS_M 0
#define MLX_VORT_UNITS_CM 1

/* the tiling of the packed path: a wave's tile is MLX_VORT_TILE_LANES packs of 16 bytes of the
 * arithmetic dtype wide (128 float64 / 256 float32 cells) and MLX_VORT_TILE_H rows high; a block
 * stacks MLX_VORT_TILE_BANDS such tiles in y */
#define MLX_VORT_TILE_LANES 64
#define MLX_VORT_TILE_H 16
#define MLX_VORT_TILE_BANDS 4

/* cells across one tile for arithmetic in `arith_dtype` (MLX_DTYPE_F64: 128, MLX_DTYPE_F32: 256);
 * 0 for any other value */
int64_t mlx_vort_tile_width(int arith_dtype);

/* Records one launch of the packed path takes for a corner plane of (ny, nx) and arithmetic in
 * `arith_dtype`: a call over more records is cut into launches of that many, each at its own
 * offset of whole planes into the fields and the result.  0 where the shape sends the plane cell
 * by cell (nx not a multiple of the pack, or a plane of more tiles than one grid holds), for
 * ny or nx < 1 or ny * nx > 2^38, and for any other dtype.  (A symmetric grid or a pointer that is
 * not aligned for its pack access also goes cell by cell; the query cannot see those.)  Host
 * arithmetic only, the rule the launches themselves go by; a cell's bits do not depend on it. */
int64_t mlx_vort_records_per_launch(int64_t ny, int64_t nx, int arith_dtype);

/* zeta = ( -diff_y(u * dx) + diff_x(v * dy) ) / area                        derived.py:232-239
 *
 * ny, nx: the extents of the corner plane.  With s = symmetric (0 or 1):
 *   u:    (nrec, ny - s, nx)   v:  (nrec, ny, nx - s)         `field_dtype`, both of them
 *   dx:   (ny - s, nx)         dy: (ny, nx - s)        area: (ny, nx)      `metric_dtype`, all three
 *   out:  (nrec, ny, nx)       float32 when field_dtype and metric_dtype are both MLX_DTYPE_F32,
 *                              float64 otherwise (numpy's promotion; that is the arithmetic too)
 * all contiguous on the device.  nrec == 0 returns 0 without a launch.
 *
 * Refused before any HIP call: a dtype that is not MLX_DTYPE_F64 / MLX_DTYPE_F32, symmetric not
 * 0 / 1 (MLX_E_ENUM); nrec < 0, ny or nx < 1 + symmetric, nrec * ny * nx > 2^38 (MLX_E_SHAPE); a
 * NULL pointer with nrec > 0 (MLX_E_NULL); a pointer not aligned to its element (MLX_E_ALIGN). */
int mlx_vort_rel_vort(const void *u, const void *v, int field_dtype, const void *dx,
                      const void *dy, const void *area, int metric_dtype, int64_t nrec,
                      int64_t ny, int64_t nx, int symmetric, void *out, void *stream);

/* pv = (zeta + coriolis) * (n2c / gravity), optionally | (pv / 100) * 1e14 |    derived.py:538-556
 *
 *   zeta:     (nrec, ny, nx)  `zeta_dtype`        coriolis: (ny, nx)  `coriolis_dtype`
 *   n2:       `n2_dtype`; (nrec, ny, nx) with interp = 0, (nrec, ny - s, nx - s) with interp = 1:
 *             then n2c is n2 averaged along x and then along y, each step 0.5 * (a + b) with the
 *             padding above, fused into the pass (no interpolated N^2 is written anywhere)
 *   out:      (nrec, ny, nx), float32 when all three dtypes are MLX_DTYPE_F32, float64 otherwise
 * zeta + coriolis is formed in the promotion of those two, the average and n2c / gravity in n2's
 * dtype (`gravity` is rounded to it: a python float is weak), the product and the three "cm"
 * operations in the promotion of both sides.  `symmetric` is not looked at when interp = 0.
 *
 * Refused before any HIP call: as above, and interp not 0 / 1 or units not MLX_VORT_UNITS_M /
 * MLX_VORT_UNITS_CM (MLX_E_ENUM). */
int mlx_vort_pv(const void *zeta, int zeta_dtype, const void *coriolis, int coriolis_dtype,
                const void *n2, int n2_dtype, int64_t nrec, int64_t ny, int64_t nx, int interp,
                int symmetric, double gravity, int units, void *out, void *stream);

/* out[o,p,i] = c[o,p,i] / |f[p]|  (IEEE division: c / 0 is +-inf, 0 / 0 and NaN are NaN)
 *                                                                            derived.py:588
 *   c:   (outer, plane, inner)  `c_dtype`        f: (plane)  `f_dtype`
 *   out: (outer, plane, inner), float32 when both dtypes are MLX_DTYPE_F32, float64 otherwise
 * Refused before any HIP call: as above; outer, plane or inner < 0 or their product > 2^38
 * (MLX_E_SHAPE).  A zero extent returns 0 without a launch. */
int mlx_vort_rossby(const void *c, int c_dtype, const void *f, int f_dtype, int64_t outer,
                    int64_t plane, int64_t inner, void *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MOMLEVEL_VORT_H */
