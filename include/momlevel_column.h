/*
 * momlevel_column.h -- the depth of the first crossing along z of a (record, z, plane) field: mixed
 * layer depths, isotherm and isopycnal depths, in libmomlevel_hip.so (gfx950).
 *
 * AN EXTENSION: momlevel has no such function.  It is what a user of its theta / S fields asks
 * next ("how deep is the mixed layer, the 20 degC isotherm, sigma0 = 27?"); the specification is
 * the numpy restatement tests/column_numpy.py.
 *
 * ONE OPERATOR, per record r, cell c and target j.  The column value x[k] is a float64:
 *
 *   FIELD source (b == NULL): a[r, k, c], float32 widened exactly.
 *   SIGMA source (b != NULL): the potential density of (theta, S) = (a[r, k, c], b[r, k, c]) at the
 *     ONE scalar pressure p_ref, with the exact operator-for-operator density of csrc/eos_device.hpp
 *     (Wright or linear, ExactOps) IN FLOAT64 ON EXACTLY WIDENED OPERANDS, FOR EVERY INPUT DTYPE.
 *     theta and S carry their own dtype each.  A deliberate exception, of the kind mlx_spice_map
 *     is: numpy's calc_pdens on float32 fields evaluates the polynomial in float32, and a float32
 *     rho near 1027 kg m-3 has an ulp of 2^-13 = 1.2e-4 kg m-3 -- 0.4 % of a 0.03 threshold, 1.2 %
 *     of a 0.01 one: too coarse to search in.  For float64 fields x is bit for bit mlx_eos_map's
 *     density at p_ref, for float32 fields mlx_eos_map's density of the widened copies.
 *
 * With z[nz] the strictly increasing level depths, kref the reference level, v[j] the targets:
 *
 *   1. x[0] is NaN: land.  Every out[r, j, c] is the canonical NaN.
 *   2. x_ref = x[kref].  NaN: the column is shallower than the reference level; every target gets
 *      the miss value of step 6.
 *   3. RISE:   tgt_j = relative ? x_ref + v_j : v_j ; a hit is x >= tgt_j
 *      FALL:   tgt_j = relative ? x_ref - v_j : v_j ; a hit is x <= tgt_j
 *      DEPART: relative only; a hit is |x - x_ref| >= v_j, and at the hit
 *              tgt_j = x > x_ref ? x_ref + v_j : x_ref - v_j
 *      Relative targets need v_j > 0.
 *   4. x[kref] itself is a hit: the surface outcrops, the result is NaN.
 *   5. Scan k = kref .. nz-2.  A NaN x[k+1] is the sea floor and ends the scan.  The FIRST k for
 *      which x[k+1] is a hit gives
 *
 *          out = z[k] + ((tgt_j - x[k]) / (x[k+1] - x[k])) * (z[k+1] - z[k])
 *
 *      every operator one IEEE float64 operation in exactly this parenthesisation, no fma, the
 *      division correctly rounded.  (The denominator is not zero: x[k] is not a hit, x[k+1] is.)
 *      The first crossing wins, also in a column that un-crosses and crosses again deeper.
 *   6. No crossing: the miss value.  MLX_COLUMN_MISS_NAN: NaN.  MLX_COLUMN_MISS_FLOOR: floor[c]
 *      when floor is given (a NaN there included), else z[klast], klast the deepest level of the
 *      scan with a value: the last level before the scan ended.  For the column of step 2, whose
 *      scan never began, klast is the deepest level above kref with no NaN at or above it.
 *
 * A result depends on its own column and target only: not on nrec, not on the other targets of the
 * launch, not on pointer alignment, not on whether 16-byte packs or single cells were loaded.
 *
 * THE KERNEL stops reading a column when all its targets are decided or it met the sea floor, and
 * a wave leaves the z loop when all of its 64 lanes have: a shallow mixed layer costs a few levels
 * of a 75-level column.  A lane that is still searching is never cut short by its neighbours.
 *
 * A header of its own, as include/momlevel_layer.h: the entry points have no host build.  They live
 * in the same library, follow the same conventions (momlevel_hip.h, "Conventions": int status,
 * MLX_E_* argument errors before any HIP call, caller-owned device buffers, the caller's stream
 * last, text through mlx_last_error) and do not move MLX_ABI_VERSION.
 */
#ifndef MOMLEVEL_COLUMN_H
#define MOMLEVEL_COLUMN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* targets per launch: their state lives in registers */
#define MLX_COLUMN_MAX_TARGETS 8

/* mode */
#define MLX_COLUMN_RISE 0
#define MLX_COLUMN_FALL 1
#define MLX_COLUMN_DEPART 2

/* miss */
#define MLX_COLUMN_MISS_NAN 0
#define MLX_COLUMN_MISS_FLOOR 1

/* Cells of the plane one block of mlx_column_crossing covers: 256 threads of one 16-byte pack each
 * -- 2 cells when a float64 field takes part, 4 when every field is float32 -- or, `generic` != 0,
 * of one cell each.  `has_b` == 0: FIELD source, b_dtype is not looked at.  Host arithmetic only,
 * the rule the launch itself goes by.  0 for a dtype that is not MLX_DTYPE_F64 / MLX_DTYPE_F32. */
int64_t mlx_column_block_cells(int a_dtype, int has_b, int b_dtype, int generic);

/* Block rows along the records (gridDim.y) of a call over nrec records: min(nrec, cap).  Up to
 * the cap a block row carries one record; past it a row goes on to the record cap rows further,
 * and so on.  Host arithmetic only, the rule the launch itself goes by; a record's bits do not
 * depend on it.  0 for nrec <= 0 or nrec > 2^38. */
int mlx_column_record_rows(int64_t nrec);

/* out[r, j, c] as defined above.
 *
 *   a:       (nrec, nz, plane)  `a_dtype` (MLX_DTYPE_F64 | MLX_DTYPE_F32), device: the field, or theta
 *   b:       NULL (FIELD source), or S: (nrec, nz, plane) `b_dtype`, device (SIGMA source)
 *   eos:     MLX_EOS_WRIGHT | MLX_EOS_LINEAR; p_ref: the pressure in Pa (SIGMA source only)
 *   z:       (nz) float64 level depths, strictly increasing (the caller's to check), device
 *   kref:    0 <= kref < nz
 *   mode:    MLX_COLUMN_RISE | _FALL | _DEPART;  relative: 0 | 1;  miss: MLX_COLUMN_MISS_NAN | _FLOOR
 *   targets: `ntargets` float64, a HOST array, passed to the kernel by value
 *   floor:   (plane) float64 on the device, or NULL
 *   out:     (nrec, ntargets, plane) float64, device
 * all contiguous.  nrec == 0 or plane == 0 returns 0 without a launch (pointers are not looked at;
 * nothing is written).
 *
 * Refused before any HIP call: a dtype that is not MLX_DTYPE_F64 / MLX_DTYPE_F32 (b_dtype and eos
 * are looked at for b != NULL only), a mode, relative or miss that is none of the above
 * (MLX_E_ENUM); ntargets < 1 or > MLX_COLUMN_MAX_TARGETS, nz < 1, kref outside 0 .. nz-1, nrec or
 * plane < 0, nrec * nz * plane > 2^38 (MLX_E_SHAPE); a, z, targets or out NULL with work to do
 * (MLX_E_NULL); a pointer not aligned to its element (MLX_E_ALIGN); a NaN target, a relative
 * target <= 0, MLX_COLUMN_DEPART without relative (MLX_E_SHAPE). */
int mlx_column_crossing(const void *a, int a_dtype, const void *b, int b_dtype, int eos,
                        double p_ref, int64_t nrec, int64_t nz, int64_t plane, const double *z,
                        int64_t kref, int mode, int relative, int miss, const double *targets,
                        int ntargets, const double *floor, double *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MOMLEVEL_COLUMN_H */
