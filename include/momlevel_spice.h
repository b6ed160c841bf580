/*
 * momlevel_spice.h -- seawater spiciness after Flament (2002), in libmomlevel_hip.so (gfx950): one
 * pointwise map of (theta, S) to pi.
 *
 * It replaces the array work of momlevel.spice.flament.spice (src/momlevel/spice/flament.py:43-95),
 * which momlevel.derived.calc_spice (src/momlevel/derived.py:669-711) applies to thetao and so: six
 * powers of theta and five of S - 35 stacked, tiled to (n, 6, 5), multiplied by the coefficient
 * table and summed.  Here a cell is 29 fused multiply-adds and one subtraction in registers:
 *
 *     s    = S - 35.0
 *     q_k  = ((((b[5][k] theta + b[4][k]) theta + b[3][k]) theta + b[2][k]) theta + b[1][k]) theta
 *            + b[0][k]                                              for k = 0..4
 *     pi   = (((q_4 s + q_3) s + q_2) s + q_1) s + q_0
 *
 * every "x y + z" one fma (one rounding), whatever contraction flags the library is compiled with.
 * b is the published table of P. Flament, 2002: A state variable for characterizing water masses
 * and their diffusive stability: spiciness.  Progress in Oceanography 54, 493-501; b[0][0] = 0
 * stays a term.
 *
 * A header of its own, as include/momlevel_trend.h, momlevel_clim.h and momlevel_gauge.h: the entry
 * point has no host build.  It lives in the same library, follows the same conventions
 * (momlevel_hip.h, "Conventions": int status, MLX_E_* argument errors before any HIP call,
 * caller-owned device buffers, the caller's stream last, text through mlx_last_error) and does not
 * move MLX_ABI_VERSION.
 *
 * The contract:
 *   - theta and S are float64 or float32, each on its own; a float32 value is widened exactly and
 *     ALL arithmetic is float64.  The result is float64 for every combination, the dtype numpy
 *     gives the reference.  (numpy computes the powers of float32 operands in float32; the kernel
 *     does not restate that -- the result is gated by a bound, not by bits: DESIGN.md 3.11.)
 *   - the value of a cell depends on its two operands only: not on its position, on n, on the
 *     alignment of the pointers or on the vector path the call took;
 *   - a NaN in either operand gives NaN;
 *   - INFINITE OPERANDS ARE OUTSIDE THE CONTRACT (the terms become infinities of both
 *     signs; the reference's flat sum and the nested form need not agree on what is left);
 *   - no workspace, no atomics: two runs are bit-identical.
 */
#ifndef MOMLEVEL_SPICE_H
#define MOMLEVEL_SPICE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* pi[i] = sum_{j=0..5} sum_{k=0..4} b[j][k] * theta[i]^j * (so[i] - 35)^k      flament.py:82-90
 *
 * theta, so: (n) on the device, `theta_dtype` / `so_dtype` each MLX_DTYPE_F64 or MLX_DTYPE_F32,
 * independently; out: (n) float64 on the device.  Pointers need the natural alignment of their
 * element type only: ranges that cannot be brought to 16-byte alignment together are evaluated
 * cell by cell, with the same bits.  n == 0 returns 0 without a launch (pointers are not looked
 * at).
 *
 * Refused before any HIP call: an unknown dtype (MLX_E_ENUM); n < 0 or n > 2^38 (MLX_E_SHAPE);
 * theta, so or out NULL with n > 0 (MLX_E_NULL); theta / so not element-aligned, out not 8-byte
 * aligned (MLX_E_ALIGN). */
int mlx_spice_map(const void *theta, int theta_dtype, const void *so, int so_dtype,
                  int64_t n, double *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MOMLEVEL_SPICE_H */
