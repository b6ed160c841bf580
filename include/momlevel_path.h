/*
 * momlevel_path.h -- which kernel shape a call of the pointwise EOS entry points of
 * libmomlevel_hip.so takes.  Host arithmetic only: no HIP call, no device, no pointer is read.
 *
 * mlx_eos_map / mlx_inverse_barometer choose between a generic kernel (one cell a lane, the
 * function, EOS and pressure mode run-time arguments) and fast ones (16-byte packs, the function a
 * template argument; for the density also with a (z,y,x) pressure field), and cut the time axis
 * into launches.  mlx_eos_map_promote chooses how many cells a lane takes.  The two queries below
 * are THE rule: the launchers call the same functions, so what a query answers is what a call with
 * those arguments launches.  Tests size their cases from the answers and assert the path from them.
 *
 * A header of its own, as include/momlevel_filter.h: the queries have no host build.  They live in
 * the same library, follow the same conventions (momlevel_hip.h, "Conventions") and do not move
 * MLX_ABI_VERSION.  Results never depend on the path: every shape gives the same bits.
 */
#ifndef MOMLEVEL_PATH_H
#define MOMLEVEL_PATH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* what mlx_path_eos_map returns */
#define MLX_PATH_GENERIC  0 /* one cell a lane, several cells a thread */
#define MLX_PATH_FAST     1 /* 16-byte packs, z-profile pressure */
#define MLX_PATH_FAST_P3D 2 /* 16-byte packs, the pressure a (z,y,x) field read in packs too */

/* bits of `aligned16`: the operand's base address is a multiple of 16 bytes */
#define MLX_PATH_ALIGNED_T   1
#define MLX_PATH_ALIGNED_S   2
#define MLX_PATH_ALIGNED_OUT 4
#define MLX_PATH_ALIGNED_P   8
#define MLX_PATH_ALIGNED_ALL 15

/* The kernel shape of mlx_eos_map(T, S, dtype, p, p_mode, eos, func, nt, nz, plane, sT, sS, flags,
 * out) -- func MLX_FUNC_IBH: of mlx_inverse_barometer -- for operands whose 16-byte alignment is
 * `aligned16`.  Returns MLX_PATH_*; *cells_per_block (when not NULL) receives the cells of one z
 * level a block covers, *launch_steps the time steps one launch takes (a call of more is cut into
 * launches of that many).
 *
 * Fast needs: the Wright EOS; a z-profile pressure, or -- the density only -- a (z,y,x) field that
 * is 16-byte aligned; plane, sT and sS whole packs (2 cells of float64, 4 of float32); T, S and out
 * 16-byte aligned; float64 fields unless the function is the density; never the inverse barometer.
 *
 * Refused (MLX_E_ENUM / MLX_E_SHAPE, text through mlx_last_error): what mlx_eos_map refuses of
 * these arguments -- an unknown dtype, p_mode, eos, func or flag, theta / salinity of different
 * dtypes, MLX_FLAG_FMA with anything but the density, plane <= 0, a negative stride -- and bits of
 * aligned16 outside MLX_PATH_ALIGNED_ALL. */
int mlx_path_eos_map(int dtype, int p_mode, int eos, int func, int64_t plane, int64_t sT,
                     int64_t sS, int flags, int aligned16, int64_t *cells_per_block,
                     int64_t *launch_steps);

/* The cells a lane takes (4, 2 or 1) in mlx_eos_map_promote for operands of kinds kind_T, kind_S,
 * kind_p (MLX_KIND_*); `aligned16` the MLX_PATH_ALIGNED_* bits of the result and of the operands:
 * set for an array of n elements whose base is a multiple of 16 bytes and for a one-element array
 * (stride 0: read as a scalar wherever it lies); the bit of a python float or of an operand that
 * is not read is ignored.  *out_kind (when not NULL) receives the kind of the result, MLX_KIND_F32
 * or MLX_KIND_F64.  4 when float32 arrays and python floats give a float32 result, 2 as soon as a
 * float64 array takes part or the result is float64, 1 when an array or the result lacks the
 * alignment.  The linear EOS reads the pressure for MLX_FUNC_IBH and MLX_FUNC_DENSITY_REF only:
 * otherwise kind_p and its bit take no part.  Refused (MLX_E_ENUM): an unknown kind, eos or func,
 * MLX_FUNC_DENSITY_REF with the Wright EOS, bits outside MLX_PATH_ALIGNED_ALL. */
int mlx_path_eos_promote(int kind_T, int kind_S, int kind_p, int eos, int func, int aligned16,
                         int *out_kind);

#ifdef __cplusplus
}
#endif
#endif /* MOMLEVEL_PATH_H */
