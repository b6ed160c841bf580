/*
 * momlevel_layer.h -- depth-layer sums of a (record, z, plane) field: for every record, layer and
 * cell the sum over z of calc_dz(top, bottom) * x, in libmomlevel_hip.so (gfx950).
 *
 * AN EXTENSION: momlevel has no such function.  It is what a user of its steric fields does next
 * ("how much of this rise is in the upper 700 m?"), spelled with the reference's own pieces
 *
 *     dz_l  = momlevel.derived.calc_dz(z_l, z_i, deptho, top=top, bottom=bottom)
 *     eta_l = (-1.0 / rhozero) * (dz_l * delta_rho).sum("z_l")
 *
 * The specification is the numpy restatement tests/layer_numpy.py.  For every record r, layer l
 * and cell c:
 *
 *     acc = +0.0
 *     for z ascending:
 *         w    = calc_dz's arithmetic for (z_i[z], z_i[z+1], depth[c], top[l], bottom[l])
 *         term = w * (double) x[r, z, c]         one IEEE multiply, no fma
 *         if term is not NaN: acc = acc + term   skipna, z ascending
 *     out[r, l, c] = scale * acc ;  canonical NaN where surface != NULL and surface[c] is NaN
 *
 * calc_dz's arithmetic (derived.py:295-318, fraction=False), with d = min(fillna(depth[c], 0),
 * bottom[l]):
 *
 *     w = min(min(max(d - z_i[z], 0), z_i[z+1] - z_i[z]), max(z_i[z+1] - top[l], 0))
 *
 * -- the one __device__ function (csrc/mlx_internal.hpp calc_dz_cell) that mlx_calc_dz and the
 * default dz of mlx_steric_local use.  NOTE what this gives where top and the floor (or bottom) cut
 * the SAME model cell: min(z_i[z+1] - top, d - z_i[z]), not d - top.  Parity with calc_dz is the
 * contract; the kernel does not repair it.
 *
 * THE ORDER OF SUMMATION is z ascending, one sum per (record, layer, cell), owned by one thread: no
 * atomics, no reduction across threads.  Every path gives the same bits -- 16-byte packs where the
 * plane is a whole number of packs and x / out are 16-byte aligned, cell by cell elsewhere -- and
 * the result of a record depends neither on nrec, on the records around it, on the alignment of
 * the pointers nor on which layers share the launch.  A level that does not overlap a layer
 * (z_i[z+1] <= top[l] or z_i[z] >= bottom[l]) is skipped: its terms are +-0 or NaN, which never
 * change a sum that started from +0.0.
 *
 * A header of its own, as include/momlevel_area.h: the entry points have no host build.  They live
 * in the same library, follow the same conventions (momlevel_hip.h, "Conventions": int status,
 * MLX_E_* argument errors before any HIP call, caller-owned device buffers, the caller's stream
 * last, text through mlx_last_error) and do not move MLX_ABI_VERSION.
 */
#ifndef MOMLEVEL_LAYER_H
#define MOMLEVEL_LAYER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* layers per launch: their column sums live in registers */
#define MLX_LAYER_MAX 8

/* records a thread carries through the z loop (the kernel's NTI): the dz of a level and layer is
 * formed once and used for that many records */
int mlx_layer_steps(void);

/* Block rows along the records (gridDim.y) of a call over nrec records: min(ceil(nrec /
 * mlx_layer_steps()), cap).  Up to the cap a block carries one group of mlx_layer_steps() records;
 * past it a block goes on to the group cap rows further, and so on, so mlx_layer_record_blocks of
 * a huge nrec is the cap.  Host arithmetic only, the rule the launch itself goes by; a record's
 * bits do not depend on it.  0 for nrec <= 0 or nrec > 2^38. */
int mlx_layer_record_blocks(int64_t nrec);

/* out[r, l, c] as defined above.
 *
 *   x:       (nrec, nz, plane)  `x_dtype` (MLX_DTYPE_F64 | MLX_DTYPE_F32), device
 *   z_i:     (nz + 1) float64 interfaces, device
 *   depth:   (plane) float64, device; NaN = land -> 0, as calc_dz's fillna(0.0)
 *   top, bottom: `nlayers` float64 each, HOST arrays, passed to the kernel by value;
 *            bottom[l] = +inf means "no bottom" (np.minimum(depth, inf) == depth)
 *   surface: (plane) float64 on the device, or NULL; out is NaN where surface is NaN
 *   out:     (nrec, nlayers, plane) float64, device
 * all contiguous.  nrec == 0 or plane == 0 returns 0 without a launch (pointers are not looked at;
 * nothing is written).
 *
 * Refused before any HIP call: a dtype that is not MLX_DTYPE_F64 / MLX_DTYPE_F32 (MLX_E_ENUM);
 * nlayers < 1 or > MLX_LAYER_MAX, nz < 1, nrec or plane < 0, nrec * nz * plane > 2^38
 * (MLX_E_SHAPE); x, z_i, depth, top, bottom or out NULL with work to do (MLX_E_NULL); a pointer not
 * aligned to its element (MLX_E_ALIGN); a NaN in top or bottom, top[l] < 0, bottom[l] <= top[l]
 * (MLX_E_SHAPE). */
int mlx_layer_integral(const void *x, int x_dtype, int64_t nrec, int64_t nz, int64_t plane,
                       const double *z_i, const double *depth, const double *top,
                       const double *bottom, int nlayers, const double *surface, double scale,
                       double *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MOMLEVEL_LAYER_H */
