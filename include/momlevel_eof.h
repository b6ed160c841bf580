/*
 * momlevel_eof.h -- the time-by-time Gram matrix of one or two (time, cells) records, centred and
 * scaled per cell on the way in: the contraction behind the EOFs and principal components of
 * momlevel_amd.eof, in libmomlevel_hip.so (gfx950).
 *
 * AN EXTENSION: momlevel has no such function.  The specification is the numpy restatement of
 * tests/eof_numpy.py: with y1, y2 widened exactly to float64,
 *
 *     ok      = ~isnan(center1) & ~isnan(center2) & ~isnan(scale)         per cell
 *     b1[s,c] = where(ok, (y1[s,c] - center1[c]) * scale[c], 0.0)         two IEEE roundings, no fma
 *     b2[t,c] = where(ok, (y2[t,c] - center2[c]) * scale[c], 0.0)
 *     G[s,t]  = sum_c b1[s,c] * b2[t,c]                                   (nt1, nt2) float64
 *
 * An excluded cell contributes exactly 0 whatever y holds there (NaN, Inf).  A NaN in y at an
 * included cell propagates into its row and column of G.  Infinities at included cells are outside
 * the contract.  A NULL center is 0 and a NULL scale is 1: the same arithmetic, so the same bits as
 * arrays of zeros and ones.
 *
 * y2 == NULL is THE SYMMETRIC FORM: b2 = b1 (nt2, dtype2 and center2 are ignored), only the tiles
 * on and above the diagonal are computed -- in a diagonal tile only the elements on and above it --
 * and G is mirrored: G == G.T bit for bit.
 *
 * THE KERNELS.  Stage 1: a block owns one output tile of mlx_gram_tile() rows by as many columns
 * and one contiguous range of mlx_gram_cells(n) cells.  It walks its range in chunks of 16 cells:
 * the row tiles of b1 and b2 are staged through LDS with the centring and scaling applied on the way
 * in (16-byte loads along the cells where a lane's pack is aligned and inside the range, element by
 * element elsewhere: the same cells, the same bits; rows past nt* and cells past the range are
 * zero-filled in LDS and never read), and accumulated with v_mfma_f64_16x16x4_f64 into register
 * tiles.  The block's partial tile goes to the workspace.  Stage 2: one thread per element of G adds
 * the partials of its element in ascending range order and writes G (and its mirror).  No atomics.
 *
 * THE ORDER OF SUMMATION is fixed.  The number of ranges is ceil(n / mlx_gram_cells(n)), a function
 * of n alone, at most MLX_GRAM_MAX_SPLIT; it depends neither on the device, nor on the pointers, nor
 * on nt*.  The bits of G[s,t] depend on the rows s and t and on n: not on the rows around them, not
 * on where in a tile they fall, not on the path the loads took.  Two runs are bit-identical.
 *
 * A header of its own, as include/momlevel_area.h: the entry points have no host build.  They live
 * in the same library, follow the same conventions (momlevel_hip.h, "Conventions": int status,
 * MLX_E_* argument errors before any HIP call, caller-owned device buffers, the caller's stream
 * last, text through mlx_last_error) and do not move MLX_ABI_VERSION.
 */
#ifndef MOMLEVEL_EOF_H
#define MOMLEVEL_EOF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the most ranges the cells are cut into: the partial tiles of one element that stage 2 adds */
#define MLX_GRAM_MAX_SPLIT 32

/* rows (and columns) of G one block of stage 1 owns */
int mlx_gram_tile(void);

/* cells of one block's range for a record of n cells: a multiple of 16, a constant up to
 * MLX_GRAM_MAX_SPLIT times itself and ceil(n / MLX_GRAM_MAX_SPLIT) rounded up beyond; 0 for n < 1 */
int64_t mlx_gram_cells(int64_t n);

/* bytes of workspace mlx_gram_matrix needs: 8 per element of a tile, tile pair and range; nt2 == 0
 * asks for the symmetric form.  0 for arguments the call would refuse */
size_t mlx_gram_matrix_workspace_bytes(int64_t nt1, int64_t nt2, int64_t n);

/* G as defined above.
 *
 *   y1: (nt1, n) `dtype1`     y2: (nt2, n) `dtype2`, or NULL (the symmetric form: G is (nt1, nt1))
 *   center1, center2, scale: (n) float64, each may be NULL      G: (nt1, nt2) float64
 *   workspace: 8-byte aligned, caller-owned
 * all contiguous on the device; G must not overlap an operand.
 *
 * Refused before any HIP call: a dtype that is not MLX_DTYPE_F64 / MLX_DTYPE_F32 (MLX_E_ENUM);
 * nt1, nt2 or n < 1, nt1 * n or nt2 * n beyond what a record kernel addresses (2^31 steps, 2^38
 * cells), more than 2^31 - 1 blocks (MLX_E_SHAPE); y1, G or workspace NULL (MLX_E_NULL);
 * workspace_bytes below mlx_gram_matrix_workspace_bytes or a workspace not 8-byte aligned
 * (MLX_E_WORKSPACE); y1 / y2 not aligned to their element, center1 / center2 / scale / G not
 * 8-byte aligned (MLX_E_ALIGN). */
int mlx_gram_matrix(const void *y1, int dtype1, const double *center1, int64_t nt1,
                    const void *y2, int dtype2, const double *center2, int64_t nt2,
                    const double *scale, int64_t n, double *G,
                    void *workspace, size_t workspace_bytes, void *stream);

/* Measurement aid: `blocks` blocks of 4 waves issue `iters` rounds of 8 independent
 * v_mfma_f64_16x16x4_f64 each on registers (no memory traffic but 8 bytes per lane at the end, to
 * sink[blocks * 256]); *flop, when not NULL, receives the floating-point operations of the launch
 * (2 * 16 * 16 * 4 per instruction).  Refused: iters or blocks < 1, blocks > 2^20 (MLX_E_SHAPE);
 * sink NULL (MLX_E_NULL) or not 8-byte aligned (MLX_E_ALIGN). */
int mlx_gram_issue_probe(int64_t iters, int64_t blocks, double *sink, int64_t *flop, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MOMLEVEL_EOF_H */
