// momlevel_layer.hip -- mlx_layer_integral (include/momlevel_layer.h): the sums over z of
// calc_dz(top[l], bottom[l]) * x for up to MLX_LAYER_MAX depth layers of a (record, z, plane) field.
// An EXTENSION (momlevel has no such function); the specification is tests/layer_numpy.py.
//
// k_layer_integral: wave64, 256-thread blocks, grid = (tiles of the plane, blocks of kLayerSteps
// records).  A thread owns one 16-byte pack of adjacent cells (2 float64 or 4 float32) and
// kLayerSteps consecutive records, as K2 does: z is the outer, sequential loop (numpy's axis
// reduce), the records are unrolled inside it with their NL x kLayerSteps x VEC column sums in
// registers, so a level's dz_l is formed once per layer and reused for every record of the thread.
// z_i and the layer bounds are wave-uniform (scalar loads, kernel arguments).  A level that does not
// overlap a layer is skipped wave-uniformly -- its terms would be +-0 or NaN, which never change a
// sum that started from +0.0 -- so disjoint layers cost one or two sums per level, not NL.  The
// field's loads are streaming (`nt`), the next level's are issued before the current one is summed.
// No atomics, no LDS: a column belongs to one thread.
//
// GENERIC twin: one cell per thread, scalar loads and stores, for planes that are not a whole
// number of packs and for x / out that are not 16-byte aligned.  The same arithmetic in the same
// order: the same bits.
//
// NLC is the compile-time capacity (1, 2, 4 or 8 layers) so that one or three layers do not pay
// the registers of eight; nl <= NLC is the launch's count.  A layer's bits do not depend on it.
//
// Compile: with momlevel_hip.hip (csrc/build.py), -ffp-contract=off and the pragma below: w * x is
// one rounding, then one add.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/momlevel_hip.h"
#include "../../include/momlevel_layer.h"
#include "mlx_internal.hpp"
#include "mlx_pack.hpp"

#pragma clang fp contract(off)

namespace mlx {
namespace {

constexpr int kLayerBlock = 256;  // 4 waves of 64
constexpr int kLayerSteps = 4;    // records per thread (NTI)
constexpr int64_t kLayerMaxCells = (int64_t)1 << 38;
constexpr unsigned kLayerMaxGridY = 65535;

struct LayerBounds {
  double top[MLX_LAYER_MAX];
  double bottom[MLX_LAYER_MAX];
};

__device__ __forceinline__ bool layer_isnan(double x) { return x != x; }
__device__ __forceinline__ double layer_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

template <typename TV, int VEC>
__device__ __forceinline__ Pack<TV, VEC> layer_load(const TV* __restrict__ p) {
  if constexpr (VEC == 1) {
    Pack<TV, 1> r;
    r.v[0] = __builtin_nontemporal_load(p);
    return r;
  } else {
    return load_pack<TV, VEC, true>(p);
  }
}

template <typename TV, int NLC, bool GENERIC>
__global__ __launch_bounds__(kLayerBlock) void k_layer_integral(
    const TV* __restrict__ x, int64_t nrec, int64_t nz, int64_t plane,
    const double* __restrict__ z_i, const double* __restrict__ depth, LayerBounds lb, int nl,
    const double* __restrict__ surface, double scale, double* __restrict__ out) {
  constexpr int VEC = GENERIC ? 1 : 16 / (int)sizeof(TV);
  constexpr int NTI = kLayerSteps;
  const int64_t col = ((int64_t)blockIdx.x * kLayerBlock + threadIdx.x) * VEC;
  if (col + VEC > plane) return;  // whole packs only (the host picks GENERIC otherwise); no barrier
  const int64_t n3 = nz * plane;
  const int64_t nrb = (nrec + NTI - 1) / NTI;

  // the floor of this thread's cells per layer: fillna(0.0), then np.minimum(depth, bottom)
  double d0[VEC];
  bool dry[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    const double d = depth[col + k];
    d0[k] = layer_isnan(d) ? 0.0 : d;
    dry[k] = surface != nullptr && layer_isnan(surface[col + k]);
  }

  for (int64_t rb = blockIdx.y; rb < nrb; rb += gridDim.y) {
    const int64_t r0 = rb * NTI;
    const int nvalid = (int)((nrec - r0) < NTI ? (nrec - r0) : NTI);
    const TV* __restrict__ xr = x + r0 * n3 + col;

    double acc[NLC][NTI][VEC];
#pragma unroll
    for (int l = 0; l < NLC; ++l)
#pragma unroll
      for (int j = 0; j < NTI; ++j)
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[l][j][k] = 0.0;

    Pack<TV, VEC> cur[NTI], nxt[NTI];
#pragma unroll
    for (int j = 0; j < NTI; ++j) {
      cur[j] = {};
      nxt[j] = {};
      if (j < nvalid) cur[j] = layer_load<TV, VEC>(xr + j * n3);
    }

    for (int64_t z = 0; z < nz; ++z) {
      if (z + 1 < nz) {  // the next level's loads fly while this one is summed
#pragma unroll
        for (int j = 0; j < NTI; ++j)
          if (j < nvalid) nxt[j] = layer_load<TV, VEC>(xr + j * n3 + (z + 1) * plane);
      }
      const double ztop = z_i[z], zbot = z_i[z + 1];
#pragma unroll
      for (int l = 0; l < NLC; ++l) {
        if (l < nl) {
          const double top = lb.top[l], bottom = lb.bottom[l];
          // wave-uniform: no overlap, every term is +-0 or NaN -> the sums do not move
          if (zbot <= top || ztop >= bottom) continue;
          double w[VEC];
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            const double d = (bottom < d0[k]) ? bottom : d0[k];  // np.minimum(depth, bottom)
            w[k] = calc_dz_cell<true>(d, ztop, zbot, top);
          }
#pragma unroll
          for (int j = 0; j < NTI; ++j) {
            if (j < nvalid) {
#pragma unroll
              for (int k = 0; k < VEC; ++k) {
                const double term = w[k] * (double)cur[j].v[k];  // float -> double: exact
                acc[l][j][k] += layer_isnan(term) ? 0.0 : term;  // skipna, z ascending
              }
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < NTI; ++j) cur[j] = nxt[j];
    }

#pragma unroll
    for (int j = 0; j < NTI; ++j) {
      if (j < nvalid) {
#pragma unroll
        for (int l = 0; l < NLC; ++l) {
          if (l < nl) {
            double* __restrict__ o = out + ((r0 + j) * nl + l) * plane + col;
            Pack<double, VEC> e;
#pragma unroll
            for (int k = 0; k < VEC; ++k) e.v[k] = dry[k] ? layer_nan() : scale * acc[l][j][k];
            if constexpr (VEC == 1) o[0] = e.v[0];
            else store_pack<double, VEC, false>(o, e);
          }
        }
      }
    }
  }
}

// gridDim.y of a call over nrec > 0 records: one block row per kLayerSteps records up to the cap,
// past which the rows stride.  The one rule: mlx_layer_record_blocks reports it, the launch uses it.
inline int64_t layer_record_blocks(int64_t nrec) {
  const int64_t nrb = ceil_div(nrec, kLayerSteps);
  return nrb < (int64_t)kLayerMaxGridY ? nrb : (int64_t)kLayerMaxGridY;
}

template <typename TV, int NLC>
void layer_launch(bool generic, dim3 grid, hipStream_t st, const void* x, int64_t nrec, int64_t nz,
                  int64_t plane, const double* z_i, const double* depth, const LayerBounds& lb,
                  int nl, const double* surface, double scale, double* out) {
  if (generic)
    hipLaunchKernelGGL((k_layer_integral<TV, NLC, true>), grid, dim3(kLayerBlock), 0, st,
                       (const TV*)x, nrec, nz, plane, z_i, depth, lb, nl, surface, scale, out);
  else
    hipLaunchKernelGGL((k_layer_integral<TV, NLC, false>), grid, dim3(kLayerBlock), 0, st,
                       (const TV*)x, nrec, nz, plane, z_i, depth, lb, nl, surface, scale, out);
}

template <typename TV>
void layer_dispatch(bool generic, dim3 grid, hipStream_t st, const void* x, int64_t nrec,
                    int64_t nz, int64_t plane, const double* z_i, const double* depth,
                    const LayerBounds& lb, int nl, const double* surface, double scale,
                    double* out) {
#define MLX_LAYER_GO(NLC) \
  layer_launch<TV, NLC>(generic, grid, st, x, nrec, nz, plane, z_i, depth, lb, nl, surface, scale, out)
  if (nl <= 1) MLX_LAYER_GO(1);
  else if (nl <= 2) MLX_LAYER_GO(2);
  else if (nl <= 4) MLX_LAYER_GO(4);
  else MLX_LAYER_GO(8);
#undef MLX_LAYER_GO
}

}  // namespace
}  // namespace mlx

extern "C" int mlx_layer_steps(void) { return mlx::kLayerSteps; }

extern "C" int mlx_layer_record_blocks(int64_t nrec) {
  if (nrec <= 0 || nrec > mlx::kLayerMaxCells) return 0;
  return (int)mlx::layer_record_blocks(nrec);
}

extern "C" int mlx_layer_integral(const void* x, int x_dtype, int64_t nrec, int64_t nz,
                                  int64_t plane, const double* z_i, const double* depth,
                                  const double* top, const double* bottom, int nlayers,
                                  const double* surface, double scale, double* out, void* stream) {
  using namespace mlx;
  using detail::fail;
  using detail::hip_status;
  if (!is_float_dtype(x_dtype)) return fail(MLX_E_ENUM, "x_dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  if (nlayers < 1 || nlayers > MLX_LAYER_MAX)
    return fail(MLX_E_SHAPE, "need 1 <= nlayers <= MLX_LAYER_MAX");
  if (nz < 1) return fail(MLX_E_SHAPE, "need nz >= 1");
  if (nrec < 0 || plane < 0) return fail(MLX_E_SHAPE, "nrec and plane must not be negative");
  if (nz > kLayerMaxCells || (nrec > 0 && plane > 0 &&
                              (plane > kLayerMaxCells / nz || nrec > kLayerMaxCells / (nz * plane))))
    return fail(MLX_E_SHAPE, "need nrec * nz * plane <= 2^38");
  if (nrec == 0 || plane == 0) return 0;
  if (!x || !z_i || !depth || !top || !bottom || !out)
    return fail(MLX_E_NULL, "x, z_i, depth, top, bottom and out must not be NULL");
  if (!aligned(x, dtype_size(x_dtype)) || !aligned(z_i, 8) || !aligned(depth, 8) ||
      !aligned(top, 8) || !aligned(bottom, 8) || !aligned(surface, 8) || !aligned(out, 8))
    return fail(MLX_E_ALIGN, "x / z_i / depth / top / bottom / surface / out not aligned to their element");
  LayerBounds lb;
  for (int l = 0; l < MLX_LAYER_MAX; ++l) {
    lb.top[l] = 0.0;
    lb.bottom[l] = 0.0;
  }
  for (int l = 0; l < nlayers; ++l) {
    if (top[l] != top[l] || bottom[l] != bottom[l])
      return fail(MLX_E_SHAPE, "top and bottom must not hold NaN");
    if (top[l] < 0.0) return fail(MLX_E_SHAPE, "need top[l] >= 0");
    if (bottom[l] <= top[l]) return fail(MLX_E_SHAPE, "need bottom[l] > top[l]");
    lb.top[l] = top[l];
    lb.bottom[l] = bottom[l];
  }
  const bool f64 = x_dtype == MLX_DTYPE_F64;
  const int vec = f64 ? 2 : 4;
  // packs: every level of every record starts on a 16-byte boundary, and so does every out plane
  const bool generic = plane % vec != 0 || !aligned(x, 16) || !aligned(out, 16);
  const int64_t per_block = (int64_t)kLayerBlock * (generic ? 1 : vec);
  const dim3 grid((unsigned)ceil_div(plane, per_block), (unsigned)layer_record_blocks(nrec));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (f64)
    layer_dispatch<double>(generic, grid, st, x, nrec, nz, plane, z_i, depth, lb, nlayers, surface,
                           scale, out);
  else
    layer_dispatch<float>(generic, grid, st, x, nrec, nz, plane, z_i, depth, lb, nlayers, surface,
                          scale, out);
  return hip_status(hipGetLastError(), "k_layer_integral launch");
}
