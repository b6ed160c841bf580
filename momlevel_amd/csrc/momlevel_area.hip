// momlevel_area.hip -- mlx_area_mean / mlx_area_anomaly (include/momlevel_area.h): area-weighted,
// NaN-aware means over the plane of a (record, plane) field per region, and the anomalies from them.
// An EXTENSION (momlevel has no such function); the specification is tests/area_numpy.py.
//
// Memory-bound: the record is read once (8 or 4 bytes per cell), the 2-D maps once per window of
// records, and a mean is 16 bytes per (record, tile, slot) of workspace.  No atomics, global or LDS.
//
// STAGE 1, k_area_partial: wave64, 256-thread blocks, one block per (tile, window of
// MLX_AREA_WINDOW records).  A thread owns kAreaU packs of 16 bytes of the record per tile -- cells
// base + (u * 256 + tid) * P + k -- and holds their weights (float64, NaN = no weight) and slots in
// registers for the whole window (as K1 holds vol0).  Per record it loads its packs (the next
// record's loads are issued before the current one is reduced), forms w and w * v per cell and adds
// them IN ASCENDING (u, k)
//   - slot == NULL: into two registers,
//   - otherwise: into its private LDS column acc[2 * slot + {0: num, 1: den}][tid] -- row-major,
//     256 doubles a row, so a wave's 64 columns of any mix of rows fall on 64 different 8-byte bank
//     pairs: no conflicts, and no LDS atomics since nobody else touches the column;
// then the block adds each row's 256 columns: wave q takes rows q, q + 4, ...:
// ((c[l] + c[l+64]) + c[l+128]) + c[l+192], a shuffle tree over the 64 lanes, lane 0 stores the
// partial (and the row is zeroed for the next record).  num and den rows run the same code.
//
// STAGE 2, k_area_finish: one block per (record, slot) adds the tiles' (num, den) partials -- thread
// t the tiles t, t + 256, ... in ascending order, then the binary LDS tree of k_reduce_rows -- and
// writes mean = num / den (and den).
//
// LOADS.  Which thread owns which cell never depends on the pointers: a record's tile is moved in
// 16-byte `nt` packs when it is whole and its first cell is 16-byte aligned, and cell by cell (the
// same cells, the same order, the same bits) when it is not -- the last tile of the plane, every
// other record of an odd plane, a view offset by one element.  The maps are read cell by cell: once
// per window.
//
// k_area_anomaly: out = (float64) v - mean[rec, slot], the same windows (the slot map stays in
// registers), 16-byte stores on the aligned body.
//
// Compile: with momlevel_hip.hip (csrc/build.py), -ffp-contract=off and the pragma below: w * v is
// one rounding, then one add.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/momlevel_hip.h"
#include "../../include/momlevel_area.h"
#include "mlx_internal.hpp"
#include "mlx_pack.hpp"

#pragma clang fp contract(off)

namespace mlx {
namespace {

constexpr int kAreaBlock = 256;  // 4 waves of 64
constexpr int kAreaU = 4;        // 16-byte packs per thread, tile and record
constexpr int kAnomU = 4;        // packs of two cells per thread, chunk and record (anomaly)
constexpr int kAnomP = 2;
constexpr int64_t kAreaWindow = MLX_AREA_WINDOW;
constexpr int64_t kAreaMaxCells = (int64_t)1 << 38;
constexpr int64_t kAreaMaxRecords = (int64_t)1 << 26;
constexpr int kAnomMaxSlots = 1 << 24;

template <typename TV>
constexpr int64_t area_tile_cells() {
  return (int64_t)kAreaBlock * kAreaU * (16 / (int)sizeof(TV));
}
constexpr int64_t kAnomChunk = (int64_t)kAreaBlock * kAnomU * kAnomP;

__device__ __forceinline__ bool area_isnan(double x) { return x != x; }
__device__ __forceinline__ double area_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// the cells of one record this thread owns in the tile at `p` (its first cell): in packs, or -- the
// tile is not whole or `p` not 16-byte aligned -- cell by cell; cells past the plane read as 0
template <typename TV, int U, int P>
__device__ __forceinline__ void area_load(const TV* __restrict__ p, int64_t left, bool whole,
                                          TV (&x)[U * P]) {
  const int tid = threadIdx.x;
  if (whole && (reinterpret_cast<uintptr_t>(p) % (sizeof(TV) * P)) == 0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const Pack<TV, P> r = load_pack<TV, P, true>(p + (int64_t)(u * kAreaBlock + tid) * P);
#pragma unroll
      for (int k = 0; k < P; ++k) x[u * P + k] = r.v[k];
    }
  } else {
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int k = 0; k < P; ++k) {
        const int64_t i = (int64_t)(u * kAreaBlock + tid) * P + k;
        x[u * P + k] = i < left ? __builtin_nontemporal_load(p + i) : (TV)0;
      }
    }
  }
}

// the sum of a row's 256 columns in the block's fixed order; every lane of the wave calls it
__device__ __forceinline__ double area_row_sum(double* __restrict__ row, int lane, bool clear) {
  double x = ((row[lane] + row[lane + 64]) + row[lane + 128]) + row[lane + 192];
  if (clear) row[lane] = row[lane + 64] = row[lane + 128] = row[lane + 192] = 0.0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;  // (lane 0 holds the sum)
}

// partials[((rec * ntiles + tile) * nslots + slot) * 2 + {0: num, 1: den}]
template <typename TV, typename TA, bool SLOTS>
__global__ __launch_bounds__(kAreaBlock) void k_area_partial(const TV* __restrict__ v,
                                                             const TA* __restrict__ area,
                                                             const int32_t* __restrict__ slot,
                                                             int nslots, int64_t nrec, int64_t plane,
                                                             int64_t ntiles,
                                                             double* __restrict__ partials) {
  constexpr int P = 16 / (int)sizeof(TV), C = kAreaU * P;
  constexpr int64_t T = area_tile_cells<TV>();
  extern __shared__ __attribute__((aligned(16))) char area_smem[];
  double* acc = reinterpret_cast<double*>(area_smem);  // [2 * nslots][kAreaBlock]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nrows = 2 * nslots;
  const int64_t tile = blockIdx.x % ntiles, win = blockIdx.x / ntiles;
  const int64_t base = tile * T, left = plane - base;  // left >= 1
  const bool whole = left >= T;
  const int64_t r0 = win * kAreaWindow, r1 = r0 + kAreaWindow < nrec ? r0 + kAreaWindow : nrec;

  // the maps of this thread's cells: for the whole window
  double a[C];
  int s[C];
#pragma unroll
  for (int u = 0; u < kAreaU; ++u) {
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const int64_t i = (int64_t)(u * kAreaBlock + tid) * P + k;
      const int c = u * P + k;
      a[c] = i < left ? (double)area[base + i] : area_nan();  // float -> double: exact
      if constexpr (SLOTS) {
        const int sv = i < left ? slot[base + i] : -1;
        s[c] = (unsigned)sv < (unsigned)nslots ? sv : -1;
      }
    }
  }
  if constexpr (SLOTS) {
    for (int r = 0; r < nrows; ++r) acc[r * kAreaBlock + tid] = 0.0;  // (its own column)
  }

  TV cur[C], nxt[C] = {};
  area_load<TV, kAreaU, P>(v + r0 * plane + base, left, whole, cur);
  for (int64_t rec = r0; rec < r1; ++rec) {
    if (rec + 1 < r1) area_load<TV, kAreaU, P>(v + (rec + 1) * plane + base, left, whole, nxt);
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {  // cells in ascending order: the order of summation is fixed
      const double x = (double)cur[c];
      const bool valid = !area_isnan(x) && !area_isnan(a[c]);
      const double w = valid ? a[c] : 0.0;
      const double t = w * (valid ? x : 0.0);
      if constexpr (SLOTS) {
        if (s[c] >= 0) {
          double* col = acc + (2 * s[c]) * kAreaBlock + tid;
          col[0] += t;
          col[kAreaBlock] += w;
        }
      } else {
        num += t;
        den += w;
      }
    }
    if constexpr (!SLOTS) {
      acc[tid] = num;
      acc[kAreaBlock + tid] = den;
    }
    __syncthreads();
    for (int row = wave; row < nrows; row += kAreaBlock / 64) {
      const double sum = area_row_sum(acc + row * kAreaBlock, lane, SLOTS);
      if (lane == 0) partials[(rec * ntiles + tile) * nrows + row] = sum;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C; ++c) cur[c] = nxt[c];
  }
}

// mean[rec, slot] = num / den over the tiles' partials; one block per (rec, slot), fixed order
__global__ __launch_bounds__(kAreaBlock) void k_area_finish(const double* __restrict__ partials,
                                                            int nslots, int64_t ntiles,
                                                            double* __restrict__ mean,
                                                            double* __restrict__ wsum) {
  __shared__ double red[2][kAreaBlock];
  const int64_t rec = blockIdx.x / nslots;
  const int sl = (int)(blockIdx.x % nslots);
  const int64_t nrows = 2 * (int64_t)nslots;
  const double* p = partials + rec * ntiles * nrows + 2 * sl;
  double num = 0.0, den = 0.0;
  for (int64_t i = threadIdx.x; i < ntiles; i += kAreaBlock) {
    num += p[i * nrows];
    den += p[i * nrows + 1];
  }
  red[0][threadIdx.x] = num;
  red[1][threadIdx.x] = den;
  __syncthreads();
#pragma unroll
  for (int st = kAreaBlock / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      red[0][threadIdx.x] += red[0][threadIdx.x + st];
      red[1][threadIdx.x] += red[1][threadIdx.x + st];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    mean[blockIdx.x] = red[0][0] / red[1][0];  // 0 / 0: NaN, nothing was valid
    if (wsum) wsum[blockIdx.x] = red[1][0];
  }
}

// out[rec, c] = v[rec, c] - mean[rec, slot[c]]; one block per (chunk of the plane, window)
template <typename TV, bool SLOTS>
__global__ __launch_bounds__(kAreaBlock) void k_area_anomaly(const TV* __restrict__ v,
                                                             const int32_t* __restrict__ slot,
                                                             int nslots,
                                                             const double* __restrict__ mean,
                                                             int64_t nrec, int64_t plane,
                                                             int64_t nchunks,
                                                             double* __restrict__ out) {
  constexpr int P = kAnomP, U = kAnomU, C = U * P;
  const int tid = threadIdx.x;
  const int64_t chunk = blockIdx.x % nchunks, win = blockIdx.x / nchunks;
  const int64_t base = chunk * kAnomChunk, left = plane - base;
  const bool whole = left >= kAnomChunk;
  const int64_t r0 = win * kAreaWindow, r1 = r0 + kAreaWindow < nrec ? r0 + kAreaWindow : nrec;
  int s[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int64_t i = (int64_t)((c / P) * kAreaBlock + tid) * P + c % P;
    if constexpr (SLOTS) {
      const int sv = i < left ? slot[base + i] : -1;
      s[c] = (unsigned)sv < (unsigned)nslots ? sv : -1;
    } else {
      s[c] = 0;
    }
  }
  for (int64_t rec = r0; rec < r1; ++rec) {
    const TV* p = v + rec * plane + base;
    double* o = out + rec * plane + base;
    const double* m = mean + rec * nslots;
    TV x[C];
    area_load<TV, U, P>(p, left, whole, x);
    double r[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const double mc = m[s[c] < 0 ? 0 : s[c]];
      r[c] = s[c] < 0 ? area_nan() : (double)x[c] - mc;  // float -> double: exact; one subtraction
    }
    if (whole && (reinterpret_cast<uintptr_t>(o) % 16) == 0) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        Pack<double, P> q;
#pragma unroll
        for (int k = 0; k < P; ++k) q.v[k] = r[u * P + k];
        store_pack<double, P, true>(o + (int64_t)(u * kAreaBlock + tid) * P, q);
      }
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int64_t i = (int64_t)((c / P) * kAreaBlock + tid) * P + c % P;
        if (i < left) o[i] = r[c];
      }
    }
  }
}

inline int64_t area_tile_of(int v_dtype) {
  return v_dtype == MLX_DTYPE_F64 ? area_tile_cells<double>()
         : v_dtype == MLX_DTYPE_F32 ? area_tile_cells<float>() : 0;
}

// the checks mlx_area_mean and mlx_area_anomaly share; 0 or the MLX_E_* code (text recorded)
int area_check_shape(int v_dtype, int nslots, int max_slots, bool has_slot, int64_t nrec,
                     int64_t plane) {
  using detail::fail;
  if (!is_float_dtype(v_dtype)) return fail(MLX_E_ENUM, "v_dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  if (nslots < 1 || nslots > max_slots)
    return fail(MLX_E_SHAPE, max_slots == MLX_AREA_MAX_SLOTS
                                 ? "need 1 <= nslots <= MLX_AREA_MAX_SLOTS"
                                 : "need 1 <= nslots <= 2^24");
  if (!has_slot && nslots != 1) return fail(MLX_E_SHAPE, "slot == NULL is one region: nslots must be 1");
  if (nrec < 0 || plane < 0) return fail(MLX_E_SHAPE, "nrec and plane must not be negative");
  if (nrec > kAreaMaxRecords) return fail(MLX_E_SHAPE, "need nrec <= 2^26");
  if (plane > kAreaMaxCells || (nrec > 0 && plane > kAreaMaxCells / nrec))
    return fail(MLX_E_SHAPE, "need nrec * plane <= 2^38");
  return 0;
}

template <typename TV, typename TA>
void area_launch_partial(const void* v, const void* area, const int32_t* slot, int nslots,
                         int64_t nrec, int64_t plane, int64_t ntiles, double* partials,
                         hipStream_t st) {
  const int64_t nwin = ceil_div(nrec, kAreaWindow);
  const dim3 grid((unsigned)(ntiles * nwin)), block(kAreaBlock);
  const size_t lds = (size_t)2 * nslots * kAreaBlock * sizeof(double);
  if (slot)
    hipLaunchKernelGGL((k_area_partial<TV, TA, true>), grid, block, lds, st, (const TV*)v,
                       (const TA*)area, slot, nslots, nrec, plane, ntiles, partials);
  else
    hipLaunchKernelGGL((k_area_partial<TV, TA, false>), grid, block, lds, st, (const TV*)v,
                       (const TA*)area, slot, nslots, nrec, plane, ntiles, partials);
}

}  // namespace
}  // namespace mlx

extern "C" int64_t mlx_area_tile(int v_dtype) { return mlx::area_tile_of(v_dtype); }

extern "C" size_t mlx_area_mean_workspace_bytes(int64_t nrec, int64_t plane, int nslots,
                                                int v_dtype) {
  using namespace mlx;
  const int64_t tile = area_tile_of(v_dtype);
  if (tile == 0 || nslots < 1 || nslots > MLX_AREA_MAX_SLOTS || nrec < 0 || plane < 0 ||
      nrec > kAreaMaxRecords || plane > kAreaMaxCells || (nrec > 0 && plane > kAreaMaxCells / nrec))
    return 0;
  return (size_t)nrec * (size_t)ceil_div(plane, tile) * (size_t)nslots * 2 * sizeof(double);
}

extern "C" int mlx_area_mean(const void* v, int v_dtype, const void* area, int area_dtype,
                             const int32_t* slot, int nslots, int64_t nrec, int64_t plane,
                             double* mean, double* wsum, void* workspace, size_t workspace_bytes,
                             void* stream) {
  using namespace mlx;
  using detail::fail;
  using detail::hip_status;
  if (!is_float_dtype(area_dtype))
    return fail(MLX_E_ENUM, "area_dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  if (int rc = area_check_shape(v_dtype, nslots, MLX_AREA_MAX_SLOTS, slot != nullptr, nrec, plane))
    return rc;
  if (nrec == 0 || plane == 0) return 0;
  if (!v || !area || !mean || !workspace)
    return fail(MLX_E_NULL, "v, area, mean and workspace must not be NULL");
  if (!aligned(v, dtype_size(v_dtype)) || !aligned(area, dtype_size(area_dtype)) ||
      !aligned(slot, 4))
    return fail(MLX_E_ALIGN, "v / area / slot not aligned to their element");
  if (!aligned(mean, 8) || !aligned(wsum, 8)) return fail(MLX_E_ALIGN, "mean / wsum not 8-byte aligned");
  const size_t need = mlx_area_mean_workspace_bytes(nrec, plane, nslots, v_dtype);
  if (workspace_bytes < need || !aligned(workspace, 8))
    return fail(MLX_E_WORKSPACE, "workspace too small (mlx_area_mean_workspace_bytes) or not 8-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* partials = static_cast<double*>(workspace);
  const int64_t ntiles = ceil_div(plane, area_tile_of(v_dtype));
  const bool v64 = v_dtype == MLX_DTYPE_F64, a64 = area_dtype == MLX_DTYPE_F64;
  if (v64) {
    if (a64) area_launch_partial<double, double>(v, area, slot, nslots, nrec, plane, ntiles, partials, st);
    else area_launch_partial<double, float>(v, area, slot, nslots, nrec, plane, ntiles, partials, st);
  } else {
    if (a64) area_launch_partial<float, double>(v, area, slot, nslots, nrec, plane, ntiles, partials, st);
    else area_launch_partial<float, float>(v, area, slot, nslots, nrec, plane, ntiles, partials, st);
  }
  if (int rc = hip_status(hipGetLastError(), "k_area_partial launch")) return rc;
  hipLaunchKernelGGL(k_area_finish, dim3((unsigned)(nrec * nslots)), dim3(kAreaBlock), 0, st,
                     (const double*)partials, nslots, ntiles, mean, wsum);
  return hip_status(hipGetLastError(), "k_area_finish launch");
}

extern "C" int mlx_area_anomaly(const void* v, int v_dtype, const int32_t* slot, int nslots,
                                const double* mean, int64_t nrec, int64_t plane, double* out,
                                void* stream) {
  using namespace mlx;
  using detail::fail;
  using detail::hip_status;
  if (int rc = area_check_shape(v_dtype, nslots, kAnomMaxSlots, slot != nullptr, nrec, plane))
    return rc;
  if (nrec == 0 || plane == 0) return 0;
  if (!v || !mean || !out) return fail(MLX_E_NULL, "v, mean and out must not be NULL");
  if (!aligned(v, dtype_size(v_dtype)) || !aligned(slot, 4))
    return fail(MLX_E_ALIGN, "v / slot not aligned to their element");
  if (!aligned(mean, 8) || !aligned(out, 8)) return fail(MLX_E_ALIGN, "mean / out not 8-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t nchunks = ceil_div(plane, kAnomChunk), nwin = ceil_div(nrec, kAreaWindow);
  const dim3 grid((unsigned)(nchunks * nwin)), block(kAreaBlock);
  const bool v64 = v_dtype == MLX_DTYPE_F64;
#define MLX_AREA_ANOM(TV, SL)                                                                    \
  hipLaunchKernelGGL((k_area_anomaly<TV, SL>), grid, block, 0, st, (const TV*)v, slot, nslots,   \
                     mean, nrec, plane, nchunks, out)
  if (v64) {
    if (slot) MLX_AREA_ANOM(double, true);
    else MLX_AREA_ANOM(double, false);
  } else {
    if (slot) MLX_AREA_ANOM(float, true);
    else MLX_AREA_ANOM(float, false);
  }
#undef MLX_AREA_ANOM
  return hip_status(hipGetLastError(), "k_area_anomaly launch");
}
