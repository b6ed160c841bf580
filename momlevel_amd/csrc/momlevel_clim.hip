// momlevel_clim.hip -- a NaN-skipping statistic over groups of time steps of a (time, cells)
// record, one result row per group (include/momlevel_clim.h):
//
//   util.monthly_average  (src/momlevel/util.py:454-511)   groupby year, groupby month, .mean
//   util.annual_cycle     (src/momlevel/util.py:122-196)   groupby month, .mean/.std/.min/.max
//
// The reference does these through xarray's groupby on one CPU thread.  Here a group is a list of
// time indices (steps[offsets[g] .. offsets[g + 1])): calendar months of a daily record have 28 to
// 31 steps, the steps of "all Januaries" lie 12 rows apart.  A lane owns a pack of horizontally
// adjacent cells (16-byte nontemporal loads: two float64 or four float32) and walks ONE group in
// the order steps[] lists it, with kClimUnroll row loads in flight ahead of the dependent adds:
// the add chain is sequential by contract (bit-identical to numpy's nanmean / nanstd over axis 0).
// The step indices are wave-uniform and come through the scalar cache, one batch ahead of the
// rows they address.  MEAN, MIN and MAX read every selected element once (8 B, 4 B at float32,
// per cell-step); STD reads the group twice (mean, then squared deviations), as numpy does.
//
// grid = (cell tiles, min(ngroups, 65535)); a block loops over g = blockIdx.y, += gridDim.y, so
// any number of groups works (a daily record with one group per step has more than 65535).  No
// group is ever split between threads and there are no atomics: results do not depend on the
// launch geometry or on how a caller blocks the cells.
//
// Cells that do not fill a pack (n not a multiple of it, or rows that are then not 16-byte
// aligned) are handled by the narrower instantiations, down to one cell per lane.
//
// Compile: with momlevel_hip.hip (csrc/build.py), -ffp-contract=off -- STD's d * d and the add
// that follows must stay two operations.  Not part of the kernel sources whose hash guards the
// committed steric profiles (build.clim_source_sha is this file's).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/momlevel_hip.h"
#include "../../include/momlevel_clim.h"
#include "mlx_record.hpp"

#pragma clang fp contract(off)

namespace mlx {
namespace {

constexpr int kClimBlock = 256;  // 4 waves of 64
constexpr int kClimUnroll = 8;   // row packs a lane has in flight
constexpr unsigned kClimMaxGridY = 65535;

// Visit the rows steps[lo .. hi) in order: kClimUnroll loads are issued before the first of them
// is consumed, and the next batch of step indices is fetched before the loads of this one.  Rows
// move with the `nt` policy (a group is read once, twice for STD) and every index is tested.
// (momlevel_quantile.hip's walk_rows is another loop -- no index prefetch, a hook after each batch,
// a mode without a list -- and one loop for both would branch on its caller.)
template <typename TIn, int V, typename F>
__device__ __forceinline__ void walk_group(const TIn* __restrict__ ycol,
                                           const int32_t* __restrict__ steps, int64_t lo, int64_t hi,
                                           int64_t nt, int64_t n, F&& consume) {
  constexpr int U = kClimUnroll;
  int64_t j = lo;
  if (j + U <= hi) {
    int32_t cur[U];
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = steps[j + u];
    for (; j + U <= hi; j += U) {
      int32_t nxt[U];
      const int64_t ahead = j + 2 * U <= hi ? j + U : j;  // (the last batch re-reads itself)
#pragma unroll
      for (int u = 0; u < U; ++u) nxt[u] = steps[ahead + u];
      Row<TIn, V> r[U];
#pragma unroll
      for (int u = 0; u < U; ++u) r[u] = row_load<TIn, V, true, true>(ycol, cur[u], nt, n);
#pragma unroll
      for (int u = 0; u < U; ++u) consume(r[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
  }
  for (; j < hi; ++j) consume(row_load<TIn, V, true, true>(ycol, steps[j], nt, n));
}

// ------------------------------------------------------------------------------------------
// k_group_stat: out[g][cell] = STAT over the steps of group g.  n % V == 0.
// ------------------------------------------------------------------------------------------
template <typename TIn, int V, int STAT>
__global__ __launch_bounds__(kClimBlock) void k_group_stat(const TIn* __restrict__ y,
                                                           const int32_t* __restrict__ steps,
                                                           const int64_t* __restrict__ offsets,
                                                           int64_t nsel, int64_t ngroups, int64_t nt,
                                                           int64_t n, TIn* __restrict__ out) {
  const int64_t i = ((int64_t)blockIdx.x * kClimBlock + threadIdx.x) * V;
  if (i >= n) return;
  const TIn* ycol = y + i;
  for (int64_t g = blockIdx.y; g < ngroups; g += gridDim.y) {
    int64_t lo, hi;
    group_bounds(offsets, g, nsel, lo, hi);
    double res[V];
    if constexpr (STAT == MLX_STAT_MEAN || STAT == MLX_STAT_STD) {
      // -0.0 + x is x for every x, and -0.0 + (+0.0) is +0.0: the sum starts as the first step's
      // value, or as +0.0 when that is NaN -- numpy's sum over the NaN-zeroed rows
      double acc[V], cnt[V];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        acc[k] = -0.0;
        cnt[k] = 0.0;
      }
      walk_group<TIn, V>(ycol, steps, lo, hi, nt, n, [&](const Row<TIn, V>& r) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const double yv = r.at(k);
          const bool bad = is_nan(yv);
          acc[k] += bad ? 0.0 : yv;
          cnt[k] += bad ? 0.0 : 1.0;
        }
      });
#pragma unroll
      for (int k = 0; k < V; ++k) res[k] = cnt[k] == 0.0 ? canonical_nan() : acc[k] / cnt[k];
      if constexpr (STAT == MLX_STAT_STD) {
        double ss[V];
#pragma unroll
        for (int k = 0; k < V; ++k) ss[k] = 0.0;
        walk_group<TIn, V>(ycol, steps, lo, hi, nt, n, [&](const Row<TIn, V>& r) {
#pragma unroll
          for (int k = 0; k < V; ++k) {
            const double yv = r.at(k);
            const double d = yv - res[k];
            const double sq = d * d;
            ss[k] += is_nan(yv) ? 0.0 : sq;
          }
        });
#pragma unroll
        for (int k = 0; k < V; ++k)
          res[k] = cnt[k] == 0.0 ? canonical_nan() : __dsqrt_rn(ss[k] / cnt[k]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) res[k] = canonical_nan();
      walk_group<TIn, V>(ycol, steps, lo, hi, nt, n, [&](const Row<TIn, V>& r) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const double yv = r.at(k);
          const bool better = STAT == MLX_STAT_MIN ? yv < res[k] : yv > res[k];  // false for NaN yv
          res[k] = (better || (is_nan(res[k]) && !is_nan(yv))) ? yv : res[k];
        }
      });
    }
    Pack<TIn, V> o;
#pragma unroll
    for (int k = 0; k < V; ++k) o.v[k] = narrow<TIn>(res[k], is_nan(res[k]));
    store_pack<TIn, V, false>(out + g * n + i, o);
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
using detail::fail;
using detail::hip_status;

template <typename TIn, int V, int STAT>
int launch_stat(const void* y, const int32_t* steps, const int64_t* offsets, int64_t nsel,
                int64_t ngroups, int64_t nt, int64_t n, void* out, hipStream_t st) {
  const unsigned gy = ngroups < (int64_t)kClimMaxGridY ? (unsigned)ngroups : kClimMaxGridY;
  dim3 grid((unsigned)ceil_div(n, (int64_t)kClimBlock * V), gy);
  hipLaunchKernelGGL((k_group_stat<TIn, V, STAT>), grid, dim3(kClimBlock), 0, st, (const TIn*)y,
                     steps, offsets, nsel, ngroups, nt, n, (TIn*)out);
  return hip_status(hipGetLastError(), "k_group_stat launch");
}

template <typename TIn, int V>
int launch_any(int stat, const void* y, const int32_t* steps, const int64_t* offsets, int64_t nsel,
               int64_t ngroups, int64_t nt, int64_t n, void* out, hipStream_t st) {
  switch (stat) {
    case MLX_STAT_MEAN:
      return launch_stat<TIn, V, MLX_STAT_MEAN>(y, steps, offsets, nsel, ngroups, nt, n, out, st);
    case MLX_STAT_STD:
      return launch_stat<TIn, V, MLX_STAT_STD>(y, steps, offsets, nsel, ngroups, nt, n, out, st);
    case MLX_STAT_MIN:
      return launch_stat<TIn, V, MLX_STAT_MIN>(y, steps, offsets, nsel, ngroups, nt, n, out, st);
    default:
      return launch_stat<TIn, V, MLX_STAT_MAX>(y, steps, offsets, nsel, ngroups, nt, n, out, st);
  }
}

}  // namespace
}  // namespace mlx

using namespace mlx;

extern "C" {

int mlx_clim_group_stat(const void* y, int dtype, const int32_t* steps, const int64_t* offsets,
                        int64_t nsel, int64_t ngroups, int64_t nt, int64_t n, int stat, void* out,
                        void* stream) {
  if (!y || !steps || !offsets || !out)
    return fail(MLX_E_NULL, "y, steps, offsets, out must not be NULL");
  if (stat < MLX_STAT_MEAN || stat > MLX_STAT_MAX) return fail(MLX_E_ENUM, "unknown MLX_STAT_* stat");
  if (int rc = check_grouped(y, dtype, steps, offsets, nsel, ngroups, nt, n, 1)) return rc;
  const size_t elem = dtype_size(dtype);
  if (!aligned(out, elem)) return fail(MLX_E_ALIGN, "out not element-aligned");
  hipStream_t st = (hipStream_t)stream;
  const int v = pack_width(n, elem, {{y, elem}, {out, elem}});
  return dispatch_pack(dtype, v, [&](auto t, auto w) {
    return launch_any<typename decltype(t)::type, decltype(w)::value>(stat, y, steps, offsets, nsel,
                                                                      ngroups, nt, n, out, st);
  });
}

}  // extern "C"
