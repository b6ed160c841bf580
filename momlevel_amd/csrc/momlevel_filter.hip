// momlevel_filter.hip -- a banded linear operator along the time axis of a (time, cells) record
// (include/momlevel_filter.h):
//
//   out[t] = sum_k w[t, k] * y[t - lead + k],  k = 0 .. W-1,  NaN-aware
//
// EXTENSION: momlevel has no such function.  Rolling means and sums, Lanczos low-pass filters, FIR
// weights and running least-squares slopes are this operator with weight tables made on the host
// (momlevel_amd/filters.py).
//
// A lane owns a pack of horizontally adjacent cells (16 bytes of y: two float64 or four float32)
// and a TILE of kFilterSteps consecutive output steps at a time.  It walks the W + tile - 1 rows
// the tile's windows cover ONCE, in time order, and every row is added into each output of the
// tile whose window holds it, with that output's own weight: for one output the rows arrive with
// k ascending, so each output is the sequential sum of the contract, summed afresh -- nothing is
// carried from one output to the next.  A row is therefore loaded (W + tile - 1) / tile times per
// output instead of W times; the rows a lane reads again for its next tile are the ones it has
// just read (L2 at the latest).  The weights are wave-uniform and come through the scalar cache.
//
// The walk over a tile's rows has three parts: a head of tile - 1 rows that serve the first
// outputs only, a middle of W - tile + 1 rows that serve every output of the tile (no window test;
// kFilterUnroll row loads in flight), and a tail of tile - 1 rows that serve the last outputs only.
// W < tile has no middle.  mlx_filter_window_edge reports where that changes.
//
// grid = (cell tiles, time chunks): a block walks a run of consecutive tiles.  How many chunks
// there are is a matter of occupancy alone: no output is ever split between threads and there are
// no atomics, so results depend neither on the launch geometry nor on how a caller blocks the cells.
// mlx_filter_tiles_per_block reports the length of a block's run.
//
// Cells that do not fill a pack (n not a multiple of it, or rows that are then not aligned) are
// handled by the narrower instantiations, down to one cell per lane.
//
// Compile: with momlevel_hip.hip (csrc/build.py), -ffp-contract=off -- w * y and the add that
// follows must stay two operations.  Not part of the kernel sources whose hash guards the committed
// steric profiles (build.filter_source_sha is this file's).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/momlevel_hip.h"
#include "../../include/momlevel_filter.h"
#include "mlx_record.hpp"

#pragma clang fp contract(off)

namespace mlx {
namespace {

constexpr int kFilterBlock = 256;  // 4 waves of 64
constexpr int kFilterSteps = 8;    // output steps of a tile
constexpr int kFilterUnroll = 4;   // row packs in flight in the middle of a tile's walk
constexpr unsigned kFilterMaxGridY = 65535;
constexpr int64_t kFilterTargetBlocks = 8192;  // blocks a launch aims at before it stops cutting time

// The row of step s, widened to float64; a step outside [0, nt) is a NaN row and is not loaded.
// s is wave-uniform.  (Not mlx_record.hpp's Row: that one loads row 0 for such a step, and here the
// steps before and after the record are the ordinary case, at every edge tile.)
template <typename TIn, int V>
struct FRow {
  Pack<TIn, V> raw;
  bool ok;
  __device__ __forceinline__ double at(int c) const {
    return ok ? (double)raw.v[c] : canonical_nan();  // float32 -> float64 is exact
  }
};

template <typename TIn, int V>
__device__ __forceinline__ FRow<TIn, V> frow_load(const TIn* __restrict__ ycol, int32_t s,
                                                  int32_t nt, int64_t n) {
  FRow<TIn, V> r;
  r.ok = (uint32_t)s < (uint32_t)nt;
  if (r.ok) {
    r.raw = load_pack<TIn, V, false>(ycol + (int64_t)s * n);  // (read again by the next tile)
  } else {
#pragma unroll
    for (int c = 0; c < V; ++c) r.raw.v[c] = (TIn)0;
  }
  return r;
}

template <int V>
struct FAcc {
  double acc[kFilterSteps][V];
  double ws[kFilterSteps][V];
  int32_t cnt[kFilterSteps][V];
};

// Row j of a tile's walk (step t0 - lead + j) into every output r of the tile whose window holds
// it: tap k = j - r.  CHECK: test 0 <= k < W (wave-uniform); without it the caller guarantees it.
template <typename TIn, int V, bool NORM, bool CHECK>
__device__ __forceinline__ void serve(const FRow<TIn, V>& row, int32_t j, int32_t W,
                                      const double* const (&wrow)[kFilterSteps], FAcc<V>& a) {
#pragma unroll
  for (int r = 0; r < kFilterSteps; ++r) {
    const int32_t k = j - r;
    if (!CHECK || (uint32_t)k < (uint32_t)W) {
      const double wk = wrow[r][k];
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const double yv = row.at(c);
        const bool valid = !is_nan(yv);
        const double p = wk * yv;
        a.acc[r][c] += valid ? p : 0.0;
        if constexpr (NORM) a.ws[r][c] += valid ? wk : 0.0;
        a.cnt[r][c] += valid ? 1 : 0;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// k_time_filter: n % V == 0; per = tiles per block along time
// ------------------------------------------------------------------------------------------
template <typename TIn, typename TOut, int V, bool NORM>
__global__ __launch_bounds__(kFilterBlock) void k_time_filter(
    const TIn* __restrict__ y, const double* __restrict__ w, int32_t W, int64_t w_stride,
    int32_t lead, int32_t min_count, int32_t nt, int64_t n, int32_t per, TOut* __restrict__ out) {
  constexpr int R = kFilterSteps, U = kFilterUnroll;
  const int64_t i = ((int64_t)blockIdx.x * kFilterBlock + threadIdx.x) * V;
  if (i >= n) return;
  const TIn* ycol = y + i;
  const int32_t ntiles = (nt + R - 1) / R;
  const int32_t b0 = (int32_t)blockIdx.y * per;
  const int32_t b1 = b0 + per < ntiles ? b0 + per : ntiles;
  const int32_t mid_end = W > R - 1 ? W : R - 1;  // first row of the tail
  const int32_t jend = W + R - 1;
  for (int32_t b = b0; b < b1; ++b) {
    const int32_t t0 = b * R;
    const int32_t s0 = t0 - lead;
    const double* wrow[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int32_t t = t0 + r < nt ? t0 + r : nt - 1;  // (outputs past the record are not stored)
      wrow[r] = w + (int64_t)t * w_stride;
    }
    FAcc<V> a;
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int c = 0; c < V; ++c) {
        a.acc[r][c] = -0.0;  // -0.0 + x is x for every x, and -0.0 + (+0.0) is +0.0
        a.ws[r][c] = 0.0;
        a.cnt[r][c] = 0;
      }
    }
    {  // head: rows 0 .. R-2 serve the outputs r <= j
      FRow<TIn, V> rows[R - 1];
#pragma unroll
      for (int j = 0; j < R - 1; ++j) rows[j] = frow_load<TIn, V>(ycol, s0 + j, nt, n);
#pragma unroll
      for (int j = 0; j < R - 1; ++j) serve<TIn, V, NORM, true>(rows[j], j, W, wrow, a);
    }
    int32_t j = R - 1;
    for (; j + U <= mid_end; j += U) {  // middle: rows that serve every output of the tile
      FRow<TIn, V> rows[U];
#pragma unroll
      for (int u = 0; u < U; ++u) rows[u] = frow_load<TIn, V>(ycol, s0 + j + u, nt, n);
#pragma unroll
      for (int u = 0; u < U; ++u) serve<TIn, V, NORM, false>(rows[u], j + u, W, wrow, a);
    }
    for (; j < mid_end; ++j)
      serve<TIn, V, NORM, false>(frow_load<TIn, V>(ycol, s0 + j, nt, n), j, W, wrow, a);
    {  // tail: rows mid_end .. W+R-2 serve the outputs r > j - W
      FRow<TIn, V> rows[R - 1];
#pragma unroll
      for (int q = 0; q < R - 1; ++q)
        rows[q] = frow_load<TIn, V>(ycol, mid_end + q < jend ? s0 + mid_end + q : -1, nt, n);
#pragma unroll
      for (int q = 0; q < R - 1; ++q) serve<TIn, V, NORM, true>(rows[q], mid_end + q, W, wrow, a);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (t0 + r < nt) {
        Pack<TOut, V> o;
#pragma unroll
        for (int c = 0; c < V; ++c) {
          double res = NORM ? a.acc[r][c] / a.ws[r][c] : a.acc[r][c];
          o.v[c] = narrow<TOut>(res, a.cnt[r][c] < min_count || is_nan(res));
        }
        store_pack<TOut, V, true>(out + (int64_t)(t0 + r) * n + i, o);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
using detail::fail;
using detail::hip_status;

constexpr int64_t kMaxSteps = (int64_t)1 << 30;  // (t - lead + k stays inside int32)

struct FilterArgs {
  const void* y;
  const double* w;
  int32_t W;
  int64_t w_stride;
  int32_t lead, min_count, nt;
  int64_t n;
  void* out;
  hipStream_t st;
};

// Consecutive time tiles a block walks (the kernel's `per`) for v cells a lane: the one rule, which
// mlx_filter_tiles_per_block reports and launch_filter launches by.
inline int64_t filter_tiles_per_block(int64_t nt, int64_t n, int v) {
  const int64_t gx = ceil_div(n, (int64_t)kFilterBlock * v);
  const int64_t ntiles = ceil_div(nt, kFilterSteps);
  int64_t gy = ceil_div(kFilterTargetBlocks, gx);
  gy = gy > ntiles ? ntiles : gy;
  gy = gy > (int64_t)kFilterMaxGridY ? (int64_t)kFilterMaxGridY : gy;
  return ceil_div(ntiles, gy);
}

template <typename TIn, typename TOut, int V, bool NORM>
int launch_filter(const FilterArgs& a) {
  const int64_t gx = ceil_div(a.n, (int64_t)kFilterBlock * V);
  const int64_t ntiles = ceil_div(a.nt, kFilterSteps);
  const int64_t per = filter_tiles_per_block(a.nt, a.n, V);
  const int64_t gy = ceil_div(ntiles, per);
  hipLaunchKernelGGL((k_time_filter<TIn, TOut, V, NORM>), dim3((unsigned)gx, (unsigned)gy),
                     dim3(kFilterBlock), 0, a.st, (const TIn*)a.y, a.w, a.W, a.w_stride, a.lead,
                     a.min_count, a.nt, a.n, (int32_t)per, (TOut*)a.out);
  return hip_status(hipGetLastError(), "k_time_filter launch");
}

template <typename TIn, typename TOut, int V>
int launch_norm(bool norm, const FilterArgs& a) {
  return norm ? launch_filter<TIn, TOut, V, true>(a) : launch_filter<TIn, TOut, V, false>(a);
}

}  // namespace
}  // namespace mlx

using namespace mlx;

extern "C" {

int64_t mlx_filter_tile(void) { return kFilterSteps; }

int64_t mlx_filter_window_edge(int i) {
  // W = tile: the first window with a middle row; W = tile + unroll - 1: the first with a batch
  if (i == 0) return kFilterSteps;
  if (i == 1) return kFilterSteps + kFilterUnroll - 1;
  return 0;
}

int64_t mlx_filter_tiles_per_block(int64_t nt, int64_t n, int cells_per_lane) {
  if (!record_fits(nt, n, kMaxSteps)) return 0;
  if (cells_per_lane != 1 && cells_per_lane != 2 && cells_per_lane != 4) return 0;
  if (n % cells_per_lane != 0) return 0;  // (no launch has lanes that wide)
  return filter_tiles_per_block(nt, n, cells_per_lane);
}

int mlx_filter_apply(const void* y, int dtype, const double* w, int64_t W, int64_t w_stride,
                    int64_t lead, int64_t min_count, int flags, int64_t nt, int64_t n, void* out,
                    int out_dtype, void* stream) {
  if (!y || !w || !out) return fail(MLX_E_NULL, "y, w, out must not be NULL");
  if (!is_float_dtype(dtype) || !is_float_dtype(out_dtype))
    return fail(MLX_E_ENUM, "dtype and out_dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  if (flags & ~MLX_FILTER_NORMALISE) return fail(MLX_E_ENUM, "unknown MLX_FILTER_* flag");
  if (!record_fits(nt, n, kMaxSteps))
    return fail(MLX_E_SHAPE, "need 0 < nt < 2^30, 0 < n <= 2^38, nt*n addressable");
  if (W < 1 || W > nt) return fail(MLX_E_SHAPE, "need 1 <= W <= nt");
  if (lead < 0 || lead >= W) return fail(MLX_E_SHAPE, "need 0 <= lead < W");
  if (min_count < 1 || min_count > W) return fail(MLX_E_SHAPE, "need 1 <= min_count <= W");
  if (w_stride != 0 && w_stride != W) return fail(MLX_E_SHAPE, "w_stride must be 0 or W");
  const size_t elem = dtype_size(dtype), oelem = dtype_size(out_dtype);
  if (!aligned(y, elem) || !aligned(out, oelem)) return fail(MLX_E_ALIGN, "y / out not element-aligned");
  if (!aligned(w, 8)) return fail(MLX_E_ALIGN, "w not 8-byte aligned");
  const int v = pack_width(n, elem, {{y, elem}, {out, oelem}});
  const FilterArgs a{y, w, (int32_t)W, w_stride, (int32_t)lead, (int32_t)min_count, (int32_t)nt, n,
                     out, (hipStream_t)stream};
  const bool norm = (flags & MLX_FILTER_NORMALISE) != 0;
  return dispatch_pack(dtype, v, [&](auto t, auto width) {
    typedef typename decltype(t)::type TIn;
    constexpr int V = decltype(width)::value;
    return out_dtype == MLX_DTYPE_F64 ? launch_norm<TIn, double, V>(norm, a)
                                      : launch_norm<TIn, float, V>(norm, a);
  });
}

}  // extern "C"
