// momlevel_quantile.hip -- NaN-skipping quantiles over groups of time steps of a (time, cells)
// record, and the count of steps above a per-cell threshold (include/momlevel_quantile.h).
// EXTENSION: momlevel has no such function; numpy.nanquantile(method="linear") is the authority.
//
// A quantile is a selection, not a sum: the kernel finds the lo-th smallest valid value of a cell
// by most-significant-digit radix select on the order-preserving key of its bits
// (bits ^ (sign ? ~0 : signbit); NaN left out), four bits a pass.  A lane owns a pack of
// horizontally adjacent cells (16 bytes: two float64 or four float32) from the first pass to the
// last.  Each pass walks the group's rows once, kQuantUnroll row loads in flight, and counts the 16
// values of the next digit among the values that match the cell's prefix so far, in 16 register
// counters per cell; the lane then picks the digit in which its rank falls, extends the prefix and
// reduces the rank.  The first pass's counters also sum to c, the number of valid steps, so the
// rank lo = floor((c - 1) q) is known before any digit is chosen.  16 passes for float64, 8 for
// float32 (whose order is that of the widened values), and one closing pass that counts the keys
// <= key(a) and takes the smallest key above it: b = a when hi < that count, else that minimum --
// both order statistics from one selection.  The lerp is numpy's, in float64.
//
// Prefix, rank and counters stay in registers: no workspace, no LDS, no atomics, no cross-lane
// traffic, so the results depend neither on the launch geometry nor on how the cells are split
// between calls.  A runtime-indexed register array would live in scratch, and 16 compare-and-adds
// per value make the float32 four-pack VALU-bound; so a value adds one to a 4-bit field of a packed
// word, and the fields are spread into the 32-bit counters once per batch of rows.
//
// grid = (cell tiles, nq, min(ngroups, 65535)); a block loops over g = blockIdx.z, += gridDim.z.
// Each (group, q) re-reads its rows.  Element offsets are 64-bit: t * n passes 2^31 on the records
// this is for.
//
// Cells that do not fill a pack (n not a multiple of it, or rows that are then not 16-byte
// aligned) go to the narrower instantiations, down to one cell per lane.
//
// Compile: with momlevel_hip.hip (csrc/build.py), -ffp-contract=off -- the lerp's d * g and the
// add that follows must stay two operations.  build.quantile_source_sha is this file's guard.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/momlevel_hip.h"
#include "../../include/momlevel_quantile.h"
#include "mlx_record.hpp"

#pragma clang fp contract(off)

namespace mlx {
namespace {

constexpr int kQuantBlock = 256;  // 4 waves of 64
constexpr int kQuantUnroll = 8;   // row packs a lane has in flight
constexpr unsigned kQuantMaxGridZ = 65535;
constexpr int kDigitBits = 4, kDigits = 1 << kDigitBits;
static_assert(kDigits == 16 && kQuantUnroll < 16, "a 4-bit field holds the rows of one batch");

struct QList {
  double v[MLX_QUANTILE_MAX_Q];
};

// ---- the order-preserving key of a value's bits, and back
template <typename T>
struct Key;
template <>
struct Key<double> {
  typedef uint64_t type;
  static constexpr int bits = 64;
  static __device__ __forceinline__ type of(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return b ^ ((b >> 63) ? ~0ULL : 0x8000000000000000ULL);
  }
  static __device__ __forceinline__ double value(type k) {
    const uint64_t b = k ^ ((k >> 63) ? 0x8000000000000000ULL : ~0ULL);
    return __longlong_as_double((long long)b);
  }
};
template <>
struct Key<float> {
  typedef uint32_t type;
  static constexpr int bits = 32;
  static __device__ __forceinline__ type of(float v) {
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? ~0U : 0x80000000U);
  }
  static __device__ __forceinline__ double value(type k) {
    const uint32_t b = k ^ ((k >> 31) ? 0x80000000U : ~0U);
    return (double)__uint_as_float(b);  // float32 -> float64 is exact
  }
};

// Visit the rows steps[lo .. hi) (LISTED) or lo .. hi themselves: kQuantUnroll loads are issued
// before the first of them is consumed.  after_batch() runs once at least every kQuantUnroll rows
// and after the last one.  The order does not matter to a count.  Rows stay cached: every pass
// reads them again.  Unlisted, s walks [0, nt) itself and is not tested.
// (momlevel_clim.hip's walk_group is another loop -- it prefetches the next batch of indices and
// has neither the hook nor the unlisted mode -- and one loop for both would branch on its caller.)
template <typename TIn, int V, bool LISTED, typename F, typename B>
__device__ __forceinline__ void walk_rows(const TIn* __restrict__ ycol,
                                          const int32_t* __restrict__ steps, int64_t lo, int64_t hi,
                                          int64_t nt, int64_t n, F&& consume, B&& after_batch) {
  constexpr int U = kQuantUnroll;
  int64_t j = lo;
  for (; j + U <= hi; j += U) {
    int32_t s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) s[u] = LISTED ? steps[j + u] : (int32_t)(j + u);
    Row<TIn, V> r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) r[u] = row_load<TIn, V, false, LISTED>(ycol, s[u], nt, n);
#pragma unroll
    for (int u = 0; u < U; ++u) consume(r[u]);
    after_batch();
  }
  for (; j < hi; ++j)
    consume(row_load<TIn, V, false, LISTED>(ycol, LISTED ? steps[j] : (int32_t)j, nt, n));
  after_batch();
}

// the bounds of group g: clamped to the list, or every row
template <bool LISTED>
__device__ __forceinline__ void group_rows(const int64_t* __restrict__ offsets, int64_t g,
                                           int64_t nsel, int64_t nt, int64_t& lo, int64_t& hi) {
  if constexpr (LISTED) {
    group_bounds(offsets, g, nsel, lo, hi);
  } else {
    lo = 0;
    hi = nt;
  }
}

// numpy 2.2's "linear": the two ranks and gamma of c >= 1 valid values
__device__ __forceinline__ void lerp_plan(uint32_t c, double q, uint32_t& lo, uint32_t& hi, double& g) {
  const double top = (double)(c - 1u);
  const double vi = top * q;
  if (vi >= top) {
    lo = hi = c - 1u;
    g = vi - (-1.0);
  } else if (vi < 0.0) {
    lo = hi = 0u;
    g = vi - 0.0;
  } else {
    const double f = floor(vi);
    lo = (uint32_t)f;
    hi = lo + 1u;
    g = vi - f;
  }
}

// ------------------------------------------------------------------------------------------
// k_quantile_select: out[qi][g][cell] = quantile q[qi] over the steps of group g.  n % V == 0.
// ------------------------------------------------------------------------------------------
template <typename TIn, int V, bool LISTED>
__global__ __launch_bounds__(kQuantBlock) void k_quantile_select(
    const TIn* __restrict__ y, const int32_t* __restrict__ steps, const int64_t* __restrict__ offsets,
    int64_t nsel, int64_t ngroups, int64_t nt, int64_t n, QList qs, TIn* __restrict__ out) {
  typedef typename Key<TIn>::type K;
  constexpr int KB = Key<TIn>::bits, NP = KB / kDigitBits;
  const int64_t i = ((int64_t)blockIdx.x * kQuantBlock + threadIdx.x) * V;
  if (i >= n) return;
  const TIn* ycol = y + i;
  const int qi = blockIdx.y;
  double q = qs.v[0];
#pragma unroll
  for (int j = 1; j < MLX_QUANTILE_MAX_Q; ++j) q = qi == j ? qs.v[j] : q;
  for (int64_t g = blockIdx.z; g < ngroups; g += gridDim.z) {
    int64_t lo, hi;
    group_rows<LISTED>(offsets, g, nsel, nt, lo, hi);
    K prefix[V];
    uint32_t rank[V], c[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      prefix[k] = 0;
      rank[k] = 0;
      c[k] = 0;
    }
    for (int p = 0; p < NP; ++p) {
      const int shift = KB - kDigitBits * (p + 1);
      // the digits above this pass's: none in the first pass (a shift by KB is not defined)
      const K himask = p == 0 ? (K)0 : (K)(~(K)0 << (shift + kDigitBits));
      uint32_t cnt[V][kDigits];
#pragma unroll
      for (int k = 0; k < V; ++k)
#pragma unroll
        for (int d = 0; d < kDigits; ++d) cnt[k][d] = 0;
      // Between two flushes a value adds one to a 4-bit field of one of two packed words (digits
      // 0..7 and 8..15): at most kQuantUnroll < 16 rows go by before the fields are added into the
      // sixteen 32-bit counters, so no field overflows.
      uint32_t nib[V][2];
#pragma unroll
      for (int k = 0; k < V; ++k) nib[k][0] = nib[k][1] = 0;
      walk_rows<TIn, V, LISTED>(
          ycol, steps, lo, hi, nt, n,
          [&](const Row<TIn, V>& r) {
#pragma unroll
            for (int k = 0; k < V; ++k) {
              const K key = Key<TIn>::of(r.raw.v[k]);
              const bool in = r.valid(k) && ((key ^ prefix[k]) & himask) == 0;
              const uint32_t digit = (uint32_t)(key >> shift) & (kDigits - 1);
              const uint32_t one = 1u << ((digit & 7u) * 4u);
              nib[k][0] += (in && digit < 8u) ? one : 0u;
              nib[k][1] += (in && digit >= 8u) ? one : 0u;
            }
          },
          [&]() {
#pragma unroll
            for (int k = 0; k < V; ++k) {
#pragma unroll
              for (int d = 0; d < 8; ++d) {
                cnt[k][d] += (nib[k][0] >> (4 * d)) & 15u;
                cnt[k][8 + d] += (nib[k][1] >> (4 * d)) & 15u;
              }
              nib[k][0] = nib[k][1] = 0;
            }
          });
#pragma unroll
      for (int k = 0; k < V; ++k) {
        if (p == 0) {
          uint32_t sum = 0;
#pragma unroll
          for (int d = 0; d < kDigits; ++d) sum += cnt[k][d];
          c[k] = sum;
          uint32_t hi_rank;
          double gam;
          lerp_plan(sum == 0 ? 1u : sum, q, rank[k], hi_rank, gam);
        }
        uint32_t run = 0, chosen = 0, left = rank[k];
        bool found = false;
#pragma unroll
        for (int d = 0; d < kDigits; ++d) {
          const uint32_t next = run + cnt[k][d];
          const bool here = !found && rank[k] < next;
          chosen = here ? (uint32_t)d : chosen;
          left = here ? rank[k] - run : left;
          found = found || here;
          run = next;
        }
        rank[k] = left;
        prefix[k] |= (K)chosen << shift;
      }
    }
    // the closing pass: prefix is key(a).  How many keys are <= it, and the smallest above it
    uint32_t le[V];
    K above[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      le[k] = 0;
      above[k] = ~(K)0;
    }
    walk_rows<TIn, V, LISTED>(ycol, steps, lo, hi, nt, n, [&](const Row<TIn, V>& r) {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const K key = Key<TIn>::of(r.raw.v[k]);
        const bool ok = r.valid(k);
        const bool below = key <= prefix[k];
        le[k] += (ok && below) ? 1u : 0u;
        above[k] = (ok && !below && key < above[k]) ? key : above[k];
      }
    }, [] {});
    Pack<TIn, V> o;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      uint32_t lo_rank, hi_rank;
      double gam;
      lerp_plan(c[k] == 0 ? 1u : c[k], q, lo_rank, hi_rank, gam);
      const double a = Key<TIn>::value(prefix[k]);
      const double b = hi_rank < le[k] ? a : Key<TIn>::value(above[k]);
      const double d = b - a;
      double res = a + d * gam;
      if (gam >= 0.5) res = b - d * (1.0 - gam);
      o.v[k] = narrow<TIn>(res, c[k] == 0 || is_nan(res));
    }
    store_pack<TIn, V, false>(out + ((int64_t)qi * ngroups + g) * n + i, o);
  }
}

// ------------------------------------------------------------------------------------------
// k_exceed_count: out[g][cell] = #{steps of group g : y > thr[g][cell]}.  n % V == 0.
// ------------------------------------------------------------------------------------------
template <typename TIn, int V, bool LISTED>
__global__ __launch_bounds__(kQuantBlock) void k_exceed_count(
    const TIn* __restrict__ y, const int32_t* __restrict__ steps, const int64_t* __restrict__ offsets,
    int64_t nsel, int64_t ngroups, int64_t nt, int64_t n, const double* __restrict__ thr,
    int64_t* __restrict__ out) {
  const int64_t i = ((int64_t)blockIdx.x * kQuantBlock + threadIdx.x) * V;
  if (i >= n) return;
  const TIn* ycol = y + i;
  for (int64_t g = blockIdx.z; g < ngroups; g += gridDim.z) {
    int64_t lo, hi;
    group_rows<LISTED>(offsets, g, nsel, nt, lo, hi);
    const Pack<double, V> t = load_pack<double, V, false>(thr + g * n + i);
    Pack<int64_t, V> cnt;
#pragma unroll
    for (int k = 0; k < V; ++k) cnt.v[k] = 0;
    walk_rows<TIn, V, LISTED>(ycol, steps, lo, hi, nt, n, [&](const Row<TIn, V>& r) {
#pragma unroll
      for (int k = 0; k < V; ++k)
        cnt.v[k] += (r.ok && (double)r.raw.v[k] > t.v[k]) ? 1 : 0;  // false for NaN on either side
    }, [] {});
    store_pack<int64_t, V, false>(out + g * n + i, cnt);
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
using detail::fail;
using detail::hip_status;

dim3 quant_grid(int64_t n, int v, int nq, int64_t ngroups) {
  const unsigned gz = ngroups < (int64_t)kQuantMaxGridZ ? (unsigned)ngroups : kQuantMaxGridZ;
  return dim3((unsigned)ceil_div(n, (int64_t)kQuantBlock * v), (unsigned)nq, gz);
}

template <typename TIn, int V>
int launch_select(const void* y, const int32_t* steps, const int64_t* offsets, int64_t nsel,
                  int64_t ngroups, int64_t nt, int64_t n, const QList& qs, int nq, void* out,
                  hipStream_t st) {
  const dim3 grid = quant_grid(n, V, nq, ngroups);
  if (steps)
    hipLaunchKernelGGL((k_quantile_select<TIn, V, true>), grid, dim3(kQuantBlock), 0, st,
                       (const TIn*)y, steps, offsets, nsel, ngroups, nt, n, qs, (TIn*)out);
  else
    hipLaunchKernelGGL((k_quantile_select<TIn, V, false>), grid, dim3(kQuantBlock), 0, st,
                       (const TIn*)y, steps, offsets, nsel, ngroups, nt, n, qs, (TIn*)out);
  return hip_status(hipGetLastError(), "k_quantile_select launch");
}

template <typename TIn, int V>
int launch_exceed(const void* y, const int32_t* steps, const int64_t* offsets, int64_t nsel,
                  int64_t ngroups, int64_t nt, int64_t n, const double* thr, int64_t* out,
                  hipStream_t st) {
  const dim3 grid = quant_grid(n, V, 1, ngroups);
  if (steps)
    hipLaunchKernelGGL((k_exceed_count<TIn, V, true>), grid, dim3(kQuantBlock), 0, st,
                       (const TIn*)y, steps, offsets, nsel, ngroups, nt, n, thr, out);
  else
    hipLaunchKernelGGL((k_exceed_count<TIn, V, false>), grid, dim3(kQuantBlock), 0, st,
                       (const TIn*)y, steps, offsets, nsel, ngroups, nt, n, thr, out);
  return hip_status(hipGetLastError(), "k_exceed_count launch");
}

}  // namespace
}  // namespace mlx

using namespace mlx;

extern "C" {

int64_t mlx_quantile_block_cells(int dtype) {
  return is_float_dtype(dtype) ? (int64_t)kQuantBlock * (int64_t)(16 / dtype_size(dtype)) : 0;
}

int64_t mlx_quantile_unroll(void) { return kQuantUnroll; }

int mlx_quantile_select(const void* y, int dtype, const int32_t* steps, const int64_t* offsets,
                        int64_t nsel, int64_t ngroups, int64_t nt, int64_t n, const double* q,
                        int nq, void* out, void* stream) {
  if (!q || !out) return fail(MLX_E_NULL, "q, out must not be NULL");
  if (nq < 1 || nq > MLX_QUANTILE_MAX_Q)
    return fail(MLX_E_SHAPE, "nq must lie in [1, MLX_QUANTILE_MAX_Q]");
  if (int rc = check_grouped(y, dtype, steps, offsets, nsel, ngroups, nt, n, nq)) return rc;
  QList qs;
  for (int j = 0; j < MLX_QUANTILE_MAX_Q; ++j) {
    qs.v[j] = j < nq ? q[j] : 0.0;
    if (!(qs.v[j] >= 0.0 && qs.v[j] <= 1.0)) return fail(MLX_E_ENUM, "every q must lie in [0, 1]");
  }
  const size_t elem = dtype_size(dtype);
  if (!aligned(out, elem)) return fail(MLX_E_ALIGN, "out not element-aligned");
  hipStream_t st = (hipStream_t)stream;
  const int v = pack_width(n, elem, {{y, elem}, {out, elem}});
  return dispatch_pack(dtype, v, [&](auto t, auto w) {
    return launch_select<typename decltype(t)::type, decltype(w)::value>(y, steps, offsets, nsel,
                                                                         ngroups, nt, n, qs, nq, out, st);
  });
}

int mlx_quantile_exceed_count(const void* y, int dtype, const int32_t* steps,
                              const int64_t* offsets, int64_t nsel, int64_t ngroups, int64_t nt,
                              int64_t n, const double* thr, int64_t* out, void* stream) {
  if (!thr || !out) return fail(MLX_E_NULL, "thr, out must not be NULL");
  if (int rc = check_grouped(y, dtype, steps, offsets, nsel, ngroups, nt, n, 1)) return rc;
  if (!aligned(thr, 8) || !aligned(out, 8)) return fail(MLX_E_ALIGN, "thr / out not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const size_t elem = dtype_size(dtype);
  // (the threshold and the counts are 8-byte cells: accesses of 16 once a lane holds two or more)
  const int v = pack_width(n, elem, {{y, elem}, {thr, 8}, {out, 8}});
  return dispatch_pack(dtype, v, [&](auto t, auto w) {
    return launch_exceed<typename decltype(t)::type, decltype(w)::value>(y, steps, offsets, nsel,
                                                                         ngroups, nt, n, thr, out, st);
  });
}

}  // extern "C"
