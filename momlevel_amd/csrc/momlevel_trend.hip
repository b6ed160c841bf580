// momlevel_trend.hip -- per-cell fits along the time axis of a (time, cells) record, and the
// elementwise pass that applies them (include/momlevel_trend.h):
//
//   trend.calc_linear_trend  (src/momlevel/trend.py:214-290)   xarray polyfit(dim, 1) per cell
//   trend.broadcast_trend    (src/momlevel/trend.py:20-112)    slope * x[t]
//   trend._detrend_array     (src/momlevel/trend.py:167-211)   arr - (slope * x + intercept)
//   trend.seasonal_model     (src/momlevel/trend.py:360-461)   pinv(model).dot(ts); model.dot(coeff)
//   trend.deseason           (src/momlevel/trend.py:464-534, 683-856)
//
// The reference does these through numpy.polyfit / a dask map over single time series, one CPU
// thread.  Here the record is streamed ONCE per pass: a lane owns a pack of horizontally adjacent
// cells (16-byte nontemporal loads: two float64 or four float32), walks time in ascending order
// and keeps a handful of float64 accumulators per cell in registers.  8 B (4 B at float32) per
// cell-step for a fit; 16 B (12 B) for the apply pass.  The small tables (xt, P, M) are indexed
// by wave-uniform values and come through the scalar cache.
//
// The time axis is cut into windows over blockIdx.y.  The window length is a function of nt alone
// (fit_window), never of the device: a record of a few thousand cells still fills the chip, and a
// cell's sums are the same whatever else is in the launch.  Each window writes its partial sums to
// the workspace; k_linfit_finish / k_project_finish add them in ascending window order.  No float
// atomics anywhere: results are bit-identical from run to run.
//
// Cells that do not fill a pack (n not a multiple of it, or rows that are then not 16-byte
// aligned) are handled by the narrower instantiations, down to one cell per lane: every cell of
// every shape is computed, none is left to the caller.
//
// Compile: with momlevel_hip.hip (csrc/build.py), -ffp-contract=off -- k_time_apply's straight-line
// modes keep the reference's operator order and are bit-identical to numpy.  Not part of the kernel
// sources whose hash guards the committed steric profiles (build.trend_source_sha is this file's).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/momlevel_hip.h"
#include "../../include/momlevel_trend.h"
#include "mlx_record.hpp"

#pragma clang fp contract(off)

namespace mlx {
namespace {

constexpr int kTrendBlock = 256;  // 4 waves of 64
constexpr int kFitTerms = 5;      // n_valid, Sx, Sxx, Sy, Sxy
constexpr int kFitUnroll = 8;     // packs a lane has in flight in the fit loops
constexpr int kApplyWindow = 64;  // time steps a lane of the apply pass walks

typedef float tf4_t __attribute__((ext_vector_type(4)));

template <typename TIn, int V>
struct TPack {
  TIn v[V];
};

// once-read data moves with the `nt` cache policy (the idiom of momlevel_hip.hip's load_pack):
// one global_load_dword / dwordx2 / dwordx4 per lane.  (Not mlx_pack.hpp's Pack / load_pack /
// store_pack: on them the two-cell float32 kernels measured slower -- the figures are in that
// header's comment and in profiles/record_fold_ab.log.)
template <typename TIn, int V>
__device__ __forceinline__ TPack<TIn, V> tload(const TIn* __restrict__ p) {
  TPack<TIn, V> r;
  if constexpr (V == 1) {
    r.v[0] = __builtin_nontemporal_load(p);
  } else if constexpr (sizeof(TIn) * V == 8) {
    double raw = __builtin_nontemporal_load(reinterpret_cast<const double*>(p));
    __builtin_memcpy(&r, &raw, 8);
  } else {
    static_assert(sizeof(TIn) * V == 16, "a pack is at most 16 bytes");
    tf4_t raw = __builtin_nontemporal_load(reinterpret_cast<const tf4_t*>(p));
    __builtin_memcpy(&r, &raw, 16);
  }
  return r;
}

// cached loads of the per-cell coefficients (read by every time window of the apply pass)
template <int V>
__device__ __forceinline__ TPack<double, V> cload(const double* __restrict__ p) {
  TPack<double, V> r;
#pragma unroll
  for (int k = 0; k < V; ++k) r.v[k] = p[k];
  return r;
}

template <int V, bool STREAM>
__device__ __forceinline__ void tstore(double* __restrict__ p, const TPack<double, V>& r) {
  if constexpr (V % 2 == 0) {
#pragma unroll
    for (int h = 0; h < V / 2; ++h) {
      tf4_t raw;
      __builtin_memcpy(&raw, &r.v[2 * h], 16);
      if constexpr (STREAM) __builtin_nontemporal_store(raw, reinterpret_cast<tf4_t*>(p) + h);
      else reinterpret_cast<tf4_t*>(p)[h] = raw;
    }
  } else {
    static_assert(V == 1, "packs hold 1, 2 or 4 cells");
    if constexpr (STREAM) __builtin_nontemporal_store(r.v[0], p);
    else p[0] = r.v[0];
  }
}

// ------------------------------------------------------------------------------------------
// k_time_linfit: per window, per cell: n_valid, Sx, Sxx, Sy, Sxy over the valid steps.
// grid = (ceil(n / (kTrendBlock * V)), windows); ws[(w * 5 + j) * n + cell].  n % V == 0.
// ------------------------------------------------------------------------------------------
template <typename TIn, int V>
__global__ __launch_bounds__(kTrendBlock) void k_time_linfit(const TIn* __restrict__ y,
                                                             const double* __restrict__ xt,
                                                             int64_t nt, int64_t n, int64_t window,
                                                             double* __restrict__ ws) {
  const int64_t i = ((int64_t)blockIdx.x * kTrendBlock + threadIdx.x) * V;
  if (i >= n) return;
  const int64_t w = blockIdx.y;
  const int64_t t0 = w * window;
  const int64_t t1 = (t0 + window < nt) ? t0 + window : nt;
  double cnt[V], sx[V], sxx[V], sy[V], sxy[V];
#pragma unroll
  for (int k = 0; k < V; ++k) cnt[k] = sx[k] = sxx[k] = sy[k] = sxy[k] = 0.0;

  auto add = [&](const TPack<TIn, V>& v, double x) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const double yv = (double)v.v[k];  // float32 -> float64 is exact
      const bool bad = is_nan(yv);
      const double xk = bad ? 0.0 : x;
      const double yk = bad ? 0.0 : yv;
      cnt[k] += bad ? 0.0 : 1.0;
      sx[k] += xk;
      sxx[k] += xk * xk;
      sy[k] += yk;
      sxy[k] += xk * yk;
    }
  };

  const TIn* p = y + t0 * n + i;
  int64_t t = t0;
  for (; t + kFitUnroll <= t1; t += kFitUnroll) {
    TPack<TIn, V> v[kFitUnroll];
#pragma unroll
    for (int u = 0; u < kFitUnroll; ++u) v[u] = tload<TIn, V>(p + u * n);
#pragma unroll
    for (int u = 0; u < kFitUnroll; ++u) add(v[u], xt[t + u]);
    p += kFitUnroll * n;
  }
  for (; t < t1; ++t) {
    add(tload<TIn, V>(p), xt[t]);
    p += n;
  }

  double* q = ws + (w * kFitTerms) * n + i;
  TPack<double, V> r;
#pragma unroll
  for (int k = 0; k < V; ++k) r.v[k] = cnt[k];
  tstore<V, false>(q, r);
#pragma unroll
  for (int k = 0; k < V; ++k) r.v[k] = sx[k];
  tstore<V, false>(q + n, r);
#pragma unroll
  for (int k = 0; k < V; ++k) r.v[k] = sxx[k];
  tstore<V, false>(q + 2 * n, r);
#pragma unroll
  for (int k = 0; k < V; ++k) r.v[k] = sy[k];
  tstore<V, false>(q + 3 * n, r);
#pragma unroll
  for (int k = 0; k < V; ++k) r.v[k] = sxy[k];
  tstore<V, false>(q + 4 * n, r);
}

// the windows' sums in ascending order, then the closed form of the straight-line fit
__global__ __launch_bounds__(kTrendBlock) void k_linfit_finish(const double* __restrict__ ws,
                                                               int64_t windows, int64_t n, double s,
                                                               double xmean,
                                                               double* __restrict__ slope,
                                                               double* __restrict__ intercept) {
  const int64_t i = (int64_t)blockIdx.x * kTrendBlock + threadIdx.x;
  if (i >= n) return;
  double a[kFitTerms];
#pragma unroll
  for (int j = 0; j < kFitTerms; ++j) a[j] = 0.0;
  for (int64_t w = 0; w < windows; ++w) {
#pragma unroll
    for (int j = 0; j < kFitTerms; ++j) a[j] += ws[(w * kFitTerms + j) * n + i];
  }
  const double cnt = a[0], sx = a[1], sxx = a[2], sy = a[3], sxy = a[4];
  const double den = cnt * sxx - sx * sx;
  double m = canonical_nan(), b = canonical_nan();
  if (cnt >= 2.0 && den != 0.0) {
    const double mt = (cnt * sxy - sx * sy) / den;
    m = mt / s;
    b = (sy - mt * sx) / cnt - m * xmean;
    m = is_nan(m) ? canonical_nan() : m;
    b = is_nan(b) ? canonical_nan() : b;
  }
  slope[i] = m;
  intercept[i] = b;
}

// ------------------------------------------------------------------------------------------
// k_time_project<KT>: per window, per cell: sum_t P[t][k] * y[t][cell] for k < K <= KT.
// NaN propagates (numpy's dot).  dst[(w * K + k) * n + cell]: the workspace, or coef itself when
// the record is one window.
// ------------------------------------------------------------------------------------------
template <typename TIn, int V, int KT>
__global__ __launch_bounds__(kTrendBlock) void k_time_project(const TIn* __restrict__ y,
                                                              const double* __restrict__ P, int K,
                                                              int64_t nt, int64_t n, int64_t window,
                                                              double* __restrict__ dst) {
  const int64_t i = ((int64_t)blockIdx.x * kTrendBlock + threadIdx.x) * V;
  if (i >= n) return;
  const int64_t w = blockIdx.y;
  const int64_t t0 = w * window;
  const int64_t t1 = (t0 + window < nt) ? t0 + window : nt;
  double acc[KT][V];
#pragma unroll
  for (int k = 0; k < KT; ++k)
#pragma unroll
    for (int c = 0; c < V; ++c) acc[k][c] = 0.0;

  auto add = [&](const TPack<TIn, V>& v, const double* __restrict__ row) {
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      if (k < K) {  // wave-uniform
        const double pk = row[k];
#pragma unroll
        for (int c = 0; c < V; ++c) acc[k][c] += pk * (double)v.v[c];
      }
    }
  };

  constexpr int U = 4;
  const TIn* p = y + t0 * n + i;
  int64_t t = t0;
  for (; t + U <= t1; t += U) {
    TPack<TIn, V> v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = tload<TIn, V>(p + u * n);
#pragma unroll
    for (int u = 0; u < U; ++u) add(v[u], P + (t + u) * K);
    p += U * n;
  }
  for (; t < t1; ++t) {
    add(tload<TIn, V>(p), P + t * K);
    p += n;
  }
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    if (k < K) {
      TPack<double, V> r;
#pragma unroll
      for (int c = 0; c < V; ++c) r.v[c] = acc[k][c];
      tstore<V, false>(dst + (w * K + k) * n + i, r);
    }
  }
}

// rows = K * n consecutive sums per window: coef[j] = sum_w ws[w * rows + j], w ascending
__global__ __launch_bounds__(kTrendBlock) void k_project_finish(const double* __restrict__ ws,
                                                                int64_t windows, int64_t rows,
                                                                double* __restrict__ coef) {
  const int64_t j = (int64_t)blockIdx.x * kTrendBlock + threadIdx.x;
  if (j >= rows) return;
  double a = 0.0;
  for (int64_t w = 0; w < windows; ++w) a += ws[w * rows + j];
  coef[j] = a;
}

// ------------------------------------------------------------------------------------------
// k_time_apply_line: the straight-line modes, operator for operator as trend.py:105, :190-202:
// fit = slope * x[t]; fit = fit + intercept (REMOVE); out = y - fit.
// grid = (ceil(n / (kTrendBlock * V)), ceil(nt / kApplyWindow)).
// ------------------------------------------------------------------------------------------
template <typename TIn, int V, int MODE>
__global__ __launch_bounds__(kTrendBlock) void k_time_apply_line(const TIn* __restrict__ y,
                                                                 const double* __restrict__ x,
                                                                 const double* __restrict__ slope,
                                                                 const double* __restrict__ icpt,
                                                                 int64_t nt, int64_t n,
                                                                 double* __restrict__ out) {
  constexpr bool READS_Y = (MODE == MLX_APPLY_REMOVE || MODE == MLX_APPLY_CORRECT);
  const int64_t i = ((int64_t)blockIdx.x * kTrendBlock + threadIdx.x) * V;
  if (i >= n) return;
  const int64_t t0 = (int64_t)blockIdx.y * kApplyWindow;
  const int64_t t1 = (t0 + kApplyWindow < nt) ? t0 + kApplyWindow : nt;
  const TPack<double, V> m = cload<V>(slope + i);
  TPack<double, V> b;
  if constexpr (MODE == MLX_APPLY_REMOVE) b = cload<V>(icpt + i);
  TPack<double, V> first;
  if constexpr (MODE == MLX_APPLY_TREND_ANOM) {
    const double x0 = x[0];
#pragma unroll
    for (int k = 0; k < V; ++k) first.v[k] = m.v[k] * x0;
  }
#pragma unroll 4
  for (int64_t t = t0; t < t1; ++t) {
    const double xv = x[t];
    TPack<TIn, V> v;
    if constexpr (READS_Y) v = tload<TIn, V>(y + t * n + i);
    TPack<double, V> r;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      double fit = m.v[k] * xv;
      if constexpr (MODE == MLX_APPLY_REMOVE) fit = fit + b.v[k];
      if constexpr (MODE == MLX_APPLY_TREND_ANOM) fit = fit - first.v[k];
      r.v[k] = READS_Y ? (double)v.v[k] - fit : fit;
    }
    tstore<V, true>(out + t * n + i, r);
  }
}

// k_time_apply_model: model = sum_k M[k][t] * c[k][cell], k ascending; out = y - model or model
template <typename TIn, int V, int KT, bool RESID>
__global__ __launch_bounds__(kTrendBlock) void k_time_apply_model(const TIn* __restrict__ y,
                                                                  const double* __restrict__ M,
                                                                  const double* __restrict__ coef,
                                                                  int K, int64_t nt, int64_t n,
                                                                  double* __restrict__ out) {
  const int64_t i = ((int64_t)blockIdx.x * kTrendBlock + threadIdx.x) * V;
  if (i >= n) return;
  const int64_t t0 = (int64_t)blockIdx.y * kApplyWindow;
  const int64_t t1 = (t0 + kApplyWindow < nt) ? t0 + kApplyWindow : nt;
  TPack<double, V> c[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) {
#pragma unroll
    for (int q = 0; q < V; ++q) c[k].v[q] = 0.0;
    if (k < K) c[k] = cload<V>(coef + k * n + i);
  }
#pragma unroll 2
  for (int64_t t = t0; t < t1; ++t) {
    TPack<TIn, V> v;
    if constexpr (RESID) v = tload<TIn, V>(y + t * n + i);
    TPack<double, V> r;
    const double m0 = M[t];
#pragma unroll
    for (int q = 0; q < V; ++q) r.v[q] = m0 * c[0].v[q];
#pragma unroll
    for (int k = 1; k < KT; ++k) {
      if (k < K) {  // wave-uniform
        const double mk = M[k * nt + t];
#pragma unroll
        for (int q = 0; q < V; ++q) r.v[q] += mk * c[k].v[q];
      }
    }
    if constexpr (RESID) {
#pragma unroll
      for (int q = 0; q < V; ++q) r.v[q] = (double)v.v[q] - r.v[q];
    }
    tstore<V, true>(out + t * n + i, r);
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
using detail::fail;
using detail::hip_status;

// Steps per time window of the fit kernels: a function of nt ALONE.  At most 16 windows (their
// partial sums cost 40 B per cell and window against 8 * window bytes of record), none shorter
// than 256 steps unless the record is.
inline int64_t fit_window(int64_t nt) {
  const int64_t w = ceil_div(nt, 16);
  return w < 256 ? 256 : w;
}

constexpr int64_t kMaxSteps = (int64_t)1 << 31;

inline int check_record(const void* y, int dtype, int64_t nt, int64_t n, bool need_y) {
  if (need_y && !y) return fail(MLX_E_NULL, "y must not be NULL");
  if (!is_float_dtype(dtype)) return fail(MLX_E_ENUM, "dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  if (!record_fits(nt, n, kMaxSteps)) return fail(MLX_E_SHAPE, "need 0 < nt < 2^31, 0 < n <= 2^38, nt*n addressable");
  if (y && !aligned(y, dtype_size(dtype))) return fail(MLX_E_ALIGN, "y not element-aligned");
  return 0;
}

template <typename TIn, int V>
int launch_linfit(const void* y, const double* xt, int64_t nt, int64_t n, double* ws, hipStream_t st) {
  const int64_t window = fit_window(nt);
  dim3 grid((unsigned)ceil_div(n, (int64_t)kTrendBlock * V), (unsigned)ceil_div(nt, window));
  hipLaunchKernelGGL((k_time_linfit<TIn, V>), grid, dim3(kTrendBlock), 0, st, (const TIn*)y, xt, nt,
                     n, window, ws);
  return hip_status(hipGetLastError(), "k_time_linfit launch");
}

template <typename TIn, int V>
int launch_project(const void* y, const double* P, int K, int64_t nt, int64_t n, double* dst,
                   hipStream_t st) {
  const int64_t window = fit_window(nt);
  dim3 grid((unsigned)ceil_div(n, (int64_t)kTrendBlock * V), (unsigned)ceil_div(nt, window));
  const TIn* yy = (const TIn*)y;
#define MLX_PROJECT(KT)                                                                          \
  hipLaunchKernelGGL((k_time_project<TIn, V, KT>), grid, dim3(kTrendBlock), 0, st, yy, P, K, nt, \
                     n, window, dst)
  if (K <= 2) MLX_PROJECT(2);
  else if (K <= 4) MLX_PROJECT(4);
  else if (K <= 6) MLX_PROJECT(6);
  else MLX_PROJECT(8);
#undef MLX_PROJECT
  return hip_status(hipGetLastError(), "k_time_project launch");
}

template <typename TIn, int V>
int launch_apply(const void* y, int mode, const double* xm, const double* a, const double* b, int K,
                 int64_t nt, int64_t n, double* out, hipStream_t st) {
  dim3 grid((unsigned)ceil_div(n, (int64_t)kTrendBlock * V), (unsigned)ceil_div(nt, kApplyWindow));
  dim3 block(kTrendBlock);
  const TIn* yy = (const TIn*)y;
#define MLX_LINE(MODE) \
  hipLaunchKernelGGL((k_time_apply_line<TIn, V, MODE>), grid, block, 0, st, yy, xm, a, b, nt, n, out)
#define MLX_MODEL(KT, RESID) \
  hipLaunchKernelGGL((k_time_apply_model<TIn, V, KT, RESID>), grid, block, 0, st, yy, xm, a, K, nt, n, out)
  switch (mode) {
    case MLX_APPLY_REMOVE: MLX_LINE(MLX_APPLY_REMOVE); break;
    case MLX_APPLY_CORRECT: MLX_LINE(MLX_APPLY_CORRECT); break;
    case MLX_APPLY_TREND: MLX_LINE(MLX_APPLY_TREND); break;
    case MLX_APPLY_TREND_ANOM: MLX_LINE(MLX_APPLY_TREND_ANOM); break;
    case MLX_APPLY_MODEL_RESID:
      if (K <= 4) MLX_MODEL(4, true);
      else if (K <= 6) MLX_MODEL(6, true);
      else MLX_MODEL(8, true);
      break;
    default:
      if (K <= 4) MLX_MODEL(4, false);
      else if (K <= 6) MLX_MODEL(6, false);
      else MLX_MODEL(8, false);
      break;
  }
#undef MLX_LINE
#undef MLX_MODEL
  return hip_status(hipGetLastError(), "k_time_apply launch");
}

}  // namespace
}  // namespace mlx

using namespace mlx;

extern "C" {

size_t mlx_time_fit_workspace_bytes(int64_t nt, int64_t n, int nterms) {
  if (!record_fits(nt, n, kMaxSteps) || nterms <= 0 || nterms > MLX_TREND_MAX_TERMS) return 0;
  const int64_t windows = ceil_div(nt, fit_window(nt));
  return (size_t)windows * (size_t)nterms * (size_t)n * sizeof(double);
}

int mlx_time_linfit(const void* y, int dtype, const double* xt, int64_t nt, int64_t n, double s,
                    double xmean, double* slope, double* intercept, void* workspace,
                    size_t workspace_bytes, void* stream) {
  if (!xt || !slope || !intercept || !workspace)
    return fail(MLX_E_NULL, "y, xt, slope, intercept, workspace must not be NULL");
  if (int rc = check_record(y, dtype, nt, n, true)) return rc;
  if (!(s > 0.0) || s != s || xmean != xmean) return fail(MLX_E_SHAPE, "need s > 0 and a finite xmean");
  if (!aligned(xt, 8) || !aligned(slope, 8) || !aligned(intercept, 8))
    return fail(MLX_E_ALIGN, "xt / slope / intercept not 8-byte aligned");
  if (!aligned(workspace, 16) || workspace_bytes < mlx_time_fit_workspace_bytes(nt, n, kFitTerms))
    return fail(MLX_E_WORKSPACE, "workspace misaligned or smaller than mlx_time_fit_workspace_bytes(nt, n, 5)");
  hipStream_t st = (hipStream_t)stream;
  double* ws = (double*)workspace;
  const size_t elem = dtype_size(dtype);
  const int v = pack_width(n, elem, {{y, elem}, {ws, 8}});
  const int rc = dispatch_pack(dtype, v, [&](auto t, auto w) {
    return launch_linfit<typename decltype(t)::type, decltype(w)::value>(y, xt, nt, n, ws, st);
  });
  if (rc) return rc;
  const int64_t windows = ceil_div(nt, fit_window(nt));
  hipLaunchKernelGGL(k_linfit_finish, dim3((unsigned)ceil_div(n, kTrendBlock)), dim3(kTrendBlock), 0,
                     st, (const double*)ws, windows, n, s, xmean, slope, intercept);
  return hip_status(hipGetLastError(), "k_linfit_finish launch");
}

int mlx_time_project(const void* y, int dtype, const double* P, int K, int64_t nt, int64_t n,
                     double* coef, void* workspace, size_t workspace_bytes, void* stream) {
  if (!P || !coef || !workspace) return fail(MLX_E_NULL, "y, P, coef, workspace must not be NULL");
  if (int rc = check_record(y, dtype, nt, n, true)) return rc;
  if (K < 1 || K > MLX_TREND_MAX_TERMS) return fail(MLX_E_SHAPE, "need 1 <= K <= MLX_TREND_MAX_TERMS");
  if (!aligned(P, 8) || !aligned(coef, 8)) return fail(MLX_E_ALIGN, "P / coef not 8-byte aligned");
  if (!aligned(workspace, 16) || workspace_bytes < mlx_time_fit_workspace_bytes(nt, n, K))
    return fail(MLX_E_WORKSPACE, "workspace misaligned or smaller than mlx_time_fit_workspace_bytes(nt, n, K)");
  int64_t rows;
  if (__builtin_mul_overflow((int64_t)K, n, &rows) || ceil_div(rows, kTrendBlock) > 2147483647LL)
    return fail(MLX_E_SHAPE, "n too large");
  hipStream_t st = (hipStream_t)stream;
  const int64_t windows = ceil_div(nt, fit_window(nt));
  double* dst = windows == 1 ? coef : (double*)workspace;  // one window: its sums ARE the result
  const size_t elem = dtype_size(dtype);
  const int v = pack_width(n, elem, {{y, elem}, {dst, 8}});
  const int rc = dispatch_pack(dtype, v, [&](auto t, auto w) {
    return launch_project<typename decltype(t)::type, decltype(w)::value>(y, P, K, nt, n, dst, st);
  });
  if (rc || windows == 1) return rc;
  hipLaunchKernelGGL(k_project_finish, dim3((unsigned)ceil_div(rows, kTrendBlock)), dim3(kTrendBlock),
                     0, st, (const double*)dst, windows, rows, coef);
  return hip_status(hipGetLastError(), "k_project_finish launch");
}

int mlx_time_apply(const void* y, int dtype, int mode, const double* xm, const double* a,
                   const double* b, int K, int64_t nt, int64_t n, double* out, void* stream) {
  if (mode < MLX_APPLY_REMOVE || mode > MLX_APPLY_MODEL) return fail(MLX_E_ENUM, "unknown MLX_APPLY_* mode");
  const bool reads_y = mode == MLX_APPLY_REMOVE || mode == MLX_APPLY_CORRECT || mode == MLX_APPLY_MODEL_RESID;
  const bool model = mode == MLX_APPLY_MODEL_RESID || mode == MLX_APPLY_MODEL;
  if (!xm || !a || !out) return fail(MLX_E_NULL, "xm, a, out must not be NULL");
  if (mode == MLX_APPLY_REMOVE && !b) return fail(MLX_E_NULL, "b (the intercept) must not be NULL in MLX_APPLY_REMOVE");
  if (int rc = check_record(reads_y ? y : nullptr, dtype, nt, n, false)) return rc;
  if (reads_y && !y) return fail(MLX_E_NULL, "y must not be NULL in this mode");
  if (model && (K < 1 || K > MLX_TREND_MAX_TERMS))
    return fail(MLX_E_SHAPE, "need 1 <= K <= MLX_TREND_MAX_TERMS");
  if (!aligned(xm, 8) || !aligned(a, 8) || (b && !aligned(b, 8)) || !aligned(out, 8))
    return fail(MLX_E_ALIGN, "xm / a / b / out not 8-byte aligned");
  if (ceil_div(nt, kApplyWindow) > 65535) return fail(MLX_E_SHAPE, "nt too large for one call: chunk it");
  hipStream_t st = (hipStream_t)stream;
  const void* yy = reads_y ? y : nullptr;
  const int ydtype = reads_y ? dtype : MLX_DTYPE_F64;  // (y is not read: the float64 instantiation)
  const size_t elem = dtype_size(ydtype);
  const int v = pack_width(n, elem, {{yy, elem}, {out, 8}});
  return dispatch_pack(ydtype, v, [&](auto t, auto w) {
    return launch_apply<typename decltype(t)::type, decltype(w)::value>(yy, mode, xm, a, b, K, nt, n,
                                                                        out, st);
  });
}

}  // extern "C"
