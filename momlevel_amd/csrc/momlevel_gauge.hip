// momlevel_gauge.hip -- tide gauges on the model grid (include/momlevel_gauge.h):
//
//   util.geolocate_points       (src/momlevel/util.py:252-367)     BallTree(haversine).query(k=1)
//   tidegauge.extract_tidegauge (src/momlevel/tidegauge.py:40-152) one arr.sel per gauge
//
// k_gauge_prepare   one pass over the points: degrees -> radians -> unit vector, validity from the
//                   mask (== 1.0 exactly) and the finiteness of the coordinates.  The only kernel
//                   with transcendentals per point.
// k_gauge_nearest   the brute-force search.  A lane keeps kGaugePer gauges in registers (unit
//                   vector, best chord^2, best index); a one-wave block streams its part of the
//                   points through LDS in tiles of kGaugeTile (the next tile's loads are in flight
//                   while the current one is consumed) and every lane reads each point as an LDS
//                   broadcast.  Per pair: 3 subtractions, 3 multiplications, 2 additions, a compare
//                   and the selects, all float64 VALU -- no transcendental, no memory traffic
//                   beyond the broadcast.  grid = (gauge tiles, parts of the points); a block writes
//                   its (chord^2, index) partial per gauge.  Points are visited in ascending index
//                   and replaced only by a strictly smaller chord: the lowest index wins a tie.
// k_gauge_combine   16 lanes per gauge share the partials, the candidates meet in LDS (same tie
//                   rule: a total order, so the winner does not depend on the order) and the
//                   haversine angle is evaluated once, for the winner.
// k_gauge_gather    out[g, r] = y[r, index[g]], bits copied; lanes run along r (coalesced stores,
//                   the loads are one element per row of the record by nature).
//
// No atomics anywhere; every pair's value is one fixed expression, so index and angle do not depend
// on the launch geometry or on the split of the points.
//
// Compile: with momlevel_hip.hip (csrc/build.py), -ffp-contract=off -- the squared chord must keep
// its association and its separate roundings.  Not part of the kernel sources whose hash guards the
// committed steric profiles (build.gauge_source_sha is this file's).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/momlevel_hip.h"
#include "../../include/momlevel_gauge.h"
#include "mlx_record.hpp"  // (the host checks: aligned, ceil_div, kMaxCells)

#pragma clang fp contract(off)

namespace mlx {
namespace {

constexpr int kGaugeBlock = 64;    // one wave
constexpr int kGaugePer = 4;       // gauges a lane keeps in registers
constexpr int kGaugeTile = 256;    // points per LDS tile
constexpr int kGaugeLoads = kGaugeTile / kGaugeBlock;  // points a lane stages per tile
constexpr int kPrepBlock = 256;
constexpr unsigned kGaugeMaxGridY = 65535;
constexpr double kDegToRad = 3.14159265358979323846 / 180.0;  // numpy.deg2rad's factor

__device__ __forceinline__ double plus_inf() { return __longlong_as_double(0x7FF0000000000000LL); }
__device__ __forceinline__ bool finite(double x) { return (x - x) == 0.0; }  // false for NaN, +-inf

// ------------------------------------------------------------------------------------------
// k_gauge_prepare
// ------------------------------------------------------------------------------------------
template <typename TC, typename TM>
__global__ __launch_bounds__(kPrepBlock) void k_gauge_prepare(const TC* __restrict__ lat,
                                                              const TC* __restrict__ lon,
                                                              const TM* __restrict__ mask, int64_t n,
                                                              double* __restrict__ table,
                                                              uint8_t* __restrict__ valid) {
  const int64_t i = (int64_t)blockIdx.x * kPrepBlock + threadIdx.x;
  if (i >= n) return;
  const double la = (double)lat[i], lo = (double)lon[i];  // float32 -> float64 is exact
  const bool wet = mask ? (double)mask[i] == 1.0 : true;  // NaN, 0.5, 0: dry
  const bool ok = wet && finite(la) && finite(lo);
  const double phi = la * kDegToRad, lam = lo * kDegToRad;
  const double cphi = cos(phi);
  table[MLX_GAUGE_ROW_X * n + i] = ok ? cphi * cos(lam) : plus_inf();
  table[MLX_GAUGE_ROW_Y * n + i] = ok ? cphi * sin(lam) : plus_inf();
  table[MLX_GAUGE_ROW_Z * n + i] = ok ? sin(phi) : plus_inf();
  table[MLX_GAUGE_ROW_PHI * n + i] = ok ? phi : canonical_nan();
  table[MLX_GAUGE_ROW_LAM * n + i] = ok ? lam : canonical_nan();
  valid[i] = ok ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// k_gauge_nearest: block (bx, by) searches the points [by * chunk, min(n, (by + 1) * chunk)) for
// the gauges bx * 256 + k * 64 + lane, k < 4.  chunk < 2^31: the winner is kept as an offset.
// ------------------------------------------------------------------------------------------
struct Staged {
  double x[kGaugeLoads], y[kGaugeLoads], z[kGaugeLoads];
};

// the tile that starts at point p: lane's share, +inf (can never win) past the end of the part
__device__ __forceinline__ Staged stage_load(const double* __restrict__ px,
                                             const double* __restrict__ py,
                                             const double* __restrict__ pz, int64_t p, int64_t end) {
  Staged s;
#pragma unroll
  for (int u = 0; u < kGaugeLoads; ++u) {
    const int64_t j = p + u * kGaugeBlock + threadIdx.x;
    const bool in = j < end;
    const int64_t jj = in ? j : end - 1;  // (end >= 1: a part is never empty)
    const double x = px[jj], y = py[jj], z = pz[jj];
    s.x[u] = in ? x : plus_inf();
    s.y[u] = in ? y : plus_inf();
    s.z[u] = in ? z : plus_inf();
  }
  return s;
}

__global__ __launch_bounds__(kGaugeBlock) void k_gauge_nearest(const double* __restrict__ points,
                                                               int64_t n,
                                                               const double* __restrict__ gauges,
                                                               int64_t ng, int64_t chunk,
                                                               double* __restrict__ part_d,
                                                               int64_t* __restrict__ part_i) {
  __shared__ double sx[kGaugeTile], sy[kGaugeTile], sz[kGaugeTile];
  const double* px = points + MLX_GAUGE_ROW_X * n;
  const double* py = points + MLX_GAUGE_ROW_Y * n;
  const double* pz = points + MLX_GAUGE_ROW_Z * n;
  const int64_t g0 = (int64_t)blockIdx.x * (kGaugeBlock * kGaugePer) + threadIdx.x;

  for (int64_t part = blockIdx.y; part * chunk < n; part += gridDim.y) {
    const int64_t p0 = part * chunk;
    const int64_t end = p0 + chunk < n ? p0 + chunk : n;

    double gx[kGaugePer], gy[kGaugePer], gz[kGaugePer], best[kGaugePer];
    int32_t where[kGaugePer];
#pragma unroll
    for (int k = 0; k < kGaugePer; ++k) {
      const int64_t g = g0 + k * kGaugeBlock;
      const bool in = g < ng;
      const int64_t gg = in ? g : ng - 1;
      const double x = gauges[MLX_GAUGE_ROW_X * ng + gg], y = gauges[MLX_GAUGE_ROW_Y * ng + gg],
                   z = gauges[MLX_GAUGE_ROW_Z * ng + gg];
      gx[k] = x;
      gy[k] = y;
      gz[k] = z;
      best[k] = plus_inf();
      where[k] = -1;
    }

    Staged next = stage_load(px, py, pz, p0, end);
    for (int64_t p = p0; p < end; p += kGaugeTile) {
      __syncthreads();  // the previous tile has been consumed
#pragma unroll
      for (int u = 0; u < kGaugeLoads; ++u) {
        sx[u * kGaugeBlock + threadIdx.x] = next.x[u];
        sy[u * kGaugeBlock + threadIdx.x] = next.y[u];
        sz[u * kGaugeBlock + threadIdx.x] = next.z[u];
      }
      __syncthreads();
      if (p + kGaugeTile < end) next = stage_load(px, py, pz, p + kGaugeTile, end);
      const int32_t base = (int32_t)(p - p0);
#pragma unroll 4
      for (int j = 0; j < kGaugeTile; ++j) {
        const double ux = sx[j], uy = sy[j], uz = sz[j];  // one address per wave: a broadcast
#pragma unroll
        for (int k = 0; k < kGaugePer; ++k) {
          const double dx = gx[k] - ux, dy = gy[k] - uy, dz = gz[k] - uz;
          const double d = (dx * dx + dy * dy) + dz * dz;
          const bool closer = d < best[k];  // strict: the earlier (lower) index keeps a tie
          best[k] = closer ? d : best[k];
          where[k] = closer ? base + j : where[k];
        }
      }
    }

#pragma unroll
    for (int k = 0; k < kGaugePer; ++k) {
      const int64_t g = g0 + k * kGaugeBlock;
      if (g < ng) {
        part_d[part * ng + g] = best[k];
        part_i[part * ng + g] = where[k] < 0 ? (int64_t)-1 : p0 + where[k];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// k_gauge_combine: block = kCombX gauges x kCombY lanes.  Lane (x, y) walks the partials y, y +
// kCombY, ... of gauge x (reads coalesced along x), lane (x, 0) then takes the kCombY candidates
// from LDS in order and evaluates the haversine angle of the winner.  "Smaller chord, then lower
// index" is a total order on (chord^2, index): the winner is the same whatever the order.
// ------------------------------------------------------------------------------------------
constexpr int kCombX = 64;
constexpr int kCombY = 16;

__device__ __forceinline__ void take_better(double d, int64_t i, int64_t n, double& best, int64_t& bi) {
  const bool take = i >= 0 && i < n && (bi < 0 || d < best || (d == best && i < bi));
  best = take ? d : best;
  bi = take ? i : bi;
}

__global__ __launch_bounds__(kCombX* kCombY) void k_gauge_combine(const double* __restrict__ points,
                                                                  int64_t n,
                                                                  const double* __restrict__ gauges,
                                                                  int64_t ng, int64_t parts,
                                                                  const double* __restrict__ part_d,
                                                                  const int64_t* __restrict__ part_i,
                                                                  int64_t* __restrict__ index,
                                                                  double* __restrict__ angle) {
  __shared__ double sd[kCombY][kCombX];
  __shared__ int64_t si[kCombY][kCombX];
  const int64_t g = (int64_t)blockIdx.x * kCombX + threadIdx.x;
  double best = plus_inf();
  int64_t bi = -1;
  if (g < ng)
    for (int64_t s = threadIdx.y; s < parts; s += kCombY)
      take_better(part_d[s * ng + g], part_i[s * ng + g], n, best, bi);
  sd[threadIdx.y][threadIdx.x] = best;
  si[threadIdx.y][threadIdx.x] = bi;
  __syncthreads();
  if (threadIdx.y != 0 || g >= ng) return;
  for (int y = 1; y < kCombY; ++y) take_better(sd[y][threadIdx.x], si[y][threadIdx.x], n, best, bi);
  index[g] = bi;
  double a = canonical_nan();
  if (bi >= 0) {
    const double phi1 = gauges[MLX_GAUGE_ROW_PHI * ng + g], lam1 = gauges[MLX_GAUGE_ROW_LAM * ng + g];
    const double phi2 = points[MLX_GAUGE_ROW_PHI * n + bi], lam2 = points[MLX_GAUGE_ROW_LAM * n + bi];
    const double s0 = sin(0.5 * (phi1 - phi2));
    const double s1 = sin(0.5 * (lam1 - lam2));
    const double h = s0 * s0 + cos(phi1) * cos(phi2) * s1 * s1;
    const double r = __dsqrt_rn(h);
    a = 2.0 * asin(r > 1.0 ? 1.0 : r);
  }
  angle[g] = a;
}

// ------------------------------------------------------------------------------------------
// k_gauge_gather: U is the unsigned integer of the record's element width -- bits are copied
// ------------------------------------------------------------------------------------------
template <typename U>
__global__ __launch_bounds__(kPrepBlock) void k_gauge_gather(const U* __restrict__ y,
                                                             const int64_t* __restrict__ index,
                                                             int64_t nrest, int64_t n, int64_t ng,
                                                             U* __restrict__ out, U nan_bits) {
  const int64_t r = (int64_t)blockIdx.x * kPrepBlock + threadIdx.x;
  if (r >= nrest) return;
  for (int64_t g = blockIdx.y; g < ng; g += gridDim.y) {
    const int64_t i = index[g];
    const bool in = i >= 0 && i < n;
    const U v = y[r * n + (in ? i : 0)];
    out[g * nrest + r] = in ? v : nan_bits;
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
using detail::fail;
using detail::hip_status;

constexpr int64_t kMaxGauges = (int64_t)1 << 31;
constexpr int64_t kMaxChunk = (int64_t)1 << 30;  // the winner's offset in its part is an int32
constexpr int64_t kWantBlocks = 8192;            // one-wave blocks: 8 per SIMD of 256 CUs

// points per part and the number of parts
inline void cut(int64_t n, int64_t ng, int64_t split, int64_t* chunk, int64_t* parts) {
  int64_t c;
  if (split > 0) {
    c = ceil_div(n, split < n ? split : n);
  } else {
    const int64_t gblocks = ceil_div(ng, kGaugeBlock * kGaugePer);
    int64_t want = kWantBlocks / gblocks;
    want = want < 1 ? 1 : want;
    c = ceil_div(n, want);
    c = c < 4 * kGaugeTile ? 4 * kGaugeTile : c;
    c = ceil_div(c, kGaugeTile) * kGaugeTile;  // whole tiles: no padded lanes but in the last part
  }
  const int64_t least = ceil_div(n, (int64_t)kGaugeMaxGridY);  // every part gets a block of its own
  c = c < least ? least : c;
  c = c > kMaxChunk ? kMaxChunk : c;  // (n <= 2^38: at most 256 parts then)
  *chunk = c;
  *parts = ceil_div(n, c);
}

template <typename TC>
int launch_prepare(const void* lat, const void* lon, const void* mask, int mask_dtype, int64_t n,
                   double* table, uint8_t* valid, hipStream_t st) {
  dim3 grid((unsigned)ceil_div(n, kPrepBlock));
  if (mask && mask_dtype == MLX_DTYPE_F32)
    hipLaunchKernelGGL((k_gauge_prepare<TC, float>), grid, dim3(kPrepBlock), 0, st, (const TC*)lat,
                       (const TC*)lon, (const float*)mask, n, table, valid);
  else
    hipLaunchKernelGGL((k_gauge_prepare<TC, double>), grid, dim3(kPrepBlock), 0, st, (const TC*)lat,
                       (const TC*)lon, (const double*)mask, n, table, valid);
  return hip_status(hipGetLastError(), "k_gauge_prepare launch");
}

}  // namespace
}  // namespace mlx

using namespace mlx;

extern "C" {

int mlx_gauge_prepare(const void* lat, const void* lon, int dtype, const void* mask, int mask_dtype,
                      int64_t n, double* table, uint8_t* valid, void* stream) {
  if (!lat || !lon || !table || !valid) return fail(MLX_E_NULL, "lat, lon, table, valid must not be NULL");
  if (n <= 0 || n > kMaxCells) return fail(MLX_E_SHAPE, "need 0 < n <= 2^38");
  if (dtype != MLX_DTYPE_F64 && dtype != MLX_DTYPE_F32)
    return fail(MLX_E_ENUM, "dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  if (mask && mask_dtype != MLX_DTYPE_F64 && mask_dtype != MLX_DTYPE_F32)
    return fail(MLX_E_ENUM, "mask_dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  const size_t elem = dtype == MLX_DTYPE_F64 ? 8 : 4;
  if (!aligned(lat, elem) || !aligned(lon, elem)) return fail(MLX_E_ALIGN, "lat / lon not element-aligned");
  if (mask && !aligned(mask, mask_dtype == MLX_DTYPE_F64 ? 8 : 4))
    return fail(MLX_E_ALIGN, "mask not element-aligned");
  if (!aligned(table, 8)) return fail(MLX_E_ALIGN, "table not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  return dtype == MLX_DTYPE_F64 ? launch_prepare<double>(lat, lon, mask, mask_dtype, n, table, valid, st)
                                : launch_prepare<float>(lat, lon, mask, mask_dtype, n, table, valid, st);
}

int64_t mlx_gauge_nearest_split(int64_t n, int64_t ng, int64_t split) {
  if (n <= 0 || ng <= 0 || n > kMaxCells || ng >= kMaxGauges || split < 0) return 0;
  int64_t chunk, parts;
  cut(n, ng, split, &chunk, &parts);
  return parts;
}

size_t mlx_gauge_nearest_workspace_bytes(int64_t n, int64_t ng, int64_t split) {
  const int64_t parts = mlx_gauge_nearest_split(n, ng, split);
  return parts <= 0 ? 0 : (size_t)parts * (size_t)ng * 16;
}

int mlx_gauge_nearest(const double* points, int64_t n, const double* gauges, int64_t ng,
                      int64_t split, int64_t* index, double* angle, void* workspace,
                      size_t workspace_bytes, void* stream) {
  if (!points || !gauges || !index || !angle || !workspace)
    return fail(MLX_E_NULL, "points, gauges, index, angle, workspace must not be NULL");
  if (n <= 0 || ng <= 0 || n > kMaxCells || ng >= kMaxGauges || split < 0)
    return fail(MLX_E_SHAPE, "need 0 < n <= 2^38, 0 < ng < 2^31, split >= 0");
  if (!aligned(points, 8) || !aligned(gauges, 8) || !aligned(index, 8) || !aligned(angle, 8))
    return fail(MLX_E_ALIGN, "points / gauges / index / angle not 8-byte aligned");
  int64_t chunk, parts;
  cut(n, ng, split, &chunk, &parts);
  if (!aligned(workspace, 16) || workspace_bytes < (size_t)parts * (size_t)ng * 16)
    return fail(MLX_E_WORKSPACE, "workspace too small (mlx_gauge_nearest_workspace_bytes) or not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  double* part_d = (double*)workspace;
  int64_t* part_i = (int64_t*)(part_d + parts * ng);
  dim3 grid((unsigned)ceil_div(ng, kGaugeBlock * kGaugePer), (unsigned)parts);
  hipLaunchKernelGGL(k_gauge_nearest, grid, dim3(kGaugeBlock), 0, st, points, n, gauges, ng, chunk,
                     part_d, part_i);
  int rc = hip_status(hipGetLastError(), "k_gauge_nearest launch");
  if (rc) return rc;
  hipLaunchKernelGGL(k_gauge_combine, dim3((unsigned)ceil_div(ng, kCombX)), dim3(kCombX, kCombY), 0,
                     st, points, n, gauges, ng, parts, part_d, part_i, index, angle);
  return hip_status(hipGetLastError(), "k_gauge_combine launch");
}

int mlx_gauge_gather(const void* y, int dtype, const int64_t* index, int64_t nrest, int64_t n,
                     int64_t ng, void* out, void* stream) {
  if (!y || !index || !out) return fail(MLX_E_NULL, "y, index, out must not be NULL");
  if (dtype != MLX_DTYPE_F64 && dtype != MLX_DTYPE_F32)
    return fail(MLX_E_ENUM, "dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  int64_t total, rows;
  if (nrest <= 0 || n <= 0 || ng <= 0 || nrest >= kMaxGauges || ng >= kMaxGauges || n > kMaxCells ||
      __builtin_mul_overflow(nrest, n, &total) || total > INT64_MAX / 64 ||
      __builtin_mul_overflow(ng, nrest, &rows) || rows > INT64_MAX / 64)
    return fail(MLX_E_SHAPE,
                "need 0 < nrest, ng < 2^31, 0 < n <= 2^38, nrest*n and ng*nrest addressable");
  const size_t elem = dtype == MLX_DTYPE_F64 ? 8 : 4;
  if (!aligned(y, elem) || !aligned(out, elem)) return fail(MLX_E_ALIGN, "y / out not element-aligned");
  if (!aligned(index, 8)) return fail(MLX_E_ALIGN, "index not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)ceil_div(nrest, kPrepBlock),
            ng < (int64_t)kGaugeMaxGridY ? (unsigned)ng : kGaugeMaxGridY);
  if (dtype == MLX_DTYPE_F64)
    hipLaunchKernelGGL((k_gauge_gather<uint64_t>), grid, dim3(kPrepBlock), 0, st, (const uint64_t*)y,
                       index, nrest, n, ng, (uint64_t*)out, (uint64_t)0x7FF8000000000000ULL);
  else
    hipLaunchKernelGGL((k_gauge_gather<uint32_t>), grid, dim3(kPrepBlock), 0, st, (const uint32_t*)y,
                       index, nrest, n, ng, (uint32_t*)out, (uint32_t)0x7FC00000U);
  return hip_status(hipGetLastError(), "k_gauge_gather launch");
}

}  // extern "C"
