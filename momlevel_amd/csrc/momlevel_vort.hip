// momlevel_vort.hip -- mlx_vort_rel_vort, mlx_vort_pv, mlx_vort_rossby (include/momlevel_vort.h):
// the array work of momlevel.derived.calc_rel_vort, calc_pv and calc_rossby_rd
// (src/momlevel/derived.py:232-239, 538-556, 588).
//
// The two stencils are memory-bound passes over (record, y, x): two fields in, one out -- 24 bytes
// per cell at float64 -- plus 2-D metrics (dx, dy, area; the Coriolis parameter) that every record
// reads again.  No LDS, no atomics, no workspace.
//
// Shape of the packed path: wave64, 256-thread blocks = kVortBands waves stacked in y.  A lane owns
// one 16-byte pack of columns (2 float64 / 4 float32 cells of the arithmetic dtype; a float32
// operand of float64 arithmetic comes as an 8-byte load) and walks down the kVortH rows of its
// wave's tile with the CURRENT row of fu = u * dx (of the x-averaged N^2) in registers: it loads
// row j + 1, uses it as the neighbour and keeps it as the next current row.  A row of u (of N^2) is
// so read once per tile plus one halo row, (24 + 8 / kVortH) / 24 of the algorithmic bytes -- and
// the halo row of a wave is the first row of the wave below it in the same block.  The loads of
// kVortR rows are issued together before the first of their cells is computed.  fv[j, i + 1] (the
// N^2 of column i + 1) beyond the pack is one overlapping element load of the neighbouring lane's
// line.  ONE TILE PER BLOCK (a striding grid was slower on this machine), the
// RECORD fastest in the grid: the blocks that run together work on the same tile of different
// records, so that the 2-D metrics of the tile are fetched once per XCD and then found in its L2.
// u, v, zeta and N^2 are touched once: `nt` loads and stores.
//
// Everything else -- symmetric grids, nx not a multiple of the pack, pointers that are not aligned
// for their pack accesses -- goes cell by cell through the same device functions (vort_zeta_cell,
// vort_pv_cell, vort_avg): the bits of a cell do not depend on the path.
//
// Compile: with momlevel_hip.hip (csrc/build.py).  Contraction is off for the whole file: every
// operation is rounded on its own, as numpy rounds it.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/momlevel_hip.h"
#include "../../include/momlevel_vort.h"
#include "mlx_internal.hpp"
#include "mlx_pack.hpp"

#pragma clang fp contract(off)

namespace mlx {
namespace {

constexpr int kVortLanes = MLX_VORT_TILE_LANES;  // packs across a tile: one wave
constexpr int kVortH = MLX_VORT_TILE_H;          // rows of a tile
constexpr int kVortBands = MLX_VORT_TILE_BANDS;  // tiles (waves) stacked in a block
constexpr int kVortBlock = kVortLanes * kVortBands;
constexpr int kVortR = 2;                        // rows whose loads are in flight together
constexpr int64_t kVortMaxBlocks = (int64_t)1 << 23;  // (a HIP grid holds < 2^32 threads)
constexpr int64_t kVortMaxCells = (int64_t)1 << 38;

static_assert(kVortLanes == 64 && kVortH % kVortR == 0, "a tile is one wave wide");

// numpy's promotion of two of {float32, float64}
template <typename A, typename B>
struct Promote {
  typedef double type;
};
template <>
struct Promote<float, float> {
  typedef float type;
};

// P cells of X in one load of sizeof(X) * P bytes (16, 8, or the element); NT: touched once
template <typename X, int P, bool NT>
__device__ __forceinline__ void vort_load(const X* __restrict__ p, X (&v)[P]) {
  const Pack<X, P> r = load_pack<X, P, NT>(p);
#pragma unroll
  for (int k = 0; k < P; ++k) v[k] = r.v[k];
}

template <typename X, int P>
__device__ __forceinline__ void vort_store(X* __restrict__ p, const X (&v)[P]) {
  static_assert(sizeof(X) * P == 16, "a pack of the result is 16 bytes");
  Pack<X, P> r;
#pragma unroll
  for (int k = 0; k < P; ++k) r.v[k] = v[k];
  store_pack<X, P, true>(p, r);
}

__device__ __forceinline__ float vort_abs(float x) { return __builtin_fabsf(x); }
__device__ __forceinline__ double vort_abs(double x) { return __builtin_fabs(x); }

// ( -(fu_hi - fu_lo) + (fv_hi - fv_lo) ) / area                              derived.py:232-239
template <typename TA>
__device__ __forceinline__ TA vort_zeta_cell(TA fu_lo, TA fu_hi, TA fv_lo, TA fv_hi, TA area) {
  const TA dy_fu = fu_hi - fu_lo;
  const TA dx_fv = fv_hi - fv_lo;
  const TA num = -dy_fu + dx_fv;
  return num / area;
}

// grid.interp's step: 0.5 * (a + b)
template <typename TN>
__device__ __forceinline__ TN vort_avg(TN a, TN b) {
  const TN sum = a + b;
  return (TN)0.5 * sum;
}

// (zeta + f) * (n2c / gravity) [ -> | (pv / 100) * 1e14 | ]                   derived.py:547, 556
template <typename TZ, typename TC, typename TN>
__device__ __forceinline__ typename Promote<typename Promote<TZ, TC>::type, TN>::type vort_pv_cell(
    TZ zeta, TC f, TN n2c, TN gravity, int cm) {
  typedef typename Promote<TZ, TC>::type TS;
  typedef typename Promote<TS, TN>::type TR;
  const TS absvort = (TS)zeta + (TS)f;
  const TN strat = n2c / gravity;
  TR pv = (TR)absvort * (TR)strat;
  if (cm) {
    pv = pv / (TR)100.0;
    pv = pv * (TR)1.0e14;
    pv = vort_abs(pv);
  }
  return pv;
}

// ---------------------------------------------------------------------------- zeta, packed
// Non-symmetric grids with nx % P == 0 and every pointer aligned for its pack access.
// grid = (records, ceil(nx / (P kVortLanes)), ceil(ny / (kVortH kVortBands))).
template <typename TF, typename TM>
__global__ __launch_bounds__(kVortBlock) void k_vort_zeta(
    const TF* __restrict__ u, const TF* __restrict__ v, const TM* __restrict__ dx,
    const TM* __restrict__ dy, const TM* __restrict__ area,
    typename Promote<TF, TM>::type* __restrict__ out, int ny, int nx) {
  typedef typename Promote<TF, TM>::type TA;
  constexpr int P = 16 / (int)sizeof(TA);
  const int lane = threadIdx.x & (kVortLanes - 1), band = threadIdx.x / kVortLanes;
  const int64_t i0 = ((int64_t)blockIdx.y * kVortLanes + lane) * P;
  const int64_t j0 = ((int64_t)blockIdx.z * kVortBands + band) * kVortH;
  if (i0 >= nx || j0 >= ny) return;  // (no barrier in this kernel)
  const int64_t plane = (int64_t)ny * nx, rec = (int64_t)blockIdx.x * plane + i0;
  u += rec, v += rec, out += rec;
  dx += i0, dy += i0, area += i0;
  const bool edge = i0 + P >= nx;  // the pack's right-hand neighbour is past the end: 0.0

  TA fu[P];
  {
    TF a[P];
    TM m[P];
    vort_load<TF, P, true>(u + j0 * nx, a);
    vort_load<TM, P, false>(dx + j0 * nx, m);
#pragma unroll
    for (int k = 0; k < P; ++k) fu[k] = (TA)a[k] * (TA)m[k];
  }
#pragma unroll 1
  for (int c = 0; c < kVortH && j0 + c < ny; c += kVortR) {
    TF un[kVortR][P], vv[kVortR][P], vx[kVortR];
    TM dn[kVortR][P], dv[kVortR][P], dvx[kVortR], ar[kVortR][P];
#pragma unroll
    for (int r = 0; r < kVortR; ++r) {
      const int64_t j = j0 + c + r;
      if (j < ny) {
        const int64_t o = j * nx;
        if (j + 1 < ny) {
          vort_load<TF, P, true>(u + o + nx, un[r]);
          vort_load<TM, P, false>(dx + o + nx, dn[r]);
        }
        vort_load<TF, P, true>(v + o, vv[r]);
        vort_load<TM, P, false>(dy + o, dv[r]);
        vort_load<TM, P, false>(area + o, ar[r]);
        if (!edge) {
          vx[r] = v[o + P];
          dvx[r] = dy[o + P];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kVortR; ++r) {
      const int64_t j = j0 + c + r;
      if (j < ny) {
        TA fn[P], fv[P + 1], res[P];
#pragma unroll
        for (int k = 0; k < P; ++k) {
          fn[k] = j + 1 < ny ? (TA)un[r][k] * (TA)dn[r][k] : (TA)0.0;
          fv[k] = (TA)vv[r][k] * (TA)dv[r][k];
        }
        fv[P] = edge ? (TA)0.0 : (TA)vx[r] * (TA)dvx[r];
#pragma unroll
        for (int k = 0; k < P; ++k) {
          res[k] = vort_zeta_cell<TA>(fu[k], fn[k], fv[k], fv[k + 1], (TA)ar[r][k]);
          fu[k] = fn[k];
        }
        vort_store<TA, P>(out + j * nx, res);
      }
    }
  }
}

// ---------------------------------------------------------------------------- zeta, cell by cell
// Any grid, any alignment.  s = symmetric: the neighbours of corner (j, i) are rows j - s and
// j + 1 - s of u (ny - s rows) and columns i - s and i + 1 - s of v (nx - s columns); out of range
// is the literal 0.0.
template <typename TF, typename TM>
__global__ __launch_bounds__(kVortBlock) void k_vort_zeta_cells(
    const TF* __restrict__ u, const TF* __restrict__ v, const TM* __restrict__ dx,
    const TM* __restrict__ dy, const TM* __restrict__ area,
    typename Promote<TF, TM>::type* __restrict__ out, int64_t nrec, int64_t ny, int64_t nx, int s) {
  typedef typename Promote<TF, TM>::type TA;
  const int64_t plane = ny * nx, n = nrec * plane;
  const int64_t nyu = ny - s, nxv = nx - s;
  for (int64_t idx = (int64_t)blockIdx.x * kVortBlock + threadIdx.x; idx < n;
       idx += (int64_t)gridDim.x * kVortBlock) {
    const int64_t rec = idx / plane, cell = idx - rec * plane;
    const int64_t j = cell / nx, i = cell - j * nx;
    const int64_t jl = j - s, jh = j + 1 - s, il = i - s, ih = i + 1 - s;
    const TF* ur = u + rec * nyu * nx;
    const TF* vr = v + rec * ny * nxv;
    const TA fu_lo = jl >= 0 ? (TA)ur[jl * nx + i] * (TA)dx[jl * nx + i] : (TA)0.0;
    const TA fu_hi = jh < nyu ? (TA)ur[jh * nx + i] * (TA)dx[jh * nx + i] : (TA)0.0;
    const TA fv_lo = il >= 0 ? (TA)vr[j * nxv + il] * (TA)dy[j * nxv + il] : (TA)0.0;
    const TA fv_hi = ih < nxv ? (TA)vr[j * nxv + ih] * (TA)dy[j * nxv + ih] : (TA)0.0;
    out[idx] = vort_zeta_cell<TA>(fu_lo, fu_hi, fv_lo, fv_hi, (TA)area[cell]);
  }
}

// ---------------------------------------------------------------------------- pv, packed
template <typename TN, int P>
__device__ __forceinline__ void vort_avg_x(const TN (&n)[P], TN next, TN (&ax)[P]) {
#pragma unroll
  for (int k = 0; k < P; ++k) ax[k] = vort_avg<TN>(n[k], k + 1 < P ? n[k + 1] : next);
}

template <typename TZ, typename TC, typename TN, bool INTERP>
__global__ __launch_bounds__(kVortBlock) void k_vort_pv(
    const TZ* __restrict__ zeta, const TC* __restrict__ f, const TN* __restrict__ n2,
    typename Promote<typename Promote<TZ, TC>::type, TN>::type* __restrict__ out, int ny, int nx,
    TN gravity, int cm) {
  typedef typename Promote<typename Promote<TZ, TC>::type, TN>::type TR;
  constexpr int P = 16 / (int)sizeof(TR);
  const int lane = threadIdx.x & (kVortLanes - 1), band = threadIdx.x / kVortLanes;
  const int64_t i0 = ((int64_t)blockIdx.y * kVortLanes + lane) * P;
  const int64_t j0 = ((int64_t)blockIdx.z * kVortBands + band) * kVortH;
  if (i0 >= nx || j0 >= ny) return;  // (no barrier in this kernel)
  const int64_t plane = (int64_t)ny * nx, rec = (int64_t)blockIdx.x * plane + i0;
  zeta += rec, n2 += rec, out += rec;
  f += i0;
  const bool edge = i0 + P >= nx;

  TN ax[P];  // the x-averaged N^2 of the current row
  if constexpr (INTERP) {
    TN n[P];
    vort_load<TN, P, true>(n2 + j0 * nx, n);
    vort_avg_x<TN, P>(n, edge ? (TN)0.0 : n2[j0 * nx + P], ax);
  }
#pragma unroll 1
  for (int c = 0; c < kVortH && j0 + c < ny; c += kVortR) {
    TZ z[kVortR][P];
    TC cf[kVortR][P];
    TN nn[kVortR][P], nxt[kVortR];
#pragma unroll
    for (int r = 0; r < kVortR; ++r) {
      const int64_t j = j0 + c + r;
      if (j < ny) {
        const int64_t o = j * nx;
        vort_load<TZ, P, true>(zeta + o, z[r]);
        vort_load<TC, P, false>(f + o, cf[r]);
        if constexpr (INTERP) {
          if (j + 1 < ny) {
            vort_load<TN, P, true>(n2 + o + nx, nn[r]);
            if (!edge) nxt[r] = n2[o + nx + P];
          }
        } else {
          vort_load<TN, P, true>(n2 + o, nn[r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kVortR; ++r) {
      const int64_t j = j0 + c + r;
      if (j < ny) {
        TR res[P];
        if constexpr (INTERP) {
          TN an[P];
          if (j + 1 < ny) {
            vort_avg_x<TN, P>(nn[r], edge ? (TN)0.0 : nxt[r], an);
          } else {
#pragma unroll
            for (int k = 0; k < P; ++k) an[k] = (TN)0.0;
          }
#pragma unroll
          for (int k = 0; k < P; ++k) {
            res[k] = vort_pv_cell<TZ, TC, TN>(z[r][k], cf[r][k], vort_avg<TN>(ax[k], an[k]),
                                              gravity, cm);
            ax[k] = an[k];
          }
        } else {
#pragma unroll
          for (int k = 0; k < P; ++k)
            res[k] = vort_pv_cell<TZ, TC, TN>(z[r][k], cf[r][k], nn[r][k], gravity, cm);
        }
        vort_store<TR, P>(out + j * nx, res);
      }
    }
  }
}

// ---------------------------------------------------------------------------- pv, cell by cell
// interp: N^2 is (ny - s, nx - s); the x-average at row jj, corner column i is
// 0.5 * (n2[jj, i - s] + n2[jj, i + 1 - s]) and the corner value 0.5 * (ax[j - s] + ax[j + 1 - s]),
// out of range the literal 0.0 at either step.
template <typename TZ, typename TC, typename TN>
__global__ __launch_bounds__(kVortBlock) void k_vort_pv_cells(
    const TZ* __restrict__ zeta, const TC* __restrict__ f, const TN* __restrict__ n2,
    typename Promote<typename Promote<TZ, TC>::type, TN>::type* __restrict__ out, int64_t nrec,
    int64_t ny, int64_t nx, int interp, int s, TN gravity, int cm) {
  const int64_t plane = ny * nx, n = nrec * plane;
  const int64_t nyn = ny - s, nxn = nx - s;
  for (int64_t idx = (int64_t)blockIdx.x * kVortBlock + threadIdx.x; idx < n;
       idx += (int64_t)gridDim.x * kVortBlock) {
    const int64_t rec = idx / plane, cell = idx - rec * plane;
    TN n2c;
    if (interp) {
      const int64_t j = cell / nx, i = cell - j * nx;
      const int64_t il = i - s, ih = i + 1 - s;
      const TN* nr = n2 + rec * nyn * nxn;
      TN ax[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int64_t jj = j + h - s;
        if (jj >= 0 && jj < nyn) {
          const TN a = il >= 0 ? nr[jj * nxn + il] : (TN)0.0;
          const TN b = ih < nxn ? nr[jj * nxn + ih] : (TN)0.0;
          ax[h] = vort_avg<TN>(a, b);
        } else {
          ax[h] = (TN)0.0;
        }
      }
      n2c = vort_avg<TN>(ax[0], ax[1]);
    } else {
      n2c = n2[idx];
    }
    out[idx] = vort_pv_cell<TZ, TC, TN>(zeta[idx], f[cell], n2c, gravity, cm);
  }
}

// ---------------------------------------------------------------------------- Rossby radius
template <typename TCs, typename TF>
__global__ __launch_bounds__(kVortBlock) void k_vort_rossby(
    const TCs* __restrict__ c, const TF* __restrict__ f,
    typename Promote<TCs, TF>::type* __restrict__ out, int64_t n, int64_t plane, int64_t inner) {
  typedef typename Promote<TCs, TF>::type TR;
  for (int64_t idx = (int64_t)blockIdx.x * kVortBlock + threadIdx.x; idx < n;
       idx += (int64_t)gridDim.x * kVortBlock) {
    const int64_t p = (idx / inner) % plane;
    const TF af = vort_abs(f[p]);
    out[idx] = (TR)c[idx] / (TR)af;
  }
}

// ---------------------------------------------------------------------------- host side
inline bool vort_aligned(const void* p, size_t width) {
  return reinterpret_cast<uintptr_t>(p) % width == 0;
}

inline unsigned vort_cell_grid(int64_t n) {
  const int64_t blocks = (n + kVortBlock - 1) / kVortBlock;
  return (unsigned)(blocks < kVortMaxBlocks ? blocks : kVortMaxBlocks);
}

// the grid of the packed path for one record, or false when the plane does not fit one
inline bool vort_tile_grid(int64_t ny, int64_t nx, int P, int64_t* gy, int64_t* gz) {
  *gy = (nx / P + kVortLanes - 1) / kVortLanes;
  *gz = (ny + (int64_t)kVortH * kVortBands - 1) / ((int64_t)kVortH * kVortBands);
  return *gy <= 65535 && *gz <= 65535 && *gy * *gz <= kVortMaxBlocks;
}

// Records one launch of the packed path takes (the record is the grid's x) for a corner plane of
// (ny, nx) in packs of P cells, with that record's grid in *gy, *gz; 0 where the plane's shape
// sends it cell by cell.  The one rule: mlx_vort_records_per_launch reports it, zeta_launch and
// pv_launch cut their calls by it.
inline int64_t vort_records_per_launch(int64_t ny, int64_t nx, int P, int64_t* gy, int64_t* gz) {
  if (nx % P != 0 || !vort_tile_grid(ny, nx, P, gy, gz)) return 0;
  return kVortMaxBlocks / (*gy * *gz);
}

template <typename TF, typename TM>
int zeta_launch(const void* u_, const void* v_, const void* dx_, const void* dy_, const void* area_,
                int64_t nrec, int64_t ny, int64_t nx, int s, void* out_, hipStream_t st) {
  typedef typename Promote<TF, TM>::type TA;
  constexpr int P = 16 / (int)sizeof(TA);
  const TF* u = (const TF*)u_;
  const TF* v = (const TF*)v_;
  const TM* dx = (const TM*)dx_;
  const TM* dy = (const TM*)dy_;
  const TM* area = (const TM*)area_;
  TA* out = (TA*)out_;
  int64_t gy, gz;
  const int64_t step = vort_records_per_launch(ny, nx, P, &gy, &gz);
  const bool packed = s == 0 && step > 0 && vort_aligned(u, sizeof(TF) * P) &&
                      vort_aligned(v, sizeof(TF) * P) && vort_aligned(dx, sizeof(TM) * P) &&
                      vort_aligned(dy, sizeof(TM) * P) && vort_aligned(area, sizeof(TM) * P) &&
                      vort_aligned(out, 16);
  if (!packed) {
    hipLaunchKernelGGL((k_vort_zeta_cells<TF, TM>), dim3(vort_cell_grid(nrec * ny * nx)),
                       dim3(kVortBlock), 0, st, u, v, dx, dy, area, out, nrec, ny, nx, s);
    return detail::hip_status(hipGetLastError(), "k_vort_zeta_cells launch");
  }
  const int64_t plane = ny * nx;
  for (int64_t r0 = 0; r0 < nrec; r0 += step) {
    const int64_t nr = nrec - r0 < step ? nrec - r0 : step;
    hipLaunchKernelGGL((k_vort_zeta<TF, TM>), dim3((unsigned)nr, (unsigned)gy, (unsigned)gz),
                       dim3(kVortBlock), 0, st, u + r0 * plane, v + r0 * plane, dx, dy, area,
                       out + r0 * plane, (int)ny, (int)nx);
    if (int rc = detail::hip_status(hipGetLastError(), "k_vort_zeta launch")) return rc;
  }
  return 0;
}

template <typename TZ, typename TC, typename TN>
int pv_launch(const void* zeta_, const void* f_, const void* n2_, int64_t nrec, int64_t ny,
              int64_t nx, int interp, int s, double gravity, int cm, void* out_, hipStream_t st) {
  typedef typename Promote<typename Promote<TZ, TC>::type, TN>::type TR;
  constexpr int P = 16 / (int)sizeof(TR);
  const TZ* zeta = (const TZ*)zeta_;
  const TC* f = (const TC*)f_;
  const TN* n2 = (const TN*)n2_;
  TR* out = (TR*)out_;
  const TN g = (TN)gravity;  // (a python float is weak: it takes N^2's dtype)
  int64_t gy, gz;
  const int64_t step = vort_records_per_launch(ny, nx, P, &gy, &gz);
  const bool packed = (s == 0 || !interp) && step > 0 && vort_aligned(zeta, sizeof(TZ) * P) &&
                      vort_aligned(f, sizeof(TC) * P) && vort_aligned(n2, sizeof(TN) * P) &&
                      vort_aligned(out, 16);
  if (!packed) {
    hipLaunchKernelGGL((k_vort_pv_cells<TZ, TC, TN>), dim3(vort_cell_grid(nrec * ny * nx)),
                       dim3(kVortBlock), 0, st, zeta, f, n2, out, nrec, ny, nx, interp,
                       interp ? s : 0, g, cm);
    return detail::hip_status(hipGetLastError(), "k_vort_pv_cells launch");
  }
  const int64_t plane = ny * nx;
  for (int64_t r0 = 0; r0 < nrec; r0 += step) {
    const int64_t nr = nrec - r0 < step ? nrec - r0 : step;
    const dim3 grid((unsigned)nr, (unsigned)gy, (unsigned)gz);
    if (interp)
      hipLaunchKernelGGL((k_vort_pv<TZ, TC, TN, true>), grid, dim3(kVortBlock), 0, st,
                         zeta + r0 * plane, f, n2 + r0 * plane, out + r0 * plane, (int)ny, (int)nx,
                         g, cm);
    else
      hipLaunchKernelGGL((k_vort_pv<TZ, TC, TN, false>), grid, dim3(kVortBlock), 0, st,
                         zeta + r0 * plane, f, n2 + r0 * plane, out + r0 * plane, (int)ny, (int)nx,
                         g, cm);
    if (int rc = detail::hip_status(hipGetLastError(), "k_vort_pv launch")) return rc;
  }
  return 0;
}

template <typename TCs, typename TF>
int rossby_launch(const void* c, const void* f, int64_t n, int64_t plane, int64_t inner, void* out,
                  hipStream_t st) {
  typedef typename Promote<TCs, TF>::type TR;
  hipLaunchKernelGGL((k_vort_rossby<TCs, TF>), dim3(vort_cell_grid(n)), dim3(kVortBlock), 0, st,
                     (const TCs*)c, (const TF*)f, (TR*)out, n, plane, inner);
  return detail::hip_status(hipGetLastError(), "k_vort_rossby launch");
}

inline bool vort_dtype_ok(int dt) { return dt == MLX_DTYPE_F64 || dt == MLX_DTYPE_F32; }
inline size_t vort_elem(int dt) { return dt == MLX_DTYPE_F64 ? 8 : 4; }

// 0, or the status of a refused (nrec, ny, nx, symmetric)
int vort_check_extents(int64_t nrec, int64_t ny, int64_t nx, int symmetric) {
  using detail::fail;
  if (symmetric != 0 && symmetric != 1) return fail(MLX_E_ENUM, "symmetric must be 0 or 1");
  if (nrec < 0) return fail(MLX_E_SHAPE, "need nrec >= 0");
  if (ny < 1 + symmetric || nx < 1 + symmetric)
    return fail(MLX_E_SHAPE, "need ny, nx >= 1 (>= 2 on a symmetric grid): the corner extents");
  if (ny > kVortMaxCells || nx > kVortMaxCells / ny ||
      (nrec > 0 && ny * nx > kVortMaxCells / nrec))
    return fail(MLX_E_SHAPE, "need nrec * ny * nx <= 2^38");
  return 0;
}

}  // namespace
}  // namespace mlx

extern "C" int64_t mlx_vort_tile_width(int arith_dtype) {
  if (arith_dtype == MLX_DTYPE_F64) return (int64_t)mlx::kVortLanes * 2;
  if (arith_dtype == MLX_DTYPE_F32) return (int64_t)mlx::kVortLanes * 4;
  return 0;
}

extern "C" int64_t mlx_vort_records_per_launch(int64_t ny, int64_t nx, int arith_dtype) {
  if (ny < 1 || nx < 1 || ny > mlx::kVortMaxCells || nx > mlx::kVortMaxCells / ny ||
      !mlx::vort_dtype_ok(arith_dtype))
    return 0;
  int64_t gy, gz;
  return mlx::vort_records_per_launch(ny, nx, 16 / (int)mlx::vort_elem(arith_dtype), &gy, &gz);
}

extern "C" int mlx_vort_rel_vort(const void* u, const void* v, int field_dtype, const void* dx,
                                 const void* dy, const void* area, int metric_dtype, int64_t nrec,
                                 int64_t ny, int64_t nx, int symmetric, void* out, void* stream) {
  using namespace mlx;
  using detail::fail;
  if (!vort_dtype_ok(field_dtype) || !vort_dtype_ok(metric_dtype))
    return fail(MLX_E_ENUM, "field_dtype / metric_dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  if (int rc = vort_check_extents(nrec, ny, nx, symmetric)) return rc;
  if (nrec == 0) return 0;
  if (!u || !v || !dx || !dy || !area || !out)
    return fail(MLX_E_NULL, "u, v, dx, dy, area, out must not be NULL");
  const size_t ef = vort_elem(field_dtype), em = vort_elem(metric_dtype);
  const size_t eo = ef == 4 && em == 4 ? 4 : 8;
  if (!vort_aligned(u, ef) || !vort_aligned(v, ef))
    return fail(MLX_E_ALIGN, "u / v not element-aligned");
  if (!vort_aligned(dx, em) || !vort_aligned(dy, em) || !vort_aligned(area, em))
    return fail(MLX_E_ALIGN, "dx / dy / area not element-aligned");
  if (!vort_aligned(out, eo)) return fail(MLX_E_ALIGN, "out not element-aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (ef == 8)
    return em == 8 ? zeta_launch<double, double>(u, v, dx, dy, area, nrec, ny, nx, symmetric, out, st)
                   : zeta_launch<double, float>(u, v, dx, dy, area, nrec, ny, nx, symmetric, out, st);
  return em == 8 ? zeta_launch<float, double>(u, v, dx, dy, area, nrec, ny, nx, symmetric, out, st)
                 : zeta_launch<float, float>(u, v, dx, dy, area, nrec, ny, nx, symmetric, out, st);
}

extern "C" int mlx_vort_pv(const void* zeta, int zeta_dtype, const void* coriolis,
                           int coriolis_dtype, const void* n2, int n2_dtype, int64_t nrec,
                           int64_t ny, int64_t nx, int interp, int symmetric, double gravity,
                           int units, void* out, void* stream) {
  using namespace mlx;
  using detail::fail;
  if (!vort_dtype_ok(zeta_dtype) || !vort_dtype_ok(coriolis_dtype) || !vort_dtype_ok(n2_dtype))
    return fail(MLX_E_ENUM, "zeta / coriolis / n2 dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  if (interp != 0 && interp != 1) return fail(MLX_E_ENUM, "interp must be 0 or 1");
  if (units != MLX_VORT_UNITS_M && units != MLX_VORT_UNITS_CM)
    return fail(MLX_E_ENUM, "units must be MLX_VORT_UNITS_M or MLX_VORT_UNITS_CM");
  if (symmetric != 0 && symmetric != 1) return fail(MLX_E_ENUM, "symmetric must be 0 or 1");
  if (int rc = vort_check_extents(nrec, ny, nx, interp ? symmetric : 0)) return rc;
  if (nrec == 0) return 0;
  if (!zeta || !coriolis || !n2 || !out)
    return fail(MLX_E_NULL, "zeta, coriolis, n2, out must not be NULL");
  const size_t ez = vort_elem(zeta_dtype), ec = vort_elem(coriolis_dtype), en = vort_elem(n2_dtype);
  const size_t eo = ez == 4 && ec == 4 && en == 4 ? 4 : 8;
  if (!vort_aligned(zeta, ez) || !vort_aligned(coriolis, ec) || !vort_aligned(n2, en))
    return fail(MLX_E_ALIGN, "zeta / coriolis / n2 not element-aligned");
  if (!vort_aligned(out, eo)) return fail(MLX_E_ALIGN, "out not element-aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int cm = units == MLX_VORT_UNITS_CM;
#define MLX_VORT_PV(TZ, TC, TN) \
  pv_launch<TZ, TC, TN>(zeta, coriolis, n2, nrec, ny, nx, interp, symmetric, gravity, cm, out, st)
  if (ez == 8) {
    if (ec == 8) return en == 8 ? MLX_VORT_PV(double, double, double) : MLX_VORT_PV(double, double, float);
    return en == 8 ? MLX_VORT_PV(double, float, double) : MLX_VORT_PV(double, float, float);
  }
  if (ec == 8) return en == 8 ? MLX_VORT_PV(float, double, double) : MLX_VORT_PV(float, double, float);
  return en == 8 ? MLX_VORT_PV(float, float, double) : MLX_VORT_PV(float, float, float);
#undef MLX_VORT_PV
}

extern "C" int mlx_vort_rossby(const void* c, int c_dtype, const void* f, int f_dtype,
                               int64_t outer, int64_t plane, int64_t inner, void* out,
                               void* stream) {
  using namespace mlx;
  using detail::fail;
  if (!vort_dtype_ok(c_dtype) || !vort_dtype_ok(f_dtype))
    return fail(MLX_E_ENUM, "c_dtype / f_dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  if (outer < 0 || plane < 0 || inner < 0) return fail(MLX_E_SHAPE, "need outer, plane, inner >= 0");
  if (outer == 0 || plane == 0 || inner == 0) return 0;
  if (outer > kVortMaxCells || plane > kVortMaxCells / outer ||
      inner > kVortMaxCells / (outer * plane))
    return fail(MLX_E_SHAPE, "need outer * plane * inner <= 2^38");
  if (!c || !f || !out) return fail(MLX_E_NULL, "c, f, out must not be NULL");
  const size_t ec = vort_elem(c_dtype), ef = vort_elem(f_dtype);
  if (!vort_aligned(c, ec) || !vort_aligned(f, ef))
    return fail(MLX_E_ALIGN, "c / f not element-aligned");
  if (!vort_aligned(out, ec == 4 && ef == 4 ? 4 : 8))
    return fail(MLX_E_ALIGN, "out not element-aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t n = outer * plane * inner;
  if (ec == 8)
    return ef == 8 ? rossby_launch<double, double>(c, f, n, plane, inner, out, st)
                   : rossby_launch<double, float>(c, f, n, plane, inner, out, st);
  return ef == 8 ? rossby_launch<float, double>(c, f, n, plane, inner, out, st)
                 : rossby_launch<float, float>(c, f, n, plane, inner, out, st);
}
