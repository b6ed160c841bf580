// momlevel_regrid.hip -- mlx_regrid_apply (include/momlevel_regrid.h): the remap of the flattened
// (y, x) plane of a (nrec, nsrc) record to ndst destinations through a sparse weight table in a
// sliced ELLPACK layout.  An EXTENSION (momlevel has no such function); the specification is
// tests/regrid_numpy.py.
//
// k_regrid: wave64, 256-thread blocks.  A wave owns one slice of kRgSlice destinations, a lane one
// destination; a block (four neighbouring slices) walks a window of kRgRecWin records with num, den
// and cnt of each of them in registers, so that a table entry -- one coalesced read of col and of S
// per wave and k -- is read once for the window and the window's gathers are in flight together.
// The slice index is the fast axis of the grid (blockIdx.x) and the record window the slow one
// (blockIdx.y): blocks in flight together work on neighbouring destinations of the same records,
// whose source rows they share through the L2, while the record streams from memory about once.
//
// Rows of a slice differ in length: the wave runs to its longest row (clipped to what of the slice
// lies inside the table) and a lane past its own len[d] is predicated off, not branched around.
// Every position is checked against nentries and every col against nsrc before it is used as an
// address; a record index past nrec (a partial window) is clamped to the last record and its result
// not stored.  One lane per row means a very long row is slow (see the header).
//
// Every product and every add is formed alone (-ffp-contract=off and the pragma below); there is
// one path, one order of summation (k ascending), no atomics and no LDS: the bits of out[rec, d]
// depend on row d of the table and on record rec alone.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/momlevel_hip.h"
#include "../../include/momlevel_regrid.h"
#include "mlx_internal.hpp"
#include "mlx_pack.hpp"

#pragma clang fp contract(off)

namespace mlx {
namespace {

constexpr int kRgBlock = 256;  // 4 waves of 64
constexpr int kRgSlice = 64;   // destinations of a slice: one per lane
constexpr int kRgWaves = kRgBlock / kRgSlice;
constexpr int kRgRecWin = 8;
constexpr int kRgMaxGridY = 65535;
constexpr int64_t kRgMaxCells = (int64_t)1 << 38;
constexpr int64_t kRgMaxSrc = (int64_t)1 << 31;

constexpr int kRgSkipna = 0, kRgNoRenorm = 1, kRgPropagate = 2;  // the kernel's MODE

__device__ __forceinline__ bool rg_isnan(double x) { return x != x; }
__device__ __forceinline__ double rg_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

template <typename TO>
__device__ __forceinline__ TO rg_narrow(double r) {
  if constexpr (sizeof(TO) == 8) return rg_isnan(r) ? rg_nan() : r;
  else return rg_isnan(r) ? __int_as_float(0x7fc00000) : (float)r;  // rounded once
}

struct RegridArgs {
  const void* v;
  const int64_t* slice_ptr;
  const int32_t* len;
  const int32_t* col;
  const double* S;
  void* out;
  int64_t nentries, nrec, nsrc, ndst, nslices, nwin;
  double min_frac;
};

template <typename TV, typename TO, int MODE>
__global__ __launch_bounds__(kRgBlock) void k_regrid(const RegridArgs g) {
  constexpr int R = kRgRecWin;
  const TV* __restrict__ v = static_cast<const TV*>(g.v);
  const int32_t* __restrict__ col = g.col;
  const double* __restrict__ S = g.S;
  TO* __restrict__ out = static_cast<TO*>(g.out);
  const int lane = threadIdx.x & (kRgSlice - 1);
  const int64_t s = (int64_t)blockIdx.x * kRgWaves + (threadIdx.x / kRgSlice);
  if (s >= g.nslices) return;  // (wave-uniform; the kernel has no barrier)
  const int64_t d = s * kRgSlice + lane;
  const bool owner = d < g.ndst;
  const int mylen = owner ? g.len[d] : 0;
  const int lenc = mylen > 0 ? mylen : 0;
  int longest = lenc;
#pragma unroll
  for (int m = kRgSlice / 2; m >= 1; m >>= 1) {
    const int o = __shfl_xor(longest, m, kRgSlice);
    longest = o > longest ? o : longest;
  }
  // what of the slice lies inside the table: steps k with pos(d, k) < nentries for some lane
  const int64_t p0 = g.slice_ptr[s];
  int64_t kend = 0;
  if (p0 >= 0 && p0 < g.nentries) {
    const int64_t inside = (g.nentries - p0 + kRgSlice - 1) / kRgSlice;
    kend = longest < inside ? longest : inside;
  }

  for (int64_t win = blockIdx.y; win < g.nwin; win += gridDim.y) {
    const int64_t r0 = win * R;
    const TV* vr[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t rec = r0 + r < g.nrec ? r0 + r : g.nrec - 1;  // (clamped: read, not stored)
      vr[r] = v + rec * g.nsrc;
    }
    double num[R], den[R], tot = 0.0;
    int cnt[R];
#pragma unroll
    for (int r = 0; r < R; ++r) num[r] = 0.0, den[r] = 0.0, cnt[r] = 0;

    // the entry of step k + 1 is fetched before the gathers of step k are waited for
    int cn = -1;
    double wn = 0.0;
    if (0 < kend && 0 < lenc && p0 + lane < g.nentries) cn = col[p0 + lane], wn = S[p0 + lane];
#pragma unroll 2
    for (int64_t k = 0; k < kend; ++k) {
      const bool active = k < lenc && p0 + k * kRgSlice + lane < g.nentries;
      const int c = active ? cn : -1;
      const double w = active ? wn : 0.0;
      {
        const int64_t pos = p0 + (k + 1) * kRgSlice + lane;
        if (k + 1 < kend && k + 1 < lenc && pos < g.nentries) cn = col[pos], wn = S[pos];
      }
      const bool in_range = active && c >= 0 && (int64_t)c < g.nsrc;
      TV x[R];
#pragma unroll
      for (int r = 0; r < R; ++r) x[r] = (TV)0;
      if (in_range) {
#pragma unroll
        for (int r = 0; r < R; ++r) x[r] = vr[r][c];
      }
      tot += in_range ? w : 0.0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const double xd = (double)x[r];  // float -> double: exact
        const double p = w * xd;
        if constexpr (MODE == kRgPropagate) {
          num[r] += in_range ? p : 0.0;
        } else {
          const bool valid = in_range && !rg_isnan(xd);
          num[r] += valid ? p : 0.0;
          den[r] += valid ? w : 0.0;
          cnt[r] += valid;
        }
      }
    }

    if (owner) {
      const double floor = g.min_frac * tot;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r0 + r < g.nrec) {
          double res;
          if (mylen <= 0) res = rg_nan();
          else if constexpr (MODE == kRgPropagate) res = num[r];
          else if (cnt[r] == 0 || den[r] < floor) res = rg_nan();
          else if constexpr (MODE == kRgNoRenorm) res = num[r];
          else res = num[r] / den[r];
          out[(r0 + r) * g.ndst + d] = rg_narrow<TO>(res);
        }
      }
    }
  }
}

// gridDim.y of a call over nrec > 0 records: one block row per window of kRgRecWin records up to the
// cap, past which the rows stride.  The one rule: mlx_regrid_window_rows reports it, the launch
// uses it.
inline int64_t regrid_window_rows(int64_t nrec) {
  const int64_t nwin = ceil_div(nrec, kRgRecWin);
  return nwin < (int64_t)kRgMaxGridY ? nwin : (int64_t)kRgMaxGridY;
}

template <typename TV, typename TO>
void regrid_launch(const RegridArgs& g, int mode, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div(g.nslices, kRgWaves), (unsigned)regrid_window_rows(g.nrec)),
      block(kRgBlock);
  if (mode == kRgPropagate)
    hipLaunchKernelGGL((k_regrid<TV, TO, kRgPropagate>), grid, block, 0, st, g);
  else if (mode == kRgNoRenorm)
    hipLaunchKernelGGL((k_regrid<TV, TO, kRgNoRenorm>), grid, block, 0, st, g);
  else
    hipLaunchKernelGGL((k_regrid<TV, TO, kRgSkipna>), grid, block, 0, st, g);
}

inline bool rg_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return na > 0 && nb > 0 && x < y + nb && y < x + na;
}

}  // namespace
}  // namespace mlx

extern "C" int64_t mlx_regrid_slice(void) { return mlx::kRgSlice; }

extern "C" int64_t mlx_regrid_record_window(void) { return mlx::kRgRecWin; }

extern "C" int mlx_regrid_window_rows(int64_t nrec) {
  if (nrec <= 0 || nrec > mlx::kRgMaxCells) return 0;
  return (int)mlx::regrid_window_rows(nrec);
}

extern "C" int mlx_regrid_apply(const void* v, int dtype, const int64_t* slice_ptr,
                                const int32_t* len, const int32_t* col, const double* S,
                                int64_t nentries, double min_frac, int flags, int64_t nrec,
                                int64_t nsrc, int64_t ndst, void* out, int out_dtype, void* stream) {
  using namespace mlx;
  using detail::fail;
  using detail::hip_status;
  if (!is_float_dtype(dtype) || !is_float_dtype(out_dtype))
    return fail(MLX_E_ENUM, "dtype and out_dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  if (flags & ~(MLX_REGRID_PROPAGATE | MLX_REGRID_NO_RENORM))
    return fail(MLX_E_ENUM, "flags: MLX_REGRID_PROPAGATE and MLX_REGRID_NO_RENORM are the only ones");
  if (nrec < 0 || nsrc < 0 || ndst < 0 || nentries < 0)
    return fail(MLX_E_SHAPE, "nrec, nsrc, ndst and nentries must not be negative");
  if (nsrc >= kRgMaxSrc) return fail(MLX_E_SHAPE, "need nsrc < 2^31 (col is int32)");
  const int64_t widest = nsrc > ndst ? nsrc : ndst;
  if (widest > kRgMaxCells || (widest > 0 && nrec > kRgMaxCells / widest))
    return fail(MLX_E_SHAPE, "need nrec * max(nsrc, ndst) <= 2^38");
  if (!(min_frac >= 0.0 && min_frac <= 1.0))  // (a NaN compares false)
    return fail(MLX_E_SHAPE, "min_frac must lie in [0, 1]");
  if (nrec == 0 || ndst == 0) return 0;
  if ((!v && nsrc > 0) || !slice_ptr || !len || !out || (nentries > 0 && (!col || !S)))
    return fail(MLX_E_NULL, "v, slice_ptr, len, col, S and out must not be NULL");
  if (!aligned(v, dtype_size(dtype)) || !aligned(out, dtype_size(out_dtype)))
    return fail(MLX_E_ALIGN, "v / out not aligned to their element");
  if (!aligned(slice_ptr, 8) || !aligned(S, 8) || !aligned(len, 4) || !aligned(col, 4))
    return fail(MLX_E_ALIGN, "slice_ptr / S not 8-byte or len / col not 4-byte aligned");
  const int64_t nslices = ceil_div(ndst, kRgSlice);
  const size_t nout = (size_t)nrec * (size_t)ndst * dtype_size(out_dtype);
  if (rg_overlap(out, nout, v, (size_t)nrec * (size_t)nsrc * dtype_size(dtype)) ||
      rg_overlap(out, nout, slice_ptr, (size_t)(nslices + 1) * 8) ||
      rg_overlap(out, nout, len, (size_t)ndst * 4) ||
      rg_overlap(out, nout, col, (size_t)nentries * 4) ||
      rg_overlap(out, nout, S, (size_t)nentries * 8))
    return fail(MLX_E_SHAPE, "out overlaps an operand");

  RegridArgs g;
  g.v = v, g.slice_ptr = slice_ptr, g.len = len, g.col = col, g.S = S, g.out = out;
  g.nentries = nentries, g.nrec = nrec, g.nsrc = nsrc, g.ndst = ndst;
  g.nslices = nslices, g.nwin = ceil_div(nrec, kRgRecWin);
  g.min_frac = min_frac;
  const int mode = (flags & MLX_REGRID_PROPAGATE) ? kRgPropagate
                   : (flags & MLX_REGRID_NO_RENORM) ? kRgNoRenorm : kRgSkipna;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == MLX_DTYPE_F64) {
    if (out_dtype == MLX_DTYPE_F64) regrid_launch<double, double>(g, mode, st);
    else regrid_launch<double, float>(g, mode, st);
  } else {
    if (out_dtype == MLX_DTYPE_F64) regrid_launch<float, double>(g, mode, st);
    else regrid_launch<float, float>(g, mode, st);
  }
  return hip_status(hipGetLastError(), "k_regrid launch");
}
