// momlevel_spice.hip -- mlx_spice_map (include/momlevel_spice.h): seawater spiciness after Flament
// (2002), the array work of momlevel.spice.flament.spice (src/momlevel/spice/flament.py:82-90).
//
// A pointwise map: theta and S in (float64 or float32, each on its own), float64 out -- 24 / 20 /
// 16 bytes per cell and 29 fmas + 1 subtraction: the streams of K0 (mlx_eos_map) with less
// arithmetic and no divide, bound by HBM.  No LDS, no atomics, no workspace.
//
// Shape: wave64, 256-thread blocks.  A lane moves 16-byte packs with the `nt` policy (every byte is
// touched once): 2 cells per pack as soon as a float64 field takes part (its float32 partner then
// comes as an 8-byte load), 4 cells when both fields are float32 (one 16-byte load each, TWO
// 16-byte stores).  ONE TILE PER BLOCK, the shape of K0 and of the stream probes: a block loads
// kSpiceU = 2 packs per thread and field -- all loads of the tile are issued before the first fma
// -- stores, and ends.  Measured on one 0.25-degree step (scripts/bench_spice.py):
// 0.440 ms at float64, 1.02 x the two-read one-write probe; a grid of 8 blocks per CU striding
// over the tiles took 0.500 ms (4 packs in flight: 0.508; 1 pack: 0.563), slower than the density
// map.  (Beyond 2^23 tiles the blocks stride over the tiles: a HIP grid holds < 2^32 threads.)
//
// The three pointers need only their element alignment.  The host looks for the number of leading
// cells (< a pack) after which all three are aligned for their pack accesses; those cells and the
// ragged end (< a pack) are evaluated one by one by a few threads of block 0.  When no such number
// exists -- theta offset by one element and S not -- the whole range goes cell by cell (the same
// kernel with one-cell packs).  Every path evaluates spice_cell() on the widened operands: the bits
// of a cell do not depend on the path.
//
// Compile: with momlevel_hip.hip (csrc/build.py).  The fmas are explicit (__builtin_fma) and nothing
// else could contract, so the bits do not depend on -ffp-contract.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/momlevel_hip.h"
#include "../../include/momlevel_spice.h"
#include "mlx_internal.hpp"
#include "mlx_pack.hpp"

#pragma clang fp contract(off)

namespace mlx {
namespace {

constexpr int kSpiceBlock = 256;  // 4 waves of 64
constexpr int kSpiceU = 2;        // packs per thread and field in flight
constexpr int64_t kSpiceMaxBlocks = (int64_t)1 << 23;
constexpr int64_t kSpiceMaxCells = (int64_t)1 << 38;

// Flament (2002), table 1: the coefficient of theta^j (S - 35)^k, here one ROW PER POWER OF
// (S - 35) -- the order the nested scheme consumes them in.  Compile-time constants: after
// unrolling they are scalar-register operands of the fmas.
__device__ __forceinline__ double spice_cell(double theta, double so) {
  constexpr double c[5][6] = {
      //  theta^0     theta^1     theta^2      theta^3      theta^4     theta^5
      {0.0,         5.1655e-2,  6.64783e-3,  -5.4023e-5,  3.949e-7,   -6.36e-10},    // s^0
      {7.7442e-1,   2.034e-3,   -2.4681e-4,  7.326e-6,    -3.029e-8,  -1.309e-9},    // s^1
      {-5.85e-3,    -2.742e-4,  -1.428e-5,   7.0036e-6,   -3.8209e-7, 6.048e-9},     // s^2
      {-9.84e-4,    -8.5e-6,    3.337e-5,    -3.0412e-6,  1.0012e-7,  -1.1409e-9},   // s^3
      {-2.06e-4,    1.36e-5,    7.894e-6,    -1.0853e-6,  4.7133e-8,  -6.676e-10},   // s^4
  };
  const double s = so - 35.0;
  double q[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    double a = c[k][5];
#pragma unroll
    for (int j = 4; j >= 0; --j) a = __builtin_fma(a, theta, c[k][j]);
    q[k] = a;
  }
  double pi = q[4];
#pragma unroll
  for (int k = 3; k >= 0; --k) pi = __builtin_fma(pi, s, q[k]);
  return pi;
}

// P cells of X, widened: one nt load of sizeof(X) * P bytes (16, 8, or the element)
template <typename X, int P>
__device__ __forceinline__ void spice_load(const X* __restrict__ p, double (&v)[P]) {
  const Pack<X, P> raw = load_pack<X, P, true>(p);
#pragma unroll
  for (int k = 0; k < P; ++k) v[k] = (double)raw.v[k];  // float -> double: exact
}

// Cells [head, head + P * npacks) in packs of P; cells [0, head) and [head + P * npacks, n) -- fewer
// than P each -- one by one.  The host guarantees theta + head, so + head and out + head aligned
// for the pack accesses.
template <typename TT, typename TS, int P>
__global__ __launch_bounds__(kSpiceBlock) void k_spice_map(const TT* __restrict__ theta,
                                                           const TS* __restrict__ so,
                                                           double* __restrict__ out, int64_t n,
                                                           int64_t head, int64_t npacks) {
  constexpr int U = kSpiceU;
  constexpr int64_t kTile = (int64_t)kSpiceBlock * U;
  const int64_t ntiles = (npacks + kTile - 1) / kTile;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * kTile + threadIdx.x;
    double t[U][P], s[U][P];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + (int64_t)u * kSpiceBlock;
      if (i < npacks) {
        spice_load<TT, P>(theta + head + P * i, t[u]);
        spice_load<TS, P>(so + head + P * i, s[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + (int64_t)u * kSpiceBlock;
      if (i < npacks) {
        Pack<double, P> r;
#pragma unroll
        for (int k = 0; k < P; ++k) r.v[k] = spice_cell(t[u][k], s[u][k]);
        store_pack<double, P, true>(out + head + P * i, r);  // (four cells: two accesses of 16)
      }
    }
  }
  if constexpr (P > 1) {
    const int64_t body_end = head + P * npacks, edge = head + (n - body_end);  // edge < 2 P
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < edge) {
      const int64_t e = threadIdx.x;
      const int64_t i = e < head ? e : body_end + (e - head);
      out[i] = spice_cell((double)theta[i], (double)so[i]);
    }
  }
}

inline bool spice_aligned(const void* p, int64_t cells, size_t elem, size_t width) {
  return (reinterpret_cast<uintptr_t>(p) + (uintptr_t)cells * elem) % width == 0;
}

template <typename TT, typename TS>
int spice_launch(const void* theta, const void* so, int64_t n, double* out, hipStream_t st) {
  // both float32: 4 cells = one 16-byte load per field; otherwise 2 cells = 16 bytes of float64
  constexpr int P = (sizeof(TT) == 4 && sizeof(TS) == 4) ? 4 : 2;
  int64_t head = -1;
  for (int h = 0; h < P && head < 0; ++h)
    if (spice_aligned(theta, h, sizeof(TT), sizeof(TT) * P) &&
        spice_aligned(so, h, sizeof(TS), sizeof(TS) * P) && spice_aligned(out, h, 8, 16))
      head = h;
  const int64_t cap = kSpiceMaxBlocks;
  const int64_t tile = (int64_t)kSpiceBlock * kSpiceU;
  if (head < 0) {  // the pointers disagree about alignment: cell by cell
    const int64_t ntiles = (n + tile - 1) / tile;
    const dim3 grid((unsigned)(ntiles < cap ? ntiles : cap));
    hipLaunchKernelGGL((k_spice_map<TT, TS, 1>), grid, dim3(kSpiceBlock), 0, st, (const TT*)theta,
                       (const TS*)so, out, n, (int64_t)0, n);
  } else {
    if (head > n) head = n;
    const int64_t npacks = (n - head) / P;
    int64_t ntiles = (npacks + tile - 1) / tile;
    if (ntiles < 1) ntiles = 1;  // (block 0 owns the edge cells)
    const dim3 grid((unsigned)(ntiles < cap ? ntiles : cap));
    hipLaunchKernelGGL((k_spice_map<TT, TS, P>), grid, dim3(kSpiceBlock), 0, st, (const TT*)theta,
                       (const TS*)so, out, n, head, npacks);
  }
  return detail::hip_status(hipGetLastError(), "k_spice_map launch");
}

}  // namespace
}  // namespace mlx

extern "C" int mlx_spice_map(const void* theta, int theta_dtype, const void* so, int so_dtype,
                             int64_t n, double* out, void* stream) {
  using namespace mlx;
  using detail::fail;
  if (theta_dtype != MLX_DTYPE_F64 && theta_dtype != MLX_DTYPE_F32)
    return fail(MLX_E_ENUM, "theta_dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  if (so_dtype != MLX_DTYPE_F64 && so_dtype != MLX_DTYPE_F32)
    return fail(MLX_E_ENUM, "so_dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  if (n < 0 || n > kSpiceMaxCells) return fail(MLX_E_SHAPE, "need 0 <= n <= 2^38");
  if (n == 0) return 0;
  if (!theta || !so || !out) return fail(MLX_E_NULL, "theta, so, out must not be NULL");
  const bool t64 = theta_dtype == MLX_DTYPE_F64, s64 = so_dtype == MLX_DTYPE_F64;
  if (!spice_aligned(theta, 0, 1, t64 ? 8 : 4) || !spice_aligned(so, 0, 1, s64 ? 8 : 4))
    return fail(MLX_E_ALIGN, "theta / so not element-aligned");
  if (!spice_aligned(out, 0, 1, 8)) return fail(MLX_E_ALIGN, "out not 8-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (t64) return s64 ? spice_launch<double, double>(theta, so, n, out, st)
                      : spice_launch<double, float>(theta, so, n, out, st);
  return s64 ? spice_launch<float, double>(theta, so, n, out, st)
             : spice_launch<float, float>(theta, so, n, out, st);
}
