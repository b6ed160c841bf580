// momlevel_eof.hip -- mlx_gram_matrix (include/momlevel_eof.h): G[s,t] = sum_c b1[s,c] * b2[t,c] over
// the cells of one or two (time, cells) records, b = (y - center) * scale formed while the rows are
// staged.  An EXTENSION (momlevel has no such function); the specification is tests/eof_numpy.py.
//
// The one arithmetic-bound kernel of the library, and the one that uses the matrix cores:
// v_mfma_f64_16x16x4_f64 through __builtin_amdgcn_mfma_f64_16x16x4f64.  Its lane maps (wave64):
//   A operand: lane l holds A[i = l & 15][k = l >> 4]      B operand: B[k = l >> 4][j = l & 15]
//   C / D:     register r of lane l holds D[row = (l >> 4) + 4 r][col = l & 15]
// -- the float64 C/D map, NOT the  row = 4 (l >> 4) + r  of every other shape.
//
// STAGE 1, k_gram_partial: wave64, 256-thread blocks.  A block owns the output tile (ti, tj) of
// kGramTile x kGramTile elements and the cells [range * cells, min(n, (range + 1) * cells)).  The
// four waves split the tile 2 x 2: a wave holds a 64 x 64 quarter as 4 x 4 MFMA tiles, 16 float64x4
// accumulators.  The range is walked in chunks of kGramChunk = 16 cells:
//   - every thread loads its packs of the chunk's rows raw (16 bytes along the cells: 2 float64 or 4
//     float32; 8 or 4 lanes a row) and the center / scale of ITS cells (the same for all its rows),
//     for the NEXT chunk, before the MFMAs of the current one: the loads land behind the matrix work;
//   - at the hand-over it forms b = ok ? (y - center) * scale : 0 -- one subtraction, one multiply,
//     contraction off -- and writes it to LDS.  Cells past the range and rows past nt are written as
//     0 and never read from memory;
//   - each wave reads its fragments (ds_read_b64, lane l: row l & 15, cell kk + (l >> 4)) and issues
//     16 MFMAs per 4 cells.
// In the symmetric form a diagonal tile stages one operand and reads both fragments from it, and the
// wave below the diagonal of a diagonal tile issues no MFMAs (stage 2 does not read its quarter).
//
// LDS IMAGE: [row][kGramChunk + kGramPad] float64, kGramPad = 2: a row is 18 float64 = 144 bytes.
// ds_read_b64 serves lanes 0-31 and 32-63 in one cycle each when the 32 lanes fall on 32 different
// 8-byte bank pairs, (address / 8) mod 32.  The 32 lanes of a group are rows r = 0..15 at cells k and
// k + 1: (18 r + k) mod 32 -- 18 r mod 32 runs through the 16 even residues, k + 1 gives the odd
// ones: no conflicts.  Unpadded (16 float64 a row) the 16 rows fall on 2 residues: 8-way.  144 bytes
// keep a row 16-byte aligned for the writes.  2 x 128 x 144 bytes = 36 KiB a block.
//
// STAGE 2, k_gram_finish: one thread per element of a tile pair adds the ranges' partials in
// ascending order and writes G[s,t] and, in the symmetric form, G[t,s].
//
// Compile: with momlevel_hip.hip (csrc/build.py), -ffp-contract=off and the pragma below.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/momlevel_hip.h"
#include "../../include/momlevel_eof.h"
#include "mlx_internal.hpp"
#include "mlx_pack.hpp"
#include "mlx_record.hpp"

#pragma clang fp contract(off)

#ifndef MLX_GRAM_LDS_PAD
#define MLX_GRAM_LDS_PAD 2  // (0 builds the conflicting image, for the tuning log only)
#endif

namespace mlx {
namespace {

constexpr int kGramBlock = 256;  // 4 waves of 64, 2 x 2 over the tile
constexpr int kGramTile = 128;   // rows and columns of G per block
constexpr int kGramWave = 64;    // rows and columns per wave: 4 x 4 MFMA tiles of 16 x 16
constexpr int kGramChunk = 16;   // cells per LDS stage: 4 MFMA steps of 4
constexpr int kGramPad = MLX_GRAM_LDS_PAD;
constexpr int kGramStride = kGramChunk + kGramPad;  // float64 per LDS row
constexpr int64_t kGramMinCells = 2048;  // a block's range below MLX_GRAM_MAX_SPLIT of them
constexpr int64_t kGramMaxSteps = (int64_t)1 << 31;
constexpr int64_t kGramTileElems = (int64_t)kGramTile * kGramTile;

typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool gram_isnan(double x) { return x != x; }

// what a thread holds of one operand's chunk: its pack of each of its rows, raw
template <typename T>
struct GramRaw {
  static constexpr int P = 16 / (int)sizeof(T);          // cells per lane
  static constexpr int kLanesPerRow = kGramChunk / P;    // 8 (float64) or 4 (float32)
  static constexpr int kRowsPerPass = kGramBlock / kLanesPerRow;
  static constexpr int kPasses = kGramTile / kRowsPerPass;
  T v[kPasses][P];
};

// the rows [row0, row0 + kGramTile) of y at the cells [c, c + kGramChunk) that lie below `cend`
// (<= n): rows >= nt and cells >= cend are not read (0)
template <typename T>
__device__ __forceinline__ void gram_load(const T* __restrict__ y, int64_t nt, int64_t n,
                                          int64_t row0, int64_t c, int64_t cend, GramRaw<T>& raw) {
  typedef GramRaw<T> R;
  const int tid = threadIdx.x;
  const int lr = tid / R::kLanesPerRow, lc = (tid % R::kLanesPerRow) * R::P;
  const int64_t c0 = c + lc;
#pragma unroll
  for (int p = 0; p < R::kPasses; ++p) {
    const int64_t row = row0 + p * R::kRowsPerPass + lr;
#pragma unroll
    for (int k = 0; k < R::P; ++k) raw.v[p][k] = (T)0;
    if (row < nt) {
      const T* q = y + row * n + c0;
      if (c0 + R::P <= cend && (reinterpret_cast<uintptr_t>(q) % 16) == 0) {
        const Pack<T, R::P> pk = load_pack<T, R::P, false>(q);
#pragma unroll
        for (int k = 0; k < R::P; ++k) raw.v[p][k] = pk.v[k];
      } else {
#pragma unroll
        for (int k = 0; k < R::P; ++k)
          if (c0 + k < cend) raw.v[p][k] = q[k];
      }
    }
  }
}

// center and scale of this thread's P cells of the chunk at c; a cell past cend is excluded (NaN)
template <int P>
__device__ __forceinline__ void gram_load_maps(const double* __restrict__ center,
                                               const double* __restrict__ scale, int64_t c0,
                                               int64_t cend, double (&cen)[P], double (&scl)[P]) {
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const bool in = c0 + k < cend;
    cen[k] = (in && center) ? center[c0 + k] : 0.0;
    scl[k] = in ? (scale ? scale[c0 + k] : 1.0) : __longlong_as_double(0x7ff8000000000000LL);
  }
}

// b = ok ? (y - center) * scale : 0 into the LDS image of one operand
template <typename T>
__device__ __forceinline__ void gram_stage(const GramRaw<T>& raw, const double (&cen)[GramRaw<T>::P],
                                           const double (&scl)[GramRaw<T>::P],
                                           const bool (&ok)[GramRaw<T>::P],
                                           double* __restrict__ tile) {
  typedef GramRaw<T> R;
  const int tid = threadIdx.x;
  const int lr = tid / R::kLanesPerRow, lc = (tid % R::kLanesPerRow) * R::P;
#pragma unroll
  for (int p = 0; p < R::kPasses; ++p) {
    double* dst = tile + (p * R::kRowsPerPass + lr) * kGramStride + lc;
#pragma unroll
    for (int k = 0; k < R::P; ++k) {
      const double d = (double)raw.v[p][k] - cen[k];  // float -> double: exact
      const double b = d * scl[k];
      dst[k] = ok[k] ? b : 0.0;
    }
  }
}

// the tile pair of a block: SYM walks the pairs ti <= tj row by row
template <bool SYM>
__device__ __forceinline__ void gram_pair(int64_t pair, int64_t ntile1, int64_t ntile2, int64_t& ti,
                                          int64_t& tj) {
  if constexpr (SYM) {
    ti = 0;
    while (pair >= ntile1 - ti) {
      pair -= ntile1 - ti;
      ++ti;
    }
    tj = ti + pair;
  } else {
    ti = pair / ntile2;
    tj = pair % ntile2;
  }
}

// partials[((range * npairs + pair) * kGramTile + row) * kGramTile + col]
template <typename T1, typename T2, bool SYM>
__global__ __launch_bounds__(kGramBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_gram_partial(
    const T1* __restrict__ y1, const double* __restrict__ center1, int64_t nt1,
    const T2* __restrict__ y2, const double* __restrict__ center2, int64_t nt2,
    const double* __restrict__ scale, int64_t n, int64_t cells, int64_t ntile1, int64_t ntile2,
    int64_t npairs, double* __restrict__ partials) {
  typedef GramRaw<T1> R1;
  typedef GramRaw<T2> R2;
  __shared__ __attribute__((aligned(16))) double lds[2][kGramTile * kGramStride];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1;
  const int64_t pair = blockIdx.x % npairs, range = blockIdx.x / npairs;
  int64_t ti, tj;
  gram_pair<SYM>(pair, ntile1, ntile2, ti, tj);
  const bool diag = SYM && ti == tj;
  const bool active = !(diag && wr > wc);  // wave-uniform
  const int64_t cbeg = range * cells;
  const int64_t cend = cbeg + cells < n ? cbeg + cells : n;
  const int64_t row1 = ti * kGramTile, row2 = tj * kGramTile;
  double* tileA = lds[0];
  double* tileB = diag ? lds[0] : lds[1];

  f64x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

  R1 ra;
  R2 rb;
  double cen1[R1::P], scl1[R1::P], oth1[R1::P], cen2[R2::P], scl2[R2::P], oth2[R2::P];
  const int lc1 = (tid % R1::kLanesPerRow) * R1::P, lc2 = (tid % R2::kLanesPerRow) * R2::P;

  // what a chunk needs from memory: the raw packs, and the maps of this thread's cells (a cell is
  // excluded by either center, so each operand's lanes read the other operand's center too).  In
  // the symmetric form the host passes y2 = y1 and center2 = center1.
  auto fetch = [&](int64_t c) {
    double unused1[R1::P], unused2[R2::P];
    gram_load<T1>(y1, nt1, n, row1, c, cend, ra);
    gram_load_maps<R1::P>(center1, scale, c + lc1, cend, cen1, scl1);
    if constexpr (SYM) {
#pragma unroll
      for (int k = 0; k < R1::P; ++k) oth1[k] = 0.0;
    } else {
      gram_load_maps<R1::P>(center2, nullptr, c + lc1, cend, oth1, unused1);
    }
    if (!diag) {
      gram_load<T2>(y2, nt2, n, row2, c, cend, rb);
      gram_load_maps<R2::P>(center2, scale, c + lc2, cend, cen2, scl2);
      if constexpr (SYM) {
#pragma unroll
        for (int k = 0; k < R2::P; ++k) oth2[k] = 0.0;
      } else {
        gram_load_maps<R2::P>(center1, nullptr, c + lc2, cend, oth2, unused2);
      }
    }
  };
  auto stage = [&]() {
    bool ok1[R1::P], ok2[R2::P];
#pragma unroll
    for (int k = 0; k < R1::P; ++k)
      ok1[k] = !gram_isnan(cen1[k]) && !gram_isnan(scl1[k]) && !gram_isnan(oth1[k]);
    gram_stage<T1>(ra, cen1, scl1, ok1, tileA);
    if (!diag) {
#pragma unroll
      for (int k = 0; k < R2::P; ++k)
        ok2[k] = !gram_isnan(cen2[k]) && !gram_isnan(scl2[k]) && !gram_isnan(oth2[k]);
      gram_stage<T2>(rb, cen2, scl2, ok2, tileB);
    }
  };

  const double* fa = tileA + (wr * kGramWave + (lane & 15)) * kGramStride + (lane >> 4);
  const double* fb = tileB + (wc * kGramWave + (lane & 15)) * kGramStride + (lane >> 4);

  fetch(cbeg);
  for (int64_t c = cbeg; c < cend; c += kGramChunk) {
    stage();
    __syncthreads();
    if (c + kGramChunk < cend) fetch(c + kGramChunk);
    if (active) {
#pragma unroll
      for (int kk = 0; kk < kGramChunk; kk += 4) {
        double a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a[i] = fa[i * 16 * kGramStride + kk];
          b[i] = fb[i * 16 * kGramStride + kk];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  if (active) {
    double* out = partials + (range * npairs + pair) * kGramTileElems;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = wr * kGramWave + i * 16 + (lane >> 4) + 4 * r;  // the float64 C/D map
          const int col = wc * kGramWave + j * 16 + (lane & 15);
          out[row * kGramTile + col] = acc[i][j][r];
        }
  }
}

// G[s,t] = the partials of the element, ranges ascending; SYM: elements on and above the diagonal,
// mirrored
template <bool SYM>
__global__ __launch_bounds__(kGramBlock) void k_gram_finish(const double* __restrict__ partials,
                                                            int64_t nt1, int64_t nt2,
                                                            int64_t ntile1, int64_t ntile2,
                                                            int64_t npairs, int64_t nranges,
                                                            double* __restrict__ G) {
  const int64_t e = (int64_t)blockIdx.x * kGramBlock + threadIdx.x;  // < npairs * kGramTileElems
  const int64_t pair = e / kGramTileElems;
  const int row = (int)((e % kGramTileElems) / kGramTile), col = (int)(e % kGramTile);
  int64_t ti, tj;
  gram_pair<SYM>(pair, ntile1, ntile2, ti, tj);
  const int64_t s = ti * kGramTile + row, t = tj * kGramTile + col;
  if (s >= nt1 || t >= nt2 || (SYM && t < s)) return;
  double sum = 0.0;
  for (int64_t r = 0; r < nranges; ++r) sum += partials[r * npairs * kGramTileElems + e];
  G[s * nt2 + t] = sum;
  if (SYM && s != t) G[t * nt2 + s] = sum;
}

// 8 independent accumulators a wave: the issue rate of v_mfma_f64_16x16x4_f64
__global__ __launch_bounds__(kGramBlock) void k_gram_issue_probe(int64_t iters,
                                                                 double* __restrict__ sink) {
  const double a = 1.0 + (double)(threadIdx.x & 7) * 0.125, b = 1.0 / (1.0 + (double)(threadIdx.x & 3));
  f64x4 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int64_t it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  sink[(int64_t)blockIdx.x * kGramBlock + threadIdx.x] = s;
}

inline int64_t gram_cells_of(int64_t n) {
  if (n < 1) return 0;
  const int64_t even = ceil_div(ceil_div(n, MLX_GRAM_MAX_SPLIT), kGramChunk) * kGramChunk;
  return even > kGramMinCells ? even : kGramMinCells;
}

// the launch geometry of valid arguments; false for what mlx_gram_matrix refuses by shape
struct GramPlan {
  int64_t ntile1, ntile2, npairs, cells, nranges;
  size_t bytes;
};

inline bool gram_plan(int64_t nt1, int64_t nt2, int64_t n, bool sym, GramPlan& g) {
  if (!record_fits(nt1, n, kGramMaxSteps) || (!sym && !record_fits(nt2, n, kGramMaxSteps)))
    return false;
  g.ntile1 = ceil_div(nt1, kGramTile);
  g.ntile2 = sym ? g.ntile1 : ceil_div(nt2, kGramTile);
  g.npairs = sym ? g.ntile1 * (g.ntile1 + 1) / 2 : g.ntile1 * g.ntile2;  // < 2^49
  g.cells = gram_cells_of(n);
  g.nranges = ceil_div(n, g.cells);  // <= MLX_GRAM_MAX_SPLIT
  // grid x of both stages: npairs * nranges and npairs * kGramTileElems / kGramBlock blocks
  if (g.npairs > (int64_t)2147483647 / (kGramTileElems / kGramBlock)) return false;
  g.bytes = (size_t)g.npairs * (size_t)g.nranges * (size_t)kGramTileElems * sizeof(double);
  return true;
}

}  // namespace
}  // namespace mlx

static_assert(MLX_GRAM_MAX_SPLIT <= mlx::kGramTileElems / mlx::kGramBlock,
              "stage 1 has no more blocks than stage 2: one grid check covers both");

extern "C" int mlx_gram_tile(void) { return mlx::kGramTile; }

extern "C" int64_t mlx_gram_cells(int64_t n) { return mlx::gram_cells_of(n); }

extern "C" size_t mlx_gram_matrix_workspace_bytes(int64_t nt1, int64_t nt2, int64_t n) {
  mlx::GramPlan g;
  if (nt2 < 0 || !mlx::gram_plan(nt1, nt2, n, nt2 == 0, g)) return 0;
  return g.bytes;
}

extern "C" int mlx_gram_matrix(const void* y1, int dtype1, const double* center1, int64_t nt1,
                             const void* y2, int dtype2, const double* center2, int64_t nt2,
                             const double* scale, int64_t n, double* G, void* workspace,
                             size_t workspace_bytes, void* stream) {
  using namespace mlx;
  using detail::fail;
  using detail::hip_status;
  const bool sym = y2 == nullptr;
  if (!is_float_dtype(dtype1) || (!sym && !is_float_dtype(dtype2)))
    return fail(MLX_E_ENUM, "dtype1 / dtype2 must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  if (nt1 < 1 || n < 1 || (!sym && nt2 < 1)) return fail(MLX_E_SHAPE, "need nt1, nt2 and n >= 1");
  GramPlan g;
  if (!gram_plan(nt1, nt2, n, sym, g))
    return fail(MLX_E_SHAPE, "need nt < 2^31, n <= 2^38, nt * n addressable and at most 2^31 - 1 blocks");
  if (!y1 || !G || !workspace) return fail(MLX_E_NULL, "y1, G and workspace must not be NULL");
  if (workspace_bytes < g.bytes || !aligned(workspace, 8))
    return fail(MLX_E_WORKSPACE,
                "workspace too small (mlx_gram_matrix_workspace_bytes) or not 8-byte aligned");
  if (!aligned(y1, dtype_size(dtype1)) || (!sym && !aligned(y2, dtype_size(dtype2))))
    return fail(MLX_E_ALIGN, "y1 / y2 not aligned to their element");
  if (!aligned(center1, 8) || (!sym && !aligned(center2, 8)) || !aligned(scale, 8) || !aligned(G, 8))
    return fail(MLX_E_ALIGN, "center1 / center2 / scale / G not 8-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* partials = static_cast<double*>(workspace);
  const dim3 grid((unsigned)(g.npairs * g.nranges)), block(kGramBlock);
  const int64_t ncols = sym ? nt1 : nt2;
#define MLX_GRAM(T1, T2, SYM)                                                                    \
  hipLaunchKernelGGL((k_gram_partial<T1, T2, SYM>), grid, block, 0, st, (const T1*)y1, center1,  \
                     nt1, (const T2*)y2, center2, ncols, scale, n, g.cells, g.ntile1, g.ntile2,  \
                     g.npairs, partials)
  const bool a64 = dtype1 == MLX_DTYPE_F64, b64 = dtype2 == MLX_DTYPE_F64;
  if (sym) {  // the second operand is the first
    y2 = y1;
    center2 = center1;
    if (a64) MLX_GRAM(double, double, true);
    else MLX_GRAM(float, float, true);
  } else if (a64) {
    if (b64) MLX_GRAM(double, double, false);
    else MLX_GRAM(double, float, false);
  } else {
    if (b64) MLX_GRAM(float, double, false);
    else MLX_GRAM(float, float, false);
  }
#undef MLX_GRAM
  if (int rc = hip_status(hipGetLastError(), "k_gram_partial launch")) return rc;
  const dim3 fgrid((unsigned)(g.npairs * (kGramTileElems / kGramBlock)));
  if (sym)
    hipLaunchKernelGGL(k_gram_finish<true>, fgrid, block, 0, st, (const double*)partials, nt1,
                       ncols, g.ntile1, g.ntile2, g.npairs, g.nranges, G);
  else
    hipLaunchKernelGGL(k_gram_finish<false>, fgrid, block, 0, st, (const double*)partials, nt1,
                       ncols, g.ntile1, g.ntile2, g.npairs, g.nranges, G);
  return hip_status(hipGetLastError(), "k_gram_finish launch");
}

extern "C" int mlx_gram_issue_probe(int64_t iters, int64_t blocks, double* sink, int64_t* flop,
                                    void* stream) {
  using namespace mlx;
  using detail::fail;
  using detail::hip_status;
  if (iters < 1 || blocks < 1 || blocks > ((int64_t)1 << 20) || iters > ((int64_t)1 << 40))
    return fail(MLX_E_SHAPE, "need 1 <= iters <= 2^40 and 1 <= blocks <= 2^20");
  if (!sink) return fail(MLX_E_NULL, "sink must not be NULL");
  if (!aligned(sink, 8)) return fail(MLX_E_ALIGN, "sink not 8-byte aligned");
  if (flop) *flop = iters * blocks * (kGramBlock / 64) * 8 * (2 * 16 * 16 * 4);
  hipLaunchKernelGGL(k_gram_issue_probe, dim3((unsigned)blocks), dim3(kGramBlock), 0,
                     static_cast<hipStream_t>(stream), iters, sink);
  return hip_status(hipGetLastError(), "k_gram_issue_probe launch");
}
