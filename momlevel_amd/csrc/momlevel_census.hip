// momlevel_census.hip -- mlx_census_histogram (include/momlevel_census.h): per record of a
// (nrec, ncells) record, the count, the weight and the weight * value of the cells of every bin of a
// table over one or two binning fields.  An EXTENSION (momlevel has no such function); the
// specification is tests/census_numpy.py (numpy.histogramdd with explicit edges).
//
// STAGE 1, k_census_partial: wave64, 256-thread blocks, mlx_census_blocks(ncells) blocks per record;
// block b walks the tiles b, b + blocks, ... of kCensusTile cells in ascending order (the next
// tile's loads are issued before the current one is resolved).  In a tile thread t owns the cells
// 4t .. 4t + 3 of every operand: one 16-byte `nt` access of a float32 operand and two of a float64
// one when the tile is whole and its first cell 16-byte aligned, cell by cell (the same cells to the
// same lanes) when not.  The edges are staged in LDS once per block; a cell's bin comes from a
// branch-free binary search whose trip count depends on the number of edges only, the searches of a
// thread's four cells walking in step.
//
// Resolving 64 lanes onto bins, per k = 0 .. 3: a wave-uniform leader loop.  While lanes remain: the
// lowest remaining lane (s_ff1 of the 64-bit ballot: a scalar) names a bin, read with readlane at
// that scalar index; the lanes of that bin are the ballot of (bin == leader's bin); members
// contribute w (and w * v), every other lane +0.0, to a fixed 64-lane __shfl_down tree; lane 0 adds
// the tree's sum to that one bin of the WAVE'S OWN LDS histogram with a plain read-modify-write and
// advances the count by the ballot's popcount; the members retire.  One lane writes one bin per
// step: no LDS atomics, no reliance on the order of conflicting writes.  Lanes past the record and
// cells that are left out stay in the loop as non-members (bin -1): nobody leaves before the
// shuffles.  Every iteration retires at least the leader, so the loop ends after at most 64.
//
// After a barrier the block adds its four histograms in ascending wave order and stores one partial
// per (record, block, bin): workspace[((rec * blocks + b) * K + k) * nbins + bin], 8-byte words, k =
// 0 the count (int64), 1 wsum, 2 vsum.
//
// STAGE 2, k_census_finish: one thread per (record, bin) adds the partials in ascending block order.
//
// Compile: with momlevel_hip.hip (csrc/build.py), -ffp-contract=off and the pragma below: w * v is
// one rounding, then one add.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/momlevel_hip.h"
#include "../../include/momlevel_census.h"
#include "mlx_internal.hpp"
#include "mlx_pack.hpp"

#pragma clang fp contract(off)

namespace mlx {
namespace {

constexpr int kCensusBlock = 256;  // 4 waves of 64
constexpr int kCensusWaves = kCensusBlock / 64;
constexpr int kCensusC = 4;  // consecutive cells a thread owns in a tile
constexpr int64_t kCensusTile = (int64_t)kCensusBlock * kCensusC;
constexpr int64_t kCensusTilesPerBlock = 8;  // a block has at least this many tiles before ...
constexpr int64_t kCensusMaxBlocks = 1024;   // ... a record is cut into this many blocks
constexpr int64_t kCensusLds = 64 * 1024;    // bytes of LDS a block may ask for
constexpr int64_t kCensusMaxCells = (int64_t)1 << 38;
constexpr int64_t kCensusMaxElems = (int64_t)1 << 40;
constexpr int64_t kCensusMaxGrid = ((int64_t)1 << 31) - 1;

struct CNone {};  // an operand that is not there

template <typename T>
struct CCells {
  T v[kCensusC];
};
template <>
struct CCells<CNone> {};

__device__ __forceinline__ bool census_isnan(double x) { return x != x; }

// the four cells of one operand this thread owns in the tile at rec[base]; cells past the record
// read as 0 (their lanes are non-members)
template <typename T, bool NT>
__device__ __forceinline__ void census_load(const T* __restrict__ rec, int64_t base, int64_t left,
                                            bool whole, CCells<T>& x) {
  if constexpr (!__is_same(T, CNone)) {
    const int tid = threadIdx.x;
    const T* p = rec + base;
    if (whole && (reinterpret_cast<uintptr_t>(p) % 16) == 0) {
      const Pack<T, kCensusC> r = load_pack<T, kCensusC, NT>(p + (int64_t)tid * kCensusC);
#pragma unroll
      for (int k = 0; k < kCensusC; ++k) x.v[k] = r.v[k];
    } else {
#pragma unroll
      for (int k = 0; k < kCensusC; ++k) {
        const int64_t i = (int64_t)tid * kCensusC + k;
        x.v[k] = i < left ? (NT ? __builtin_nontemporal_load(p + i) : p[i]) : (T)0;
      }
    }
  }
}

// searchsorted(e[0 .. n], x, side="right") - 1 for the thread's four cells, the last edge closed when
// `closed`; -1 when x lies in no bin.  The four searches walk in step, so their LDS reads are in
// flight together; the trip count depends on n alone; e[] is read at 0 .. n only, whatever it holds.
__device__ __forceinline__ void census_bins(const double* __restrict__ e, int n, bool closed,
                                            const double (&x)[kCensusC], int (&bin)[kCensusC]) {
  int base[kCensusC];
#pragma unroll
  for (int k = 0; k < kCensusC; ++k) base[k] = 0;
  int len = n + 1;
  while (len > 1) {
    const int half = len >> 1;
#pragma unroll
    for (int k = 0; k < kCensusC; ++k) base[k] += (e[base[k] + half - 1] <= x[k]) ? half : 0;
    len -= half;
  }
  const double last = e[n];
#pragma unroll
  for (int k = 0; k < kCensusC; ++k) {
    int i = base[k] + ((e[base[k]] <= x[k]) ? 1 : 0) - 1;  // (a NaN compares false: -1)
    i = (closed && i == n && x[k] == last) ? n - 1 : i;
    bin[k] = (i >= 0 && i < n) ? i : -1;
  }
}

struct CensusArgs {
  const void* f0;
  const void* f1;
  const double* e0;
  const double* e1;
  const void* w;
  const void* val;
  int64_t* partials;
  int64_t nrec, ncells, ntiles, nblocks;
  int n0, n1, nbins, closed, w_per_record;
};

template <typename T>
__device__ __forceinline__ const T* census_rec(const void* p, int64_t rec, int64_t ncells) {
  return static_cast<const T*>(p) + rec * ncells;
}

template <typename F0, typename F1, typename W, typename V>
__global__ __launch_bounds__(kCensusBlock) void k_census_partial(const CensusArgs g) {
  constexpr bool D2 = !__is_same(F1, CNone), HW = !__is_same(W, CNone), HV = !__is_same(V, CNone);
  constexpr int K = 1 + (HW ? 1 : 0) + (HV ? 1 : 0);
  extern __shared__ __attribute__((aligned(16))) char census_smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nbins = g.nbins, n0 = g.n0, n1 = g.n1;
  // LDS: edges0 (n0 + 1), edges1 (n1 + 1, D = 2), then [wave][bin] of wsum, of vsum, of count
  double* e0 = reinterpret_cast<double*>(census_smem);
  double* e1 = e0 + (n0 + 1);
  double* hw = e1 + (D2 ? n1 + 1 : 0);
  double* hv = hw + (HW ? kCensusWaves * nbins : 0);
  unsigned* hc = reinterpret_cast<unsigned*>(hv + (HV ? kCensusWaves * nbins : 0));
  for (int i = tid; i <= n0; i += kCensusBlock) e0[i] = g.e0[i];
  if constexpr (D2) {
    for (int i = tid; i <= n1; i += kCensusBlock) e1[i] = g.e1[i];
  }
  for (int i = tid; i < kCensusWaves * nbins; i += kCensusBlock) {
    hc[i] = 0u;
    if constexpr (HW) hw[i] = 0.0;
    if constexpr (HV) hv[i] = 0.0;
  }
  __syncthreads();
  double* myw = hw + wave * nbins;
  double* myv = hv + wave * nbins;
  unsigned* myc = hc + wave * nbins;

  const int64_t rec = blockIdx.x / g.nblocks, blk = blockIdx.x % g.nblocks;
  const F0* f0 = census_rec<F0>(g.f0, rec, g.ncells);
  const F1* f1 = census_rec<F1>(g.f1, D2 ? rec : 0, g.ncells);
  const W* w = census_rec<W>(g.w, (HW && g.w_per_record) ? rec : 0, g.ncells);
  const V* val = census_rec<V>(g.val, HV ? rec : 0, g.ncells);
  const bool closed0 = g.closed & 1, closed1 = g.closed & 2;

  CCells<F0> a0, b0 = {};
  CCells<F1> a1, b1 = {};
  CCells<W> aw, bw = {};
  CCells<V> av, bv = {};
  int64_t tile = blk;  // (blk < ntiles: blocks <= tiles)
  {
    const int64_t base = tile * kCensusTile, left = g.ncells - base;
    const bool whole = left >= kCensusTile;
    census_load<F0, true>(f0, base, left, whole, a0);
    census_load<F1, true>(f1, base, left, whole, a1);
    census_load<W, false>(w, base, left, whole, aw);
    census_load<V, true>(val, base, left, whole, av);
  }
  for (; tile < g.ntiles; tile += g.nblocks) {
    const int64_t left = g.ncells - tile * kCensusTile;
    if (tile + g.nblocks < g.ntiles) {
      const int64_t nbase = (tile + g.nblocks) * kCensusTile, nleft = g.ncells - nbase;
      const bool nwhole = nleft >= kCensusTile;
      census_load<F0, true>(f0, nbase, nleft, nwhole, b0);
      census_load<F1, true>(f1, nbase, nleft, nwhole, b1);
      census_load<W, false>(w, nbase, nleft, nwhole, bw);
      census_load<V, true>(val, nbase, nleft, nwhole, bv);
    }
    // the bins of the thread's four cells first (the searches overlap), then the leader loops
    int bins[kCensusC];
    {
      double x[kCensusC];
#pragma unroll
      for (int k = 0; k < kCensusC; ++k) x[k] = (double)a0.v[k];  // float -> double: exact
      census_bins(e0, n0, closed0, x, bins);
      if constexpr (D2) {
        int i1[kCensusC];
#pragma unroll
        for (int k = 0; k < kCensusC; ++k) x[k] = (double)a1.v[k];
        census_bins(e1, n1, closed1, x, i1);
#pragma unroll
        for (int k = 0; k < kCensusC; ++k)
          bins[k] = (bins[k] >= 0 && i1[k] >= 0) ? bins[k] * n1 + i1[k] : -1;
      }
    }
#pragma unroll
    for (int k = 0; k < kCensusC; ++k) {
      bool in = (int64_t)tid * kCensusC + k < left;
      int bin = bins[k];
      double wk = 0.0, pk = 0.0;
      if constexpr (HW) {
        wk = (double)aw.v[k];
        in = in && !census_isnan(wk);
      }
      if constexpr (HV) {
        const double vk = (double)av.v[k];
        in = in && !census_isnan(vk);
        pk = wk * vk;  // rounded once
      }
      // the address test: whatever the edges hold, 0 <= bin < nbins or the lane is no member
      bin = (in && bin >= 0 && bin < nbins) ? bin : -1;
      uint64_t remaining = __ballot(bin >= 0);
      while (remaining != 0) {  // (wave-uniform: a ballot)
        const int leader = __builtin_ctzll(remaining);              // scalar
        const int lb = __builtin_amdgcn_readlane(bin, leader);      // scalar: the leader's bin, >= 0
        const bool member = bin == lb;
        const uint64_t mask = __ballot(member);
        double sw = member ? wk : 0.0, sv = member ? pk : 0.0;
        if constexpr (HW) {
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) sw += __shfl_down(sw, off, 64);
        }
        if constexpr (HV) {
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) sv += __shfl_down(sv, off, 64);
        }
        if (lane == 0) {  // lb is in range (tested above): one lane, one bin of the wave's own table
          myc[lb] += (unsigned)__builtin_popcountll(mask);
          if constexpr (HW) myw[lb] += sw;
          if constexpr (HV) myv[lb] += sv;
        }
        bin = member ? -1 : bin;
        remaining &= ~mask;
      }
    }
    a0 = b0, a1 = b1, aw = bw, av = bv;
  }
  __syncthreads();
  int64_t* out = g.partials + (rec * g.nblocks + blk) * (int64_t)K * nbins;
  for (int b = tid; b < nbins; b += kCensusBlock) {
    unsigned c = hc[b];
#pragma unroll
    for (int q = 1; q < kCensusWaves; ++q) c += hc[q * nbins + b];
    out[b] = (int64_t)c;
    if constexpr (HW) {
      double s = hw[b];
#pragma unroll
      for (int q = 1; q < kCensusWaves; ++q) s += hw[q * nbins + b];
      out[nbins + b] = __double_as_longlong(s);
    }
    if constexpr (HV) {
      double s = hv[b];
#pragma unroll
      for (int q = 1; q < kCensusWaves; ++q) s += hv[q * nbins + b];
      out[2 * nbins + b] = __double_as_longlong(s);
    }
  }
}

// one thread per (record, bin): the partials in ascending block order
__global__ __launch_bounds__(kCensusBlock) void k_census_finish(const int64_t* __restrict__ partials,
                                                                int64_t nrec, int64_t nblocks,
                                                                int nbins, int K,
                                                                int64_t* __restrict__ count,
                                                                double* __restrict__ wsum,
                                                                double* __restrict__ vsum) {
  const int64_t i = (int64_t)blockIdx.x * kCensusBlock + threadIdx.x;
  if (i >= nrec * nbins) return;
  const int64_t rec = i / nbins, b = i % nbins;
  const int64_t* p = partials + rec * nblocks * K * nbins + b;
  int64_t c = 0;
  double sw = 0.0, sv = 0.0;
  for (int64_t blk = 0; blk < nblocks; ++blk, p += (int64_t)K * nbins) {
    c += p[0];
    if (K > 1) sw += __longlong_as_double(p[nbins]);
    if (K > 2) sv += __longlong_as_double(p[2 * (int64_t)nbins]);
  }
  count[i] = c;
  if (K > 1) wsum[i] = sw;
  if (K > 2) vsum[i] = sv;
}

inline int64_t census_blocks_of(int64_t ncells) {
  if (ncells <= 0 || ncells > kCensusMaxCells) return 0;
  const int64_t per = ceil_div(ceil_div(ncells, kCensusTile), kCensusTilesPerBlock);
  return per < kCensusMaxBlocks ? per : kCensusMaxBlocks;
}

inline int64_t census_bin_bytes(bool hw, bool hv) { return 4 + (hw ? 8 : 0) + (hv ? 8 : 0); }

inline int64_t census_max_bins_of(int D, bool hw, bool hv) {
  if ((D != 1 && D != 2) || (hv && !hw)) return 0;
  // edges: at most nbins + 1 (D = 1) or n0 + n1 + 2 <= nbins + 3 (D = 2) doubles
  return (kCensusLds - 8 * (D == 1 ? 1 : 3)) / (8 + kCensusWaves * census_bin_bytes(hw, hv));
}

inline bool census_sizes_ok(int64_t nrec, int64_t ncells) {
  if (nrec < 0 || ncells < 0 || ncells > kCensusMaxCells) return false;
  if (ncells > 0 && nrec > kCensusMaxElems / ncells) return false;
  if (ncells > 0 && nrec > kCensusMaxGrid / census_blocks_of(ncells)) return false;
  return true;
}

template <typename F0, typename F1, typename W, typename V>
void census_launch(const CensusArgs& g, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL((k_census_partial<F0, F1, W, V>), dim3((unsigned)(g.nrec * g.nblocks)),
                     dim3(kCensusBlock), lds, st, g);
}

// dtype codes of the dispatch: MLX_DTYPE_F64, MLX_DTYPE_F32, kCensusAbsent
constexpr int kCensusAbsent = -1;

template <typename F0, typename F1, typename W>
void census_pick_v(int vdt, const CensusArgs& g, size_t lds, hipStream_t st) {
  if constexpr (__is_same(W, CNone)) {
    census_launch<F0, F1, CNone, CNone>(g, lds, st);
  } else {
    if (vdt == MLX_DTYPE_F64) census_launch<F0, F1, W, double>(g, lds, st);
    else if (vdt == MLX_DTYPE_F32) census_launch<F0, F1, W, float>(g, lds, st);
    else census_launch<F0, F1, W, CNone>(g, lds, st);
  }
}

template <typename F0, typename F1>
void census_pick_w(int wdt, int vdt, const CensusArgs& g, size_t lds, hipStream_t st) {
  if (wdt == MLX_DTYPE_F64) census_pick_v<F0, F1, double>(vdt, g, lds, st);
  else if (wdt == MLX_DTYPE_F32) census_pick_v<F0, F1, float>(vdt, g, lds, st);
  else census_pick_v<F0, F1, CNone>(vdt, g, lds, st);
}

template <typename F0>
void census_pick_f1(int f1dt, int wdt, int vdt, const CensusArgs& g, size_t lds, hipStream_t st) {
  if (f1dt == MLX_DTYPE_F64) census_pick_w<F0, double>(wdt, vdt, g, lds, st);
  else if (f1dt == MLX_DTYPE_F32) census_pick_w<F0, float>(wdt, vdt, g, lds, st);
  else census_pick_w<F0, CNone>(wdt, vdt, g, lds, st);
}

}  // namespace
}  // namespace mlx

extern "C" int64_t mlx_census_tile(void) { return mlx::kCensusTile; }

extern "C" int64_t mlx_census_blocks(int64_t ncells) { return mlx::census_blocks_of(ncells); }

extern "C" int64_t mlx_census_max_bins(int D, int has_weights, int has_values) {
  return mlx::census_max_bins_of(D, has_weights != 0, has_values != 0);
}

extern "C" size_t mlx_census_workspace_bytes(int64_t nrec, int64_t ncells, int64_t nbins,
                                             int has_weights, int has_values) {
  using namespace mlx;
  if (has_values && !has_weights) return 0;
  if (!census_sizes_ok(nrec, ncells) || nbins < 1 ||
      nbins > census_max_bins_of(1, has_weights != 0, has_values != 0))
    return 0;
  const size_t K = 1 + (has_weights ? 1 : 0) + (has_values ? 1 : 0);
  return (size_t)nrec * (size_t)census_blocks_of(ncells) * (size_t)nbins * K * 8;
}

extern "C" int mlx_census_histogram(const void* f0, int f0_dtype, const void* f1, int f1_dtype,
                                    int D, const double* edges0, int64_t n0, const double* edges1,
                                    int64_t n1, int closed, const void* w, int w_dtype,
                                    int w_per_record, const void* val, int val_dtype, int64_t nrec,
                                    int64_t ncells, int64_t* count, double* wsum, double* vsum,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  using namespace mlx;
  using detail::fail;
  using detail::hip_status;
  if (D != 1 && D != 2) return fail(MLX_E_SHAPE, "D must be 1 or 2: one or two binning fields");
  const bool hw = w != nullptr, hv = val != nullptr;
  if (!is_float_dtype(f0_dtype) || (D == 2 && !is_float_dtype(f1_dtype)) ||
      (hw && !is_float_dtype(w_dtype)) || (hv && !is_float_dtype(val_dtype)))
    return fail(MLX_E_ENUM, "f0_dtype, f1_dtype, w_dtype and val_dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  if (closed < 0 || closed > 3) return fail(MLX_E_ENUM, "closed must be 0 .. 3");
  if (hv && !hw) return fail(MLX_E_SHAPE, "val needs w: a sum of w * val");
  if (n0 < 1 || n1 < 1 || (D == 1 && n1 != 1))
    return fail(MLX_E_SHAPE, "need n0 >= 1 and n1 >= 1 (n1 == 1 when D == 1)");
  const int64_t cap = census_max_bins_of(D, hw, hv);
  if (n0 > cap || n1 > cap || n0 * n1 > cap)
    return fail(MLX_E_SHAPE, "nbins = n0 * n1 is over mlx_census_max_bins: launch in bin groups");
  if (nrec < 0 || ncells < 0) return fail(MLX_E_SHAPE, "nrec and ncells must not be negative");
  if (!census_sizes_ok(nrec, ncells))
    return fail(MLX_E_SHAPE, "need ncells <= 2^38, nrec * ncells <= 2^40 and nrec * blocks < 2^31");
  if (nrec == 0 || ncells == 0) return 0;
  if (!f0 || (D == 2 && !f1) || !edges0 || (D == 2 && !edges1) || !count || (hw && !wsum) ||
      (hv && !vsum) || !workspace)
    return fail(MLX_E_NULL, "f0, f1, edges0, edges1, count, wsum, vsum and workspace must not be NULL");
  if (!aligned(f0, dtype_size(f0_dtype)) || (D == 2 && !aligned(f1, dtype_size(f1_dtype))) ||
      (hw && !aligned(w, dtype_size(w_dtype))) || (hv && !aligned(val, dtype_size(val_dtype))))
    return fail(MLX_E_ALIGN, "f0 / f1 / w / val not aligned to their element");
  if (!aligned(edges0, 8) || (D == 2 && !aligned(edges1, 8)) || !aligned(count, 8) ||
      (hw && !aligned(wsum, 8)) || (hv && !aligned(vsum, 8)))
    return fail(MLX_E_ALIGN, "edges0 / edges1 / count / wsum / vsum not 8-byte aligned");
  const int64_t nbins = n0 * n1;
  const size_t need = mlx_census_workspace_bytes(nrec, ncells, nbins, hw, hv);
  if (workspace_bytes < need || !aligned(workspace, 8))
    return fail(MLX_E_WORKSPACE, "workspace too small (mlx_census_workspace_bytes) or not 8-byte aligned");

  CensusArgs g;
  g.f0 = f0, g.f1 = D == 2 ? f1 : nullptr, g.e0 = edges0, g.e1 = D == 2 ? edges1 : nullptr;
  g.w = w, g.val = val, g.partials = static_cast<int64_t*>(workspace);
  g.nrec = nrec, g.ncells = ncells, g.ntiles = ceil_div(ncells, kCensusTile);
  g.nblocks = census_blocks_of(ncells);
  g.n0 = (int)n0, g.n1 = (int)n1, g.nbins = (int)nbins, g.closed = closed;
  g.w_per_record = w_per_record != 0;
  const size_t lds = 8 * (size_t)(n0 + 1 + (D == 2 ? n1 + 1 : 0)) +
                     (size_t)kCensusWaves * (size_t)nbins * (size_t)census_bin_bytes(hw, hv);
  const int f1dt = D == 2 ? f1_dtype : kCensusAbsent;
  const int wdt = hw ? w_dtype : kCensusAbsent, vdt = hv ? val_dtype : kCensusAbsent;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (f0_dtype == MLX_DTYPE_F64) census_pick_f1<double>(f1dt, wdt, vdt, g, lds, st);
  else census_pick_f1<float>(f1dt, wdt, vdt, g, lds, st);
  if (int rc = hip_status(hipGetLastError(), "k_census_partial launch")) return rc;
  const int K = 1 + (hw ? 1 : 0) + (hv ? 1 : 0);
  hipLaunchKernelGGL(k_census_finish, dim3((unsigned)ceil_div(nrec * nbins, kCensusBlock)),
                     dim3(kCensusBlock), 0, st, (const int64_t*)g.partials, nrec, g.nblocks,
                     (int)nbins, K, count, wsum, vsum);
  return hip_status(hipGetLastError(), "k_census_finish launch");
}
