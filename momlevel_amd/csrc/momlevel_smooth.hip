// momlevel_smooth.hip -- mlx_smooth_apply (include/momlevel_smooth.h): a separable, normalised,
// mask-aware, area-weighted convolution over the (y, x) plane of a (nrec, ny, nx) record.  An
// EXTENSION (momlevel has no such function); the specification is tests/smooth_numpy.py.
//
// TILED PATH, k_smooth_tiled: wave64, 256-thread blocks, one block per (tile of kSmTH x kSmTW
// output cells, window of kSmRecWin records).  Before its first record the block puts into LDS what
// does not depend on the record: the masked area (0.0 = carries no weight) of the tile and its
// halo, kSmTH + Wy - 1 rows by kSmTW + Wx - 1 columns widened to whole 16-byte packs, the x weights
// of those rows and the y weights -- the 2-D maps are read once per window of records.  Per record:
//   ROW PASS.  Wave q takes the halo rows q, q + 4, ...: lane p loads one 16-byte pack of each of
//     them (a chunk of up to six rows at once, the next chunk's -- of this record or the next --
//     before this one's are summed: one pack at a time left the kernel waiting on memory), writes (m, a) =
//     (a64 * v64, a64), or (0, 0) where the cell is not valid, for its cells into the wave's staging
//     row S[q][.] and the centre values into Vc; then lane i sums output column i of that row over
//     k ascending -- one 16-byte LDS read per tap at a 16-byte lane stride, the whole wave on one
//     row: conflict-free, the weight a broadcast -- and writes Rn, Rd, Rc[row][i].
//   COLUMN PASS.  A thread owns one 16-byte pack of output cells of a row (two rows for float64
//     results): it adds wy[l] * Rn, Rd[row + l][pack] and Rc over l ascending from LDS, a wave's
//     lanes on adjacent 16 or 32 bytes of a row, divides, applies the rule for min_count, FILL and
//     RESIDUAL and stores the pack (nt).
// A cell of v comes from memory once per tile that needs it: the tile and its halo.  No global
// temporary.  LDS is static, in three window classes (kSmClass*): its size, not the registers, sets
// the blocks per CU.
//
// GENERIC PATH, k_smooth_cells: one thread per output cell and record, the same sums in the same
// order from global memory.  Windows above kSmMaxWindow, an nx that is no multiple of 4, pointers
// that are not 16-byte aligned, planes smaller than a tile.
//
// Rn[r, i] is a function of (rec, r, i) only, so the halo rows two tiles both sum have the same
// bits, and both paths form every product and every add alone (-ffp-contract=off and the pragma
// below): a cell's bits depend on neither the path nor the tiling.  No atomics, no running sums.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/momlevel_hip.h"
#include "../../include/momlevel_smooth.h"
#include "mlx_internal.hpp"
#include "mlx_pack.hpp"

#pragma clang fp contract(off)

namespace mlx {
namespace {

constexpr int kSmBlock = 256;  // 4 waves of 64
constexpr int kSmTH = 16;      // output rows of a tile
constexpr int kSmTW = 64;      // output columns of a tile: one per lane of the row pass
constexpr int kSmAlign = 4;    // cells the staged columns start on a multiple of (16 bytes of float32)
constexpr int kSmMaxWindow = 33;
constexpr int kSmRecWin = 8;
constexpr int kSmMaxGridY = 65535;
constexpr int64_t kSmMaxCells = (int64_t)1 << 38;
// the window classes of the tiled kernel: static LDS of 49.6, 58.8 and 124.4 KiB -- 3, 2 and 1 blocks per CU
constexpr int kSmClassS = 5, kSmClassM = 9, kSmClassL = kSmMaxWindow;

__device__ __forceinline__ bool sm_isnan(double x) { return x != x; }
__device__ __forceinline__ double sm_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

constexpr int sm_staged_cols(int W) {  // kSmTW + W - 1 columns from a start rounded down to a pack
  return (kSmTW + W - 1 + (kSmAlign - 1) + (kSmAlign - 1)) / kSmAlign * kSmAlign;
}

// the rule of the header for one output cell; centre: v64 where the centre is valid, else NaN
__device__ __forceinline__ double sm_finish(double num, double den, int64_t cnt, double centre,
                                            int64_t min_count, int flags) {
  const double smooth = num / den;
  const bool cvalid = !sm_isnan(centre);
  double r;
  if (cnt < min_count || (!cvalid && !(flags & MLX_SMOOTH_FILL))) r = sm_nan();
  else if (flags & MLX_SMOOTH_RESIDUAL) r = centre - smooth;
  else r = smooth;
  return sm_isnan(r) ? sm_nan() : r;
}

template <typename TO>
__device__ __forceinline__ TO sm_narrow(double r) {
  if constexpr (sizeof(TO) == 8) return r;
  else return sm_isnan(r) ? __int_as_float(0x7fc00000) : (float)r;  // rounded once
}

struct SmoothArgs {
  const void* v;
  const void* area;
  const double* wx;
  const double* wy;
  void* out;
  int64_t nrec, ny, nx, min_count;
  int Wx, Wy, lead_x, lead_y;
  int table, periodic, flags;
  int64_t tiles_x, tiles_y;
};

template <typename TV, typename TA, typename TO, int MAXW>
__global__ __launch_bounds__(kSmBlock) void k_smooth_tiled(const SmoothArgs g) {
  constexpr int NR = kSmTH + MAXW - 1;     // halo rows at most
  constexpr int SCM = sm_staged_cols(MAXW);  // staged columns at most
  constexpr int P = 16 / (int)sizeof(TV);  // cells of a load
  constexpr int PO = 16 / (int)sizeof(TO);  // cells of a store
  __shared__ __attribute__((aligned(16))) double sA[NR * SCM];       // masked area, 0.0 = no weight
  __shared__ __attribute__((aligned(16))) double sRn[NR * kSmTW];
  __shared__ __attribute__((aligned(16))) double sRd[NR * kSmTW];
  __shared__ __attribute__((aligned(16))) int sRc[NR * kSmTW];
  __shared__ __attribute__((aligned(16))) double2 sS[(kSmBlock / 64) * SCM];  // (m, a) of a wave's row
  __shared__ __attribute__((aligned(16))) double sVc[kSmTH * kSmTW];  // centre v64, NaN = not valid
  __shared__ __attribute__((aligned(16))) double sWx[NR * MAXW];
  __shared__ __attribute__((aligned(16))) double sWy[MAXW];

  const TV* __restrict__ v = static_cast<const TV*>(g.v);
  const TA* __restrict__ area = static_cast<const TA*>(g.area);
  TO* __restrict__ out = static_cast<TO*>(g.out);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int Wx = g.Wx, Wy = g.Wy;
  const int nrows = kSmTH + Wy - 1;            // <= NR
  const int sc = sm_staged_cols(Wx);           // <= SCM
  const int64_t ny = g.ny, nx = g.nx;
  const int64_t ntiles = g.tiles_x * g.tiles_y;
  const int64_t tile = blockIdx.x % ntiles, win = blockIdx.x / ntiles;
  const int64_t j0 = (tile / g.tiles_x) * kSmTH, c0 = (tile % g.tiles_x) * kSmTW;
  const int64_t r0 = win * kSmRecWin, r1 = r0 + kSmRecWin < g.nrec ? r0 + kSmRecWin : g.nrec;
  // the first staged column: c0 - lead_x rounded down to a multiple of kSmAlign (c0 is one)
  const int back = (g.lead_x + kSmAlign - 1) / kSmAlign * kSmAlign;
  const int64_t s0 = c0 - back;
  const int off = back;  // staged index of tile column 0: output column i reads s[i + off - lead_x + k]
  const int shift = off - g.lead_x;  // 0 .. kSmAlign - 1

  // the global column of staged column q, -1: outside the plane (closed x edges)
  auto column_of = [&](int q) -> int64_t {
    int64_t c = s0 + q;
    if (g.periodic) {
      c %= nx;
      return c < 0 ? c + nx : c;
    }
    return (c < 0 || c >= nx) ? -1 : c;
  };

  // ---- what does not depend on the record: masked area, weights
  for (int e = tid; e < nrows * sc; e += kSmBlock) {
    const int rr = e / sc, q = e - rr * sc;
    const int64_t gr = j0 - g.lead_y + rr, gc = column_of(q);
    double a = 0.0;
    if (gr >= 0 && gr < ny && gc >= 0) {
      a = (double)area[gr * nx + gc];  // float -> double: exact
      a = a > 0.0 ? a : 0.0;           // (NaN compares false)
    }
    sA[rr * sc + q] = a;
  }
  for (int e = tid; e < (g.table ? nrows * Wx : Wx); e += kSmBlock) {
    const int rr = e / Wx, k = e - rr * Wx;
    const int64_t gr = j0 - g.lead_y + rr;
    sWx[e] = g.table ? ((gr >= 0 && gr < ny) ? g.wx[gr * Wx + k] : 0.0) : g.wx[k];
  }
  for (int e = tid; e < Wy; e += kSmBlock) sWy[e] = g.wy[e];

  // this lane's pack of a staged row: columns q0 .. q0 + P - 1 (a pack never straddles the seam or
  // an edge: nx, s0 and q0 are multiples of P)
  const int q0 = lane * P;
  const bool stager = q0 < sc;
  const int64_t gc0 = stager ? column_of(q0) : -1;
  const int niter = (nrows + kSmBlock / 64 - 1) / (kSmBlock / 64);
  double2* __restrict__ srow = sS + wave * SCM;

  auto load_row = [&](int64_t rec, int it, TV (&x)[P]) {
    const int rr = it * (kSmBlock / 64) + wave;
    const int64_t gr = j0 - g.lead_y + rr;
    if (stager && gc0 >= 0 && rr < nrows && gr >= 0 && gr < ny) {
      const Pack<TV, P> r = load_pack<TV, P, false>(v + (rec * ny + gr) * nx + gc0);
#pragma unroll
      for (int k = 0; k < P; ++k) x[k] = r.v[k];
    } else {
#pragma unroll
      for (int k = 0; k < P; ++k) x[k] = (TV)0;  // (its area is 0.0: not valid)
    }
  };

  // a wave's rows go in chunks of CH, a chunk's loads in flight together and the next chunk's (of
  // this record or the next) issued before this one's rows are summed
  constexpr int IT = (NR + kSmBlock / 64 - 1) / (kSmBlock / 64);
  constexpr int CH = IT <= 6 ? IT : 4;
  const int nchunk = (niter + CH - 1) / CH;
  const int64_t nseq = (r1 - r0) * nchunk;
  auto load_chunk = [&](int64_t seq, TV (&x)[CH][P]) {
    const int64_t rec = r0 + seq / nchunk;
    const int ch = (int)(seq % nchunk);
#pragma unroll
    for (int u = 0; u < CH; ++u) load_row(rec, ch * CH + u, x[u]);
  };

  __syncthreads();
  TV cur[CH][P], nxt[CH][P] = {};
  load_chunk(0, cur);
  for (int64_t rec = r0; rec < r1; ++rec) {
    // ---- row pass
    for (int ch = 0; ch < nchunk; ++ch) {
      const int64_t seq = (rec - r0) * nchunk + ch;
      if (seq + 1 < nseq) load_chunk(seq + 1, nxt);
#pragma unroll
      for (int u = 0; u < CH; ++u) {
        const int it = ch * CH + u;
        if (it >= niter) break;  // (block-uniform)
        const int rr = it * (kSmBlock / 64) + wave;
        const bool row = rr < nrows;
        if (stager && row) {
#pragma unroll
          for (int k = 0; k < P; ++k) {
            const int q = q0 + k;
            const double x = (double)cur[u][k], a = sA[rr * sc + q];
            const bool valid = a > 0.0 && !sm_isnan(x);
            srow[q] = valid ? make_double2(a * x, a) : make_double2(0.0, 0.0);
            const int tc = q - off, tr = rr - g.lead_y;
            if (tc >= 0 && tc < kSmTW && tr >= 0 && tr < kSmTH) sVc[tr * kSmTW + tc] = valid ? x : sm_nan();
          }
        }
        __syncthreads();  // (a wave reads only the row it staged)
        if (row) {
          const double* __restrict__ X = sWx + (g.table ? rr * Wx : 0);
          const double2* __restrict__ s = srow + lane + shift;
          double rn = 0.0, rd = 0.0;
          int rc = 0;
#pragma unroll 8
          for (int k = 0; k < Wx; ++k) {
            const double2 c = s[k];
            const bool valid = c.y > 0.0;
            const double w = X[k];
            const double tn = w * c.x, td = w * c.y;
            rn += valid ? tn : 0.0;
            rd += valid ? td : 0.0;
            rc += valid;
          }
          sRn[rr * kSmTW + lane] = rn;
          sRd[rr * kSmTW + lane] = rd;
          sRc[rr * kSmTW + lane] = rc;
        }
        // (the wave's next staging store follows its own reads in program order)
      }
#pragma unroll
      for (int u = 0; u < CH; ++u) {
#pragma unroll
        for (int k = 0; k < P; ++k) cur[u][k] = nxt[u][k];
      }
    }
    __syncthreads();

    // ---- column pass
    constexpr int NP = kSmTW / PO;          // packs of a tile row
    constexpr int RPP = kSmBlock / NP;      // tile rows of one pass over the block
#pragma unroll
    for (int pass = 0; pass < kSmTH / RPP; ++pass) {
      const int tr = pass * RPP + tid / NP, pc = (tid % NP) * PO;
      const int64_t j = j0 + tr, i = c0 + pc;
      if (j < ny && i < nx) {  // (a pack is inside the plane or outside it: nx is a multiple of 4)
        const int64_t lo = g.lead_y - j, hi = ny + g.lead_y - j;
        const int l0 = lo > 0 ? (int)lo : 0, l1 = hi < Wy ? (int)hi : Wy;
        double num[PO], den[PO];
        int cnt[PO];
#pragma unroll
        for (int e = 0; e < PO; ++e) num[e] = den[e] = 0.0, cnt[e] = 0;
        for (int l = l0; l < l1; ++l) {
          const double w = sWy[l];
          const int at = (tr + l) * kSmTW + pc;
#pragma unroll
          for (int e = 0; e < PO; ++e) {
            const double tn = w * sRn[at + e], td = w * sRd[at + e];
            num[e] += tn;
            den[e] += td;
            cnt[e] += sRc[at + e];
          }
        }
        Pack<TO, PO> r;
#pragma unroll
        for (int e = 0; e < PO; ++e)
          r.v[e] = sm_narrow<TO>(sm_finish(num[e], den[e], cnt[e], sVc[tr * kSmTW + pc + e],
                                           g.min_count, g.flags));
        store_pack<TO, PO, true>(out + (rec * ny + j) * nx + i, r);
      }
    }
    __syncthreads();  // (the next record's row pass writes what this column pass reads)
  }
}

// one thread per output cell of the plane, the records along gridDim.y
template <typename TV, typename TA, typename TO>
__global__ __launch_bounds__(kSmBlock) void k_smooth_cells(const SmoothArgs g) {
  const TV* __restrict__ v = static_cast<const TV*>(g.v);
  const TA* __restrict__ area = static_cast<const TA*>(g.area);
  TO* __restrict__ out = static_cast<TO*>(g.out);
  const int64_t ny = g.ny, nx = g.nx, plane = ny * nx;
  const int64_t cell = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
  if (cell >= plane) return;
  const int64_t j = cell / nx, i = cell - j * nx;
  const int Wx = g.Wx, Wy = g.Wy;
  const double ac = (double)area[cell];
  for (int64_t rec = blockIdx.y; rec < g.nrec; rec += gridDim.y) {
    const TV* __restrict__ p = v + rec * plane;
    double num = 0.0, den = 0.0;
    int64_t cnt = 0;
    for (int l = 0; l < Wy; ++l) {
      const int64_t r = j - g.lead_y + l;
      if (r < 0 || r >= ny) continue;
      const double* __restrict__ X = g.wx + (g.table ? r * Wx : 0);
      double rn = 0.0, rd = 0.0;
      int rc = 0;
      for (int k = 0; k < Wx; ++k) {
        int64_t c = i - g.lead_x + k;
        if (g.periodic) c = c < 0 ? c + nx : (c >= nx ? c - nx : c);  // (Wx <= nx: one lap at most)
        else if (c < 0 || c >= nx) continue;
        const double a = (double)area[r * nx + c], x = (double)p[r * nx + c];
        const bool valid = !sm_isnan(x) && !sm_isnan(a) && a > 0.0;
        const double m = a * x;
        const double w = X[k];
        const double tn = w * m, td = w * a;
        rn += valid ? tn : 0.0;
        rd += valid ? td : 0.0;
        rc += valid;
      }
      const double w = g.wy[l];
      const double tn = w * rn, td = w * rd;
      num += tn;
      den += td;
      cnt += rc;
    }
    const double xc = (double)p[cell];
    const bool cvalid = !sm_isnan(xc) && !sm_isnan(ac) && ac > 0.0;
    out[rec * plane + cell] = sm_narrow<TO>(sm_finish(num, den, cnt, cvalid ? xc : sm_nan(),
                                                      g.min_count, g.flags));
  }
}

// gridDim.y of k_smooth_cells over nrec > 0 records: one block row per record up to the cap, past
// which the rows stride.  The one rule: mlx_smooth_record_rows reports it, the launch uses it.
inline int64_t smooth_record_rows(int64_t nrec) {
  return nrec < (int64_t)kSmMaxGridY ? nrec : (int64_t)kSmMaxGridY;
}

// the shape part of the choice of path, for extents mlx_smooth_apply accepts: windows the LDS of a
// class holds, rows of whole packs, a plane of at least one tile each way.  The one rule:
// mlx_smooth_tiled reports it, mlx_smooth_apply goes by it (and by the alignment of v and out).
inline bool smooth_tiled_shape(int64_t Wx, int64_t Wy, int64_t ny, int64_t nx) {
  return Wx <= kSmMaxWindow && Wy <= kSmMaxWindow && nx % kSmAlign == 0 && ny >= kSmTH && nx >= kSmTW;
}

template <typename TV, typename TA, typename TO>
void smooth_launch(const SmoothArgs& g, bool tiled, hipStream_t st) {
  if (tiled) {
    const int64_t nwin = ceil_div(g.nrec, kSmRecWin);
    const dim3 grid((unsigned)(g.tiles_x * g.tiles_y * nwin)), block(kSmBlock);
    const int W = g.Wx > g.Wy ? g.Wx : g.Wy;
    if (W <= kSmClassS)
      hipLaunchKernelGGL((k_smooth_tiled<TV, TA, TO, kSmClassS>), grid, block, 0, st, g);
    else if (W <= kSmClassM)
      hipLaunchKernelGGL((k_smooth_tiled<TV, TA, TO, kSmClassM>), grid, block, 0, st, g);
    else
      hipLaunchKernelGGL((k_smooth_tiled<TV, TA, TO, kSmClassL>), grid, block, 0, st, g);
  } else {
    const dim3 grid((unsigned)ceil_div(g.ny * g.nx, kSmBlock), (unsigned)smooth_record_rows(g.nrec)),
        block(kSmBlock);
    hipLaunchKernelGGL((k_smooth_cells<TV, TA, TO>), grid, block, 0, st, g);
  }
}

template <typename TV, typename TA>
void smooth_launch_out(const SmoothArgs& g, int out_dtype, bool tiled, hipStream_t st) {
  if (out_dtype == MLX_DTYPE_F64) smooth_launch<TV, TA, double>(g, tiled, st);
  else smooth_launch<TV, TA, float>(g, tiled, st);
}

inline bool sm_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}

}  // namespace
}  // namespace mlx

extern "C" int64_t mlx_smooth_tile_h(void) { return mlx::kSmTH; }

extern "C" int64_t mlx_smooth_tile_w(int dtype) { return mlx::is_float_dtype(dtype) ? mlx::kSmTW : 0; }

extern "C" int64_t mlx_smooth_max_window(void) { return mlx::kSmMaxWindow; }

extern "C" int64_t mlx_smooth_record_window(void) { return mlx::kSmRecWin; }

extern "C" int mlx_smooth_record_rows(int64_t nrec) {
  if (nrec <= 0 || nrec > mlx::kSmMaxCells) return 0;
  return (int)mlx::smooth_record_rows(nrec);
}

extern "C" int mlx_smooth_tiled(int64_t Wx, int64_t Wy, int64_t ny, int64_t nx) {
  using namespace mlx;
  if (ny < 1 || nx < 1 || ny > kSmMaxCells / nx || Wx < 1 || Wx > nx || Wy < 1 || Wy > ny) return 0;
  return smooth_tiled_shape(Wx, Wy, ny, nx) ? 1 : 0;
}

extern "C" int mlx_smooth_apply(const void* v, int dtype, const void* area, int area_dtype,
                                const double* wx, int64_t Wx, int64_t wx_stride, int64_t lead_x,
                                const double* wy, int64_t Wy, int64_t lead_y, int periodic_x,
                                int64_t min_count, int flags, int64_t nrec, int64_t ny, int64_t nx,
                                void* out, int out_dtype, void* stream) {
  using namespace mlx;
  using detail::fail;
  using detail::hip_status;
  if (!is_float_dtype(dtype) || !is_float_dtype(area_dtype) || !is_float_dtype(out_dtype))
    return fail(MLX_E_ENUM, "dtype, area_dtype and out_dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  if (flags & ~(MLX_SMOOTH_FILL | MLX_SMOOTH_RESIDUAL))
    return fail(MLX_E_ENUM, "flags: MLX_SMOOTH_FILL and MLX_SMOOTH_RESIDUAL are the only ones");
  if (periodic_x != 0 && periodic_x != 1) return fail(MLX_E_ENUM, "periodic_x must be 0 or 1");
  if (nrec < 0) return fail(MLX_E_SHAPE, "nrec must not be negative");
  if (ny < 1 || nx < 1) return fail(MLX_E_SHAPE, "need ny >= 1 and nx >= 1");
  if (ny > kSmMaxCells / nx || (nrec > 0 && ny * nx > kSmMaxCells / nrec))
    return fail(MLX_E_SHAPE, "need nrec * ny * nx <= 2^38");
  if (Wx < 1 || Wx > nx) return fail(MLX_E_SHAPE, "need 1 <= Wx <= nx (a periodic window may not lap itself)");
  if (Wy < 1 || Wy > ny) return fail(MLX_E_SHAPE, "need 1 <= Wy <= ny");
  if (lead_x < 0 || lead_x >= Wx) return fail(MLX_E_SHAPE, "need 0 <= lead_x < Wx");
  if (lead_y < 0 || lead_y >= Wy) return fail(MLX_E_SHAPE, "need 0 <= lead_y < Wy");
  if (min_count < 1 || min_count > Wx * Wy) return fail(MLX_E_SHAPE, "need 1 <= min_count <= Wx * Wy");
  if (wx_stride != 0 && wx_stride != Wx) return fail(MLX_E_SHAPE, "wx_stride must be 0 or Wx");
  if (nrec == 0) return 0;
  if (!v || !area || !wx || !wy || !out)
    return fail(MLX_E_NULL, "v, area, wx, wy and out must not be NULL");
  if (!aligned(v, dtype_size(dtype)) || !aligned(area, dtype_size(area_dtype)) ||
      !aligned(out, dtype_size(out_dtype)))
    return fail(MLX_E_ALIGN, "v / area / out not aligned to their element");
  if (!aligned(wx, 8) || !aligned(wy, 8)) return fail(MLX_E_ALIGN, "wx / wy not 8-byte aligned");
  const size_t plane = (size_t)ny * (size_t)nx;
  const size_t nout = (size_t)nrec * plane * dtype_size(out_dtype);
  if (sm_overlap(out, nout, v, (size_t)nrec * plane * dtype_size(dtype)) ||
      sm_overlap(out, nout, area, plane * dtype_size(area_dtype)) ||
      sm_overlap(out, nout, wx, (size_t)(wx_stride ? ny * Wx : Wx) * 8) ||
      sm_overlap(out, nout, wy, (size_t)Wy * 8))
    return fail(MLX_E_SHAPE, "out overlaps an operand");

  SmoothArgs g;
  g.v = v, g.area = area, g.wx = wx, g.wy = wy, g.out = out;
  g.nrec = nrec, g.ny = ny, g.nx = nx, g.min_count = min_count;
  g.Wx = (int)Wx, g.Wy = (int)Wy, g.lead_x = (int)lead_x, g.lead_y = (int)lead_y;
  g.table = wx_stride != 0, g.periodic = periodic_x, g.flags = flags;
  g.tiles_x = ceil_div(nx, kSmTW), g.tiles_y = ceil_div(ny, kSmTH);
  // (Wx, Wy beyond int only reach the generic kernel through nx, ny > 2^31: refuse the cast)
  if (Wx > (int64_t)1 << 30 || Wy > (int64_t)1 << 30)
    return fail(MLX_E_SHAPE, "need Wx and Wy <= 2^30");
  const bool tiled = smooth_tiled_shape(Wx, Wy, ny, nx) && aligned(v, 16) && aligned(out, 16);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool v64 = dtype == MLX_DTYPE_F64, a64 = area_dtype == MLX_DTYPE_F64;
  if (v64) {
    if (a64) smooth_launch_out<double, double>(g, out_dtype, tiled, st);
    else smooth_launch_out<double, float>(g, out_dtype, tiled, st);
  } else {
    if (a64) smooth_launch_out<float, double>(g, out_dtype, tiled, st);
    else smooth_launch_out<float, float>(g, out_dtype, tiled, st);
  }
  return hip_status(hipGetLastError(), tiled ? "k_smooth_tiled launch" : "k_smooth_cells launch");
}
