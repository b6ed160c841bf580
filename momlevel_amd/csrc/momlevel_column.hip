// momlevel_column.hip -- mlx_column_crossing (include/momlevel_column.h): the depth of the first
// crossing along z of a (record, z, plane) field, or of the potential density of a (theta, S) pair,
// for up to MLX_COLUMN_MAX_TARGETS targets.  An EXTENSION (momlevel has no such function); the
// specification is tests/column_numpy.py.
//
// k_column_crossing: wave64, 256-thread blocks, grid = (tiles of the plane, block rows of records).
// A thread owns one 16-byte pack of adjacent cells -- 2 when a float64 field takes part (its
// float32 partner then comes as an 8-byte load), 4 when every field is float32 -- and one record at
// a time.  z is the sequential loop; z[k], kref, the mode and the targets are wave-uniform (scalar
// loads, kernel arguments).  The field's loads are streaming (`nt`), the next level's are issued
// before the current one is tested.  No atomics, no LDS, no workspace: a column belongs to one
// thread.
//
// THE EXIT is what no other kernel of the library has: a trip count that depends on the data.  A
// cell whose targets are all decided, or whose column met NaN (land, the sea floor), stops; a lane
// whose cells have all stopped is `fin`: it issues no further loads and skips the level's
// arithmetic, and nothing it holds can change any more.  The WAVE leaves the z loop when a ballot
// over its active lanes shows no lane left that is not `fin` -- a wave-uniform scalar branch.  A lane
// still searching keeps the wave in the loop, so it is never cut short by 63 finished neighbours;
// one prefetched level per lane is the price of issuing loads ahead of the test.
//
// A cell's state: val[j] holds target j's threshold until it is decided and its result after (one
// register pair, not two), one bit per target in `done`, the previous level's value, the depth of
// the last level with a value, x_ref.  NTC is the compile-time capacity (1, 2, 4 or 8 targets) so
// that one target does not pay the registers of eight; nt <= NTC is the launch's count.  A
// target's bits do not depend on it.
//
// SIGMA source: x is the exact float64 density of eos_device.hpp (wright_density<kF64, double,
// ExactOps> / linear_density<kF64>) of the widened operands, for every input dtype: the bits of
// mlx_eos_map on float64 copies (momlevel_column.h says why).
//
// GENERIC twin: one cell per thread, scalar loads and stores, for planes that are not a whole
// number of packs and for a / b / out that are not aligned for their pack accesses.  The same
// arithmetic in the same order: the same bits.
//
// Compile: with momlevel_hip.hip (csrc/build.py), -ffp-contract=off and the pragma below: the
// interpolation is a subtraction, a subtraction, a division, a multiplication and an addition.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/momlevel_hip.h"
#include "../../include/momlevel_column.h"
#include "eos_device.hpp"
#include "mlx_internal.hpp"
#include "mlx_pack.hpp"

#pragma clang fp contract(off)

namespace mlx {
namespace {

constexpr int kColBlock = 256;  // 4 waves of 64
constexpr int64_t kColMaxCells = (int64_t)1 << 38;
constexpr unsigned kColMaxGridY = 65535;

struct ColumnTargets {
  double v[MLX_COLUMN_MAX_TARGETS];
};
struct NoField {};  // the TB of the FIELD source

template <typename TV, int VEC>
__device__ __forceinline__ Pack<TV, VEC> col_load(const TV* __restrict__ p) {
  if constexpr (VEC == 1) {
    Pack<TV, 1> r;
    r.v[0] = __builtin_nontemporal_load(p);
    return r;
  } else {
    return load_pack<TV, VEC, true>(p);
  }
}

// the column value of one cell and level: the field itself, or the density of (theta, S) at p_ref
template <bool SIGMA>
__device__ __forceinline__ double col_value(double t, double s, int eos, double p_ref) {
  if constexpr (!SIGMA) return t;
  else
    return eos == kLinear ? linear_density<kF64, double>(t, s)
                          : wright_density<kF64, double, ExactOps>(t, s, p_ref);
}

template <typename TA, typename TB, int NTC, bool GENERIC>
__global__ __launch_bounds__(kColBlock) void k_column_crossing(
    const TA* __restrict__ a, const void* __restrict__ b_, int eos, double p_ref, int64_t nrec,
    int64_t nz, int64_t plane, const double* __restrict__ z, int64_t kref, int mode, int relative,
    int miss, ColumnTargets tg, int nt, const double* __restrict__ floor,
    double* __restrict__ out) {
  constexpr bool SIGMA = !std::is_same<TB, NoField>::value;
  typedef typename std::conditional<SIGMA, TB, TA>::type TBL;  // (FIELD: never loaded)
  constexpr int WIDE = (SIGMA && sizeof(TBL) > sizeof(TA)) ? (int)sizeof(TBL) : (int)sizeof(TA);
  constexpr int VEC = GENERIC ? 1 : 16 / WIDE;
  const TBL* __restrict__ b = static_cast<const TBL*>(b_);
  const int64_t col = ((int64_t)blockIdx.x * kColBlock + threadIdx.x) * VEC;
  if (col + VEC > plane) return;  // whole packs only (the host picks GENERIC otherwise); no barrier
  const int64_t n3 = nz * plane;
  const unsigned allt = (1u << nt) - 1u;

  for (int64_t r = blockIdx.y; r < nrec; r += gridDim.y) {
    const TA* __restrict__ ar = a + r * n3 + col;
    const TBL* __restrict__ br = SIGMA ? b + r * n3 + col : nullptr;

    double val[NTC][VEC];  // target j's threshold until it is decided, its result after
    double xref[VEC], prev[VEC], zlast[VEC];
    unsigned done[VEC];  // bit j: target j is decided
    bool stop[VEC], wet[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
#pragma unroll
      for (int j = 0; j < NTC; ++j) val[j][c] = canonical_nan();
      xref[c] = prev[c] = 0.0;
      zlast[c] = canonical_nan();
      done[c] = 0;
      stop[c] = false;
      wet[c] = true;
    }

    Pack<TA, VEC> ca = col_load<TA, VEC>(ar), na = ca;
    Pack<TBL, VEC> cb = {}, nb = {};
    if constexpr (SIGMA) {
      cb = col_load<TBL, VEC>(br);
      nb = cb;
    }
    bool fin = false;
    double zprev = 0.0;

    for (int64_t k = 0; k < nz; ++k) {
      if (k + 1 < nz && !fin) {  // the next level's loads fly while this one is tested
        na = col_load<TA, VEC>(ar + (k + 1) * plane);
        if constexpr (SIGMA) nb = col_load<TBL, VEC>(br + (k + 1) * plane);
      }
      const double zk = z[k];
      const double dzk = zk - zprev;  // z[k] - z[k-1]: used from kref + 1 on
      if (!fin) {
        double x[VEC];
#pragma unroll
        for (int c = 0; c < VEC; ++c)  // float -> double: exact
          x[c] = col_value<SIGMA>((double)ca.v[c], SIGMA ? (double)cb.v[c] : 0.0, eos, p_ref);
        bool all_stopped = true;
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
          if (!stop[c]) {
            const double xc = x[c];
            const bool xnan = xc != xc;
            if (xnan && k == 0) {  // 1. land: val is NaN already
              done[c] = allt;
            } else if (k < kref) {  // above the reference level: the deepest level with a value
              if (xnan) wet[c] = false;
              else if (wet[c]) zlast[c] = zk;
            } else if (xnan) {  // 2. shallower than kref, or 5. the sea floor: misses, below
              stop[c] = true;
            } else if (k == kref) {  // 3. the targets, 4. the outcrop
              xref[c] = xc;
#pragma unroll
              for (int j = 0; j < NTC; ++j) {
                if (j < nt) {
                  const double v = tg.v[j];
                  double t;
                  bool hit;
                  if (mode == MLX_COLUMN_RISE) {
                    t = relative ? xc + v : v;
                    hit = xc >= t;
                  } else if (mode == MLX_COLUMN_FALL) {
                    t = relative ? xc - v : v;
                    hit = xc <= t;
                  } else {  // DEPART keeps v itself; |x_ref - x_ref| is 0 or NaN, never >= v > 0
                    t = v;
                    hit = false;
                  }
                  val[j][c] = hit ? canonical_nan() : t;
                  if (hit) done[c] |= 1u << j;
                }
              }
            } else {  // 5. the scan: is x[k] the first hit of a target?
#pragma unroll
              for (int j = 0; j < NTC; ++j) {
                if (j < nt && !(done[c] & (1u << j))) {
                  double t;
                  bool hit;
                  if (mode == MLX_COLUMN_RISE) {
                    t = val[j][c];
                    hit = xc >= t;
                  } else if (mode == MLX_COLUMN_FALL) {
                    t = val[j][c];
                    hit = xc <= t;
                  } else {
                    const double v = val[j][c];
                    hit = __builtin_fabs(xc - xref[c]) >= v;
                    t = xc > xref[c] ? xref[c] + v : xref[c] - v;
                  }
                  if (hit) {
                    val[j][c] = zprev + ((t - prev[c]) / (xc - prev[c])) * dzk;
                    done[c] |= 1u << j;
                  }
                }
              }
            }
            if (!xnan && k >= kref) {
              prev[c] = xc;
              zlast[c] = zk;
            }
            if (done[c] == allt) stop[c] = true;
          }
          all_stopped = all_stopped && stop[c];
        }
        fin = all_stopped;
      }
      // the wave goes on while one lane is still searching
      if (__builtin_amdgcn_ballot_w64(!fin) == 0) break;
      zprev = zk;
      ca = na;
      if constexpr (SIGMA) cb = nb;
    }

    // 6. what is not decided is a miss
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      if (done[c] != allt) {
        double m = canonical_nan();
        if (miss == MLX_COLUMN_MISS_FLOOR) m = floor != nullptr ? floor[col + c] : zlast[c];
#pragma unroll
        for (int j = 0; j < NTC; ++j)
          if (j < nt && !(done[c] & (1u << j))) val[j][c] = m;
      }
    }
#pragma unroll
    for (int j = 0; j < NTC; ++j) {
      if (j < nt) {
        double* __restrict__ o = out + (r * nt + j) * plane + col;
        Pack<double, VEC> e;
#pragma unroll
        for (int c = 0; c < VEC; ++c) e.v[c] = val[j][c];
        if constexpr (VEC == 1) o[0] = e.v[0];
        else store_pack<double, VEC, false>(o, e);
      }
    }
  }
}

// cells of a pack: 16 bytes of the widest field
inline int column_vec(int a_dtype, bool has_b, int b_dtype) {
  const size_t wide = has_b && dtype_size(b_dtype) > dtype_size(a_dtype) ? dtype_size(b_dtype)
                                                                        : dtype_size(a_dtype);
  return (int)(16 / wide);
}

// gridDim.y of a call over nrec > 0 records: one block row per record up to the cap, past which the
// rows stride.  The one rule: mlx_column_record_rows reports it, the launch uses it.
inline int64_t column_record_rows(int64_t nrec) {
  return nrec < (int64_t)kColMaxGridY ? nrec : (int64_t)kColMaxGridY;
}

struct ColumnCall {
  const void *a, *b;
  int eos;
  double p_ref;
  int64_t nrec, nz, plane;
  const double* z;
  int64_t kref;
  int mode, relative, miss;
  ColumnTargets tg;
  int nt;
  const double* floor;
  double* out;
  bool generic;
  dim3 grid;
  hipStream_t st;
};

template <typename TA, typename TB, int NTC>
void column_launch(const ColumnCall& c) {
#define MLX_COLUMN_GO(GENERIC)                                                                    \
  hipLaunchKernelGGL((k_column_crossing<TA, TB, NTC, GENERIC>), c.grid, dim3(kColBlock), 0, c.st, \
                     (const TA*)c.a, c.b, c.eos, c.p_ref, c.nrec, c.nz, c.plane, c.z, c.kref,     \
                     c.mode, c.relative, c.miss, c.tg, c.nt, c.floor, c.out)
  if (c.generic) MLX_COLUMN_GO(true);
  else MLX_COLUMN_GO(false);
#undef MLX_COLUMN_GO
}

template <typename TA, typename TB>
void column_dispatch(const ColumnCall& c) {
  if (c.nt <= 1) column_launch<TA, TB, 1>(c);
  else if (c.nt <= 2) column_launch<TA, TB, 2>(c);
  else if (c.nt <= 4) column_launch<TA, TB, 4>(c);
  else column_launch<TA, TB, 8>(c);
}

template <typename TA>
void column_dispatch_b(const ColumnCall& c, int b_dtype) {
  if (c.b == nullptr) column_dispatch<TA, NoField>(c);
  else if (b_dtype == MLX_DTYPE_F64) column_dispatch<TA, double>(c);
  else column_dispatch<TA, float>(c);
}

}  // namespace
}  // namespace mlx

extern "C" int64_t mlx_column_block_cells(int a_dtype, int has_b, int b_dtype, int generic) {
  using namespace mlx;
  if (!is_float_dtype(a_dtype) || (has_b && !is_float_dtype(b_dtype))) return 0;
  return (int64_t)kColBlock * (generic ? 1 : column_vec(a_dtype, has_b != 0, b_dtype));
}

extern "C" int mlx_column_record_rows(int64_t nrec) {
  if (nrec <= 0 || nrec > mlx::kColMaxCells) return 0;
  return (int)mlx::column_record_rows(nrec);
}

extern "C" int mlx_column_crossing(const void* a, int a_dtype, const void* b, int b_dtype, int eos,
                                   double p_ref, int64_t nrec, int64_t nz, int64_t plane,
                                   const double* z, int64_t kref, int mode, int relative, int miss,
                                   const double* targets, int ntargets, const double* floor,
                                   double* out, void* stream) {
  using namespace mlx;
  using detail::fail;
  using detail::hip_status;
  const bool sigma = b != nullptr;
  if (!is_float_dtype(a_dtype)) return fail(MLX_E_ENUM, "a_dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  if (sigma && !is_float_dtype(b_dtype))
    return fail(MLX_E_ENUM, "b_dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  if (sigma && eos != MLX_EOS_WRIGHT && eos != MLX_EOS_LINEAR)
    return fail(MLX_E_ENUM, "eos must be MLX_EOS_WRIGHT or MLX_EOS_LINEAR");
  if (mode != MLX_COLUMN_RISE && mode != MLX_COLUMN_FALL && mode != MLX_COLUMN_DEPART)
    return fail(MLX_E_ENUM, "mode must be MLX_COLUMN_RISE, MLX_COLUMN_FALL or MLX_COLUMN_DEPART");
  if (relative != 0 && relative != 1) return fail(MLX_E_ENUM, "relative must be 0 or 1");
  if (miss != MLX_COLUMN_MISS_NAN && miss != MLX_COLUMN_MISS_FLOOR)
    return fail(MLX_E_ENUM, "miss must be MLX_COLUMN_MISS_NAN or MLX_COLUMN_MISS_FLOOR");
  if (ntargets < 1 || ntargets > MLX_COLUMN_MAX_TARGETS)
    return fail(MLX_E_SHAPE, "need 1 <= ntargets <= MLX_COLUMN_MAX_TARGETS");
  if (nz < 1) return fail(MLX_E_SHAPE, "need nz >= 1");
  if (kref < 0 || kref >= nz) return fail(MLX_E_SHAPE, "need 0 <= kref < nz");
  if (nrec < 0 || plane < 0) return fail(MLX_E_SHAPE, "nrec and plane must not be negative");
  if (nz > kColMaxCells || (nrec > 0 && plane > 0 &&
                            (plane > kColMaxCells / nz || nrec > kColMaxCells / (nz * plane))))
    return fail(MLX_E_SHAPE, "need nrec * nz * plane <= 2^38");
  if (mode == MLX_COLUMN_DEPART && !relative)
    return fail(MLX_E_SHAPE, "MLX_COLUMN_DEPART is relative to x[kref]: relative must be 1");
  if (nrec == 0 || plane == 0) return 0;
  if (!a || !z || !targets || !out) return fail(MLX_E_NULL, "a, z, targets and out must not be NULL");
  if (!aligned(a, dtype_size(a_dtype)) || (sigma && !aligned(b, dtype_size(b_dtype))) ||
      !aligned(z, 8) || !aligned(targets, 8) || !aligned(floor, 8) || !aligned(out, 8))
    return fail(MLX_E_ALIGN, "a / b / z / targets / floor / out not aligned to their element");
  ColumnCall c;
  for (int j = 0; j < MLX_COLUMN_MAX_TARGETS; ++j) c.tg.v[j] = 0.0;
  for (int j = 0; j < ntargets; ++j) {
    if (targets[j] != targets[j]) return fail(MLX_E_SHAPE, "targets must not hold NaN");
    if (relative && !(targets[j] > 0.0)) return fail(MLX_E_SHAPE, "relative targets must be > 0");
    c.tg.v[j] = targets[j];
  }
  const int vec = column_vec(a_dtype, sigma, b_dtype);
  // packs: every level of every record starts on a pack boundary, and so does every out plane
  c.generic = plane % vec != 0 || !aligned(a, vec * dtype_size(a_dtype)) ||
              (sigma && !aligned(b, vec * dtype_size(b_dtype))) || !aligned(out, 16);
  const int64_t per_block = (int64_t)kColBlock * (c.generic ? 1 : vec);
  c.grid = dim3((unsigned)ceil_div(plane, per_block), (unsigned)column_record_rows(nrec));
  c.a = a, c.b = b, c.eos = eos, c.p_ref = p_ref;
  c.nrec = nrec, c.nz = nz, c.plane = plane, c.z = z, c.kref = kref;
  c.mode = mode, c.relative = relative, c.miss = miss, c.nt = ntargets;
  c.floor = floor, c.out = out;
  c.st = static_cast<hipStream_t>(stream);
  if (a_dtype == MLX_DTYPE_F64) column_dispatch_b<double>(c, b_dtype);
  else column_dispatch_b<float>(c, b_dtype);
  return hip_status(hipGetLastError(), "k_column_crossing launch");
}
