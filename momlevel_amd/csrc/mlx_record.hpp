// Shared by the translation units that work on a (time, cells) record of float64 or float32 in
// which a lane owns a 16-byte pack of adjacent cells: momlevel_trend.hip, momlevel_clim.hip,
// momlevel_filter.hip and momlevel_quantile.hip.  The record's shape limits, the one rule for the
// cells a lane takes, the dtype x width dispatch, and the row of one time step as the grouped
// kernels read it.  Nothing here is part of the C ABI, and nothing here has fewer than two users.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "eos_device.hpp"
#include "mlx_internal.hpp"
#include "mlx_pack.hpp"

namespace mlx {

// ---- host side
constexpr int64_t kMaxCells = (int64_t)1 << 38;
// grid x: the record kernels run blocks of 256 lanes, a cell a lane at least
static_assert((kMaxCells >> 8) <= 2147483647LL, "a row of kMaxCells cells fits grid x");

// 0 < nt < max_steps, 0 < n <= kMaxCells, and every byte offset into nt * n cells fits int64
inline bool record_fits(int64_t nt, int64_t n, int64_t max_steps) {
  int64_t total;
  return nt > 0 && n > 0 && nt < max_steps && n <= kMaxCells &&
         !__builtin_mul_overflow(nt, n, &total) && total <= INT64_MAX / 64;
}

// A record whose steps are listed in groups: steps[offsets[g] .. offsets[g + 1]) for g < ngroups,
// nsel entries in all, and rows_per_group result rows of n cells per group.  Both lists may be NULL
// together: one group of every row (a caller that has no such mode refuses NULL lists first).  What
// the entry points of the grouped kernels refuse alike; 0, or the code that detail::fail recorded.
inline int check_grouped(const void* y, int dtype, const int32_t* steps, const int64_t* offsets,
                         int64_t nsel, int64_t ngroups, int64_t nt, int64_t n,
                         int64_t rows_per_group) {
  using detail::fail;
  if (!y) return fail(MLX_E_NULL, "y must not be NULL");
  if ((steps == nullptr) != (offsets == nullptr))
    return fail(MLX_E_NULL, "steps and offsets must both be given or both be NULL");
  if (!steps && ngroups != 1)
    return fail(MLX_E_NULL, "NULL steps / offsets mean one group of all rows: ngroups must be 1");
  if (!is_float_dtype(dtype)) return fail(MLX_E_ENUM, "dtype must be MLX_DTYPE_F64 or MLX_DTYPE_F32");
  int64_t rows;
  if (!record_fits(nt, n, (int64_t)1 << 31) || nsel <= 0 || nsel >= ((int64_t)1 << 31) ||
      ngroups <= 0 || __builtin_mul_overflow(ngroups, n, &rows) ||
      rows > INT64_MAX / (64 * rows_per_group))
    return fail(MLX_E_SHAPE,
                "need 0 < nt, nsel < 2^31, ngroups > 0, 0 < n <= 2^38, nt*n and the result addressable");
  if (!steps && nsel != nt)
    return fail(MLX_E_SHAPE, "NULL steps / offsets list every row: nsel must equal nt");
  if (!aligned(y, dtype_size(dtype))) return fail(MLX_E_ALIGN, "y not element-aligned");
  if (steps && (!aligned(steps, 4) || !aligned(offsets, 8)))
    return fail(MLX_E_ALIGN, "steps not 4-byte or offsets not 8-byte aligned");
  return 0;
}

// A row pointer of a launch and the bytes one cell takes in it; a NULL pointer is not an operand.
struct Operand {
  const void* p;
  size_t cell;
};

// Cells per lane: the widest v in {16 / elem, .., 2, 1} that divides every row (n % v == 0) and
// keeps every row of every operand aligned to its access, min(16, cell * v) bytes (a pack wider
// than 16 bytes moves as accesses of 16).
inline int pack_width(int64_t n, size_t elem, std::initializer_list<Operand> operands) {
  for (int v = (int)(16 / elem); v > 1; v /= 2) {
    bool ok = n % v == 0;
    for (const Operand& o : operands)
      ok = ok && (o.p == nullptr || aligned(o.p, o.cell * v < 16 ? o.cell * v : 16));
    if (ok) return v;
  }
  return 1;
}

template <typename T>
struct TypeTag {
  typedef T type;
};

// f(TypeTag<T>, integral_constant<int, V>) for the record's element type and v cells per lane:
// the five instantiations a record kernel has.
template <typename F>
inline int dispatch_pack(int dtype, int v, F&& f) {
  using std::integral_constant;
  if (dtype == MLX_DTYPE_F64)
    return v == 2 ? f(TypeTag<double>{}, integral_constant<int, 2>{})
                  : f(TypeTag<double>{}, integral_constant<int, 1>{});
  return v == 4   ? f(TypeTag<float>{}, integral_constant<int, 4>{})
         : v == 2 ? f(TypeTag<float>{}, integral_constant<int, 2>{})
                  : f(TypeTag<float>{}, integral_constant<int, 1>{});
}

// ---- device side
// The row of step index s.  s is wave-uniform.  An index outside [0, nt) -- a caller's mistake the
// entry point cannot see -- reads row 0 and is a row of NaN: never out of bounds.
template <typename TIn, int V>
struct Row {
  Pack<TIn, V> raw;
  bool ok;
  __device__ __forceinline__ double at(int k) const {
    return ok ? (double)raw.v[k] : canonical_nan();  // float32 -> float64 is exact
  }
  __device__ __forceinline__ bool valid(int k) const { return ok && raw.v[k] == raw.v[k]; }
};

// NT: load_pack's cache policy.  CHECKED: test s against nt; without it the caller walks [0, nt).
template <typename TIn, int V, bool NT, bool CHECKED>
__device__ __forceinline__ Row<TIn, V> row_load(const TIn* __restrict__ ycol, int32_t s, int64_t nt,
                                                int64_t n) {
  Row<TIn, V> r;
  r.ok = CHECKED ? (uint32_t)s < (uint32_t)nt : true;
  r.raw = load_pack<TIn, V, NT>(ycol + (int64_t)(r.ok ? s : 0) * n);
  return r;
}

// the bounds of group g, clamped to the list
__device__ __forceinline__ void group_bounds(const int64_t* __restrict__ offsets, int64_t g,
                                             int64_t nsel, int64_t& lo, int64_t& hi) {
  lo = offsets[g];
  hi = offsets[g + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > nsel ? nsel : hi;
}

// a float64 result as the output's element: the canonical NaN, or the one rounding to float32
template <typename TOut>
__device__ __forceinline__ TOut narrow(double res, bool nan) {
  if constexpr (sizeof(TOut) == 8) {
    return nan ? canonical_nan() : res;
  } else {
    return nan ? canonical_nan_f32() : (float)res;
  }
}

}  // namespace mlx
