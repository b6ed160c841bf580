// Shared by feature translation units of libmomlevel_hip.so: a pack of adjacent cells that moves in
// one memory instruction, and the operand checks of their entry points.  Nothing here is part of the
// C ABI.  Every feature unit but momlevel_trend.hip takes its pack I/O from here (mlx_record.hpp
// adds what the (time, cells) record units share on top; momlevel_gauge.hip uses the host checks):
//   strat, clim, area, layer, filter, quantile, spice: the instructions of a private copy.
//   vort: 18 of its 36 kernels changed with the move.  The private copy loaded a float32 pair as one
//     `double`, which in the mixed-dtype kernels went through 4 to 12 KiB of LDS; on load_pack they
//     use none and up to 6 VGPRs fewer.  Timed against the parent's library on one MI355X
//     (profiles/record_fold_ab.log; scripts/bench_vort.py, alternating processes): no case slower
//     than the parent's slowest round, the 14 mixed-dtype cases 3 to 17 % faster.
//   trend: keeps its own TPack / tload / tstore.  On load_pack / store_pack 16 float32 kernels
//     changed and the two-cell ones measured slower in the same log (1200 x 1081 x 1442, float32,
//     median against the parent's slowest round): k_time_linfit 1.62-1.65 ms against 1.53,
//     k_time_project<6> 1.68-1.70 against 1.60, k_time_apply remove 5.48-5.49 against 5.40; model_resid
//     5.56 against 5.59 passed.  The private `double` spelling of a float32 pair loses the `nt`
//     policy on the loads of the unrolled fit loop, and that is the faster code.
//   momlevel_hip.hip keeps its own load_pack: its sources are the ones whose hash guards the
//     committed steric profiles, and the move changes 228 of its 473 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/momlevel_hip.h"

namespace mlx {

template <typename T, int V>
struct Pack {
  T v[V];
};

// What one access moves: N cells of T as a vector of T itself (global_{load,store}_dword / dwordx2 /
// dwordx4), unpacked element by element: no type punning for the compiler to trip over.
template <typename T, int N>
struct PackWord {
  typedef T type __attribute__((ext_vector_type(N)));
};
template <typename T>
struct PackWord<T, 1> {
  typedef T type;
};

// V cells of T in one access of 4, 8 or 16 bytes (32 bytes: two of 16); p is aligned to the access.
// NT: the `nt` cache policy, for data that is touched once.
template <typename T, int V, bool NT>
__device__ __forceinline__ Pack<T, V> load_pack(const T* __restrict__ p) {
  constexpr int B = (int)sizeof(T) * V, W = B == 32 ? 16 : B;
  static_assert(B == 4 || B == 8 || B == 16 || B == 32, "a pack is 4, 8, 16 or 32 bytes");
  typedef typename PackWord<T, W / (int)sizeof(T)>::type word;
  Pack<T, V> r;
#pragma unroll
  for (int h = 0; h < B / W; ++h) {
    const word* q = reinterpret_cast<const word*>(p) + h;
    const word raw = NT ? __builtin_nontemporal_load(q) : *q;
    if constexpr (W == (int)sizeof(T)) {
      r.v[h] = raw;
    } else {
#pragma unroll
      for (int k = 0; k < W / (int)sizeof(T); ++k) r.v[h * (W / (int)sizeof(T)) + k] = raw[k];
    }
  }
  return r;
}

template <typename T, int V, bool NT>
__device__ __forceinline__ void store_pack(T* __restrict__ p, const Pack<T, V>& r) {
  constexpr int B = (int)sizeof(T) * V, W = B == 32 ? 16 : B;
  static_assert(B == 4 || B == 8 || B == 16 || B == 32, "a pack is 4, 8, 16 or 32 bytes");
  typedef typename PackWord<T, W / (int)sizeof(T)>::type word;
#pragma unroll
  for (int h = 0; h < B / W; ++h) {
    word raw;
    if constexpr (W == 16) {
      __builtin_memcpy(&raw, reinterpret_cast<const char*>(&r) + h * W, W);
    } else if constexpr (W == (int)sizeof(T)) {
      raw = r.v[h];
    } else {  // two float32 cells
      raw = word{r.v[0], r.v[1]};
    }
    word* q = reinterpret_cast<word*>(p) + h;
    if constexpr (NT) __builtin_nontemporal_store(raw, q);
    else *q = raw;
  }
}

// ---- host side: the operand checks of the entry points
inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }
inline int64_t ceil_div(int64_t a, int64_t b) { return a / b + (a % b != 0); }
inline bool is_float_dtype(int dt) { return dt == MLX_DTYPE_F64 || dt == MLX_DTYPE_F32; }
inline size_t dtype_size(int dt) { return dt == MLX_DTYPE_F64 ? 8 : 4; }

}  // namespace mlx
