// Shared by feature translation units of libmomlevel_hip.so: a pack of adjacent cells that moves in
// one memory instruction, and the operand checks of their entry points.  Nothing here is part of the
// C ABI.  Included by momlevel_strat.hip and momlevel_clim.hip, whose kernels compile to the
// instructions they had with their private copies.  (momlevel_hip.hip keeps its own load_pack: its
// sources are the ones whose hash guards the committed steric profiles.  The trend, gauge, spice
// and vort units keep theirs until a GPU visit times them: moving them changes their code -- the
// `double` spelling of a float32 pair there costs LDS and the `nt` policy -- and their hashes, which
// the committed logs under profiles/ quote.)
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
