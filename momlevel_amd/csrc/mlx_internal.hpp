// Shared by the translation units of libmomlevel_hip.so; nothing here is part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace mlx {
namespace detail {
// record the text mlx_last_error() returns on this thread and hand back `code`
__attribute__((visibility("hidden"))) int fail(int code, const char* msg);
// 0 for hipSuccess; otherwise records "<what>: <hip error string>" and returns the hipError_t
__attribute__((visibility("hidden"))) int hip_status(hipError_t e, const char* what);
}  // namespace detail

// The codes of include/momlevel_path.h for the translation units that answer its queries.
// momlevel_promote.hip includes that header and holds these to it; momlevel_hip.hip is also
// compiled on its own beside include/momlevel_hip.h alone (tests/test_isa_flags.py).
namespace path {
constexpr int kGeneric = 0, kFast = 1, kFastP3D = 2;
constexpr int kAlignedT = 1, kAlignedS = 2, kAlignedOut = 4, kAlignedP = 8, kAlignedAll = 15;
}  // namespace path

// calc_dz's arithmetic for one cell and level (derived.py:295-318, fraction=False): the thickness
// of the part of the level [ztop, zbot] that lies below `top` and above `d`, where d is the sea
// floor after fillna(0.0) and, with a bottom, np.minimum(depth, bottom).  The ONE definition for
// K2's default dz (top = 0, no bottom), k_calc_dz and the layer integral (momlevel_layer.hip), so
// that their bits cannot drift.  NANS: np.minimum's NaN propagation, for callers whose d or top
// may be NaN (k_calc_dz: a NaN top / bottom is the caller's); without it the selects are K2's.
template <bool NANS>
__device__ __forceinline__ double calc_dz_cell(double d, double ztop, double zbot, double top) {
  const double dz_field = zbot - ztop;
  double part = d - ztop;
  part = (part < 0.0) ? 0.0 : part;
  double result = ((NANS && part != part) || part < dz_field) ? part : dz_field;  // np.minimum
  part = zbot - top;
  part = (part < 0.0) ? 0.0 : part;
  result = ((NANS && part != part) || part < result) ? part : result;
  return result;
}
}  // namespace mlx
