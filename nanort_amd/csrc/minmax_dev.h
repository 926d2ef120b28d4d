// nanort_amd/csrc/minmax_dev.h — the comparison helpers of the builder (build.hip, build_subtree.hip) and the refit (refit.hip).
//
// Both compute node boxes with these exact selects, in a fixed order, so a box never depends on scheduling and a refit of
// an unchanged mesh reproduces the built boxes.
#pragma once

#include <hip/hip_runtime.h>

namespace nrt {

template <typename T>
struct Lim;
template <>
struct Lim<float> {
  static __device__ __forceinline__ float max() { return 3.402823466e+38f; }
  static __device__ __forceinline__ float inf() { return __builtin_huge_valf(); }
};
template <>
struct Lim<double> {
  static __device__ __forceinline__ double max() { return 1.7976931348623157e+308; }
  static __device__ __forceinline__ double inf() { return __builtin_huge_val(); }
};

template <typename T>
__device__ __forceinline__ T tmin(T a, T b) {
  return (b < a) ? b : a;
}
template <typename T>
__device__ __forceinline__ T tmax(T a, T b) {
  return (a < b) ? b : a;
}

} // namespace nrt
