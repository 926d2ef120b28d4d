// nanort_amd/csrc/motion_dev.h — the leaf record of a moving triangle at a ray's time: the one device statement of it, which the
// motion walk (motion.hip) and the combined query walk (query.hip) share.  The rule itself is include/nanort_motion.h's.
#pragma once

#include "traverse_dev.h"
#include "../../include/nanort_motion.h"

namespace nrt {

// The leaf record a ray at shutter time `s` sees: nine interpolated components, the id of keyframe 0's record.
template <typename T>
__device__ __forceinline__ LeafTri<T> motion_record(const LeafTri<T> &k0, const LeafTri<T> &k1, T s) {
  LeafTri<T> tri;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    tri.p0[j] = nanort_motion::Lerp<T>(k0.p0[j], k1.p0[j], s);
    tri.p1[j] = nanort_motion::Lerp<T>(k0.p1[j], k1.p1[j], s);
    tri.p2[j] = nanort_motion::Lerp<T>(k0.p2[j], k1.p2[j], s);
  }
  tri.prim_id = k0.prim_id;
  return tri;
}

} // namespace nrt
