// include/nanort_motion.h — THE one statement of the motion-blur vertex rule (include/nanort_hip.h, "motion blur").
//
// A triangle mesh may hold a second vertex keyframe.  A vertex moves linearly between keyframe 0 (a) and keyframe 1 (b); its
// position at a ray's shutter time is defined per component, each operation rounded on its own (no contraction: the library and
// every program that wants its bits compile with -ffp-contract=off):
//
//   s = (time > 0) ? (time < 1 ? time : 1) : 0          // NaN and negatives -> 0, above 1 -> 1
//   x = (T(1) - s) * a + s * b
//   x = x < min(a, b) ? min(a, b) : (x > max(a, b) ? max(a, b) : x)
//
// Time 0 is keyframe 0 and time 1 is keyframe 1, and the clamp puts every interpolated vertex inside the box the builder gives the
// primitive (the union of the two keyframes' boxes), so a moving triangle is as watertight against its boxes as a static one.
//
// Included by the device walk (nanort_amd/csrc/own_walks.hip) and by the host intersector (nanort.h, MotionTriangleIntersector).
#ifndef NANORT_MOTION_H_
#define NANORT_MOTION_H_

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NANORT_MOTION_FN __host__ __device__ inline
#else
#define NANORT_MOTION_FN inline
#endif

namespace nanort_motion {

// The shutter time a ray's `time` stands for.
template <typename T>
NANORT_MOTION_FN T ClampTime(T time) {
  return (time > T(0)) ? (time < T(1) ? time : T(1)) : T(0);
}

// One component of a vertex at shutter time `s` (already clamped): a at keyframe 0, b at keyframe 1.
template <typename T>
NANORT_MOTION_FN T Lerp(T a, T b, T s) {
  const T lo = (b < a) ? b : a;
  const T hi = (a < b) ? b : a;
  const T x = (T(1) - s) * a + s * b;
  return x < lo ? lo : (x > hi ? hi : x);
}

}  // namespace nanort_motion

#endif  // NANORT_MOTION_H_
