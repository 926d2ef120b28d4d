// nanort_amd/csrc/motion.hip — motion-blur traversal for gfx950: every ray carries a shutter time, every triangle two keyframes.
//
// The contract is include/nanort_hip.h's (nrtTraverseBatchMotion* / nrtOccludedBatchMotion*):
//   * the reference's binary loop over the context's node array (nanort.h:2487-2556) — binary_walk (binary_walk_dev.h), the loop
//     k_traverse and the multi-hit walk run, with the query below; lane_init / slab_test / tri_test of traverse_dev.h unchanged.
//     The boxes of a motion context hold both keyframes (build.hip, k_prim_records<T, true>), so the walk reaches every leaf the
//     moving triangle can be in whatever the ray's time is;
//   * refill: the lane loads times[rid] with its ray, clamps it (nanort_motion::ClampTime) and keeps the shutter time in one register;
//   * leaf step: the record of keyframe 0 (a.tris[k]) and of keyframe 1 (tris1[k], the same leaf order) are interpolated component
//     by component (nanort_motion::Lerp — THE rule, shared with the host intersector of include/nanort.h) into one LeafTri, which
//     goes through tri_test exactly as k_traverse's leaf step hands it a stored record; prim_id is record 0's;
//   * occlusion (a.any_hit): a ray is settled once hit_t < max_t — the predicate the finish writes as the closest-hit flag; a
//     settled lane tests no further record and finishes its ray;
//   * finish: the record and mask stores of k_traverse (store_closest_hit).
// Like the multi-hit walk the launch publishes no completion record: its slot is closed by an event (api_query.hip, enqueue_launch).
#include "binary_walk_dev.h"
#include "kernels.h"
#include "motion_dev.h" // motion_record: the interpolated leaf record (shared with query.hip)

namespace nrt {

template <typename T>
struct MotionArgs {
  TraverseArgs<T> a;       // the closest-hit launch block (a.tris: the leaf records of keyframe 0)
  const LeafTri<T> *tris1; // the leaf records of keyframe 1, in the same leaf order
  const T *times;          // [num_rays] one time per ray, or null: every ray at time 0
};

// The motion query of the binary walk: closest hit, or occlusion when `any`.
template <typename T>
struct MotionQuery : BinaryQuery {
  const MotionArgs<T> &m;
  const bool any;     // an occlusion query (a.any_hit; wave-uniform)
  T shutter = T(0);   // the clamped time of the ray this lane holds

  __device__ __forceinline__ typename Wire<T>::Ray load(const TraverseArgs<T> &a, uint32_t rid) const {
    return load_ray<T>(as_global(a.rays) + rid, 0u); // (k_traverse's load without its probe bit: this walk has no profiling arm)
  }
  __device__ __forceinline__ void begin(const TraverseArgs<T> &, uint32_t rid) {
    shutter = m.times != nullptr ? nanort_motion::ClampTime<T>(as_global(m.times)[rid]) : T(0);
  }
  // an occlusion query's ray is settled by the first record that brings hit_t below max_t: its lane's records end there
  __device__ __forceinline__ bool settled(const Lane<T> &L) const { return any && L.hit_t < L.max_t; }
  // the lane interpolates the record to its own time and tests it
  __device__ __forceinline__ void record(const TraverseArgs<T> &a, Lane<T> &L, uint32_t, uint32_t k) const {
    const LeafTri<T> k0 = a.tris[k];
    const LeafTri<T> k1 = m.tris1[k];
    const LeafTri<T> tri = motion_record<T>(k0, k1, shutter);
    tri_test<T>(L, tri, true, a.range0, a.range1, a.skip_prim, a.cull_back_face != 0);
  }
  __device__ __forceinline__ void finish(const TraverseArgs<T> &a, const Lane<T> &L, uint32_t rid) const { store_closest_hit<T>(a, L, rid); }
};

template <typename T, int STACK>
__global__ __launch_bounds__(kTraverseBlock) void k_traverse_motion(const MotionArgs<T> m) {
  // [depth][thread]: a wave's 64 lanes hit 64 consecutive dwords -> conflict-free.
  __shared__ uint32_t s_stack[STACK][kTraverseBlock];
  binary_walk<T, STACK>(m.a, s_stack, MotionQuery<T>{{}, m, m.a.any_hit != 0});
}

template <typename T>
hipError_t launch_traverse_motion(const TraverseArgs<T> &args, const void *tris1, const T *times, unsigned grid, hipStream_t s) {
  MotionArgs<T> m;
  m.a = args;
  m.tris1 = (const LeafTri<T> *)tris1;
  m.times = times;
  launch_persistent((const void *)k_traverse_motion<T, kLdsStackDefault>, grid, m, s);
  return hipGetLastError();
}

template <typename T>
int traverse_motion_blocks_per_cu() {
  return resident_blocks((const void *)k_traverse_motion<T, kLdsStackDefault>, 1);
}

NRT_INSTANTIATE_F32_F64(launch_traverse_motion)
NRT_INSTANTIATE_F32_F64(traverse_motion_blocks_per_cu)

} // namespace nrt

