// nanort_amd/csrc/query.hip — the combined ray query for gfx950: per-ray skip ids, visibility masks and motion times on the SAME ray.
//
// The contract is include/nanort_hip.h's (nrtQueryBatch* with two or more of the three):
//   * the reference's binary loop over the context's node array (nanort.h:2487-2556) — binary_walk (binary_walk_dev.h), the loop
//     k_traverse, the multi-hit, the motion and the masked walk run, with the query below; lane_init / slab_test / tri_test of
//     traverse_dev.h unchanged;
//   * MOTION and MASKED are COMPILE-TIME: the instantiation without MOTION never fetches keyframe 1 and has no shutter register, the
//     one without MASKED never fetches a word.  Three instantiations per precision: {MOTION, ids}, {MASKED, ids}, {MOTION, MASKED}
//     with or without ids (a launch with one feature alone is k_traverse_motion's or k_traverse_masked's, with ids alone k_traverse's
//     or the wide walk's: api_query.hip);
//   * refill: the lane loads its ray's time (clamped: nanort_motion::ClampTime), its word and its skip id with the ray, each only if
//     its array is there (null times: time 0; null words: 0xFFFFFFFF; null ids: the launch's skip_prim_id), one register each;
//   * leaf step: leaf_masks[k], a.tris[k] and tris1[k] are three independent loads of one address computation, issued together (as
//     masked.hip explains for the first two); the record is interpolated to the lane's time (motion_dev.h) and goes through tri_test
//     with `active` = (word & ray_mask) != 0 and the lane's own skip id — an invisible record, a record outside prim_ids_range and
//     the skipped record take part in no reject and no accept, which is the reference's intersector returning false before it
//     touches the ray's state;
//   * occlusion (a.any_hit), finish: as in the motion and masked walks — settled once hit_t < max_t, store_closest_hit.
// Like those walks the launch publishes no completion record: its slot is closed by an event (api_query.hip, enqueue_launch).
#include "binary_walk_dev.h"
#include "kernels.h"
#include "motion_dev.h"

namespace nrt {

template <typename T>
struct QueryArgs {
  TraverseArgs<T> a;          // the closest-hit launch block (a.tris: the leaf records of keyframe 0; a.skip_ids: one id per ray, or null)
  const LeafTri<T> *tris1;    // MOTION: the leaf records of keyframe 1, in the same leaf order
  const T *times;             // MOTION: [num_rays] one time per ray, or null: every ray at time 0
  const uint32_t *leaf_masks; // MASKED: [num_indices] the triangles' words in leaf order, beside a.tris
  const uint32_t *ray_masks;  // MASKED: [num_rays] one word per ray, or null: every ray 0xFFFFFFFF
};

// The combined query of the binary walk: closest hit, or occlusion when `any`.
template <typename T, bool MOTION, bool MASKED>
struct CombinedQuery : BinaryQuery {
  const QueryArgs<T> &m;
  const bool any;           // an occlusion query (a.any_hit; wave-uniform)
  T shutter = T(0);         // MOTION: the clamped time of the ray this lane holds
  uint32_t ray_mask = ~0u;  // MASKED: its word
  uint32_t skip = kInvalid; // its skip id

  __device__ __forceinline__ typename Wire<T>::Ray load(const TraverseArgs<T> &a, uint32_t rid) const {
    return load_ray<T>(as_global(a.rays) + rid, 0u); // (as the motion walk: no profiling arm)
  }
  __device__ __forceinline__ void begin(const TraverseArgs<T> &a, uint32_t rid) {
    if constexpr (MOTION) shutter = m.times != nullptr ? nanort_motion::ClampTime<T>(as_global(m.times)[rid]) : T(0);
    if constexpr (MASKED) ray_mask = m.ray_masks != nullptr ? as_global(m.ray_masks)[rid] : ~0u;
    skip = a.skip_ids != nullptr ? as_global(a.skip_ids)[rid] : a.skip_prim;
  }
  __device__ __forceinline__ bool settled(const Lane<T> &L) const { return any && L.hit_t < L.max_t; }
  // the word and the record(s) are fetched together; the word decides whether the record exists for this ray
  __device__ __forceinline__ void record(const TraverseArgs<T> &a, Lane<T> &L, uint32_t, uint32_t k) const {
    uint32_t word = ~0u;
    if constexpr (MASKED) word = as_global(m.leaf_masks)[k];
    LeafTri<T> tri = a.tris[k];
    if constexpr (MOTION) {
      const LeafTri<T> k1 = m.tris1[k];
      tri = motion_record<T>(tri, k1, shutter);
    }
    tri_test<T>(L, tri, (word & ray_mask) != 0u, a.range0, a.range1, skip, a.cull_back_face != 0);
  }
  __device__ __forceinline__ void finish(const TraverseArgs<T> &a, const Lane<T> &L, uint32_t rid) const { store_closest_hit<T>(a, L, rid); }
};

template <typename T, int STACK, bool MOTION, bool MASKED>
__global__ __launch_bounds__(kTraverseBlock) void k_traverse_query(const QueryArgs<T> m) {
  // [depth][thread]: a wave's 64 lanes hit 64 consecutive dwords -> conflict-free.
  __shared__ uint32_t s_stack[STACK][kTraverseBlock];
  binary_walk<T, STACK>(m.a, s_stack, CombinedQuery<T, MOTION, MASKED>{{}, m, m.a.any_hit != 0});
}

// The instantiation a launch with these features runs (a launch with neither never arrives: api_query.hip).
template <typename T>
static const void *query_kernel(bool motion, bool masked) {
  if (motion && masked) return (const void *)k_traverse_query<T, kLdsStackDefault, true, true>;
  return motion ? (const void *)k_traverse_query<T, kLdsStackDefault, true, false> : (const void *)k_traverse_query<T, kLdsStackDefault, false, true>;
}

template <typename T>
hipError_t launch_traverse_query(const TraverseArgs<T> &args, bool motion, bool masked, const void *tris1, const T *times, const uint32_t *leaf_masks,
                                 const uint32_t *ray_masks, unsigned grid, hipStream_t s) {
  if (!motion && !masked) return hipErrorInvalidValue;
  QueryArgs<T> m;
  m.a = args;
  m.tris1 = motion ? (const LeafTri<T> *)tris1 : nullptr;
  m.times = motion ? times : nullptr;
  m.leaf_masks = masked ? leaf_masks : nullptr;
  m.ray_masks = masked ? ray_masks : nullptr;
  launch_persistent(query_kernel<T>(motion, masked), grid, m, s);
  return hipGetLastError();
}

template <typename T>
int traverse_query_blocks_per_cu(bool motion, bool masked) {
  return resident_blocks(query_kernel<T>(motion, masked), 1);
}

NRT_INSTANTIATE_F32_F64(launch_traverse_query)
NRT_INSTANTIATE_F32_F64(traverse_query_blocks_per_cu)

} // namespace nrt
