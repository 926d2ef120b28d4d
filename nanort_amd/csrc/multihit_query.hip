// nanort_amd/csrc/multihit_query.hip — multi-hit with per-ray skip ids, visibility masks and motion times for gfx950: the K frontmost
// triangles of every ray, under the intersector of the combined ray query.
//
// The contract is include/nanort_hip.h's (nrtMultiHitQueryBatch*): the multi-hit contract (multihit.hip) in which
// "the intersector" is the one of nrtQueryBatch* (query.hip).  The kernel composes the two queries of binary_walk (binary_walk_dev.h)
// that state those halves:
//   * refill, as CombinedQuery::begin: the lane loads its ray's time (clamped: nanort_motion::ClampTime), its word and its skip id with
//     the ray, each only if its array is there (null times: time 0; null words: 0xFFFFFFFF; null ids: the launch's skip_prim_id), and
//     empties its K-buffer;
//   * MOTION and MASKED are COMPILE-TIME: the instantiation without MOTION never fetches keyframe 1 and has no shutter register, the
//     one without MASKED never fetches a word.  Four instantiations per precision — <false, false> is the launch with ids alone, which
//     no other entry point can express;
//   * leaf step: leaf_masks[k], a.tris[k] and tris1[k] are three independent loads of one address computation, issued together; the
//     record is interpolated to the lane's time (motion_dev.h) and goes through tri_test with `active` = (word & ray_mask) != 0 and the
//     lane's own skip id, against L.hit_t = B with L.prim = kInvalid — an invisible record, a record outside prim_ids_range and the
//     skipped record take part in no reject and no accept, so they never become candidates; what tri_test accepted is offered to the
//     K-buffer (multihit_dev.h: enter / insert / new bound, the statement k_traverse_multihit runs);
//   * finish: the K-buffer's miss fill and count.
// Like the multi-hit walk the launch publishes no completion record: its slot is closed by an event (api_query.hip, enqueue_launch).
#include "kernels.h"
#include "motion_dev.h"
#include "multihit_dev.h"

namespace nrt {

template <typename T>
struct MultiHitQueryArgs {
  MultiHitArgs<T> mh;         // the multi-hit launch block (mh.a.tris: the leaf records of keyframe 0; mh.a.skip_ids: one id per ray, or null)
  const LeafTri<T> *tris1;    // MOTION: the leaf records of keyframe 1, in the same leaf order
  const T *times;             // MOTION: [num_rays] one time per ray, or null: every ray at time 0
  const uint32_t *leaf_masks; // MASKED: [num_indices] the triangles' words in leaf order, beside mh.a.tris
  const uint32_t *ray_masks;  // MASKED: [num_rays] one word per ray, or null: every ray 0xFFFFFFFF
};

// The multi-hit query of the binary walk under the combined intersector.  L.hit_t == B outside the triangle test.
template <typename T, bool MOTION, bool MASKED>
struct MultiHitCombinedQuery : BinaryQuery {
  const MultiHitQueryArgs<T> &m;
  KBuffer<T> kb;
  T shutter = T(0);         // MOTION: the clamped time of the ray this lane holds
  uint32_t ray_mask = ~0u;  // MASKED: its word
  uint32_t skip = kInvalid; // its skip id

  __device__ __forceinline__ typename Wire<T>::Ray load(const TraverseArgs<T> &a, uint32_t rid) const {
    return load_ray_nt<T>(a.rays + rid); // (as the multi-hit walk)
  }
  __device__ __forceinline__ void begin(const TraverseArgs<T> &a, uint32_t rid) {
    if constexpr (MOTION) shutter = m.times != nullptr ? nanort_motion::ClampTime<T>(as_global(m.times)[rid]) : T(0);
    if constexpr (MASKED) ray_mask = m.ray_masks != nullptr ? as_global(m.ray_masks)[rid] : ~0u;
    skip = a.skip_ids != nullptr ? as_global(a.skip_ids)[rid] : a.skip_prim;
    kb.reset();
  }
  // the word and the record(s) are fetched together; the word decides whether the record exists for this ray
  __device__ __forceinline__ void record(const TraverseArgs<T> &a, Lane<T> &L, uint32_t rid, uint32_t k) {
    uint32_t word = ~0u;
    if constexpr (MASKED) word = as_global(m.leaf_masks)[k];
    LeafTri<T> tri = a.tris[k];
    if constexpr (MOTION) {
      const LeafTri<T> k1 = m.tris1[k];
      tri = motion_record<T>(tri, k1, shutter);
    }
    const T B = L.hit_t;
    L.prim = kInvalid;
    tri_test<T>(L, tri, (word & ray_mask) != 0u, a.range0, a.range1, skip, a.cull_back_face != 0);
    kb.offer(m.mh, L, rid, B);
  }
  __device__ __forceinline__ void finish(const TraverseArgs<T> &, const Lane<T> &L, uint32_t rid) const { kb.fill(m.mh, L, rid); }
};

template <typename T, int STACK, bool MOTION, bool MASKED>
__global__ __launch_bounds__(kTraverseBlock) void k_multihit_query(const MultiHitQueryArgs<T> m) {
  // [depth][thread]: a wave's 64 lanes hit 64 consecutive dwords -> conflict-free.
  __shared__ uint32_t s_stack[STACK][kTraverseBlock];
  binary_walk<T, STACK>(m.mh.a, s_stack, MultiHitCombinedQuery<T, MOTION, MASKED>{{}, m, {}});
}

// The instantiation a launch with these features runs.
template <typename T>
static const void *multihit_query_kernel(bool motion, bool masked) {
  if (motion) return masked ? (const void *)k_multihit_query<T, kLdsStackDefault, true, true> : (const void *)k_multihit_query<T, kLdsStackDefault, true, false>;
  return masked ? (const void *)k_multihit_query<T, kLdsStackDefault, false, true> : (const void *)k_multihit_query<T, kLdsStackDefault, false, false>;
}

template <typename T>
hipError_t launch_multihit_query(const TraverseArgs<T> &args, uint32_t max_hits, uint32_t *counts, bool motion, bool masked, const void *tris1, const T *times,
                                 const uint32_t *leaf_masks, const uint32_t *ray_masks, unsigned grid, hipStream_t s) {
  if (motion && !tris1) return hipErrorInvalidValue;
  if (masked && !leaf_masks) return hipErrorInvalidValue;
  MultiHitQueryArgs<T> m;
  m.mh.a = args;
  m.mh.max_hits = max_hits;
  m.mh.counts = counts;
  m.tris1 = motion ? (const LeafTri<T> *)tris1 : nullptr;
  m.times = motion ? times : nullptr;
  m.leaf_masks = masked ? leaf_masks : nullptr;
  m.ray_masks = masked ? ray_masks : nullptr;
  launch_persistent(multihit_query_kernel<T>(motion, masked), grid, m, s);
  return hipGetLastError();
}

template <typename T>
int multihit_query_blocks_per_cu(bool motion, bool masked) {
  return resident_blocks(multihit_query_kernel<T>(motion, masked), 1);
}

NRT_INSTANTIATE_F32_F64(launch_multihit_query)
NRT_INSTANTIATE_F32_F64(multihit_query_blocks_per_cu)

} // namespace nrt
