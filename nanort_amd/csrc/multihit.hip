// nanort_amd/csrc/multihit.hip — multi-hit traversal for gfx950: the K frontmost triangles of every ray.
//
// The reference declares BVHAccel::MultiHitTraverse / MultiHitTestLeafNode (nanort.h:761-770, 846-852, 2409-2485,
// 2694-2797) but keeps them inside `#if 0`; this is the walk they describe, with the contract of include/nanort_hip.h
// (nrtMultiHitTraverseBatch*):
//   * the reference's binary loop over the node array (nanort.h:2487-2556): pop, slab test on [ray.min_t, B], near child
//     first by dir_sign[axis] — binary_walk (binary_walk_dev.h), the loop k_traverse runs, with the query below: another leaf
//     step and another finish;
//   * B = ray.max_t while fewer than K hits are held, else the t of the worst held hit;
//   * a primitive is a candidate when TriangleIntersector::Intersect accepts it against B (tri_test, unchanged) and its
//     t is < ray.max_t (a NaN t never is);
//   * hits are ranked by (t, prim_id) ascending; a candidate enters when fewer than K are held or when its key is smaller
//     than the worst held key, which is then evicted.
// The bound only ever prunes, so a ray's result is the K smallest keys among the candidates of the leaves it reaches.
//
// K-buffer: multihit_dev.h (the held hits live sorted in the ray's own output row; registers hold the count and the worst held
// prim_id), which the kernel shares with k_multihit_query (multihit_query.hip); the kernel keeps k_traverse's register budget.
#include "kernels.h"
#include "multihit_dev.h"

namespace nrt {

// The multi-hit query of the binary walk.  L.hit_t == B outside the triangle test.
template <typename T>
struct MultiHitQuery : BinaryQuery {
  const MultiHitArgs<T> &m;
  KBuffer<T> kb;

  __device__ __forceinline__ typename Wire<T>::Ray load(const TraverseArgs<T> &a, uint32_t rid) const {
    return load_ray_nt<T>(a.rays + rid); // (deliberate: the comment above load_ray_nt)
  }
  __device__ __forceinline__ void begin(const TraverseArgs<T> &, uint32_t) { kb.reset(); }
  // a candidate enters the row
  __device__ __forceinline__ void record(const TraverseArgs<T> &a, Lane<T> &L, uint32_t rid, uint32_t k) {
    const LeafTri<T> tri = a.tris[k];
    const T B = L.hit_t;
    L.prim = kInvalid;
    tri_test<T>(L, tri, true, a.range0, a.range1, a.skip_prim, a.cull_back_face != 0); // accepted: L.prim, L.hit_t, L.u, L.v changed
    kb.offer(m, L, rid, B);
  }
  __device__ __forceinline__ void finish(const TraverseArgs<T> &, const Lane<T> &L, uint32_t rid) const { kb.fill(m, L, rid); }
};

template <typename T, int STACK>
__global__ __launch_bounds__(kTraverseBlock) void k_traverse_multihit(const MultiHitArgs<T> m) {
  // [depth][thread]: a wave's 64 lanes hit 64 consecutive dwords -> conflict-free.
  __shared__ uint32_t s_stack[STACK][kTraverseBlock];
  binary_walk<T, STACK>(m.a, s_stack, MultiHitQuery<T>{{}, m, {}});
}

template <typename T>
hipError_t launch_traverse_multihit(const TraverseArgs<T> &args, uint32_t max_hits, uint32_t *counts, unsigned grid, hipStream_t s) {
  MultiHitArgs<T> m;
  m.a = args;
  m.max_hits = max_hits;
  m.counts = counts;
  launch_persistent((const void *)k_traverse_multihit<T, kLdsStackDefault>, grid, m, s);
  return hipGetLastError();
}

template <typename T>
int traverse_multihit_blocks_per_cu() {
  return resident_blocks((const void *)k_traverse_multihit<T, kLdsStackDefault>, 1);
}

NRT_INSTANTIATE_F32_F64(launch_traverse_multihit)
NRT_INSTANTIATE_F32_F64(traverse_multihit_blocks_per_cu)

} // namespace nrt
