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
// K-buffer: the held hits live SORTED in the ray's own output row (hits[ray * K + j]); registers hold only the count and
// the worst held prim_id (the worst t is B itself, kept in Lane::hit_t where the slab test reads it).  Insertions are rare
// next to node visits, so the row costs no LDS and no VGPRs for any K up to NRT_MAX_MULTIHIT, and the kernel keeps
// k_traverse's register budget.
#include "binary_walk_dev.h"
#include "kernels.h"

namespace nrt {

template <typename T>
struct MultiHitArgs {
  TraverseArgs<T> a;  // the closest-hit launch block (a.hits = the rows of K records, a.mask unused)
  uint32_t max_hits;  // K, 1..NRT_MAX_MULTIHIT
  uint32_t *counts;   // [num_rays] held hits per ray, may be null
};

// (t, prim) > (bt, bp) in the contract's order: t numerically (-0 == +0), then prim_id
template <typename T>
__device__ __forceinline__ bool key_greater(T t, uint32_t p, T bt, uint32_t bp) {
  return t > bt || (t == bt && p > bp);
}

// The multi-hit query of the binary walk.  L.hit_t == B outside the triangle test.
template <typename T>
struct MultiHitQuery : BinaryQuery {
  typedef typename Wire<T>::Hit Hit;
  const MultiHitArgs<T> &m;
  uint32_t held = 0;              // hits held in the ray's row
  uint32_t worst_prim = kInvalid; // prim_id of the worst held hit (row[held - 1]) once K are held

  __device__ __forceinline__ typename Wire<T>::Ray load(const TraverseArgs<T> &a, uint32_t rid) const {
    return load_ray_nt<T>(a.rays + rid); // (deliberate: the comment above load_ray_nt)
  }
  __device__ __forceinline__ void begin(const TraverseArgs<T> &, uint32_t) { // (lane_init: L.hit_t = ray.max_t == B with no hit held)
    held = 0;
    worst_prim = kInvalid;
  }
  // a candidate enters the row
  __device__ __forceinline__ void record(const TraverseArgs<T> &a, Lane<T> &L, uint32_t rid, uint32_t k) {
    const uint32_t K = m.max_hits;
    const LeafTri<T> tri = a.tris[k];
    const T B = L.hit_t;
    L.prim = kInvalid;
    tri_test<T>(L, tri, true, a.range0, a.range1, a.skip_prim, a.cull_back_face != 0); // accepted: L.prim, L.hit_t, L.u, L.v changed
    const T tt = L.hit_t;
    // (accepted means !(tt > B): with K held, tt < B or a tie on t, which the prim_id decides)
    const bool enter = L.prim != kInvalid && tt < L.max_t && (held < K || tt < B || L.prim < worst_prim);
    T nb = B;
    if (enter) {
      Hit *row = a.hits + (size_t)rid * K;
      uint32_t j = held < K ? held : K - 1u; // the slot the shift starts from (the worst is dropped when full)
      while (j > 0u) {
        const Hit prev = row[j - 1u];
        if (!key_greater<T>(prev.t, prev.prim_id, tt, L.prim)) break;
        row[j] = prev;
        j--;
      }
      Hit h;
      h.u = L.u;
      h.v = L.v;
      h.t = tt;
      h.prim_id = L.prim;
      row[j] = h;
      held = held < K ? held + 1u : K;
      if (held == K) {
        const Hit w = row[K - 1u];
        nb = w.t;
        worst_prim = w.prim_id;
      }
    }
    L.hit_t = nb;
  }
  // the unused slots of the ray's row get the miss record {0, 0, ray.max_t, 0xFFFFFFFF} and the count is written
  __device__ __forceinline__ void finish(const TraverseArgs<T> &a, const Lane<T> &L, uint32_t rid) const {
    const uint32_t K = m.max_hits;
    Hit *row = a.hits + (size_t)rid * K;
    Hit miss;
    miss.u = T(0);
    miss.v = T(0);
    miss.t = L.max_t;
    miss.prim_id = kInvalid;
    for (uint32_t j = held; j < K; j++) row[j] = miss;
    if (m.counts) m.counts[rid] = held;
  }
};

template <typename T, int STACK>
__global__ __launch_bounds__(kTraverseBlock) void k_traverse_multihit(const MultiHitArgs<T> m) {
  // [depth][thread]: a wave's 64 lanes hit 64 consecutive dwords -> conflict-free.
  __shared__ uint32_t s_stack[STACK][kTraverseBlock];
  binary_walk<T, STACK>(m.a, s_stack, MultiHitQuery<T>{{}, m});
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
