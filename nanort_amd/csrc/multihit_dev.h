// nanort_amd/csrc/multihit_dev.h — the K-buffer of the multi-hit walks: the one device statement of the insertion, the eviction rule
// and the miss fill of include/nanort_hip.h's multi-hit contract (items 2-4), which k_traverse_multihit (multihit.hip) and
// k_multihit_query (multihit_query.hip) share.
//
// The held hits live SORTED in the ray's own output row (hits[ray * K + j]); registers hold only the count and the worst held prim_id
// (the worst t is B itself, kept in Lane::hit_t where the slab test reads it).  Insertions are rare next to node visits, so the row
// costs no LDS and no VGPRs for any K up to NRT_MAX_MULTIHIT.
#pragma once

#include "binary_walk_dev.h"

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

template <typename T>
struct KBuffer {
  typedef typename Wire<T>::Hit Hit;
  uint32_t held = 0;              // hits held in the ray's row
  uint32_t worst_prim = kInvalid; // prim_id of the worst held hit (row[held - 1]) once K are held

  __device__ __forceinline__ void reset() { // (lane_init: L.hit_t = ray.max_t == B with no hit held)
    held = 0;
    worst_prim = kInvalid;
  }
  // Behind a tri_test against L.hit_t == B that was entered with L.prim = kInvalid: the primitive it accepted (L.prim, L.hit_t, L.u,
  // L.v changed), if any, enters the row; L.hit_t leaves as the new bound.
  __device__ __forceinline__ void offer(const MultiHitArgs<T> &m, Lane<T> &L, uint32_t rid, T B) {
    const uint32_t K = m.max_hits;
    const T tt = L.hit_t;
    // (accepted means !(tt > B): with K held, tt < B or a tie on t, which the prim_id decides)
    const bool enter = L.prim != kInvalid && tt < L.max_t && (held < K || tt < B || L.prim < worst_prim);
    T nb = B;
    if (enter) {
      Hit *row = m.a.hits + (size_t)rid * K;
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
  __device__ __forceinline__ void fill(const MultiHitArgs<T> &m, const Lane<T> &L, uint32_t rid) const {
    const uint32_t K = m.max_hits;
    Hit *row = m.a.hits + (size_t)rid * K;
    Hit miss;
    miss.u = T(0);
    miss.v = T(0);
    miss.t = L.max_t;
    miss.prim_id = kInvalid;
    for (uint32_t j = held; j < K; j++) row[j] = miss;
    if (m.counts) m.counts[rid] = held;
  }
};

} // namespace nrt
