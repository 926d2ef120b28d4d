// nanort_amd/csrc/binary_walk_dev.h — THE one statement of the reference's binary while-while loop (BVHAccel::Traverse,
// nanort.h:2487-2556) as a persistent-threads walk: one ray per lane, rays claimed in chunks and handed to idle lanes by ballot rank,
// inner nodes until a lane reaches a leaf, the leaves of the whole wave together, then pop or finish.  k_traverse (traverse.hip)
// runs it, and the five kernels of own_walks.hip (k_traverse_multihit, k_traverse_motion, k_traverse_masked, k_traverse_query,
// k_multihit_query) — each with its own __shared__ stack array and a QUERY: a compile-time type that says what the kernels do
// differently, and nothing else.
//
// A query Q derives from BinaryQuery and states (every member __forceinline__; `a` is the launch block, `L` the lane's ray):
//   Ray  load(a, rid)                       the ray a lane takes at a refill
//   void begin(a, rid)                      its own per-ray state, reset at a refill
//   void enter_leaves(a, rid, at_leaf)      the wave is about to take its leaves, converged; at_leaf: this lane holds one
//                                           (BinaryQuery: nothing)
//   void record(a, L, rid, k)               leaf record k against the lane's ray: the fetch and the test
//   bool settled(L)                         the ray needs no further record and no further node (BinaryQuery: never)
//   void finish(a, L, rid)                  the ray's result leaves the lane
//   void node() / pushed(sp) / leaf()       per inner node fetched / push / leaf entered (BinaryQuery: nothing — the counting pass)
//   void after(a, lane)                     the wave has left the loop (BinaryQuery: nothing — the counting pass)
// How the pieces are cut follows the compiler's register allocation, read per form from its resource remarks: the
// leaf loop stands in the walk, not in a member (as a member it cost k_traverse four to nine registers, a wave per SIMD at two of
// its stack depths); the walk takes its query by value (by reference: three registers more in the fp64 counting pass, a wave).
#pragma once

#include "traverse_dev.h"

namespace nrt {

struct BinaryQuery {
  __device__ __forceinline__ void node() {}
  __device__ __forceinline__ void pushed(int) {}
  __device__ __forceinline__ void leaf() {}
  template <typename A>
  __device__ __forceinline__ void enter_leaves(const A &, uint32_t, bool) {}
  template <typename A>
  __device__ __forceinline__ void after(const A &, unsigned) {}
  template <typename T>
  __device__ __forceinline__ bool settled(const Lane<T> &) const {
    return false;
  }
};

// The closest-hit finish: PostTraversal (nanort.h:1205-1211) with the strict final predicate (:2552).
template <typename T>
__device__ __forceinline__ void store_closest_hit(const TraverseArgs<T> &a, const Lane<T> &L, uint32_t rid) {
  const bool hit = L.hit_t < L.max_t;
  if (a.hits) {
    typename Wire<T>::Hit h;
    h.u = hit ? L.u : T(0);
    h.v = hit ? L.v : T(0);
    h.t = hit ? L.hit_t : L.max_t;
    h.prim_id = hit ? L.prim : kInvalid;
    store_hit_nt<T>(a.hits + rid, h);
  }
  if (a.mask) a.mask[rid] = hit ? 1 : 0;
}

// (The block's LDS array is an argument, not a member of anything: LaneStack's comment in traverse_dev.h says why.)
template <typename T, int STACK, typename Q>
__device__ __forceinline__ void binary_walk(const TraverseArgs<T> &a, uint32_t (&s_stack)[STACK][kTraverseBlock], Q q) {
  typedef typename Wire<T>::Node Node;
  typedef typename Wire<T>::Ray Ray;

  const unsigned tid = threadIdx.x;
  const unsigned lane = lane_id();
  const LaneStack<StackRef, STACK, TraverseArgs<T>> stk = {a, tid, blockIdx.x * kTraverseBlock + tid};

  Lane<T> L;
  uint32_t rid = kInvalid; // ray this lane is working on
  uint32_t cur = 0;        // node to visit next (LANE_TRAV)
  uint32_t leaf_first = 0, leaf_cnt = 0; // pending leaf (LANE_LEAF)
  int state = LANE_IDLE;
  int sp = 0; // entries on this lane's stack

  Claim ck; // wave-uniform claimed range
  claim_init<T>(a, ck);
  if (blockIdx.x == 0 && threadIdx.x < kMaxParts) a.next_cursor[kCursorStrideWords * threadIdx.x] = 0u;

  // Pop the next node, or finish the ray when the stack is empty (`done_`: or when the query has settled it).  Select-style updates:
  // every state variable is assigned on both paths, which keeps them all in registers.  (A macro of one flag, local to this
  // function: as a function over references to the lane state, or as a lambda, the same lines compile to branch-local updates of
  // `sp` with copies behind them instead of one saturating subtract, and k_traverse_motion measured 1 % slower: DESIGN.md 3.10.)
#define NRT_POP_OR_FINISH(done_)                  \
  do {                                            \
    const bool fin_ = (sp == 0) | (done_);        \
    if (fin_) q.finish(a, L, rid);                \
    if (!fin_) stk.load(s_stack, sp - 1, cur);    \
    sp = fin_ ? 0 : sp - 1;                       \
    rid = fin_ ? kInvalid : rid;                  \
    state = fin_ ? LANE_IDLE : LANE_TRAV;         \
  } while (0)

  for (;;) {
    // ---- hand new rays to idle lanes (ballot rank inside the wave's chunk) ----
    unsigned long long idle = __ballot(state == LANE_IDLE);
    if (!ck.exhausted && (unsigned)__builtin_popcountll(idle) >= a.refill_min) {
      while (idle != 0ull && !ck.exhausted) {
        if (ck.next == ck.end && !claim_chunk<T>(a, ck, lane, __builtin_ctzll(idle))) break;
        const unsigned want = (unsigned)__builtin_popcountll(idle);
        const unsigned avail = ck.end - ck.next;
        const unsigned take = want < avail ? want : avail;
        const unsigned rank = (unsigned)__builtin_popcountll(idle & ((1ull << lane) - 1ull));
        if (state == LANE_IDLE && rank < take) {
          rid = ck.next + rank;
          const Ray r = q.load(a, rid);
          q.begin(a, rid);
          lane_init<T>(L, r);
          cur = 0;
          sp = 0;
          state = LANE_TRAV;
        }
        ck.next += take;
        idle = __ballot(state == LANE_IDLE);
      }
    }
    if (idle == ~0ull) {
      if (ck.exhausted) break; // nothing left anywhere in this wave
      continue;                // (cannot happen: refill_min <= 64)
    }

    // ---- phase 1: inner nodes, until this lane reaches a leaf or finishes -----------
    while (state == LANE_TRAV) {
      const Node nd = a.nodes[cur];
      q.node();
      if (slab_test<T>(L, nd.bmin, nd.bmax)) {
        if (nd.flag == 0) {
          const int near = L.sign(nd.axis);
          const uint32_t far_child = near ? nd.data[0] : nd.data[1];
          cur = near ? nd.data[1] : nd.data[0];
          // push far; near stays in `cur` (it would be popped next anyway: nanort.h:2542-2543)
          stk.store(s_stack, sp, far_child);
          sp++;
          q.pushed(sp);
        } else {
          leaf_cnt = nd.data[0];
          leaf_first = nd.data[1];
          state = LANE_LEAF;
          q.leaf();
        }
      } else {
        NRT_POP_OR_FINISH(false);
      }
      // leave early when too few lanes are still walking inner nodes
      if ((unsigned)__builtin_popcountll(__ballot(state == LANE_TRAV)) < a.trav_min) break;
    }

    // ---- phase 2: lanes holding a leaf take its records together --------------------
    if (__ballot(state == LANE_LEAF) != 0ull) {
      const uint32_t cnt = state == LANE_LEAF ? leaf_cnt : 0u;
      q.enter_leaves(a, rid, state == LANE_LEAF);
      for (uint32_t i = 0; __ballot(i < cnt && !q.settled(L)) != 0ull; i++) {
        if (i < cnt && !q.settled(L)) q.record(a, L, rid, leaf_first + i);
      }
      if (state == LANE_LEAF) NRT_POP_OR_FINISH(q.settled(L));
    }
  }
#undef NRT_POP_OR_FINISH
  q.after(a, lane);
}

} // namespace nrt
