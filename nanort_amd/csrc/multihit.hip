// nanort_amd/csrc/multihit.hip — multi-hit traversal for gfx950: the K frontmost triangles of every ray.
//
// The reference declares BVHAccel::MultiHitTraverse / MultiHitTestLeafNode (nanort.h:761-770, 846-852, 2409-2485,
// 2694-2797) but keeps them inside `#if 0`; this is the walk they describe, with the contract of include/nanort_hip.h
// (nrtMultiHitTraverseBatch*):
//   * the reference's binary loop over the node array (nanort.h:2487-2556): pop, slab test on [ray.min_t, B], near child
//     first by dir_sign[axis] — literally k_traverse (traverse.hip) with another leaf step and another finish;
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
#include "kernels.h"
#include "traverse_dev.h"

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

template <typename T, int STACK>
__global__ __launch_bounds__(kTraverseBlock) void k_traverse_multihit(const MultiHitArgs<T> m) {
  // [depth][thread]: a wave's 64 lanes hit 64 consecutive dwords -> conflict-free.
  __shared__ uint32_t s_stack[STACK][kTraverseBlock];

  typedef typename Wire<T>::Ray Ray;
  typedef typename Wire<T>::Hit Hit;
  const TraverseArgs<T> &a = m.a;
  const uint32_t K = m.max_hits;

  const unsigned tid = threadIdx.x;
  const unsigned lane = lane_id();
  const unsigned gslot = blockIdx.x * kTraverseBlock + tid;
  const bool cull = a.cull_back_face != 0;
  const LaneStack<StackRef, STACK, TraverseArgs<T>> stk = {a, tid, gslot};

  Lane<T> L; // L.hit_t == B outside the triangle test
  uint32_t rid = kInvalid;
  uint32_t cur = 0;
  uint32_t leaf_first = 0, leaf_cnt = 0;
  uint32_t held = 0;              // hits held in the ray's row
  uint32_t worst_prim = kInvalid; // prim_id of the worst held hit (row[held - 1]) once K are held
  int state = LANE_IDLE;
  int sp = 0;

  Claim ck;
  claim_init<T>(a, ck);
  if (blockIdx.x == 0 && threadIdx.x < kMaxParts) a.next_cursor[kCursorStrideWords * threadIdx.x] = 0u;

  // Pop the next node, or finish the ray when the stack is empty: the unused slots of its row get the miss record
  // {0, 0, ray.max_t, 0xFFFFFFFF} and the count is written.
#define NRT_MH_POP_OR_FINISH()                                                                    \
  do {                                                                                            \
    const bool fin_ = (sp == 0);                                                                  \
    if (fin_) {                                                                                   \
      Hit *row_ = a.hits + (size_t)rid * K;                                                       \
      Hit miss_;                                                                                  \
      miss_.u = T(0);                                                                             \
      miss_.v = T(0);                                                                             \
      miss_.t = L.max_t;                                                                          \
      miss_.prim_id = kInvalid;                                                                   \
      for (uint32_t j_ = held; j_ < K; j_++) row_[j_] = miss_;                                    \
      if (m.counts) m.counts[rid] = held;                                                         \
    }                                                                                             \
    if (!fin_) stk.load(s_stack, sp - 1, cur);                                                    \
    sp = fin_ ? sp : sp - 1;                                                                      \
    rid = fin_ ? kInvalid : rid;                                                                  \
    state = fin_ ? LANE_IDLE : LANE_TRAV;                                                         \
  } while (0)

  for (;;) {
    // ---- hand new rays to idle lanes (ballot rank inside the wave's chunk): k_traverse's refill ----
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
          const Ray r = load_ray_nt<T>(a.rays + rid);
          lane_init<T>(L, r); // (L.hit_t = ray.max_t == B with no hit held)
          held = 0;
          worst_prim = kInvalid;
          cur = 0;
          sp = 0;
          state = LANE_TRAV;
        }
        ck.next += take;
        idle = __ballot(state == LANE_IDLE);
      }
    }
    if (idle == ~0ull) {
      if (ck.exhausted) break;
      continue;
    }

    // ---- phase 1: inner nodes, until this lane reaches a leaf or finishes (k_traverse's loop, bound B) ----
    while (state == LANE_TRAV) {
      const typename Wire<T>::Node nd = a.nodes[cur];
      if (slab_test<T>(L, nd.bmin, nd.bmax)) {
        if (nd.flag == 0) {
          const int near = L.sign(nd.axis);
          const uint32_t far_child = near ? nd.data[0] : nd.data[1];
          cur = near ? nd.data[1] : nd.data[0];
          stk.store(s_stack, sp, far_child);
          sp++;
        } else {
          leaf_cnt = nd.data[0];
          leaf_first = nd.data[1];
          state = LANE_LEAF;
        }
      } else {
        NRT_MH_POP_OR_FINISH();
      }
      if ((unsigned)__builtin_popcountll(__ballot(state == LANE_TRAV)) < a.trav_min) break;
    }

    // ---- phase 2: lanes holding a leaf test its triangles together; candidates enter the row ----
    if (__ballot(state == LANE_LEAF) != 0ull) {
      const uint32_t cnt = state == LANE_LEAF ? leaf_cnt : 0u;
      for (uint32_t i = 0; __ballot(i < cnt) != 0ull; i++) {
        if (i < cnt) {
          const LeafTri<T> tri = a.tris[leaf_first + i];
          const T B = L.hit_t;
          L.prim = kInvalid;
          tri_test<T>(L, tri, true, a.range0, a.range1, a.skip_prim, cull); // accepted: L.prim, L.hit_t, L.u, L.v changed
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
      }
      if (state == LANE_LEAF) NRT_MH_POP_OR_FINISH();
    }
  }
#undef NRT_MH_POP_OR_FINISH
}

template <typename T, int STACK>
static hipError_t launch_multihit_s(const MultiHitArgs<T> &m, unsigned grid, hipStream_t s) {
  hipLaunchKernelGGL((k_traverse_multihit<T, STACK>), dim3(grid), dim3(kTraverseBlock), 0, s, m);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_traverse_multihit(const TraverseArgs<T> &args, uint32_t max_hits, uint32_t *counts, unsigned grid, hipStream_t s) {
  MultiHitArgs<T> m;
  m.a = args;
  m.max_hits = max_hits;
  m.counts = counts;
  return launch_multihit_s<T, kLdsStackDefault>(m, grid, s);
}

template <typename T>
int traverse_multihit_blocks_per_cu() {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_traverse_multihit<T, kLdsStackDefault>, kTraverseBlock, 0) != hipSuccess || n < 1)
    n = 1;
  return n;
}

NRT_INSTANTIATE_F32_F64(launch_traverse_multihit)
NRT_INSTANTIATE_F32_F64(traverse_multihit_blocks_per_cu)

} // namespace nrt
