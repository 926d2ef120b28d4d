// nanort_amd/csrc/motion.hip — motion-blur traversal for gfx950: every ray carries a shutter time, every triangle two keyframes.
//
// The contract is include/nanort_hip.h's (nrtTraverseBatchMotion* / nrtOccludedBatchMotion*):
//   * the reference's binary loop over the context's node array (nanort.h:2487-2556) — literally k_traverse (traverse.hip): the same
//     claim and refill, the same LaneStack with its global overflow, lane_init / slab_test / tri_test of traverse_dev.h unchanged.
//     The boxes of a motion context hold both keyframes (build.hip, k_prim_records<T, true>), so the walk reaches every leaf the
//     moving triangle can be in whatever the ray's time is;
//   * refill: the lane loads times[rid] with its ray, clamps it (nanort_motion::ClampTime) and keeps the shutter time in one register;
//   * leaf step: the record of keyframe 0 (a.tris[k]) and of keyframe 1 (tris1[k], the same leaf order) are interpolated component
//     by component (nanort_motion::Lerp — THE rule, shared with the host intersector of include/nanort.h) into one LeafTri, which
//     goes through tri_test exactly as k_traverse's leaf step hands it a stored record; prim_id is record 0's;
//   * occlusion (a.any_hit): a ray is settled once hit_t < max_t — the predicate the finish writes as the closest-hit flag; a
//     settled lane tests no further record and finishes its ray;
//   * finish: the record and mask stores of k_traverse.
// Like the multi-hit walk the launch publishes no completion record: its slot is closed by an event (api.hip, enqueue_launch).
#include "kernels.h"
#include "traverse_dev.h"
#include "../../include/nanort_motion.h"

namespace nrt {

template <typename T>
struct MotionArgs {
  TraverseArgs<T> a;       // the closest-hit launch block (a.tris: the leaf records of keyframe 0)
  const LeafTri<T> *tris1; // the leaf records of keyframe 1, in the same leaf order
  const T *times;          // [num_rays] one time per ray, or null: every ray at time 0
};

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

template <typename T, int STACK>
__global__ __launch_bounds__(kTraverseBlock) void k_traverse_motion(const MotionArgs<T> m) {
  // [depth][thread]: a wave's 64 lanes hit 64 consecutive dwords -> conflict-free.
  __shared__ uint32_t s_stack[STACK][kTraverseBlock];

  typedef typename Wire<T>::Ray Ray;
  typedef typename Wire<T>::Hit Hit;
  const TraverseArgs<T> &a = m.a;

  const unsigned tid = threadIdx.x;
  const unsigned lane = lane_id();
  const unsigned gslot = blockIdx.x * kTraverseBlock + tid;
  const bool cull = a.cull_back_face != 0;
  const bool any = a.any_hit != 0; // (wave-uniform)
  const LaneStack<StackRef, STACK, TraverseArgs<T>> stk = {a, tid, gslot};

  Lane<T> L;
  T shutter = T(0); // the clamped time of the ray this lane holds
  uint32_t rid = kInvalid;
  uint32_t cur = 0;
  uint32_t leaf_first = 0, leaf_cnt = 0;
  int state = LANE_IDLE;
  int sp = 0;

  Claim ck;
  claim_init<T>(a, ck);
  if (blockIdx.x == 0 && threadIdx.x < kMaxParts) a.next_cursor[kCursorStrideWords * threadIdx.x] = 0u;

  // Pop the next node, or finish the ray when the stack is empty (`done_`: or when an occlusion query has settled it): k_traverse's
  // finish — PostTraversal (nanort.h:1205-1211) with the strict final predicate (:2552).
#define NRT_MO_POP_OR_FINISH(done_)                                                      \
  do {                                                                                   \
    const bool fin_ = (sp == 0) | (done_);                                               \
    if (fin_) {                                                                          \
      const bool hit_ = L.hit_t < L.max_t;                                               \
      if (a.hits) {                                                                      \
        Hit h_;                                                                          \
        h_.u = hit_ ? L.u : T(0);                                                        \
        h_.v = hit_ ? L.v : T(0);                                                        \
        h_.t = hit_ ? L.hit_t : L.max_t;                                                 \
        h_.prim_id = hit_ ? L.prim : kInvalid;                                           \
        store_hit_nt<T>(a.hits + rid, h_);                                               \
      }                                                                                  \
      if (a.mask) a.mask[rid] = hit_ ? 1 : 0;                                            \
    }                                                                                    \
    if (!fin_) stk.load(s_stack, sp - 1, cur);                                           \
    sp = fin_ ? 0 : sp - 1;                                                              \
    rid = fin_ ? kInvalid : rid;                                                         \
    state = fin_ ? LANE_IDLE : LANE_TRAV;                                                \
  } while (0)

  for (;;) {
    // ---- hand new rays to idle lanes (ballot rank inside the wave's chunk): k_traverse's refill, + the ray's time ----
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
          const Ray r = load_ray<T>(as_global(a.rays) + rid, 0u);
          shutter = m.times != nullptr ? nanort_motion::ClampTime<T>(as_global(m.times)[rid]) : T(0);
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
      if (ck.exhausted) break;
      continue;
    }

    // ---- phase 1: inner nodes, until this lane reaches a leaf or finishes (k_traverse's loop) ----
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
        NRT_MO_POP_OR_FINISH(false);
      }
      if ((unsigned)__builtin_popcountll(__ballot(state == LANE_TRAV)) < a.trav_min) break;
    }

    // ---- phase 2: lanes holding a leaf interpolate its records to their own time and test them together ----
    if (__ballot(state == LANE_LEAF) != 0ull) {
      const uint32_t cnt = state == LANE_LEAF ? leaf_cnt : 0u;
      // (an occlusion query: `open` ends a lane's records at the first one that settles its ray)
      for (uint32_t i = 0; __ballot(i < cnt && !(any && L.hit_t < L.max_t)) != 0ull; i++) {
        if (i < cnt && !(any && L.hit_t < L.max_t)) {
          const LeafTri<T> k0 = a.tris[leaf_first + i];
          const LeafTri<T> k1 = m.tris1[leaf_first + i];
          const LeafTri<T> tri = motion_record<T>(k0, k1, shutter);
          tri_test<T>(L, tri, true, a.range0, a.range1, a.skip_prim, cull);
        }
      }
      if (state == LANE_LEAF) NRT_MO_POP_OR_FINISH(any && L.hit_t < L.max_t);
    }
  }
#undef NRT_MO_POP_OR_FINISH
}

template <typename T>
hipError_t launch_traverse_motion(const TraverseArgs<T> &args, const void *tris1, const T *times, unsigned grid, hipStream_t s) {
  MotionArgs<T> m;
  m.a = args;
  m.tris1 = (const LeafTri<T> *)tris1;
  m.times = times;
  hipLaunchKernelGGL((k_traverse_motion<T, kLdsStackDefault>), dim3(grid), dim3(kTraverseBlock), 0, s, m);
  return hipGetLastError();
}

template <typename T>
int traverse_motion_blocks_per_cu() {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_traverse_motion<T, kLdsStackDefault>, kTraverseBlock, 0) != hipSuccess || n < 1)
    n = 1;
  return n;
}

NRT_INSTANTIATE_F32_F64(launch_traverse_motion)
NRT_INSTANTIATE_F32_F64(traverse_motion_blocks_per_cu)

} // namespace nrt
