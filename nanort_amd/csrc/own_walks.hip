// nanort_amd/csrc/own_walks.hip — the triangle queries that run a binary walk of their own for gfx950: multi-hit, motion blur,
// visibility masks, and any of the three per-ray inputs (skip ids, shutter times, visibility words) on the same ray.
//
// The contracts are include/nanort_hip.h's; DESIGN.md says why each is built as it is (multi-hit §3.5, motion §3.9, masks §3.12,
// the combined query §3.13, multi-hit under it §3.16).  Every kernel here is binary_walk (binary_walk_dev.h) — the reference's loop
// over the context's node array (nanort.h:2487-2556), lane_init / slab_test / tri_test of traverse_dev.h unchanged — with ONE query,
// OwnQuery, whose four COMPILE-TIME choices say what the kernels do differently:
//   * MULTI: the K frontmost triangles of a ray instead of its closest.  The reference declares this walk (MultiHitTraverse,
//     nanort.h:761-770, 846-852, 2409-2485, 2694-2797) inside `#if 0`.  The bound B is ray.max_t while fewer than K hits are held,
//     else the t of the worst held hit, and lives in L.hit_t outside the triangle test; what tri_test accepts against B (entered with
//     L.prim = kInvalid) is offered to the K-buffer below; the finish is its miss fill and count.  B only ever prunes, so a ray's
//     result is the K smallest keys among the candidates of the leaves it reaches.  Not MULTI: closest hit, or occlusion when
//     a.any_hit — a ray is settled once hit_t < max_t (the predicate the finish writes as the flag), a settled lane tests no further
//     record; the finish is k_traverse's (store_closest_hit);
//   * IDS: the lane keeps a skip id of its own, skip_ids[rid] where the array is there, else the launch's skip_prim_id.  Not IDS: the
//     launch's, no register;
//   * MOTION: the lane keeps its ray's time (null times: 0; clamped, nanort_motion::ClampTime) and interpolates the records of
//     keyframe 0 (a.tris[k]) and keyframe 1 (tris1[k], the same leaf order) into the one tri_test sees (motion_record).  The boxes of
//     a motion context hold both keyframes (build.hip), so the walk reaches every leaf the triangle can be in at any time.  Not
//     MOTION: keyframe 1 is never fetched, no register;
//   * MASKED: the lane keeps its ray's word (null ray_masks: 0xFFFFFFFF); a triangle's word is read IN LEAF ORDER, leaf_masks[k]
//     beside a.tris[k], and its AND with the ray's is the `active` predicate of tri_test.  (Gathered through the record's prim_id the
//     word would be a second round trip behind the record's in every leaf step of a latency-bound chain; the leaf-order words come
//     from prims.hip's k_permute_masks.)  The boxes know nothing of the words.  Not MASKED: no word is fetched, no register.
// An invisible record, a record outside prim_ids_range and the skipped record take part in no reject and no accept, which is the
// reference's intersector returning false before it touches the ray's state.  The leaf step's loads — word, keyframe 0, keyframe 1 —
// are independent loads of one address computation, issued together.
// Which of the sixteen combinations exist, and under which kernel name, is the table at the end; which of them a launch runs is
// api_query.hip's (TraverseLaunch::own_walk_id).  None of these launches publishes a completion record: the slot is closed by an
// event (api_query.hip, enqueue_launch).
#include "binary_walk_dev.h"
#include "kernels.h"
#include "../../include/nanort_motion.h"

namespace nrt {

template <typename T>
struct MultiHitArgs {
  TraverseArgs<T> a;  // the closest-hit launch block (MULTI: a.hits = the rows of K records, a.mask unused; a.skip_ids: one id per ray, or null)
  uint32_t max_hits;  // MULTI: K, 1..NRT_MAX_MULTIHIT
  uint32_t *counts;   // MULTI: [num_rays] held hits per ray, may be null
};

template <typename T>
struct OwnWalkArgs {
  MultiHitArgs<T> mh;
  const LeafTri<T> *tris1;    // MOTION: the leaf records of keyframe 1, in the leaf order of mh.a.tris
  const T *times;             // MOTION: [num_rays] one time per ray, or null: every ray at time 0
  const uint32_t *leaf_masks; // MASKED: [num_indices] the triangles' words in leaf order, beside mh.a.tris
  const uint32_t *ray_masks;  // MASKED: [num_rays] one word per ray, or null: every ray 0xFFFFFFFF
};

// The leaf record a ray at shutter time `s` sees: nine interpolated components (nanort_motion::Lerp — THE rule, shared with the host
// intersector of include/nanort.h), the id of keyframe 0's record.
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

// ---- the K-buffer: the one device statement of the insertion, the eviction rule and the miss fill of the multi-hit contract ----
// Hits are ranked by (t, prim_id) ascending; a candidate enters when fewer than K are held or when its key is smaller than the worst
// held key, which is then evicted.  The held hits live SORTED in the ray's own output row (hits[ray * K + j]); registers hold only
// the count and the worst held prim_id (the worst t is B itself, kept in Lane::hit_t where the slab test reads it).  Insertions are
// rare next to node visits, so the row costs no LDS and no VGPRs for any K up to NRT_MAX_MULTIHIT.

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
  // L.v changed), if any, enters the row when its t is < ray.max_t (a NaN t never is); L.hit_t leaves as the new bound.
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

// ---- the query ------------------------------------------------------------------------------------------------------------------
template <typename T, bool MULTI, bool IDS, bool MOTION, bool MASKED>
struct OwnQuery : BinaryQuery {
  const OwnWalkArgs<T> &m;
  const bool any;           // not MULTI: an occlusion query (a.any_hit; wave-uniform)
  KBuffer<T> kb;            // MULTI
  T shutter = T(0);         // MOTION: the clamped time of the ray this lane holds
  uint32_t ray_mask = ~0u;  // MASKED: its word
  uint32_t skip = kInvalid; // IDS: its skip id

  __device__ __forceinline__ typename Wire<T>::Ray load(const TraverseArgs<T> &a, uint32_t rid) const {
    if constexpr (MULTI) return load_ray_nt<T>(a.rays + rid); // (deliberate: the comment above load_ray_nt)
    else return load_ray<T>(as_global(a.rays) + rid, 0u);     // (k_traverse's load without its probe bit: no profiling arm here)
  }
  __device__ __forceinline__ void begin(const TraverseArgs<T> &a, uint32_t rid) {
    if constexpr (MOTION) shutter = m.times != nullptr ? nanort_motion::ClampTime<T>(as_global(m.times)[rid]) : T(0);
    if constexpr (MASKED) ray_mask = m.ray_masks != nullptr ? as_global(m.ray_masks)[rid] : ~0u;
    if constexpr (IDS) skip = a.skip_ids != nullptr ? as_global(a.skip_ids)[rid] : a.skip_prim;
    if constexpr (MULTI) kb.reset();
  }
  __device__ __forceinline__ bool settled(const Lane<T> &L) const {
    if constexpr (MULTI) return false;
    else return any && L.hit_t < L.max_t;
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
    const bool active = MASKED ? (word & ray_mask) != 0u : true;
    const uint32_t skip_prim = IDS ? skip : a.skip_prim;
    if constexpr (MULTI) {
      const T B = L.hit_t;
      L.prim = kInvalid;
      tri_test<T>(L, tri, active, a.range0, a.range1, skip_prim, a.cull_back_face != 0); // accepted: L.prim, L.hit_t, L.u, L.v changed
      kb.offer(m.mh, L, rid, B);
    } else {
      tri_test<T>(L, tri, active, a.range0, a.range1, skip_prim, a.cull_back_face != 0);
    }
  }
  __device__ __forceinline__ void finish(const TraverseArgs<T> &a, const Lane<T> &L, uint32_t rid) const {
    if constexpr (MULTI) kb.fill(m.mh, L, rid);
    else store_closest_hit<T>(a, L, rid);
  }
};

template <typename T, int STACK, bool MULTI, bool IDS, bool MOTION, bool MASKED>
__device__ __forceinline__ void own_walk(const OwnWalkArgs<T> &m) {
  // [depth][thread]: a wave's 64 lanes hit 64 consecutive dwords -> conflict-free.
  __shared__ uint32_t s_stack[STACK][kTraverseBlock];
  binary_walk<T, STACK>(m.mh.a, s_stack, OwnQuery<T, MULTI, IDS, MOTION, MASKED>{{}, m, m.mh.a.any_hit != 0, {}});
}

// ---- the kernels: the names rocprofv3 and nrtLastKernelName show, each one form of the query --------------------------------------
template <typename T, int STACK>
__global__ __launch_bounds__(kTraverseBlock) void k_traverse_multihit(const OwnWalkArgs<T> m) {
  own_walk<T, STACK, true, false, false, false>(m);
}
template <typename T, int STACK>
__global__ __launch_bounds__(kTraverseBlock) void k_traverse_motion(const OwnWalkArgs<T> m) {
  own_walk<T, STACK, false, false, true, false>(m);
}
template <typename T, int STACK>
__global__ __launch_bounds__(kTraverseBlock) void k_traverse_masked(const OwnWalkArgs<T> m) {
  own_walk<T, STACK, false, false, false, true>(m);
}
template <typename T, int STACK, bool MOTION, bool MASKED> // (with or without ids; <false, false> does not exist: ids alone is k_traverse's or the wide walk's)
__global__ __launch_bounds__(kTraverseBlock) void k_traverse_query(const OwnWalkArgs<T> m) {
  own_walk<T, STACK, false, true, MOTION, MASKED>(m);
}
template <typename T, int STACK, bool MOTION, bool MASKED> // (<false, false>: ids alone, which no other multi-hit entry point can express)
__global__ __launch_bounds__(kTraverseBlock) void k_multihit_query(const OwnWalkArgs<T> m) {
  own_walk<T, STACK, true, true, MOTION, MASKED>(m);
}

// One row per own walk: what it reads besides the launch block, its kernel and its name as rocprofv3 prints it without the argument
// list, per precision ([0] fp32, [1] fp64).
struct OwnWalkRow {
  OwnWalk id;
  bool motion, masked;
  const void *kernel[2];
  const char *name[2];
};
static_assert(kLdsStackDefault == 32, "the names below carry the stack depth");
#define NRT_OWN_KERNELS(k, ...) {(const void *)k<float, kLdsStackDefault, ##__VA_ARGS__>, (const void *)k<double, kLdsStackDefault, ##__VA_ARGS__>}
static const OwnWalkRow kOwnWalks[kNumOwnWalks] = {
    {kOwnMultiHit, false, false, NRT_OWN_KERNELS(k_traverse_multihit), {"nrt::k_traverse_multihit<float>", "nrt::k_traverse_multihit<double>"}},
    {kOwnMotion, true, false, NRT_OWN_KERNELS(k_traverse_motion), {"nrt::k_traverse_motion<float>", "nrt::k_traverse_motion<double>"}},
    {kOwnMasked, false, true, NRT_OWN_KERNELS(k_traverse_masked), {"nrt::k_traverse_masked<float>", "nrt::k_traverse_masked<double>"}},
    {kOwnQueryMotion, true, false, NRT_OWN_KERNELS(k_traverse_query, true, false),
     {"nrt::k_traverse_query<float, 32, true, false>", "nrt::k_traverse_query<double, 32, true, false>"}},
    {kOwnQueryMasked, false, true, NRT_OWN_KERNELS(k_traverse_query, false, true),
     {"nrt::k_traverse_query<float, 32, false, true>", "nrt::k_traverse_query<double, 32, false, true>"}},
    {kOwnQueryMotionMasked, true, true, NRT_OWN_KERNELS(k_traverse_query, true, true),
     {"nrt::k_traverse_query<float, 32, true, true>", "nrt::k_traverse_query<double, 32, true, true>"}},
    {kOwnMultiHitIds, false, false, NRT_OWN_KERNELS(k_multihit_query, false, false),
     {"nrt::k_multihit_query<float, 32, false, false>", "nrt::k_multihit_query<double, 32, false, false>"}},
    {kOwnMultiHitMotion, true, false, NRT_OWN_KERNELS(k_multihit_query, true, false),
     {"nrt::k_multihit_query<float, 32, true, false>", "nrt::k_multihit_query<double, 32, true, false>"}},
    {kOwnMultiHitMasked, false, true, NRT_OWN_KERNELS(k_multihit_query, false, true),
     {"nrt::k_multihit_query<float, 32, false, true>", "nrt::k_multihit_query<double, 32, false, true>"}},
    {kOwnMultiHitMotionMasked, true, true, NRT_OWN_KERNELS(k_multihit_query, true, true),
     {"nrt::k_multihit_query<float, 32, true, true>", "nrt::k_multihit_query<double, 32, true, true>"}},
};
#undef NRT_OWN_KERNELS

static const OwnWalkRow *own_walk_row(OwnWalk w) {
  for (const OwnWalkRow &r : kOwnWalks)
    if (r.id == w) return &r;
  return nullptr;
}

template <typename T>
hipError_t launch_own_walk(OwnWalk w, const TraverseArgs<T> &args, const OwnWalkInputs<T> &in, unsigned grid, hipStream_t s, const char **name_out) {
  const OwnWalkRow *row = own_walk_row(w);
  if (!row || (row->motion && !in.tris1) || (row->masked && !in.leaf_masks)) return hipErrorInvalidValue;
  OwnWalkArgs<T> m;
  m.mh.a = args;
  m.mh.max_hits = in.max_hits;
  m.mh.counts = in.counts;
  m.tris1 = row->motion ? (const LeafTri<T> *)in.tris1 : nullptr; // (the arrays of a feature the walk has not are not read)
  m.times = row->motion ? in.times : nullptr;
  m.leaf_masks = row->masked ? in.leaf_masks : nullptr;
  m.ray_masks = row->masked ? in.ray_masks : nullptr;
  launch_persistent(row->kernel[sizeof(T) == 4 ? 0 : 1], grid, m, s);
  if (name_out) *name_out = row->name[sizeof(T) == 4 ? 0 : 1];
  return hipGetLastError();
}

template <typename T>
int own_walk_blocks_per_cu(OwnWalk w) {
  const OwnWalkRow *row = own_walk_row(w);
  return row ? resident_blocks(row->kernel[sizeof(T) == 4 ? 0 : 1], 1) : 1;
}

NRT_INSTANTIATE_F32_F64(launch_own_walk)
NRT_INSTANTIATE_F32_F64(own_walk_blocks_per_cu)

} // namespace nrt
