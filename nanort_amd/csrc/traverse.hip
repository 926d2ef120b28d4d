// nanort_amd/csrc/traverse.hip — batched closest-hit traversal of ONE tree for gfx950: the single-level walks (k_traverse, the
// closest-hit query of the binary loop that binary_walk_dev.h states; k_traverse_wide, the production kernel, and its variant
// table) and, at the end of the file, the conversion of a reference-format tree into the WideNode / Wide4Node records they step
// through (k_wide_count … k_make_wide).
//
// Replaces N calls of the reference's BVHAccel<T>::Traverse (nanort.h:2487-2556)
// with its TriangleIntersector (nanort.h:1014-1229) by one persistent-threads
// kernel: one ray per lane, per-lane stack in LDS (global spill beyond
// kLdsStack entries), rays claimed in chunks through one atomic per wave and
// handed to idle lanes by ballot rank.
//
// The arithmetic is the reference's, operation for operation (this file is
// compiled with -ffp-contract=off; IEEE division; denormals kept):
//   vsafe_inverse            nanort.h:442-461  (the `v < 0` sign rule)
//   IntersectRayAABB         nanort.h:2285-2370 (MaxMult 1.00000024f / 1.0000000000000004)
//   PrepareTraversal         nanort.h:1163-1201 (kz = argmax |dir|, strict <)
//   Intersect (watertight)   nanort.h:1054-1150 (fp64 edge fallback, tie rules)
//   Traverse / TestLeafNode  nanort.h:2526-2556, 2374-2407 (near child first,
//                            hit iff t_best < ray.max_t)
#include "binary_walk_dev.h"
#include "kernels.h"
#include "walk_dev.h"

#include <algorithm>

namespace nrt {

// The closest-hit query of the binary walk (binary_walk_dev.h).  COUNT: the counting pass — nodes fetched, leaves entered, records
// tested and the deepest stack the reference would have held, per launch.
template <typename T, bool COUNT>
struct ClosestQuery : BinaryQuery {
  unsigned long long c_nodes = 0, c_leaves = 0, c_tris = 0;
  unsigned c_stack = 0; // (a depth: 32 bits in the lane, widened for the atomic — the fp64 instantiation sits on the 96-register edge of five waves)
  uint32_t skip = 0; // the skip id of the leaves the wave is taking

  __device__ __forceinline__ typename Wire<T>::Ray load(const TraverseArgs<T> &a, uint32_t rid) const {
    return load_ray<T>(as_global(a.rays) + rid, a.debug_flags);
  }
  __device__ __forceinline__ void begin(const TraverseArgs<T> &, uint32_t) {
    if (COUNT) c_stack = c_stack > 1u ? c_stack : 1u;
  }
  __device__ __forceinline__ void node() {
    if (COUNT) c_nodes++;
  }
  __device__ __forceinline__ void pushed(int sp) {
    if (COUNT) {
      // the reference holds near+far on its stack at this point
      const unsigned need = (unsigned)sp + 1u;
      c_stack = need > c_stack ? need : c_stack;
    }
  }
  __device__ __forceinline__ void leaf() {
    if (COUNT) c_leaves++;
  }
  __device__ __forceinline__ void enter_leaves(const TraverseArgs<T> &a, uint32_t rid, bool at_leaf) {
    skip = a.skip_prim;
    if constexpr (!COUNT) // (the counting pass takes no ids: api_query.hip)
      if (a.skip_ids != nullptr && at_leaf) skip = a.skip_ids[rid]; // per-ray skip ids (common.h): the id of the ray the lane holds NOW
  }
  __device__ __forceinline__ void record(const TraverseArgs<T> &a, Lane<T> &L, uint32_t, uint32_t k) {
    const LeafTri<T> tri = a.tris[k];
    if (COUNT) c_tris++;
    tri_test<T>(L, tri, true, a.range0, a.range1, skip, a.cull_back_face != 0);
  }
  __device__ __forceinline__ void finish(const TraverseArgs<T> &a, const Lane<T> &L, uint32_t rid) const { store_closest_hit<T>(a, L, rid); }
  // wave reduction, then one atomic per wave per counter
  __device__ __forceinline__ void after(const TraverseArgs<T> &a, unsigned lane) {
    if (!COUNT) return;
    for (int off = 32; off > 0; off >>= 1) {
      c_nodes += __shfl_xor(c_nodes, off);
      c_leaves += __shfl_xor(c_leaves, off);
      c_tris += __shfl_xor(c_tris, off);
      const unsigned o = __shfl_xor(c_stack, off);
      c_stack = o > c_stack ? o : c_stack;
    }
    if (lane == 0) {
      atomicAdd(&a.counters[0], c_nodes);
      atomicAdd(&a.counters[1], c_leaves);
      atomicAdd(&a.counters[2], c_tris);
      atomicMax(&a.counters[3], (unsigned long long)c_stack);
    }
  }
};

template <typename T, bool COUNT, int STACK>
__global__ __launch_bounds__(kTraverseBlock) void k_traverse(const TraverseArgs<T> a) {
  // [depth][thread]: a wave's 64 lanes hit 64 consecutive dwords -> conflict-free.
  __shared__ uint32_t s_stack[STACK][kTraverseBlock];
  binary_walk<T, STACK>(a, s_stack, ClosestQuery<T, COUNT>());
}

// ---------------------------------------------------------------------------
// Production kernel: same traversal ORDER and same culling decisions as the
// binary loop of k_traverse (hence the same hit records, ties included), but each step
// fetches one WideNode and tests both children.  A child that passes its slab
// test is entered at once (near first) or pushed with its t_min; a popped entry
// is entered iff t_min <= hit_t, which is exactly the reference's test at pop
// time, because its slab test factors into (t_min <= t_max of the planes) — which
// does not depend on hit_t and was established at push time — and
// (t_min <= hit_t) (nanort.h:2315-2318: hit_t is the innermost operand of the
// safemin chain).
// ---------------------------------------------------------------------------
// PLAIN: the launch uses trace options that cannot reject a primitive (full prim_ids_range, no skip_prim_id, no
// back-face culling — the reference's defaults): the three id comparisons per triangle test are compiled out.
//
// (Round 2 also carried a SPLIT variant here — exact work splitting in the drain of a launch: a busy lane handed the oldest
// entry of its stack to an idle lane, results folded per ray by (smallest t, latest segment) — and a per-lane drain loop.
// Both were exact and soaked; both were measured to lose (the variant's bulk loop ran 9 % slower than production through
// register pressure and the extra checks, 13 % per step in all: profiles/r02c_split_*.txt, r03g_split_asis.txt) and were
// removed in round 3.  What a launch waits for at its end is the dependent chain of its few longest rays
// (tools/drain_probe.py, tools/tail_first_probe.py); DESIGN.md 3.1 and 10 keep the numbers.)
// (the box tests, stack entry and step macros of this walk, NRT_W4_FAST_PUSH among them: walk_dev.h)
#ifndef NRT_W4_P1_UNROLL
#define NRT_W4_P1_UNROLL 2 // fp32 two-level walk: pop + step rounds per trip of the inner-node loop
#endif
#ifndef NRT_W2_F64_P1_UNROLL
#define NRT_W2_F64_P1_UNROLL 2 // ... of the fp64 one-level walk
#endif
#ifndef NRT_W4_PRESEL
#define NRT_W4_PRESEL 1 // fp32 two-level walk: the near / far plane rows are fetched by the ray's signs (slab4_presel) instead of selected per value
#endif
#ifndef NRT_W2_F64_PRESEL
#define NRT_W2_F64_PRESEL 1 // fp64 one-level walk: the plane rows of both children are fetched by the ray's signs (slab_pair_presel)
#endif
#ifndef NRT_W4_TRI_UNROLL
#define NRT_W4_TRI_UNROLL 2 // triangle records fetched per trip of the leaf loop in the WIDTH = 4 variants (1 or 2)
#endif
#ifndef NRT_SPHERE_UNROLL
#define NRT_SPHERE_UNROLL 2 // sphere records fetched per trip of the leaf loop (sphere kind)
#endif
#ifndef NRT_W2_TRI_UNROLL
#define NRT_W2_TRI_UNROLL 2 // ... and in the one-level variants (fp32 and fp64)
#endif
#ifndef NRT_W4_WAVES
#define NRT_W4_WAVES 1 // minimum waves per SIMD asked of the WIDTH = 4 variants (1: whatever the register allocation gives)
#endif
// CLOCK: profiling instantiation that stamps when each wave starts, runs dry and finishes (tools/drain_probe.py).
// WIDTH: 2 = one WideNode (two boxes) per step, 4 = one Wide4Node (two levels, four boxes) per step.

// Quad helpers of the tail of a launch (k_traverse_wide, "four lanes to a ray"): the OR of a value over the four lanes of a quad,
// and lane K's value in all four (DPP quad permutes: no LDS, no memory).
__device__ __forceinline__ uint32_t quad_or(uint32_t x) {
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, true); // quad_perm [1,0,3,2]
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, true); // quad_perm [2,3,0,1]
  return x;
}
template <int K>
__device__ __forceinline__ float quad_bcast(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), K * 0x55, 0xF, 0xF, true));
}

// ORDER (WIDTH = 4 only), two bits: bit 0: 0 = the four slots in the binary loop's order (same leaf sequence as the reference), 1 = by
// entry distance.  Bit 1 (tunable leaf_compact): the LEAF PHASE hands the records of all the lanes waiting at a leaf out over the
// whole wave, one record per lane and trip (leaf_items_one_trip, walk_dev.h) — same tests on the same operands, accepted in the same order.
template <typename T, int STACK, bool STATS, int KIND, bool PLAIN = false, bool CLOCK = false, int WIDTH = 2, int ORDER = 0>
__global__ __launch_bounds__(kTraverseBlock, (WIDTH == 4 && sizeof(T) == 4) ? NRT_W4_WAVES : 1) void k_traverse_wide(const TraverseArgs<T> a) {
  static_assert(WIDTH == 2 || WIDTH == 4, "one or two tree levels per step");
  static_assert(KIND != kPrimCurves || sizeof(T) == 4, "curves are fp32 only, as their example");
  static_assert(ORDER == 0 || (WIDTH == 4 && sizeof(T) == 4), "distance order / leaf items are variants of the fp32 two-level step");
  static_assert((ORDER & 2) == 0 || (KIND == kPrimTriangles && !STATS), "leaf items: triangle records, production instantiations");
  static_assert((ORDER & 4) == 0 || ((ORDER & 1) == 0 && KIND == kPrimTriangles && !STATS && !CLOCK), "records addressed by 64-bit offsets: the default walk of triangle trees");
  constexpr bool LEAFC = (ORDER & 2) != 0;
  constexpr bool BIG = (ORDER & 4) != 0; // a Wide4Node array of 4 GiB or more (trees beyond ~110 M triangles): 64-bit record offsets
  typedef typename std::conditional<BIG, uint64_t, uint32_t>::type RecOff;
  // the tail of a launch four lanes to a ray (a.tail_lanes, below): the fp32 two-level triangle walk in the reference's order
  constexpr bool QUAD = WIDTH == 4 && sizeof(T) == 4 && KIND == kPrimTriangles && !STATS && (ORDER & 1) == 0 && !BIG;
  // leaf items (LEAFC): which lane owns the record a lane tests, and which of the owner's records it is (lane | k << 6)
  __shared__ uint32_t s_item_owner[LEAFC ? kTraverseBlock / kWave : 1][LEAFC ? kWave : 1];
  __shared__ uint32_t s_item_rec[LEAFC ? kTraverseBlock / kWave : 1][LEAFC ? kWave : 1]; // ... and which record of a.tris that is
  typedef StackEntry<T> SE;
  __shared__ typename SE::type s_stack[STACK][kTraverseBlock];

  typedef typename Wire<T>::Node Node;
  typedef typename Wire<T>::Ray Ray;
  typedef typename Wire<T>::Hit Hit;

  const unsigned tid = threadIdx.x;
  const unsigned lane = lane_id();
  const unsigned gslot = blockIdx.x * kTraverseBlock + tid;
  const bool cull = a.cull_back_face != 0;
  const LaneStack<SE, STACK, TraverseArgs<T>> stk = {a, tid, gslot};

  NRT_BATCH_TABLE_SETUP();
  Lane<T> L;
  uint32_t rid = kInvalid; // ray whose result this lane holds (W_IDLE with rid valid: finished, not yet written)
  uint32_t cur = 0;        // W_TRAV: WideNode index; W_LEAF: leaf reference without the leaf bit
  int state = W_IDLE;
  int sp = 0;
  // (profiling, NRT_DEBUG bit 8192: when did this wave start, run out of rays, finish — 100 MHz realtime ticks)
  const bool clocked = CLOCK && a.wave_clock != nullptr;
  unsigned long long clk_begin = 0ull, clk_dry = 0ull;
  unsigned long long clk_l16 = 0ull, clk_l8 = 0ull, clk_l4 = 0ull; // ... and, once it has, when its live lanes (state != idle) first numbered <= 16, 8, 4
  if (clocked) clk_begin = __builtin_amdgcn_s_memrealtime();
  // (live_: wave-uniform; looked at where the wave could switch to another way of walking: the top of the outer loop and the end
  // of every trip of the inner-node loop)
#define NRT_TAIL_N (a.tail_lanes < 16u ? a.tail_lanes : 16u) /* (16 quads to a wave) */
#define NRT_CLOCK_LIVE(live_)                                                  \
  do {                                                                         \
    if constexpr (CLOCK) {                                                     \
      if (clocked && ck.exhausted && clk_l4 == 0ull && (live_) <= 16u) {       \
        const unsigned long long now_ = __builtin_amdgcn_s_memrealtime();      \
        if (clk_l16 == 0ull) clk_l16 = now_;                                   \
        if (clk_l8 == 0ull && (live_) <= 8u) clk_l8 = now_;                    \
        if ((live_) <= 4u) clk_l4 = now_;                                      \
      }                                                                        \
    }                                                                          \
  } while (0)
  Claim ck;
  claim_init<T>(a, ck);
  // (an atomic store: performed at the memory side, so that the slot's next launch sees it wherever and whenever it runs)
  if (blockIdx.x == 0 && threadIdx.x < kMaxParts)
    __hip_atomic_store(a.next_cursor + kCursorStrideWords * threadIdx.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  done_begin<T>(a);
  // STATS (profiling instantiation only): wave-level loop occupancy
  unsigned long long st_it1 = 0, st_act1 = 0, st_idle2 = 0, st_it2 = 0, st_act2 = 0, st_refills = 0, st_refilled = 0, st_entries2 = 0;
  uint32_t st_steps = 0, st_tris = 0; // per ray; with debug flag 64 they replace u, v of the hit record
  // ... and where the wave's time goes (shader-clock ticks): refill (claim, result stores, ray loads, lane set-up), inner-node phase, leaf phase
  unsigned long long st_t_refill = 0, st_t_p1 = 0, st_t_p2 = 0, st_act2b = 0, st_stamp = 0;
  // ... and the same occupancy counts restricted to the STEADY part of the launch (rays still to be handed out), so that the
  // drain (every wave finishing what it holds) can be told from the steady state: counters[12..15]
  unsigned long long st_it1_s = 0, st_act1_s = 0, st_it2_s = 0, st_act2_s = 0;

  // PostTraversal (nanort.h:1205-1211) with the strict final predicate (:2552).  Finished lanes keep
  // their result in registers until the lane is refilled (or the wave runs out of rays), so the
  // stores are issued by many lanes at once instead of by the odd lane of every loop iteration.
#define NRT_WRITE_RESULT()                              \
  do {                                                  \
    const bool hit_ = L.hit_t < L.max_t;                \
    Hit h_;                                             \
    h_.u = hit_ ? L.u : T(0);                           \
    h_.v = hit_ ? L.v : T(0);                           \
    if (STATS && (a.debug_flags & 64u)) {               \
      h_.u = T(st_steps);                               \
      h_.v = T(st_tris);                                \
    }                                                   \
    h_.t = hit_ ? L.hit_t : L.max_t;                    \
    h_.prim_id = hit_ ? L.prim : kInvalid;              \
    Hit NRT_GLOBAL *hp_ = as_global(a.hits);            \
    uint8_t NRT_GLOBAL *mp_ = as_global(a.mask);        \
    if (multi) {                                        \
      const BatchPtrs bp_ = s_tbl[batch_of<T>(a, rid)]; \
      hp_ = as_global((Hit *)bp_.hits_v);               \
      mp_ = as_global(bp_.mask_v);                      \
    }                                                   \
    if (hp_) store_hit_nt<T>(hp_ + rid, h_);            \
    if (mp_) mp_[rid] = hit_ ? ((KIND == kPrimCylinders && !a.any_hit) ? (uint8_t)(1u | (L.cap << 1)) : (uint8_t)1) : (uint8_t)0; /* (an occlusion flag is 0 or 1: no cap bit) */ \
  } while (0)

  // The skip id of the ray a lane holds (`live_`: it holds one and waits at a leaf), into skip_: the launch's, or with per-ray skip
  // ids (common.h TraverseArgs::skip_ids; a multi-batch launch: its batch's array, or none) the ray's own, re-read at every leaf by the
  // index the lane keeps for its output — so whoever works on a ray (its lane after a refill, a quad of the tail) tests against ITS id.
#define NRT_RAY_SKIP(skip_, live_)                                                                     \
  uint32_t skip_ = a.skip_prim;                                                                        \
  if constexpr (!PLAIN && KIND == kPrimTriangles) {                                                    \
    const uint32_t NRT_GLOBAL *ids_ = as_global(a.skip_ids);                                           \
    if (multi) ids_ = as_global(s_tbl[batch_of<T>(a, rid)].skip_v);                                    \
    if ((live_) && ids_ != nullptr) skip_ = ids_[rid];                                                 \
  }                                                                                                    \
  (void)skip_

  // Occlusion queries of the sphere, cylinder and curve kinds (api_query.hip, Query::OcclusionPrims: a.any_hit on these instantiations,
  // flags into the caller's mask, no records).  A ray is SETTLED once `L.hit_t < L.max_t` — the very predicate NRT_WRITE_RESULT
  // writes as the closest-hit flag, and nothing weaker.  A settled lane tests no further record of its leaf (NRT_RAY_OPEN in the
  // record loops' `act_` and in their ballots: NRT_SPHERE_LOOP, NRT_RECORD_LOOP), a curve stops at its first accepted segment
  // (curve_test), and the exit behind the leaf phase drops the stack.  Why the flag is the closest-hit call's, exactly:
  //  * until a ray settles nothing here differs from the closest-hit walk: the bound of its box tests is still hit_t == max_t (or
  //    the NaN an acceptance left), so its pops, steps and leaf tests are the same, in the same order, on the same operands;
  //  * an acceptance that does not settle leaves the closest-hit flag 0 as well — a sphere accepted at t == max_t (`!(t > hit_t)`),
  //    an acceptance that leaves a NaN — and the ray walks on, as there;
  //  * a settled ray stays settled in the closest-hit walk: cylinders (`t <= tmax`, `pT < tmax`) and curves (`t < current`) accept
  //    only smaller, ordered distances, so hit_t < max_t is final the moment it holds.  Spheres accept `!(t > hit_t)`: the same,
  //    unless a LATER test yields a NaN distance (a NaN centre or radius, or an overflow inside the quadratic) — the closest-hit
  //    call then ends on whatever it accepts last, the occlusion call has answered 1.  Finite spheres under finite rays, and rays
  //    whose every test is NaN, agree exactly (include/nanort_hip.h says so);
  //  * a cylinder that its tree names once per segment (tunable cyl_split) is a pure function of (ray, cylinder, current t):
  //    skipping its repeats after the ray settled, or testing it again before, changes nothing.
  // Any-hit only REMOVES tests; those that run keep their order.  The record loops of these kinds stand twice in the code, behind
  // one wave-uniform branch (AH_ is the literal true or false): the closest-hit copy carries no trace of the predicate — measured
  // with it folded into one loop, the closest-hit calls of the sphere and curve kinds ran 1 - 3 % slower than before.
  const bool anyhit_ = KIND != kPrimTriangles && a.any_hit != 0u; // (wave-uniform)
#define NRT_RAY_OPEN(AH_) (!((AH_) && L.hit_t < L.max_t))

  // One primitive record (slot `slot_` of the leaf-ordered arrays) against a lane's ray; `act_` false -> no effect.
  // (`skip` is the leaf phase's: NRT_RAY_SKIP)
#define NRT_TEST_PRIM(slot_, act_, AH_)                                                                \
  do {                                                                                                 \
    if (KIND == kPrimSpheres) {                                                                        \
      const LeafSphere<T> sp_ = a.spheres[(slot_)];                                                    \
      sphere_test<T>(L, sp_, (act_), a.range0, a.range1);                                              \
    } else if (KIND == kPrimCylinders) {                                                               \
      const LeafCylinder<T> cy_ = a.cylinders[(slot_)];                                                \
      cylinder_test<T>(L, cy_, (act_), a.range0, a.range1, a.cyl_test_cap != 0u);                      \
    } else if constexpr (KIND == kPrimCurves) { /* (compile-time: no other instantiation sees it) */   \
      const LeafCurve cv_ = a.curves[(slot_)];                                                         \
      curve_test<T>(L, cv_, (act_), a.range0, a.range1, a.curve_subdiv, (AH_));                        \
    } else {                                                                                           \
      const LeafTri<T> tri_ = a.tris[(slot_)];                                                         \
      if (PLAIN)                                                                                       \
        tri_test<T, true>(L, tri_, (act_), 0u, 0u, 0u, false);                                         \
      else                                                                                             \
        tri_test<T>(L, tri_, (act_), a.range0, a.range1, skip, cull);                                  \
    }                                                                                                  \
  } while (0)

  // The record loops of a leaf for the sphere kind (NRT_SPHERE_UNROLL records fetched per trip, all before any is tested) and for
  // whatever has no loop of its own; AH_: the occlusion copy, which ends when no waiting lane has an unsettled record left.
#define NRT_SPHERE_LOOP(AH_)                                                                                              \
  for (uint32_t i = 0; __ballot(i < cnt && NRT_RAY_OPEN(AH_)) != 0ull; i += NRT_SPHERE_UNROLL) {                          \
    LeafSphere<T> s_[NRT_SPHERE_UNROLL];                                                                                  \
    _Pragma("unroll") for (uint32_t j = 0; j < NRT_SPHERE_UNROLL; j++) s_[j] = a.spheres[first + (i + j < cnt ? i + j : 0u)]; \
    _Pragma("unroll") for (uint32_t j = 0; j < NRT_SPHERE_UNROLL; j++)                                                    \
      sphere_test<T>(L, s_[j], i + j < cnt && NRT_RAY_OPEN(AH_), a.range0, a.range1);                                     \
  }
#define NRT_RECORD_LOOP(AH_)                                                                                              \
  for (uint32_t i = 0; __ballot(i < cnt && NRT_RAY_OPEN(AH_)) != 0ull; i++) {                                             \
    if (STATS) {                                                                                                          \
      st_it2++;                                                                                                           \
      st_act2 += (unsigned)__builtin_popcountll(__ballot(i < cnt));                                                       \
      if (i < cnt) st_tris++;                                                                                             \
    }                                                                                                                     \
    /* no divergent region here: lanes past their count re-test their first record with ok = false */                    \
    NRT_TEST_PRIM(first + (i < cnt ? i : 0u), i < cnt && NRT_RAY_OPEN(AH_), AH_);                                         \
  }

  // (QUAD: the wave leaves the loop for the tail below; which of its lanes were idle then)
  bool to_tail = false;
  unsigned long long tail_idle = 0ull;
  for (;;) {
    // ---- refill idle lanes ---------------------------------------------------------
    if (STATS) st_stamp = __builtin_amdgcn_s_memtime();
    unsigned long long idle = __ballot(state == W_IDLE);
    if (!ck.exhausted && (unsigned)__builtin_popcountll(idle) >= a.refill_min) {
      // lanes that still hold a result and lanes that never had a ray are both W_IDLE
      unsigned long long fresh = idle;
      while (fresh != 0ull && !ck.exhausted) {
        if (ck.next == ck.end && !claim_chunk<T>(a, ck, lane, __builtin_ctzll(fresh))) break;
        const unsigned want = (unsigned)__builtin_popcountll(fresh);
        const unsigned avail = ck.end - ck.next;
        const unsigned take = want < avail ? want : avail;
        const unsigned rank = (unsigned)__builtin_popcountll(fresh & ((1ull << lane) - 1ull));
        if (state == W_IDLE && rank < take) {
          if (rid != kInvalid) NRT_WRITE_RESULT();
          rid = ck.next + rank;
          const Ray NRT_GLOBAL *rp_ = as_global(a.rays);
          uint32_t bq_ = 0u; // this ray belongs to an occlusion-query batch
          if (multi) {
            const uint32_t b_ = batch_of<T>(a, rid);
            rp_ = as_global((const Ray *)s_tbl[b_].rays_v);
            bq_ = (a.batch_anyhit >> b_) & 1u;
          }
          const Ray r = load_ray<T>(rp_ + rid, a.debug_flags);
          lane_init<T>(L, r);
          L.pk |= bq_ << 9;
          sp = 0;
          if (STATS) st_steps = st_tris = 0;
          // The reference pops and tests the root first (nanort.h:2526-2533).  For a branch root that test is implied by
          // the first step: a ray that misses the root's box misses both children's boxes (each lies inside it and the
          // slab arithmetic is monotone), so the step on record 0 ends in W_POP with an empty stack — the same miss.
          if (a.root_is_branch && !a.root_test) {
            cur = 0u;
            state = W_TRAV;
          } else if (a.root_is_branch) { // adopted tree whose child boxes may stick out of node 0's box: test it, as the reference does
            const Node root = a.nodes[0];
            cur = 0u;
            state = slab_test<T>(L, root.bmin, root.bmax) ? W_TRAV : W_POP;
          } else { // single-leaf tree: test the root box, then its primitives
            const Node root = a.nodes[0];
            const bool root_hit = slab_test<T>(L, root.bmin, root.bmax);
            cur = a.packed_leaves ? packed_leaf_ref(root.data[0], root.data[1]) : 0u;
            state = root_hit ? W_LEAF : W_POP; // W_POP with sp == 0 finishes the ray
          }
          if (a.debug_flags & 2u) state = W_POP;
        }
        if (STATS) {
          st_refills++;
          st_refilled += take;
        }
        ck.next += take;
        fresh = __ballot(state == W_IDLE);
      }
      idle = __ballot(state == W_IDLE);
    }
    if (clocked && ck.exhausted && clk_dry == 0ull) clk_dry = __builtin_amdgcn_s_memrealtime();
    NRT_CLOCK_LIVE(64u - (unsigned)__builtin_popcountll(idle));
    if constexpr (QUAD) {
      // The tail of a launch, four lanes to a ray (behind this loop): no rays are left to hand out and at most a.tail_lanes lanes of
      // this wave still hold one (tunable tail_quad).  The tail finishes every ray the wave holds and nothing returns from it, so
      // only the switch stands here: the tail's twenty moved registers and its temporaries stay out of the allocation and the
      // scheduling of the loop that every launch runs (profiles/r07b_tail_behind_loop.txt).
      const unsigned live_n_ = 64u - (unsigned)__builtin_popcountll(idle);
      if (ck.exhausted && live_n_ != 0u && live_n_ <= NRT_TAIL_N) { // (wave-uniform)
        tail_idle = idle;
        to_tail = true;
        break;
      }
    }
    if (idle == ~0ull) {
      if (ck.exhausted) break;
      continue;
    }

    // ---- phase 1: inner nodes / stack pops ---------------------------------------------
    // (lanes that leave the loop are invisible to its ballots: the wave counts those waiting at a leaf itself)
    if (STATS) {
      const unsigned long long now_ = __builtin_amdgcn_s_memtime();
      st_t_refill += now_ - st_stamp;
      st_stamp = now_;
    }
    unsigned n_wait_leaf = (unsigned)__builtin_popcountll(__ballot(state == W_LEAF));
    while (state == W_TRAV || state == W_POP) {
      if (STATS) {
        st_it1++;
        st_act1 += (unsigned)__builtin_popcountll(__ballot(true));
        if (!ck.exhausted) {
          st_it1_s++;
          st_act1_s += (unsigned)__builtin_popcountll(__ballot(true));
        }
      }
      // a lane that must pop does so first and, if the popped entry survives, steps into it in the same iteration
#pragma unroll
      for (int u_ = 0; u_ < ((WIDTH == 4 && sizeof(T) == 4 && !STATS) ? NRT_W4_P1_UNROLL : ((WIDTH == 2 && sizeof(T) == 8 && !STATS) ? NRT_W2_F64_P1_UNROLL : 1)); u_++) { // (several pop + step rounds per trip: the loop's own bookkeeping — two ballots, the exit test — runs once per trip)
      if (state == W_POP) NRT_POP_ENTRY(stk);
      if (state == W_TRAV) {
        if (STATS) st_steps++;
        if constexpr (WIDTH == 4) {
#if NRT_W4_PRESEL
          if constexpr (sizeof(T) == 4) {
            const char *wb_ = reinterpret_cast<const char *>(a.wide4);
            const RecOff rec_ = (RecOff)cur << 7; // (32 bits: api_query.hip sends arrays of 4 GiB and more to the ORDER & 4 instantiations)
            const Slab4<float> sl = slab4_presel<RecOff>(L, wb_, rec_);
            const Wide4Tail w = *reinterpret_cast<const Wide4Tail *>(wb_ + (size_t)rec_ + 96);
            if constexpr ((ORDER & 1) == 1)
              NRT_STEP_NODE4_DIST(sl, w);
            else
              NRT_STEP_NODE4_SL(sl, w);
          } else
#endif
          {
            const Wide4Node<T> w = a.wide4[cur];
            NRT_STEP_NODE4(w);
          }
        } else {
#ifdef NRT_PROBE_EXTRA_LOADS // sensitivity probe (tools/variant_ab.sh): N more 16-byte reads of the record about to be fetched
          typedef uint32_t u4v_ __attribute__((ext_vector_type(4)));
          u4v_ d0_; // (issued before the record's own loads, which return after them; kept live past the step)
          asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(d0_) : "v"(a.wide + cur) : "memory");
          for (int x_ = 1; x_ < NRT_PROBE_EXTRA_LOADS; x_++) // (same destination: the returns are in order)
            asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "+v"(d0_) : "v"(a.wide + cur) : "memory");
#endif
#if NRT_W2_F64_PRESEL
          bool stepped_ = false;
          if constexpr (sizeof(T) == 8) {
            if (a.wide_below_4g) { // (wave-uniform)
              const char *wb_ = reinterpret_cast<const char *>(a.wide);
              const uint32_t rec_ = cur * (uint32_t)sizeof(WideNode<double>);
              const SlabPair<double> sl = slab_pair_presel(L, wb_, rec_);
              const WideTail w = *reinterpret_cast<const WideTail *>(wb_ + (size_t)rec_ + 96);
              NRT_STEP_NODE_SL(sl, w);
              stepped_ = true;
            }
          }
          if (!stepped_)
#endif
          {
          const WideNode<T> w = a.wide[cur];
#ifdef NRT_PROBE_EXTRA_VALU // ... N more dependent v_fma_f32 per step
          {
            float f_ = __uint_as_float(cur);
            for (int x_ = 0; x_ < NRT_PROBE_EXTRA_VALU; x_++) asm volatile("v_fma_f32 %0, %0, %0, %0" : "+v"(f_));
            asm volatile("" :: "v"(f_));
          }
#endif
          NRT_STEP_NODE(w);
          }
#ifdef NRT_PROBE_EXTRA_LOADS
          asm volatile("" :: "v"(d0_));
#endif
        }
      }
      }
      // Leave when only a few lanes still walk — unless nothing else could be done anyway: no lane waits at a leaf
      // and there are no rays left to hand out (the drain of a launch: the last long rays then stay in this
      // tight loop instead of paying the outer loop's bookkeeping on every step).
      n_wait_leaf += (unsigned)__builtin_popcountll(__ballot(state == W_LEAF));
      const unsigned n_walk_ = (unsigned)__builtin_popcountll(__ballot(state == W_TRAV || state == W_POP));
      NRT_CLOCK_LIVE(n_walk_ + n_wait_leaf);
      if (n_walk_ < a.trav_min && (n_wait_leaf != 0u || !ck.exhausted)) break;
      if constexpr (QUAD) { // the drain otherwise never leaves this loop: few enough rays left for four lanes to a ray (top of the outer loop)
        if (ck.exhausted && n_walk_ + n_wait_leaf <= NRT_TAIL_N) break;
      }
    }
    if constexpr (QUAD) {
      if (ck.exhausted && (unsigned)__builtin_popcountll(__ballot(state != W_IDLE)) <= NRT_TAIL_N) continue;
    }

    // ---- phase 2: leaves ------------------------------------------------------------------
    // With only a few lanes at a leaf and a refill due, take the refill first: the new rays walk to
    // their first leaves while these lanes wait, and the triangle loop then runs with many more
    // lanes.  (Every skip is followed by a refill that hands out at least one ray or marks the
    // claim exhausted, so this always makes progress.)
    if (STATS) {
      const unsigned long long now_ = __builtin_amdgcn_s_memtime();
      st_t_p1 += now_ - st_stamp;
      st_stamp = now_;
    }
    const unsigned n_leaf = (unsigned)__builtin_popcountll(__ballot(state == W_LEAF));
    const bool refill_due = !ck.exhausted && (unsigned)__builtin_popcountll(__ballot(state == W_IDLE)) >= a.refill_min;
    if (n_leaf != 0u && !(n_leaf < a.leaf_min && refill_due)) {
      uint32_t cnt = 0, first = 0;
      if (state == W_LEAF) leaf_span(a.packed_leaves, a.nodes, cur, cnt, first);
      if (a.debug_flags & 1u) cnt = 0;
      NRT_RAY_SKIP(skip, state == W_LEAF);
      if (STATS) {
        st_entries2++;
        st_idle2 += (unsigned)__builtin_popcountll(__ballot(state == W_IDLE));
      }
      bool items_done_ = false; // (wave-uniform)
      if constexpr (LEAFC) {
        // ---- leaf items: the records of every waiting lane, spread over the wave --------------------------------------------
        // In the steady state fewer than half of the lanes wait at a leaf when this phase runs (tools/loop_stats.py: 30 of 64
        // on C3's primaries, 20 on its bounce rays) and a lane's 1-4 records are tested two per trip by their OWNER, the other
        // lanes idling.  When all the waiting lanes' records together fit ONE trip of the wave (<= 64: the rule on incoherent
        // waves), record k of owner o becomes ITEM base(o) + k, item j is tested by lane j with the owner's ray constants (fetched
        // by ds_bpermute: org, Sx Sy Sz, the packed axes), and the owner then takes its items' results IN RECORD ORDER through
        // the reference's own accept rule (`tt > t` / `tt < min_t` reject, equality and NaN accepted, nanort.h:1133-1139): the
        // same tests on the same operands, accepted in the same sequence, so the lane state after the leaf is bit for bit what
        // the owner's own loop leaves (tests/test_gpu_leaf_items.py).  More records than lanes: the owners' loop below.  Trees
        // whose leaves hold more than four records do not take this variant at all (api_query.hip).
        items_done_ = leaf_items_one_trip<PLAIN, uint32_t>(L, cnt, a.tris, first, lane, s_item_owner[tid / kWave], s_item_rec[tid / kWave], a.range0, a.range1,
                                                 skip, cull);
      }
      if (items_done_) {
        // (the waiting lanes' records were tested as items)
      } else if constexpr (KIND == kPrimTriangles && (WIDTH == 4 ? NRT_W4_TRI_UNROLL : NRT_W2_TRI_UNROLL) > 1) {
        // several records per trip, all fetched before any is tested (same tests in the same order; fewer dependent
        // round trips per leaf — this variant has the registers for it)
        constexpr uint32_t U_ = WIDTH == 4 ? NRT_W4_TRI_UNROLL : NRT_W2_TRI_UNROLL;
        for (uint32_t i = 0; __ballot(i < cnt) != 0ull; i += U_) {
          LeafTri<T> t_[U_];
          if (STATS) {
            st_it2++;
            st_act2 += (unsigned)__builtin_popcountll(__ballot(i < cnt));
            st_act2b += (unsigned)__builtin_popcountll(__ballot(i + 1u < cnt));
            if (!ck.exhausted) {
              st_it2_s++;
              st_act2_s += (unsigned)__builtin_popcountll(__ballot(i < cnt)) + (unsigned)__builtin_popcountll(__ballot(i + 1u < cnt));
            }
            if (i < cnt) st_tris += (i + 1u < cnt) ? 2u : 1u;
          }
#pragma unroll
          for (uint32_t j = 0; j < U_; j++) t_[j] = a.tris[first + (i + j < cnt ? i + j : 0u)];
#pragma unroll
          for (uint32_t j = 0; j < U_; j++) {
            if (PLAIN)
              tri_test<T, true>(L, t_[j], i + j < cnt, 0u, 0u, 0u, false);
            else
              tri_test<T>(L, t_[j], i + j < cnt, a.range0, a.range1, skip, cull);
          }
        }
      } else if constexpr (!STATS && KIND == kPrimSpheres && NRT_SPHERE_UNROLL > 1) { // the same for the 20-byte sphere records
        if (anyhit_) {
          NRT_SPHERE_LOOP(true)
        } else {
          NRT_SPHERE_LOOP(false)
        }
      } else if constexpr (KIND != kPrimTriangles) {
        if (anyhit_) {
          NRT_RECORD_LOOP(true)
        } else {
          NRT_RECORD_LOOP(false)
        }
      } else {
        NRT_RECORD_LOOP(false)
      }
      // occlusion query: any accepted primitive settles the ray — drop what is left of its stack
      if (a.any_hit | a.batch_anyhit) sp = (state == W_LEAF && L.hit_t < L.max_t && (a.any_hit != 0u || (L.pk & 512u) != 0u)) ? 0 : sp;
      state = (state == W_LEAF) ? W_POP : state;
    }
    if (STATS) st_t_p2 += __builtin_amdgcn_s_memtime() - st_stamp;
  }
  if constexpr (QUAD) {
    // ---- the tail of a launch: FOUR LANES TO A RAY ------------------------------------------------------------------------
    // No rays are left to hand out and at most a.tail_lanes lanes of this wave still hold one (tunable tail_quad): what the launch
    // waits for from here on is the dependent chain of those rays, ~200 wave instructions a step of which a handful of lanes use
    // anything.  The wave's own idle lanes shorten the step instead.  Live ray number q (ballot rank) moves to quad q — its
    // constants and state by ds_bpermute, its stack stays where it is: the quad pops and pushes through a LaneStack over its
    // owner's column (`ostk_`; the pop is NRT_POP_ENTRY itself) — and the quads finish the rays: lane j tests box j of a record
    // (slab_axis on the rows slab4_presel fetches) and ranks its slot in the binary loop's order (NRT_STEP_NODE4_SL), two DPP quad
    // permutes combine the four hit bits, the first hit in rank order is entered and the others are pushed in reverse rank order
    // with their t_min; at a leaf lane j tests record i + j (tri_solve, as tri_test) and the four results are accepted IN RECORD ORDER
    // through the reference's rule (nanort.h:1133-1139), every lane following the sequence on its copy of the hit distance; u, v
    // and the primitive stay with the lane that tested the accepted record (`owner_`), which writes the result.  Every ray sees
    // the pops, steps and leaf tests its lane would have continued with, in the same order: records bit-identical
    // (tests/test_gpu_tail_quad.py).  Nothing leaves the wave.
    if (to_tail) { // (wave-uniform; the only way here with a live lane)
      const unsigned long long idle = tail_idle;
      const unsigned live_n_ = 64u - (unsigned)__builtin_popcountll(idle);
      if (state == W_IDLE && rid != kInvalid) NRT_WRITE_RESULT(); // finished results leave before their lanes are reused
      const unsigned q_ = lane >> 2, j_ = lane & 3u;
      uint32_t src_ = 0u; // the lane whose ray this quad takes: the q-th live one
      {
        unsigned k_ = 0u;
        for (unsigned long long m_ = ~idle; m_ != 0ull; m_ &= m_ - 1ull, k_++) src_ = (q_ == k_) ? (uint32_t)__builtin_ctzll(m_) : src_;
      }
      const bool has_ = q_ < live_n_;
      const int sa_ = (int)(src_ << 2);
#define NRT_QMOVE_F(x_) x_ = __int_as_float(__builtin_amdgcn_ds_bpermute(sa_, __float_as_int(x_)))
#define NRT_QMOVE_U(x_) x_ = (uint32_t)__builtin_amdgcn_ds_bpermute(sa_, (int)(x_))
      NRT_QMOVE_F(L.org0);
      NRT_QMOVE_F(L.org1);
      NRT_QMOVE_F(L.org2);
      NRT_QMOVE_F(L.inv0);
      NRT_QMOVE_F(L.inv1);
      NRT_QMOVE_F(L.inv2);
      NRT_QMOVE_F(L.min_t);
      NRT_QMOVE_F(L.max_t);
      NRT_QMOVE_F(L.hit_t);
      NRT_QMOVE_F(L.Sx);
      NRT_QMOVE_F(L.Sy);
      NRT_QMOVE_F(L.Sz);
      NRT_QMOVE_F(L.u);
      NRT_QMOVE_F(L.v);
      NRT_QMOVE_U(L.pk); // (with the any-hit bit of the ray's batch)
      NRT_QMOVE_U(L.prim);
      NRT_QMOVE_U(rid);
      NRT_QMOVE_U(cur);
      state = __builtin_amdgcn_ds_bpermute(sa_, state);
      sp = __builtin_amdgcn_ds_bpermute(sa_, sp);
#undef NRT_QMOVE_F
#undef NRT_QMOVE_U
      L.so0 = (L.pk & 1u) ? 48u : 0u; // (lane_init: 48 where the direction is negative — the sign bits of pk)
      L.so1 = (L.pk & 2u) ? 48u : 0u;
      L.so2 = (L.pk & 4u) ? 48u : 0u;
      state = has_ ? state : W_IDLE; // (a lane waiting at a leaf stays waiting at that leaf)
      rid = has_ ? rid : kInvalid;
      sp = has_ ? sp : 0;
      const unsigned otid_ = (tid & ~63u) | src_; // the owner's column of s_stack, and of the spill arrays: the stack of the ray this quad took
      const LaneStack<SE, STACK, TraverseArgs<T>> ostk_ = {a, otid_, blockIdx.x * kTraverseBlock + otid_};
      bool owner_ = j_ == 0u; // this lane holds u, v, prim of the ray's best hit (exactly one lane of a quad)
      const char *wb_ = reinterpret_cast<const char *>(a.wide4);
      for (;;) {
        const unsigned long long liveq_ = __ballot(state != W_IDLE);
        NRT_CLOCK_LIVE((unsigned)__builtin_popcountll(liveq_) >> 2);
        if (liveq_ == 0ull) break;
        if (state == W_POP) NRT_POP_ENTRY(ostk_); // (every lane of the quad alike)
        if (state == W_TRAV) { // NRT_STEP_NODE4_SL's order over the rows slab4_presel fetches, slot j in lane j
          const uint32_t rec0_ = cur << 7, rec_ = rec0_ + 4u * j_, rec48_ = rec_ + 48u;
          const float lo0 = *reinterpret_cast<const float *>(wb_ + (size_t)(rec_ + L.so0));
          const float hi0 = *reinterpret_cast<const float *>(wb_ + (size_t)(rec48_ - L.so0));
          const float lo1 = *reinterpret_cast<const float *>(wb_ + (size_t)(rec_ + L.so1) + 16);
          const float hi1 = *reinterpret_cast<const float *>(wb_ + (size_t)(rec48_ - L.so1) + 16);
          const float lo2 = *reinterpret_cast<const float *>(wb_ + (size_t)(rec_ + L.so2) + 32);
          const float hi2 = *reinterpret_cast<const float *>(wb_ + (size_t)(rec48_ - L.so2) + 32);
          const uint32_t c_ = *reinterpret_cast<const uint32_t *>(wb_ + (size_t)rec_ + 96);
          const int ax0_ = *reinterpret_cast<const int32_t *>(wb_ + (size_t)rec0_ + 112);
          const int axh_ = *reinterpret_cast<const int32_t *>(wb_ + (size_t)(rec0_ + 4u * (j_ >> 1)) + 116); // axis1 for slots 0, 1; axis2 for slots 2, 3
          float tmin = L.min_t, tmax = L.hit_t;
          slab_axis<float>(lo0, hi0, L.org0, L.inv0, tmin, tmax);
          slab_axis<float>(lo1, hi1, L.org1, L.inv1, tmin, tmax);
          slab_axis<float>(lo2, hi2, L.org2, L.inv2, tmin, tmax);
          const bool h_ = (tmin <= tmax) & (((j_ & 1u) == 0u) | (c_ != kWide4Empty)); // (slots 1 and 3 can be empty)
          // rank of slot j in the binary loop's order: the near half (by the node's axis) first, inside a half its near slot first
          const uint32_t s0_ = (uint32_t)L.sign(ax0_), sh_ = (uint32_t)L.sign(axh_);
          const uint32_t rank_ = ((((j_ >> 1) ^ s0_) & 1u) << 1) | ((j_ ^ sh_) & 1u);
          const uint32_t m_ = quad_or(h_ ? (1u << rank_) : 0u); // the quad's hits by rank
          const uint32_t n_ = (uint32_t)__builtin_popcount(m_);
          const uint32_t pos_ = (uint32_t)__builtin_popcount(m_ & ((1u << rank_) - 1u)); // hits before mine
          // the first hit in rank order is entered; the others are pushed in reverse rank order (they pop in rank order)
          if (h_ && pos_ != 0u) NRT_STACK_STORE(ostk_, sp + (int)(n_ - 1u - pos_), c_, tmin);
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // (what one lane of the quad pushed, the four pop: program order holds across lanes)
          sp += n_ != 0u ? (int)(n_ - 1u) : 0;
          const uint32_t next_ = quad_or((h_ && pos_ == 0u) ? c_ : 0u); // (a reference is never 0: record 0 is the root)
          cur = n_ != 0u ? (next_ & ~kLeafBit) : cur;
          state = n_ != 0u ? ((next_ & kLeafBit) ? W_LEAF : W_TRAV) : W_POP;
        }
        if (__ballot(state == W_LEAF) != 0ull) { // records i .. i + 3 per trip, any count
          uint32_t cnt = 0, first = 0;
          if (state == W_LEAF) leaf_span(a.packed_leaves, a.nodes, cur, cnt, first);
          if (a.debug_flags & 1u) cnt = 0;
          NRT_RAY_SKIP(skip, state == W_LEAF); // (the quad's ray's: rid moved with the ray)
          for (uint32_t i = 0; __ballot(i < cnt) != 0ull; i += 4u) {
            const bool act_ = i + j_ < cnt;
            const LeafTri<T> tri = a.tris[first + (act_ ? i + j_ : 0u)];
            const uint32_t prim_i = tri.prim_id;
            const TriSolve<T> ts_ = tri_solve<T, PLAIN>(tri, act_, L.org0, L.org1, L.org2, L.Sx, L.Sy, L.Sz, L.kx(), L.ky(), L.kz(), a.range0, a.range1, skip, cull);
            const bool ok = ts_.ok;
            const T tt_i = ts_.tt, uu_i = ts_.uu, vv_i = ts_.vv;
            // ... accepted in record order, the same sequence in every lane of the quad
            const uint32_t okm_ = quad_or(ok ? (1u << j_) : 0u);
            if (__ballot(okm_ != 0u) != 0ull) {
              bool got_ = false;
              uint32_t win_ = 0u;
#define NRT_QUAD_ACCEPT(K_)                                                                                                    \
              do {                                                                                                           \
                const T ttk_ = quad_bcast<K_>(tt_i);                                                                         \
                const bool acc_ = ((okm_ >> K_) & 1u) != 0u && !(ttk_ > L.hit_t) && !(ttk_ < L.min_t); /* nanort.h:1133-1139 */ \
                L.hit_t = acc_ ? ttk_ : L.hit_t;                                                                             \
                win_ = acc_ ? (uint32_t)K_ : win_;                                                                           \
                got_ = got_ | acc_;                                                                                          \
              } while (0)
              NRT_QUAD_ACCEPT(0);
              NRT_QUAD_ACCEPT(1);
              NRT_QUAD_ACCEPT(2);
              NRT_QUAD_ACCEPT(3);
#undef NRT_QUAD_ACCEPT
              const bool me_ = got_ & (win_ == j_);
              owner_ = got_ ? me_ : owner_;
              L.u = me_ ? uu_i : L.u;
              L.v = me_ ? vv_i : L.v;
              L.prim = me_ ? prim_i : L.prim;
            }
          }
          // occlusion query: any accepted primitive settles the ray — drop what is left of its stack
          if (a.any_hit | a.batch_anyhit) sp = (state == W_LEAF && L.hit_t < L.max_t && (a.any_hit != 0u || (L.pk & 512u) != 0u)) ? 0 : sp;
          state = (state == W_LEAF) ? W_POP : state;
        }
      }
      if (owner_ && rid != kInvalid) NRT_WRITE_RESULT();
      rid = kInvalid;
    }
  }
  if (rid != kInvalid) NRT_WRITE_RESULT(); // results still held in registers
#undef NRT_WRITE_RESULT
#undef NRT_RECORD_LOOP
#undef NRT_SPHERE_LOOP
#undef NRT_TEST_PRIM
#undef NRT_RAY_OPEN
#undef NRT_RAY_SKIP
#undef NRT_CLOCK_LIVE
#undef NRT_TAIL_N
  done_end<T>(a, lane);
  if (clocked && lane == 0u) { // one record per wave, reduced on the host (atomics on one line would serialise the exits)
    unsigned long long *rec = a.wave_clock + (size_t)kWaveClockWords * (size_t)(gslot / kWave);
    const unsigned long long clk_end = __builtin_amdgcn_s_memrealtime();
    rec[0] = clk_begin;
    rec[1] = clk_dry == 0ull ? clk_end : clk_dry;
    rec[2] = clk_end;
    rec[3] = clk_l16 == 0ull ? clk_end : clk_l16;
    rec[4] = clk_l8 == 0ull ? clk_end : clk_l8;
    rec[5] = clk_l4 == 0ull ? clk_end : clk_l4;
  }
  if (STATS && lane == 0) { // counters[0..7]: it1, act1, idle lanes at phase-2 entry, it2, act2, refills, refilled, phase-2 entries
    atomicAdd(&a.counters[0], st_it1);
    atomicAdd(&a.counters[1], st_act1);
    atomicAdd(&a.counters[2], st_idle2);
    atomicAdd(&a.counters[3], st_it2);
    atomicAdd(&a.counters[4], st_act2);
    atomicAdd(&a.counters[5], st_refills);
    atomicAdd(&a.counters[6], st_refilled);
    atomicAdd(&a.counters[7], st_entries2);
    atomicAdd(&a.counters[8], st_t_refill); // [8..10]: shader-clock ticks of the wave spent refilling / in the inner-node phase / in the leaf phase
    atomicAdd(&a.counters[9], st_t_p1);
    atomicAdd(&a.counters[10], st_t_p2);
    atomicAdd(&a.counters[11], st_act2b);   // leaf loop, two records per trip: lanes with a second record
    atomicAdd(&a.counters[12], st_it1_s);   // [12..15]: inner iterations / their active lanes / leaf trips / records tested while rays were still being handed out
    atomicAdd(&a.counters[13], st_act1_s);
    atomicAdd(&a.counters[14], st_it2_s);
    atomicAdd(&a.counters[15], st_act2_s);
  }
}

// BVHNode[] -> dense WideNode[]: (1) branches per 1024-node tile, (2) exclusive scan of the
// tile counts, (3) dense index of every branch node, (4) the records.
__device__ __forceinline__ uint32_t block_exclusive_scan_256(uint32_t v, uint32_t *s_wave, uint32_t &total) {
  const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t inc = v;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(inc, off);
    if (lane >= (unsigned)off) inc += t;
  }
  if (lane == 63) s_wave[w] = inc;
  __syncthreads();
  uint32_t pre = 0;
  total = 0;
  for (unsigned j = 0; j < 4; j++) {
    if (j < w) pre += s_wave[j];
    total += s_wave[j];
  }
  __syncthreads();
  return pre + inc - v;
}

template <typename T>
__global__ __launch_bounds__(256) void k_wide_count(const typename Wire<T>::Node *__restrict__ nodes, uint32_t n,
                                                    uint32_t *__restrict__ tile_count) {
  __shared__ uint32_t s_wave[4];
  uint32_t c = 0;
  const uint32_t base = blockIdx.x * 1024u + threadIdx.x * 4u;
  for (uint32_t k = 0; k < 4; k++)
    if (base + k < n && nodes[base + k].flag == 0) c++;
  uint32_t total;
  (void)block_exclusive_scan_256(c, s_wave, total);
  if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_wide_scan_tiles(uint32_t *tile_count, uint32_t num_tiles) {
  __shared__ uint32_t s_wave[4];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < num_tiles; base += 256u) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < num_tiles ? tile_count[i] : 0u;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan_256(v, s_wave, total);
    if (i < num_tiles) tile_count[i] = carry + ex;
    carry += total;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_wide_index(const typename Wire<T>::Node *__restrict__ nodes, uint32_t n,
                                                    const uint32_t *__restrict__ tile_base,
                                                    uint32_t *__restrict__ dense_of, uint32_t scramble_mod) {
  __shared__ uint32_t s_wave[4];
  const uint32_t base = blockIdx.x * 1024u + threadIdx.x * 4u;
  uint32_t flags[4], c = 0;
  for (uint32_t k = 0; k < 4; k++) {
    flags[k] = (base + k < n && nodes[base + k].flag == 0) ? 1u : 0u;
    c += flags[k];
  }
  uint32_t total;
  uint32_t ex = tile_base[blockIdx.x] + block_exclusive_scan_256(c, s_wave, total);
  for (uint32_t k = 0; k < 4; k++) {
    // (layout probe, tunable wide_scramble: record j of the pre-order goes to slot j * P mod #records — a bijection that
    // keeps the root at 0 and tears every subtree apart; how much the walk slows down bounds what any re-ordering can win)
    if (base + k < n) dense_of[base + k] = scramble_mod ? (uint32_t)(((uint64_t)ex * 2654435761ull) % scramble_mod) : ex;
    ex += flags[k];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_make_wide(const typename Wire<T>::Node *__restrict__ nodes, uint32_t n,
                                                   const uint32_t *__restrict__ dense_of, uint32_t packed,
                                                   WideNode<T> *__restrict__ wide, Wide4Node<T> *__restrict__ wide4) {
  typedef typename Wire<T>::Node Node;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const Node nd = nodes[i];
  if (nd.flag != 0) return;
  if (nd.data[0] >= n || nd.data[1] >= n) return; // an unreachable record of a loaded tree: never visited
  const Node a = nodes[nd.data[0]], b = nodes[nd.data[1]];
  WideNode<T> w;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if constexpr (sizeof(T) == 8) { // (component-major: see WideNode<double>)
      w.mn[k][0] = a.bmin[k];
      w.mx[k][0] = a.bmax[k];
      w.mn[k][1] = b.bmin[k];
      w.mx[k][1] = b.bmax[k];
    } else {
      w.box0[k] = a.bmin[k];
      w.box0[3 + k] = a.bmax[k];
      w.box1[k] = b.bmin[k];
      w.box1[3 + k] = b.bmax[k];
    }
  }
  const uint32_t la = packed ? packed_leaf_ref(a.data[0], a.data[1]) : nd.data[0];
  const uint32_t lb = packed ? packed_leaf_ref(b.data[0], b.data[1]) : nd.data[1];
  w.c0 = a.flag != 0 ? (kLeafBit | la) : dense_of[nd.data[0]];
  w.c1 = b.flag != 0 ? (kLeafBit | lb) : dense_of[nd.data[1]];
  w.axis = nd.axis;
  w.pad = 0;
  wide[dense_of[i]] = w;
  if (wide4 == nullptr) return;
  // the record over two levels: each child's children (or the child itself, when it is a leaf)
  Wide4Node<T> q;
  q.axis0 = nd.axis;
  q.pad = 0;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const Node &ch = h == 0 ? a : b;
    const uint32_t ch_ref = h == 0 ? w.c0 : w.c1;
    const bool two = ch.flag == 0 && ch.data[0] < n && ch.data[1] < n;
    int32_t axis = 0;
    if (two) {
      axis = ch.axis;
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const uint32_t gi = ch.data[j];
        const Node g = nodes[gi];
#pragma unroll
        for (int k = 0; k < 3; k++) {
          q.bmin[k][2 * h + j] = g.bmin[k];
          q.bmax[k][2 * h + j] = g.bmax[k];
        }
        const uint32_t lg = packed ? packed_leaf_ref(g.data[0], g.data[1]) : gi;
        q.c[2 * h + j] = g.flag != 0 ? (kLeafBit | lg) : dense_of[gi];
      }
    } else { // a leaf child (or a branch whose children cannot be read: then it is entered through its own record)
#pragma unroll
      for (int k = 0; k < 3; k++) {
        q.bmin[k][2 * h] = ch.bmin[k];
        q.bmax[k][2 * h] = ch.bmax[k];
        q.bmin[k][2 * h + 1] = ch.bmin[k];
        q.bmax[k][2 * h + 1] = ch.bmax[k];
      }
      q.c[2 * h] = ch_ref;
      q.c[2 * h + 1] = kWide4Empty;
    }
    if (h == 0) q.axis1 = axis; else q.axis2 = axis;
  }
  wide4[dense_of[i]] = q;
}

// ---- host-side launchers (kernels.h) ----------------------------------------

template <typename T>
static const void *traverse_kernel(bool count, int lds_entries) { // 16, 24, anything else -> 32
  switch (lds_entries) {
    case 16: return count ? (const void *)k_traverse<T, true, 16> : (const void *)k_traverse<T, false, 16>;
    case 24: return count ? (const void *)k_traverse<T, true, 24> : (const void *)k_traverse<T, false, 24>;
    default: return count ? (const void *)k_traverse<T, true, 32> : (const void *)k_traverse<T, false, 32>;
  }
}
template <typename T>
hipError_t launch_traverse(const TraverseArgs<T> &args, unsigned grid, bool count, int lds_entries, hipStream_t s) {
  launch_persistent(traverse_kernel<T>(count, lds_entries), grid, args, s);
  return hipGetLastError();
}
template <typename T>
int traverse_blocks_per_cu(int lds_entries) { // (of the non-counting kernel)
  return resident_blocks(traverse_kernel<T>(false, lds_entries), 4);
}

// Every instantiation of k_traverse_wide in this library, by its template arguments (walk_variant.h), with its name as
// rocprofv3 prints it without the argument list.  The profiling instantiations exist in libnanort_hip_prof.so only (nanort_hip_prof.h).
#ifdef NRT_PROF
constexpr bool kProfBuild = true;
#else
constexpr bool kProfBuild = false;
#endif
struct WideKernel {
  WalkVariant v;
  const void *kernel;
  const char *name;
};
#define NRT_STR2(x) #x
#define NRT_STR(x) NRT_STR2(x)
#define NRT_WIDE_KERNEL(T_, STACK_, STATS_, KIND_, PLAIN_, CLOCK_, WIDTH_, ORDER_)                          \
  {{sizeof(T_) == 4, STACK_, STATS_, KIND_, PLAIN_, CLOCK_, WIDTH_, ORDER_},                                \
   (const void *)k_traverse_wide<T_, STACK_, STATS_, KIND_, PLAIN_, CLOCK_, WIDTH_, ORDER_>,                \
   "nrt::k_traverse_wide<" #T_ ", " NRT_STR(STACK_) ", " #STATS_ ", " #KIND_ ", " #PLAIN_ ", " #CLOCK_ ", " #WIDTH_ ", " #ORDER_ ">"},
static const WideKernel kWideKernels[] = {
    NRT_WALK_VARIANTS(NRT_WIDE_KERNEL)
#ifdef NRT_PROF
    NRT_WALK_VARIANTS_PROF(NRT_WIDE_KERNEL)
#endif
};
#undef NRT_WIDE_KERNEL
static const WideKernel *find_wide_kernel(const WalkVariant &v) {
  for (const WideKernel &k : kWideKernels)
    if (k.v == v) return &k;
  return nullptr; // (tests/test_walk_variant.py: no request picks a variant that is not listed)
}

template <typename T>
hipError_t launch_traverse_wide(const TraverseArgs<T> &args, unsigned grid, int lds_entries, int prim_kind, hipStream_t s,
                                const char **name_out) {
  const WalkRequest r = {sizeof(T) == 4, prim_kind, lds_entries, args.wide4 != nullptr, args.wide4_big != 0, args.leaf_items != 0, args.order4 != 0,
                         args.plain_options != 0, (args.debug_flags & 32u) != 0, args.wave_clock != nullptr};
  const WideKernel *k = find_wide_kernel(pick_wide_variant(r, kProfBuild));
  if (!k) return hipErrorInvalidValue;
  NRT_RANGE_PUSH(k->name); // (profiling library: a marker range per traversal launch, named like the kernel)
  launch_persistent(k->kernel, grid, args, s);
  NRT_RANGE_POP();
  if (name_out) *name_out = k->name;
  return hipGetLastError();
}

template <typename T>
int traverse_wide_blocks_per_cu(int lds_entries, int prim_kind, bool wide4) {
  const WideKernel *k = find_wide_kernel(occupancy_variant(sizeof(T) == 4, prim_kind, lds_entries, wide4));
  return k ? resident_blocks(k->kernel, 4) : 4;
}

template <typename T>
hipError_t launch_make_wide(const typename Wire<T>::Node *nodes, uint32_t n, uint32_t packed, uint32_t *scratch,
                            WideNode<T> *wide, Wide4Node<T> *wide4, uint32_t scramble_mod, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint32_t tiles = (n + 1023u) / 1024u;
  uint32_t *tile_count = scratch, *dense_of = scratch + tiles;
  hipLaunchKernelGGL((k_wide_count<T>), dim3(tiles), dim3(256), 0, s, nodes, n, tile_count);
  hipLaunchKernelGGL(k_wide_scan_tiles, dim3(1), dim3(256), 0, s, tile_count, tiles);
  hipLaunchKernelGGL((k_wide_index<T>), dim3(tiles), dim3(256), 0, s, nodes, n, tile_count, dense_of, scramble_mod);
  hipLaunchKernelGGL((k_make_wide<T>), dim3((n + 255u) / 256u), dim3(256), 0, s, nodes, n, dense_of, packed, wide, wide4);
  return hipGetLastError();
}

NRT_INSTANTIATE_F32_F64(launch_traverse)
NRT_INSTANTIATE_F32_F64(launch_traverse_wide)
NRT_INSTANTIATE_F32_F64(traverse_wide_blocks_per_cu)
NRT_INSTANTIATE_F32_F64(launch_make_wide)
NRT_INSTANTIATE_F32_F64(traverse_blocks_per_cu)

} // namespace nrt
