// nanort_amd/csrc/scene_kernels.hip — every kernel of the two-level (instanced) path, and their launchers (kernels.h):
//   k_scene_walk      the single-pass walk: the top-level tree and the instances' trees in the same lane on one stack, no list;
//   k_scene_list*     the listing kernels: per ray, the (at most 64 nearest) instances whose world boxes it enters;
//   k_scene_trace     the reference's loop over such a list (or, for a handful of instances, over its own scan of their boxes).
// What the two tracing kernels share is stated once, above them (scene_claim_ray … scene_local_ray); the per-lane moves they
// share with the single-level walk are walk_dev.h's.  Which of the kernels a call runs, Commit and the tunables: scene.hip.
#include "kernels.h"
#include "walk_dev.h"

#include <algorithm>

namespace nrt {

#ifndef NRT_SCENE_WALK_WAVES
#define NRT_SCENE_WALK_WAVES 4 // waves per SIMD k_scene_walk is compiled for (128 registers; 5 -> 96 registers spills 30 of them and measured slower)
#endif
#ifndef NRT_SCENE_P1_UNROLL
#define NRT_SCENE_P1_UNROLL 2 // pop + step rounds per trip of the inner-node loop of both tracing kernels
#endif

// ---------------------------------------------------------------------------
// Two-level (instanced) traversal, nanosg::Scene::Traverse (examples/nanosg/nanosg.h:778-870) for a whole batch in ONE
// launch.  A ray arrives with the list of instances whose world boxes it enters, nearest entry first (at most 64:
// BVHAccel::ListNodeIntersections, nanort.h:2608-2692 — built by the listing kernels below over the top-level BVH).
// The lane then does what the reference's loop does, candidate after candidate: skip the instance if the nearest world
// distance so far is below its entry distance (nanosg.h:795), else carry the ray into the instance's space (MultV with
// inv_xform / inv_xform33, :806-808, the local interval left at Ray()'s defaults), walk the instance's OWN tree with the
// single-level machinery (walk_dev.h: same WideNode step, same watertight test, same order: the local record is what
// nrtTraverseBatchDevice would return for that local ray, bit for bit), measure the world distance of the local hit
// (:823-836) and keep it if strictly nearer (:838).  Lanes of a wave are at different candidates of different instances
// at the same time — every lane carries its instance's array bases — so there is no per-instance launch, no compaction
// and no host round trip; the wave alternates between the inner-node phase and the leaf phase like k_traverse_wide.
// A lane whose ray is finished takes the next one from a per-partition work cursor (a wave refills once `refill_min` lanes are
// free).  Since round 4 this kernel traces small scenes and the rays the single-pass walk (k_scene_walk, below) hands over;
// scenes of thousands of instances go through that walk, which keeps no list at all.
// ---------------------------------------------------------------------------
enum : int { S_NEXT = 4, S_FIN = 5, S_DONE = 6 }; // besides W_TRAV / W_LEAF / W_POP: pick the next candidate / a local walk ended / ray finished

// ---- what k_scene_trace and k_scene_walk share, stated once ---------------------------------------------------------------
// The ray a free lane takes (a.n: none).  Persistent threads: a wave claims for all its free lanes by one atomic once `refill_min`
// of them are free, so it keeps its lanes busy to the end of the batch instead of waiting for the slowest of 64 fixed rays.  One cursor per ray partition (== XCD, as in k_traverse_wide): a wave drains its home range first, so an XCD
// walks one band of the batch and its L2 keeps one part of the scene; then it steals from the others (`part`, and `tried` = the
// partitions found empty: both wave-uniform, kept by the caller; tried == a.num_parts: nothing is left anywhere).
template <typename A>
__device__ __forceinline__ uint32_t scene_claim_ray(const A &a, unsigned long long free_lanes, unsigned want, unsigned lane, uint32_t &part, uint32_t &tried) {
  const uint32_t per = a.n / a.num_parts;
  uint32_t mine = a.n;
  while (tried < a.num_parts) {
    const uint32_t lo = part * per, len = (part + 1u == a.num_parts) ? a.n - lo : per;
    uint32_t base = 0;
    if (lane == (unsigned)__builtin_ctzll(free_lanes)) base = atomicAdd(a.cursor + kCursorStrideWords * part, want);
    base = (uint32_t)__builtin_amdgcn_readlane((int)base, __builtin_ctzll(free_lanes));
    if (base < len) {
      const uint32_t off = base + (uint32_t)__builtin_popcountll(free_lanes & ((1ull << lane) - 1ull));
      mine = off < len ? lo + off : a.n;
      break;
    }
    part = (part + 1u == a.num_parts) ? 0u : part + 1u;
    tried++;
  }
  return mine;
}

// The miss record a ray starts with; overwritten by every better hit.
__device__ __forceinline__ nrt_scene_hit_f32 scene_miss_record(float max_t) {
  nrt_scene_hit_f32 h;
  h.t = max_t;
  h.u = 0.0f;
  h.v = 0.0f;
  h.prim_id = 0xFFFFFFFFu;
  h.node_id = 0xFFFFFFFFu;
  return h;
}

// The world distance of the local hit L holds, in an instance whose local -> world matrix is `xform`.
__device__ __forceinline__ float scene_world_distance(const Lane<float> &L, const float (&xform)[4][4], const float worg[3]) {
  float lp[3], wp[3];
  lp[0] = L.org0 + L.hit_t * L.d0; // nanosg.h:823-825
  lp[1] = L.org1 + L.hit_t * L.d1;
  lp[2] = L.org2 + L.hit_t * L.d2;
  mult_v(wp, xform, lp);
  const float px = wp[0] - worg[0], py = wp[1] - worg[1], pz = wp[2] - worg[2];
  return __builtin_sqrtf(px * px + py * py + pz * pz); // vlength, nanort.h:383-385
}

// The world ray carried into an instance's space, into L (`inv`, `inv33`: the instance's inv_xform / inv_xform33, whole or the twelve
// entries MultV reads).
template <int W>
__device__ __forceinline__ void scene_local_ray(const float (&inv)[4][W], const float (&inv33)[4][W], const float worg[3], const float wdir[3], Lane<float> &L) {
  nrt_ray_f32 lr;
  mult_v(lr.org, inv, worg);   // nanosg.h:807
  mult_v(lr.dir, inv33, wdir); // nanosg.h:808
  lr.min_t = 0.0f;             // Ray() defaults (nanort.h:477-487): the world interval is not propagated
  lr.max_t = 3.402823466e+38f;
  lr.type = 0;
  lane_init<float>(L, lr);
}

// SKIP (both tracing kernels): the skip id a lane tests a leaf of instance `inst` with — its ray's pair {prim_id, node_id} at
// pairs + rid * stride names ONE primitive of ONE instance, so the id is the pair's primitive when the open instance is the pair's node
// and kInvalid (rejects nothing) otherwise.  The pair lives nowhere: it is re-read at every leaf, so a refilled lane, whose rid is
// new, has its new ray's pair, and the load is issued before the leaf's records and independent of them.  A pair that names no
// primitive of the scene (either id 0xFFFFFFFF or out of range) needs no test of its own: no instance and no record carries such an id.
__device__ __forceinline__ uint32_t scene_skip_id(const void *pairs, uint32_t stride, uint32_t rid, uint32_t inst) {
  const uint32_t *p = (const uint32_t *)((const char *)pairs + (size_t)rid * stride);
  const uint32_t prim = p[0], node = p[1];
  return node == inst ? prim : kInvalid;
}

// SCAN: a scene of a handful of instances (a.scan_nodes of them): the lane lists the instances its ray enters ITSELF when it fetches
// the ray — every world box tested in id order, exactly what the listing kernel of such scenes did in a launch of its own
// (k_scene_list) — into its own slots of the list arrays, which it alone reads back: one launch per batch, no second
// pass over the rays.
// ANY: the occlusion query (nrtSceneOccludedBatch*): only the flag is wanted.  The flag of the closest-hit form is "some candidate
// the loop opens has a local hit whose world distance is < FLT_MAX" — the first such hit sets it and nothing clears it, and until
// that hit the nearest distance is still FLT_MAX, so the cull (nanosg.h:795) opens the same candidates in both forms.  So the ANY
// form walks the same candidates in the same order, lets a local walk drop its stack at the first leaf that accepts a primitive
// (the single-level any-hit rule of k_traverse_wide), and finishes the ray with flag 1 at the first local hit with
// t_world < FLT_MAX.  It writes no record (a.hits is not read).  The one place the forms can differ: the dropped walk's hit is the
// first accepted, not the nearest, and where world distances overflow or are NaN the two may disagree on t_world < FLT_MAX
// (include/nanort_hip.h states that limit).
// MASKED (with SCAN: a listed ray's list comes from a listing kernel, which has applied the words already): instance visibility
// masks — an instance exists for a ray iff (a.inst_masks[id] & ray word) != 0, so a hidden instance's box is not accepted as
// entered and never reaches the list.  The ray's word is read with the ray and dies with the scan.
// SKIP: per-ray skip pairs (nrtSceneQueryBatch*) — the leaf steps use the rejecting form of the triangle test with
// scene_skip_id's id and the range [0, 0xFFFFFFFF), which holds every primitive; nothing else moves.  The scan of a SKIP query always
// runs as the MASKED form, with a null a.inst_masks standing for all-ones words (the bytes of the unmasked scan, §3.14 item 3).
template <int STACK, bool SCAN, bool ANY = false, bool MASKED = false, bool SKIP = false>
__global__ __launch_bounds__(kTraverseBlock) void k_scene_trace(const SceneTraceArgs a) {
  typedef float T;
  typedef StackEntry<float> SE;
  __shared__ SE::type s_stack[STACK][kTraverseBlock];

  const unsigned tid = threadIdx.x;
  const unsigned lane = lane_id();
  const unsigned gslot = blockIdx.x * kTraverseBlock + tid;
  const LaneStack<SE, STACK, SceneTraceArgs> stk = {a, tid, gslot};

  Lane<float> L;
  uint32_t i = 0, ri = 0; // this lane's slot in the launch (lists, counts) and its ray (== i unless the launch traces a subset)
  uint32_t cur = 0;
  int state = S_DONE, sp = 0;
  uint32_t cnt = 0, j = 0, inst = 0; // candidates of this ray; how many of them have been taken; the instance being walked
  float last_t = 0.0f;               // (entry distance, id) of the candidate taken last: the next one is the smallest above it
  uint32_t last_id = 0u;
  float best_t = 3.402823466e+38f; // t_nearest = numeric_limits<T>::max(), nanosg.h:787
  bool has_hit = false;
  float worg[3] = {0.f, 0.f, 0.f}, wdir[3] = {0.f, 0.f, 0.f};
  const WideNode<float> *wide = nullptr;
  const Wide4Node<float> *wide4 = nullptr; // non-null: this instance's tree is walked two levels per step
  const LeafTri<float> *tris = nullptr;
  const nrt_node_f32 *nodes = nullptr;
  uint32_t packed = 1u;
  bool exhausted = false;
  uint32_t part = blockIdx.x % a.num_parts, tried = 0u; // ray partition this wave claims from (its home first), partitions found empty

  for (;;) {
    // ---- refill free lanes -------------------------------------------------------------------------------------------
    {
      const unsigned long long free_lanes = __ballot(state == S_DONE);
      const unsigned want = (unsigned)__builtin_popcountll(free_lanes);
      if (!exhausted && want >= a.refill_min) {
        const uint32_t mine = scene_claim_ray(a, free_lanes, want, lane, part, tried);
        exhausted = tried >= a.num_parts;
        if (state == S_DONE && mine < a.n) {
          i = mine;
          ri = a.subset ? a.subset[i] : i;
          const nrt_ray_f32 r = a.rays[ri];
#pragma unroll
          for (int k = 0; k < 3; k++) {
            worg[k] = r.org[k];
            wdir[k] = r.dir[k];
          }
          if (SCAN) {
            cnt = 0u;
            uint32_t rm = 0xFFFFFFFFu;
            if constexpr (MASKED) rm = a.ray_masks ? a.ray_masks[ri] : 0xFFFFFFFFu;
            for (uint32_t k = 0; k < a.scan_nodes; k++) { // (wave-uniform addresses: the boxes arrive through the scalar cache)
              float t;
              if constexpr (MASKED) {
                const uint32_t iw = (SKIP && a.inst_masks == nullptr) ? 0xFFFFFFFFu : a.inst_masks[k];
                if ((iw & rm) == 0u) continue; // hidden from this ray: it does not exist
              }
              if (!scene_node_interval(r, a.insts[k].xbmin, a.insts[k].xbmax, t)) continue;
              a.list_t[(size_t)cnt * a.n + i] = t;
              a.list_node[(size_t)cnt * a.n + i] = k;
              cnt++;
            }
          } else {
            cnt = a.count[i];
          }
          j = 0;
          last_t = 0.0f;
          last_id = 0u;
          best_t = 3.402823466e+38f;
          has_hit = false;
          if constexpr (!ANY) a.hits[ri] = scene_miss_record(r.max_t);
          state = S_NEXT;
        }
      }
    }
    // ---- candidates: finish a local walk, pick the next instance ---------------------------------------------------
    // (Both steps are long and run under divergence — matrix products, a division-heavy lane set-up, the selection scan over the
    // ray's list: the wave runs them for SEVERAL lanes at a time.  Lanes between two instances wait until `cand_min` of them have
    // gathered, unless fewer than `cand_busy_max` lanes would be walking meanwhile.  Walking lanes always finish, so the waiting
    // ones are served at the latest when nobody walks.)
    const unsigned n_cand = (unsigned)__builtin_popcountll(__ballot(state == S_FIN || state == S_NEXT));
    const unsigned n_busy = (unsigned)__builtin_popcountll(__ballot(state == W_TRAV || state == W_POP || state == W_LEAF));
    const bool do_cand = n_cand != 0u && (n_cand >= a.cand_min || n_busy < a.cand_busy_max);
    if (do_cand) {
    if (state == S_FIN) {
      if (L.hit_t < L.max_t) { // the local Traverse() hit (strict final predicate, nanort.h:2552)
        const float t_world = scene_world_distance(L, a.insts[inst].xform, worg);
        if constexpr (ANY) {
          if (t_world < best_t) { // (best_t is still FLT_MAX) occluded: no further candidate is opened, S_NEXT below writes the flag
            has_hit = true;
            j = cnt;
          }
        } else
        if (t_world < best_t) {                                             // strict, nanosg.h:838
          best_t = t_world;
          has_hit = true;
          nrt_scene_hit_f32 h;
          h.t = t_world;
          h.u = L.u;
          h.v = L.v;
          h.prim_id = L.prim;
          h.node_id = inst;
          a.hits[ri] = h;
        }
      }
      state = S_NEXT;
    }
    if (state == S_NEXT) {
      state = S_DONE;
      // The ray's candidates — the (at most 64 nearest) instances whose world boxes it enters — lie UNSORTED in its list
      // (scene.hip appends them as the top-level walk finds them).  The reference visits them in the order of (entry distance,
      // id) and skips one whose entry distance lies beyond the nearest hit so far (nanosg.h:795) — and then every later one
      // too, their entry distances being no smaller.  So: pick the smallest (t_min, id) above the one taken last; if the hit
      // so far is nearer than that, the ray is done.  Rays take one or two candidates before that happens, so a selection scan
      // per candidate taken costs far less than sorting every list (round 2: an insertion sort in global memory while listing).
      if (j < cnt) {
        float bt = 0.0f;
        uint32_t bid = 0xFFFFFFFFu;
        bool found = false;
        for (uint32_t q = 0; q < cnt; q++) {
          const float t = a.list_t[(size_t)q * a.n + i];
          if (j != 0u && t < last_t) continue;
          if (found && t > bt) continue;
          const uint32_t id = a.list_node[(size_t)q * a.n + i];
          if (j != 0u && t == last_t && id <= last_id) continue; // taken already (ids are unique)
          if (!found || t < bt || id < bid) { // (here t <= bt: nearer, or as near with the lower id)
            bt = t;
            bid = id;
            found = true;
          }
        }
        if (found && !(best_t < bt)) { // (else: early cull, nanosg.h:795 — for this candidate and all that follow)
          last_t = bt;
          last_id = bid;
          j++;
          inst = bid;
          const SceneInst &nd = a.insts[inst];
          scene_local_ray(nd.inv_xform, nd.inv_xform33, worg, wdir, L);
          wide =(const WideNode<float> *)nd.wide;
          wide4 = (const Wide4Node<float> *)nd.wide4;
          tris = (const LeafTri<float> *)nd.tris;
          nodes = nd.nodes;
          packed = nd.packed_leaves;
          sp = 0;
          cur = 0u;
          if (nd.root_is_branch && nd.tree_nested) {
            state = W_TRAV; // (a ray that misses node 0's box misses both children's: see k_traverse_wide)
          } else {
            const nrt_node_f32 root = nodes[0];
            const bool root_hit = slab_test<float>(L, root.bmin, root.bmax);
            if (nd.root_is_branch) {
              state = root_hit ? W_TRAV : W_POP;
            } else { // single-leaf tree
              cur = packed ? packed_leaf_ref(root.data[0], root.data[1]) : 0u;
              state = root_hit ? W_LEAF : W_POP;
            }
          }
        }
      }
      if (state == S_DONE && a.mask) a.mask[ri] = has_hit ? 1 : 0; // this ray is finished
    }
    }
    if (__ballot(state != S_DONE) == 0ull) {
      if (exhausted) break;
      continue;
    }

    // ---- phase 1: inner nodes / stack pops ---------------------------------------------------------------------
    unsigned n_wait = (unsigned)__builtin_popcountll(__ballot(state == W_LEAF || state == S_FIN));
    while (state == W_TRAV || state == W_POP) {
#pragma unroll
      for (int u_ = 0; u_ < NRT_SCENE_P1_UNROLL; u_++) { // (pop + step rounds per trip, as in k_traverse_wide)
      if (state == W_POP) {
        NRT_POP_ENTRY(stk);
        state = (state == W_IDLE) ? S_FIN : state; // an empty stack ends this instance's walk
      }
      if (state == W_TRAV) {
        if (wide4 != nullptr) { // (trees whose child boxes lie inside their parents': two levels per step, NRT_STEP_NODE4)
          const Wide4Node<float> w = load_global_record(wide4 + cur);
          NRT_STEP_NODE4(w);
        } else {
          const WideNode<float> w = load_global_record(wide + cur);
          NRT_STEP_NODE(w);
        }
      }
      }
      n_wait += (unsigned)__builtin_popcountll(__ballot(state == W_LEAF || state == S_FIN));
      if ((unsigned)__builtin_popcountll(__ballot(state == W_TRAV || state == W_POP)) < a.trav_min && n_wait != 0u) break;
    }

    // ---- phase 2: leaves -----------------------------------------------------------------------------------------
    if (__ballot(state == W_LEAF) != 0ull) {
      uint32_t lcnt = 0, first = 0;
      uint32_t skip = kInvalid;
      if constexpr (SKIP) {
        if (state == W_LEAF) skip = scene_skip_id(a.skip_pairs, a.skip_stride, ri, inst);
      }
      if (state == W_LEAF) leaf_span(packed, nodes, cur, lcnt, first);
      for (uint32_t k = 0; __ballot(k < lcnt) != 0ull; k += 2u) { // two records per trip, as in k_traverse_wide
        if (k < lcnt) { // (divergent on purpose: the lanes' record arrays differ)
          const bool two = k + 1u < lcnt;
          const LeafTri<float> t0 = load_global_record(tris + first + k);
          const LeafTri<float> t1 = load_global_record(tris + first + (two ? k + 1u : k));
          tri_test<float, !SKIP>(L, t0, true, 0u, 0xFFFFFFFFu, skip, false); // default trace options (nanosg.h:817); SKIP: but for skip_prim_id
          tri_test<float, !SKIP>(L, t1, two, 0u, 0xFFFFFFFFu, skip, false);
        }
      }
      // occlusion query: any accepted primitive settles this instance — drop what is left of its stack (as k_traverse_wide does)
      if constexpr (ANY) sp = (state == W_LEAF && L.hit_t < L.max_t) ? 0 : sp;
      state = (state == W_LEAF) ? W_POP : state;
    }
  }
}

static const void *scene_trace_kernel(bool scan, bool any, bool masked = false, bool skip = false) {
  if (skip && scan) return any ? (const void *)k_scene_trace<kSceneLdsStack, true, true, true, true> : (const void *)k_scene_trace<kSceneLdsStack, true, false, true, true>;
  if (skip) return any ? (const void *)k_scene_trace<kSceneLdsStack, false, true, false, true> : (const void *)k_scene_trace<kSceneLdsStack, false, false, false, true>;
  if (masked && scan) return any ? (const void *)k_scene_trace<kSceneLdsStack, true, true, true> : (const void *)k_scene_trace<kSceneLdsStack, true, false, true>;
  if (any) return scan ? (const void *)k_scene_trace<kSceneLdsStack, true, true> : (const void *)k_scene_trace<kSceneLdsStack, false, true>;
  return scan ? (const void *)k_scene_trace<kSceneLdsStack, true> : (const void *)k_scene_trace<kSceneLdsStack, false>;
}
hipError_t launch_scene_trace(const SceneTraceArgs &args, unsigned grid, hipStream_t s) {
  if (args.n == 0) return hipSuccess;
  launch_persistent(scene_trace_kernel(args.scan_nodes != 0, args.any_hit != 0, args.masked != 0, args.skip != 0), grid, args, s);
  return hipGetLastError();
}
int scene_trace_blocks_per_cu() { // (one grid size for both: the fewer)
  return std::min(resident_blocks(scene_trace_kernel(false, false), 4), resident_blocks(scene_trace_kernel(true, false), 8));
}

// ---------------------------------------------------------------------------
// The single-pass scene walk: nanosg::Scene::Traverse (examples/nanosg/nanosg.h:778-870) WITHOUT the list.  The reference first
// lists the (at most 64 nearest) instances whose world boxes the ray enters (BVHAccel::ListNodeIntersections,
// nanort.h:2608-2692), sorted by (entry distance, id) =: rank, then walks the list: an instance is skipped once the nearest world
// distance so far lies below its entry distance (:795), else traced with a fresh local ray, and a strictly nearer world
// distance wins (:838).  The listing must follow the ray through the WHOLE scene before the first triangle is tested — on
// 100 000 instances that was three quarters of the time.  This kernel walks the top-level tree (its Wide4Node records, near
// slots first) and, whenever it reaches an entered instance, walks that instance's tree at once, in the same lane, on the same
// stack (top-level entries below, the open instance's entries above `base`).  What makes that exact:
//   * winner     = the traced hit with the smallest (t_world, rank) — the list order with strict '<' picks exactly that;
//   * skipping   an instance or a top-level subtree entered at e is allowed when the current winner w has t_world_w < e and
//                t_min_w < e: w ranks before everything in there, so the reference's cull has fired at or before it (entry
//                distances only grow from a box to a box inside it — for rays whose direction components are ordinary non-zero
//                numbers; other rays skip per instance only, never a subtree);
//   * certificate at the end: at most 64 instances traced, and no OTHER traced hit lies in front of the winner's own box entry
//                (t2 >= t_min_w).  Then the winner is inside the prefix of the list the reference processes, everything in
//                that prefix was traced here, and nothing behind it can win.  A ray without the certificate (a hit that rounds
//                to the near side of its own box while another hit lies in between; more than 64 boxes; direction vectors
//                far shorter than 1, where the reference's cull compares a distance with a parameter and fires early) is
//                appended to `redo` and traced by the listing path (k_scene_list* + k_scene_trace over the subset).
// The argument is spelled out and tested on the CPU, with random visiting orders and random skipping, by the model
// sgo_traverse_unordered_model (tests/test_scene_walk_model.py); tests/test_gpu_scene.py compares this kernel with the listing
// path and the restatement record by record.
//
// ANY = true: THE OCCLUSION FORM (nrtSceneOccludedBatch*).  Only the flag is wanted, and the reference's flag is
//     F = "one of the 64 entered instances of smallest rank (entry distance, id) has a local hit with t_world < FLT_MAX"
// (before the first such hit the nearest distance is still FLT_MAX, so the cull at nanosg.h:795 cannot skip a listed instance
// whose entry distance is <= FLT_MAX; the first such hit sets the flag and nothing clears it).  The closest-hit certificate above
// does not carry over — there is no winner to compare with.  The walk instead runs in two modes:
//   * searching  (no qualifying hit yet): nothing is skipped — skipping needs a winner, cull_t stays +inf — so every entered
//                instance the top-level walk reaches is opened (`traced` counts them), and its local walk drops its stack at the
//                first leaf that accepts a primitive.  If the top-level walk ends in this mode, EVERY entered instance was traced
//                and none has a qualifying hit; the reference's 64 are a subset of them: F = 0, however many boxes were entered.
//   * counting   after the first qualifying hit, in instance h entered at e_h: F = 1 if h is one of the 64 of smallest rank, i.e.
//                if fewer than 64 entered instances rank before (e_h, id_h).  (If h is NOT among them, F depends on instances this
//                lane has not traced: nothing is claimed, the ray goes to `redo`.)  The lane does not keep the ranks of the
//                instances it opened before h, so it bounds: B = (instances opened before h, all of them taken to rank before h)
//                + (entered instances met later in the top-level walk with (e, id) < (e_h, id_h)).  B >= the true number in front
//                of h, so B < 64 proves F = 1.  In this mode no instance is opened; top-level subtrees entered beyond
//                max(e_h, ray.min_t) are skipped for tame rays (everything inside is entered no earlier than the subtree's box,
//                hence ranks behind h and does not count — the closest-hit skip rule with the hit distance left out); other rays
//                walk every top-level box they enter.  B reaching 64 sends the ray to `redo` at once; so does a hit in an instance
//                entered beyond FLT_MAX (the one entry distance the reference's cull does fire on before a hit).
//   * shortcut   a scene of at most 64 instances: every entered instance is listed, the first qualifying hit ends the ray with 1.
// `redo` rays go through the listing path in its ANY form, which is exact.  No record is written (a.hits is not read).  The rule
// is modelled and tested on the CPU with random visiting orders and random legal skipping (tests/test_scene_occlusion_model.py).
//
// MASKED = true: INSTANCE VISIBILITY MASKS (nrtScene*BatchMasked*).  An instance exists for a ray iff (its word & the ray's word)
// != 0, and the answer is the unmasked one on the scene of the visible instances with their ids kept.  The one change: where an
// instance's world box is accepted as entered (`entered`, below), the acceptance is ANDed with that test.  A hidden instance is
// therefore neither opened nor counted — not in `traced` (the at-most-64 certificate), not in the ANY form's bound B, not among
// its "entered instances met later".  Both arguments above carry over unchanged, because they are the unmasked arguments on the
// visible sub-scene: the top-level tree only ever prunes (a subtree is skipped by its box and the winner, never by what it holds),
// so walking the tree of ALL instances and dropping the hidden ones at the leaves visits the visible instances a tree over
// them alone would let the lane reach, in some order — and the arguments hold for any order.  The `num_insts <= 64` shortcut stays
// valid: visible <= total.  The ray's word is loaded when the lane claims the ray and kept in a register; an instance's word
// comes from a.top_masks, in the order of a.open_top, so its load is issued WITH the 128-byte line's, not behind it.
//
// SKIP = true: PER-RAY SKIP PAIRS (nrtSceneQueryBatch*).  The leaf phase tests with scene_skip_id's id (the lane keeps
// the open instance's id for the record already; leaf_items_one_trip fetches the OWNER's id across the wave) in the rejecting form of
// the triangle test over the range [0, 0xFFFFFFFF).  The intersector then returns false for that one primitive of that one instance
// without touching the ray's state, which is all the contract changes: certificate, cull and hand-over argue about hits that WERE
// accepted and hold as they are.  Only MASKED forms exist with SKIP; a null a.top_masks stands for all-ones words.
// ---------------------------------------------------------------------------
enum : int { T_ENTER = 7, S_END = 8 }; // a top-level leaf was reached: open its instance / the top-level stack ran empty: the ray is finished

// The top-level tree is walked by the SAME step as the instances' trees: while a lane is in the top-level tree its Lane holds the
// WORLD ray (hit_t pinned at ray.max_t: the box test is then ListNodeIntersections' own, nanort.h:2651), its record pointer is
// the top-level tree's, and `cull_t` — max(winner's distance, winner's box entry, ray.min_t), +inf without a hit — takes the
// place of the hit distance where the walk skips (a box entered beyond it ranks behind a nearer hit; the clipped entry
// distance the step computes is the unclipped one whenever it exceeds ray.min_t).  A leaf reference of the top-level tree names
// instances instead of triangles: the lane leaves the loop, opens the instance (its Lane becomes the local ray, `base` = the
// stack height) and rejoins the same loop; when the stack is back at `base` the world ray returns.  Lanes in the top-level
// tree and lanes inside instances therefore execute the same instructions.
#define NRT_POP_ENTRY_SCENE()                                                                          \
do {                                                                                                 \
  const bool fin_ = (sp <= base);                     /* this level's part of the stack is empty */  \
  const int s1_ = fin_ ? sp : sp - 1;                                                                \
  typename SE::type e_;                                                                              \
  stk.load(s_stack, s1_ > 0 ? s1_ : 0, e_, !fin_); /* (fin_: entry sp is nobody's) */                 \
  const bool enter_ = !fin_ & (SE::tmin(e_) <= (in_top ? cull_t : L.hit_t));                         \
  const uint32_t ref_ = SE::ref(e_);                                                                 \
  sp = s1_;                                                                                          \
  cur = enter_ ? (ref_ & ~kLeafBit) : cur;                                                           \
  state = fin_ ? (in_top ? S_END : S_FIN) : (enter_ ? ((ref_ & kLeafBit) ? W_LEAF : W_TRAV) : W_POP); \
} while (0)

template <int STACK, bool STATS, bool ANY = false, bool MASKED = false, bool SKIP = false>
__global__ __launch_bounds__(kTraverseBlock, STATS ? 1 : NRT_SCENE_WALK_WAVES) void k_scene_walk(const SceneWalkArgs a) {
  typedef float T;
  typedef StackEntry<float> SE;
  __shared__ SE::type s_stack[STACK][kTraverseBlock];
  __shared__ uint32_t s_item_owner[kTraverseBlock / kWave][kWave]; // leaf items (leaf_items_one_trip)
  __shared__ const LeafTri<float> *s_item_rec[kTraverseBlock / kWave][kWave];
  // (profiling build only) per wave: [0] outer trips, [1..2] level-change blocks run / lanes served, [3..4] inner-phase trips / lane
  // steps, [5] of those steps in the top-level tree, [6..7] leaf-phase trips / lanes with a first record, [8] instances opened,
  // [9] top-level leaves reached, [10..12] shader-clock ticks in level changes / the inner phase / the leaf phase
  unsigned long long st[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

  const unsigned tid = threadIdx.x;
  const unsigned lane = lane_id();
  const unsigned gslot = blockIdx.x * kTraverseBlock + tid;
  const LaneStack<SE, STACK, SceneWalkArgs> stk = {a, tid, gslot};

  Lane<float> L;
  uint32_t i = 0;   // this lane's ray
  uint32_t cur = 0; // record due (of the top-level tree or of the open instance's tree) / leaf reference reached
  int state = S_DONE, sp = 0, base = 0;
  bool in_top = true, tame = true;
  float cur_tmin = 0.f; // box entry distance of the open instance
  uint32_t inst = 0, traced = 0; // the open instance's id; instances opened so far
  float best_t = 3.402823466e+38f, best_tmin = 0.f, t2 = __builtin_huge_valf(); // winner's distance and box entry; runner-up distance
  float cull_t = __builtin_huge_valf();
  uint32_t best_id = 0;
  bool has_hit = false;
  float worg[3] = {0.f, 0.f, 0.f}, wdir[3] = {0.f, 0.f, 0.f}, winv[3] = {0.f, 0.f, 0.f};
  float wmin_t = 0.f, wmax_t = 0.f;
  const Wide4Node<float> *wide4 = nullptr; // the tree being walked: the top-level tree's records or the open instance's
  const LeafTri<float> *tris = nullptr;
  bool exhausted = false;
  uint32_t part = blockIdx.x % a.num_parts, tried = 0u;
  uint32_t ray_word = 0xFFFFFFFFu; // MASKED: this ray's visibility word

  auto world_ray = [&]() { // the lane (re-)enters the top-level tree
    L.org0 = worg[0];
    L.org1 = worg[1];
    L.org2 = worg[2];
    L.inv0 = winv[0];
    L.inv1 = winv[1];
    L.inv2 = winv[2];
    L.min_t = wmin_t;
    L.hit_t = wmax_t;
    L.max_t = wmax_t;
    L.pk = (wdir[0] < 0.0f ? 1u : 0u) | (wdir[1] < 0.0f ? 2u : 0u) | (wdir[2] < 0.0f ? 4u : 0u);
    wide4 = a.top_wide4;
    in_top = true;
    base = 0;
  };

  for (;;) {
    if (STATS) st[0]++;
    // ---- refill free lanes --------------------------------------------------------------------------------------------
    {
      const unsigned long long free_lanes = __ballot(state == S_DONE);
      const unsigned want = (unsigned)__builtin_popcountll(free_lanes);
      if (!exhausted && want >= a.refill_min) {
        const uint32_t mine = scene_claim_ray(a, free_lanes, want, lane, part, tried);
        exhausted = tried >= a.num_parts;
        if (state == S_DONE && mine < a.n) {
          i = mine;
          const nrt_ray_f32 r = a.rays[i];
          if constexpr (MASKED) ray_word = a.ray_masks ? a.ray_masks[i] : 0xFFFFFFFFu;
          // tame: ordinary non-zero direction components and a finite origin — entry distances then only grow from a box to a
          // box inside it, which is what skipping top-level SUBTREES rests on.  Any other ray (axis-parallel, say) walks the whole
          // top-level tree it enters (cull_t stays +inf) and skips per instance only, by the instance's own entry distance.
          tame = true;
#pragma unroll
          for (int k = 0; k < 3; k++) {
            worg[k] = r.org[k];
            wdir[k] = r.dir[k];
            winv[k] = safe_inverse<float>(r.dir[k]); // vsafe_inverse (nanort.h:2509 via :349-357): what the top-level boxes are tested with
            tame = tame && (__builtin_fabsf(r.dir[k]) >= 1.1920928955078125e-07f) && (__builtin_fabsf(winv[k]) < __builtin_huge_valf()) &&
                   (__builtin_fabsf(r.org[k]) < __builtin_huge_valf());
          }
          wmin_t = r.min_t;
          wmax_t = r.max_t;
          best_t = 3.402823466e+38f; // t_nearest = numeric_limits<T>::max(), nanosg.h:787
          best_tmin = 0.f;
          best_id = 0u;
          t2 = __builtin_huge_valf();
          cull_t = __builtin_huge_valf();
          has_hit = false;
          traced = 0u;
          if constexpr (!ANY) a.hits[i] = scene_miss_record(r.max_t);
          sp = 0;
          world_ray();
          cur = 0u; // record 0 == the root branch (its own box test is implied by its children's)
          state = W_TRAV;
        }
      }
    }
    // ---- level changes: a local walk ended / an instance is opened / the ray is finished (long, divergent: for several lanes at a time) ----
    {
      const unsigned n_cand = (unsigned)__builtin_popcountll(__ballot(state == S_FIN || state == T_ENTER || state == S_END));
      const unsigned n_busy = (unsigned)__builtin_popcountll(__ballot(state == W_TRAV || state == W_POP || state == W_LEAF));
      if (n_cand != 0u && (n_cand >= a.cand_min || n_busy < a.cand_busy_max)) {
        const unsigned long long c0_ = STATS ? clock64() : 0ull;
        if (STATS) {
          st[1]++;
          st[2] += n_cand;
          st[9] += (unsigned)__builtin_popcountll(__ballot(state == T_ENTER));
        }
        if (state == S_FIN) {
          if (L.hit_t < L.max_t) { // the local Traverse() hit (strict final predicate, nanort.h:2552)
            const float t_world = scene_world_distance(L, a.insts[inst].xform, worg); // (the full record, by id: only an instance that was hit needs its xform)
            if constexpr (ANY) {
              if (t_world < 3.402823466e+38f) { // the first qualifying hit (searching mode ends; see the comment above the kernel)
                const uint32_t before = traced - 1u; // instances opened before this one: all taken to rank before it
                if (3.402823466e+38f < cur_tmin || before >= 64u) {
                  a.redo[atomicAdd(a.redo_count, 1u)] = i;
                  state = S_DONE;
                } else if (a.num_insts <= 64u) {
                  a.mask[i] = 1;
                  state = S_DONE;
                } else { // counting mode: (best_tmin, best_id) = h's rank, traced = the bound B
                  has_hit = true;
                  best_tmin = cur_tmin;
                  best_id = inst;
                  traced = before;
                  cull_t = tame ? (cur_tmin > wmin_t ? cur_tmin : wmin_t) : __builtin_huge_valf();
                }
              }
            } else {
            // strict '<' in rank order (nanosg.h:838) == smallest (t_world, rank) in any order
            const bool wins = t_world < best_t ||
                              (has_hit && t_world == best_t && (cur_tmin < best_tmin || (cur_tmin == best_tmin && inst < best_id)));
            if (wins) {
              if (has_hit && best_t < t2) t2 = best_t; // the old winner becomes the runner-up
              best_t = t_world;
              best_tmin = cur_tmin;
              best_id = inst;
              has_hit = true;
              const float c = best_t > best_tmin ? best_t : best_tmin;
              cull_t = tame ? (c > wmin_t ? c : wmin_t) : __builtin_huge_valf();
              nrt_scene_hit_f32 h;
              h.t = t_world;
              h.u = L.u;
              h.v = L.v;
              h.prim_id = L.prim;
              h.node_id = inst;
              a.hits[i] = h;
            } else if (t_world < t2) {
              t2 = t_world;
            }
            }
          }
          if (!ANY || state != S_DONE) {
            world_ray();
            state = W_POP;
          }
        } else if (state == T_ENTER) {
          // cur: a leaf reference of the top-level tree, (count - 1, first) into its index array.  One instance is opened now;
          // the others of a leaf of several (boxes the builder could not separate) wait on the stack as a leaf of one fewer.
          const uint32_t lcount = packed_leaf_count(cur), lfirst = packed_leaf_first(cur);
          NRT_PUSH_IF(lcount > 1u, kLeafBit | packed_leaf_ref(lcount - 1u, lfirst + 1u), -__builtin_huge_valf());
          const SceneOpen &nd = a.open_top[lfirst]; // (everything the opening needs in one 128-byte line: id, world box, matrices, mesh)
          const uint32_t k = nd.id;
          uint32_t inst_word = 0xFFFFFFFFu;
          if constexpr (MASKED) inst_word = (SKIP && a.top_masks == nullptr) ? 0xFFFFFFFFu : a.top_masks[lfirst]; // (no address depends on the line: both loads are in flight together)
          const float bx[6] = {nd.xbmin[0], nd.xbmin[1], nd.xbmin[2], nd.xbmax[0], nd.xbmax[1], nd.xbmax[2]};
          const bool s0 = wdir[0] < 0.0f, s1 = wdir[1] < 0.0f, s2 = wdir[2] < 0.0f;
          const float n0 = ((s0 ? bx[3] : bx[0]) - worg[0]) * winv[0], n1 = ((s1 ? bx[4] : bx[1]) - worg[1]) * winv[1],
                      n2 = ((s2 ? bx[5] : bx[2]) - worg[2]) * winv[2];
          const float f0 = ((s0 ? bx[0] : bx[3]) - worg[0]) * winv[0], f1 = ((s1 ? bx[1] : bx[4]) - worg[1]) * winv[1],
                      f2 = ((s2 ? bx[2] : bx[5]) - worg[2]) * winv[2];
          // the leaf's own box test of ListNodeIntersections (IntersectRayAABB, nanort.h:2285-2325, hit_t == ray.max_t) ...
          float tmn = wmin_t, tmx = wmax_t;
          tmn = (n0 > tmn) ? n0 : tmn;
          tmn = (n1 > tmn) ? n1 : tmn;
          tmn = (n2 > tmn) ? n2 : tmn;
          const float g0 = f0 * 1.00000024f, g1 = f1 * 1.00000024f, g2 = f2 * 1.00000024f;
          tmx = (g0 < tmx) ? g0 : tmx;
          tmx = (g1 < tmx) ? g1 : tmx;
          tmx = (g2 < tmx) ? g2 : tmx;
          // ... then NodeBBoxIntersector::Intersect (nanosg.h:603-639): the unclipped interval by the PLAIN reciprocal (for a tame
          // ray the same numbers as above), whose near end the list is sorted by
          float p0 = winv[0], p1 = winv[1], p2 = winv[2]; // (a tame ray's safe reciprocal IS the plain one: the same division)
          if (!tame) {
            p0 = 1.0f / wdir[0];
            p1 = 1.0f / wdir[1];
            p2 = 1.0f / wdir[2];
          }
          const float a0 = ((s0 ? bx[3] : bx[0]) - worg[0]) * p0, a1 = ((s1 ? bx[4] : bx[1]) - worg[1]) * p1,
                      a2 = ((s2 ? bx[5] : bx[2]) - worg[2]) * p2;
          const float b0 = ((s0 ? bx[0] : bx[3]) - worg[0]) * p0, b1 = ((s1 ? bx[1] : bx[4]) - worg[1]) * p1,
                      b2 = ((s2 ? bx[2] : bx[5]) - worg[2]) * p2;
          float e = (a1 > a0) ? a1 : a0;
          e = (a2 > e) ? a2 : e;
          float f = (b1 < b0) ? b1 : b0;
          f = (b2 < f) ? b2 : f;
          bool entered = tmn <= tmx && e <= f;
          if constexpr (MASKED) entered = entered && (inst_word & ray_word) != 0u; // hidden from this ray: it does not exist
          bool behind = has_hit && best_t < e && (best_tmin < e || (best_tmin == e && best_id < k)); // ranks behind a nearer hit
          if constexpr (ANY) { // counting mode: nothing is opened any more; an entered box that ranks before the hit instance's counts
            behind = has_hit;
            if (has_hit && entered && (e < best_tmin || (e == best_tmin && k < best_id))) traced++;
          }
          if (!entered || behind) {
            state = W_POP; // (still in the top-level tree)
            if constexpr (ANY) {
              if (has_hit && traced >= 64u) { // B reached 64: the hit instance may lie outside the reference's list
                a.redo[atomicAdd(a.redo_count, 1u)] = i;
                state = S_DONE;
              }
            }
          } else {
            inst = k;
            cur_tmin = e;
            traced++;
            scene_local_ray(nd.inv, nd.inv33, worg, wdir, L); // (the twelve entries of each matrix that MultV reads)
            const SceneMesh &mesh = a.meshes[nd.mesh];
            wide4 = (const Wide4Node<float> *)mesh.wide4;
            tris = (const LeafTri<float> *)mesh.tris;
            in_top = false;
            base = sp;
            cur = 0u;
            state = W_TRAV; // (a branch root whose children's boxes lie inside it: scene.hip checks ...)
            if (mesh.root_leaf) { // (... or a tree of one leaf: node 0's own box test, nanort.h:2526-2531, then its triangles)
              cur = mesh.leaf_ref;
              state = slab_test<float>(L, mesh.bmin, mesh.bmax) ? W_LEAF : S_FIN;
            }
          }
        } else if (state == S_END) {
          const bool certified = ANY || (traced <= 64u && (!has_hit || t2 >= best_tmin)); // (ANY: no hit: 0; a hit with B < 64: 1 — B >= 64 left above)
          if (certified) {
            if (a.mask) a.mask[i] = has_hit ? 1 : 0;
          } else {
            a.redo[atomicAdd(a.redo_count, 1u)] = i;
          }
          state = S_DONE;
        }
        if (STATS) {
          st[8] += (unsigned)__builtin_popcountll(__ballot(!in_top && base == sp && (state == W_TRAV || state == W_LEAF || state == S_FIN) && cur == 0u));
          st[10] += clock64() - c0_;
        }
      }
    }
    if (__ballot(state != S_DONE) == 0ull) {
      if (exhausted) break;
      continue;
    }

    // ---- phase 1: inner nodes / stack pops, of the top-level tree and of the open instances alike --------------------
    const unsigned long long c1_ = STATS ? clock64() : 0ull;
    unsigned n_wait = (unsigned)__builtin_popcountll(__ballot(state == W_LEAF || state == S_FIN || state == T_ENTER || state == S_END));
    while (state == W_TRAV || state == W_POP) {
      if (STATS) st[3]++;
#pragma unroll
      for (int u_ = 0; u_ < NRT_SCENE_P1_UNROLL; u_++) {
        if (state == W_POP) {
          NRT_POP_ENTRY_SCENE();
          if (state == S_FIN && !(L.hit_t < L.max_t)) { // the instance was missed (most are): back into the top-level tree right here
            world_ray();
            state = W_POP;
          }
        }
        if (STATS) {
          st[4] += (unsigned)__builtin_popcountll(__ballot(state == W_TRAV));
          st[5] += (unsigned)__builtin_popcountll(__ballot(state == W_TRAV && in_top));
        }
        if (state == W_TRAV) {
          const Wide4Node<float> w = load_global_record(wide4 + cur);
          Slab4<float> sl4_ = slab4(L, w);
          const float ct_ = in_top ? cull_t : __builtin_huge_valf(); // (in the top-level tree: nothing entered beyond a nearer hit that ranks before it)
#pragma unroll
          for (int j_ = 0; j_ < 4; j_++) sl4_.h[j_] = sl4_.h[j_] && (sl4_.tm[j_] <= ct_);
          NRT_STEP_NODE4_SL(sl4_, w);
        }
        state = (in_top && state == W_LEAF) ? T_ENTER : state; // a top-level leaf: instances, not triangles
      }
      n_wait += (unsigned)__builtin_popcountll(__ballot(state == W_LEAF || state == S_FIN || state == T_ENTER || state == S_END));
      if ((unsigned)__builtin_popcountll(__ballot(state == W_TRAV || state == W_POP)) < a.trav_min && n_wait != 0u) break;
    }

    // ---- phase 2: leaves ---------------------------------------------------------------------------------------------
    const unsigned long long c2_ = STATS ? clock64() : 0ull;
    if (STATS) st[11] += c2_ - c1_;
    if (__ballot(state == W_LEAF) != 0ull) {
      uint32_t lcnt = 0, first = 0;
      uint32_t skip = kInvalid;
      if constexpr (SKIP) {
        if (state == W_LEAF) skip = scene_skip_id(a.skip_pairs, a.skip_stride, i, inst);
      }
      if (state == W_LEAF) { // (packed leaf references: scene.hip checks)
        lcnt = packed_leaf_count(cur);
        first = packed_leaf_first(cur);
      }
      // (few lanes wait at a leaf in this kernel — 10 of 64 on the instanced scenes: their records nearly always fit one trip)
      const bool items_done_ = !STATS && a.leaf_items != 0u &&
                               leaf_items_one_trip<!SKIP, const LeafTri<float> *>(L, lcnt, nullptr, tris + first, lane, s_item_owner[tid / kWave], s_item_rec[tid / kWave], 0u, 0xFFFFFFFFu, skip, false);
      if (!items_done_)
      for (uint32_t k = 0; __ballot(k < lcnt) != 0ull; k += 2u) { // (k_scene_trace's loop, with the counters: as ONE function it costs this kernel two registers)
        if (STATS) {
          st[6]++;
          st[7] += (unsigned)__builtin_popcountll(__ballot(k < lcnt));
        }
        if (k < lcnt) {
          const bool two = k + 1u < lcnt;
          const LeafTri<float> t0 = load_global_record(tris + first + k);
          const LeafTri<float> t1 = load_global_record(tris + first + (two ? k + 1u : k));
          tri_test<float, !SKIP>(L, t0, true, 0u, 0xFFFFFFFFu, skip, false); // default trace options (nanosg.h:817); SKIP: but for skip_prim_id
          tri_test<float, !SKIP>(L, t1, two, 0u, 0xFFFFFFFFu, skip, false);
        }
      }
      // occlusion query: any accepted primitive settles this instance — drop what is left of ITS part of the stack
      if constexpr (ANY) sp = (state == W_LEAF && L.hit_t < L.max_t) ? base : sp;
      state = (state == W_LEAF) ? W_POP : state;
      if (STATS) st[12] += clock64() - c2_;
    }
  }
  if (STATS && lane == 0 && a.counters) {
#pragma unroll
    for (int q = 0; q < 13; q++) atomicAdd(&a.counters[q], st[q]);
  }
}

hipError_t launch_scene_walk(const SceneWalkArgs &args, unsigned grid, hipStream_t s) {
  if (args.n == 0) return hipSuccess;
#ifdef NRT_PROF
  if (args.counters) {
    hipLaunchKernelGGL((k_scene_walk<kSceneWalkLdsStack, true>), dim3(grid), dim3(kTraverseBlock), 0, s, args);
    return hipGetLastError();
  }
#endif
  NRT_RANGE("scene walk launch (k_scene_walk)");
  if (args.skip && args.any_hit)
    hipLaunchKernelGGL((k_scene_walk<kSceneWalkLdsStack, false, true, true, true>), dim3(grid), dim3(kTraverseBlock), 0, s, args);
  else if (args.skip)
    hipLaunchKernelGGL((k_scene_walk<kSceneWalkLdsStack, false, false, true, true>), dim3(grid), dim3(kTraverseBlock), 0, s, args);
  else if (args.masked && args.any_hit)
    hipLaunchKernelGGL((k_scene_walk<kSceneWalkLdsStack, false, true, true>), dim3(grid), dim3(kTraverseBlock), 0, s, args);
  else if (args.masked)
    hipLaunchKernelGGL((k_scene_walk<kSceneWalkLdsStack, false, false, true>), dim3(grid), dim3(kTraverseBlock), 0, s, args);
  else if (args.any_hit)
    hipLaunchKernelGGL((k_scene_walk<kSceneWalkLdsStack, false, true>), dim3(grid), dim3(kTraverseBlock), 0, s, args);
  else
    hipLaunchKernelGGL((k_scene_walk<kSceneWalkLdsStack, false>), dim3(grid), dim3(kTraverseBlock), 0, s, args);
  return hipGetLastError();
}
int scene_walk_blocks_per_cu() { return resident_blocks((const void *)k_scene_walk<kSceneWalkLdsStack, false>, 3); }

} // namespace nrt

// ---- the listing kernels: which instances does a ray enter (BVHAccel::ListNodeIntersections, nanort.h:2608-2692) --------------
namespace {

using nrt::kMaxList, nrt::kTopStack, nrt::NodeDev;

// nrt::scene_node_interval (common.h) on an instance's world box, behind a function that is NOT forced inline, and for that alone:
// called directly, the listing kernels take 14-19 registers more and lose a wave or two per SIMD (profiles/scene_kernels_split_resources.md).
__device__ inline bool node_interval(const nrt_ray_f32 &r, const NodeDev &nd, float &t_min_out) {
  return nrt::scene_node_interval(r, nd.xbmin, nd.xbmax, t_min_out);
}

// A ray's candidate list while it is being collected: UNSORTED, at most `cap` entries — the cap nearest by (entry distance,
// node id), which is what BVHAccel::ListNodeIntersections keeps (nanort.h:2608-2692: a priority queue of kMaxIntersections).
// Adding a candidate is one store; only a ray that enters more than `cap` boxes pays for finding the farthest entry to
// replace.  k_scene_trace picks the candidates in (distance, id) order as it needs them (round 2 kept the list sorted by
// insertion in global memory: most of the listing kernel's time).
struct ListTail {
  uint32_t cnt = 0;
  bool far_known = false; // far_* describe the farthest entry of a full list
  float far_t = 0.0f;
  uint32_t far_id = 0, far_pos = 0;
};
__device__ inline void list_farthest(ListTail &st, uint32_t cap, const float *list_t, const uint32_t *list_node, uint32_t n, uint32_t i) {
  st.far_t = list_t[i];
  st.far_id = list_node[i];
  st.far_pos = 0;
  for (uint32_t q = 1; q < cap; q++) {
    const float qt = list_t[(size_t)q * n + i];
    const uint32_t qk = list_node[(size_t)q * n + i];
    if (qt > st.far_t || (qt == st.far_t && qk > st.far_id)) {
      st.far_t = qt;
      st.far_id = qk;
      st.far_pos = q;
    }
  }
  st.far_known = true;
}
__device__ inline void list_add(ListTail &st, float t, uint32_t k, uint32_t cap, float *__restrict__ list_t,
                                uint32_t *__restrict__ list_node, uint32_t n, uint32_t i) {
  if (st.cnt < cap) {
    list_t[(size_t)st.cnt * n + i] = t;
    list_node[(size_t)st.cnt * n + i] = k;
    st.cnt++;
    return;
  }
  if (!st.far_known) list_farthest(st, cap, list_t, list_node, n, i);
  if (t < st.far_t || (t == st.far_t && k < st.far_id)) { // nearer than the farthest kept: takes its place
    list_t[(size_t)st.far_pos * n + i] = t;
    list_node[(size_t)st.far_pos * n + i] = k;
    st.far_known = false;
  }
}

// MASKED, in all three listing kernels: instance visibility masks (`inst_masks`: one word per instance by id; `ray_masks`: one word
// per ray, indexed like `rays`, or null = 0xFFFFFFFF).  Wherever an instance's box would be accepted as entered, the acceptance is
// ANDed with (inst word & ray word) != 0: a hidden instance is never ADDED, so it takes no place among the `cap` nearest and the
// pruning walk's "full list" is a list of visible entries.  Subtree pruning is untouched: the tree only prunes.
__device__ __forceinline__ uint32_t list_ray_word(const uint32_t *ray_masks, uint32_t ray) { return ray_masks ? ray_masks[ray] : 0xFFFFFFFFu; }

// list_t / list_node: [kMaxList or num_nodes][n] (entry-major, so lane-consecutive accesses coalesce)
template <bool MASKED = false>
__global__ __launch_bounds__(256) void k_scene_list(const nrt_ray_f32 *__restrict__ rays, uint32_t n,
                                                    const NodeDev *__restrict__ nodes, uint32_t num_nodes, uint32_t cap,
                                                    float *__restrict__ list_t, uint32_t *__restrict__ list_node,
                                                    uint32_t *__restrict__ count, const uint32_t *__restrict__ subset,
                                                    const uint32_t *__restrict__ inst_masks, const uint32_t *__restrict__ ray_masks) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const nrt_ray_f32 r = rays[subset ? subset[i] : i]; // (a subset launch lists rays[subset[i]] into slot i of n)
  uint32_t rm = 0xFFFFFFFFu;
  if constexpr (MASKED) rm = list_ray_word(ray_masks, subset ? subset[i] : i);
  ListTail st;
  for (uint32_t k = 0; k < num_nodes; k++) {
    float t;
    if constexpr (MASKED) {
      if ((inst_masks[k] & rm) == 0u) continue;
    }
    if (!node_interval(r, nodes[k], t)) continue;
    list_add(st, t, k, cap, list_t, list_node, n, i);
  }
  count[i] = st.cnt;
}

// The same listing through the top-level BVH: reference-format nodes over the instances' world boxes, leaves name the
// instances through `top_indices`.  Inner boxes are tested as ListNodeIntersections tests them (IntersectRayAABB with
// hit_t == ray.max_t throughout, nanort.h:2651), leaves with node_interval; entries are kept sorted by (entry distance,
// node id) — the order the scan above produces — whatever order the walk finds them in.
__device__ inline bool top_box_hit(const nrt_ray_f32 &r, const float inv[3], const int sign[3], const float bmin[3], const float bmax[3]) {
  float tmin = r.min_t, tmax = r.max_t;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float lo = sign[k] ? bmax[k] : bmin[k], hi = sign[k] ? bmin[k] : bmax[k];
    const float t0 = (lo - r.org[k]) * inv[k];
    const float t1 = (hi - r.org[k]) * inv[k] * 1.00000024f;
    tmin = (t0 > tmin) ? t0 : tmin;
    tmax = (t1 < tmax) ? t1 : tmax;
  }
  return tmin <= tmax;
}

template <bool MASKED = false>
__global__ __launch_bounds__(256) void k_scene_list_bvh(const nrt_ray_f32 *__restrict__ rays, uint32_t n,
                                                        const nrt_node_f32 *__restrict__ top_nodes,
                                                        const uint32_t *__restrict__ top_indices,
                                                        const NodeDev *__restrict__ nodes, uint32_t cap,
                                                        float *__restrict__ list_t, uint32_t *__restrict__ list_node,
                                                        uint32_t *__restrict__ count, const uint32_t *__restrict__ subset,
                                                        const uint32_t *__restrict__ inst_masks, const uint32_t *__restrict__ ray_masks) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const nrt_ray_f32 r = rays[subset ? subset[i] : i];
  uint32_t rm = 0xFFFFFFFFu;
  if constexpr (MASKED) rm = list_ray_word(ray_masks, subset ? subset[i] : i);
  float inv[3];
  int sign[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float d = r.dir[k];
    sign[k] = d < 0.0f ? 1 : 0;
    inv[k] = (__builtin_fabsf(d) < 1.1920928955078125e-07f) ? __builtin_huge_valf() * (sign[k] ? -1.0f : 1.0f) : 1.0f / d;
  }
  uint32_t stack[kTopStack];
  int sp = 0;
  stack[0] = 0u;
  ListTail st;
  while (sp >= 0) {
    const nrt_node_f32 nd = top_nodes[stack[sp]];
    sp--;
    if (!top_box_hit(r, inv, sign, nd.bmin, nd.bmax)) continue;
    if (nd.flag == 0) {
      const int near = sign[nd.axis];
      stack[++sp] = nd.data[1 - near];
      stack[++sp] = nd.data[near];
      continue;
    }
    for (uint32_t q = 0; q < nd.data[0]; q++) {
      const uint32_t k = top_indices[nd.data[1] + q];
      float t;
      if constexpr (MASKED) {
        if ((inst_masks[k] & rm) == 0u) continue;
      }
      if (!node_interval(r, nodes[k], t)) continue;
      list_add(st, t, k, cap, list_t, list_node, n, i);
    }
  }
  count[i] = st.cnt;
}

// The same listing through the top-level tree's Wide4Node records (two tree levels per 128-byte fetch: a third of the
// dependent round trips of the walk above).  Which instances a ray lists does not depend on the walk: an instance is listed iff
// node_interval passes on its world box, and the tree only prunes — a subtree is skipped when the ray misses its box by the
// same IntersectRayAABB arithmetic, and a box that contains an entered box is entered (the slab arithmetic is monotone), so
// testing the four grandchild boxes instead of child-then-grandchild prunes the same subtrees.  A leaf of one instance needs
// no fetch at all: its slot's box IS the instance's world box (the builder's box of the zero-radius cylinder xbmin -> xbmax).
// PRUNE: keep entry distances on the stack, walk front to back and skip what lies beyond a full list (scenes of many
// instances, where rays enter more boxes than the list holds; on smaller scenes the bookkeeping costs 5-10 % and buys nothing).
// (MASKED: the leaf of one instance, listed from its slot's box, has to fetch that instance's word.)
template <bool PRUNE, bool MASKED = false>
__global__ __launch_bounds__(256) void k_scene_list_w4(const nrt_ray_f32 *__restrict__ rays, uint32_t n,
                                                       const nrt::Wide4Node<float> *__restrict__ wide4,
                                                       const nrt_node_f32 *__restrict__ top_nodes, uint32_t packed_leaves,
                                                       const uint32_t *__restrict__ top_indices,
                                                       const NodeDev *__restrict__ nodes, uint32_t cap,
                                                       float *__restrict__ list_t, uint32_t *__restrict__ list_node,
                                                       uint32_t *__restrict__ count, const uint32_t *__restrict__ subset,
                                                       const uint32_t *__restrict__ inst_masks, const uint32_t *__restrict__ ray_masks) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const nrt_ray_f32 r = rays[subset ? subset[i] : i];
  uint32_t rm = 0xFFFFFFFFu;
  if constexpr (MASKED) rm = list_ray_word(ray_masks, subset ? subset[i] : i);
  float inv[3], pinv[3];
  int sign[3];
  bool tame = PRUNE; // every direction component is an ordinary non-zero number and the origin is finite: entry distances are monotone in the box
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float d = r.dir[k];
    sign[k] = d < 0.0f ? 1 : 0;
    inv[k] = (__builtin_fabsf(d) < 1.1920928955078125e-07f) ? __builtin_huge_valf() * (sign[k] ? -1.0f : 1.0f) : 1.0f / d;
    pinv[k] = 1.0f / d; // NodeBBoxIntersector's plain reciprocal (nanosg.h:603-639)
    tame = tame && (__builtin_fabsf(d) >= 1.1920928955078125e-07f) && (__builtin_fabsf(pinv[k]) < __builtin_huge_valf()) &&
           (__builtin_fabsf(r.org[k]) < __builtin_huge_valf());
  }
  // entry distance of a box as node_interval computes it for an instance's box (unclipped, plain reciprocal): for a tame ray
  // it can only grow from a box to a box inside it, so a subtree whose box is entered beyond the farthest entry of a FULL
  // list holds nothing that could still make the list — the walk skips it (a ray through 100 000 instances lists its 64
  // nearest without visiting the rest)
  auto entry = [&](const float bmin[3], const float bmax[3]) -> float {
    float a = -__builtin_huge_valf();
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float lo = sign[k] ? bmax[k] : bmin[k];
      const float t = (lo - r.org[k]) * pinv[k];
      a = (t > a) ? t : a;
    }
    return a;
  };
  uint32_t stack[kTopStack];
  float stack_t[PRUNE ? kTopStack : 1]; // entry distance of the pushed record's box (tame rays; else unused)
  int sp = 0;
  stack[0] = 0u; // record 0 == the root branch
  stack_t[0] = -__builtin_huge_valf();
  sp = 1;
  ListTail st;
  while (sp > 0) {
    sp--;
    if constexpr (PRUNE) {
      if (tame && st.cnt == cap) { // the list is full: anything entered beyond its farthest entry cannot get in
        if (!st.far_known) list_farthest(st, cap, list_t, list_node, n, i);
        if (stack_t[sp] > st.far_t) continue;
      }
    }
    const nrt::Wide4Node<float> w = wide4[stack[sp]];
    uint32_t in_ref[4];
    float in_t[4];
    int nin = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t cj = w.c[j];
      if (cj == nrt::kWide4Empty) continue;
      const float bmin[3] = {w.bmin[0][j], w.bmin[1][j], w.bmin[2][j]}, bmax[3] = {w.bmax[0][j], w.bmax[1][j], w.bmax[2][j]};
      if (!(cj & nrt::kLeafBit)) {
        if (top_box_hit(r, inv, sign, bmin, bmax)) {
          in_ref[nin] = cj;
          in_t[nin] = PRUNE ? entry(bmin, bmax) : 0.0f;
          nin++;
        }
        continue;
      }
      uint32_t lcount, lfirst;
      nrt::leaf_span(packed_leaves, top_nodes, cj & ~nrt::kLeafBit, lcount, lfirst);
      for (uint32_t q = 0; q < lcount; q++) {
        const uint32_t k = top_indices[lfirst + q];
        float t;
        if constexpr (MASKED) {
          if ((inst_masks[k] & rm) == 0u) continue;
        }
        if (lcount == 1u) {
          if (!nrt::scene_node_interval(r, bmin, bmax, t)) continue;
        } else if (!node_interval(r, nodes[k], t)) {
          continue;
        }
        list_add(st, t, k, cap, list_t, list_node, n, i);
      }
    }
    // nearest box on top of the stack: the walk runs roughly front to back, the list fills with near entries first and the
    // far subtrees fall to the test above (insertion sort of at most four entries, farthest first)
    for (int x = 1; PRUNE && x < nin; x++)
      for (int y = x; y > 0 && in_t[y] > in_t[y - 1]; y--) {
        const float tt = in_t[y];
        in_t[y] = in_t[y - 1];
        in_t[y - 1] = tt;
        const uint32_t rr = in_ref[y];
        in_ref[y] = in_ref[y - 1];
        in_ref[y - 1] = rr;
      }
    for (int x = 0; x < nin; x++) {
      stack[sp] = in_ref[x];
      if constexpr (PRUNE) stack_t[sp] = in_t[x];
      sp++;
    }
  }
  count[i] = st.cnt;
}

} // namespace

namespace nrt {

hipError_t launch_scene_list(SceneListForm form, const TreeViewF32 &top, const nrt_ray_f32 *rays, uint32_t n, const NodeDev *nodes, uint32_t num_nodes,
                             uint32_t cap, float *list_t, uint32_t *list_node, uint32_t *count, const uint32_t *subset, const uint32_t *inst_masks,
                             const uint32_t *ray_masks, hipStream_t s) {
  const dim3 grid((n + 255u) / 256u), block(256); // one ray per thread
  const Wide4Node<float> *wide4 = (const Wide4Node<float> *)top.wide4;
  const bool masked = inst_masks != nullptr; // (the unmasked instantiations read neither array)
#define NRT_LIST_W4(K) hipLaunchKernelGGL(K, grid, block, 0, s, rays, n, wide4, top.nodes, top.packed_leaves, top.indices, nodes, cap, list_t, list_node, count, subset, inst_masks, ray_masks)
#define NRT_LIST_BVH(K) hipLaunchKernelGGL(K, grid, block, 0, s, rays, n, top.nodes, top.indices, nodes, cap, list_t, list_node, count, subset, inst_masks, ray_masks)
#define NRT_LIST_SCAN(K) hipLaunchKernelGGL(K, grid, block, 0, s, rays, n, nodes, num_nodes, cap, list_t, list_node, count, subset, inst_masks, ray_masks)
  switch (form) {
    case kSceneListW4Prune:
      if (masked) NRT_LIST_W4((k_scene_list_w4<true, true>));
      else NRT_LIST_W4((k_scene_list_w4<true, false>));
      break;
    case kSceneListW4:
      if (masked) NRT_LIST_W4((k_scene_list_w4<false, true>));
      else NRT_LIST_W4((k_scene_list_w4<false, false>));
      break;
    case kSceneListBvh:
      if (masked) NRT_LIST_BVH(k_scene_list_bvh<true>);
      else NRT_LIST_BVH(k_scene_list_bvh<false>);
      break;
    case kSceneListScan:
      if (masked) NRT_LIST_SCAN(k_scene_list<true>);
      else NRT_LIST_SCAN(k_scene_list<false>);
      break;
  }
#undef NRT_LIST_W4
#undef NRT_LIST_BVH
#undef NRT_LIST_SCAN
  return hipGetLastError();
}

} // namespace nrt
