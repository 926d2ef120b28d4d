// nanort_amd/csrc/scene_closest.hip — the closest-point query on an instanced scene for gfx950: which face of which node of the
// committed scene is nearest to a point, and where on it (include/nanort_hip.h, "closest-point queries on scenes").
//
// The rule is include/nanort_closest.h's: a face of an instance is the triangle of the three XformPoint images of its local
// vertices, ClosestPointOnTriangle of the world point against it, and the answer a minimum over all (node, face) pairs with a total
// tie-break (BetterInScene: dist2, node_id, prim_id) — so the answer depends neither on the trees nor on the order of the nodes'
// boxes, and the walk below only decides which faces need not be looked at.  A subtree is skipped iff the BoxDist2 of its WORLD box
// is strictly greater than the best dist2 so far (Culled): the world box of an instance (what Commit stores), the boxes of the
// top-level tree over those, and inside an instance XformBox of a node's local box, which contains the XformPoint image of every
// vertex in it, in floating point.  No inverse matrix is read.
//
// k_scene_closest_point<STACK> is closest_walk (closest.hip) over two levels: one query per lane, points claimed a chunk per wave and
// handed to idle lanes by ballot rank, the lane's stack in LDS with the launch's overflow area behind it (LaneStack), inner steps
// until a lane reaches a leaf of an instance, the leaves of the whole wave together, then pop or finish.
//   * A stack entry is a node index of the level it was pushed at, or — bit 31 set — an instance id.  BOTH LEVELS SHARE THE STACK: on
//     entering an instance the lane remembers the stack's height (`base`); entries above it are nodes of the instance's tree, and a
//     pop at that height returns the lane to the top level, whose entries lie below.
//   * Top level.  With a top-level tree (args.top_nodes) its reference-format nodes are walked as closest_walk walks a mesh's — the
//     popped node's box against the current best, the nearer child first, the farther pushed unless culled — and a leaf's instances
//     become instance entries.  Without one (a handful of nodes: Commit built no tree) every instance is such an entry from the start.
//   * An instance entry is opened iff the instance is admitted (its word & the point's word, where the query carries words) and its
//     world box is not culled: the lane takes the twelve matrix entries XformPoint reads and the instance's arrays, and walks its
//     reference-format nodes from node 0 in the same way, each box through XformBox.
//   * A lane tests its leaf's LeafTri<float> records in leaf order: three XformPoint, ClosestPointOnTriangle, BetterInScene.
//   * A point that is not Searchable takes its not-found record at the refill and walks nothing.
// No inline assembly; the instance's arrays are read through global-address-space pointers (load_global_record), the records are
// stored as two 16-byte non-temporal pieces (as closest.hip's store_closest_record).
// The profiling library (-DNRT_PROF) counts nodes opened, instances entered and triangles tested into args.counters[0..2]
// (tools/scene_closest_probe.py).
#include "kernels.h"
#include "walk_dev.h" // (traverse_dev.h: LaneStack, the lane states, launch_persistent; load_global_record)
#include "../../include/nanort_closest.h"

namespace nrt {


// (The lane's answer as scalars: held in a struct passed here by reference, seven of its words stayed in scratch.)
__device__ __forceinline__ void store_scene_closest_record(const SceneClosestArgs &a, uint32_t rid, float q0, float q1, float q2, float dist2, float u, float v,
                                                           uint32_t prim, uint32_t node) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  static_assert(offsetof(nrt_scene_closest_f32, dist2) == 12 && offsetof(nrt_scene_closest_f32, u) == 16 && offsetof(nrt_scene_closest_f32, prim_id) == 24 &&
                    offsetof(nrt_scene_closest_f32, node_id) == 28, "the record as two 16-byte pieces");
  const u32x4 lo = {__float_as_uint(q0), __float_as_uint(q1), __float_as_uint(q2), __float_as_uint(dist2)}; // point, dist2
  const u32x4 hi = {__float_as_uint(u), __float_as_uint(v), prim, node};                                     // u, v, prim_id, node_id
  u32x4 NRT_GLOBAL *dst = (u32x4 NRT_GLOBAL *)(a.out + rid); // 32-byte records of a 16-byte aligned array
  __builtin_nontemporal_store(lo, dst);
  __builtin_nontemporal_store(hi, dst + 1);
  if (a.found) a.found[rid] = prim != kInvalid ? 1 : 0;
}

// BoxDist2 of a node's box as the lane's level sees it: a top-level box is a world box, an instance's is carried there by XformBox.
__device__ __forceinline__ float scene_box_dist2(bool top, const float (&m)[4][3], const float p[3], const float bmin[3], const float bmax[3]) {
  if (top) return nanort_closest::BoxDist2<float>(p, bmin, bmax); // (`m` is not the box's: no instance is open)
  float wmin[3], wmax[3];
  nanort_closest::XformBox<float, 3>(m, bmin, bmax, wmin, wmax);
  return nanort_closest::BoxDist2<float>(p, wmin, wmax);
}

// The next chunk of points for the wave: [next, end), or false when every partition is drained.  One counter of CHUNKS per
// partition (a.cursor), the wave's home partition first, then the others; all lanes call it, `leader` is any active lane.
struct SceneClosestClaim {
  uint32_t next, end;
  uint32_t part, tried;
  bool exhausted;
};
__device__ __forceinline__ bool scene_closest_claim(const SceneClosestArgs &a, SceneClosestClaim &c, unsigned lane, int leader) {
  const uint32_t chunks = (a.n + kSceneClosestChunk - 1u) / kSceneClosestChunk, per = (chunks + a.num_parts - 1u) / a.num_parts;
  while (c.tried < a.num_parts) {
    const uint32_t lo = c.part * per, hi = lo + per < chunks ? lo + per : chunks;
    uint32_t idx = 0;
    if (lane == (unsigned)leader) idx = atomicAdd(a.cursor + kCursorStrideWords * c.part, 1u);
    idx = __builtin_amdgcn_readfirstlane(__shfl(idx, leader));
    if (lo < hi && idx < hi - lo) {
      c.next = (lo + idx) * kSceneClosestChunk;
      c.end = c.next + kSceneClosestChunk < a.n ? c.next + kSceneClosestChunk : a.n;
      return true;
    }
    c.part = (c.part + 1u == a.num_parts) ? 0u : c.part + 1u;
    c.tried++;
  }
  c.exhausted = true;
  return false;
}

template <int STACK>
__global__ __launch_bounds__(kTraverseBlock) void k_scene_closest_point(const SceneClosestArgs a) {
  __shared__ uint32_t s_stack[STACK][kTraverseBlock];
  const unsigned tid = threadIdx.x;
  const unsigned lane = lane_id();
  const LaneStack<StackRef, STACK, SceneClosestArgs> stk = {a, tid, blockIdx.x * kTraverseBlock + tid};

  // the lane's query and its best answer so far (best: r2 until a face is accepted)
  float L_p0 = 0.0f, L_p1 = 0.0f, L_p2 = 0.0f, L_best = 0.0f, L_q0 = 0.0f, L_q1 = 0.0f, L_q2 = 0.0f, L_u = 0.0f, L_v = 0.0f;
  uint32_t L_prim = kInvalid, L_node = kInvalid;
  // the open instance: the entries of its xform that XformPoint reads, its tree, its id
  float m[4][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
  const nrt_node_f32 *inst_nodes = nullptr;
  const LeafTri<float> *inst_tris = nullptr;
  uint32_t inst = kInvalid;
  uint32_t rid = kInvalid;
  uint32_t cur = 0;
  uint32_t leaf_first = 0, leaf_cnt = 0;
  int state = LANE_IDLE;
  int sp = 0;
  int base = -1; // the stack's height when the open instance was entered; -1: the lane is at the top level
#ifdef NRT_PROF
  unsigned long long n_nodes = 0ull, n_insts = 0ull, n_tris = 0ull;
#endif

  SceneClosestClaim ck;
  ck.next = ck.end = 0u;
  ck.part = blockIdx.x % a.num_parts;
  ck.tried = 0u;
  ck.exhausted = false;

  // Pop the next entry, or finish the query when the stack is empty.  A pop at the height the open instance was entered at leaves
  // the instance: what lies below are top-level entries.  The popped entry's box is tested when it is opened, against the best of
  // that moment.
#define NRT_SCENE_CLOSEST_POP_OR_FINISH()                 \
  do {                                                    \
    base = sp == base ? -1 : base;                        \
    const bool fin_ = sp == 0;                            \
    if (fin_) store_scene_closest_record(a, rid, L_q0, L_q1, L_q2, L_best, L_u, L_v, L_prim, L_node);      \
    if (!fin_) stk.load(s_stack, sp - 1, cur);            \
    sp = fin_ ? 0 : sp - 1;                               \
    rid = fin_ ? kInvalid : rid;                          \
    state = fin_ ? LANE_IDLE : LANE_TRAV;                 \
  } while (0)

  for (;;) {
    // ---- hand new points to idle lanes (ballot rank inside the wave's chunk) ----
    unsigned long long idle = __ballot(state == LANE_IDLE);
    if (!ck.exhausted && (unsigned)__builtin_popcountll(idle) >= a.refill_min) {
      while (idle != 0ull && !ck.exhausted) {
        if (ck.next == ck.end && !scene_closest_claim(a, ck, lane, __builtin_ctzll(idle))) break;
        const unsigned want = (unsigned)__builtin_popcountll(idle);
        const unsigned avail = ck.end - ck.next;
        const unsigned take = want < avail ? want : avail;
        const unsigned rank = (unsigned)__builtin_popcountll(idle & ((1ull << lane) - 1ull));
        if (state == LANE_IDLE && rank < take) {
          rid = ck.next + rank;
          const nrt_point_f32 pt = a.points[rid];
          const float p[3] = {pt.p[0], pt.p[1], pt.p[2]};
          L_p0 = p[0], L_p1 = p[1], L_p2 = p[2];
          L_best = pt.max_dist * pt.max_dist; // r2
          L_q0 = p[0], L_q1 = p[1], L_q2 = p[2];
          L_u = 0.0f, L_v = 0.0f;
          L_prim = kInvalid, L_node = kInvalid;
          if (nanort_closest::Searchable<float>(p, pt.max_dist)) {
            sp = 0;
            base = -1;
            if (a.top_nodes) {
              cur = 0;
            } else { // every instance is an entry, the first on top
              for (uint32_t k = a.num_insts - 1u; k > 0u; k--) {
                stk.store(s_stack, sp, kLeafBit | k);
                sp++;
              }
              cur = kLeafBit;
            }
            state = LANE_TRAV;
          } else { // finds nothing and walks nothing: the lane stays idle and takes another point
            store_scene_closest_record(a, rid, L_q0, L_q1, L_q2, L_best, L_u, L_v, L_prim, L_node);
            rid = kInvalid;
          }
        }
        ck.next += take;
        idle = __ballot(state == LANE_IDLE);
      }
    }
    if (idle == ~0ull) {
      if (ck.exhausted) break;
      continue;
    }

    // ---- phase 1: instance entries and inner nodes of both levels, until this lane reaches a leaf of an instance or finishes ----
    while (state == LANE_TRAV) {
      const float p[3] = {L_p0, L_p1, L_p2};
      const bool top = base < 0;
      if (top && (cur & kLeafBit) != 0u) { // an instance: admitted, and its world box not culled?
        const uint32_t id = cur & ~kLeafBit;
        const SceneInst *e = a.insts + id;
        bool open = true;
        if (a.node_masks) open = (a.node_masks[id] & (a.point_masks ? a.point_masks[rid] : 0xFFFFFFFFu)) != 0u;
        if (open) {
          const float xbmin[3] = {e->xbmin[0], e->xbmin[1], e->xbmin[2]}, xbmax[3] = {e->xbmax[0], e->xbmax[1], e->xbmax[2]};
          open = !nanort_closest::Culled<float>(nanort_closest::BoxDist2<float>(p, xbmin, xbmax), L_best);
        }
        if (open) {
#pragma unroll
          for (int r = 0; r < 4; r++)
#pragma unroll
            for (int k = 0; k < 3; k++) m[r][k] = e->xform[r][k];
          inst_nodes = e->nodes;
          inst_tris = (const LeafTri<float> *)e->tris;
          inst = id;
          base = sp;
          cur = 0;
#ifdef NRT_PROF
          n_insts++;
#endif
        } else {
          NRT_SCENE_CLOSEST_POP_OR_FINISH();
        }
      } else { // a node of the level's tree
        const nrt_node_f32 *nodes = top ? a.top_nodes : inst_nodes;
        const nrt_node_f32 nd = load_global_record(nodes + cur);
#ifdef NRT_PROF
        n_nodes++;
#endif
        if (!nanort_closest::Culled<float>(scene_box_dist2(top, m, p, nd.bmin, nd.bmax), L_best)) {
          if (nd.flag == 0) {
            const uint32_t c0 = nd.data[0], c1 = nd.data[1];
            const nrt_node_f32 n0 = load_global_record(nodes + c0);
            const nrt_node_f32 n1 = load_global_record(nodes + c1);
            const float d0 = scene_box_dist2(top, m, p, n0.bmin, n0.bmax), d1 = scene_box_dist2(top, m, p, n1.bmin, n1.bmax);
            const bool second = d1 < d0; // on ties (and NaN) the first child
            const uint32_t near_child = second ? c1 : c0, far_child = second ? c0 : c1;
            const float d_near = second ? d1 : d0, d_far = second ? d0 : d1;
            if (!nanort_closest::Culled<float>(d_far, L_best)) {
              stk.store(s_stack, sp, far_child);
              sp++;
            }
            if (!nanort_closest::Culled<float>(d_near, L_best)) {
              cur = near_child;
            } else {
              NRT_SCENE_CLOSEST_POP_OR_FINISH();
            }
          } else if (top) { // a leaf of the top-level tree: its instances become entries, the first is opened next
            const uint32_t cnt = nd.data[0], first = nd.data[1];
            for (uint32_t k = cnt; k > 1u; k--) {
              stk.store(s_stack, sp, kLeafBit | a.top_indices[first + k - 1u]);
              sp++;
            }
            if (cnt != 0u) {
              cur = kLeafBit | a.top_indices[first];
            } else {
              NRT_SCENE_CLOSEST_POP_OR_FINISH();
            }
          } else {
            leaf_cnt = nd.data[0];
            leaf_first = nd.data[1];
            state = LANE_LEAF;
          }
        } else {
          NRT_SCENE_CLOSEST_POP_OR_FINISH();
        }
      }
      if ((unsigned)__builtin_popcountll(__ballot(state == LANE_TRAV)) < a.trav_min) break;
    }

    // ---- phase 2: lanes holding a leaf take its records together --------------------
    if (__ballot(state == LANE_LEAF) != 0ull) {
      const uint32_t cnt = state == LANE_LEAF ? leaf_cnt : 0u;
      for (uint32_t i = 0; __ballot(i < cnt) != 0ull; i++) {
        if (i < cnt) {
          const LeafTri<float> tri = load_global_record(inst_tris + leaf_first + i);
          const float p[3] = {L_p0, L_p1, L_p2};
          float wa[3], wb[3], wc[3];
          nanort_closest::XformPoint<float, 3>(m, tri.p0, wa);
          nanort_closest::XformPoint<float, 3>(m, tri.p1, wb);
          nanort_closest::XformPoint<float, 3>(m, tri.p2, wc);
          float u, v, q[3];
          const float dist2 = nanort_closest::ClosestPointOnTriangle<float>(p, wa, wb, wc, &u, &v, q);
          const bool acc = nanort_closest::BetterInScene<float>(dist2, inst, tri.prim_id, L_best, L_node, L_prim);
          L_best = acc ? dist2 : L_best;
          L_q0 = acc ? q[0] : L_q0;
          L_q1 = acc ? q[1] : L_q1;
          L_q2 = acc ? q[2] : L_q2;
          L_u = acc ? u : L_u;
          L_v = acc ? v : L_v;
          L_prim = acc ? tri.prim_id : L_prim;
          L_node = acc ? inst : L_node;
#ifdef NRT_PROF
          n_tris++;
#endif
        }
      }
      if (state == LANE_LEAF) NRT_SCENE_CLOSEST_POP_OR_FINISH();
    }
  }
#undef NRT_SCENE_CLOSEST_POP_OR_FINISH
#ifdef NRT_PROF
  if (a.counters) {
    atomicAdd(a.counters + 0, n_nodes);
    atomicAdd(a.counters + 1, n_insts);
    atomicAdd(a.counters + 2, n_tris);
  }
#endif
}

static_assert(kLdsStackDefault == 32, "the name below carries the stack depth");
static const void *scene_closest_kernel() { return (const void *)k_scene_closest_point<kLdsStackDefault>; }

hipError_t launch_scene_closest_point(const SceneClosestArgs &args, unsigned grid, hipStream_t s) {
  launch_persistent(scene_closest_kernel(), grid, args, s);
  return hipGetLastError();
}

int scene_closest_point_blocks_per_cu() { return resident_blocks(scene_closest_kernel(), 1); }

} // namespace nrt
