// nanort_amd/csrc/closest.hip — the closest-point query for gfx950: which triangle of the context's mesh is nearest to a point, and
// where on it (include/nanort_hip.h, "closest-point queries").
//
// The rule is include/nanort_closest.h's — ClosestPointOnTriangle, BoxDist2, and the answer as a minimum over the admitted
// faces with a total tie-break (smallest dist2, then smallest prim_id) — so the answer does not depend on the tree, and the walk
// below only decides which faces need not be looked at: a subtree is skipped iff the BoxDist2 of its box is strictly greater than
// the best dist2 found so far, which in floating point can hide no face at or below it.
//
// k_closest_point<T, STACK> is a persistent walk in the shape of binary_walk (binary_walk_dev.h), ordered by distance instead of
// along a ray: one query per lane, points claimed as the walks claim rays (claim_init / claim_chunk) and handed to idle lanes by
// ballot rank, the lane's stack of node indices in LDS with the launch's overflow area behind it (LaneStack), inner nodes until a
// lane reaches a leaf, the leaves of the whole wave together, then pop or finish.
//   * It reads the reference-format node array.  A step opens node `cur`: its box is tested against the CURRENT best — the test of a
//     popped entry, re-derived instead of carried on the stack (a distance beside each index would double the stack's LDS, and LDS
//     is what bounds this kernel's occupancy: DESIGN.md §3.17) — then, at a branch, both children's boxes are fetched, the nearer
//     child is entered (on ties the first) and the farther one pushed unless it is culled already.
//   * A lane tests its leaf's LeafTri<T> records in leaf order with nanort_closest::Better.  prim_ids_range and skip_prim_id of the
//     trace options are honoured as tri_solve honours them; cull_back_face means nothing here.
//   * A point that is not Searchable (a non-finite coordinate, a NaN or negative max_dist) takes its not-found record at the refill
//     and walks nothing.
// closest_walk<T, STACK, SIGNED> states that walk once, for two kernels.  k_signed_distance<T, STACK> (SIGNED; nrtSignedDistanceBatch*,
// DESIGN.md §3.18) carries the winning candidate's feature code of the best face beside its prim_id (ClosestFeatureOnTriangle) and,
// when a lane finishes a FOUND query, fetches one pseudonormal — the face's record [4][3] for features 0..3, the vertex normal of
// faces[3 * prim + feature - 4] for 4..6 — and sets bit 31 of the record's last word where nanort_sdf::Inside says so: once per
// query, not per face; the cull, the order and the tie-break are the unsigned walk's.
// No inline assembly; plain loads and stores, the records in 16-byte (fp32) and 8-byte (fp64) pieces.
// The profiling library (-DNRT_PROF) counts nodes opened and triangles tested into a.counters[0] / [2] (tools/closest_probe.py).
#include "traverse_dev.h"
#include "kernels.h"
#include "../../include/nanort_sdf.h" // (includes nanort_closest.h)

namespace nrt {

template <typename T>
struct ClosestArgs {
  TraverseArgs<T> a; // the tree, the trace options, the claim plan and the overflow stack of a launch (rays, hits, mask: unused)
  const typename ClosestWire<T>::Point *points;
  typename ClosestWire<T>::Record *out;
  uint8_t *found; // may be null
};

// A lane's query and its best answer so far.
template <typename T>
struct ClosestLane {
  T p0, p1, p2;
  T best; // r2 until a face is accepted
  T q0, q1, q2, u, v;
  uint32_t prim;
};
// ... and, in the signed walk, the feature code of that answer.
template <bool SIGNED>
struct FeatureLane {};
template <>
struct FeatureLane<true> {
  uint32_t feature;
};

template <typename T>
__device__ __forceinline__ void store_closest_record(const ClosestArgs<T> &m, const ClosestLane<T> &L, uint32_t rid, uint32_t last_word = 0u) {
  typename ClosestWire<T>::Record r;
  r.point[0] = L.q0, r.point[1] = L.q1, r.point[2] = L.q2;
  r.dist2 = L.best;
  r.u = L.u, r.v = L.v;
  r.prim_id = L.prim;
  r._pad = last_word; // (the signed record's `feature`)
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  if constexpr (sizeof(T) == 4) { // 32-byte records of a 16-byte aligned array
    const u32x4 *src = reinterpret_cast<const u32x4 *>(&r);
    u32x4 NRT_GLOBAL *dst = (u32x4 NRT_GLOBAL *)(m.out + rid);
    __builtin_nontemporal_store(src[0], dst);
    __builtin_nontemporal_store(src[1], dst + 1);
  } else { // 56-byte records of an 8-byte aligned array
    const u32x2 *src = reinterpret_cast<const u32x2 *>(&r);
    u32x2 NRT_GLOBAL *dst = (u32x2 NRT_GLOBAL *)(m.out + rid);
#pragma unroll
    for (unsigned k = 0; k < sizeof(r) / 8; k++) __builtin_nontemporal_store(src[k], dst + k);
  }
  if (m.found) m.found[rid] = L.prim != kInvalid ? 1 : 0;
}

// The `feature` word of a finished signed query: the code, and bit 31 when the point is inside (0 when nothing was found).
template <typename T>
__device__ __forceinline__ uint32_t signed_word(const SignedInputs<T> &in, const ClosestLane<T> &L, uint32_t feature) {
  if (L.prim == kInvalid || L.prim >= in.num_faces) return 0u;
  const T *n = in.face_normals + 12 * (size_t)L.prim + 3u * feature;
  if (feature >= nanort_sdf::kFeatureVertexA) {
    const uint32_t vtx = in.faces[3 * (size_t)L.prim + (feature - nanort_sdf::kFeatureVertexA)];
    if (vtx >= in.num_verts) return feature;
    n = in.vertex_normals + 3 * (size_t)vtx;
  }
  const T p[3] = {L.p0, L.p1, L.p2}, q[3] = {L.q0, L.q1, L.q2}, nn[3] = {n[0], n[1], n[2]};
  return nanort_sdf::FeatureWord<T>(p, q, nn, feature);
}

template <typename T, int STACK, bool SIGNED>
// (the arguments BY VALUE: by reference the unsigned kernel came out at 96 / 125 VGPRs instead of 82 / 122)
__device__ __forceinline__ void closest_walk(const ClosestArgs<T> m, const SignedInputs<T> sn) {
  __shared__ uint32_t s_stack[STACK][kTraverseBlock]; // (one per kernel: the walk is inlined into each)
  typedef typename Wire<T>::Node Node;
  typedef typename ClosestWire<T>::Point Point;
  const TraverseArgs<T> &a = m.a;

  const unsigned tid = threadIdx.x;
  const unsigned lane = lane_id();
  const LaneStack<StackRef, STACK, TraverseArgs<T>> stk = {a, tid, blockIdx.x * kTraverseBlock + tid};

  ClosestLane<T> L;
  FeatureLane<SIGNED> F;
  uint32_t rid = kInvalid;
  uint32_t cur = 0;
  uint32_t leaf_first = 0, leaf_cnt = 0;
  int state = LANE_IDLE;
  int sp = 0;
#ifdef NRT_PROF
  unsigned long long n_nodes = 0ull, n_tris = 0ull;
#endif

  Claim ck;
  claim_init<T>(a, ck);
  if (blockIdx.x == 0 && threadIdx.x < kMaxParts) a.next_cursor[kCursorStrideWords * threadIdx.x] = 0u;

  // Pop the next node, or finish the query when the stack is empty (select-style updates, as binary_walk's).  The popped node's box
  // is tested when the node is opened, against the best of that moment.
#define NRT_CLOSEST_STORE()                                                         \
  do {                                                                              \
    if constexpr (SIGNED) store_closest_record<T>(m, L, rid, signed_word<T>(sn, L, F.feature)); \
    else store_closest_record<T>(m, L, rid);                                        \
  } while (0)
#define NRT_CLOSEST_POP_OR_FINISH()               \
  do {                                            \
    const bool fin_ = sp == 0;                    \
    if (fin_) NRT_CLOSEST_STORE();                \
    if (!fin_) stk.load(s_stack, sp - 1, cur);    \
    sp = fin_ ? 0 : sp - 1;                       \
    rid = fin_ ? kInvalid : rid;                  \
    state = fin_ ? LANE_IDLE : LANE_TRAV;         \
  } while (0)

  for (;;) {
    // ---- hand new points to idle lanes (ballot rank inside the wave's chunk) ----
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
          const Point pt = m.points[rid];
          const T p[3] = {pt.p[0], pt.p[1], pt.p[2]};
          L.p0 = p[0], L.p1 = p[1], L.p2 = p[2];
          L.best = pt.max_dist * pt.max_dist; // r2
          L.q0 = p[0], L.q1 = p[1], L.q2 = p[2];
          L.u = T(0), L.v = T(0);
          L.prim = kInvalid;
          if constexpr (SIGNED) F.feature = 0u;
          if (nanort_closest::Searchable<T>(p, pt.max_dist)) {
            cur = 0;
            sp = 0;
            state = LANE_TRAV;
          } else { // finds nothing and walks nothing: the lane stays idle and takes another point
            NRT_CLOSEST_STORE();
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

    // ---- phase 1: inner nodes, until this lane reaches a leaf or finishes -----------
    while (state == LANE_TRAV) {
      const Node nd = a.nodes[cur];
      const T p[3] = {L.p0, L.p1, L.p2};
#ifdef NRT_PROF
      n_nodes++;
#endif
      if (!nanort_closest::Culled<T>(nanort_closest::BoxDist2<T>(p, nd.bmin, nd.bmax), L.best)) {
        if (nd.flag == 0) {
          const uint32_t c0 = nd.data[0], c1 = nd.data[1];
          const Node n0 = a.nodes[c0];
          const Node n1 = a.nodes[c1];
          const T d0 = nanort_closest::BoxDist2<T>(p, n0.bmin, n0.bmax), d1 = nanort_closest::BoxDist2<T>(p, n1.bmin, n1.bmax);
          const bool second = d1 < d0; // on ties (and NaN) the first child
          const uint32_t near_child = second ? c1 : c0, far_child = second ? c0 : c1;
          const T d_near = second ? d1 : d0, d_far = second ? d0 : d1;
          if (!nanort_closest::Culled<T>(d_far, L.best)) {
            stk.store(s_stack, sp, far_child);
            sp++;
          }
          if (!nanort_closest::Culled<T>(d_near, L.best)) {
            cur = near_child;
          } else {
            NRT_CLOSEST_POP_OR_FINISH();
          }
        } else {
          leaf_cnt = nd.data[0];
          leaf_first = nd.data[1];
          state = LANE_LEAF;
        }
      } else {
        NRT_CLOSEST_POP_OR_FINISH();
      }
      if ((unsigned)__builtin_popcountll(__ballot(state == LANE_TRAV)) < a.trav_min) break;
    }

    // ---- phase 2: lanes holding a leaf take its records together --------------------
    if (__ballot(state == LANE_LEAF) != 0ull) {
      const uint32_t cnt = state == LANE_LEAF ? leaf_cnt : 0u;
      for (uint32_t i = 0; __ballot(i < cnt) != 0ull; i++) {
        if (i < cnt) {
          const LeafTri<T> tri = a.tris[leaf_first + i];
          const uint32_t prim = tri.prim_id;
          if ((prim >= a.range0) & (prim < a.range1) & (prim != a.skip_prim)) { // (as tri_solve: nanort.h:2387-2395)
            const T p[3] = {L.p0, L.p1, L.p2};
            T u, v, q[3];
            uint32_t feature = 0u;
            T dist2;
            if constexpr (SIGNED) dist2 = nanort_closest::ClosestFeatureOnTriangle<T>(p, tri.p0, tri.p1, tri.p2, &u, &v, q, &feature);
            else dist2 = nanort_closest::ClosestPointOnTriangle<T>(p, tri.p0, tri.p1, tri.p2, &u, &v, q);
            const bool acc = nanort_closest::Better<T>(dist2, prim, L.best, L.prim);
            L.best = acc ? dist2 : L.best;
            L.q0 = acc ? q[0] : L.q0;
            L.q1 = acc ? q[1] : L.q1;
            L.q2 = acc ? q[2] : L.q2;
            L.u = acc ? u : L.u;
            L.v = acc ? v : L.v;
            L.prim = acc ? prim : L.prim;
            if constexpr (SIGNED) F.feature = acc ? feature : F.feature;
#ifdef NRT_PROF
            n_tris++;
#endif
          }
        }
      }
      if (state == LANE_LEAF) NRT_CLOSEST_POP_OR_FINISH();
    }
  }
#undef NRT_CLOSEST_POP_OR_FINISH
#undef NRT_CLOSEST_STORE
#ifdef NRT_PROF
  if (a.counters) {
    atomicAdd(a.counters + 0, n_nodes);
    atomicAdd(a.counters + 2, n_tris);
  }
#endif
}

template <typename T, int STACK>
__global__ __launch_bounds__(kTraverseBlock) void k_closest_point(const ClosestArgs<T> m) {
  const SignedInputs<T> none = {};
  closest_walk<T, STACK, false>(m, none);
}

template <typename T>
struct SignedArgs {
  ClosestArgs<T> m;
  SignedInputs<T> in;
};
template <typename T, int STACK>
__global__ __launch_bounds__(kTraverseBlock) void k_signed_distance(const SignedArgs<T> sa) {
  closest_walk<T, STACK, true>(sa.m, sa.in);
}

static_assert(kLdsStackDefault == 32, "the names below carry the stack depth");
template <typename T>
static const void *closest_kernel() {
  return (const void *)k_closest_point<T, kLdsStackDefault>;
}

template <typename T>
hipError_t launch_closest_point(const TraverseArgs<T> &args, const void *points, void *out, uint8_t *found, unsigned grid, hipStream_t s,
                                const char **name_out) {
  ClosestArgs<T> m;
  m.a = args;
  m.points = (const typename ClosestWire<T>::Point *)points;
  m.out = (typename ClosestWire<T>::Record *)out;
  m.found = found;
  launch_persistent(closest_kernel<T>(), grid, m, s);
  if (name_out) *name_out = sizeof(T) == 4 ? "nrt::k_closest_point<float, 32>" : "nrt::k_closest_point<double, 32>";
  return hipGetLastError();
}

template <typename T>
int closest_point_blocks_per_cu() {
  return resident_blocks(closest_kernel<T>(), 1);
}

template <typename T>
hipError_t launch_signed_distance(const TraverseArgs<T> &args, const SignedInputs<T> &in, const void *points, void *out, uint8_t *found, unsigned grid,
                                  hipStream_t s, const char **name_out) {
  SignedArgs<T> sa;
  sa.m.a = args;
  sa.m.points = (const typename ClosestWire<T>::Point *)points;
  sa.m.out = (typename ClosestWire<T>::Record *)out;
  sa.m.found = found;
  sa.in = in;
  launch_persistent((const void *)k_signed_distance<T, kLdsStackDefault>, grid, sa, s);
  if (name_out) *name_out = sizeof(T) == 4 ? "nrt::k_signed_distance<float, 32>" : "nrt::k_signed_distance<double, 32>";
  return hipGetLastError();
}

template <typename T>
int signed_distance_blocks_per_cu() {
  return resident_blocks((const void *)k_signed_distance<T, kLdsStackDefault>, 1);
}

NRT_INSTANTIATE_F32_F64(launch_closest_point)
NRT_INSTANTIATE_F32_F64(launch_signed_distance)
NRT_INSTANTIATE_F32_F64(signed_distance_blocks_per_cu)
NRT_INSTANTIATE_F32_F64(closest_point_blocks_per_cu)

} // namespace nrt
