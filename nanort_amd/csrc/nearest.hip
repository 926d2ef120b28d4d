// nanort_amd/csrc/nearest.hip — the nearest-faces query for gfx950: the K faces of the context's mesh nearest to a point, in order
// (include/nanort_hip.h, "nearest-faces queries").
//
// The rule is include/nanort_closest.h's K-nearest rule: the candidates are the admitted faces with dist2 <= r2, ranked by
// (dist2, prim_id); NearestEnters says whether a face enters the held set, NearestBound what a box is culled against.  The answer
// is a pure function of the mesh and the query, so the walk below only decides which faces need not be looked at.
//
// k_nearest_faces<T, STACK> walks as closest_walk does (closest.hip): persistent, one query per lane, points claimed by claim_init /
// claim_chunk and handed to idle lanes by ballot rank, the lane's stack of node indices in LDS with the launch's overflow area
// behind it (LaneStack), inner nodes until a lane reaches a leaf, the leaves of the whole wave together, then pop or finish.  The
// walk is stated on its own and not as a third mode of closest_walk: the two kernels there keep their registers.
//   * The held set: up to NRT_MAX_NEAREST records per lane fit neither registers nor LDS.  They lie SORTED in the point's own output
//     row, out[rid * K + j], as the K-buffer of the multi-hit walk keeps its hits (own_walks.hip); registers hold the count and the
//     worst held key — the bound (r2 while fewer than K are held) and its prim_id.  A face that enters shifts the records behind it
//     one slot up, in 16-byte (fp32) and 8-byte (fp64) pieces, and the new worst key is read back from the row's last slot.  A lane
//     reads only what it wrote itself, in program order.
//   * The fill: the unused slots of a row get the not-found record {p, r2, 0, 0, 0xFFFFFFFF, 0} and the count is written when the
//     lane finishes, and for a point that is not Searchable at the refill.  Every byte of every row is written.
//   * Row indexing is in 64 bits.
// No inline assembly; plain loads and stores.  The profiling library (-DNRT_PROF) counts nodes opened and triangles tested into
// a.counters[0] / [2] (tools/nearest_probe.py).
#include "traverse_dev.h"
#include "kernels.h"
#include "../../include/nanort_closest.h"

namespace nrt {

template <typename T>
struct NearestArgs {
  TraverseArgs<T> a; // the tree, the trace options, the claim plan and the overflow stack of a launch (rays, hits, mask: unused)
  const typename ClosestWire<T>::Point *points;
  typename ClosestWire<T>::Record *out; // num_points * max_faces records
  uint32_t *counts;                     // may be null
  uint32_t max_faces;                   // K, 1..NRT_MAX_NEAREST
};

// A record of a row, in the pieces the Device form's alignment allows.
template <typename T>
struct RecordPieces {
  typedef uint32_t Piece __attribute__((ext_vector_type(sizeof(T) == 4 ? 4 : 2)));
  static constexpr unsigned kCount = sizeof(typename ClosestWire<T>::Record) / sizeof(Piece);
  union {
    typename ClosestWire<T>::Record r;
    Piece p[kCount];
  };
  __device__ __forceinline__ RecordPieces() {}
  __device__ __forceinline__ void load(const typename ClosestWire<T>::Record *src) {
    const Piece *s = reinterpret_cast<const Piece *>(src);
#pragma unroll
    for (unsigned k = 0; k < kCount; k++) p[k] = s[k];
  }
  __device__ __forceinline__ void store(typename ClosestWire<T>::Record *dst) const {
    Piece *d = reinterpret_cast<Piece *>(dst);
#pragma unroll
    for (unsigned k = 0; k < kCount; k++) d[k] = p[k];
  }
};

// A lane's query and what it knows of its held set (the set itself is the point's output row).
template <typename T>
struct NearestLane {
  T p0, p1, p2;
  T r2;
  T bound;             // NearestBound: r2 until K are held, then the worst held dist2
  uint32_t worst_prim; // ... and its prim_id (0xFFFFFFFF until K are held)
  uint32_t held;
};

// The unused slots of the row and the count.
template <typename T>
__device__ __forceinline__ void fill_row(const NearestArgs<T> &m, const NearestLane<T> &L, uint32_t rid) {
  RecordPieces<T> miss;
  miss.r.point[0] = L.p0, miss.r.point[1] = L.p1, miss.r.point[2] = L.p2;
  miss.r.dist2 = L.r2;
  miss.r.u = T(0), miss.r.v = T(0);
  miss.r.prim_id = kInvalid;
  miss.r._pad = 0u;
  typename ClosestWire<T>::Record *row = m.out + (size_t)rid * m.max_faces;
#pragma nounroll
  for (uint32_t j = L.held; j < m.max_faces; j++) miss.store(row + j);
  if (m.counts) m.counts[rid] = L.held;
}

template <typename T, int STACK>
__global__ __launch_bounds__(kTraverseBlock) void k_nearest_faces(const NearestArgs<T> m) {
  __shared__ uint32_t s_stack[STACK][kTraverseBlock];
  typedef typename Wire<T>::Node Node;
  typedef typename ClosestWire<T>::Point Point;
  typedef typename ClosestWire<T>::Record Record;
  const TraverseArgs<T> &a = m.a;
  const uint32_t K = m.max_faces;

  const unsigned tid = threadIdx.x;
  const unsigned lane = lane_id();
  const LaneStack<StackRef, STACK, TraverseArgs<T>> stk = {a, tid, blockIdx.x * kTraverseBlock + tid};

  NearestLane<T> L;
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

  // Pop the next node, or finish the query when the stack is empty (as closest_walk's).
#define NRT_NEAREST_POP_OR_FINISH()               \
  do {                                            \
    const bool fin_ = sp == 0;                    \
    if (fin_) fill_row<T>(m, L, rid);             \
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
          L.r2 = pt.max_dist * pt.max_dist;
          L.bound = L.r2;
          L.worst_prim = kInvalid;
          L.held = 0u;
          if (nanort_closest::Searchable<T>(p, pt.max_dist)) {
            cur = 0;
            sp = 0;
            state = LANE_TRAV;
          } else { // no candidates: the row is all not-found records; the lane stays idle and takes another point
            fill_row<T>(m, L, rid);
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
      if (!nanort_closest::Culled<T>(nanort_closest::BoxDist2<T>(p, nd.bmin, nd.bmax), L.bound)) {
        if (nd.flag == 0) {
          const uint32_t c0 = nd.data[0], c1 = nd.data[1];
          const Node n0 = a.nodes[c0];
          const Node n1 = a.nodes[c1];
          const T d0 = nanort_closest::BoxDist2<T>(p, n0.bmin, n0.bmax), d1 = nanort_closest::BoxDist2<T>(p, n1.bmin, n1.bmax);
          const bool second = d1 < d0; // on ties (and NaN) the first child
          const uint32_t near_child = second ? c1 : c0, far_child = second ? c0 : c1;
          const T d_near = second ? d1 : d0, d_far = second ? d0 : d1;
          if (!nanort_closest::Culled<T>(d_far, L.bound)) {
            stk.store(s_stack, sp, far_child);
            sp++;
          }
          if (!nanort_closest::Culled<T>(d_near, L.bound)) {
            cur = near_child;
          } else {
            NRT_NEAREST_POP_OR_FINISH();
          }
        } else {
          leaf_cnt = nd.data[0];
          leaf_first = nd.data[1];
          state = LANE_LEAF;
        }
      } else {
        NRT_NEAREST_POP_OR_FINISH();
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
          if ((prim >= a.range0) & (prim < a.range1) & (prim != a.skip_prim)) { // (as closest_walk)
            const T p[3] = {L.p0, L.p1, L.p2};
            RecordPieces<T> rec;
            rec.r.dist2 = nanort_closest::ClosestPointOnTriangle<T>(p, tri.p0, tri.p1, tri.p2, &rec.r.u, &rec.r.v, rec.r.point);
            rec.r.prim_id = prim;
            rec.r._pad = 0u;
#ifdef NRT_PROF
            n_tris++;
#endif
            if (nanort_closest::NearestEnters<T>(rec.r.dist2, prim, L.r2, L.held, K, L.bound, L.worst_prim)) {
              Record *row = m.out + (size_t)rid * K;
              uint32_t j = L.held < K ? L.held : K - 1u; // the slot the shift starts from (the worst is dropped when full)
#pragma nounroll
              while (j > 0u) {
                RecordPieces<T> prev;
                prev.load(row + (j - 1u));
                if (!nanort_closest::Better<T>(rec.r.dist2, prim, prev.r.dist2, prev.r.prim_id)) break;
                prev.store(row + j);
                j--;
              }
              rec.store(row + j);
              L.held = L.held < K ? L.held + 1u : K;
              if (L.held == K) {
                RecordPieces<T> w;
                w.load(row + (K - 1u));
                L.worst_prim = w.r.prim_id;
                L.bound = nanort_closest::NearestBound<T>(L.held, K, L.r2, w.r.dist2);
              }
            }
          }
        }
      }
      if (state == LANE_LEAF) NRT_NEAREST_POP_OR_FINISH();
    }
  }
#undef NRT_NEAREST_POP_OR_FINISH
#ifdef NRT_PROF
  if (a.counters) {
    atomicAdd(a.counters + 0, n_nodes);
    atomicAdd(a.counters + 2, n_tris);
  }
#endif
}

static_assert(kLdsStackDefault == 32, "the names below carry the stack depth");
template <typename T>
static const void *nearest_kernel() {
  return (const void *)k_nearest_faces<T, kLdsStackDefault>;
}

template <typename T>
hipError_t launch_nearest_faces(const TraverseArgs<T> &args, const void *points, uint32_t max_faces, void *out, uint32_t *counts, unsigned grid,
                                hipStream_t s, const char **name_out) {
  NearestArgs<T> m;
  m.a = args;
  m.points = (const typename ClosestWire<T>::Point *)points;
  m.out = (typename ClosestWire<T>::Record *)out;
  m.counts = counts;
  m.max_faces = max_faces;
  launch_persistent(nearest_kernel<T>(), grid, m, s);
  if (name_out) *name_out = sizeof(T) == 4 ? "nrt::k_nearest_faces<float, 32>" : "nrt::k_nearest_faces<double, 32>";
  return hipGetLastError();
}

template <typename T>
int nearest_faces_blocks_per_cu() {
  return resident_blocks(nearest_kernel<T>(), 1);
}

NRT_INSTANTIATE_F32_F64(launch_nearest_faces)
NRT_INSTANTIATE_F32_F64(nearest_faces_blocks_per_cu)

} // namespace nrt
