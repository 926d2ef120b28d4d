// nanort_amd/csrc/traverse.hip — batched closest-hit traversal for gfx950.
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
#include "kernels.h"
#include "traverse_dev.h"

#include <algorithm>

namespace nrt {

// The host side of every persistent launch of this file: the kernel is picked once, as a pointer, and the launch and the
// occupancy query that sizes its grid go through that pointer.
template <typename A>
static void launch_persistent(const void *kernel, unsigned grid, const A &args, hipStream_t s) {
  void *params[] = {(void *)&args};
  (void)hipLaunchKernel(kernel, dim3(grid), dim3(kTraverseBlock), params, 0, s); // (the callers return hipGetLastError())
}
// Resident blocks per CU of `kernel`, 8 at the most; `fallback` where the runtime cannot say.
static int resident_blocks(const void *kernel, int fallback) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, kTraverseBlock, 0) != hipSuccess || n < 1) n = fallback;
  return n > 8 ? 8 : n;
}

template <typename T, bool COUNT, int STACK>
__global__ __launch_bounds__(kTraverseBlock) void k_traverse(const TraverseArgs<T> a) {
  // [depth][thread]: a wave's 64 lanes hit 64 consecutive dwords -> conflict-free.
  __shared__ uint32_t s_stack[STACK][kTraverseBlock];

  typedef typename Wire<T>::Node Node;
  typedef typename Wire<T>::Ray Ray;
  typedef typename Wire<T>::Hit Hit;

  const unsigned tid = threadIdx.x;
  const unsigned lane = lane_id();
  const unsigned gslot = blockIdx.x * kTraverseBlock + tid;
  const bool cull = a.cull_back_face != 0;
  const LaneStack<StackRef, STACK, TraverseArgs<T>> stk = {a, tid, gslot};

  Lane<T> L;
  uint32_t rid = kInvalid; // ray this lane is working on
  uint32_t cur = 0;        // node to visit next (LANE_TRAV)
  uint32_t leaf_first = 0, leaf_cnt = 0; // pending leaf (LANE_LEAF)
  int state = LANE_IDLE;
  int sp = 0; // entries on this lane's stack

  Claim ck; // wave-uniform claimed range
  claim_init<T>(a, ck);
  if (blockIdx.x == 0 && threadIdx.x < kMaxParts) a.next_cursor[kCursorStrideWords * threadIdx.x] = 0u;

  unsigned long long c_nodes = 0, c_leaves = 0, c_tris = 0, c_stack = 0;

  // Pop the next node, or finish the ray when the stack is empty:
  // PostTraversal (nanort.h:1205-1211) with the strict final predicate (:2552).
  // (A macro with select-style updates: every state variable is assigned on both
  // paths, which keeps them all in registers.)
#define NRT_POP_OR_FINISH()                                                              \
  do {                                                                                   \
    const bool fin_ = (sp == 0);                                                         \
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
    sp = fin_ ? sp : sp - 1;                                                             \
    rid = fin_ ? kInvalid : rid;                                                         \
    state = fin_ ? LANE_IDLE : LANE_TRAV;                                                \
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
          const Ray r = (a.debug_flags & 4u) ? a.rays[rid] : load_ray_nt<T>(a.rays + rid);
          lane_init<T>(L, r);
          cur = 0;
          sp = 0;
          state = LANE_TRAV;
          if (COUNT) c_stack = c_stack > 1ull ? c_stack : 1ull;
        }
        ck.next += take;
        idle = __ballot(state == LANE_IDLE);
      }
    }
    if (idle == ~0ull) {
      if (ck.exhausted) break; // nothing left anywhere in this wave
      continue;             // (cannot happen: refill_min <= 64)
    }

    // ---- phase 1: inner nodes, until this lane reaches a leaf or finishes -----------
    while (state == LANE_TRAV) {
      const Node nd = a.nodes[cur];
      if (COUNT) c_nodes++;
      if (slab_test<T>(L, nd.bmin, nd.bmax)) {
        if (nd.flag == 0) {
          const int near = L.sign(nd.axis);
          const uint32_t far_child = near ? nd.data[0] : nd.data[1];
          cur = near ? nd.data[1] : nd.data[0];
          // push far; near stays in `cur` (it would be popped next anyway: nanort.h:2542-2543)
          stk.store(s_stack, sp, far_child);
          sp++;
          if (COUNT) {
            // the reference holds near+far on its stack at this point
            const unsigned long long need = (unsigned long long)sp + 1ull;
            c_stack = need > c_stack ? need : c_stack;
          }
        } else {
          leaf_cnt = nd.data[0];
          leaf_first = nd.data[1];
          state = LANE_LEAF;
          if (COUNT) c_leaves++;
        }
      } else {
        NRT_POP_OR_FINISH();
      }
      // leave early when too few lanes are still walking inner nodes
      if ((unsigned)__builtin_popcountll(__ballot(state == LANE_TRAV)) < a.trav_min) break;
    }

    // ---- phase 2: lanes holding a leaf test its triangles together ------------------
    if (__ballot(state == LANE_LEAF) != 0ull) {
      const uint32_t cnt = state == LANE_LEAF ? leaf_cnt : 0u;
      uint32_t skip = a.skip_prim;
      if constexpr (!COUNT) // (the counting pass takes no ids: api.hip)
        if (a.skip_ids != nullptr && state == LANE_LEAF) skip = a.skip_ids[rid]; // per-ray skip ids (common.h): the id of the ray the lane holds NOW
      for (uint32_t i = 0; __ballot(i < cnt) != 0ull; i++) {
        if (i < cnt) {
          const LeafTri<T> tri = a.tris[leaf_first + i];
          if (COUNT) c_tris++;
          tri_test<T>(L, tri, true, a.range0, a.range1, skip, cull);
        }
      }
      if (state == LANE_LEAF) NRT_POP_OR_FINISH();
    }
  }

  if (COUNT) {
    // wave reduction, then one atomic per wave per counter
    for (int off = 32; off > 0; off >>= 1) {
      c_nodes += __shfl_xor(c_nodes, off);
      c_leaves += __shfl_xor(c_leaves, off);
      c_tris += __shfl_xor(c_tris, off);
      unsigned long long o = __shfl_xor(c_stack, off);
      c_stack = o > c_stack ? o : c_stack;
    }
    if (lane == 0) {
      atomicAdd(&a.counters[0], c_nodes);
      atomicAdd(&a.counters[1], c_leaves);
      atomicAdd(&a.counters[2], c_tris);
      atomicMax(&a.counters[3], c_stack);
    }
  }
#undef NRT_POP_OR_FINISH
}

// ---------------------------------------------------------------------------
// Production kernel: same traversal ORDER and same culling decisions as the
// binary loop above (hence the same hit records, ties included), but each step
// fetches one WideNode and tests both children.  A child that passes its slab
// test is entered at once (near first) or pushed with its t_min; a popped entry
// is entered iff t_min <= hit_t, which is exactly the reference's test at pop
// time, because its slab test factors into (t_min <= t_max of the planes) — which
// does not depend on hit_t and was established at push time — and
// (t_min <= hit_t) (nanort.h:2315-2318: hit_t is the innermost operand of the
// safemin chain).
// ---------------------------------------------------------------------------
enum : int { W_IDLE = 0, W_TRAV = 1, W_LEAF = 2, W_POP = 3 };

// Both child boxes of one WideNode at once.  For fp32 the two boxes ride in the two halves of
// 64-bit register pairs, so the subtract / multiply chain issues as v_pk_add_f32 / v_pk_mul_f32
// (one VALU slot for two IEEE operations: same operations, same rounding, half the issue slots).
template <typename T>
struct SlabPair {
  bool h0, h1;
  T tm0, tm1;
};

__device__ __forceinline__ SlabPair<float> slab_pair(const Lane<float> &L, const WideNode<float> &w) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  const f2 mm = {Const<float>::maxmult(), Const<float>::maxmult()};
  float tmin0 = L.min_t, tmin1 = L.min_t, tmax0 = L.hit_t, tmax1 = L.hit_t;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int sg = L.sign(k);
    const f2 lo = {sg ? w.box0[3 + k] : w.box0[k], sg ? w.box1[3 + k] : w.box1[k]};
    const f2 hi = {sg ? w.box0[k] : w.box0[3 + k], sg ? w.box1[k] : w.box1[3 + k]};
    const f2 o = {L.org(k), L.org(k)};
    const f2 iv = {L.inv(k), L.inv(k)};
    const f2 t0 = (lo - o) * iv;
    const f2 t1 = ((hi - o) * iv) * mm;
    tmin0 = Const<float>::fmax(t0.x, tmin0); // see slab_axis
    tmin1 = Const<float>::fmax(t0.y, tmin1);
    tmax0 = Const<float>::fmin(t1.x, tmax0);
    tmax1 = Const<float>::fmin(t1.y, tmax1);
  }
  SlabPair<float> r;
  r.h0 = tmin0 <= tmax0;
  r.h1 = tmin1 <= tmax1;
  r.tm0 = tmin0;
  r.tm1 = tmin1;
  return r;
}

__device__ __forceinline__ SlabPair<double> slab_pair(const Lane<double> &L, const WideNode<double> &w) {
  SlabPair<double> r;
  const double b0[6] = {w.mn[0][0], w.mn[1][0], w.mn[2][0], w.mx[0][0], w.mx[1][0], w.mx[2][0]};
  const double b1[6] = {w.mn[0][1], w.mn[1][1], w.mn[2][1], w.mx[0][1], w.mx[1][1], w.mx[2][1]};
  r.h0 = slab_test_tmin<double>(L, b0, b0 + 3, r.tm0);
  r.h1 = slab_test_tmin<double>(L, b1, b1 + 3, r.tm1);
  return r;
}
// The same two tests with the near / far rows of each axis fetched by the ray's direction signs (Lane::so0..2: 0 or 48,
// the distance between the mn and mx rows of a WideNode<double>): the same values into slab_axis's arithmetic,
// twelve 64-bit selects per step fewer.  `rec` = byte offset of the record (32 bits: arrays below 4 GiB).
struct WideTail { // bytes 96..111 of a WideNode<double>
  uint32_t c0, c1;
  int32_t axis;
  uint32_t pad;
};
__device__ __forceinline__ SlabPair<double> slab_pair_presel(const Lane<double> &L, const char *base, uint32_t rec) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  const double mm = Const<double>::maxmult();
  double tmin0 = L.min_t, tmin1 = L.min_t, tmax0 = L.hit_t, tmax1 = L.hit_t;
  const uint32_t rec48 = rec + 48u;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const uint32_t so = k == 0 ? L.so0 : (k == 1 ? L.so1 : L.so2);
    const d2 lo = *reinterpret_cast<const d2 *>(base + (size_t)(rec + so) + 16 * k);
    const d2 hi = *reinterpret_cast<const d2 *>(base + (size_t)(rec48 - so) + 16 * k);
    const double t00 = (lo.x - L.org(k)) * L.inv(k), t01 = (lo.y - L.org(k)) * L.inv(k);
    const double t10 = (hi.x - L.org(k)) * L.inv(k) * mm, t11 = (hi.y - L.org(k)) * L.inv(k) * mm;
    tmin0 = Const<double>::fmax(t00, tmin0); // see slab_axis
    tmin1 = Const<double>::fmax(t01, tmin1);
    tmax0 = Const<double>::fmin(t10, tmax0);
    tmax1 = Const<double>::fmin(t11, tmax1);
  }
  SlabPair<double> r;
  r.h0 = tmin0 <= tmax0;
  r.h1 = tmin1 <= tmax1;
  r.tm0 = tmin0;
  r.tm1 = tmin1;
  return r;
}

// The four boxes of one Wide4Node.  fp32: slots (0,1) and (2,3) ride in register pairs as in slab_pair.
template <typename T>
struct Slab4 {
  bool h[4];
  T tm[4];
};

__device__ __forceinline__ Slab4<float> slab4(const Lane<float> &L, const Wide4Node<float> &w) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  const f2 mm = {Const<float>::maxmult(), Const<float>::maxmult()};
  float tmin[4] = {L.min_t, L.min_t, L.min_t, L.min_t}, tmax[4] = {L.hit_t, L.hit_t, L.hit_t, L.hit_t};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int sg = L.sign(k);
    const f2 o = {L.org(k), L.org(k)};
    const f2 iv = {L.inv(k), L.inv(k)};
#pragma unroll
    for (int p = 0; p < 2; p++) {
      const f2 lo = {sg ? w.bmax[k][2 * p] : w.bmin[k][2 * p], sg ? w.bmax[k][2 * p + 1] : w.bmin[k][2 * p + 1]};
      const f2 hi = {sg ? w.bmin[k][2 * p] : w.bmax[k][2 * p], sg ? w.bmin[k][2 * p + 1] : w.bmax[k][2 * p + 1]};
      const f2 t0 = (lo - o) * iv;
      const f2 t1 = ((hi - o) * iv) * mm;
      tmin[2 * p] = Const<float>::fmax(t0.x, tmin[2 * p]); // see slab_axis
      tmin[2 * p + 1] = Const<float>::fmax(t0.y, tmin[2 * p + 1]);
      tmax[2 * p] = Const<float>::fmin(t1.x, tmax[2 * p]);
      tmax[2 * p + 1] = Const<float>::fmin(t1.y, tmax[2 * p + 1]);
    }
  }
  Slab4<float> r;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    r.h[j] = tmin[j] <= tmax[j];
    r.tm[j] = tmin[j];
  }
  return r;
}

// The same four tests with the near / far plane rows fetched straight from where the ray's direction signs say they are
// (a per-ray byte offset inside the record: Lane::so0..2) instead of fetching both rows of every axis and selecting per
// value: the same values reach the same arithmetic, 24 selects per step do not.  `rec` = byte offset of the record in the
// array (32 bits: arrays below 4 GiB).
struct Wide4Tail { // bytes 96..127 of a Wide4Node<float>
  uint32_t c[4];
  int32_t axis0, axis1, axis2;
  uint32_t pad;
};
// (OFF = uint32_t for arrays below 4 GiB — scalar base + 32-bit lane offset —, uint64_t for larger ones: template bit ORDER & 4)
template <typename OFF>
__device__ __forceinline__ Slab4<float> slab4_presel(const Lane<float> &L, const char *base, OFF rec) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  typedef float f4 __attribute__((ext_vector_type(4)));
  const f2 mm = {Const<float>::maxmult(), Const<float>::maxmult()};
  float tmin[4] = {L.min_t, L.min_t, L.min_t, L.min_t}, tmax[4] = {L.hit_t, L.hit_t, L.hit_t, L.hit_t};
  const OFF rec48 = rec + (OFF)48u;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const uint32_t so = k == 0 ? L.so0 : (k == 1 ? L.so1 : L.so2);
    const f4 lo4 = *reinterpret_cast<const f4 *>(base + (size_t)(rec + so) + 16 * k);   // bmin[k][0..3] or bmax[k][0..3]
    const f4 hi4 = *reinterpret_cast<const f4 *>(base + (size_t)(rec48 - so) + 16 * k); // the other row
    const f2 o = {L.org(k), L.org(k)};
    const f2 iv = {L.inv(k), L.inv(k)};
#pragma unroll
    for (int p = 0; p < 2; p++) {
      const f2 lo = {p ? lo4.z : lo4.x, p ? lo4.w : lo4.y};
      const f2 hi = {p ? hi4.z : hi4.x, p ? hi4.w : hi4.y};
      const f2 t0 = (lo - o) * iv;
      const f2 t1 = ((hi - o) * iv) * mm;
      tmin[2 * p] = Const<float>::fmax(t0.x, tmin[2 * p]); // see slab_axis
      tmin[2 * p + 1] = Const<float>::fmax(t0.y, tmin[2 * p + 1]);
      tmax[2 * p] = Const<float>::fmin(t1.x, tmax[2 * p]);
      tmax[2 * p + 1] = Const<float>::fmin(t1.y, tmax[2 * p + 1]);
    }
  }
  Slab4<float> r;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    r.h[j] = tmin[j] <= tmax[j];
    r.tm[j] = tmin[j];
  }
  return r;
}

__device__ __forceinline__ Slab4<double> slab4(const Lane<double> &L, const Wide4Node<double> &w) {
  Slab4<double> r;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const double box[6] = {w.bmin[0][j], w.bmin[1][j], w.bmin[2][j], w.bmax[0][j], w.bmax[1][j], w.bmax[2][j]};
    r.h[j] = slab_test_tmin<double>(L, box, box + 3, r.tm[j]);
  }
  return r;
}

// One stack entry: child reference + its t_min (the t_min is kept as raw bits next to the reference so
// that one LDS access moves both).
template <typename T>
struct StackEntry;
template <>
struct StackEntry<float> {
  typedef uint2 type;
  static constexpr bool kHasTmin = true; // (LaneStack: the t_min half lies in spill_tmin)
  static __device__ __forceinline__ type make(uint32_t ref, float tm) { return make_uint2(ref, __float_as_uint(tm)); }
  static __device__ __forceinline__ uint32_t ref(const type &e) { return e.x; }
  static __device__ __forceinline__ float tmin(const type &e) { return __uint_as_float(e.y); }
};
template <>
struct StackEntry<double> {
  typedef uint4 type; // {ref, pad, t_min lo, t_min hi}
  static constexpr bool kHasTmin = true;
  static __device__ __forceinline__ type make(uint32_t ref, double tm) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(tm);
    return make_uint4(ref, 0u, (uint32_t)b, (uint32_t)(b >> 32));
  }
  static __device__ __forceinline__ uint32_t ref(const type &e) { return e.x; }
  static __device__ __forceinline__ double tmin(const type &e) {
    return __longlong_as_double((long long)(((unsigned long long)e.w << 32) | e.z));
  }
};

// The per-lane moves of the wide walks, shared by k_traverse_wide, the tail of its launches and the scene kernels
// (k_scene_trace, k_scene_walk).  What a macro may assume in the scope it expands in, and nothing else:
//   L (Lane<T>), cur, state, sp   the lane's ray and where its walk stands — read and written;
//   T, STACK, SE = StackEntry<T>  the kernel's types;
//   s_stack[STACK][block]         the block's LDS stacks;
//   stk                           the lane's OWN stack in them and in the launch's overflow arrays (LaneStack<SE, STACK, ...>,
//                                 traverse_dev.h: its two columns): the step macros push there;
//   a                             the launch's argument block: NRT_STACK_STORE writes its .spill / .spill_tmin;
//   tid                           NRT_STEP_NODE4_SL / _DIST only: the lane's column of s_stack, for the three unguarded stores they
//                                 make when every lane of the wave has room in LDS.
// A pop names the stack it pops from as its argument: a lane's own (`stk`) or, in the tail of a launch, its owner's column.
// Where entry i lies is said twice, once per direction: LaneStack::load reads it, NRT_STACK_STORE writes it, both over the
// view's columns and its spill_at(); no other macro and no kernel computes a stack address.

// One stack pop (a lane in W_POP) from the stack `stk_`: the entry is entered iff its t_min still beats the hit distance — the
// reference's slab test at pop time (see the comment above the kernel); an empty stack finishes the ray.
#define NRT_POP_ENTRY(stk_)                                                                            \
do {                                                                                                 \
  int s1_ = sp - 1;                                                                                  \
  s1_ = s1_ < 0 ? 0 : s1_; /* (with the accessor's own clamp at STACK - 1: one v_med3_i32) */        \
  typename SE::type e_;                                                                              \
  (stk_).load(s_stack, s1_, e_);                                                                     \
  const bool fin_ = (sp == 0);                        /* empty stack: the ray is done */             \
  const bool enter_ = !fin_ & (SE::tmin(e_) <= L.hit_t);                                             \
  const uint32_t ref_ = SE::ref(e_);                                                                 \
  sp = s1_;                                                                                          \
  cur = enter_ ? (ref_ & ~kLeafBit) : cur;                                                           \
  state = fin_ ? W_IDLE : (enter_ ? ((ref_ & kLeafBit) ? W_LEAF : W_TRAV) : W_POP);                  \
} while (0)

// Entry `i_` of the stack `stk_` := {ref_, tm_}: LaneStack::load's counterpart for StackEntry.  A macro, its columns taken from the
// view: as a function (member or free, whatever it is handed) the fp64 one-level walk's step loads its record's 12-byte tail
// in two pieces and C5 runs 9 % slower (profiles/r08a_one_statement.txt).
#define NRT_STACK_STORE(stk_, i_, ref_, tm_)                                                           \
do {                                                                                                 \
  if ((i_) < STACK) {                                                                                \
    s_stack[(i_)][(stk_).col] = SE::make((ref_), (tm_));                                             \
  } else {                                                                                           \
    const size_t o_ = (stk_).spill_at((i_));                                                         \
    a.spill[o_] = (ref_);                                                                            \
    a.spill_tmin[o_] = (tm_);                                                                        \
  }                                                                                                  \
} while (0)

// One push onto the lane's own stack.
#define NRT_PUSH_IF(cond_, ref_, tm_)                                                                  \
do {                                                                                                 \
  if (cond_) {                                                                                       \
    NRT_STACK_STORE(stk, sp, (ref_), (tm_));                                                         \
    sp++;                                                                                            \
  }                                                                                                  \
} while (0)

// One step of a lane in W_TRAV over the WideNode record `w_`: both child boxes tested, the far child of two hits
// pushed with its t_min, the near one (or the only one) entered.
#define NRT_STEP_NODE(w_)                                                                              \
do {                                                                                                 \
  const SlabPair<T> sl2_ = slab_pair(L, (w_));                                                       \
  NRT_STEP_NODE_SL(sl2_, (w_));                                                                      \
} while (0)
/* (sl_: the two box tests; w_: anything with c0, c1, axis) */
#define NRT_STEP_NODE_SL(sl_, w_)                                                                      \
do {                                                                                                 \
  const bool near1_ = L.sign((w_).axis) != 0; /* near child = data[dir_sign[axis]] (nanort.h:2538) */ \
  const bool both_ = sl_.h0 & sl_.h1, any_ = sl_.h0 | sl_.h1;                                        \
  /* the far child of two hits waits with its t_min */                                               \
  NRT_PUSH_IF(both_, near1_ ? (w_).c0 : (w_).c1, near1_ ? sl_.tm0 : sl_.tm1);                        \
  /* both hit: the near one; one hit: that one */                                                    \
  const bool go1_ = both_ ? near1_ : sl_.h1;                                                         \
  const uint32_t next_ = go1_ ? (w_).c1 : (w_).c0;                                                   \
  cur = any_ ? (next_ & ~kLeafBit) : cur;                                                            \
  state = any_ ? ((next_ & kLeafBit) ? W_LEAF : W_TRAV) : W_POP;                                     \
} while (0)


// The same step over a Wide4Node record: the four grandchild boxes tested at once.  Why this visits the same leaves in
// the same order as the binary loop (nanort.h:2526-2548) on a tree whose child boxes lie inside their parents':
//  * order — the binary loop enters near child (by the node's axis) before far child, and inside each child its near
//    grandchild (by the child's axis) before its far one; the four slots are ranked by exactly that rule, the first hit
//    in rank order is entered and the others are pushed in reverse rank order, so they pop in rank order;
//  * culling — the binary loop would also test the child's own box; a ray that hits a grandchild's box within
//    [min_t, hit_t] hits the child's box within it too (the grandchild's box lies inside, the slab arithmetic is
//    monotone), and a ray that misses the child's box misses both grandchildren, so skipping that test changes nothing;
//  * hit distance — a grandchild of the FAR child is tested here with the hit distance of this moment instead of the
//    later one the binary loop would use; every pushed entry is re-tested against the current hit distance when it is
//    popped (NRT_POP_ENTRY), which is the binary loop's decision.
// The half of a leaf child has one slot (the other is marked empty and never hit).
#define NRT_STEP_NODE4(w_)                                                                             \
do {                                                                                                 \
  const Slab4<T> sl4_ = slab4(L, (w_));                                                              \
  NRT_STEP_NODE4_SL(sl4_, (w_));                                                                     \
} while (0)
/* (sl_: the four box tests of the record; w_: anything with c[4], axis0, axis1, axis2) */
#define NRT_STEP_NODE4_SL(sl_, w_)                                                                     \
do {                                                                                                 \
  const bool sA_ = L.sign((w_).axis1) != 0, sB_ = L.sign((w_).axis2) != 0, s0_ = L.sign((w_).axis0) != 0; \
  const bool v1_ = (w_).c[1] != kWide4Empty, v3_ = (w_).c[3] != kWide4Empty;                         \
  const bool h0_ = sl_.h[0], h1_ = sl_.h[1] & v1_, h2_ = sl_.h[2], h3_ = sl_.h[3] & v3_;             \
  /* inside each half: near slot first */                                                            \
  const bool an_ = sA_ ? h1_ : h0_, af_ = sA_ ? h0_ : h1_, bn_ = sB_ ? h3_ : h2_, bf_ = sB_ ? h2_ : h3_; \
  const uint32_t ran_ = sA_ ? (w_).c[1] : (w_).c[0], raf_ = sA_ ? (w_).c[0] : (w_).c[1];             \
  const uint32_t rbn_ = sB_ ? (w_).c[3] : (w_).c[2], rbf_ = sB_ ? (w_).c[2] : (w_).c[3];             \
  const T tan_ = sA_ ? sl_.tm[1] : sl_.tm[0], taf_ = sA_ ? sl_.tm[0] : sl_.tm[1];                    \
  const T tbn_ = sB_ ? sl_.tm[3] : sl_.tm[2], tbf_ = sB_ ? sl_.tm[2] : sl_.tm[3];                    \
  /* the near half (by the node's own axis) first: ranks 0..3 */                                     \
  const bool q0_ = s0_ ? bn_ : an_, q1_ = s0_ ? bf_ : af_, q2_ = s0_ ? an_ : bn_, q3_ = s0_ ? af_ : bf_; \
  const uint32_t r0_ = s0_ ? rbn_ : ran_, r1_ = s0_ ? rbf_ : raf_, r2_ = s0_ ? ran_ : rbn_, r3_ = s0_ ? raf_ : rbf_; \
  const T t1_ = s0_ ? tbf_ : taf_, t2_ = s0_ ? tan_ : tbn_, t3_ = s0_ ? taf_ : tbf_;                 \
  const bool p3_ = q3_ & (q0_ | q1_ | q2_), p2_ = q2_ & (q0_ | q1_), p1_ = q1_ & q0_;                \
  if (NRT_W4_FAST_PUSH && __ballot(sp > STACK - 3) == 0ull) {                                         \
    /* every stepping lane has room for three entries in LDS: the candidates are stored unconditionally, in push order, \
       and the stack pointer moves past the ones that count — three stores and three adds instead of three guarded    \
       blocks (compare, branch, room check, store, add) that nearly always run because SOME lane needs them */         \
    s_stack[sp][tid] = SE::make(r3_, t3_);                                                           \
    sp += p3_ ? 1 : 0;                                                                               \
    s_stack[sp][tid] = SE::make(r2_, t2_);                                                           \
    sp += p2_ ? 1 : 0;                                                                               \
    s_stack[sp][tid] = SE::make(r1_, t1_);                                                           \
    sp += p1_ ? 1 : 0;                                                                               \
  } else {                                                                                           \
    NRT_PUSH_IF(p3_, r3_, t3_);                                                                      \
    NRT_PUSH_IF(p2_, r2_, t2_);                                                                      \
    NRT_PUSH_IF(p1_, r1_, t1_);                                                                      \
  }                                                                                                  \
  const bool any_ = q0_ | q1_ | q2_ | q3_;                                                           \
  const uint32_t next_ = q0_ ? r0_ : (q1_ ? r1_ : (q2_ ? r2_ : r3_));                                \
  cur = any_ ? (next_ & ~kLeafBit) : cur;                                                            \
  state = any_ ? ((next_ & kLeafBit) ? W_LEAF : W_TRAV) : W_POP;                                     \
} while (0)

// The Wide4Node step with the four slots entered in order of their ENTRY DISTANCE (template parameter ORDER = 1; tunable
// `order4`) instead of the binary loop's axis-sign order.  What this keeps and what it gives up:
//  * culling is unchanged — a slot is entered iff its slab test passes now and, when it was pushed, iff its t_min still
//    beats the hit distance at pop time — so the walk tests a subset of the primitives the reference can reach and every
//    primitive whose box chain the final hit distance does not cull: the closest hit's t (and u, v, prim_id of the record
//    that realises it) are the reference's, except that among several primitives at EXACTLY the same t the survivor is
//    the one this order tests last, not the one the reference's order tests last (prim_id may differ at
//    exact-t ties only; tests/helpers.py:assert_hits_match re-verifies every such ray);
//  * the LEAF SEQUENCE is no longer the reference's, so records are not bit-identical to the same-tree oracle at ties.
// Keys: a hit slot sorts by min(t_min, FLT_MAX) (a hit can carry t_min = +inf only while the hit distance is +inf: the
// clamped key then still passes the pop test), a missed or empty slot by +inf — so hits always precede misses.  Five
// compare-exchanges (a 4-input sorting network) order {key, reference}; the first hit is entered, the others are pushed
// farthest first.
#define NRT_CSWAP4(ka_, ra_, kb_, rb_)                                                                 \
do {                                                                                                 \
  const bool sw_ = kb_ < ka_;                                                                        \
  const T klo_ = Const<T>::fmin(ka_, kb_), khi_ = Const<T>::fmax(ka_, kb_);                          \
  const uint32_t rlo_ = sw_ ? rb_ : ra_, rhi_ = sw_ ? ra_ : rb_;                                     \
  ka_ = klo_; kb_ = khi_; ra_ = rlo_; rb_ = rhi_;                                                    \
} while (0)
#define NRT_STEP_NODE4_DIST(sl_, w_)                                                                   \
do {                                                                                                 \
  const T inf_ = Const<T>::inf(), big_ = Const<T>::fltmax();                                         \
  const bool h0_ = sl_.h[0], h1_ = sl_.h[1] & ((w_).c[1] != kWide4Empty);                            \
  const bool h2_ = sl_.h[2], h3_ = sl_.h[3] & ((w_).c[3] != kWide4Empty);                            \
  T k0_ = h0_ ? Const<T>::fmin(sl_.tm[0], big_) : inf_, k1_ = h1_ ? Const<T>::fmin(sl_.tm[1], big_) : inf_; \
  T k2_ = h2_ ? Const<T>::fmin(sl_.tm[2], big_) : inf_, k3_ = h3_ ? Const<T>::fmin(sl_.tm[3], big_) : inf_; \
  uint32_t r0_ = (w_).c[0], r1_ = (w_).c[1], r2_ = (w_).c[2], r3_ = (w_).c[3];                       \
  NRT_CSWAP4(k0_, r0_, k1_, r1_);                                                                    \
  NRT_CSWAP4(k2_, r2_, k3_, r3_);                                                                    \
  NRT_CSWAP4(k0_, r0_, k2_, r2_);                                                                    \
  NRT_CSWAP4(k1_, r1_, k3_, r3_);                                                                    \
  NRT_CSWAP4(k1_, r1_, k2_, r2_);                                                                    \
  const bool any_ = k0_ < inf_, p1_ = k1_ < inf_, p2_ = k2_ < inf_, p3_ = k3_ < inf_;                \
  if (__ballot(sp > STACK - 3) == 0ull) {                                                             \
    s_stack[sp][tid] = SE::make(r3_, k3_);                                                           \
    sp += p3_ ? 1 : 0;                                                                               \
    s_stack[sp][tid] = SE::make(r2_, k2_);                                                           \
    sp += p2_ ? 1 : 0;                                                                               \
    s_stack[sp][tid] = SE::make(r1_, k1_);                                                           \
    sp += p1_ ? 1 : 0;                                                                               \
  } else {                                                                                           \
    NRT_PUSH_IF(p3_, r3_, k3_);                                                                      \
    NRT_PUSH_IF(p2_, r2_, k2_);                                                                      \
    NRT_PUSH_IF(p1_, r1_, k1_);                                                                      \
  }                                                                                                  \
  cur = any_ ? (r0_ & ~kLeafBit) : cur;                                                              \
  state = any_ ? ((r0_ & kLeafBit) ? W_LEAF : W_TRAV) : W_POP;                                       \
} while (0)

// PLAIN: the launch uses trace options that cannot reject a primitive (full prim_ids_range, no skip_prim_id, no
// back-face culling — the reference's defaults): the three id comparisons per triangle test are compiled out.
//
// (Round 2 also carried a SPLIT variant here — exact work splitting in the drain of a launch: a busy lane handed the oldest
// entry of its stack to an idle lane, results folded per ray by (smallest t, latest segment) — and a per-lane drain loop.
// Both were exact and soaked; both were measured to lose (the variant's bulk loop ran 9 % slower than production through
// register pressure and the extra checks, 13 % per step in all: profiles/r02c_split_*.txt, r03g_split_asis.txt) and were
// removed in round 3.  What a launch waits for at its end is the dependent chain of its few longest rays
// (tools/drain_probe.py, tools/tail_first_probe.py); DESIGN.md 3.1 and 10 keep the numbers.)
#ifndef NRT_SCENE_WALK_WAVES
#define NRT_SCENE_WALK_WAVES 4 // waves per SIMD k_scene_walk is compiled for (128 registers; 5 -> 96 registers spills 30 of them and measured slower)
#endif
#ifndef NRT_SCENE_P1_UNROLL
#define NRT_SCENE_P1_UNROLL 2 // ... of the two-level scene kernel
#endif
#ifndef NRT_W2_F64_P1_UNROLL
#define NRT_W2_F64_P1_UNROLL 2 // ... of the fp64 one-level walk
#endif
#ifndef NRT_W4_P1_UNROLL
#define NRT_W4_P1_UNROLL 2 // fp32 two-level walk: pop + step rounds per trip of the inner-node loop
#endif
#ifndef NRT_W4_FAST_PUSH
#define NRT_W4_FAST_PUSH 1 // two-level step: unconditional stores of the three push candidates when every lane has room in LDS
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
// Leaf items (k_traverse_wide with ORDER bit 1, k_scene_walk): the records of all the lanes of a wave that wait at a leaf, tested
// ONE PER LANE in one trip when they are at most 64 together.  `cnt` (0 for a lane that does not wait, at most 4) and `first` (the
// lane's first record) describe the leaves; record k of owner o becomes item base(o) + k (prefix sums of the counts by three
// ballots), item j is tested by lane j with its OWNER's ray constants (org, Sx Sy Sz and the packed axes, fetched by ds_bpermute;
// the record's address and the owner's lane through two small LDS arrays), and every owner then takes its items' results IN RECORD
// ORDER through the reference's own accept rule (`tt > t` / `tt < min_t` reject, equality and NaN accepted, nanort.h:1133-1139).
// The same tests on the same operands (tri_solve, as tri_test), accepted in the same sequence: the lane state after
// the leaf is bit for bit what the owner's own loop leaves (tests/test_gpu_leaf_items.py, tests/test_gpu_scene.py).  Returns false
// — nothing done — when the records do not fit one trip: the caller's owner loop then runs.  Wave-uniform control flow only.
// `skip_prim` is the calling lane's OWN skip id (per-ray skip ids, common.h): an item is tested against its owner's, fetched like the
// owner's ray constants.
// (SLOT: how an item names its record in LDS — a 32-bit index into `base` (k_traverse_wide: one array per launch; 4 bytes per item
// keep the block's LDS below a sixth of the CU's) or the record's address (k_scene_walk: every owner's mesh has its own array))
template <bool PLAIN, typename SLOT>
__device__ __forceinline__ bool leaf_items_one_trip(Lane<float> &L, uint32_t cnt, const LeafTri<float> *base, SLOT first, unsigned lane, volatile uint32_t *own_,
                                                    volatile SLOT *rec_, uint32_t range0, uint32_t range1, uint32_t skip_prim, bool cull) {
  typedef float T;
  const unsigned long long b0_ = __ballot((cnt & 1u) != 0u), b1_ = __ballot((cnt & 2u) != 0u), b2_ = __ballot((cnt & 4u) != 0u);
  const uint32_t items_ = (uint32_t)__builtin_popcountll(b0_) + 2u * (uint32_t)__builtin_popcountll(b1_) + 4u * (uint32_t)__builtin_popcountll(b2_);
  if (items_ > (uint32_t)kWave || items_ == 0u) return false;
  const unsigned long long below_ = (1ull << lane) - 1ull;
  const uint32_t base_ = (uint32_t)__builtin_popcountll(b0_ & below_) + 2u * (uint32_t)__builtin_popcountll(b1_ & below_) +
                         4u * (uint32_t)__builtin_popcountll(b2_ & below_);
  const uint32_t kmax_ = b2_ ? 4u : ((b1_ & b0_) ? 3u : (b1_ ? 2u : 1u)); // most records any lane holds (wave-uniform)
#pragma unroll
  for (uint32_t k_ = 0; k_ < 4u; k_++)
    if (k_ < cnt) {
      own_[base_ + k_] = lane; // (a word per item: sub-word stores of neighbouring lanes into one word would queue)
      rec_[base_ + k_] = first + k_;
    }
  // (LDS operations of one wave are performed in issue order and the accesses are volatile: the reads below see the writes)
  const bool item_ = lane < items_;
  const uint32_t me_ = item_ ? lane : 0u; // (a lane without an item repeats item 0 — there is one: the callers come here with a lane waiting — and drops the result)
  const SLOT sv_ = rec_[me_];
  const LeafTri<float> *slot_;
  if constexpr (sizeof(SLOT) == 4)
    slot_ = base + sv_;
  else
    slot_ = sv_;
  const int oa_ = (int)(own_[me_] << 2); // the owner lane's byte address for ds_bpermute
  const LeafTri<T> tri = *slot_; // (issued before the constants are fetched: the two latencies overlap)
  const float o0 = __int_as_float(__builtin_amdgcn_ds_bpermute(oa_, __float_as_int(L.org0))), o1 = __int_as_float(__builtin_amdgcn_ds_bpermute(oa_, __float_as_int(L.org1))),
              o2 = __int_as_float(__builtin_amdgcn_ds_bpermute(oa_, __float_as_int(L.org2)));
  const float sx = __int_as_float(__builtin_amdgcn_ds_bpermute(oa_, __float_as_int(L.Sx))), sy = __int_as_float(__builtin_amdgcn_ds_bpermute(oa_, __float_as_int(L.Sy))),
              sz = __int_as_float(__builtin_amdgcn_ds_bpermute(oa_, __float_as_int(L.Sz)));
  const uint32_t pk = (uint32_t)__builtin_amdgcn_ds_bpermute(oa_, (int)L.pk);
  const int ikx = (int)((pk >> 3) & 3u), iky = (int)((pk >> 5) & 3u), ikz = (int)((pk >> 7) & 3u);
  uint32_t skip_o = 0u;
  if constexpr (!PLAIN) skip_o = (uint32_t)__builtin_amdgcn_ds_bpermute(oa_, (int)skip_prim);
  const uint32_t prim_i = tri.prim_id;
  const TriSolve<T> ts_ = tri_solve<T, PLAIN>(tri, item_, o0, o1, o2, sx, sy, sz, ikx, iky, ikz, range0, range1, skip_o, cull); // (on the owner's constants)
  const bool ok = ts_.ok;
  const T tt_i = ts_.tt, uu_i = ts_.uu, vv_i = ts_.vv;
  // ... and back to the owners, record by record
  const unsigned long long okm_ = __ballot(ok);
  bool got_ = false;
  uint32_t win_ = 0;
  for (uint32_t k2_ = 0; k2_ < kmax_; k2_++) {
    const uint32_t src_ = (base_ + k2_) & 63u;
    const T ttk = __int_as_float(__builtin_amdgcn_ds_bpermute((int)(src_ << 2), __float_as_int(tt_i)));
    const bool okk = (k2_ < cnt) & (((okm_ >> src_) & 1ull) != 0ull);
    const bool acc = okk & !(ttk > L.hit_t) & !(ttk < L.min_t); // nanort.h:1133-1139: equality and NaN accepted
    L.hit_t = acc ? ttk : L.hit_t;
    win_ = acc ? src_ : win_;
    got_ = got_ | acc;
  }
  if (__ballot(got_) != 0ull) {
    const int wa_ = (int)(win_ << 2);
    const T uw = __int_as_float(__builtin_amdgcn_ds_bpermute(wa_, __float_as_int(uu_i)));
    const T vw = __int_as_float(__builtin_amdgcn_ds_bpermute(wa_, __float_as_int(vv_i)));
    const uint32_t pw = (uint32_t)__builtin_amdgcn_ds_bpermute(wa_, (int)prim_i);
    L.u = got_ ? uw : L.u;
    L.v = got_ ? vw : L.v;
    L.prim = got_ ? pw : L.prim;
  }
  return true;
}

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
// whole wave, one record per lane and trip (see "leaf items" below) — same tests on the same operands, accepted in the same order.
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
    Hit *hp_ = a.hits;                                  \
    uint8_t *mp_ = a.mask;                              \
    if (multi) {                                        \
      const BatchPtrs bp_ = s_tbl[batch_of<T>(a, rid)]; \
      hp_ = (Hit *)bp_.hits_v;                          \
      mp_ = bp_.mask_v;                                 \
    }                                                   \
    if (hp_) store_hit_nt<T>(hp_ + rid, h_);            \
    if (mp_) mp_[rid] = hit_ ? (KIND == kPrimCylinders ? (uint8_t)(1u | (L.cap << 1)) : (uint8_t)1) : (uint8_t)0; \
  } while (0)

  // The skip id of the ray a lane holds (`live_`: it holds one and waits at a leaf), into skip_: the launch's, or with per-ray skip
  // ids (common.h TraverseArgs::skip_ids; a multi-batch launch: its batch's array, or none) the ray's own, re-read at every leaf by the
  // index the lane keeps for its output — so whoever works on a ray (its lane after a refill, a quad of the tail) tests against ITS id.
#define NRT_RAY_SKIP(skip_, live_)                                                                     \
  uint32_t skip_ = a.skip_prim;                                                                        \
  if constexpr (!PLAIN && KIND == kPrimTriangles) {                                                    \
    const uint32_t *ids_ = a.skip_ids;                                                                 \
    if (multi) ids_ = s_tbl[batch_of<T>(a, rid)].skip_v;                                               \
    if ((live_) && ids_ != nullptr) skip_ = ids_[rid];                                                 \
  }                                                                                                    \
  (void)skip_

  // One primitive record (slot `slot_` of the leaf-ordered arrays) against a lane's ray; `act_` false -> no effect.
  // (`skip` is the leaf phase's: NRT_RAY_SKIP)
#define NRT_TEST_PRIM(slot_, act_)                                                                     \
  do {                                                                                                 \
    if (KIND == kPrimSpheres) {                                                                        \
      const LeafSphere<T> sp_ = a.spheres[(slot_)];                                                    \
      sphere_test<T>(L, sp_, (act_), a.range0, a.range1);                                              \
    } else if (KIND == kPrimCylinders) {                                                               \
      const LeafCylinder<T> cy_ = a.cylinders[(slot_)];                                                \
      cylinder_test<T>(L, cy_, (act_), a.range0, a.range1, a.cyl_test_cap != 0u);                      \
    } else if constexpr (KIND == kPrimCurves) { /* (compile-time: no other instantiation sees it) */   \
      const LeafCurve cv_ = a.curves[(slot_)];                                                         \
      curve_test<T>(L, cv_, (act_), a.range0, a.range1, a.curve_subdiv);                               \
    } else {                                                                                           \
      const LeafTri<T> tri_ = a.tris[(slot_)];                                                         \
      if (PLAIN)                                                                                       \
        tri_test<T, true>(L, tri_, (act_), 0u, 0u, 0u, false);                                         \
      else                                                                                             \
        tri_test<T>(L, tri_, (act_), a.range0, a.range1, skip, cull);                                  \
    }                                                                                                  \
  } while (0)

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
          const Ray *rp_ = a.rays;
          uint32_t bq_ = 0u; // this ray belongs to an occlusion-query batch
          if (multi) {
            const uint32_t b_ = batch_of<T>(a, rid);
            rp_ = (const Ray *)s_tbl[b_].rays_v;
            bq_ = (a.batch_anyhit >> b_) & 1u;
          }
          const Ray r = (a.debug_flags & 4u) ? rp_[rid] : load_ray_nt<T>(rp_ + rid);
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
            const RecOff rec_ = (RecOff)cur << 7; // (32 bits: api.hip sends arrays of 4 GiB and more to the ORDER & 4 instantiations)
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
        // whose leaves hold more than four records do not take this variant at all (api.hip).
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
        for (uint32_t i = 0; __ballot(i < cnt) != 0ull; i += NRT_SPHERE_UNROLL) {
          LeafSphere<T> s_[NRT_SPHERE_UNROLL];
#pragma unroll
          for (uint32_t j = 0; j < NRT_SPHERE_UNROLL; j++) s_[j] = a.spheres[first + (i + j < cnt ? i + j : 0u)];
#pragma unroll
          for (uint32_t j = 0; j < NRT_SPHERE_UNROLL; j++) sphere_test<T>(L, s_[j], i + j < cnt, a.range0, a.range1);
        }
      } else
      for (uint32_t i = 0; __ballot(i < cnt) != 0ull; i++) {
        if (STATS) {
          st_it2++;
          st_act2 += (unsigned)__builtin_popcountll(__ballot(i < cnt));
          if (i < cnt) st_tris++;
        }
        // no divergent region here: lanes past their count re-test their first record with ok = false
        NRT_TEST_PRIM(first + (i < cnt ? i : 0u), i < cnt);
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
#undef NRT_TEST_PRIM
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

// ---------------------------------------------------------------------------
// Two-level (instanced) traversal, nanosg::Scene::Traverse (examples/nanosg/nanosg.h:778-870) for a whole batch in ONE
// launch.  A ray arrives with the list of instances whose world boxes it enters, nearest entry first (at most 64:
// BVHAccel::ListNodeIntersections, nanort.h:2608-2692 — built by scene.hip's listing kernel over the top-level BVH).
// The lane then does what the reference's loop does, candidate after candidate: skip the instance if the nearest world
// distance so far is below its entry distance (nanosg.h:795), else carry the ray into the instance's space (MultV with
// inv_xform / inv_xform33, :806-808, the local interval left at Ray()'s defaults), walk the instance's OWN tree with the
// single-level machinery above (same WideNode step, same watertight test, same order: the local record is what
// nrtTraverseBatchDevice would return for that local ray, bit for bit), measure the world distance of the local hit
// (:823-836) and keep it if strictly nearer (:838).  Lanes of a wave are at different candidates of different instances
// at the same time — every lane carries its instance's array bases — so there is no per-instance launch, no compaction
// and no host round trip; the wave alternates between the inner-node phase and the leaf phase like k_traverse_wide.
// A lane whose ray is finished takes the next one from a per-partition work cursor (a wave refills once `refill_min` lanes are
// free).  Since round 4 this kernel traces small scenes and the rays the single-pass walk (k_scene_walk, below) hands over;
// scenes of thousands of instances go through that walk, which keeps no list at all.
// ---------------------------------------------------------------------------
// A record fetched through a per-lane pointer that came out of memory (an instance's array bases in the scene kernels) is a FLAT
// access as far as the compiler can tell — flat loads also take a slot of the LDS queue and wait on both counters.  These
// pointers are device-memory addresses: say so (address space 1) and the loads become global_load.
template <typename R>
__device__ __forceinline__ R load_global_record(const R *p) {
  R r;
  if constexpr (sizeof(R) % 16 == 0 && alignof(R) >= 16) {
    typedef uint32_t u4g __attribute__((ext_vector_type(4)));
    const u4g __attribute__((address_space(1))) *g = (const u4g __attribute__((address_space(1))) *)p;
    u4g *d = reinterpret_cast<u4g *>(&r);
#pragma unroll
    for (unsigned q = 0; q < sizeof(R) / 16; q++) d[q] = g[q];
  } else {
    static_assert(sizeof(R) % 4 == 0, "whole words");
    const uint32_t __attribute__((address_space(1))) *g = (const uint32_t __attribute__((address_space(1))) *)p;
    uint32_t *d = reinterpret_cast<uint32_t *>(&r);
#pragma unroll
    for (unsigned q = 0; q < sizeof(R) / 4; q++) d[q] = g[q]; // (neighbouring words: the compiler merges them into the widest loads the alignment allows)
  }
  return r;
}
enum : int { S_NEXT = 4, S_FIN = 5, S_DONE = 6 }; // besides W_TRAV / W_LEAF / W_POP: pick the next candidate / a local walk ended / ray finished

__device__ __forceinline__ void scene_mult_v(float dst[3], const float m[4][4], const float v[3]) { // Matrix::MultV, nanosg.h:232-240
  const float t0 = m[0][0] * v[0] + m[1][0] * v[1] + m[2][0] * v[2] + m[3][0];
  const float t1 = m[0][1] * v[0] + m[1][1] * v[1] + m[2][1] * v[2] + m[3][1];
  const float t2 = m[0][2] * v[0] + m[1][2] * v[1] + m[2][2] * v[2] + m[3][2];
  dst[0] = t0;
  dst[1] = t1;
  dst[2] = t2;
}

// SCAN: a scene of a handful of instances (a.scan_nodes of them): the lane lists the instances its ray enters ITSELF when it fetches
// the ray — every world box tested in id order, exactly what the listing kernel of such scenes did in a launch of its own
// (scene.hip k_scene_list) — into its own slots of the list arrays, which it alone reads back: one launch per batch, no second
// pass over the rays.
// ANY: the occlusion query (nrtSceneOccludedBatch*): only the flag is wanted.  The flag of the closest-hit form is "some candidate
// the loop opens has a local hit whose world distance is < FLT_MAX" — the first such hit sets it and nothing clears it, and until
// that hit the nearest distance is still FLT_MAX, so the cull (nanosg.h:795) opens the same candidates in both forms.  So the ANY
// form walks the same candidates in the same order, lets a local walk drop its stack at the first leaf that accepts a primitive
// (the single-level any-hit rule of k_traverse_wide), and finishes the ray with flag 1 at the first local hit with
// t_world < FLT_MAX.  It writes no record (a.hits is not read).  The one place the forms can differ: the dropped walk's hit is the
// first accepted, not the nearest, and where world distances overflow or are NaN the two may disagree on t_world < FLT_MAX
// (include/nanort_hip.h states that limit).
template <int STACK, bool SCAN, bool ANY = false>
__global__ __launch_bounds__(kTraverseBlock) void k_scene_trace(const SceneTraceArgs a) {
  typedef float T;
  typedef StackEntry<float> SE;
  __shared__ SE::type s_stack[STACK][kTraverseBlock];

  const unsigned tid = threadIdx.x;
  const unsigned lane = lane_id();
  const unsigned gslot = blockIdx.x * kTraverseBlock + tid;
  const LaneStack<SE, STACK, SceneTraceArgs> stk = {a, tid, gslot};

  // Persistent threads: a lane whose ray is finished takes the next one from a work cursor (claimed for the whole wave by
  // one atomic once `refill_min` lanes are free), so a wave keeps its lanes busy to the end of the batch instead of
  // waiting for the slowest of 64 fixed rays.
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
        // one cursor per ray partition (== XCD, as in k_traverse_wide): a wave drains its home range first, so an XCD walks one
        // band of the batch and its L2 keeps one part of the scene; then it steals from the others
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
            for (uint32_t k = 0; k < a.scan_nodes; k++) { // (wave-uniform addresses: the boxes arrive through the scalar cache)
              float t;
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
          if constexpr (!ANY) {
          nrt_scene_hit_f32 h; // the miss record; overwritten by every strictly nearer hit
          h.t = r.max_t;
          h.u = 0.0f;
          h.v = 0.0f;
          h.prim_id = 0xFFFFFFFFu;
          h.node_id = 0xFFFFFFFFu;
          a.hits[ri] = h;
          }
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
        const SceneInst &nd = a.insts[inst];
        float lp[3], wp[3];
        lp[0] = L.org0 + L.hit_t * L.d0; // nanosg.h:823-825
        lp[1] = L.org1 + L.hit_t * L.d1;
        lp[2] = L.org2 + L.hit_t * L.d2;
        scene_mult_v(wp, nd.xform, lp);
        const float px = wp[0] - worg[0], py = wp[1] - worg[1], pz = wp[2] - worg[2];
        const float t_world = __builtin_sqrtf(px * px + py * py + pz * pz); // vlength, nanort.h:383-385
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
          nrt_ray_f32 lr;
          scene_mult_v(lr.org, nd.inv_xform, worg);   // nanosg.h:807
          scene_mult_v(lr.dir, nd.inv_xform33, wdir); // nanosg.h:808
          lr.min_t = 0.0f;                            // Ray() defaults (nanort.h:477-487): the world interval is not propagated
          lr.max_t = 3.402823466e+38f;
          lr.type = 0;
          lane_init<float>(L, lr);
          wide = (const WideNode<float> *)nd.wide;
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
      if (state == W_LEAF) leaf_span(packed, nodes, cur, lcnt, first);
      for (uint32_t k = 0; __ballot(k < lcnt) != 0ull; k += 2u) { // two records per trip, as in k_traverse_wide
        if (k < lcnt) { // (divergent on purpose: the lanes' record arrays differ)
          const bool two = k + 1u < lcnt;
          const LeafTri<float> t0 = load_global_record(tris + first + k);
          const LeafTri<float> t1 = load_global_record(tris + first + (two ? k + 1u : k));
          tri_test<float, true>(L, t0, true, 0u, 0u, 0u, false); // default trace options (nanosg.h:817)
          tri_test<float, true>(L, t1, two, 0u, 0u, 0u, false);
        }
      }
      // occlusion query: any accepted primitive settles this instance — drop what is left of its stack (as k_traverse_wide does)
      if constexpr (ANY) sp = (state == W_LEAF && L.hit_t < L.max_t) ? 0 : sp;
      state = (state == W_LEAF) ? W_POP : state;
    }
  }
}

static const void *scene_trace_kernel(bool scan) {
  return scan ? (const void *)k_scene_trace<kSceneLdsStack, true> : (const void *)k_scene_trace<kSceneLdsStack, false>;
}
static const void *scene_trace_any_kernel(bool scan) {
  return scan ? (const void *)k_scene_trace<kSceneLdsStack, true, true> : (const void *)k_scene_trace<kSceneLdsStack, false, true>;
}
hipError_t launch_scene_trace(const SceneTraceArgs &args, unsigned grid, hipStream_t s) {
  if (args.n == 0) return hipSuccess;
  launch_persistent(args.any_hit ? scene_trace_any_kernel(args.scan_nodes != 0) : scene_trace_kernel(args.scan_nodes != 0), grid, args, s);
  return hipGetLastError();
}
int scene_trace_blocks_per_cu() { // (one grid size for both: the fewer)
  return std::min(resident_blocks(scene_trace_kernel(false), 4), resident_blocks(scene_trace_kernel(true), 8));
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

template <int STACK, bool STATS, bool ANY = false>
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
    // ---- refill free lanes (as k_scene_trace) -------------------------------------------------------------------------
    {
      const unsigned long long free_lanes = __ballot(state == S_DONE);
      const unsigned want = (unsigned)__builtin_popcountll(free_lanes);
      if (!exhausted && want >= a.refill_min) {
        const uint32_t per = a.n / a.num_parts;
        uint32_t mine = a.n;
        while (tried < a.num_parts) {
          const uint32_t lo = part * per, len = (part + 1u == a.num_parts) ? a.n - lo : per;
          uint32_t b0 = 0;
          if (lane == (unsigned)__builtin_ctzll(free_lanes)) b0 = atomicAdd(a.cursor + kCursorStrideWords * part, want);
          b0 = (uint32_t)__builtin_amdgcn_readlane((int)b0, __builtin_ctzll(free_lanes));
          if (b0 < len) {
            const uint32_t off = b0 + (uint32_t)__builtin_popcountll(free_lanes & ((1ull << lane) - 1ull));
            mine = off < len ? lo + off : a.n;
            break;
          }
          part = (part + 1u == a.num_parts) ? 0u : part + 1u;
          tried++;
        }
        exhausted = tried >= a.num_parts;
        if (state == S_DONE && mine < a.n) {
          i = mine;
          const nrt_ray_f32 r = a.rays[i];
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
          {
            best_t = 3.402823466e+38f; // t_nearest = numeric_limits<T>::max(), nanosg.h:787
            best_tmin = 0.f;
            best_id = 0u;
            t2 = __builtin_huge_valf();
            cull_t = __builtin_huge_valf();
            has_hit = false;
            traced = 0u;
            if constexpr (!ANY) {
            nrt_scene_hit_f32 h; // the miss record; overwritten by every better hit
            h.t = r.max_t;
            h.u = 0.0f;
            h.v = 0.0f;
            h.prim_id = 0xFFFFFFFFu;
            h.node_id = 0xFFFFFFFFu;
            a.hits[i] = h;
            }
            sp = 0;
            world_ray();
            cur = 0u; // record 0 == the root branch (its own box test is implied by its children's)
            state = W_TRAV;
          }
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
            const SceneInst &nd = a.insts[inst]; // (the full record, by id: only an instance that was hit needs its xform)
            float lp[3], wp[3];
            lp[0] = L.org0 + L.hit_t * L.d0; // nanosg.h:823-825
            lp[1] = L.org1 + L.hit_t * L.d1;
            lp[2] = L.org2 + L.hit_t * L.d2;
            scene_mult_v(wp, nd.xform, lp);
            const float px = wp[0] - worg[0], py = wp[1] - worg[1], pz = wp[2] - worg[2];
            const float t_world = __builtin_sqrtf(px * px + py * py + pz * pz); // vlength, nanort.h:383-385
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
          const bool entered = tmn <= tmx && e <= f;
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
            nrt_ray_f32 lr;
            // Matrix::MultV (nanosg.h:232-240) with inv_xform / inv_xform33 (:807-808), the twelve entries it reads
            lr.org[0] = nd.inv[0][0] * worg[0] + nd.inv[1][0] * worg[1] + nd.inv[2][0] * worg[2] + nd.inv[3][0];
            lr.org[1] = nd.inv[0][1] * worg[0] + nd.inv[1][1] * worg[1] + nd.inv[2][1] * worg[2] + nd.inv[3][1];
            lr.org[2] = nd.inv[0][2] * worg[0] + nd.inv[1][2] * worg[1] + nd.inv[2][2] * worg[2] + nd.inv[3][2];
            lr.dir[0] = nd.inv33[0][0] * wdir[0] + nd.inv33[1][0] * wdir[1] + nd.inv33[2][0] * wdir[2] + nd.inv33[3][0];
            lr.dir[1] = nd.inv33[0][1] * wdir[0] + nd.inv33[1][1] * wdir[1] + nd.inv33[2][1] * wdir[2] + nd.inv33[3][1];
            lr.dir[2] = nd.inv33[0][2] * wdir[0] + nd.inv33[1][2] * wdir[1] + nd.inv33[2][2] * wdir[2] + nd.inv33[3][2];
            lr.min_t = 0.0f; // Ray() defaults (nanort.h:477-487): the world interval is not propagated
            lr.max_t = 3.402823466e+38f;
            lr.type = 0;
            lane_init<float>(L, lr);
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
      if (state == W_LEAF) { // (packed leaf references: scene.hip checks)
        lcnt = packed_leaf_count(cur);
        first = packed_leaf_first(cur);
      }
      // (few lanes wait at a leaf in this kernel — 10 of 64 on the instanced scenes: their records nearly always fit one trip)
      const bool items_done_ = !STATS && a.leaf_items != 0u &&
                               leaf_items_one_trip<true, const LeafTri<float> *>(L, lcnt, nullptr, tris + first, lane, s_item_owner[tid / kWave], s_item_rec[tid / kWave], 0u, 0u, 0u, false);
      if (!items_done_)
      for (uint32_t k = 0; __ballot(k < lcnt) != 0ull; k += 2u) {
        if (STATS) {
          st[6]++;
          st[7] += (unsigned)__builtin_popcountll(__ballot(k < lcnt));
        }
        if (k < lcnt) {
          const bool two = k + 1u < lcnt;
          const LeafTri<float> t0 = load_global_record(tris + first + k);
          const LeafTri<float> t1 = load_global_record(tris + first + (two ? k + 1u : k));
          tri_test<float, true>(L, t0, true, 0u, 0u, 0u, false); // default trace options (nanosg.h:817)
          tri_test<float, true>(L, t1, two, 0u, 0u, 0u, false);
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
  if (args.any_hit)
    hipLaunchKernelGGL((k_scene_walk<kSceneWalkLdsStack, false, true>), dim3(grid), dim3(kTraverseBlock), 0, s, args);
  else
    hipLaunchKernelGGL((k_scene_walk<kSceneWalkLdsStack, false>), dim3(grid), dim3(kTraverseBlock), 0, s, args);
  return hipGetLastError();
}
int scene_walk_blocks_per_cu() { return resident_blocks((const void *)k_scene_walk<kSceneWalkLdsStack, false>, 3); }

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
