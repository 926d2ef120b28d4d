// nanort_amd/csrc/walk_dev.h — the moves every WIDE walk shares (a step tests the two boxes of a WideNode or the four of a
// Wide4Node; stack entries carry their t_min): the box tests, the stack entry, the pop / push / step macros and their contract, the
// leaf items and the typed global record load.  Included by the two files that hold wide walks: traverse.hip (k_traverse_wide) and
// scene_kernels.hip (k_scene_trace, k_scene_walk).  What the binary walk (binary_walk_dev.h) needs as well — ray setup, slab and
// primitive tests, LaneStack, the host side of a persistent launch — is traverse_dev.h's.
#pragma once

#include "traverse_dev.h"

namespace nrt {

// Lane states of the wide walks.
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

#ifndef NRT_W4_FAST_PUSH
#define NRT_W4_FAST_PUSH 1 // two-level step: unconditional stores of the three push candidates when every lane has room in LDS
#endif

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
// NRT_ITEMS_DS: the two arrays are rows of the block's LDS that arrive here as pointers.  As generic volatile pointers (0) every one
// of the up to eight stores and two loads of a trip was a `flat_… sc0 sc1` access followed by its own s_waitcnt vmcnt(0): ten
// memory round trips one after the other in every leaf phase of the steady state.  As local-address-space pointers (1) they are
// ds_write_b32 / ds_read_b32, issued back to back and waited for once (profiles/r12a_tail_rows.txt).
#ifndef NRT_ITEMS_DS
#define NRT_ITEMS_DS 1
#endif
#ifndef NRT_ITEMS_FETCH4
#define NRT_ITEMS_FETCH4 1
#endif
template <bool PLAIN, typename SLOT>
__device__ __forceinline__ bool leaf_items_one_trip(Lane<float> &L, uint32_t cnt, const LeafTri<float> *base, SLOT first, unsigned lane, uint32_t *own_row,
                                                    SLOT *rec_row, uint32_t range0, uint32_t range1, uint32_t skip_prim, bool cull) {
  typedef float T;
#if NRT_ITEMS_DS
  uint32_t NRT_LDS *const own_ = as_lds(own_row);
  SLOT NRT_LDS *const rec_ = as_lds(rec_row);
#else
  volatile uint32_t *const own_ = own_row;
  volatile SLOT *const rec_ = rec_row;
#endif
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
  // (LDS operations of one wave are performed in issue order, and the compiler keeps the reads below behind the writes: for all it
  // can tell item `me_` is one of the lane's own.  The fence says so as well; at this scope it costs no instruction.)
#if NRT_ITEMS_DS
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#endif
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
#if NRT_ITEMS_FETCH4
  // (the distances of an owner's up to four items fetched together: one wait for all of them instead of one per record; the
  // accept sequence below is the same — a record beyond the owner's count is not `okk`)
  T tt4_[4];
#pragma unroll
  for (uint32_t k2_ = 0; k2_ < 4u; k2_++) tt4_[k2_] = __int_as_float(__builtin_amdgcn_ds_bpermute((int)(((base_ + k2_) & 63u) << 2), __float_as_int(tt_i)));
  (void)kmax_;
#pragma unroll
  for (uint32_t k2_ = 0; k2_ < 4u; k2_++) {
    const uint32_t src_ = (base_ + k2_) & 63u;
    const T ttk = tt4_[k2_];
#else
  for (uint32_t k2_ = 0; k2_ < kmax_; k2_++) {
    const uint32_t src_ = (base_ + k2_) & 63u;
    const T ttk = __int_as_float(__builtin_amdgcn_ds_bpermute((int)(src_ << 2), __float_as_int(tt_i)));
#endif
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

} // namespace nrt
