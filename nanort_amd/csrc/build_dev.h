// nanort_amd/csrc/build_dev.h — the builder's device vocabulary (build.hip, build_subtree.hip): the types and constants
// that define the tree, the integer-image and lane helpers, and the split rule — bins, cost, cut search pieces, leaf rule,
// partition predicate, object-median fallback — each stated once.  Internal to the builder: not part of kernels.h.
#pragma once
#include "common.h"
#include "minmax_dev.h"

namespace nrt {

constexpr int kSmall = 256;     // nodes at or below this many primitives are binned with kSmallBins bins (part of the tree's definition)
#ifndef NRT_BUILD_HANDOFF
#define NRT_BUILD_HANDOFF 256
#endif
// Nodes at or below this many primitives leave the level-synchronous top phase for the one-wave-per-node subtree phase.
// Both phases take the same decisions for a node (same bins — see node_bins —, same cost, same tie rules, same leaf rule),
// so this is a scheduling knob: any value <= kSmall gives the same tree (tools/tree_hash.py).
constexpr int kHandoff = NRT_BUILD_HANDOFF;
static_assert(kHandoff <= kSmall && kHandoff >= 64, "hand-off size");
constexpr int kMaxBins = 64;    // top phase: lane == bin
constexpr int kSmallBins = 16;  // subtree phase: 3 x 15 candidates == 45 lanes
constexpr uint32_t kMedian = 0xFFFFFFFFu;
constexpr int kSubStackSafe = 36; // above this many, splits are forced to the object median (depth <= log2 n more)

enum : uint32_t { KIND_SPLIT = 0, KIND_SMALL = 1, KIND_LEAF = 2 };

// ---- order-preserving integer images of floating-point values ---------------
template <typename T>
struct Ord;
template <>
struct Ord<float> {
  typedef uint32_t U;
  static __host__ __device__ __forceinline__ U enc(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  static __host__ __device__ __forceinline__ float dec(U e) {
    uint32_t u = (e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
  }
  static __host__ __device__ __forceinline__ U lowest() { return 0u; }
  static __host__ __device__ __forceinline__ U highest() { return 0xFFFFFFFFu; }
};
template <>
struct Ord<double> {
  typedef unsigned long long U;
  static __host__ __device__ __forceinline__ U enc(double f) {
    unsigned long long u;
    __builtin_memcpy(&u, &f, 8);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
  }
  static __host__ __device__ __forceinline__ double dec(U e) {
    unsigned long long u = (e & 0x8000000000000000ull) ? (e & 0x7FFFFFFFFFFFFFFFull) : ~e;
    double f;
    __builtin_memcpy(&f, &u, 8);
    return f;
  }
  static __host__ __device__ __forceinline__ U lowest() { return 0ull; }
  static __host__ __device__ __forceinline__ U highest() { return 0xFFFFFFFFFFFFFFFFull; }
};

// Primitive record carried (and physically partitioned) through the build.
template <typename T>
struct alignas(8) PrimRec {
  T bmin[3];
  T bmax[3];
  T c[3];
  uint32_t prim;
};
static_assert(sizeof(PrimRec<float>) == 40, "PrimRec<float>");
static_assert(sizeof(PrimRec<double>) == 80, "PrimRec<double>");

template <typename T>
struct TopNode {
  T bmin[3], bmax[3]; // node AABB
  T cmin[3], cmax[3]; // centroid bounds
  uint32_t l, r;      // primitive range
  uint32_t depth;
  uint32_t kind;
  int32_t axis;
  uint32_t split_bin; // kMedian: object-median fallback (reference nanort.h:1849)
  uint32_t nleft;
  uint32_t child0;    // top index of the low-side child; high side is child0 + 1
  uint32_t size;      // nodes in this subtree
  uint32_t dfs;       // final node index
  uint32_t buf;       // record buffer holding [l, r) once the node stops splitting
  uint32_t chunk_base, nchunks;
  uint32_t parent;    // top index of the parent | kHighChild when this is its high-side child; kNoParent for node 0
};
constexpr uint32_t kHighChild = 0x80000000u, kNoParent = 0x7FFFFFFFu;

template <typename T>
struct BoundsAcc { // integer-ordered images: bmin[3] bmax[3] cmin[3] cmax[3]
  typename Ord<T>::U v[12];
};

constexpr int kMaxTopLevels = 120; // top-phase levels recorded for the relayout

// Device-resident state of the top phase: the host launches level after level with
// upper-bound grids and reads this back only to decide when to stop.
struct LevelInfo {
  uint32_t num_active;  // SPLIT nodes of the level being processed
  uint32_t num_chunks;
  uint32_t num_small;   // running count of subtree tasks (all levels)
  uint32_t max_depth;   // stats
  uint32_t num_leaves;
  uint32_t num_branches;
  uint32_t max_leaf_count;
  uint32_t error;       // 1: top array capacity exceeded
  uint32_t cand_begin, cand_end; // top nodes created by the previous level (candidates for this one)
  uint32_t top_count;   // top nodes allocated so far
  uint32_t child_base;  // first top index of the children created by the level being processed
  uint32_t top_cap;
  uint32_t num_levels;  // levels recorded in level_begin
  uint32_t num_nodes;   // nodes of the finished tree (k_layout)
  uint32_t level_begin[kMaxTopLevels + 2];
};

template <typename T>
__device__ __forceinline__ T bin_scale(T lo, T hi, int K) {
  const T ext = hi - lo;
  return (ext > T(0)) ? T(K) / ext : T(0);
}
// Bins of a node of n primitives: `kpack` carries the build's bin count for large nodes (low byte) and the one for nodes
// of at most kSmall primitives (second byte) — the subtree phase's lane == (axis, bin) layout holds 16.
__device__ __forceinline__ int node_bins(int kpack, uint32_t n) { return n <= (uint32_t)kSmall ? ((kpack >> 8) & 0xFF) : (kpack & 0xFF); }
template <typename T>
__device__ __forceinline__ int bin_of(T c, T lo, T scale, int K) {
  int i = (int)((c - lo) * scale);
  i = i < 0 ? 0 : i;
  return i > K - 1 ? K - 1 : i;
}
template <typename T>
__device__ __forceinline__ T half_area(const T mn[3], const T mx[3]) {
  const T a = mx[0] - mn[0], b = mx[1] - mn[1], c = mx[2] - mn[2];
  return a * b + b * c + c * a; // CalculateSurfaceArea / 2 (nanort.h:1278-1283)
}

// ---- DPP (data-parallel primitive) moves inside 16-lane rows: VALU operand modifiers, no LDS
// crossbar (ds_bpermute) round trip.  row_shr:n = 0x110+n, row_shl:n = 0x100+n; a lane without a
// source keeps `old`, so `old` = the identity of the operation gives a clean scan step.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t old, uint32_t src) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)src, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float old, float src) {
  return __builtin_bit_cast(float, dpp_u32<CTRL>(__builtin_bit_cast(uint32_t, old), __builtin_bit_cast(uint32_t, src)));
}
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double old, double src) {
  const unsigned long long o = __builtin_bit_cast(unsigned long long, old), v = __builtin_bit_cast(unsigned long long, src);
  const uint32_t lo = dpp_u32<CTRL>((uint32_t)o, (uint32_t)v), hi = dpp_u32<CTRL>((uint32_t)(o >> 32), (uint32_t)(v >> 32));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t old, uint32_t src) {
  return dpp_u32<CTRL>(old, src);
}

// Wave-uniform broadcast of lane `src` (an SGPR): v_readlane, no LDS crossbar round trip.
__device__ __forceinline__ uint32_t lane_bcast(uint32_t x, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)x, src); }
__device__ __forceinline__ float lane_bcast(float x, int src) {
  return __builtin_bit_cast(float, lane_bcast(__builtin_bit_cast(uint32_t, x), src));
}
__device__ __forceinline__ double lane_bcast(double x, int src) {
  const unsigned long long v = __builtin_bit_cast(unsigned long long, x);
  const uint32_t lo = lane_bcast((uint32_t)v, src), hi = lane_bcast((uint32_t)(v >> 32), src);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ unsigned long long lane_bcast(unsigned long long v, int src) {
  const uint32_t lo = lane_bcast((uint32_t)v, src), hi = lane_bcast((uint32_t)(v >> 32), src);
  return ((unsigned long long)hi << 32) | lo;
}
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_mov(unsigned long long old, unsigned long long src) {
  const uint32_t lo = dpp_u32<CTRL>((uint32_t)old, (uint32_t)src), hi = dpp_u32<CTRL>((uint32_t)(old >> 32), (uint32_t)(src >> 32));
  return ((unsigned long long)hi << 32) | lo;
}
// The subtree kernel is bound by VALU issue (a wave instruction costs the same for 5 active lanes as for 64), so its
// scans and reductions run on the ORDER-PRESERVING INTEGER IMAGES of the values (Ord<T>): for fp32 the compiler then
// folds each DPP move into the v_min_u32 / v_max_u32 that consumes it — one instruction per scan step and value where
// the float form (compare + select on a separately moved operand) takes three.
template <typename U>
__device__ __forceinline__ U umin_(U a, U b) {
  return a < b ? a : b;
}
template <typename U>
__device__ __forceinline__ U umax_(U a, U b) {
  return a > b ? a : b;
}
template <typename T, int CTRL>
__device__ __forceinline__ void row_scan_step_e(uint32_t &cnt, typename Ord<T>::U mn[3], typename Ord<T>::U mx[3]) {
  cnt += dpp_mov<CTRL>(0u, cnt);
#pragma unroll
  for (int d = 0; d < 3; d++) {
    mn[d] = umin_(mn[d], dpp_mov<CTRL>(Ord<T>::highest(), mn[d]));
    mx[d] = umax_(mx[d], dpp_mov<CTRL>(Ord<T>::lowest(), mx[d]));
  }
}
template <typename T>
__device__ __forceinline__ void row_prefix_e(uint32_t &cnt, typename Ord<T>::U mn[3], typename Ord<T>::U mx[3]) {
  row_scan_step_e<T, 0x111>(cnt, mn, mx);
  row_scan_step_e<T, 0x112>(cnt, mn, mx);
  row_scan_step_e<T, 0x114>(cnt, mn, mx);
  row_scan_step_e<T, 0x118>(cnt, mn, mx);
}
template <typename T>
__device__ __forceinline__ void row_suffix_e(uint32_t &cnt, typename Ord<T>::U mn[3], typename Ord<T>::U mx[3]) {
  row_scan_step_e<T, 0x101>(cnt, mn, mx);
  row_scan_step_e<T, 0x102>(cnt, mn, mx);
  row_scan_step_e<T, 0x104>(cnt, mn, mx);
  row_scan_step_e<T, 0x108>(cnt, mn, mx);
}
// All-reduce min / max with a wave-uniform result: 4 DPP steps leave every lane with its row's value (quad_perm
// [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror; `old` = the identity so that the move folds into the min / max),
// the four rows are combined through scalar registers.
template <typename U>
__device__ __forceinline__ U wave_umin(U x) {
  x = umin_(x, dpp_mov<0xB1>((U)~(U)0, x));
  x = umin_(x, dpp_mov<0x4E>((U)~(U)0, x));
  x = umin_(x, dpp_mov<0x141>((U)~(U)0, x));
  x = umin_(x, dpp_mov<0x140>((U)~(U)0, x));
  return umin_(umin_(lane_bcast(x, 0), lane_bcast(x, 16)), umin_(lane_bcast(x, 32), lane_bcast(x, 48)));
}
template <typename U>
__device__ __forceinline__ U wave_umax(U x) {
  x = umax_(x, dpp_mov<0xB1>((U)0, x));
  x = umax_(x, dpp_mov<0x4E>((U)0, x));
  x = umax_(x, dpp_mov<0x141>((U)0, x));
  x = umax_(x, dpp_mov<0x140>((U)0, x));
  return umax_(umax_(lane_bcast(x, 0), lane_bcast(x, 16)), umax_(lane_bcast(x, 32), lane_bcast(x, 48)));
}
template <typename T>
__device__ __forceinline__ T wave_min_u(T x) {
  return Ord<T>::dec(wave_umin<typename Ord<T>::U>(Ord<T>::enc(x)));
}
template <typename T>
__device__ __forceinline__ T wave_max_u(T x) {
  return Ord<T>::dec(wave_umax<typename Ord<T>::U>(Ord<T>::enc(x)));
}

// Inclusive scans over all 64 lanes (k_split: lane == bin, up to 64 bins): the row scans above, then each row takes
// the totals of the rows before (prefix) / after (suffix) it, which travel through scalar registers.
template <typename U, bool MIN>
__device__ __forceinline__ U row_carry(U x, U t_a, U t_b, U t_c, unsigned row, bool prefix) {
  // prefix: t_a, t_b, t_c = totals of rows 0, 1, 2;  suffix: totals of rows 1, 2, 3
  const U id = MIN ? (U) ~(U)0 : (U)0;
  auto op = [](U p, U q) { return MIN ? umin_(p, q) : umax_(p, q); };
  U c;
  if (prefix)
    c = row == 0 ? id : (row == 1 ? t_a : (row == 2 ? op(t_a, t_b) : op(op(t_a, t_b), t_c)));
  else
    c = row == 3 ? id : (row == 2 ? t_c : (row == 1 ? op(t_b, t_c) : op(op(t_a, t_b), t_c)));
  return op(x, c);
}
template <typename T>
__device__ __forceinline__ void wave_prefix_e(uint32_t &cnt, typename Ord<T>::U mn[3], typename Ord<T>::U mx[3], unsigned lane) {
  typedef typename Ord<T>::U U;
  row_prefix_e<T>(cnt, mn, mx);
  const unsigned row = lane >> 4;
  const uint32_t c0 = lane_bcast(cnt, 15), c1 = lane_bcast(cnt, 31), c2 = lane_bcast(cnt, 47);
  cnt += row == 0 ? 0u : (row == 1 ? c0 : (row == 2 ? c0 + c1 : c0 + c1 + c2));
#pragma unroll
  for (int d = 0; d < 3; d++) {
    mn[d] = row_carry<U, true>(mn[d], lane_bcast(mn[d], 15), lane_bcast(mn[d], 31), lane_bcast(mn[d], 47), row, true);
    mx[d] = row_carry<U, false>(mx[d], lane_bcast(mx[d], 15), lane_bcast(mx[d], 31), lane_bcast(mx[d], 47), row, true);
  }
}
template <typename T>
__device__ __forceinline__ void wave_suffix_e(uint32_t &cnt, typename Ord<T>::U mn[3], typename Ord<T>::U mx[3], unsigned lane) {
  typedef typename Ord<T>::U U;
  row_suffix_e<T>(cnt, mn, mx);
  const unsigned row = lane >> 4;
  const uint32_t c1 = lane_bcast(cnt, 16), c2 = lane_bcast(cnt, 32), c3 = lane_bcast(cnt, 48);
  cnt += row == 3 ? 0u : (row == 2 ? c3 : (row == 1 ? c2 + c3 : c1 + c2 + c3));
#pragma unroll
  for (int d = 0; d < 3; d++) {
    mn[d] = row_carry<U, true>(mn[d], lane_bcast(mn[d], 16), lane_bcast(mn[d], 32), lane_bcast(mn[d], 48), row, false);
    mx[d] = row_carry<U, false>(mx[d], lane_bcast(mx[d], 16), lane_bcast(mx[d], 32), lane_bcast(mx[d], 48), row, false);
  }
}
// value of lane - 1 (lane 0: `first`): DPP wave_shr:1
template <typename U>
__device__ __forceinline__ U wave_shr1(U first, U x) {
  return dpp_mov<0x138>(first, x);
}

template <typename U>
__device__ __forceinline__ U row_allmin(U x) { // every lane of a 16-lane row gets the row's minimum
  x = umin_(x, dpp_mov<0xB1>((U) ~(U)0, x));
  x = umin_(x, dpp_mov<0x4E>((U) ~(U)0, x));
  x = umin_(x, dpp_mov<0x141>((U) ~(U)0, x));
  x = umin_(x, dpp_mov<0x140>((U) ~(U)0, x));
  return x;
}
template <typename U>
__device__ __forceinline__ U row_allmax(U x) {
  x = umax_(x, dpp_mov<0xB1>((U)0, x));
  x = umax_(x, dpp_mov<0x4E>((U)0, x));
  x = umax_(x, dpp_mov<0x141>((U)0, x));
  x = umax_(x, dpp_mov<0x140>((U)0, x));
  return x;
}
// (groups of 16, 32 or 64 lanes: shift = 4, 5, 6 — wave-uniform)
template <typename U>
__device__ __forceinline__ U group_allmin(U x, uint32_t shift) {
  x = row_allmin<U>(x);
  if (shift >= 5u) x = umin_(x, (U)__shfl_xor(x, 16));
  if (shift >= 6u) x = umin_(x, (U)__shfl_xor(x, 32));
  return x;
}
template <typename U>
__device__ __forceinline__ U group_allmax(U x, uint32_t shift) {
  x = row_allmax<U>(x);
  if (shift >= 5u) x = umax_(x, (U)__shfl_xor(x, 16));
  if (shift >= 6u) x = umax_(x, (U)__shfl_xor(x, 32));
  return x;
}

// ---------------------------------------------------------------------------
// the split rule: every decision the builder takes for a node, stated once.  The top phase (k_bin / k_split /
// k_partition, build.hip) and the subtree phase (build_subtree.hip) call these, so the two phases cannot drift apart.
// ---------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T pick_axis(const T v[3], int axis) { // v[axis] by selects over the three VALUES: v stays in registers
  const T x = v[0], y = v[1], z = v[2];
  return axis == 0 ? x : (axis == 1 ? y : z);
}

// The reference's leaf rule (nanort.h:1781-1783): a range of at most min_leaf_primitives, or one at the depth cap, is a leaf.
struct LeafRule {
  uint32_t max_depth, leaf_max; // leaf_max = max(min_leaf_primitives, 1)
};
inline LeafRule make_leaf_rule(uint32_t min_leaf, uint32_t max_depth) {
  const LeafRule rule = {max_depth, min_leaf > 1u ? min_leaf : 1u};
  return rule;
}
__device__ __forceinline__ bool is_leaf(uint32_t n, uint32_t depth, LeafRule rule) { return depth >= rule.max_depth || n <= rule.leaf_max; }

// The empty box in integer images — the identity of min / max — which is also what a clean bin holds.
template <typename T>
__device__ __forceinline__ void empty_box_e(typename Ord<T>::U mn[3], typename Ord<T>::U mx[3]) {
#pragma unroll
  for (int d = 0; d < 3; d++) {
    mn[d] = Ord<T>::highest();
    mx[d] = Ord<T>::lowest();
  }
}
template <typename T>
__device__ __forceinline__ void encode_box(const PrimRec<T> &r, typename Ord<T>::U emin[3], typename Ord<T>::U emax[3]) {
#pragma unroll
  for (int d = 0; d < 3; d++) {
    emin[d] = Ord<T>::enc(r.bmin[d]);
    emax[d] = Ord<T>::enc(r.bmax[d]);
  }
}
// A record's bin on each axis: bins span the node's centroid bounds (cmn, scale sc per axis)
template <typename T>
__device__ __forceinline__ void record_bins(const PrimRec<T> &r, const T cmn[3], const T sc[3], int K, int b[3]) {
#pragma unroll
  for (int k = 0; k < 3; k++) b[k] = bin_of<T>(r.c[k], cmn[k], sc[k], K);
}
// One record into a node's LDS bins (cnt[axis][bin], bmin / bmax[axis][bin][xyz]): one count and six min / max atomics per axis.
template <typename T>
__device__ __forceinline__ void bin_record_lds(const PrimRec<T> &r, const T cmn[3], const T sc[3], int K, uint32_t (*cnt)[kSmallBins],
                                               typename Ord<T>::U (*bmin)[kSmallBins][3], typename Ord<T>::U (*bmax)[kSmallBins][3]) {
  typename Ord<T>::U emin[3], emax[3];
  int b[3];
  encode_box<T>(r, emin, emax);
  record_bins<T>(r, cmn, sc, K, b);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    atomicAdd(&cnt[k][b[k]], 1u);
#pragma unroll
    for (int d = 0; d < 3; d++) {
      atomicMin(&bmin[k][b[k]][d], emin[d]);
      atomicMax(&bmax[k][b[k]][d], emax[d]);
    }
  }
}
// Bins are handed on CLEAN by whoever reads them, never re-initialised: reads a bin's count and, if it is not empty, its
// bounds into pmn / pmx (which hold the empty box on entry), and resets the bin.  The caller's next barrier publishes the reset.
template <typename T>
__device__ __forceinline__ uint32_t take_bin(uint32_t &cnt_ref, typename Ord<T>::U (&bmin_ref)[3], typename Ord<T>::U (&bmax_ref)[3],
                                             typename Ord<T>::U pmn[3], typename Ord<T>::U pmx[3]) {
  const uint32_t cnt = cnt_ref;
  if (cnt) {
#pragma unroll
    for (int d = 0; d < 3; d++) {
      pmn[d] = bmin_ref[d];
      pmx[d] = bmax_ref[d];
    }
    cnt_ref = 0;
    empty_box_e<T>(bmin_ref, bmax_ref);
  }
  return cnt;
}

// Cost of one candidate as in FindCutFromBinBuffer (nanort.h:1393-1422): nL*SA(L) + nR*SA(R) over the two sides' boxes
// (integer images).  A lane that holds no candidate (`ok`: the caller's mask), an empty side or a NaN cost never wins: inf.
template <typename T>
__device__ __forceinline__ T sah_cost(bool ok, uint32_t nl, uint32_t nr, const typename Ord<T>::U lmn[3], const typename Ord<T>::U lmx[3],
                                      const typename Ord<T>::U rmn[3], const typename Ord<T>::U rmx[3]) {
  T a0[3], a1[3], b0[3], b1[3];
#pragma unroll
  for (int d = 0; d < 3; d++) {
    a0[d] = Ord<T>::dec(lmn[d]);
    a1[d] = Ord<T>::dec(lmx[d]);
    b0[d] = Ord<T>::dec(rmn[d]);
    b1[d] = Ord<T>::dec(rmx[d]);
  }
  T cost = Lim<T>::inf();
  if (ok && nl > 0 && nr > 0) cost = T(nl) * half_area<T>(a0, a1) + T(nr) * half_area<T>(b0, b1);
  return cost == cost ? cost : Lim<T>::inf();
}
// Lane == bin inside a 16-lane row: from this lane's bin (cnt, pmn, pmx — scanned in place) the candidate "cut below this
// bin": low side = bins [0, bin) -> nl, lmn, lmx; high side = bins [bin, K) -> sc_n, smn, smx.  DPP row shifts only.
template <typename T>
__device__ __forceinline__ void row_candidate(uint32_t cnt, typename Ord<T>::U pmn[3], typename Ord<T>::U pmx[3], uint32_t &nl,
                                              typename Ord<T>::U lmn[3], typename Ord<T>::U lmx[3], uint32_t &sc_n, typename Ord<T>::U smn[3],
                                              typename Ord<T>::U smx[3]) {
  uint32_t pc = cnt;
  sc_n = cnt;
#pragma unroll
  for (int d = 0; d < 3; d++) {
    smn[d] = pmn[d];
    smx[d] = pmx[d];
  }
  row_prefix_e<T>(pc, pmn, pmx);    // inclusive over the row's lanes up to this one
  row_suffix_e<T>(sc_n, smn, smx);  // inclusive from this lane on
  nl = dpp_mov<0x111>(0u, pc);
#pragma unroll
  for (int d = 0; d < 3; d++) {
    lmn[d] = dpp_mov<0x111>(Ord<T>::highest(), pmn[d]);
    lmx[d] = dpp_mov<0x111>(Ord<T>::lowest(), pmx[d]);
  }
}

// The side a record goes to — the same rule for the cost sweep and every partition: bin(centroid on the split axis) <
// split_bin, or, for an object-median split (nanort.h:1849), its position in the node's range.
template <typename T>
__device__ __forceinline__ bool goes_left(bool median, uint32_t i_minus_lo, uint32_t nleft, T c_axis, T clo, T scl, int K, uint32_t split_bin) {
  return median ? i_minus_lo < nleft : (uint32_t)bin_of<T>(c_axis, clo, scl, K) < split_bin;
}

// No cut separates the centroids, or (subtree phase) `pending` high-side children already wait: a pathological chain of
// lopsided SAH splits could outgrow the pending stack, so past kSubStackSafe the splits are balanced (depth <= log2 n more).
__device__ __forceinline__ bool median_forced(bool found, uint32_t pending) { return !found || pending >= (uint32_t)kSubStackSafe; }
// The object-median split of n primitives; the children's boxes start empty and are reduced during the partition.
template <typename T>
__device__ __forceinline__ void median_fallback(uint32_t n, int &axis, uint32_t &split_bin, uint32_t &nleft, T cl[3], T ch[3], T rl[3], T rh[3]) {
  axis = 0;
  split_bin = kMedian;
  nleft = n >> 1;
#pragma unroll
  for (int d = 0; d < 3; d++) {
    cl[d] = rl[d] = Lim<T>::max();
    ch[d] = rh[d] = -Lim<T>::max();
  }
}

template <typename T>
__device__ __forceinline__ typename Wire<T>::Node leaf_node(const T bmin[3], const T bmax[3], uint32_t n, uint32_t first) {
  typename Wire<T>::Node nd;
#pragma unroll
  for (int d = 0; d < 3; d++) {
    nd.bmin[d] = bmin[d];
    nd.bmax[d] = bmax[d];
  }
  nd.flag = 1;
  nd.axis = 0;
  nd.data[0] = n;
  nd.data[1] = first;
  return nd;
}

// A subtree task's statistics (leaves, deepest node, largest leaf) are left in fields of its own top record that only split
// nodes use, and k_layout — which visits every top record anyway — adds them up: four device-scope atomics per task on four
// neighbouring words (22 000 per 1 M-triangle build, 220 000 at 10 M, through one L2 channel at ~100 per microsecond) were a
// queue every finishing wave stood in.
template <typename T>
__device__ __forceinline__ void task_stats(TopNode<T> &task, uint32_t leaves, uint32_t deepest, uint32_t biggest_leaf) {
  task.nleft = leaves;
  task.split_bin = deepest;
  task.nchunks = biggest_leaf;
}

} // namespace nrt
