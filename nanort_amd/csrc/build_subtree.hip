// nanort_amd/csrc/build_subtree.hip — the subtree phase of the builder (build.hip): one wave per node of at most kHandoff
// primitives builds the whole subtree out of LDS.  Every decision — bins, cost, tie rules, leaf rule, partition predicate,
// median fallback — is build_dev.h's, the one the top phase takes.  k_subtree_rows is the product kernel; k_subtree, the
// one-node-per-step form, lives in the profiling library only, as the row form's cross-check.  Both sit behind launch_subtree.
#include "build_dev.h"
#include "kernels.h"

namespace nrt {

// ---------------------------------------------------------------------------
// subtree phase: one wave builds everything below a node of <= kSmall prims
// ---------------------------------------------------------------------------
#ifdef NRT_PROF // the one-node-per-step form lives in libnanort_hip_prof.so only: the cross-check of the row form (tests/test_gpu_build.py, tunable subtree_rows = 0)
constexpr int kSubStack = 48; // pending high-side children per subtree wave (LDS)
// Pending high-side child of the per-wave subtree builder.
template <typename T>
struct SubPending {
  T bmin[3], bmax[3]; // its AABB (from the parent's bins, or reduced during the parent's median partition)
  T cmin[3], cmax[3]; // its centroid bounds (reduced during the parent's partition)
  uint16_t lo, hi, parent;
  uint16_t buf;       // which of the two permutation buffers holds [lo, hi)
  uint32_t depth;
};

// One wave per node of <= kSmall primitives: records in LDS, a 16-bit permutation ping-ponged between two
// buffers by the stable partition, LDS bin reduction (3 axes x K <= 16 bins, ds_min/ds_max on integer-ordered
// keys), lane == (axis, bin) prefix/suffix sweeps inside 16-lane groups.  The low-side child is processed next
// (so it is numbered parent + 1, pre-order); the high-side child waits on an LDS stack with its AABB and
// centroid bounds.  A node costs a chain of dependent LDS round trips, not arithmetic, so the chain is kept
// short: each lane keeps its first element (all of a node of <= 64 primitives) in registers across the binning
// and partition passes; a child's centroid bounds (and, after a median split, its AABB) are reduced in the
// parent's partition pass instead of a pass of its own; the bins are reset by the lanes that read them; wave
// reductions and the winner's broadcast go through DPP and scalar registers.  Two barriers per inner node.
template <typename T>
__global__ __launch_bounds__(64) void k_subtree(TopNode<T> *top, const uint32_t *__restrict__ small_list,
                                                const PrimRec<T> *__restrict__ recs0,
                                                const PrimRec<T> *__restrict__ recs1, int K, LeafRule rule,
                                                typename Wire<T>::Node *scratch_nodes, uint32_t *indices, LevelInfo *info) {
  typedef typename Wire<T>::Node Node;
  typedef typename Ord<T>::U U;
  // (the records stay where they are — 10 KB per subtree, contiguous: L1 / L2 hits; a copy in LDS was measured slower, profiles/r02j_build_subtree_ab.txt)
  __shared__ uint16_t s_perm[2][kHandoff];
  __shared__ SubPending<T> s_stack[kSubStack];
  __shared__ uint32_t s_cnt[3][kSmallBins];
  __shared__ U s_bmin[3][kSmallBins][3];
  __shared__ U s_bmax[3][kSmallBins][3];

  const unsigned lane = threadIdx.x;
  if (blockIdx.x >= info->num_small) return; // grid is an upper bound
  TopNode<T> &task = top[small_list[blockIdx.x]];
  const uint32_t L = task.l, n_all = task.r - task.l;
  const PrimRec<T> *src = (task.buf ? recs1 : recs0) + L;
  for (uint32_t i = lane; i < n_all; i += 64u) s_perm[0][i] = (uint16_t)i;
  if (lane < 3 * kSmallBins) { // bins start clean and are handed on clean by their readers
    const int k = (int)lane / kSmallBins, bq = (int)lane % kSmallBins;
    s_cnt[k][bq] = 0;
#pragma unroll
    for (int d = 0; d < 3; d++) {
      s_bmin[k][bq][d] = Ord<T>::highest();
      s_bmax[k][bq][d] = Ord<T>::lowest();
    }
  }
  Node *out = scratch_nodes + 2 * (size_t)L;
  uint32_t node_count = 0, leaves = 0, deepest = 0, biggest_leaf = 0;
  int sp = 0;

  // current node (wave-uniform)
  uint32_t lo = 0, hi = n_all, depth = task.depth, parent = 0xFFFFu, pb = 0;
  bool is_high = false;
  T mn[3], mx[3], cmn[3], cmx[3];
#pragma unroll
  for (int d = 0; d < 3; d++) {
    mn[d] = task.bmin[d];
    mx[d] = task.bmax[d];
    cmn[d] = task.cmin[d];
    cmx[d] = task.cmax[d];
  }
  __syncthreads();

  for (;;) {
    const uint32_t n = hi - lo;
    const uint32_t me = node_count++;
    deepest = depth > deepest ? depth : deepest;
    if (is_high && lane == 0) out[parent].data[1] = me;

    const bool leaf = is_leaf(n, depth, rule);
    // this lane's first element stays in registers for every pass over the node
    const uint32_t i_first = lo + lane;
    const bool have = i_first < hi;
    uint16_t id0 = 0;
    PrimRec<T> r0;
    if (have) {
      id0 = s_perm[pb][i_first];
      r0 = src[id0];
    }

    Node nd = leaf_node<T>(mn, mx, n, L + lo); // (an inner node sets flag, axis and data below)
    bool descend = false;
    if (leaf) {
      if (lane == 0) out[me] = nd;
      if (have) indices[L + i_first] = r0.prim;
      for (uint32_t i = i_first + 64u; i < hi; i += 64u) indices[L + i] = src[s_perm[pb][i]].prim;
      leaves++;
      biggest_leaf = n > biggest_leaf ? n : biggest_leaf;
    } else {
      // ---- LDS bin reduction ------------------------------------------------------------------
      T sc[3];
#pragma unroll
      for (int k = 0; k < 3; k++) sc[k] = bin_scale<T>(cmn[k], cmx[k], K);
      if (have) bin_record_lds<T>(r0, cmn, sc, K, s_cnt, s_bmin, s_bmax);
      for (uint32_t i = i_first + 64u; i < hi; i += 64u) bin_record_lds<T>(src[s_perm[pb][i]], cmn, sc, K, s_cnt, s_bmin, s_bmax);
      __syncthreads();

      // ---- lane == (axis, bin): sweeps inside 16-lane groups, on the integer images ----------------------
      const int ax = (int)lane >> 4, bn = (int)lane & 15;
      uint32_t cnt = 0, nl, sc_n;
      U pmn[3], pmx[3], lmn[3], lmx[3], smn[3], smx[3];
      empty_box_e<T>(pmn, pmx);
      if (ax < 3 && bn < K) cnt = take_bin<T>(s_cnt[ax][bn], s_bmin[ax][bn], s_bmax[ax][bn], pmn, pmx); // (the reset is made visible by the barrier after the partition)
      // candidate (ax, s = bn), s in 1..K-1: low side = bins [0, s), high side = bins [s, K)
      row_candidate<T>(cnt, pmn, pmx, nl, lmn, lmx, sc_n, smn, smx);
      const T cost = sah_cost<T>(ax < 3 && bn >= 1 && bn < K, nl, sc_n, lmn, lmx, smn, smx);
      // argmin: the smallest cost, ties -> lowest lane; lane order == (axis, bin): lowest axis, then lowest bin
      const U ecost = Ord<T>::enc(cost);
      const U ebest = wave_umin<U>(ecost);
      const int who = (int)__builtin_ctzll(__ballot(ecost == ebest));
      const bool found = ebest < Ord<T>::enc(Lim<T>::inf());
      int axis;
      uint32_t split_bin, nleft;
      T cl[3], ch[3], rl[3], rh[3]; // children AABBs
      if (median_forced(found, (uint32_t)sp)) {
        median_fallback<T>(n, axis, split_bin, nleft, cl, ch, rl, rh);
      } else {
        axis = who >> 4;
        split_bin = (uint32_t)who & 15u;
        nleft = lane_bcast(nl, who);
#pragma unroll
        for (int d = 0; d < 3; d++) {
          cl[d] = Ord<T>::dec(lane_bcast(lmn[d], who));
          ch[d] = Ord<T>::dec(lane_bcast(lmx[d], who));
          rl[d] = Ord<T>::dec(lane_bcast(smn[d], who));
          rh[d] = Ord<T>::dec(lane_bcast(smx[d], who));
        }
      }
      const bool median = split_bin == kMedian;

      // ---- stable partition of s_perm[pb][lo, hi) into s_perm[1 - pb], reducing the children's centroid bounds
      //      (and, after a median split, their AABBs) on the way ----------------------------------------------
      const bool low_leaf = is_leaf(nleft, depth + 1, rule), high_leaf = is_leaf(n - nleft, depth + 1, rule);
      const bool both_leaves = low_leaf && high_leaf; // the common case at the bottom: finished here, no trip through the stack
      T ccl[3], cch[3], crl[3], crh[3];
#pragma unroll
      for (int d = 0; d < 3; d++) {
        ccl[d] = crl[d] = Lim<T>::max();
        cch[d] = crh[d] = -Lim<T>::max();
      }
      {
        const T clo = pick_axis<T>(cmn, axis), scl = pick_axis<T>(sc, axis);
        uint32_t run_l = 0, run_r = 0;
        for (uint32_t i0 = lo; i0 < hi; i0 += 64u) {
          const uint32_t i = i0 + lane;
          const bool valid = i < hi;
          uint16_t id = id0;
          PrimRec<T> r = r0;
          if (valid && i0 != lo) {
            id = s_perm[pb][i];
            r = src[id];
          }
          const bool left = valid && goes_left<T>(median, i - lo, nleft, pick_axis<T>(r.c, axis), clo, scl, K, split_bin);
          const unsigned long long bl = __ballot(valid && left), br = __ballot(valid && !left);
          const unsigned long long lt = (1ull << lane) - 1ull;
          if (valid) {
            const uint32_t d = left ? lo + run_l + (uint32_t)__builtin_popcountll(bl & lt)
                                    : lo + nleft + run_r + (uint32_t)__builtin_popcountll(br & lt);
            s_perm[1 - pb][d] = id;
            if (both_leaves || (low_leaf && left)) indices[L + d] = r.prim; // index slots of the leaves emitted below, in partition order
#pragma unroll
            for (int k = 0; k < 3; k++) {
              if (left) {
                ccl[k] = tmin(ccl[k], r.c[k]);
                cch[k] = tmax(cch[k], r.c[k]);
              } else {
                crl[k] = tmin(crl[k], r.c[k]);
                crh[k] = tmax(crh[k], r.c[k]);
              }
              if (median) {
                if (left) {
                  cl[k] = tmin(cl[k], r.bmin[k]);
                  ch[k] = tmax(ch[k], r.bmax[k]);
                } else {
                  rl[k] = tmin(rl[k], r.bmin[k]);
                  rh[k] = tmax(rh[k], r.bmax[k]);
                }
              }
            }
          }
          run_l += (uint32_t)__builtin_popcountll(bl);
          run_r += (uint32_t)__builtin_popcountll(br);
        }
      }
      // (a child that becomes a leaf needs no centroid bounds)
#pragma unroll
      for (int d = 0; d < 3; d++) {
        if (!low_leaf) {
          ccl[d] = wave_min_u<T>(ccl[d]);
          cch[d] = wave_max_u<T>(cch[d]);
        }
        if (!high_leaf) {
          crl[d] = wave_min_u<T>(crl[d]);
          crh[d] = wave_max_u<T>(crh[d]);
        }
        if (median) {
          cl[d] = wave_min_u<T>(cl[d]);
          ch[d] = wave_max_u<T>(ch[d]);
          rl[d] = wave_min_u<T>(rl[d]);
          rh[d] = wave_max_u<T>(rh[d]);
        }
      }

      nd.flag = 0;
      nd.axis = axis;
      nd.data[0] = me + 1; // low-side child follows its parent (pre-order)
      nd.data[1] = 0;      // patched when the high-side child is emitted
      if (both_leaves) {
        // both children are leaves: emit the three nodes now (pre-order: parent, low leaf, high leaf)
        nd.data[1] = me + 2;
        if (lane == 0) {
          out[me] = nd;
          out[me + 1] = leaf_node<T>(cl, ch, nleft, L + lo);
          out[me + 2] = leaf_node<T>(rl, rh, n - nleft, L + lo + nleft);
        }
        node_count += 2;
        leaves += 2;
        deepest = depth + 1 > deepest ? depth + 1 : deepest;
        const uint32_t big = nleft > n - nleft ? nleft : n - nleft;
        biggest_leaf = big > biggest_leaf ? big : biggest_leaf;
        __syncthreads(); // the reset bins are visible to the next node
      } else if (low_leaf) {
        // the low child is a leaf, the high one is not: emit the leaf (node me + 1) and continue with the high child
        // right away (it is node me + 2; the loop head patches the parent's data[1]) — no stack entry
        if (lane == 0) {
          out[me] = nd;
          out[me + 1] = leaf_node<T>(cl, ch, nleft, L + lo);
        }
        node_count += 1;
        leaves += 1;
        deepest = depth + 1 > deepest ? depth + 1 : deepest;
        biggest_leaf = nleft > biggest_leaf ? nleft : biggest_leaf;
        lo = lo + nleft;
        depth = depth + 1;
        parent = me;
        is_high = true;
        pb = 1u - pb;
#pragma unroll
        for (int d = 0; d < 3; d++) {
          mn[d] = rl[d];
          mx[d] = rh[d];
          cmn[d] = crl[d];
          cmx[d] = crh[d];
        }
        descend = true;
        __syncthreads(); // the permutation and the reset bins are visible to the next node
      } else {
      if (lane == 0) {
        out[me] = nd;
        SubPending<T> &e = s_stack[sp];
#pragma unroll
        for (int d = 0; d < 3; d++) {
          e.bmin[d] = rl[d];
          e.bmax[d] = rh[d];
          e.cmin[d] = crl[d];
          e.cmax[d] = crh[d];
        }
        e.lo = (uint16_t)(lo + nleft);
        e.hi = (uint16_t)hi;
        e.parent = (uint16_t)me;
        e.buf = (uint16_t)(1u - pb);
        e.depth = depth + 1;
      }
      sp++;
      // continue with the low side
      hi = lo + nleft;
      depth = depth + 1;
      parent = me;
      is_high = false;
      pb = 1u - pb;
#pragma unroll
      for (int d = 0; d < 3; d++) {
        mn[d] = cl[d];
        mx[d] = ch[d];
        cmn[d] = ccl[d];
        cmx[d] = cch[d];
      }
      descend = true;
      __syncthreads(); // the permutation, the reset bins and the stack entry are visible to the next node
      }
    }
    if (!descend) {
      if (sp == 0) break;
      sp--;
      const SubPending<T> &e = s_stack[sp];
      lo = e.lo;
      hi = e.hi;
      depth = e.depth;
      parent = e.parent;
      pb = e.buf;
      is_high = true;
#pragma unroll
      for (int d = 0; d < 3; d++) {
        mn[d] = e.bmin[d];
        mx[d] = e.bmax[d];
        cmn[d] = e.cmin[d];
        cmx[d] = e.cmax[d];
      }
    }
  }
  if (lane == 0) { // (statistics: left in the task's record, summed by k_layout — see task_stats)
    task.size = node_count;
    task_stats<T>(task, leaves, deepest, biggest_leaf);
  }
}
#endif // NRT_PROF

// ---------------------------------------------------------------------------
// subtree phase, row form: up to four nodes of a subtree per step, one per 16-lane row
// ---------------------------------------------------------------------------
// k_subtree above spends about 700 wave instructions on an inner node whatever its size, and three quarters of a
// subtree's inner nodes hold 16 primitives or fewer (5 to 16 of 64 lanes busy).  This form keeps the nodes that wait to be
// split on an LDS stack and takes up to FOUR of them per step, one per 16-lane DPP row: lane == primitive for the binning
// and the partition (16 at a time), lane == bin for the cut search (the three axes one after the other, the 16-lane
// prefix / suffix scans are the ones k_subtree uses), the winner's data is handed to its row by ds_bpermute.  With one or
// two nodes on the stack (the first steps of a subtree, where the nodes are large) a node gets 64 or 32 lanes instead.
// Every decision is the one k_subtree takes — same bins, cost expression, tie rule (lowest axis, then lowest bin), leaf
// rule and object-median fallback (including k_subtree's stack-depth guard, whose depth every node carries along) — and
// min / max / counts do not depend on the order they are combined in, so the tree is the same.  Nodes are created in
// step order, not in pre-order: they are written to the scratch array under their creation index (children c, c + 1
// with c odd) and the wave finishes by computing each node's pre-order index from the parent links (subtree sizes by
// walking up, then the index as the sum over the path to the root), which k_emit_small applies when it splices the
// subtree into the tree (premap).
struct RowEntry {
  uint16_t lo, hi; // range in the permutation
  uint16_t me;     // creation index of the node
  uint8_t ldepth;  // depth below the subtree's root
  uint8_t misc;    // bit 7: permutation buffer holding [lo, hi); bits 0..5: k_subtree's stack depth at this node
};
static_assert(sizeof(RowEntry) == 8, "RowEntry");
constexpr int kRowStack = kHandoff / 2; // pending nodes are disjoint ranges of at least 2 primitives

template <typename T>
__global__ __launch_bounds__(64) void k_subtree_rows(TopNode<T> *top, const uint32_t *__restrict__ small_list,
                                                     const PrimRec<T> *__restrict__ recs0,
                                                     const PrimRec<T> *__restrict__ recs1, int K, LeafRule rule,
                                                     typename Wire<T>::Node *scratch_nodes, uint16_t *premap, uint32_t *indices,
                                                     LevelInfo *info) {
  typedef typename Wire<T>::Node Node;
  typedef typename Ord<T>::U U;
  __shared__ uint16_t s_perm[2][kHandoff];
  __shared__ RowEntry s_stack[kRowStack];
  __shared__ uint16_t s_parent[2 * kHandoff];
  __shared__ uint32_t s_cnt[4][3][kSmallBins];
  __shared__ U s_bmin[4][3][kSmallBins][3]; // (after the last step: the nodes' subtree sizes, 2 * kHandoff uint32)
  __shared__ U s_bmax[4][3][kSmallBins][3];
  static_assert(sizeof(U) * 4 * 3 * kSmallBins * 3 >= sizeof(uint32_t) * 2 * kHandoff, "sizes fit the bins");

  const unsigned lane = threadIdx.x;
  if (blockIdx.x >= info->num_small) return; // grid is an upper bound
  TopNode<T> &task = top[small_list[blockIdx.x]];
  const uint32_t L = task.l, n_all = task.r - task.l;
  const PrimRec<T> *src = (task.buf ? recs1 : recs0) + L;
  Node *out = scratch_nodes + 2 * (size_t)L;
  uint16_t *map = premap + 2 * (size_t)L;
  const uint32_t depth0 = task.depth;

  if (is_leaf(n_all, depth0, rule)) { // the task is a leaf
    for (uint32_t i = lane; i < n_all; i += 64u) indices[L + i] = src[i].prim;
    if (lane == 0) {
      out[0] = leaf_node<T>(task.bmin, task.bmax, n_all, L);
      map[0] = 0;
      task.size = 1;
      task_stats<T>(task, 1u, depth0, n_all);
    }
    return;
  }

  for (uint32_t i = lane; i < n_all; i += 64u) s_perm[0][i] = (uint16_t)i;
  for (uint32_t q = lane; q < 4u * 3u * kSmallBins; q += 64u) { // bins start clean and are handed on clean by their readers
    (&s_cnt[0][0][0])[q] = 0;
#pragma unroll
    for (int d = 0; d < 3; d++) {
      (&s_bmin[0][0][0][0])[3 * q + d] = Ord<T>::highest();
      (&s_bmax[0][0][0][0])[3 * q + d] = Ord<T>::lowest();
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int d = 0; d < 3; d++) {
      out[0].bmin[d] = task.bmin[d];
      out[0].bmax[d] = task.bmax[d];
    }
    RowEntry e;
    e.lo = 0;
    e.hi = (uint16_t)n_all;
    e.me = 0;
    e.ldepth = 0;
    e.misc = 0;
    s_stack[0] = e;
    s_parent[0] = 0;
  }
  uint32_t stack_n = 1, node_count = 1;                // wave-uniform
  uint32_t leaves = 0, deepest = 0, biggest_leaf = 0;  // kept by the group leaders, combined at the end
  __syncthreads();

  for (uint32_t step = 0; stack_n > 0; step++) {
    if (step > 4u * kHandoff) { // cannot happen (every step splits at least one node, a subtree has fewer than kHandoff inner nodes)
      if (lane == 0) info->error = 1;
      break;
    }
    const uint32_t m = stack_n < 4u ? stack_n : 4u;
    const uint32_t shift = m == 1u ? 6u : (m == 2u ? 5u : 4u); // lanes per node: 64, 32 or 16
    const uint32_t G = 1u << shift, g = lane >> shift, lg = lane & (G - 1u), gbase = g << shift;
    const bool act = g < m;
    RowEntry e = s_stack[act ? stack_n - 1u - g : 0u];
    stack_n -= m;
    const uint32_t lo = act ? e.lo : 0u, hi = act ? e.hi : 0u, n = hi - lo, me = e.me;
    const uint32_t ldepth = e.ldepth, depth = depth0 + ldepth, pb = e.misc >> 7, vsp = e.misc & 63u;
    // passes over the node: G primitives at a time; the wave runs the longest group's count
    const uint32_t my_pass = (n + G - 1u) >> shift;
    uint32_t npass = (uint32_t)__builtin_amdgcn_readlane((int)my_pass, 0);
    {
      const uint32_t p1 = (uint32_t)__builtin_amdgcn_readlane((int)my_pass, 16), p2 = (uint32_t)__builtin_amdgcn_readlane((int)my_pass, 32),
                     p3 = (uint32_t)__builtin_amdgcn_readlane((int)my_pass, 48);
      npass = npass > p1 ? npass : p1;
      npass = npass > p2 ? npass : p2;
      npass = npass > p3 ? npass : p3;
      npass = npass < (uint32_t)(kHandoff >> 4) ? npass : (uint32_t)(kHandoff >> 4); // (a range never exceeds the subtree)
    }

    // ---- this lane's first element stays in registers for every pass; the node's centroid bounds --------------------
    const uint32_t i0 = lo + lg;
    const bool have0 = i0 < hi;
    uint32_t id0 = 0;
    PrimRec<T> r0;
    if (have0) {
      id0 = s_perm[pb][i0];
      r0 = src[id0];
    }
    T cmn[3], cmx[3];
    if (step == 0) { // the subtree's root: reduced by the top phase
#pragma unroll
      for (int k = 0; k < 3; k++) {
        cmn[k] = task.cmin[k];
        cmx[k] = task.cmax[k];
      }
    } else {
      U emn[3], emx[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        emn[k] = have0 ? Ord<T>::enc(r0.c[k]) : Ord<T>::highest();
        emx[k] = have0 ? Ord<T>::enc(r0.c[k]) : Ord<T>::lowest();
      }
      for (uint32_t pass = 1; pass < npass; pass++) {
        const uint32_t i = i0 + (pass << shift);
        if (i < hi) {
          const PrimRec<T> &r = src[s_perm[pb][i]];
#pragma unroll
          for (int k = 0; k < 3; k++) {
            const U ec = Ord<T>::enc(r.c[k]);
            emn[k] = umin_(emn[k], ec);
            emx[k] = umax_(emx[k], ec);
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 3; k++) {
        cmn[k] = Ord<T>::dec(group_allmin<U>(emn[k], shift));
        cmx[k] = Ord<T>::dec(group_allmax<U>(emx[k], shift));
      }
    }

    // ---- LDS bin reduction into the group's bins ---------------------------------------------------------------------
    T sc[3];
#pragma unroll
    for (int k = 0; k < 3; k++) sc[k] = bin_scale<T>(cmn[k], cmx[k], K);
    for (uint32_t pass = 0; pass < npass; pass++) {
      const uint32_t i = i0 + (pass << shift);
      if (i < hi) {
        PrimRec<T> r = r0;
        if (pass) r = src[s_perm[pb][i]];
        bin_record_lds<T>(r, cmn, sc, K, s_cnt[g], s_bmin[g], s_bmax[g]);
      }
    }
    __syncthreads();

    // ---- cut search: the first 16 lanes of the group, lane == bin, one axis after the other ---------------------------
    T best_cost = Lim<T>::inf();
    int axis = 0;
    uint32_t split_bin = 0, nleft = 0; // (set by the first axis that has a candidate; none: median_fallback below)
    T cl[3], ch[3], rl[3], rh[3]; // children AABBs
    U ecl[3], ech[3], erl[3], erh[3]; // (their integer images while the axes compete)
#pragma unroll
    for (int d = 0; d < 3; d++) {
      ecl[d] = erl[d] = Ord<T>::enc(Lim<T>::max());
      ech[d] = erh[d] = Ord<T>::enc(-Lim<T>::max());
    }
    const bool bin_lane = act && lg < (uint32_t)K && lg < 16u;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      uint32_t cnt = 0, nl, sc_n;
      U pmn[3], pmx[3], lmn[3], lmx[3], smn[3], smx[3];
      empty_box_e<T>(pmn, pmx);
      if (bin_lane) cnt = take_bin<T>(s_cnt[g][k][lg], s_bmin[g][k][lg], s_bmax[g][k][lg], pmn, pmx); // (the reset is made visible by the barrier that ends the step)
      // candidate s = bin, s in 1..K-1: low side = bins [0, s), high side = bins [s, K)
      row_candidate<T>(cnt, pmn, pmx, nl, lmn, lmx, sc_n, smn, smx);
      const T cost = sah_cost<T>(bin_lane && lg >= 1u, nl, sc_n, lmn, lmx, smn, smx);
      const U ecost = Ord<T>::enc(cost);
      const U rbest = row_allmin<U>(ecost);
      const unsigned long long hit = __ballot(ecost == rbest);
      // the group's first row holds its candidates: the row's best, ties -> lowest bin
      const U gbest = (U)__shfl(rbest, (int)gbase);
      const T c = Ord<T>::dec(gbest);
      const bool better = c < best_cost; // ties -> lowest axis
      if (__ballot(better) != 0ull) {    // (uniform: the winner's data travels only when some group wants it)
        const uint32_t who = (uint32_t)__builtin_ctz(((uint32_t)(hit >> gbase) & 0xFFFFu) | 0x10000u);
        const int from = (int)(gbase + (who & 15u));
        const uint32_t w_nl = (uint32_t)__shfl(nl, from);
        U w_lmn[3], w_lmx[3], w_smn[3], w_smx[3];
#pragma unroll
        for (int d = 0; d < 3; d++) {
          w_lmn[d] = (U)__shfl(lmn[d], from);
          w_lmx[d] = (U)__shfl(lmx[d], from);
          w_smn[d] = (U)__shfl(smn[d], from);
          w_smx[d] = (U)__shfl(smx[d], from);
        }
        if (better) {
          best_cost = c;
          axis = k;
          split_bin = who;
          nleft = w_nl;
#pragma unroll
          for (int d = 0; d < 3; d++) {
            ecl[d] = w_lmn[d];
            ech[d] = w_lmx[d];
            erl[d] = w_smn[d];
            erh[d] = w_smx[d];
          }
        }
      }
    }
#pragma unroll
    for (int d = 0; d < 3; d++) {
      cl[d] = Ord<T>::dec(ecl[d]);
      ch[d] = Ord<T>::dec(ech[d]);
      rl[d] = Ord<T>::dec(erl[d]);
      rh[d] = Ord<T>::dec(erh[d]);
    }
    // (vsp: the pending high-side children k_subtree would have at this node — the same cut-off of lopsided chains)
    if (median_forced(best_cost < Lim<T>::inf(), vsp)) median_fallback<T>(n, axis, split_bin, nleft, cl, ch, rl, rh);
    const bool median = split_bin == kMedian;
    const bool low_leaf = is_leaf(nleft, depth + 1u, rule), high_leaf = is_leaf(n - nleft, depth + 1u, rule);

    // ---- stable partition of s_perm[pb][lo, hi) into s_perm[1 - pb] ---------------------------------------------------
    {
      const T clo = pick_axis<T>(cmn, axis), scl = pick_axis<T>(sc, axis);
      const unsigned long long gmask = (G == 64u ? ~0ull : ((1ull << G) - 1ull)), lt = (1ull << lg) - 1ull;
      const bool any_median = __ballot(act && median) != 0ull;
      uint32_t run_l = 0, run_r = 0;
      for (uint32_t pass = 0; pass < npass; pass++) {
        const uint32_t i = i0 + (pass << shift);
        const bool valid = i < hi;
        uint32_t id = id0;
        PrimRec<T> r = r0;
        if (valid && pass) {
          id = s_perm[pb][i];
          r = src[id];
        }
        const bool left = valid && goes_left<T>(median, i - lo, nleft, pick_axis<T>(r.c, axis), clo, scl, K, split_bin);
        const unsigned long long bl = (__ballot(valid && left) >> gbase) & gmask, br = (__ballot(valid && !left) >> gbase) & gmask;
        if (valid) {
          const uint32_t d = left ? lo + run_l + (uint32_t)__builtin_popcountll(bl & lt)
                                  : lo + nleft + run_r + (uint32_t)__builtin_popcountll(br & lt);
          s_perm[1u - pb][d] = (uint16_t)id;
          if (left ? low_leaf : high_leaf) indices[L + d] = r.prim; // index slots of the leaves emitted below, in partition order
          if (median) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
              if (left) {
                cl[k] = tmin(cl[k], r.bmin[k]);
                ch[k] = tmax(ch[k], r.bmax[k]);
              } else {
                rl[k] = tmin(rl[k], r.bmin[k]);
                rh[k] = tmax(rh[k], r.bmax[k]);
              }
            }
          }
        }
        run_l += (uint32_t)__builtin_popcountll(bl);
        run_r += (uint32_t)__builtin_popcountll(br);
      }
      if (any_median) { // (uniform: the reductions run for every group, only the median ones keep the result)
#pragma unroll
        for (int d = 0; d < 3; d++) {
          const T a = Ord<T>::dec(group_allmin<U>(Ord<T>::enc(cl[d]), shift)), b = Ord<T>::dec(group_allmax<U>(Ord<T>::enc(ch[d]), shift));
          const T c = Ord<T>::dec(group_allmin<U>(Ord<T>::enc(rl[d]), shift)), e2 = Ord<T>::dec(group_allmax<U>(Ord<T>::enc(rh[d]), shift));
          if (median) {
            cl[d] = a;
            ch[d] = b;
            rl[d] = c;
            rh[d] = e2;
          }
        }
      }
    }

    // ---- the group's first lane writes the node and its children -----------------------------------------------------
    {
      const bool lead = act && lg == 0u;
      const unsigned long long push_l = __ballot(lead && !low_leaf), push_h = __ballot(lead && !high_leaf);
      const unsigned long long below = (1ull << lane) - 1ull;
      if (lead) {
        const uint32_t c0 = node_count + 2u * g;
        out[me].flag = 0;
        out[me].axis = axis;
        out[me].data[0] = c0;
        out[me].data[1] = c0 + 1u;
        s_parent[c0] = (uint16_t)me;
        s_parent[c0 + 1u] = (uint16_t)me;
        uint32_t slot = stack_n + (uint32_t)__builtin_popcountll(push_l & below) + (uint32_t)__builtin_popcountll(push_h & below);
        if (low_leaf) {
          out[c0] = leaf_node<T>(cl, ch, nleft, L + lo);
        } else {
#pragma unroll
          for (int d = 0; d < 3; d++) {
            out[c0].bmin[d] = cl[d];
            out[c0].bmax[d] = ch[d];
          }
          RowEntry ne;
          ne.lo = (uint16_t)lo;
          ne.hi = (uint16_t)(lo + nleft);
          ne.me = (uint16_t)c0;
          ne.ldepth = (uint8_t)(ldepth + 1u);
          ne.misc = (uint8_t)(((1u - pb) << 7) | (vsp + 1u)); // k_subtree descends into the low side with the high side pending
          s_stack[slot++] = ne;
        }
        if (high_leaf) {
          out[c0 + 1u] = leaf_node<T>(rl, rh, n - nleft, L + lo + nleft);
        } else {
#pragma unroll
          for (int d = 0; d < 3; d++) {
            out[c0 + 1u].bmin[d] = rl[d];
            out[c0 + 1u].bmax[d] = rh[d];
          }
          RowEntry ne;
          ne.lo = (uint16_t)(lo + nleft);
          ne.hi = (uint16_t)hi;
          ne.me = (uint16_t)(c0 + 1u);
          ne.ldepth = (uint8_t)(ldepth + 1u);
          ne.misc = (uint8_t)(((1u - pb) << 7) | vsp);
          s_stack[slot] = ne;
        }
        if (low_leaf || high_leaf) {
          leaves += (low_leaf ? 1u : 0u) + (high_leaf ? 1u : 0u);
          deepest = depth + 1u > deepest ? depth + 1u : deepest;
          const uint32_t big = (low_leaf ? nleft : 0u) > (high_leaf ? n - nleft : 0u) ? (low_leaf ? nleft : 0u) : (high_leaf ? n - nleft : 0u);
          biggest_leaf = big > biggest_leaf ? big : biggest_leaf;
        }
      }
      stack_n += (uint32_t)__builtin_popcountll(push_l) + (uint32_t)__builtin_popcountll(push_h);
      node_count += 2u * m;
    }
    __syncthreads(); // the permutation, the reset bins, the stack and the parent links are visible to the next step
  }

  // ---- pre-order index of every node from the parent links ------------------------------------------------------------
  uint32_t *s_size = reinterpret_cast<uint32_t *>(&s_bmin[0][0][0][0]);
  const uint32_t N = node_count;
  for (uint32_t x = lane; x < N; x += 64u) s_size[x] = 1u;
  __syncthreads();
  for (uint32_t x = lane; x < N; x += 64u) {
    if (x == 0u) continue;
    uint32_t p = s_parent[x];
    for (uint32_t it = 0; it < 2u * kHandoff; it++) { // every ancestor counts this node
      atomicAdd(&s_size[p], 1u);
      if (p == 0u) break;
      p = s_parent[p];
    }
  }
  __syncthreads();
  for (uint32_t x = lane; x < N; x += 64u) {
    // pre-order: a low-side child (odd creation index) follows its parent, a high-side child follows the low side's subtree
    uint32_t acc = 0, y = x;
    for (uint32_t it = 0; it < 2u * kHandoff && y != 0u; it++) {
      acc += 1u + ((y & 1u) ? 0u : s_size[y - 1u]);
      y = s_parent[y];
    }
    map[x] = (uint16_t)acc;
  }
  // stats: the leaders' partial values
  for (int off = 32; off > 0; off >>= 1) {
    leaves += __shfl_xor(leaves, off);
    const uint32_t dd = __shfl_xor(deepest, off), bb = __shfl_xor(biggest_leaf, off);
    deepest = dd > deepest ? dd : deepest;
    biggest_leaf = bb > biggest_leaf ? bb : biggest_leaf;
  }
  if (lane == 0) {
    task.size = N;
    task_stats<T>(task, leaves, deepest, biggest_leaf);
  }
}

// (kernels.h)
template <typename T>
const uint16_t *launch_subtree(TopNode<T> *top, const uint32_t *small_list, const PrimRec<T> *recs0, const PrimRec<T> *recs1, int Ks,
                               LeafRule rule, typename Wire<T>::Node *scratch, uint16_t *premap, uint32_t *indices, LevelInfo *info,
                               uint32_t num_small, bool dfs_form, hipStream_t s) {
#ifdef NRT_PROF
  if (dfs_form) { // (tunable subtree_rows = 0 of the profiling build)
    hipLaunchKernelGGL((k_subtree<T>), dim3(num_small), dim3(64), 0, s, top, small_list, recs0, recs1, Ks, rule, scratch, indices, info);
    return nullptr;
  }
#endif
  (void)dfs_form; // (k_subtree is not in the product library)
  hipLaunchKernelGGL((k_subtree_rows<T>), dim3(num_small), dim3(64), 0, s, top, small_list, recs0, recs1, Ks, rule, scratch, premap, indices,
                     info);
  return premap;
}
NRT_INSTANTIATE_F32_F64(launch_subtree)

} // namespace nrt
