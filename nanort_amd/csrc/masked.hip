// nanort_amd/csrc/masked.hip — visibility masks for gfx950: every triangle carries 32 bits, every ray carries 32 bits, and a
// triangle exists for a ray iff (prim_mask & ray_mask) != 0.
//
// The contract is include/nanort_hip.h's (nrtSetPrimMasks* / nrtTraverseBatchMasked* / nrtOccludedBatchMasked*):
//   * the reference's binary loop over the context's node array (nanort.h:2487-2556) — binary_walk (binary_walk_dev.h), the loop
//     k_traverse, the multi-hit walk and the motion walk run, with the query below; lane_init / slab_test / tri_test of
//     traverse_dev.h unchanged.  The boxes know nothing of the masks: the walk reaches every leaf, whatever the ray may see in it;
//   * refill: the lane loads ray_masks[rid] with its ray and keeps the word in one register (null array: every ray 0xFFFFFFFF);
//   * leaf step: the triangle's word is read IN LEAF ORDER, leaf_masks[k] beside a.tris[k] — two independent loads of one address
//     computation, issued together — and its AND with the ray's word is the `active` predicate of tri_test: an invisible record
//     takes part in no reject and no accept, which is the reference's intersector returning false for it.  (Gathered through the
//     record's prim_id the word would be a second round trip behind the record's in every leaf step of a latency-bound chain.)
//     prim_ids_range, skip_prim_id and cull_back_face act on a visible record as they do in k_traverse;
//   * occlusion (a.any_hit), finish: as in the motion walk — settled once hit_t < max_t, store_closest_hit.
// The leaf-order words are derived from the caller's per-face words by k_permute_masks below, whenever either side of that
// permutation changed (api_query.hip, refresh_leaf_masks).  Like the multi-hit and motion walks the launch publishes no completion
// record: its slot is closed by an event (api_query.hip, enqueue_launch).
#include "binary_walk_dev.h"
#include "kernels.h"

namespace nrt {

template <typename T>
struct MaskedArgs {
  TraverseArgs<T> a;          // the closest-hit launch block (a.tris: the leaf records)
  const uint32_t *leaf_masks; // [num_indices] the triangles' words in leaf order, beside a.tris
  const uint32_t *ray_masks;  // [num_rays] one word per ray, or null: every ray 0xFFFFFFFF
};

// The masked query of the binary walk: closest hit, or occlusion when `any`.
template <typename T>
struct MaskedQuery : BinaryQuery {
  const MaskedArgs<T> &m;
  const bool any;             // an occlusion query (a.any_hit; wave-uniform)
  uint32_t ray_mask = ~0u;    // the word of the ray this lane holds

  __device__ __forceinline__ typename Wire<T>::Ray load(const TraverseArgs<T> &a, uint32_t rid) const {
    return load_ray<T>(as_global(a.rays) + rid, 0u); // (as the motion walk: no profiling arm)
  }
  __device__ __forceinline__ void begin(const TraverseArgs<T> &, uint32_t rid) {
    ray_mask = m.ray_masks != nullptr ? as_global(m.ray_masks)[rid] : ~0u;
  }
  __device__ __forceinline__ bool settled(const Lane<T> &L) const { return any && L.hit_t < L.max_t; }
  // the record and its word are fetched together; the word decides whether the record exists for this ray
  __device__ __forceinline__ void record(const TraverseArgs<T> &a, Lane<T> &L, uint32_t, uint32_t k) const {
    const uint32_t word = as_global(m.leaf_masks)[k];
    const LeafTri<T> tri = a.tris[k];
    tri_test<T>(L, tri, (word & ray_mask) != 0u, a.range0, a.range1, a.skip_prim, a.cull_back_face != 0);
  }
  __device__ __forceinline__ void finish(const TraverseArgs<T> &a, const Lane<T> &L, uint32_t rid) const { store_closest_hit<T>(a, L, rid); }
};

template <typename T, int STACK>
__global__ __launch_bounds__(kTraverseBlock) void k_traverse_masked(const MaskedArgs<T> m) {
  // [depth][thread]: a wave's 64 lanes hit 64 consecutive dwords -> conflict-free.
  __shared__ uint32_t s_stack[STACK][kTraverseBlock];
  binary_walk<T, STACK>(m.a, s_stack, MaskedQuery<T>{{}, m, m.a.any_hit != 0});
}

// leaf_masks[k] = masks[tris[k].prim_id]: one thread per leaf record, the grid covers them all.  (tris[k].prim_id < num_faces by
// construction: the builder emits a permutation of the face ids, nrtSetTree checks every index; read with a guard all the same.)
template <typename T>
__global__ __launch_bounds__(256) void k_permute_masks(const LeafTri<T> *__restrict__ tris, const uint32_t *__restrict__ masks, uint32_t num_faces,
                                                       uint32_t *__restrict__ leaf_masks, uint32_t n) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const uint32_t p = tris[k].prim_id;
  leaf_masks[k] = p < num_faces ? masks[p] : 0u;
}

template <typename T>
hipError_t launch_traverse_masked(const TraverseArgs<T> &args, const uint32_t *leaf_masks, const uint32_t *ray_masks, unsigned grid, hipStream_t s) {
  MaskedArgs<T> m;
  m.a = args;
  m.leaf_masks = leaf_masks;
  m.ray_masks = ray_masks;
  launch_persistent((const void *)k_traverse_masked<T, kLdsStackDefault>, grid, m, s);
  return hipGetLastError();
}

template <typename T>
int traverse_masked_blocks_per_cu() {
  return resident_blocks((const void *)k_traverse_masked<T, kLdsStackDefault>, 1);
}

template <typename T>
hipError_t launch_permute_masks(const void *tris, const uint32_t *masks, uint32_t num_faces, uint32_t *leaf_masks, uint32_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_permute_masks<T>), dim3((n + 255u) / 256u), dim3(256), 0, s, (const LeafTri<T> *)tris, masks, num_faces, leaf_masks, n);
  return hipGetLastError();
}

NRT_INSTANTIATE_F32_F64(launch_traverse_masked)
NRT_INSTANTIATE_F32_F64(traverse_masked_blocks_per_cu)
NRT_INSTANTIATE_F32_F64(launch_permute_masks)

} // namespace nrt
