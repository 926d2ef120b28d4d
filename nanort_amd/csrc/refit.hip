// nanort_amd/csrc/refit.hip — BVH refit on gfx950: the boxes of a resident tree recomputed bottom-up from moved vertices
// or moved spheres / curves (nrtRefit* / nrtRefitDevice* / nrtRefitPrims*, include/nanort_hip.h).  Topology, leaf slots and the
// index array stay as they are.
//
//   PLAN (first refit after the tree changes; cached in the context, dropped by free_tree)
//     k_plan_root      level 0: the root in the branch or the leaf list
//     k_plan_expand    one launch per level d <= tree_depth: the level's branches append their branch children to level
//                      d + 1 and their leaf children to the leaf list (slots by atomic counters: the lists' order varies
//                      from plan to plan, no box depends on it)
//   REFIT (every call)
//     (prims.hip)      launch_gather_vertices: the caller's strided vertices -> the context's tight xyz
//     k_refit_leaves   every reachable leaf: min / max over each coordinate of its triangles, in slot order.  Spheres and
//                      curves (nrtRefitPrims*, launch_refit_prims): the same fold over the builder's box of each primitive
//                      (prims_dev.h), from the context's positions and radii, which api_tree.hip has already replaced
//     k_refit_branches one launch per level, deepest first: union of the two children's boxes, low child first
//   then the existing launch_gather_leaf / launch_make_wide (api_tree.hip) re-derive LeafTri and WideNode / Wide4Node.
//
// Every level's boxes reach the next level through a launch boundary: no workgroup hands data to another inside a launch.
// Records the walk from the root never reaches (adopted trees) are in neither list and are left untouched.
#include <algorithm>

#include "kernels.h"
#include "minmax_dev.h"
#include "prims_dev.h"

namespace nrt {

constexpr unsigned kRefitBlock = 256;
constexpr unsigned kRefitMaxGrid = 1024; // grid-stride kernels: the list lengths live on the device

// Plan header, in uint32 words: cnt[levels], off[levels], leaf count; then the branch list (level-major), then the leaf list.
static inline size_t plan_header_words(uint32_t levels) { return 2 * (size_t)levels + 2; }

__global__ void __launch_bounds__(1) k_plan_root(uint32_t *plan, uint32_t levels, uint32_t root_is_branch, uint32_t *branch_list,
                                                 uint32_t *leaf_list) {
  uint32_t *cnt = plan, *leaf_cnt = plan + 2 * (size_t)levels;
  if (root_is_branch) {
    branch_list[0] = 0u;
    cnt[0] = 1u;
  } else {
    leaf_list[0] = 0u;
    *leaf_cnt = 1u;
  }
}

template <typename T>
__global__ void __launch_bounds__(kRefitBlock) k_plan_expand(const typename Wire<T>::Node *__restrict__ nodes, uint32_t *plan, uint32_t levels,
                                                             uint32_t d, uint32_t *branch_list, uint32_t branch_cap, uint32_t *leaf_list,
                                                             uint32_t leaf_cap) {
  uint32_t *cnt = plan, *off = plan + levels, *leaf_cnt = plan + 2 * (size_t)levels;
  const uint32_t begin = off[d], n = cnt[d], next = begin + n; // (level d is complete: the previous launch filled it)
  if (blockIdx.x == 0 && threadIdx.x == 0) off[d + 1] = next;
  for (uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x; i < n; i += gridDim.x * kRefitBlock) {
    const uint32_t b = branch_list[begin + i];
    for (int ch = 0; ch < 2; ch++) {
      const uint32_t k = nodes[b].data[ch];
      if (nodes[k].flag == 0) {
        const uint32_t pos = next + atomicAdd(&cnt[d + 1], 1u);
        if (pos < branch_cap) branch_list[pos] = k;
      } else {
        const uint32_t pos = atomicAdd(leaf_cnt, 1u);
        if (pos < leaf_cap) leaf_list[pos] = k;
      }
    }
  }
}

template <typename T>
__device__ __forceinline__ void store_box(typename Wire<T>::Node *n, const T lo[3], const T hi[3]) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    n->bmin[k] = lo[k];
    n->bmax[k] = hi[k];
  }
}

// The box of the primitive behind a leaf slot, one functor per family of kinds; the fold over a leaf's slots (k_refit_leaves) is
// written once.  Triangles: tmin(p0, tmin(p1, p2)) as the builder's primitive records (build.hip k_prim_records).
template <typename T>
struct TriangleBox {
  const uint32_t *__restrict__ faces;
  const T *__restrict__ verts;
  __device__ __forceinline__ void operator()(uint32_t prim, T lo[3], T hi[3]) const {
    const uint32_t *f = faces + 3 * (size_t)prim;
    const T *v0 = verts + 3 * (size_t)f[0], *v1 = verts + 3 * (size_t)f[1], *v2 = verts + 3 * (size_t)f[2];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      lo[k] = tmin(v0[k], tmin(v1[k], v2[k]));
      hi[k] = tmax(v0[k], tmax(v1[k], v2[k]));
    }
  }
};
// Spheres and curves: the builder's own rule (prims_dev.h, prim_box_axis), so a kind's box stays stated once.
template <typename T, int Kind>
struct RadiusPrimBox {
  const T *__restrict__ verts;
  const T *__restrict__ radii;
  __device__ __forceinline__ void operator()(uint32_t prim, T lo[3], T hi[3]) const {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      T centre; // (the builder's split key: not needed here)
      prim_box_axis<T>(false, Kind, prim, k, verts, radii, T(0), T(0), T(0), lo[k], hi[k], centre);
    }
  }
};

// A leaf's box: the boxes of its primitives folded over the leaf's slots in order.  An empty leaf keeps {+max, -max}, which a
// parent's union ignores.
template <typename T, typename PrimBox>
__global__ void __launch_bounds__(kRefitBlock) k_refit_leaves(typename Wire<T>::Node *__restrict__ nodes, const uint32_t *__restrict__ indices,
                                                              const PrimBox prim_box, const uint32_t *__restrict__ plan, uint32_t levels,
                                                              const uint32_t *__restrict__ leaf_list, uint32_t leaf_cap) {
  const uint32_t n = min(plan[2 * (size_t)levels], leaf_cap);
  for (uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x; i < n; i += gridDim.x * kRefitBlock) {
    typename Wire<T>::Node *node = nodes + leaf_list[i];
    const uint32_t count = node->data[0], first = node->data[1];
    T lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      lo[k] = Lim<T>::max();
      hi[k] = -Lim<T>::max();
    }
    for (uint32_t j = 0; j < count; j++) {
      T plo[3], phi[3];
      prim_box(indices[first + j], plo, phi);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        lo[k] = tmin(lo[k], plo[k]);
        hi[k] = tmax(hi[k], phi[k]);
      }
    }
    store_box<T>(node, lo, hi);
  }
}

template <typename T>
__global__ void __launch_bounds__(kRefitBlock) k_refit_branches(typename Wire<T>::Node *__restrict__ nodes, const uint32_t *__restrict__ plan,
                                                                uint32_t levels, uint32_t d, const uint32_t *__restrict__ branch_list,
                                                                uint32_t branch_cap) {
  const uint32_t begin = plan[levels + d];
  const uint32_t n = begin < branch_cap ? min(plan[d], branch_cap - begin) : 0u;
  for (uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x; i < n; i += gridDim.x * kRefitBlock) {
    typename Wire<T>::Node *node = nodes + branch_list[begin + i];
    const typename Wire<T>::Node *a = nodes + node->data[0], *b = nodes + node->data[1];
    T lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      lo[k] = tmin(a->bmin[k], b->bmin[k]);
      hi[k] = tmax(a->bmax[k], b->bmax[k]);
    }
    store_box<T>(node, lo, hi);
  }
}

static unsigned refit_grid(uint64_t most) {
  const uint64_t g = (most + kRefitBlock - 1) / kRefitBlock;
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(g, kRefitMaxGrid));
}

// header + one word per node record (the branch and the leaf list hold the reachable records, each once)
size_t refit_plan_bytes(uint32_t tree_depth, uint64_t num_nodes) { return (plan_header_words(tree_depth + 2u) + (size_t)num_nodes) * sizeof(uint32_t); }

// The plan of the current tree into `plan` (refit_plan_bytes): levels 0 .. tree_depth of the walk from the root.
template <typename T>
hipError_t launch_refit_plan(const typename Wire<T>::Node *nodes, uint64_t num_nodes, uint32_t num_branch_records, uint32_t tree_depth,
                             uint32_t root_is_branch, uint32_t *plan, hipStream_t s) {
  const uint32_t levels = tree_depth + 2u;
  const size_t hdr = plan_header_words(levels);
  uint32_t *branch_list = plan + hdr, *leaf_list = branch_list + num_branch_records;
  const uint32_t leaf_cap = (uint32_t)(num_nodes - num_branch_records);
  hipError_t e = hipMemsetAsync(plan, 0, hdr * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_plan_root, dim3(1), dim3(1), 0, s, plan, levels, root_is_branch, branch_list, leaf_list);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  for (uint32_t d = 0; d + 1 < levels; d++) { // (level d holds at most 2^d branches)
    const uint64_t most = std::min<uint64_t>(d < 32 ? (1ull << d) : ~0ull, num_branch_records);
    hipLaunchKernelGGL((k_plan_expand<T>), dim3(refit_grid(most)), dim3(kRefitBlock), 0, s, nodes, plan, levels, d, branch_list,
                       num_branch_records, leaf_list, leaf_cap);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

// The boxes of every reachable node of a planned tree, from the primitives `prim_box` describes: the leaf pass, then the branch levels.
template <typename T, typename PrimBox>
static hipError_t refit_boxes(const PrimBox &prim_box, const uint32_t *indices, typename Wire<T>::Node *nodes, uint64_t num_nodes,
                              uint32_t num_branch_records, uint32_t tree_depth, const uint32_t *plan, hipStream_t s) {
  const uint32_t levels = tree_depth + 2u;
  const size_t hdr = plan_header_words(levels);
  const uint32_t *branch_list = plan + hdr, *leaf_list = branch_list + num_branch_records;
  const uint32_t leaf_cap = (uint32_t)(num_nodes - num_branch_records);
  hipLaunchKernelGGL((k_refit_leaves<T, PrimBox>), dim3(refit_grid(leaf_cap)), dim3(kRefitBlock), 0, s, nodes, indices, prim_box, plan, levels,
                     leaf_list, leaf_cap);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  for (uint32_t d = levels - 1u; d-- > 0;) { // deepest level first (level tree_depth + 1 is empty: the walk's last level has leaves only)
    const uint64_t most = std::min<uint64_t>(d < 32 ? (1ull << d) : ~0ull, num_branch_records);
    if (most == 0) continue;
    hipLaunchKernelGGL((k_refit_branches<T>), dim3(refit_grid(most)), dim3(kRefitBlock), 0, s, nodes, plan, levels, d, branch_list,
                       num_branch_records);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

// One refit over a planned tree: vertices in, boxes of every reachable node out.
template <typename T>
hipError_t launch_refit(const void *src, size_t stride, uint32_t nv, T *verts, const uint32_t *faces, const uint32_t *indices,
                        typename Wire<T>::Node *nodes, uint64_t num_nodes, uint32_t num_branch_records, uint32_t tree_depth,
                        const uint32_t *plan, hipStream_t s) {
  const hipError_t e = launch_gather_vertices<T>(src, stride, nv, verts, s);
  if (e != hipSuccess) return e;
  return refit_boxes<T>(TriangleBox<T>{faces, verts}, indices, nodes, num_nodes, num_branch_records, tree_depth, plan, s);
}

// The same over spheres or curves (fp32, as their setters): `verts` and `radii` are the context's own arrays, already the new ones.
hipError_t launch_refit_prims(int kind, const float *verts, const float *radii, const uint32_t *indices, nrt_node_f32 *nodes, uint64_t num_nodes,
                              uint32_t num_branch_records, uint32_t tree_depth, const uint32_t *plan, hipStream_t s) {
  if (kind == kPrimSpheres)
    return refit_boxes<float>(RadiusPrimBox<float, kPrimSpheres>{verts, radii}, indices, nodes, num_nodes, num_branch_records, tree_depth, plan, s);
  if (kind == kPrimCurves)
    return refit_boxes<float>(RadiusPrimBox<float, kPrimCurves>{verts, radii}, indices, nodes, num_nodes, num_branch_records, tree_depth, plan, s);
  return hipErrorInvalidValue; // (triangles: launch_refit; cylinders: the builder's segments are not kept)
}

NRT_INSTANTIATE_F32_F64(launch_refit_plan)
NRT_INSTANTIATE_F32_F64(launch_refit)

} // namespace nrt
