// nanort_amd/csrc/kernels.h — the interface between the .hip files of this directory: every function one of them defines and
// another calls is declared here, once, and every one of them that defines or calls such a function includes this header.
// Not part of the C ABI (include/nanort_hip.h).
#pragma once
#include <string>

#include "common.h"

// ---- api_ctx.hip: what the scene and group code may ask of a context ----------------------------------------------------------
nrt_status nrt_internal_tree_view(nrt_ctx *c, nrt::TreeViewF32 *out);
uint64_t nrt_internal_generation(const nrt_ctx *c); // counts the context's rebuilds
int nrt_internal_device(const nrt_ctx *c);
int nrt_internal_prim_kind(const nrt_ctx *c); // nrt::kPrim*

namespace nrt {

// The templates below are defined in one .hip file and used from another: their definitions' file instantiates them for both precisions.
#define NRT_INSTANTIATE_F32_F64(fn)       \
  template decltype(fn<float>) fn<float>; \
  template decltype(fn<double>) fn<double>;

// ---- traverse.hip -----------------------------------------------------------------------------------------------------
// (the *_blocks_per_cu functions: resident blocks per CU of the kernel such a launch runs, what the persistent grid is sized by)
template <typename T>
hipError_t launch_traverse(const TraverseArgs<T> &, unsigned grid, bool count, int lds_entries, hipStream_t);
template <typename T>
int traverse_blocks_per_cu(int lds_entries);
// (walk_variant.h: the instantiation follows from `args`, the context's primitive kind and the LDS depth of its one-level walk;
// `name_out`, optional, receives the kernel's name as rocprofv3 prints it without the argument list)
template <typename T>
hipError_t launch_traverse_wide(const TraverseArgs<T> &args, unsigned grid, int lds_entries, int prim_kind, hipStream_t, const char **name_out);
template <typename T>
int traverse_wide_blocks_per_cu(int lds_entries, int prim_kind, bool wide4);
// scratch: tile counts (ceil(n/1024) u32) followed by dense_of (n u32)
template <typename T>
hipError_t launch_make_wide(const typename Wire<T>::Node *nodes, uint32_t n, uint32_t packed, uint32_t *scratch, WideNode<T> *wide,
                            Wide4Node<T> *wide4, uint32_t scramble_mod, hipStream_t s);

// ---- scene_kernels.hip: the kernels of the two-level path (which of them a call runs: scene.hip) -------------------------------
hipError_t launch_scene_trace(const SceneTraceArgs &args, unsigned grid, hipStream_t s);
int scene_trace_blocks_per_cu();
hipError_t launch_scene_walk(const SceneWalkArgs &args, unsigned grid, hipStream_t s);
int scene_walk_blocks_per_cu();
// The listing step in the form the host chose: a scan of every world box (`nodes`, `num_nodes`), or a walk of the top-level tree
// `top` through its reference-format nodes or its Wide4Node records, the latter with or without pruning beyond a full list.
// One ray per thread, rays[subset ? subset[i] : i] into slot i of n; at most `cap` entries per ray.
// `inst_masks` non-null: the MASKED instantiations (instance visibility masks: one word per instance by id; `ray_masks`: one word per
// ray, indexed like `rays`, or null = every ray 0xFFFFFFFF) — a hidden instance is never listed.
enum SceneListForm : int { kSceneListScan, kSceneListBvh, kSceneListW4, kSceneListW4Prune };
hipError_t launch_scene_list(SceneListForm form, const TreeViewF32 &top, const nrt_ray_f32 *rays, uint32_t n, const NodeDev *nodes, uint32_t num_nodes,
                             uint32_t cap, float *list_t, uint32_t *list_node, uint32_t *count, const uint32_t *subset, const uint32_t *inst_masks,
                             const uint32_t *ray_masks, hipStream_t s);

// ---- scene_closest.hip: the closest-point query on a scene (k_scene_closest_point; include/nanort_closest.h states its rule) -----
constexpr uint32_t kSceneClosestChunk = 64; // points a wave claims per atomic
struct SceneClosestArgs {
  const nrt_point_f32 *points;
  uint32_t n;
  uint32_t num_insts;
  const SceneInst *insts;       // by id: world box, xform, the reference-format nodes and the LeafTri<float> records of the instance's tree
  const nrt_node_f32 *top_nodes; // the top-level tree over the instances' world boxes (reference format), or null: every instance is scanned
  const uint32_t *top_indices;  // ... and its index array: slot -> instance id
  const uint32_t *node_masks;   // one word per instance by id, or null: every instance is admitted
  const uint32_t *point_masks;  // one word per point, or null: every point carries 0xFFFFFFFF
  nrt_scene_closest_f32 *out;
  uint8_t *found;               // may be null
  uint32_t *spill;              // overflow stack [levels][spill_stride], null when no lane's stack can pass the LDS entries
  uint32_t spill_stride;        // == total threads of the launch
  uint32_t *cursor;             // one chunk counter per point partition, kCursorStrideWords apart, zero at launch
  uint32_t num_parts;           // point partitions (<= kMaxParts): whole chunks each
  uint32_t refill_min, trav_min; // as TraverseArgs'
  unsigned long long *counters; // profiling build only: [0] nodes opened (both levels), [1] instances entered, [2] triangles tested; or null
};
hipError_t launch_scene_closest_point(const SceneClosestArgs &args, unsigned grid, hipStream_t s);
int scene_closest_point_blocks_per_cu();

// ---- own_walks.hip: the triangle queries with a binary walk of their own (multi-hit, motion, masks, the three per-ray inputs combined) ----
// One id per kernel; which of them a launch runs: api_query.hip, TraverseLaunch::own_walk_id.
enum OwnWalk : int {
  kOwnMultiHit,                                                                       // k_traverse_multihit
  kOwnMotion,                                                                         // k_traverse_motion
  kOwnMasked,                                                                         // k_traverse_masked
  kOwnQueryMotion, kOwnQueryMasked, kOwnQueryMotionMasked,                            // k_traverse_query<MOTION, MASKED>, with or without ids
  kOwnMultiHitIds, kOwnMultiHitMotion, kOwnMultiHitMasked, kOwnMultiHitMotionMasked,  // k_multihit_query<MOTION, MASKED>, with or without ids
  kNumOwnWalks
};
// What such a launch reads and writes besides its TraverseArgs (args.skip_ids: the per-ray skip ids; args.any_hit: the occlusion query).
// A walk reads the members of its own features only.
template <typename T>
struct OwnWalkInputs {
  uint32_t max_hits;          // multi-hit: K; args.hits holds K records per ray
  uint32_t *counts;           // multi-hit: held hits per ray, may be null
  const void *tris1;          // motion: the LeafTri<T> records of keyframe 1 in leaf order
  const T *times;             // motion: one time per ray, or null (every ray at time 0)
  const uint32_t *leaf_masks; // masked: the faces' words in leaf order, one beside each LeafTri<T> of args.tris
  const uint32_t *ray_masks;  // masked: one word per ray, or null (every ray 0xFFFFFFFF)
};
// (hipErrorInvalidValue: a motion walk without tris1, a masked walk without leaf_masks; `name_out`: as launch_traverse_wide's)
template <typename T>
hipError_t launch_own_walk(OwnWalk w, const TraverseArgs<T> &args, const OwnWalkInputs<T> &in, unsigned grid, hipStream_t s, const char **name_out);
template <typename T>
int own_walk_blocks_per_cu(OwnWalk w);

// ---- closest.hip: the closest-point query (k_closest_point; include/nanort_closest.h states its rule) ---------------------------
template <typename T>
struct ClosestWire;
template <>
struct ClosestWire<float> {
  typedef nrt_point_f32 Point;
  typedef nrt_closest_f32 Record;
};
template <>
struct ClosestWire<double> {
  typedef nrt_point_f64 Point;
  typedef nrt_closest_f64 Record;
};
// `args`: the tree, the trace options, the claim plan over num_rays points and the overflow stack (its rays / hits / mask are not
// read); `points` / `out`: ClosestWire<T>'s records, `found`: a byte per point or null; `name_out`: as launch_traverse_wide's
template <typename T>
hipError_t launch_closest_point(const TraverseArgs<T> &args, const void *points, void *out, uint8_t *found, unsigned grid, hipStream_t s,
                                const char **name_out);
template <typename T>
int closest_point_blocks_per_cu();
// The signed form (k_signed_distance: the same walk, carrying the winning feature; include/nanort_sdf.h states the sign): the
// records are ClosestWire<T>'s with the `feature` word in the place of `_pad`.  `face_normals`: [num_faces][4][3], `vertex_normals`:
// [num_verts][3] (sdf.hip), `faces`: the mesh's index trios.
template <typename T>
struct SignedInputs {
  const T *face_normals, *vertex_normals;
  const uint32_t *faces;
  uint32_t num_faces, num_verts;
};
template <typename T>
hipError_t launch_signed_distance(const TraverseArgs<T> &args, const SignedInputs<T> &in, const void *points, void *out, uint8_t *found, unsigned grid,
                                  hipStream_t s, const char **name_out);
template <typename T>
int signed_distance_blocks_per_cu();

// ---- nearest.hip: the nearest-faces query (k_nearest_faces; the K-nearest rule of include/nanort_closest.h) ----------------------
// `args`, `points`: as launch_closest_point's; `out`: num_rays * max_faces of ClosestWire<T>'s records, each point's row sorted by
// (dist2, prim_id); `counts`: a word per point or null; max_faces: 1..NRT_MAX_NEAREST
template <typename T>
hipError_t launch_nearest_faces(const TraverseArgs<T> &args, const void *points, uint32_t max_faces, void *out, uint32_t *counts, unsigned grid,
                                hipStream_t s, const char **name_out);
template <typename T>
int nearest_faces_blocks_per_cu();

// ---- sdf.hip: the angle-weighted pseudonormals of a triangle mesh (include/nanort_sdf.h states them) ---------------------------------
// The workspace of one derivation for `num_faces` faces and `num_verts` vertices, in bytes.
template <typename T>
size_t feature_normals_workspace_bytes(uint32_t num_faces, uint32_t num_verts);
// face_normals[num_faces][4][3] and vertex_normals[num_verts][3] from the mesh where it lies; the same bytes on every run (no
// floating-point atomics: the corners are sorted by vertex with build.hip's stable sort, and every sum runs in list order).
// 3 * num_faces must fit 32 bits (the caller refuses larger meshes).
template <typename T>
hipError_t launch_feature_normals(const T *verts, const uint32_t *faces, uint32_t num_faces, uint32_t num_verts, void *workspace, T *face_normals,
                                  T *vertex_normals, hipStream_t s);

// ---- build.hip --------------------------------------------------------------------------------------------------------
enum : unsigned { kBuildMorton = 1u, kBuildSubtreeDfs = 2u }; // gpu_build's build_flags: Morton pre-pass, one-node-per-step subtree kernel
struct BuildResult {
  uint64_t num_nodes;
  uint32_t max_depth, num_leaves, num_branches, max_leaf_count;
};
// enqueues a whole build; its size and statistics arrive in `pinned` behind `ev`: gpu_build_result waits for them
// (`d_verts1`: the second vertex keyframe of a triangle mesh, or null — a primitive's box then holds both keyframes)
template <typename T>
hipError_t gpu_build(hipStream_t s, const T *d_verts, const T *d_verts1, const uint32_t *d_faces, const T *d_radii, int prim_kind, const uint32_t *d_prim_map,
                     uint32_t num_faces, uint32_t min_leaf, uint32_t max_depth, uint32_t bin_size, unsigned build_flags, DevBuf *workspace,
                     DevBuf *nodes_buf, DevBuf *indices_buf, void *pinned, hipEvent_t ev, std::string *err);
hipError_t gpu_build_result(const void *pinned, hipEvent_t ev, BuildResult *res);
// The builder's stable LSD radix sort of `n` (32-bit key, value) pairs, 8 bits a pass: sorted pairs end in keys[0] / vals[0];
// keys[1] / vals[1]: scratch of n words each; block_hist: 256 * sort_pairs_blocks(n) words.  No atomics on the order: the same
// output on every run.
size_t sort_pairs_blocks(uint32_t n);
hipError_t launch_sort_pairs(uint32_t *const keys[2], uint32_t *const vals[2], uint32_t *block_hist, uint32_t n, hipStream_t s);

// ---- build_subtree.hip: the subtree phase of a build (the types are the builder's own: build_dev.h) ------------------------
template <typename T>
struct TopNode;
template <typename T>
struct PrimRec;
struct LeafRule;
struct LevelInfo;
// one wave per task of small_list; returns the creation-index map k_emit_small has to apply (nullptr: nodes in pre-order).
// dfs_form: the one-node-per-step kernel, which only the profiling library carries (the product library ignores it)
template <typename T>
const uint16_t *launch_subtree(TopNode<T> *top, const uint32_t *small_list, const PrimRec<T> *recs0, const PrimRec<T> *recs1, int Ks,
                               LeafRule rule, typename Wire<T>::Node *scratch, uint16_t *premap, uint32_t *indices, LevelInfo *info,
                               uint32_t num_small, bool dfs_form, hipStream_t stream);

// ---- refit.hip: the per-tree level plan of a refit, and one refit over it ------------------------------------------------
size_t refit_plan_bytes(uint32_t tree_depth, uint64_t num_nodes);
template <typename T>
hipError_t launch_refit_plan(const typename Wire<T>::Node *nodes, uint64_t num_nodes, uint32_t num_branch_records, uint32_t tree_depth,
                             uint32_t root_is_branch, uint32_t *plan, hipStream_t s);
template <typename T>
hipError_t launch_refit(const void *src, size_t stride, uint32_t nv, T *verts, const uint32_t *faces, const uint32_t *indices,
                        typename Wire<T>::Node *nodes, uint64_t num_nodes, uint32_t num_branch_records, uint32_t tree_depth,
                        const uint32_t *plan, hipStream_t s);
// the same for spheres and curves (fp32): the boxes from the context's positions and radii, already the new ones
hipError_t launch_refit_prims(int kind, const float *verts, const float *radii, const uint32_t *indices, nrt_node_f32 *nodes, uint64_t num_nodes,
                              uint32_t num_branch_records, uint32_t tree_depth, const uint32_t *plan, hipStream_t s);

// ---- prims.hip: per primitive kind (prim_kinds.h), outside the walk ------------------------------------------------------
// the largest of `n_indices` u32 (4-byte aligned, any length) into *out (device), 0 for none
hipError_t launch_max_index(const uint32_t *faces, uint64_t n_indices, uint32_t *out, hipStream_t s);
// `nv` rows of device memory, row i at byte offset i * stride with xyz first, to tight xyz (typed loads when `src` and `stride`
// are multiples of sizeof(T), byte loads otherwise)
template <typename T>
hipError_t launch_gather_vertices(const void *src, size_t stride, uint32_t nv, T *tight, hipStream_t s);
// leaf_masks[k] = masks[tris[k].prim_id] for the `n` LeafTri<T> records of `tris` (`masks`: num_faces words in face order)
template <typename T>
hipError_t launch_permute_masks(const void *tris, const uint32_t *masks, uint32_t num_faces, uint32_t *leaf_masks, uint32_t n, hipStream_t s);
hipError_t launch_cylinder_segments(const float *verts, const float *radii, const uint32_t *seg_off, uint32_t n, float *seg_verts,
                                    float *seg_radii, uint32_t *seg_prim, hipStream_t s);
// the kind's Leaf* record (common.h) for each of the `n` slots of `indices`, into `out` (`faces`: triangles only, `radii`: the others)
template <typename T>
size_t leaf_record_bytes(int kind);
template <typename T>
hipError_t launch_gather_leaf(int kind, const uint32_t *indices, const uint32_t *faces, const T *verts, const T *radii, void *out, uint32_t n,
                              hipStream_t s);
// the pass behind a walk over a kind whose row says post_pass; it closes the launch's completion record (`done_rec`, which the walk
// left open: done_publish == 0).  Spheres: u / v into `hits` in place.  Cylinders, curves: `hits` + `bits` are the walk's compact
// records and {hit, cap} bits, `out` the caller's records of the row's hit_bytes, `mask` (optional) its 0/1 mask.
template <typename T>
hipError_t launch_post_pass(int kind, const typename Wire<T>::Ray *rays, typename Wire<T>::Hit *hits, const uint8_t *bits, const T *verts, uint32_t n,
                            void *out, uint8_t *mask, DoneRec *done_rec, DoneCount *done_count, uint32_t done_seq, hipStream_t s);

} // namespace nrt
