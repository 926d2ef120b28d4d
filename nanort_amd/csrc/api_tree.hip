// nanort_amd/csrc/api_tree.hip — the tree behind the C ABI (include/nanort_hip.h): nrtBuild, adoption and read-back (nrtSetTree /
// nrtGetTree / nrtGetTreeBounds), and the refits.
#include "ctx.h"

// ---------------------------------------------------------------------------
// tree adoption / retrieval
// ---------------------------------------------------------------------------
// Private traversal layout of a tree, in two steps so that a build can enqueue the first while the tree's size is still
// on its way to the host: (1) leaf-ordered primitive records (needs the index array only), (2) WideNode / Wide4Node arrays.
template <typename T>
static nrt_status finish_leaf_records(nrt_ctx *c, hipStream_t s) {
  // leaf-ordered primitive records for the traversal kernel
  if (nrt_status st = ensure(c, c->b_tris, std::max<size_t>(1, c->num_indices) * leaf_record_bytes<T>(c->prim_kind))) return st;
  c->d_tris = c->b_tris.p;
  HIPCHK(c, launch_gather_leaf<T>(c->prim_kind, c->d_indices, c->d_faces, (const T *)c->d_verts, (const T *)c->d_radii, c->d_tris, (uint32_t)c->num_indices, s));
  if (c->d_verts1 && c->prim_kind == kPrimTriangles) { // motion keyframe: the same gather over the second vertex array
    if (nrt_status st = ensure(c, c->b_tris1, std::max<size_t>(1, c->num_indices) * leaf_record_bytes<T>(c->prim_kind))) return st;
    c->d_tris1 = c->b_tris1.p;
    HIPCHK(c, launch_gather_leaf<T>(c->prim_kind, c->d_indices, c->d_faces, (const T *)c->d_verts1, (const T *)nullptr, c->d_tris1, (uint32_t)c->num_indices, s));
  }
  return NRT_OK;
}

template <typename T>
static nrt_status finish_wide(nrt_ctx *c, hipStream_t s) {
  nrt_status st;
  // one WideNode per record with flag == 0 (a loaded tree may carry unreachable ones)
  if ((st = ensure(c, c->b_wide, std::max<size_t>(1, c->num_branch_records) * sizeof(WideNode<T>)))) return st;
  c->d_wide = c->b_wide.p;
  c->packed_leaves = (c->min_leaf_count >= 1 && c->max_leaf_count <= kPackedMaxCount &&
                      c->num_indices <= (uint64_t)kPackedFirstMask) ? 1u : 0u;
  const size_t tiles = (c->num_nodes + 1023) / 1024;
  if ((st = ensure(c, c->b_wide_scratch, (tiles + c->num_nodes + 1) * sizeof(uint32_t)))) return st;
  c->d_wide4 = nullptr;
  // (every primitive kind: the step does not look at the leaves.  Below 4 GiB — 2^25 records — the walk addresses the records with
  // 32-bit byte offsets; triangle trees beyond that, ~110 M triangles and more, get the array too and 64-bit offsets)
  if (c->wide4 && sizeof(T) == 4 && (c->num_branch_records < (1ull << 25) || (c->prim_kind == kPrimTriangles && c->wide4_big_ok))) {
    if ((st = ensure(c, c->b_wide4, std::max<size_t>(1, c->num_branch_records) * sizeof(Wide4Node<T>)))) return st;
    c->d_wide4 = c->b_wide4.p;
  }
  HIPCHK(c, launch_make_wide<T>((const typename Wire<T>::Node *)c->d_nodes, (uint32_t)c->num_nodes, c->packed_leaves,
                                (uint32_t *)c->b_wide_scratch.p, (WideNode<T> *)c->d_wide, (Wide4Node<T> *)c->d_wide4,
                                c->wide_scramble ? c->num_branch_records : 0u, s));
  return NRT_OK;
}

template <typename T>
static nrt_status finish_tree(nrt_ctx *c, hipStream_t s) {
  nrt_status st = finish_leaf_records<T>(c, s);
  return st ? st : finish_wide<T>(c, s);
}

template <typename T>
static nrt_status set_tree(nrt_ctx *c, const typename Wire<T>::Node *nodes, uint64_t num_nodes,
                           const uint32_t *indices, uint64_t num_indices) {
  if (!c) return NRT_ERR_INVALID;
  if (c->prec != (int)sizeof(T)) return fail(c, NRT_ERR_PRECISION, "nrtSetTree: set a mesh of this precision first");
  if (!nodes || !indices || num_nodes == 0) return fail(c, NRT_ERR_INVALID, "nrtSetTree: empty tree");
  if (num_nodes >= 0xFFFFFFFFull || num_indices >= 0xFFFFFFFFull)
    return fail(c, NRT_ERR_INVALID, "nrtSetTree: tree too large");
  // Validate what the traversal loop relies on and measure depth.
  for (uint64_t i = 0; i < num_indices; i++)
    if (indices[i] >= c->num_faces)
      return fail(c, NRT_ERR_INVALID, "nrtSetTree: indices[%llu]=%u >= num_faces %u",
                  (unsigned long long)i, indices[i], c->num_faces);
  uint32_t depth = 0, max_leaf = 0, min_leaf = 0xFFFFFFFFu, nested = 1;
  {
    std::vector<std::pair<uint32_t, uint32_t> > st;
    std::vector<uint8_t> seen(num_nodes, 0);
    st.push_back(std::make_pair(0u, 0u));
    while (!st.empty()) {
      std::pair<uint32_t, uint32_t> e = st.back();
      st.pop_back();
      const typename Wire<T>::Node &n = nodes[e.first];
      if (seen[e.first]) return fail(c, NRT_ERR_INVALID, "nrtSetTree: node %u reachable twice", e.first);
      seen[e.first] = 1;
      depth = std::max(depth, e.second);
      if (n.flag == 0) {
        if (n.data[0] >= num_nodes || n.data[1] >= num_nodes)
          return fail(c, NRT_ERR_INVALID, "nrtSetTree: node %u child out of range", e.first);
        if (n.axis < 0 || n.axis > 2) return fail(c, NRT_ERR_INVALID, "nrtSetTree: node %u axis %d", e.first, n.axis);
        for (int ch = 0; ch < 2; ch++) { // do the child boxes lie inside this one?  (true of every tree a builder emits; a
          const typename Wire<T>::Node &k = nodes[n.data[ch]]; // refit or hand-edited tree may break it: see tree_nested)
          for (int ax = 0; ax < 3; ax++)
            if (!(k.bmin[ax] >= n.bmin[ax] && k.bmax[ax] <= n.bmax[ax])) nested = 0;
        }
        st.push_back(std::make_pair(n.data[1], e.second + 1));
        st.push_back(std::make_pair(n.data[0], e.second + 1));
      } else {
        if ((uint64_t)n.data[1] + n.data[0] > num_indices)
          return fail(c, NRT_ERR_INVALID, "nrtSetTree: leaf %u slots out of range", e.first);
        max_leaf = std::max(max_leaf, n.data[0]);
        min_leaf = std::min(min_leaf, n.data[0]);
      }
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, wait_for_launches(c));
  free_tree(c);
  c->num_nodes = num_nodes;
  c->num_indices = num_indices;
  c->tree_depth = depth;
  c->max_leaf_count = max_leaf;
  c->min_leaf_count = min_leaf;
  c->root_is_branch = nodes[0].flag == 0 ? 1u : 0u;
  c->tree_nested = nested;
  c->num_branch_records = 0;
  for (uint64_t i = 0; i < num_nodes; i++)
    if (nodes[i].flag == 0) c->num_branch_records++;
  nrt_status st;
  if ((st = ensure(c, c->b_nodes, num_nodes * sizeof(typename Wire<T>::Node)))) return st;
  if ((st = ensure(c, c->b_indices, std::max<uint64_t>(1, num_indices) * sizeof(uint32_t)))) return st;
  c->d_nodes = c->b_nodes.p;
  c->d_indices = (uint32_t *)c->b_indices.p;
  HIPCHK(c, hipMemcpy(c->d_nodes, nodes, num_nodes * sizeof(typename Wire<T>::Node), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->d_indices, indices, num_indices * sizeof(uint32_t), hipMemcpyHostToDevice));
  if ((st = finish_tree<T>(c, c->stream))) return st;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NRT_OK;
}

template <typename T>
static nrt_status get_tree(nrt_ctx *c, typename Wire<T>::Node *nodes_out, uint32_t *indices_out) {
  if (!c) return NRT_ERR_INVALID;
  if (c->prec != (int)sizeof(T)) return fail(c, NRT_ERR_PRECISION, "nrtGetTree: precision mismatch");
  if (!c->d_nodes) return fail(c, NRT_ERR_INVALID, "nrtGetTree: no tree");
  NRT_RANGE("nrtGetTree (read-back)");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, refit_host_wait(c));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (nodes_out)
    HIPCHK(c, hipMemcpy(nodes_out, c->d_nodes, c->num_nodes * sizeof(typename Wire<T>::Node), hipMemcpyDeviceToHost));
  if (indices_out)
    HIPCHK(c, hipMemcpy(indices_out, c->d_indices, c->num_indices * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return NRT_OK;
}

template <typename T>
static nrt_status get_tree_bounds(nrt_ctx *c, T *bmin, T *bmax) {
  if (!c || !bmin || !bmax) return NRT_ERR_INVALID;
  if (c->prec != (int)sizeof(T)) return fail(c, NRT_ERR_PRECISION, "nrtGetTreeBounds: precision mismatch");
  if (!c->d_nodes) return fail(c, NRT_ERR_INVALID, "nrtGetTreeBounds: no tree");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, refit_host_wait(c));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  T box[6]; // BVHNode<T> starts with bmin[3], bmax[3] (nanort.h:498-550)
  HIPCHK(c, hipMemcpy(box, c->d_nodes, sizeof(box), hipMemcpyDeviceToHost));
  for (int k = 0; k < 3; k++) {
    bmin[k] = box[k];
    bmax[k] = box[3 + k];
  }
  return NRT_OK;
}

// ---------------------------------------------------------------------------
// build
// ---------------------------------------------------------------------------
template <typename T>
static nrt_status build(nrt_ctx *c, const typename Wire<T>::BuildOptions *opt, nrt_build_stats *stats_out,
                        uint64_t *num_nodes_out) {
  if (!c) return NRT_ERR_INVALID;
  if (c->prec != (int)sizeof(T)) return fail(c, NRT_ERR_PRECISION, "nrtBuild: set a mesh of this precision first");
  if (c->num_faces == 0) return fail(c, NRT_ERR_EMPTY, "nrtBuild: no primitives (reference Build() returns false)");
  uint32_t min_leaf = 4, max_depth = 256, bin_size = 64; // BVHBuildOptions() defaults, nanort.h:574-582
  if (opt) {
    min_leaf = opt->min_leaf_primitives;
    max_depth = opt->max_tree_depth;
    bin_size = opt->bin_size;
  }
  if (bin_size < 2) return fail(c, NRT_ERR_INVALID, "nrtBuild: bin_size must be > 1 (nanort.h:1905)");
  NRT_RANGE("nrtBuild");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, wait_for_launches(c));
  free_tree(c);
  BuildResult res;
  std::string err;
  HIPCHK(c, hipEventRecord(c->ev_b0, c->stream));
  // (cylinder contexts whose cylinders were cut into segments: the tree is built over the segments, each carrying its cylinder's id)
  const bool segs = c->prim_kind == kPrimCylinders && c->num_segs != 0 && sizeof(T) == 4;
  const uint32_t build_n = segs ? c->num_segs : c->num_faces;
  hipError_t e = gpu_build<T>(c->stream, segs ? (const T *)c->b_seg_verts.p : (const T *)c->d_verts, c->prim_kind == kPrimTriangles ? (const T *)c->d_verts1 : nullptr, c->d_faces, segs ? (const T *)c->b_seg_radii.p : (const T *)c->d_radii,
                              c->prim_kind, segs ? (const uint32_t *)c->b_seg_prim.p : nullptr, build_n, min_leaf, max_depth,
                              bin_size, (c->morton ? kBuildMorton : 0u) | (c->subtree_rows ? 0u : kBuildSubtreeDfs), &c->b_build_ws, &c->b_nodes, &c->b_indices, c->build_state, c->ev_build_state, &err);
  if (e != hipSuccess) return fail(c, NRT_ERR_DEVICE, "nrtBuild: %s (%s)", err.c_str(), hipGetErrorString(e));
  // everything is enqueued; the leaf-ordered primitive records need the index array only, so they are enqueued too before
  // the host waits for the tree's size (the GPU stays busy meanwhile)
  c->d_nodes = c->b_nodes.p;
  c->d_indices = (uint32_t *)c->b_indices.p;
  c->num_indices = build_n;
  NRT_RANGE_PUSH("build: leaf-ordered primitive records");
  nrt_status fst = finish_leaf_records<T>(c, c->stream);
  NRT_RANGE_POP();
  if (fst) {
    free_tree(c); // (no half-built tree is left behind: a later traversal call then reports "no tree")
    return fst;
  }
  if ((e = gpu_build_result(c->build_state, c->ev_build_state, &res)) != hipSuccess) {
    free_tree(c);
    return fail(c, NRT_ERR_DEVICE, "nrtBuild: %s", hipGetErrorString(e));
  }
  c->num_nodes = res.num_nodes;
  c->tree_depth = res.max_depth;
  c->max_leaf_count = res.max_leaf_count;
  c->num_branch_records = res.num_branches;
  c->root_is_branch = res.num_nodes > 1 ? 1u : 0u;
  c->min_leaf_count = 1; // the GPU builder never emits an empty leaf
  c->tree_nested = 1;    // a branch's box is the exact union of its children's
  NRT_RANGE_PUSH("build: WideNode / Wide4Node records");
  fst = finish_wide<T>(c, c->stream); // WideNode arrays: part of the build
  NRT_RANGE_POP();
  if (fst) {
    free_tree(c);
    return fst;
  }
  HIPCHK(c, hipEventRecord(c->ev_b1, c->stream));
  HIPCHK(c, hipEventSynchronize(c->ev_b1));
  c->have_build_time = true;
  float ms = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms, c->ev_b0, c->ev_b1));
  c->stats.max_tree_depth = res.max_depth;
  c->stats.num_leaf_nodes = res.num_leaves;
  c->stats.num_branch_nodes = res.num_branches;
  c->stats.build_secs = (ms + (segs ? c->segment_ms : 0.f)) * 1e-3f; // (cylinder trees: + the segmentation nrtSetCylinders did for this build)
  if (stats_out) *stats_out = c->stats;
  if (num_nodes_out) *num_nodes_out = c->num_nodes;
  return NRT_OK;
}

// ---------------------------------------------------------------------------
// refit (refit.hip): new vertex positions, the same topology
// ---------------------------------------------------------------------------
// The level plan of the current tree, built on the device by the first refit after the tree changed (the tree is only read).
template <typename T>
static nrt_status refit_plan(nrt_ctx *c, hipStream_t s) {
  if (c->refit_planned) return NRT_OK;
  if (nrt_status st = ensure(c, c->b_refit_plan, refit_plan_bytes(c->tree_depth, c->num_nodes))) return st;
  HIPCHK(c, launch_refit_plan<T>((const typename Wire<T>::Node *)c->d_nodes, c->num_nodes, c->num_branch_records, c->tree_depth,
                                 c->root_is_branch, (uint32_t *)c->b_refit_plan.p, s));
  c->refit_planned = true;
  return NRT_OK;
}

// What follows the new boxes (`e`: how their launches went): the leaf records and WideNode / Wide4Node arrays from the new boxes
// and positions, as a build derives them; then the host form waits, the Device form records ev_refit.  A device error leaves no
// half-refit tree behind: the context drops its tree and its primitives, and the message ends in `remedy`.
template <typename T>
static nrt_status refit_finish(nrt_ctx *c, const char *fn, hipError_t e, bool device, hipStream_t s, const char *remedy) {
  nrt_status st = NRT_OK;
  c->tree_nested = 1; // every box now lies inside its parent's
  if (e == hipSuccess && (st = finish_tree<T>(c, s))) e = hipErrorUnknown;
  if (e == hipSuccess && !device) e = hipStreamSynchronize(s);
  if (e == hipSuccess && device) {
    std::lock_guard<std::mutex> lock(c->launch_mutex);
    if ((e = hipEventRecord(c->ev_refit, s)) == hipSuccess) c->refit_pending = true;
  }
  if (e != hipSuccess) {
    const std::string why = st ? c->err : std::string(hipGetErrorString(e));
    (void)hipStreamSynchronize(s);
    free_tree(c);
    free_mesh(c);
    return fail(c, NRT_ERR_DEVICE, "%s: %s (the context's tree and primitives were dropped: %s)", fn, why.c_str(), remedy);
  }
  c->generation++; // a committed nrt_scene over this context holds stale top-level boxes: it refuses until committed again
  return NRT_OK;
}

// `device`: `vertices` is device memory read by the gather kernel, and the call returns once everything is enqueued on `s`;
// else the caller's vertex block is uploaded into b_refit_stage first and the call returns when the refit is complete.
template <typename T>
static nrt_status refit(nrt_ctx *c, const T *vertices, size_t stride, bool device, hipStream_t s) {
  const char *fn = device ? "nrtRefitDevice" : "nrtRefit";
  if (!c) return NRT_ERR_INVALID;
  if (!vertices) return fail(c, NRT_ERR_INVALID, "%s: NULL vertices", fn);
  if (c->prec != 0 && c->prec != (int)sizeof(T))
    return fail(c, NRT_ERR_PRECISION, "%s: the context holds %s primitives", fn, c->prec == 8 ? "f64" : "f32");
  if (c->prim_kind != kPrimTriangles) return fail(c, NRT_ERR_INVALID, "%s: only triangle meshes refit (this context holds %s)", fn,
                                                  kPrimKinds[c->prim_kind].name);
  if (c->d_verts1)
    return fail(c, NRT_ERR_INVALID, "%s: the context holds a motion keyframe (nrtSetMeshMotion): its boxes cover both keyframes and a refit of "
                "one would shrink them; remove the keyframe or set the mesh and build again", fn);
  if (!c->d_nodes) return fail(c, NRT_ERR_INVALID, "%s: no tree (call nrtBuild or nrtSetTree)", fn);
  if (stride < 3 * sizeof(T)) return fail(c, NRT_ERR_INVALID, "%s: vertex stride %zu < %zu", fn, stride, 3 * sizeof(T));
  if (device && (stride % sizeof(T) != 0 || (uintptr_t)vertices % sizeof(T) != 0))
    return fail(c, NRT_ERR_INVALID, "%s: vertex stride %zu or pointer not aligned to %zu bytes", fn, stride, sizeof(T));
  NRT_RANGE("nrtRefit");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, wait_for_launches(c)); // (launches in flight read the arrays the refit rewrites; also a previous Device refit)
  if (!device) s = c->stream;
  nrt_status st = NRT_OK;
  const uint32_t nv = c->num_verts;
  const size_t block = nv ? (size_t)(nv - 1) * stride + 3 * sizeof(T) : 0;
  const void *src = vertices;
  if (!device && nv) {
    if ((st = ensure(c, c->b_refit_stage, block))) return st;
    HIPCHK(c, hipMemcpyAsync(c->b_refit_stage.p, vertices, block, hipMemcpyHostToDevice, s));
    src = c->b_refit_stage.p;
  }
  if ((st = refit_plan<T>(c, s))) return st;
  // From here on the vertices, the boxes and the leaf / wide records are being rewritten: a device error leaves no half-refit
  // tree behind — the context drops its tree and its primitives (free_tree bumps generation), as a failed build drops its tree.
  c->feature_normals_stale = true; // (the vertices move: the pseudonormals of the signed distance query are the old mesh's)
  const hipError_t e = launch_refit<T>(src, stride, nv, (T *)c->d_verts, c->d_faces, c->d_indices,
                                       (typename Wire<T>::Node *)c->d_nodes, c->num_nodes, c->num_branch_records, c->tree_depth,
                                       (const uint32_t *)c->b_refit_plan.p, s);
  return refit_finish<T>(c, fn, e, device, s, "set the mesh again");
}

// nrtRefitPrims* (spheres and curves): the context's positions (and radii, when given) replaced by the caller's tight arrays, then
// the boxes from them by the kind's builder rule.  `device`: the arrays are device memory copied on `s`, and the call returns once
// everything is enqueued there; else the call returns when the refit is complete.
static nrt_status refit_prims(nrt_ctx *c, const float *positions, const float *radii, uint32_t n, bool device, hipStream_t s) {
  const char *fn = device ? "nrtRefitPrimsDevice" : "nrtRefitPrims";
  if (!c) return NRT_ERR_INVALID;
  if (!positions) return fail(c, NRT_ERR_INVALID, "%s: NULL positions", fn);
  if (c->prec == 8) return fail(c, NRT_ERR_PRECISION, "%s: the context holds f64 primitives", fn);
  if (c->prec != 0 && c->prim_kind == kPrimTriangles)
    return fail(c, NRT_ERR_INVALID, "%s: this context holds triangles: refit a mesh with nrtRefit / nrtRefitDevice", fn);
  if (c->prec != 0 && c->prim_kind == kPrimCylinders)
    return fail(c, NRT_ERR_INVALID, "%s: cylinders do not refit: the tree is built over segments the builder cut them into, and which "
                "cylinder end a slot of the index array stands for is not recoverable from it (nrtSetCylinders + nrtBuild again)", fn);
  if (!c->d_nodes) return fail(c, NRT_ERR_INVALID, "%s: no tree (call nrtBuild or nrtSetTree)", fn);
  const PrimKind &k = kPrimKinds[c->prim_kind];
  if (n != c->num_faces) return fail(c, NRT_ERR_INVALID, "%s: num_prims %u differs from the context's %u %s", fn, n, c->num_faces, k.name);
  if (device && ((uintptr_t)positions % sizeof(float) != 0 || (uintptr_t)radii % sizeof(float) != 0))
    return fail(c, NRT_ERR_INVALID, "%s: pointer not aligned to 4 bytes", fn);
  NRT_RANGE("nrtRefitPrims");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, wait_for_launches(c)); // (launches in flight read the arrays the refit rewrites; also a previous Device refit)
  if (!device) s = c->stream;
  if (nrt_status st = refit_plan<float>(c, s)) return st;
  // From here on the context's arrays are being rewritten (refit_finish: a device error drops the tree and the primitives).
  const hipMemcpyKind dir = device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  hipError_t e = hipMemcpyAsync(c->d_verts, positions, (size_t)k.pos_floats * n * sizeof(float), dir, s);
  if (e == hipSuccess && radii) e = hipMemcpyAsync(c->d_radii, radii, (size_t)k.radius_floats * n * sizeof(float), dir, s);
  if (e == hipSuccess)
    e = launch_refit_prims(c->prim_kind, (const float *)c->d_verts, (const float *)c->d_radii, c->d_indices, (nrt_node_f32 *)c->d_nodes, c->num_nodes,
                           c->num_branch_records, c->tree_depth, (const uint32_t *)c->b_refit_plan.p, s);
  return refit_finish<float>(c, fn, e, device, s, "set the primitives again");
}

extern "C" {

nrt_status nrtBuild_f32(nrt_ctx *c, const nrt_build_options_f32 *o, nrt_build_stats *st, uint64_t *nn) {
  return build<float>(c, o, st, nn);
}
nrt_status nrtBuild_f64(nrt_ctx *c, const nrt_build_options_f64 *o, nrt_build_stats *st, uint64_t *nn) {
  return build<double>(c, o, st, nn);
}

nrt_status nrtGetTree_f32(nrt_ctx *c, nrt_node_f32 *n, uint32_t *i) { return get_tree<float>(c, n, i); }
nrt_status nrtGetTree_f64(nrt_ctx *c, nrt_node_f64 *n, uint32_t *i) { return get_tree<double>(c, n, i); }
nrt_status nrtTreeSize(nrt_ctx *c, uint64_t *nn, uint64_t *ni) {
  if (!c) return NRT_ERR_INVALID;
  if (nn) *nn = c->num_nodes;
  if (ni) *ni = c->num_indices;
  return NRT_OK;
}
nrt_status nrtGetTreeBounds_f32(nrt_ctx *c, float *lo, float *hi) { return get_tree_bounds<float>(c, lo, hi); }
nrt_status nrtGetTreeBounds_f64(nrt_ctx *c, double *lo, double *hi) { return get_tree_bounds<double>(c, lo, hi); }

nrt_status nrtSetTree_f32(nrt_ctx *c, const nrt_node_f32 *n, uint64_t nn, const uint32_t *i, uint64_t ni) {
  return set_tree<float>(c, n, nn, i, ni);
}
nrt_status nrtSetTree_f64(nrt_ctx *c, const nrt_node_f64 *n, uint64_t nn, const uint32_t *i, uint64_t ni) {
  return set_tree<double>(c, n, nn, i, ni);
}

nrt_status nrtRefit_f32(nrt_ctx *c, const float *v, size_t stride) { return refit<float>(c, v, stride, false, nullptr); }
nrt_status nrtRefit_f64(nrt_ctx *c, const double *v, size_t stride) { return refit<double>(c, v, stride, false, nullptr); }
nrt_status nrtRefitDevice_f32(nrt_ctx *c, const float *v, size_t stride, void *s) { return refit<float>(c, v, stride, true, (hipStream_t)s); }
nrt_status nrtRefitDevice_f64(nrt_ctx *c, const double *v, size_t stride, void *s) { return refit<double>(c, v, stride, true, (hipStream_t)s); }
nrt_status nrtRefitPrims_f32(nrt_ctx *c, const float *p, const float *r, uint32_t n) { return refit_prims(c, p, r, n, false, nullptr); }
nrt_status nrtRefitPrimsDevice_f32(nrt_ctx *c, const float *p, const float *r, uint32_t n, void *s) { return refit_prims(c, p, r, n, true, (hipStream_t)s); }

} // extern "C"
