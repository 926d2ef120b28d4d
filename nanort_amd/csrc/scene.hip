// nanort_amd/csrc/scene.hip — the HOST side of two-level (instanced) traversal: SURVEY.md §8(f) row 3.  Commit, the choice of
// path per call, the tunables and the C entry points; every kernel it launches is scene_kernels.hip's, behind kernels.h.
//
// Replaces nanosg::Scene<float, M>::Commit / Traverse (reference examples/nanosg/nanosg.h:700-870) and the
// BVHAccel::ListNodeIntersections it rests on (reference nanort.h:2608-2692).  Two paths give the same records:
//
//   THE SINGLE-PASS WALK (scenes of kWalkMinNodes nodes or more): k_scene_walk walks the top-level tree and, on
//   reaching an instance, the instance's own tree in the same lane on the same stack — no per-ray list; a per-ray certificate
//   says when the record is provably the reference's, the other rays (few) are appended to a list and go through
//   THE LISTING PATH (small scenes; the rays handed over; tunable single_pass = 0):
//
//   k_scene_list* (per ray: the at most 64 nearest instances whose world boxes it enters, through the top-level BVH or, for a
//   handful of nodes, a scan) + k_scene_trace (the reference's loop over that list), for the whole batch or the subset handed over.
//
// The per-node arithmetic of Commit (Matrix::Mult / Inverse / MultV, XformBoundingBox) follows the
// reference operation for operation; this file is compiled with the same no-contraction / IEEE flags.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "kernels.h"
#ifdef NRT_PROF
#include "../../include/nanort_hip_prof.h"
#endif

namespace {

using nrt::kMaxList, nrt::kTopStack, nrt::mult_v, nrt::NodeDev;

constexpr uint32_t kScanMaxNodes = 8; // scenes of at most this many nodes are listed by the scan
constexpr unsigned kWalkBackoff = 15;   // listing-path calls after a batch of which the walk handed over more than a quarter
constexpr uint32_t kWalkMinNodes = 64; // scenes of at least this many nodes are traced by the single-pass walk (100 - 1 000 instances: 5-8 % faster than the
                                      // listing path, 10 000: 1.7x, 100 000: 9x; the 5-node fixture: 6-20 % slower — profiles/r04n_scene_walk.txt, r04t_*)

// ---- host-side restatement of the per-node update (nanosg.h:92-241, 246-302, 397-437) ----------------
void mat_mult(float dst[4][4], const float m0[4][4], const float m1[4][4]) {
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      dst[i][j] = 0;
      for (int k = 0; k < 4; ++k) dst[i][j] += m0[k][j] * m1[i][k];
    }
}

void mat_inverse(float m[4][4]) { // Cramer's rule, same operation order as the reference
  float tmp[12], s[16], det;
  for (int i = 0; i < 4; i++) {
    s[i] = m[i][0];
    s[i + 4] = m[i][1];
    s[i + 8] = m[i][2];
    s[i + 12] = m[i][3];
  }
  tmp[0] = s[10] * s[15]; tmp[1] = s[11] * s[14]; tmp[2] = s[9] * s[15]; tmp[3] = s[11] * s[13];
  tmp[4] = s[9] * s[14]; tmp[5] = s[10] * s[13]; tmp[6] = s[8] * s[15]; tmp[7] = s[11] * s[12];
  tmp[8] = s[8] * s[14]; tmp[9] = s[10] * s[12]; tmp[10] = s[8] * s[13]; tmp[11] = s[9] * s[12];
  m[0][0] = tmp[0] * s[5] + tmp[3] * s[6] + tmp[4] * s[7];
  m[0][0] -= tmp[1] * s[5] + tmp[2] * s[6] + tmp[5] * s[7];
  m[0][1] = tmp[1] * s[4] + tmp[6] * s[6] + tmp[9] * s[7];
  m[0][1] -= tmp[0] * s[4] + tmp[7] * s[6] + tmp[8] * s[7];
  m[0][2] = tmp[2] * s[4] + tmp[7] * s[5] + tmp[10] * s[7];
  m[0][2] -= tmp[3] * s[4] + tmp[6] * s[5] + tmp[11] * s[7];
  m[0][3] = tmp[5] * s[4] + tmp[8] * s[5] + tmp[11] * s[6];
  m[0][3] -= tmp[4] * s[4] + tmp[9] * s[5] + tmp[10] * s[6];
  m[1][0] = tmp[1] * s[1] + tmp[2] * s[2] + tmp[5] * s[3];
  m[1][0] -= tmp[0] * s[1] + tmp[3] * s[2] + tmp[4] * s[3];
  m[1][1] = tmp[0] * s[0] + tmp[7] * s[2] + tmp[8] * s[3];
  m[1][1] -= tmp[1] * s[0] + tmp[6] * s[2] + tmp[9] * s[3];
  m[1][2] = tmp[3] * s[0] + tmp[6] * s[1] + tmp[11] * s[3];
  m[1][2] -= tmp[2] * s[0] + tmp[7] * s[1] + tmp[10] * s[3];
  m[1][3] = tmp[4] * s[0] + tmp[9] * s[1] + tmp[10] * s[2];
  m[1][3] -= tmp[5] * s[0] + tmp[8] * s[1] + tmp[11] * s[2];
  tmp[0] = s[2] * s[7]; tmp[1] = s[3] * s[6]; tmp[2] = s[1] * s[7]; tmp[3] = s[3] * s[5];
  tmp[4] = s[1] * s[6]; tmp[5] = s[2] * s[5]; tmp[6] = s[0] * s[7]; tmp[7] = s[3] * s[4];
  tmp[8] = s[0] * s[6]; tmp[9] = s[2] * s[4]; tmp[10] = s[0] * s[5]; tmp[11] = s[1] * s[4];
  m[2][0] = tmp[0] * s[13] + tmp[3] * s[14] + tmp[4] * s[15];
  m[2][0] -= tmp[1] * s[13] + tmp[2] * s[14] + tmp[5] * s[15];
  m[2][1] = tmp[1] * s[12] + tmp[6] * s[14] + tmp[9] * s[15];
  m[2][1] -= tmp[0] * s[12] + tmp[7] * s[14] + tmp[8] * s[15];
  m[2][2] = tmp[2] * s[12] + tmp[7] * s[13] + tmp[10] * s[15];
  m[2][2] -= tmp[3] * s[12] + tmp[6] * s[13] + tmp[11] * s[15];
  m[2][3] = tmp[5] * s[12] + tmp[8] * s[13] + tmp[11] * s[14];
  m[2][3] -= tmp[4] * s[12] + tmp[9] * s[13] + tmp[10] * s[14];
  m[3][0] = tmp[2] * s[10] + tmp[5] * s[11] + tmp[1] * s[9];
  m[3][0] -= tmp[4] * s[11] + tmp[0] * s[9] + tmp[3] * s[10];
  m[3][1] = tmp[8] * s[11] + tmp[0] * s[8] + tmp[7] * s[10];
  m[3][1] -= tmp[6] * s[10] + tmp[9] * s[11] + tmp[1] * s[8];
  m[3][2] = tmp[6] * s[9] + tmp[11] * s[11] + tmp[3] * s[8];
  m[3][2] -= tmp[10] * s[11] + tmp[2] * s[8] + tmp[7] * s[9];
  m[3][3] = tmp[10] * s[10] + tmp[4] * s[8] + tmp[9] * s[9];
  m[3][3] -= tmp[8] * s[9] + tmp[11] * s[0] + tmp[5] * s[8];
  det = s[0] * m[0][0] + s[1] * m[0][1] + s[2] * m[0][2] + s[3] * m[0][3];
  det = 1.0f / det;
  for (int j = 0; j < 4; j++)
    for (int i = 0; i < 4; i++) m[j][i] *= det;
}

void node_update(const float local[4][4], const float lbmin[3], const float lbmax[3], NodeDev *out) {
  float ident[4][4];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) ident[i][j] = (i == j) ? 1.0f : 0.0f;
  mat_mult(out->xform, ident, local);
  float xb[8][3];
  for (int i = 0; i < 8; i++) {
    const float b[3] = {(i & 1) ? lbmax[0] : lbmin[0], (i & 2) ? lbmax[1] : lbmin[1], (i & 4) ? lbmax[2] : lbmin[2]};
    mult_v(xb[i], out->xform, b);
  }
  for (int k = 0; k < 3; k++) out->xbmin[k] = out->xbmax[k] = xb[0][k];
  for (int i = 1; i < 8; i++)
    for (int k = 0; k < 3; k++) {
      out->xbmin[k] = std::min(xb[i][k], out->xbmin[k]);
      out->xbmax[k] = std::max(xb[i][k], out->xbmax[k]);
    }
  memcpy(out->inv_xform, out->xform, sizeof(out->xform));
  mat_inverse(out->inv_xform);
  memcpy(out->inv_xform33, out->xform, sizeof(out->xform));
  out->inv_xform33[3][0] = out->inv_xform33[3][1] = out->inv_xform33[3][2] = 0.0f;
  mat_inverse(out->inv_xform33);
}

thread_local std::string g_scene_create_error;

} // namespace

struct nrt_scene {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  struct Inst {
    nrt_ctx *mesh;
    float local[4][4];
  };
  std::vector<Inst> insts;
  std::vector<NodeDev> host_nodes;
  bool committed = false;
  // instance visibility masks (nrtSceneSetNodeMasks): one word per node by id, no part of the top-level tree.  The device holds two
  // copies — by id (the listing kernels, the scan) and in the order of d_open_top (the walk: the word beside the line it opens) —
  // rewritten from this one by the next masked query when `masks_dirty` (scene calls are synchronous: nothing is in flight).
  std::vector<uint32_t> node_masks;  // insts.size() words
  std::vector<uint32_t> top_order;   // the top-level tree's index array at Commit (empty: no top-level tree)
  std::vector<uint32_t> top_masks_h; // staging: node_masks in that order
  bool masks_dirty = true;
  std::vector<std::pair<nrt_ctx *, uint64_t> > mesh_gens; // the distinct mesh contexts and their generations at Commit (the
                                                          // per-instance table caches their device addresses and flags)
  nrt_ctx *top = nullptr;        // top-level BVH over the nodes' world boxes (scenes of two nodes or more)
  nrt::TreeViewF32 top_view;
  bool use_top = false;          // the listing kernels walk the top-level tree (scenes of more than kScanMaxNodes nodes; else they scan the nodes)
  bool have_top = false;         // a top-level tree exists (two nodes or more): the single-pass walk uses it
  uint32_t max_inst_depth = 0;   // deepest instance tree: sizes the overflow stack of k_scene_trace
  nrt::DevBuf d_nodes, d_insts, d_rays, d_list_t, d_list_node, d_count, d_best, d_mask, d_spill, d_spill_tmin, d_cursor;
  nrt::DevBuf d_redo, d_redo_count, d_counters, d_open_top, d_meshes;
  nrt::DevBuf d_node_masks, d_top_masks, d_ray_masks; // the two copies of node_masks; the host forms' staged ray words
  nrt::DevBuf d_skip_pairs;               // the host form's staged skip pairs (nrtSceneQueryBatch_f32), packed to 8 bytes
  std::vector<uint32_t> skip_pairs_h;     // ... and where they are packed (alive until the call's last synchronize)
  bool walk_meshes_ok = false; // every mesh of the scene has the private layout k_scene_walk steps through (else: the listing path)
  unsigned count_loops = 0; // profiling build only (tunable "count_loops"): the next calls run the counting instantiation of k_scene_walk
  uint32_t *h_redo_count = nullptr; // page-locked: how many rays the single-pass walk left to the listing path
  uint64_t last_redone = 0;
  int last_path = 0; // 1: the last call went through the single-pass walk (0: the listing path alone)
  unsigned single_pass = 1;   // scenes of kWalkMinNodes nodes or more are traced by k_scene_walk (no per-ray list); 0: always listing +
                              // k_scene_trace; 2: k_scene_walk for every scene of two nodes or more
  unsigned walk_blocks_per_cu = 0;
  unsigned walk_leaf_items = 1; // the walk's leaf phase over items (walk_dev.h leaf_items_one_trip; records bit-identical) when every mesh's leaves hold <= 4 records
  unsigned max_mesh_leaf = 0;   // most records a leaf of any instanced mesh holds (set by commit)
  unsigned walk_trav_min = 24, walk_refill_min = 24; // the walk's own phase thresholds (profiles/r04t_scene_walk_thresholds.txt: 8 / 56, the listing path's, cost it 10-13 %)
  unsigned walk_backoff = 0;  // calls left that skip the walk (see scene_traverse)
  unsigned walk_backoff_pct = 25; // share of a batch handed to the listing path above which the next kWalkBackoff calls skip the walk (tunable)
  unsigned walk_min = kWalkMinNodes; // scenes of at least this many nodes are traced by the walk (tunable "walk_min")
  unsigned prune_min = 32768; // scenes of at least this many instances are listed by the pruning walk (k_scene_list_w4<true>)
  unsigned scan_max = kScanMaxNodes; // scenes of at most this many nodes are listed by testing every world box (no top-level tree); tunable, <= kMaxList (next Commit)
  unsigned fuse_scan = 1; // scenes of at most kScanMaxNodes nodes: k_scene_trace lists a ray's instances itself (one launch); 0: k_scene_list in a launch of its own (the A/B)
  unsigned trav_min = 8;
  unsigned cand_min = 1, cand_busy_max = 64; // batching of the per-instance steps of k_scene_trace (env NRT_SCENE_CAND / NRT_SCENE_CAND_BUSY; 1 / 64: none)
  unsigned closest_blocks_per_cu = 0; // persistent grid of k_scene_closest_point (scene_closest below)
  unsigned closest_refill_min = 44, closest_trav_min = 16; // ... and its phase thresholds: the single-mesh closest-point walk's (ctx.h), not measured apart
  unsigned trace_blocks_per_cu = 0, num_cus = 0, refill_min = 56; // persistent grid of k_scene_trace (env NRT_SCENE_REFILL; 16-48 measured slower on small scenes, 64 slower on 10 000 instances)
};

static nrt_status sfail(nrt_scene *s, nrt_status st, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (s)
    s->err = buf;
  else
    g_scene_create_error = buf;
  return st;
}

#define SCHK(s, call)                                                                                          \
  do {                                                                                                         \
    hipError_t e_ = (call);                                                                                    \
    if (e_ != hipSuccess)                                                                                      \
      return sfail((s), NRT_ERR_DEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

extern "C" {

nrt_status nrtSceneCreate(int device, nrt_scene **out) {
  if (!out) return sfail(nullptr, NRT_ERR_INVALID, "nrtSceneCreate: out == NULL");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return sfail(nullptr, NRT_ERR_DEVICE, "nrtSceneCreate: no HIP device visible");
  if (device < 0 || device >= ndev) return sfail(nullptr, NRT_ERR_INVALID, "nrtSceneCreate: device %d out of range", device);
  nrt_scene *s = new nrt_scene();
  s->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
    delete s;
    return sfail(nullptr, NRT_ERR_DEVICE, "nrtSceneCreate: stream creation failed");
  }
  *out = s;
  return NRT_OK;
}

void nrtSceneDestroy(nrt_scene *s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  (void)hipStreamSynchronize(s->stream);
  nrt::DevBuf *bufs[] = {&s->d_nodes, &s->d_insts, &s->d_rays, &s->d_list_t, &s->d_list_node, &s->d_count,
                         &s->d_best,  &s->d_mask,  &s->d_spill, &s->d_spill_tmin, &s->d_cursor, &s->d_redo, &s->d_redo_count, &s->d_counters, &s->d_open_top, &s->d_meshes,
                         &s->d_node_masks, &s->d_top_masks, &s->d_ray_masks, &s->d_skip_pairs};
  for (nrt::DevBuf *b : bufs)
    if (b->p) (void)hipFree(b->p);
  if (s->h_redo_count) (void)hipHostFree(s->h_redo_count);
  if (s->top) nrtDestroy(s->top);
  (void)hipStreamDestroy(s->stream);
  delete s;
}

const char *nrtSceneLastError(const nrt_scene *s) { return s ? s->err.c_str() : g_scene_create_error.c_str(); }

nrt_status nrtSceneAddNode_f32(nrt_scene *s, nrt_ctx *mesh, const float local_xform[16], uint32_t *node_id_out) {
  if (!s) return NRT_ERR_INVALID;
  if (!mesh || !local_xform) return sfail(s, NRT_ERR_INVALID, "nrtSceneAddNode: NULL mesh or transform");
  uint64_t nn = 0, ni = 0;
  if (nrtTreeSize(mesh, &nn, &ni) != NRT_OK || nn == 0)
    return sfail(s, NRT_ERR_INVALID, "nrtSceneAddNode: the mesh context has no tree (call nrtBuild first)");
  if (nrt_internal_prim_kind(mesh) == (int)nrt::kPrimCurves)
    return sfail(s, NRT_ERR_INVALID, "nrtSceneAddNode: scenes instance triangle meshes (this context holds curves)");
  nrt_scene::Inst in;
  in.mesh = mesh;
  memcpy(in.local, local_xform, sizeof(in.local));
  s->insts.push_back(in);
  s->node_masks.push_back(0xFFFFFFFFu); // visible to every non-zero ray word until nrtSceneSetNodeMasks says otherwise
  s->masks_dirty = true;
  s->committed = false;
  if (node_id_out) *node_id_out = (uint32_t)s->insts.size() - 1;
  return NRT_OK;
}

nrt_status nrtSceneCommit(nrt_scene *s) {
  if (!s) return NRT_ERR_INVALID;
  if (s->insts.empty()) return sfail(s, NRT_ERR_EMPTY, "nrtSceneCommit: empty scene (the reference's Commit() returns false)");
  SCHK(s, hipSetDevice(s->device));
  s->host_nodes.resize(s->insts.size());
  // per distinct mesh context (instances share them): where its tree lives, and its root box
  struct MeshInfo {
    nrt::TreeViewF32 tv;
    nrt_node_f32 root;
  };
  std::vector<std::pair<nrt_ctx *, MeshInfo> > meshes;
  s->max_mesh_leaf = 0;
  std::unordered_map<nrt_ctx *, uint32_t> mesh_index;
  std::vector<uint32_t> mesh_of(s->insts.size());
  for (size_t i = 0; i < s->insts.size(); i++) {
    std::unordered_map<nrt_ctx *, uint32_t>::iterator it = mesh_index.find(s->insts[i].mesh);
    uint32_t m = it == mesh_index.end() ? (uint32_t)meshes.size() : it->second;
    if (it == mesh_index.end()) {
      mesh_index[s->insts[i].mesh] = m;
      MeshInfo mi;
      if (nrt_internal_tree_view(s->insts[i].mesh, &mi.tv) != NRT_OK || mi.tv.prim_kind != (uint32_t)nrt::kPrimTriangles)
        return sfail(s, NRT_ERR_PRECISION, "nrtSceneCommit: node %zu is not a built f32 triangle mesh: %s", i, nrtLastError(s->insts[i].mesh));
      SCHK(s, hipMemcpy(&mi.root, mi.tv.nodes, sizeof(mi.root), hipMemcpyDeviceToHost));
      s->max_mesh_leaf = std::max(s->max_mesh_leaf, (unsigned)mi.tv.max_leaf_count);
      meshes.push_back(std::make_pair(s->insts[i].mesh, mi));
    }
    mesh_of[i] = m;
    // local AABB = the root box of the node's tree (accel_.BoundingBox, nanosg.h:411)
    node_update(s->insts[i].local, meshes[m].second.root.bmin, meshes[m].second.root.bmax, &s->host_nodes[i]);
  }
  SCHK(s, nrt::devbuf_ensure(&s->d_nodes, s->host_nodes.size() * sizeof(NodeDev)));
  SCHK(s, hipMemcpy(s->d_nodes.p, s->host_nodes.data(), s->host_nodes.size() * sizeof(NodeDev), hipMemcpyHostToDevice));
  // per-instance table of k_scene_trace: where each node's tree lives + its three matrices
  std::vector<nrt::SceneInst> table(s->insts.size());
  s->max_inst_depth = 0;
  for (size_t i = 0; i < s->insts.size(); i++) {
    const nrt::TreeViewF32 &tv = meshes[mesh_of[i]].second.tv;
    nrt::SceneInst &e = table[i];
    e.wide = tv.wide;
    e.wide4 = (tv.tree_nested && tv.root_is_branch) ? tv.wide4 : nullptr; // two levels per step need nested boxes (walk_dev.h NRT_STEP_NODE4)
    e.tris = tv.prims;
    e.nodes = tv.nodes;
    e.packed_leaves = tv.packed_leaves;
    e.root_is_branch = tv.root_is_branch;
    e.tree_nested = tv.tree_nested;
    e.pad = 0;
    memcpy(e.inv_xform, s->host_nodes[i].inv_xform, sizeof(e.inv_xform));
    memcpy(e.inv_xform33, s->host_nodes[i].inv_xform33, sizeof(e.inv_xform33));
    memcpy(e.xform, s->host_nodes[i].xform, sizeof(e.xform));
    memcpy(e.xbmin, s->host_nodes[i].xbmin, sizeof(e.xbmin));
    memcpy(e.xbmax, s->host_nodes[i].xbmax, sizeof(e.xbmax));
    e.id = (uint32_t)i;
    e.pad2 = 0;
    // deepest stack a walk of this tree can need: one pending sibling per level, three per two levels when stepping two
    s->max_inst_depth = std::max(s->max_inst_depth, e.wide4 ? 3u * (tv.tree_depth / 2u + 1u) : tv.tree_depth);
  }
  SCHK(s, nrt::devbuf_ensure(&s->d_insts, table.size() * sizeof(nrt::SceneInst)));
  SCHK(s, hipMemcpy(s->d_insts.p, table.data(), table.size() * sizeof(nrt::SceneInst), hipMemcpyHostToDevice));
  // top-level BVH over the world boxes (nanosg.h:726-735: BVHAccel over the nodes with min_leaf_primitives = 1), built
  // by the ordinary GPU builder: a box is handed over as a zero-radius "cylinder" from its low to its high corner, whose
  // bounding box is exactly the box.  Which nodes a ray lists does not depend on this tree's shape.
  s->use_top = false;
  s->have_top = false;
  s->walk_backoff = 0;
  s->top_order.clear(); // (Commit keeps the masks themselves; their copy in top-level order follows the new tree)
  s->masks_dirty = true;
  // ... only where something reads it: the listing kernels of scenes of more than kScanMaxNodes nodes, the single-pass walk from
  // walk_min nodes (or forced, single_pass = 2).  A handful of nodes is scanned: no context, no build, no read-back for them
  // (a tunable that makes the walk eligible later commits the scene again: scene_traverse).
  const bool want_top = s->insts.size() > s->scan_max || (s->single_pass && (s->insts.size() >= s->walk_min || s->single_pass > 1));
  if (s->insts.size() >= 2 && want_top) {
    if (!s->top && nrtCreate(s->device, &s->top) != NRT_OK)
      return sfail(s, NRT_ERR_DEVICE, "nrtSceneCommit: top-level context: %s", nrtLastError(nullptr));
    std::vector<float> ends(6 * s->insts.size()), radii(2 * s->insts.size(), 0.0f);
    for (size_t i = 0; i < s->insts.size(); i++)
      for (int k = 0; k < 3; k++) {
        ends[6 * i + k] = s->host_nodes[i].xbmin[k];
        ends[6 * i + 3 + k] = s->host_nodes[i].xbmax[k];
      }
    nrt_build_options_f32 o;
    memset(&o, 0, sizeof(o));
    o.cost_t_aabb = 0.2f;
    o.min_leaf_primitives = 1;
    o.max_tree_depth = 256;
    o.bin_size = 64;
    o.shallow_depth = 4;
    o.min_primitives_for_parallel_build = 1024 * 8;
    if (nrtSetCylinders_f32(s->top, ends.data(), radii.data(), (uint32_t)s->insts.size(), 0) != NRT_OK ||
        nrtBuild_f32(s->top, &o, nullptr, nullptr) != NRT_OK || nrt_internal_tree_view(s->top, &s->top_view) != NRT_OK)
      return sfail(s, NRT_ERR_DEVICE, "nrtSceneCommit: top-level build: %s", nrtLastError(s->top));
    // the single-pass walk opens an instance with ONE fetch: a 128-byte line per instance, in the order of the tree's index array
    {
      uint64_t nn = 0, ni = 0;
      if (nrtTreeSize(s->top, &nn, &ni) != NRT_OK || ni != s->insts.size())
        return sfail(s, NRT_ERR_DEVICE, "nrtSceneCommit: top-level index array: %s", nrtLastError(s->top));
      std::vector<uint32_t> order(ni);
      if (nrtGetTree_f32(s->top, nullptr, order.data()) != NRT_OK)
        return sfail(s, NRT_ERR_DEVICE, "nrtSceneCommit: top-level index array: %s", nrtLastError(s->top));
      std::vector<nrt::SceneOpen> open(ni); // (the 128-byte line an opening reads; the full record, by id, only when the instance was hit)
      for (size_t q = 0; q < ni; q++) {
        const nrt::SceneInst &e = table[order[q]];
        nrt::SceneOpen &o = open[q];
        for (int r = 0; r < 4; r++)
          for (int c = 0; c < 3; c++) {
            o.inv[r][c] = e.inv_xform[r][c];
            o.inv33[r][c] = e.inv_xform33[r][c];
          }
        memcpy(o.xbmin, e.xbmin, sizeof(o.xbmin));
        memcpy(o.xbmax, e.xbmax, sizeof(o.xbmax));
        o.id = e.id;
        o.mesh = mesh_of[order[q]];
      }
      s->top_order = order;
      SCHK(s, nrt::devbuf_ensure(&s->d_open_top, open.size() * sizeof(nrt::SceneOpen)));
      SCHK(s, hipMemcpy(s->d_open_top.p, open.data(), open.size() * sizeof(nrt::SceneOpen), hipMemcpyHostToDevice));
      std::vector<nrt::SceneMesh> mt(meshes.size());
      s->walk_meshes_ok = true; // the walk steps two levels at a time through packed leaf references, from a branch root whose children lie inside it
      for (size_t m = 0; m < meshes.size(); m++) {
        const nrt::TreeViewF32 &tv = meshes[m].second.tv;
        const nrt_node_f32 &root = meshes[m].second.root;
        memset(&mt[m], 0, sizeof(mt[m]));
        mt[m].wide4 = tv.wide4;
        mt[m].tris = tv.prims;
        const bool one_leaf = !tv.root_is_branch && root.flag != 0 && root.data[0] >= 1 && root.data[0] <= nrt::kPackedMaxCount &&
                              root.data[1] <= nrt::kPackedFirstMask;
        if (one_leaf) {
          mt[m].root_leaf = 1;
          mt[m].leaf_ref = nrt::packed_leaf_ref(root.data[0], root.data[1]);
          memcpy(mt[m].bmin, root.bmin, sizeof(mt[m].bmin));
          memcpy(mt[m].bmax, root.bmax, sizeof(mt[m].bmax));
        }
        s->walk_meshes_ok = s->walk_meshes_ok && tv.prims && (one_leaf || (tv.wide4 && tv.tree_nested && tv.root_is_branch && tv.packed_leaves));
      }
      SCHK(s, nrt::devbuf_ensure(&s->d_meshes, mt.size() * sizeof(nrt::SceneMesh)));
      SCHK(s, hipMemcpy(s->d_meshes.p, mt.data(), mt.size() * sizeof(nrt::SceneMesh), hipMemcpyHostToDevice));
    }
    s->have_top = true;                                                                              // the single-pass walk's
    s->use_top = s->insts.size() > s->scan_max && s->top_view.tree_depth + 2 < (uint32_t)kTopStack; // the listing kernels' (else: the scan)
  }
  s->mesh_gens.clear();
  for (size_t m = 0; m < meshes.size(); m++) s->mesh_gens.push_back(std::make_pair(meshes[m].first, meshes[m].second.tv.generation));
  s->committed = true;
  return NRT_OK;
}

// One visibility word per node, in node-id order (include/nanort_hip.h).  Host state only: the next masked query uploads it.
nrt_status nrtSceneSetNodeMasks(nrt_scene *s, const uint32_t *masks, uint32_t count) {
  if (!s) return NRT_ERR_INVALID;
  if (masks && (size_t)count != s->insts.size())
    return sfail(s, NRT_ERR_INVALID, "nrtSceneSetNodeMasks: %u words for a scene of %zu nodes (one word per node added so far)", count, s->insts.size());
  if (masks)
    s->node_masks.assign(masks, masks + count);
  else
    s->node_masks.assign(s->insts.size(), 0xFFFFFFFFu);
  s->masks_dirty = true;
  return NRT_OK;
}

// Scene::GetBoundingBox (nanosg.h:761-769): the root box of the top-level tree, i.e. the plain union of the nodes'
// world boxes (nanort.h:1546-1567 pads nothing).
nrt_status nrtSceneBounds_f32(nrt_scene *s, float bmin[3], float bmax[3]) {
  if (!s || !bmin || !bmax) return NRT_ERR_INVALID;
  if (!s->committed) return sfail(s, NRT_ERR_INVALID, "nrtSceneBounds: commit the scene first");
  for (int k = 0; k < 3; k++) {
    bmin[k] = s->host_nodes[0].xbmin[k];
    bmax[k] = s->host_nodes[0].xbmax[k];
  }
  for (size_t i = 1; i < s->host_nodes.size(); i++)
    for (int k = 0; k < 3; k++) {
      bmin[k] = std::min(bmin[k], s->host_nodes[i].xbmin[k]);
      bmax[k] = std::max(bmax[k], s->host_nodes[i].xbmax[k]);
    }
  return NRT_OK;
}

// What Node::Update derives from the local transform (nanosg.h:397-437), for callers that finish the
// reference's Intersection record (P, Ns, Ng) on the host: xform, inv_xform, inv_xform33 and
// inv_transpose_xform33 = transpose(inv_xform33) (nanosg.h:430-432), 16 floats each, row-major T[4][4].
nrt_status nrtSceneNodeState_f32(nrt_scene *s, uint32_t node_id, float out[64]) {
  if (!s || !out) return NRT_ERR_INVALID;
  if (!s->committed) return sfail(s, NRT_ERR_INVALID, "nrtSceneNodeState: commit the scene first");
  if (node_id >= s->host_nodes.size()) return sfail(s, NRT_ERR_INVALID, "nrtSceneNodeState: node %u out of range", node_id);
  const NodeDev &nd = s->host_nodes[node_id];
  memcpy(out, nd.xform, 64);
  memcpy(out + 16, nd.inv_xform, 64);
  memcpy(out + 32, nd.inv_xform33, 64);
  for (int j = 0; j < 4; j++)
    for (int i = 0; i < 4; i++) out[48 + 4 * j + i] = nd.inv_xform33[i][j];
  return NRT_OK;
}

} // extern "C"

// The node words on the device, enqueued on the scene's stream before a query that reads them: both copies from the host's when they
// changed since the last such query (or the top-level tree's order did).
static nrt_status upload_node_masks(nrt_scene *s) {
  if (!s->masks_dirty) return NRT_OK;
  const size_t bytes = s->node_masks.size() * sizeof(uint32_t);
  SCHK(s, nrt::devbuf_ensure(&s->d_node_masks, bytes));
  SCHK(s, hipMemcpyAsync(s->d_node_masks.p, s->node_masks.data(), bytes, hipMemcpyHostToDevice, s->stream));
  if (s->top_order.size() == s->node_masks.size()) {
    s->top_masks_h.resize(s->top_order.size());
    for (size_t q = 0; q < s->top_order.size(); q++) s->top_masks_h[q] = s->node_masks[s->top_order[q]];
    SCHK(s, nrt::devbuf_ensure(&s->d_top_masks, bytes));
    SCHK(s, hipMemcpyAsync(s->d_top_masks.p, s->top_masks_h.data(), bytes, hipMemcpyHostToDevice, s->stream));
  }
  s->masks_dirty = false;
  return NRT_OK;
}

// The listing path: one of the listing kernels + k_scene_trace, enqueued on the scene's stream, over the whole batch
// (`subset` == nullptr) or over the rays named by `subset` (the ones the single-pass walk left over).  `any_hit`: the occlusion
// instantiation of k_scene_trace — the same lists, flags only, d_hits unused.
// `masked`: the MASKED instantiations of the listing kernels and of the scan, with `d_ray_masks` (one word per ray of the batch, or
// null) and the scene's by-id words.
// `d_skip_pairs` non-null: the SKIP instantiations of k_scene_trace (the listing kernels test no primitive), pairs `skip_stride` bytes
// apart and indexed by the ray, like `d_ray_masks`.
static nrt_status scene_list_and_trace(nrt_scene *s, const nrt_ray_f32 *d_rays, uint32_t n, const uint32_t *subset,
                                       nrt_scene_hit_f32 *d_hits, uint8_t *d_mask, bool any_hit, bool masked = false,
                                       const uint32_t *d_ray_masks = nullptr, const void *d_skip_pairs = nullptr, uint32_t skip_stride = 0) {
  const uint32_t num_nodes = (uint32_t)s->insts.size();
  const uint32_t cap = std::min<uint32_t>(kMaxList, num_nodes);
  SCHK(s, nrt::devbuf_ensure(&s->d_list_t, (size_t)cap * n * sizeof(float)));
  SCHK(s, nrt::devbuf_ensure(&s->d_list_node, (size_t)cap * n * sizeof(uint32_t)));
  SCHK(s, nrt::devbuf_ensure(&s->d_count, (size_t)n * sizeof(uint32_t)));
  const unsigned grid = (n + 255u) / 256u; // the listing kernels: one ray per thread
  const unsigned trace_grid = std::min(grid, s->num_cus * s->trace_blocks_per_cu); // the trace kernel: every block resident
  const uint32_t levels = s->max_inst_depth + 2 > (uint32_t)nrt::kSceneLdsStack ? s->max_inst_depth + 2 - nrt::kSceneLdsStack : 0;
  if (levels) {
    SCHK(s, nrt::devbuf_ensure(&s->d_spill, (size_t)levels * trace_grid * 256u * sizeof(uint32_t)));
    SCHK(s, nrt::devbuf_ensure(&s->d_spill_tmin, (size_t)levels * trace_grid * 256u * sizeof(float)));
  }
  SCHK(s, hipMemsetAsync(s->d_cursor.p, 0, (size_t)nrt::kMaxParts * nrt::kCursorStrideWords * sizeof(uint32_t), s->stream));
  const NodeDev *d_nodes = (const NodeDev *)s->d_nodes.p;
  const bool fused_scan = !s->use_top && s->fuse_scan && num_nodes <= (uint32_t)kMaxList; // (every entered box fits the list: no replacement logic needed in the trace kernel)
  const bool top_w4 = s->use_top && s->top_view.wide4 && s->top_view.root_is_branch && s->top_view.tree_nested &&
                      3u * (s->top_view.tree_depth / 2u + 1u) + 2u < (uint32_t)kTopStack;
  const nrt::SceneListForm form = top_w4 ? (num_nodes >= s->prune_min ? nrt::kSceneListW4Prune // (rays can enter more boxes than the list holds: the pruning walk)
                                                                      : nrt::kSceneListW4)
                                         : (s->use_top ? nrt::kSceneListBvh : nrt::kSceneListScan);
  if (s->use_top || !fused_scan) // (else: a handful of nodes — k_scene_trace tests every world box itself as it fetches a ray: no listing launch)
    SCHK(s, nrt::launch_scene_list(form, s->top_view, d_rays, n, d_nodes, num_nodes, cap, (float *)s->d_list_t.p, (uint32_t *)s->d_list_node.p,
                                   (uint32_t *)s->d_count.p, subset, masked ? (const uint32_t *)s->d_node_masks.p : nullptr, d_ray_masks, s->stream));
  nrt::SceneTraceArgs a;
  a.scan_nodes = fused_scan ? num_nodes : 0u;
  a.rays = d_rays;
  a.n = n;
  a.insts = (const nrt::SceneInst *)s->d_insts.p;
  a.list_t = (float *)s->d_list_t.p;
  a.list_node = (uint32_t *)s->d_list_node.p;
  a.count = (const uint32_t *)s->d_count.p;
  a.hits = d_hits;
  a.mask = d_mask;
  a.spill = (uint32_t *)s->d_spill.p;
  a.spill_tmin = (float *)s->d_spill_tmin.p;
  a.spill_stride = trace_grid * 256u;
  a.cursor = (uint32_t *)s->d_cursor.p;
  a.num_parts = std::max(1u, std::min(8u, trace_grid));
  a.refill_min = s->refill_min;
  a.trav_min = s->trav_min;
  a.cand_min = s->cand_min;
  a.cand_busy_max = s->cand_busy_max;
  a.subset = subset;
  a.any_hit = any_hit ? 1u : 0u;
  a.masked = (masked && fused_scan) ? 1u : 0u; // (a listed ray's list holds visible instances only: the plain instantiation traces it)
  a.ray_masks = d_ray_masks;
  a.inst_masks = (const uint32_t *)s->d_node_masks.p;
  a.skip = d_skip_pairs ? 1u : 0u;
  a.skip_stride = skip_stride;
  a.skip_pairs = d_skip_pairs;
  if (d_skip_pairs && !masked) a.inst_masks = nullptr; // (the SKIP scan is the MASKED form: null = all-ones node words, and d_ray_masks is null)
  SCHK(s, nrt::launch_scene_trace(a, trace_grid, s->stream));
  return NRT_OK;
}

// `device` = rays / hits_out / mask_out are device pointers (no PCIe traffic).  Scenes with a top-level tree: ONE launch of the
// single-pass walk (k_scene_walk), then — only if it left rays over — the listing path on those; other scenes (a handful of
// nodes) and single_pass = 0: the listing path on the whole batch.  The call returns with everything finished (the scene owns
// the per-ray scratch).  `occluded`: the occlusion query (scene_occluded below) — the same path selection and ray staging with
// the any-hit kernel instantiations; no record buffer is allocated, written or copied (hits_out is NULL), mask_out is required,
// and the closest-hit back-off is neither consulted nor updated.  `masked`: the masked queries (nrtScene*BatchMasked*) — the same
// checks, path selection, back-off and reporting with the MASKED kernel instantiations; `ray_masks` (one word per ray, host or
// device as the rays; NULL: every ray 0xFFFFFFFF) is staged beside the rays, and the node words are uploaded first if they changed.
// `skip_pairs` non-null (nrtSceneQueryBatch* with SKIP): per-ray skip pairs `skip_stride` bytes apart, host or device as the rays —
// the same checks, path selection, back-off and reporting with the SKIP kernel instantiations; the host form stages the pairs packed
// to 8 bytes beside the rays.  `query`: the call is nrtSceneQueryBatch* (the name in messages).
static nrt_status scene_traverse(nrt_scene *s, const nrt_ray_f32 *rays, uint64_t n64, nrt_scene_hit_f32 *hits_out,
                                 uint8_t *mask_out, bool device, bool occluded = false, bool masked = false, const uint32_t *ray_masks = nullptr,
                                 const void *skip_pairs = nullptr, uint32_t skip_stride = 0, bool query = false) {
  if (!s) return NRT_ERR_INVALID;
  const char *what = query ? (device ? "nrtSceneQueryBatchDevice" : "nrtSceneQueryBatch") : masked ? (occluded ? "nrtSceneOccludedBatchMasked" : "nrtSceneTraverseBatchMasked") : (occluded ? "nrtSceneOccludedBatch" : "nrtSceneTraverseBatch");
  if (!s->committed) return sfail(s, NRT_ERR_INVALID, "%s: commit the scene first", what);
  if (n64 == 0) return NRT_OK;
  if (!rays || (occluded ? !mask_out : !hits_out)) return sfail(s, NRT_ERR_INVALID, "%s: NULL rays/%s", what, occluded ? "mask" : "hits");
  if (n64 > 0x7FFFFFFFull) return sfail(s, NRT_ERR_INVALID, "%s: too many rays in one call", what);
  if (masked && device && ((uintptr_t)ray_masks & 3u) != 0)
    return sfail(s, NRT_ERR_INVALID, "%s: d_ray_masks is not 4-byte aligned", what);
  if (skip_pairs) {
    if (skip_stride < 8u || (skip_stride & 3u) != 0)
      return sfail(s, NRT_ERR_INVALID, "%s: skip_stride_bytes = %u (a pair is 8 bytes: at least 8, and a multiple of 4)", what, skip_stride);
    if (device) {
      if (((uintptr_t)skip_pairs & 3u) != 0) return sfail(s, NRT_ERR_INVALID, "%s: skip_pairs is not 4-byte aligned", what);
      // the walk re-reads a pair while other rays' records are being written
      const uintptr_t p0 = (uintptr_t)skip_pairs, p1 = p0 + (uintptr_t)(n64 - 1) * skip_stride + 8u;
      const uintptr_t h0 = (uintptr_t)hits_out, h1 = h0 + (uintptr_t)n64 * sizeof(nrt_scene_hit_f32);
      const uintptr_t m0 = (uintptr_t)mask_out, m1 = m0 + (uintptr_t)n64;
      if ((!occluded && p0 < h1 && h0 < p1) || (mask_out && p0 < m1 && m0 < p1))
        return sfail(s, NRT_ERR_INVALID, "%s: skip_pairs overlaps %s (pass the PREVIOUS wave's records, not the ones being written)", what,
                     (!occluded && p0 < h1 && h0 < p1) ? "hits_out" : "mask_out");
    }
  }
  // the instance table holds device addresses, layout flags and stack depths of the mesh contexts' trees as they were at
  // Commit: a context rebuilt or re-set since then may have moved or re-shaped them — refuse instead of walking stale memory
  for (size_t m = 0; m < s->mesh_gens.size(); m++)
    if (nrt_internal_generation(s->mesh_gens[m].first) != s->mesh_gens[m].second)
      return sfail(s, NRT_ERR_INVALID, "%s: a mesh context was rebuilt or re-set since nrtSceneCommit (commit the scene again)", what);
  const uint32_t n = (uint32_t)n64;
  SCHK(s, hipSetDevice(s->device));
  if (!device) SCHK(s, nrt::devbuf_ensure(&s->d_rays, (size_t)n * sizeof(nrt_ray_f32)));
  if (!device && !occluded) SCHK(s, nrt::devbuf_ensure(&s->d_best, (size_t)n * sizeof(nrt_scene_hit_f32)));
  if (!device && mask_out) SCHK(s, nrt::devbuf_ensure(&s->d_mask, (size_t)n));
  if (s->trace_blocks_per_cu == 0) {
    s->trace_blocks_per_cu = (unsigned)nrt::scene_trace_blocks_per_cu();
    s->walk_blocks_per_cu = (unsigned)nrt::scene_walk_blocks_per_cu();
    hipDeviceProp_t prop;
    SCHK(s, hipGetDeviceProperties(&prop, s->device));
    s->num_cus = (unsigned)prop.multiProcessorCount;
    if (nrt::env_overrides_allowed()) {
    if (const char *e = getenv("NRT_SCENE_REFILL")) s->refill_min = (unsigned)std::min(64, std::max(1, atoi(e)));
    if (const char *e = getenv("NRT_SCENE_TRAV")) s->trav_min = (unsigned)std::min(64, std::max(1, atoi(e)));
    if (const char *e = getenv("NRT_SCENE_CAND")) s->cand_min = (unsigned)std::min(64, std::max(1, atoi(e)));
    if (const char *e = getenv("NRT_SCENE_CAND_BUSY")) s->cand_busy_max = (unsigned)std::min(65, std::max(1, atoi(e)));
    if (const char *e = getenv("NRT_SCENE_PRUNE_MIN")) s->prune_min = (unsigned)std::max(0, atoi(e)); // (debugging / tests: the pruning walk on small scenes)
    if (const char *e = getenv("NRT_SCENE_WALK_TRAV")) s->walk_trav_min = (unsigned)std::min(64, std::max(1, atoi(e)));
    if (const char *e = getenv("NRT_SCENE_WALK_REFILL")) s->walk_refill_min = (unsigned)std::min(64, std::max(1, atoi(e)));
    if (const char *e = getenv("NRT_SCENE_WALK")) s->single_pass = (unsigned)std::min(2, std::max(0, atoi(e)));
    }
  }
  // the walk became eligible after Commit (nrtSceneSetTunable / the variables above) on a scene committed without its top-level tree
  if (s->single_pass && !s->have_top && s->insts.size() >= 2 && s->insts.size() <= s->scan_max &&
      (s->insts.size() >= s->walk_min || s->single_pass > 1)) {
    const nrt_status st = nrtSceneCommit(s);
    if (st) return st;
  }
  SCHK(s, nrt::devbuf_ensure(&s->d_cursor, (size_t)nrt::kMaxParts * nrt::kCursorStrideWords * sizeof(uint32_t)));
  const nrt_ray_f32 *d_rays = device ? rays : (const nrt_ray_f32 *)s->d_rays.p;
  nrt_scene_hit_f32 *d_hits = occluded ? nullptr : (device ? hits_out : (nrt_scene_hit_f32 *)s->d_best.p);
  uint8_t *d_mask = device ? mask_out : (mask_out ? (uint8_t *)s->d_mask.p : nullptr);
  if (!device) SCHK(s, hipMemcpyAsync(s->d_rays.p, rays, (size_t)n * sizeof(nrt_ray_f32), hipMemcpyHostToDevice, s->stream));
  const uint32_t *d_ray_masks = nullptr;
  if (masked) {
    d_ray_masks = ray_masks;
    if (!device && ray_masks) { // the words travel beside the rays
      SCHK(s, nrt::devbuf_ensure(&s->d_ray_masks, (size_t)n * sizeof(uint32_t)));
      SCHK(s, hipMemcpyAsync(s->d_ray_masks.p, ray_masks, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
      d_ray_masks = (const uint32_t *)s->d_ray_masks.p;
    }
  }
  const void *d_skip_pairs = skip_pairs;
  uint32_t d_skip_stride = skip_stride;
  if (skip_pairs && !device) { // the pairs travel beside the rays, packed to 8 bytes
    s->skip_pairs_h.resize((size_t)n * 2u);
    for (uint32_t r = 0; r < n; r++) memcpy(&s->skip_pairs_h[(size_t)r * 2u], (const char *)skip_pairs + (size_t)r * skip_stride, 8);
    SCHK(s, nrt::devbuf_ensure(&s->d_skip_pairs, (size_t)n * 8u));
    SCHK(s, hipMemcpyAsync(s->d_skip_pairs.p, s->skip_pairs_h.data(), (size_t)n * 8u, hipMemcpyHostToDevice, s->stream));
    d_skip_pairs = s->d_skip_pairs.p;
    d_skip_stride = 8u;
  }
  if (masked) {
    const nrt_status st = upload_node_masks(s);
    if (st != NRT_OK) return st;
  }

  s->last_redone = 0;
  s->last_path = 0;
  const bool eligible = s->single_pass && s->have_top && (s->insts.size() >= s->walk_min || s->single_pass > 1) && s->walk_meshes_ok && s->top_view.wide4 &&
                        s->top_view.root_is_branch && s->top_view.tree_nested && s->top_view.packed_leaves;
  // a batch the walk could not certify for the most part (direction vectors far shorter than 1: the reference's cull then compares
  // a distance with a parameter and fires early, nanosg.h:795) costs more than the listing path alone: after one, the next
  // kWalkBackoff calls go straight to the listing path, then the walk is tried again
  // (an occlusion ray cannot be handed over by that cull — it acts only once there is a hit, and the first hit ends the ray — so
  // occlusion calls always take the walk when it is eligible and leave the back-off counter alone)
  const bool walk = eligible && (occluded || s->single_pass > 1 || s->walk_backoff == 0);
  if (eligible && !walk) s->walk_backoff--;
  if (walk) {
    s->last_path = 1;
    if (!s->h_redo_count) SCHK(s, hipHostMalloc((void **)&s->h_redo_count, sizeof(uint32_t), hipHostMallocDefault));
    SCHK(s, nrt::devbuf_ensure(&s->d_redo, (size_t)n * sizeof(uint32_t)));
    SCHK(s, nrt::devbuf_ensure(&s->d_redo_count, sizeof(uint32_t)));
    const unsigned grid = std::min((n + 255u) / 256u, s->num_cus * s->walk_blocks_per_cu);
    // the lane's stack: top-level entries (three per two levels of the top-level tree, the instances of one leaf) below the open instance's
    const uint32_t need = 3u * (s->top_view.tree_depth / 2u + 1u) + 2u + nrt::kPackedMaxCount + s->max_inst_depth + 2u;
    const uint32_t levels = need > (uint32_t)nrt::kSceneWalkLdsStack ? need - nrt::kSceneWalkLdsStack : 0;
    if (levels) {
      SCHK(s, nrt::devbuf_ensure(&s->d_spill, (size_t)levels * grid * 256u * sizeof(uint32_t)));
      SCHK(s, nrt::devbuf_ensure(&s->d_spill_tmin, (size_t)levels * grid * 256u * sizeof(float)));
    }
    SCHK(s, hipMemsetAsync(s->d_cursor.p, 0, (size_t)nrt::kMaxParts * nrt::kCursorStrideWords * sizeof(uint32_t), s->stream));
    SCHK(s, hipMemsetAsync(s->d_redo_count.p, 0, sizeof(uint32_t), s->stream));
    nrt::SceneWalkArgs w;
    w.rays = d_rays;
    w.n = n;
    w.open_top = (const nrt::SceneOpen *)s->d_open_top.p;
    w.meshes = (const nrt::SceneMesh *)s->d_meshes.p;
    w.insts = (const nrt::SceneInst *)s->d_insts.p;
    w.top_wide4 = (const nrt::Wide4Node<float> *)s->top_view.wide4;
    w.hits = d_hits;
    w.mask = d_mask;
    w.spill = (uint32_t *)s->d_spill.p;
    w.spill_tmin = (float *)s->d_spill_tmin.p;
    w.spill_stride = grid * 256u;
    w.cursor = (uint32_t *)s->d_cursor.p;
    w.num_parts = std::max(1u, std::min(8u, grid));
    w.refill_min = s->walk_refill_min;
    w.trav_min = s->walk_trav_min;
    w.cand_min = s->cand_min;
    w.cand_busy_max = s->cand_busy_max;
    w.leaf_items = (s->walk_leaf_items && s->max_mesh_leaf <= 4u) ? 1u : 0u;
    w.redo = (uint32_t *)s->d_redo.p;
    w.redo_count = (uint32_t *)s->d_redo_count.p;
    w.counters = nullptr;
    w.any_hit = occluded ? 1u : 0u;
    w.num_insts = (uint32_t)s->insts.size();
    w.masked = masked ? 1u : 0u;
    w.ray_masks = d_ray_masks;
    w.top_masks = (const uint32_t *)s->d_top_masks.p;
    w.skip = d_skip_pairs ? 1u : 0u;
    w.skip_stride = d_skip_stride;
    w.skip_pairs = d_skip_pairs;
    if (d_skip_pairs && !masked) w.top_masks = nullptr; // (the SKIP walk is the MASKED form: null = all-ones node words, and d_ray_masks is null)
#ifdef NRT_PROF
    if (s->count_loops && !occluded && !masked && !d_skip_pairs) {
      SCHK(s, nrt::devbuf_ensure(&s->d_counters, 16 * sizeof(unsigned long long)));
      SCHK(s, hipMemsetAsync(s->d_counters.p, 0, 16 * sizeof(unsigned long long), s->stream));
      w.counters = (unsigned long long *)s->d_counters.p;
    }
#endif
    SCHK(s, nrt::launch_scene_walk(w, grid, s->stream));
    SCHK(s, hipMemcpyAsync(s->h_redo_count, s->d_redo_count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    SCHK(s, hipStreamSynchronize(s->stream));
    s->last_redone = *s->h_redo_count;
    if (!occluded && (uint64_t)*s->h_redo_count * 100u > (uint64_t)n * s->walk_backoff_pct) s->walk_backoff = kWalkBackoff;
    if (*s->h_redo_count) {
      const nrt_status st = scene_list_and_trace(s, d_rays, *s->h_redo_count, (const uint32_t *)s->d_redo.p, d_hits, d_mask, occluded, masked, d_ray_masks, d_skip_pairs, d_skip_stride);
      if (st != NRT_OK) return st;
    }
  } else {
    const nrt_status st = scene_list_and_trace(s, d_rays, n, nullptr, d_hits, d_mask, occluded, masked, d_ray_masks, d_skip_pairs, d_skip_stride);
    if (st != NRT_OK) return st;
  }
  if (!device) {
    if (!occluded) SCHK(s, hipMemcpyAsync(hits_out, s->d_best.p, (size_t)n * sizeof(nrt_scene_hit_f32), hipMemcpyDeviceToHost, s->stream));
    if (mask_out) SCHK(s, hipMemcpyAsync(mask_out, s->d_mask.p, (size_t)n, hipMemcpyDeviceToHost, s->stream));
  }
  SCHK(s, hipStreamSynchronize(s->stream));
  return NRT_OK;
}

// The occlusion query: scene_traverse's path selection and ray staging with the any-hit kernels; one byte per ray is all that is
// produced, staged or copied (include/nanort_hip.h: the nrtSceneOccludedBatch contract).
static nrt_status scene_occluded(nrt_scene *s, const nrt_ray_f32 *rays, uint64_t n64, uint8_t *mask_out, bool device) {
  return scene_traverse(s, rays, n64, nullptr, mask_out, device, true);
}

// ---- the closest-point query (include/nanort_hip.h, "closest-point queries on scenes"; the kernel: scene_closest.hip) --------------
const uint64_t kSceneClosestPiece = 1ull << 20; // points per launch of the staged host form (16 MB and 4 MB of words up, 33 MB down)

// One launch of k_scene_closest_point over `n` points in device memory, enqueued on the scene's stream; the caller synchronises.
static nrt_status scene_closest_launch(nrt_scene *s, const nrt_point_f32 *d_points, uint32_t n, const uint32_t *d_point_masks,
                                       nrt_scene_closest_f32 *d_out, uint8_t *d_found) {
  if (s->num_cus == 0) {
    int cus = 0;
    SCHK(s, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device));
    s->num_cus = (unsigned)std::max(1, cus);
  }
  if (s->closest_blocks_per_cu == 0) s->closest_blocks_per_cu = (unsigned)nrt::scene_closest_point_blocks_per_cu();
  const unsigned grid = std::max(1u, std::min((n + 255u) / 256u, s->num_cus * s->closest_blocks_per_cu));
  // a lane's stack: the top level's entries — one pending sibling per level of the top-level tree and the instances of one of its
  // leaves, or every instance of a scanned scene — below the open instance's, one pending sibling per level of its tree
  const uint32_t top_entries = s->have_top ? s->top_view.tree_depth + 2u + s->top_view.max_leaf_count : (uint32_t)s->insts.size();
  const uint32_t need = top_entries + s->max_inst_depth + 2u;
  const uint32_t levels = need > (uint32_t)nrt::kLdsStackDefault ? need - nrt::kLdsStackDefault : 0;
  if (levels) SCHK(s, nrt::devbuf_ensure(&s->d_spill, (size_t)levels * grid * 256u * sizeof(uint32_t)));
  SCHK(s, nrt::devbuf_ensure(&s->d_cursor, (size_t)nrt::kMaxParts * nrt::kCursorStrideWords * sizeof(uint32_t)));
  SCHK(s, hipMemsetAsync(s->d_cursor.p, 0, (size_t)nrt::kMaxParts * nrt::kCursorStrideWords * sizeof(uint32_t), s->stream));
  nrt::SceneClosestArgs a;
  a.points = d_points;
  a.n = n;
  a.num_insts = (uint32_t)s->insts.size();
  a.insts = (const nrt::SceneInst *)s->d_insts.p;
  a.top_nodes = s->have_top ? s->top_view.nodes : nullptr; // (no top-level build that Commit did not make: such scenes are scanned)
  a.top_indices = s->have_top ? s->top_view.indices : nullptr;
  a.node_masks = d_point_masks ? (const uint32_t *)s->d_node_masks.p : nullptr;
  a.point_masks = d_point_masks;
  a.out = d_out;
  a.found = d_found;
  a.spill = levels ? (uint32_t *)s->d_spill.p : nullptr;
  a.spill_stride = grid * 256u;
  a.cursor = (uint32_t *)s->d_cursor.p;
  a.num_parts = std::max(1u, std::min(8u, grid));
  a.refill_min = s->closest_refill_min;
  a.trav_min = s->closest_trav_min;
  a.counters = nullptr;
#ifdef NRT_PROF
  SCHK(s, nrt::devbuf_ensure(&s->d_counters, 16 * sizeof(unsigned long long))); // (nodes opened, instances entered, triangles tested: nrtSceneDebugCounters [0..2])
  SCHK(s, hipMemsetAsync(s->d_counters.p, 0, 16 * sizeof(unsigned long long), s->stream));
  a.counters = (unsigned long long *)s->d_counters.p;
#endif
  SCHK(s, nrt::launch_scene_closest_point(a, grid, s->stream));
  return NRT_OK;
}

// `device`: points / point_masks / closest_out / found_out are device pointers, whose alignment the kernel's loads and stores rely
// on; else the caller's host arrays, staged in pieces of kSceneClosestPiece points through the scene's grow-only buffers — the piece
// and its words up, the launch, its records and bytes back.  Either way the call returns with everything finished.
static nrt_status scene_closest(nrt_scene *s, const nrt_point_f32 *points, uint64_t n64, const uint32_t *point_masks, nrt_scene_closest_f32 *out,
                                uint8_t *found, bool device) {
  const char *what = device ? "nrtSceneClosestPointBatchDevice" : "nrtSceneClosestPointBatch";
  if (!s) return sfail(nullptr, NRT_ERR_INVALID, "%s: scene == NULL", what);
  if (!s->committed) return sfail(s, NRT_ERR_INVALID, "%s: commit the scene first", what);
  if (n64 == 0) return NRT_OK;
  if (!points || !out) return sfail(s, NRT_ERR_INVALID, "%s: NULL points/closest_out", what);
  if (n64 > 0x7FFFFFFFull) return sfail(s, NRT_ERR_INVALID, "%s: more than 2^31-1 points in one call", what);
  if (device && (((uintptr_t)points & 15u) != 0 || ((uintptr_t)out & 15u) != 0))
    return sfail(s, NRT_ERR_INVALID, "%s: the device arrays are not aligned to 16 bytes", what);
  if (device && ((uintptr_t)point_masks & 3u) != 0) return sfail(s, NRT_ERR_INVALID, "%s: d_point_masks is not 4-byte aligned", what);
  // (the instance table holds the mesh contexts' device addresses and stack depths as they were at Commit: scene_traverse)
  for (size_t m = 0; m < s->mesh_gens.size(); m++)
    if (nrt_internal_generation(s->mesh_gens[m].first) != s->mesh_gens[m].second)
      return sfail(s, NRT_ERR_INVALID, "%s: a mesh context was rebuilt, re-set or refitted since nrtSceneCommit (commit the scene again)", what);
  SCHK(s, hipSetDevice(s->device));
  if (point_masks) {
    const nrt_status st = upload_node_masks(s);
    if (st != NRT_OK) return st;
  }
  s->last_redone = 0;
  s->last_path = 2;
  if (device) {
    const nrt_status st = scene_closest_launch(s, points, (uint32_t)n64, point_masks, out, found);
    if (st != NRT_OK) return st;
    SCHK(s, hipStreamSynchronize(s->stream));
    return NRT_OK;
  }
  for (uint64_t off = 0; off < n64; off += kSceneClosestPiece) {
    const uint32_t m = (uint32_t)std::min(kSceneClosestPiece, n64 - off);
    SCHK(s, nrt::devbuf_ensure(&s->d_rays, (size_t)m * sizeof(nrt_point_f32)));
    SCHK(s, nrt::devbuf_ensure(&s->d_best, (size_t)m * sizeof(nrt_scene_closest_f32)));
    SCHK(s, nrt::devbuf_ensure(&s->d_mask, (size_t)m));
    if (point_masks) SCHK(s, nrt::devbuf_ensure(&s->d_ray_masks, (size_t)m * sizeof(uint32_t)));
    SCHK(s, hipMemcpyAsync(s->d_rays.p, points + off, (size_t)m * sizeof(nrt_point_f32), hipMemcpyHostToDevice, s->stream));
    if (point_masks) SCHK(s, hipMemcpyAsync(s->d_ray_masks.p, point_masks + off, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    const nrt_status st = scene_closest_launch(s, (const nrt_point_f32 *)s->d_rays.p, m, point_masks ? (const uint32_t *)s->d_ray_masks.p : nullptr,
                                               (nrt_scene_closest_f32 *)s->d_best.p, (uint8_t *)s->d_mask.p);
    if (st != NRT_OK) {
      (void)hipStreamSynchronize(s->stream);
      return st;
    }
    SCHK(s, hipMemcpyAsync(out + off, s->d_best.p, (size_t)m * sizeof(nrt_scene_closest_f32), hipMemcpyDeviceToHost, s->stream));
    if (found) SCHK(s, hipMemcpyAsync(found + off, s->d_mask.p, (size_t)m, hipMemcpyDeviceToHost, s->stream));
    SCHK(s, hipStreamSynchronize(s->stream));
  }
  return NRT_OK;
}

extern "C" {

nrt_status nrtSceneClosestPointBatch_f32(nrt_scene *s, const nrt_point_f32 *points, uint64_t n, const uint32_t *point_masks, nrt_scene_closest_f32 *out,
                                         uint8_t *found) {
  return scene_closest(s, points, n, point_masks, out, found, false);
}

nrt_status nrtSceneClosestPointBatchDevice_f32(nrt_scene *s, const nrt_point_f32 *d_points, uint64_t n, const uint32_t *d_point_masks,
                                               nrt_scene_closest_f32 *d_out, uint8_t *d_found) {
  return scene_closest(s, d_points, n, d_point_masks, d_out, d_found, true);
}

nrt_status nrtSceneOccludedBatch_f32(nrt_scene *s, const nrt_ray_f32 *rays, uint64_t n, uint8_t *mask_out) {
  return scene_occluded(s, rays, n, mask_out, false);
}

nrt_status nrtSceneOccludedBatchDevice_f32(nrt_scene *s, const nrt_ray_f32 *d_rays, uint64_t n, uint8_t *d_mask_out) {
  return scene_occluded(s, d_rays, n, d_mask_out, true);
}

nrt_status nrtSceneTraverseBatch_f32(nrt_scene *s, const nrt_ray_f32 *rays, uint64_t n, nrt_scene_hit_f32 *hits_out,
                                     uint8_t *mask_out) {
  return scene_traverse(s, rays, n, hits_out, mask_out, false);
}

nrt_status nrtSceneTraverseBatchDevice_f32(nrt_scene *s, const nrt_ray_f32 *d_rays, uint64_t n, nrt_scene_hit_f32 *d_hits_out,
                                           uint8_t *d_mask_out) {
  return scene_traverse(s, d_rays, n, d_hits_out, d_mask_out, true);
}

// The masked queries: the four calls above with one visibility word per ray (include/nanort_hip.h).
nrt_status nrtSceneTraverseBatchMasked_f32(nrt_scene *s, const nrt_ray_f32 *rays, const uint32_t *ray_masks, uint64_t n, nrt_scene_hit_f32 *hits_out,
                                           uint8_t *mask_out) {
  return scene_traverse(s, rays, n, hits_out, mask_out, false, false, true, ray_masks);
}

nrt_status nrtSceneTraverseBatchMaskedDevice_f32(nrt_scene *s, const nrt_ray_f32 *d_rays, const uint32_t *d_ray_masks, uint64_t n,
                                                 nrt_scene_hit_f32 *d_hits_out, uint8_t *d_mask_out) {
  return scene_traverse(s, d_rays, n, d_hits_out, d_mask_out, true, false, true, d_ray_masks);
}

nrt_status nrtSceneOccludedBatchMasked_f32(nrt_scene *s, const nrt_ray_f32 *rays, const uint32_t *ray_masks, uint64_t n, uint8_t *mask_out) {
  return scene_traverse(s, rays, n, nullptr, mask_out, false, true, true, ray_masks);
}

nrt_status nrtSceneOccludedBatchMaskedDevice_f32(nrt_scene *s, const nrt_ray_f32 *d_rays, const uint32_t *d_ray_masks, uint64_t n, uint8_t *d_mask_out) {
  return scene_traverse(s, d_rays, n, nullptr, d_mask_out, true, true, true, d_ray_masks);
}

// One descriptor for the scene queries (include/nanort_hip.h).  Without SKIP, or with SKIP and no pair array, the descriptor IS one of
// the eight calls above: the same arguments reach scene_traverse.  The unmasked kinds do not read ray_masks, the OCCLUSION kinds do not
// read hits_out.
static nrt_status scene_query(nrt_scene *s, const nrt_scene_query_f32 *q, bool device) {
  const char *what = device ? "nrtSceneQueryBatchDevice" : "nrtSceneQueryBatch";
  if (!s) return sfail(nullptr, NRT_ERR_INVALID, "%s: scene == NULL", what);
  if (!q) return sfail(s, NRT_ERR_INVALID, "%s: descriptor == NULL", what);
  if (q->struct_size != sizeof(nrt_scene_query_f32))
    return sfail(s, NRT_ERR_INVALID, "%s: struct_size = %u, this library's nrt_scene_query_f32 has %zu bytes", what, q->struct_size, sizeof(nrt_scene_query_f32));
  if (q->flags & ~(uint32_t)(NRT_SCENE_QUERY_OCCLUSION | NRT_SCENE_QUERY_MASKED | NRT_SCENE_QUERY_SKIP))
    return sfail(s, NRT_ERR_INVALID, "%s: unknown flag bits 0x%x", what, q->flags);
  if (q->reserved != 0) return sfail(s, NRT_ERR_INVALID, "%s: reserved = %u (must be 0)", what, q->reserved);
  const bool occluded = (q->flags & NRT_SCENE_QUERY_OCCLUSION) != 0, masked = (q->flags & NRT_SCENE_QUERY_MASKED) != 0;
  const void *pairs = (q->flags & NRT_SCENE_QUERY_SKIP) ? q->skip_pairs : nullptr;
  return scene_traverse(s, q->rays, q->num_rays, occluded ? nullptr : q->hits_out, q->mask_out, device, occluded, masked,
                        masked ? q->ray_masks : nullptr, pairs, pairs ? q->skip_stride_bytes : 0u, true);
}

nrt_status nrtSceneQueryBatch_f32(nrt_scene *s, const nrt_scene_query_f32 *q) { return scene_query(s, q, false); }
nrt_status nrtSceneQueryBatchDevice_f32(nrt_scene *s, const nrt_scene_query_f32 *q) { return scene_query(s, q, true); }

nrt_status nrtSceneSetTunable(nrt_scene *s, const char *name, int value) {
  if (!s || !name) return NRT_ERR_INVALID;
  const std::string k(name);
  const unsigned lanes = (unsigned)std::min(64, std::max(1, value));
  if (k == "single_pass") s->single_pass = (unsigned)std::min(2, std::max(0, value));
  else if (k == "trav_min") s->trav_min = lanes;
  else if (k == "refill_min") s->refill_min = lanes;
  else if (k == "walk_trav_min") s->walk_trav_min = lanes;
  else if (k == "walk_leaf_items") s->walk_leaf_items = value ? 1u : 0u;
  else if (k == "walk_refill_min") s->walk_refill_min = lanes;
  else if (k == "cand_min") s->cand_min = lanes;
  else if (k == "cand_busy_max") s->cand_busy_max = (unsigned)std::min(65, std::max(1, value));
  else if (k == "fuse_scan") s->fuse_scan = value != 0;
  else if (k == "scan_max") s->scan_max = (unsigned)std::min(kMaxList, std::max(1, value));
  else if (k == "prune_min") s->prune_min = (unsigned)std::max(0, value);
  else if (k == "walk_min") s->walk_min = (unsigned)std::max(2, value);
  else if (k == "walk_backoff_pct") s->walk_backoff_pct = (unsigned)std::min(100, std::max(0, value));
#ifdef NRT_PROF
  else if (k == "count_loops") s->count_loops = value != 0;
#endif
  else return sfail(s, NRT_ERR_INVALID, "nrtSceneSetTunable: unknown tunable '%s'", name);
  return NRT_OK;
}

uint64_t nrtSceneLastRedone(const nrt_scene *s) { return s ? s->last_redone : 0; }
int nrtSceneLastPath(const nrt_scene *s) { return s ? s->last_path : 0; }

#ifdef NRT_PROF // libnanort_hip_prof.so only (include/nanort_hip_prof.h)
int nrtSceneDebugCounters(nrt_scene *s, unsigned long long *out, int cap) {
  if (!s || !out || cap < 16 || !s->d_counters.p) return 1;
  if (hipStreamSynchronize(s->stream) != hipSuccess) return 1;
  return hipMemcpy(out, s->d_counters.p, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
}
#endif

} // extern "C"
