// nanort_amd/csrc/ctx.h — the context behind the C ABI of libnanort_hip.so (include/nanort_hip.h): its state, its error channel
// and its waits.  Host only, and for the four api_*.hip units alone — api_ctx (life cycle, tunables, timing), api_geometry (the
// setters), api_tree (build, adoption, refit), api_query (every ray query); scene.hip, group.hip and embree_api.cc reach a context
// through the accessors of kernels.h.
//
// One nrt_ctx == one reference BVHAccel<T> (nanort.h:698-860) resident on one
// MI355X: mesh, node array, index permutation and the leaf-ordered triangle
// records live in HBM for the lifetime of the context; the host entry points
// stage rays/hits through grow-only device buffers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ctype.h>
#include <math.h>
#include <cmath>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "kernels.h"
#include "launch_plan.h"
#ifdef NRT_PROF
#include "../../include/nanort_hip_prof.h"
#endif

using namespace nrt;

inline thread_local std::string g_create_error; // why the calling thread's last nrtCreate / nrtHostAlloc failed (nrtLastError(NULL))

// The kernel a traversal launch runs (api_query.hip, choose_walk): k_traverse, k_traverse_wide of WIDTH 2 / 4, or one of own_walks.hip's.
enum class Walk { Literal, OneLevel, TwoLevel, Own };

struct nrt_ctx {
  int device = 0;
  hipStream_t stream = nullptr; // internal stream for host entry points / build
  std::string err;
  int prec = 0; // 0 unset, 4 = f32, 8 = f64
  int num_cus = 256;

  // mesh (tight xyz in HBM)
  int prim_kind = kPrimTriangles; // kPrimSpheres: d_verts = centres, d_radii = radii, no faces; kPrimCylinders: d_verts = 2 end points, d_radii = 2 radii per primitive; kPrimCurves: d_verts = 4 control points, d_radii = 4 radii per primitive
  uint32_t cyl_test_cap = 1;
  uint32_t curve_subdiv = 4; // curves: line segments per curve (the intersector's num_subdivisions; nrtSetCurves)
  // cylinders cut into segments for the builder (prims.hip k_cylinder_segments): what the tree is built over when num_segs != 0
  DevBuf b_seg_verts, b_seg_radii, b_seg_prim, b_seg_off;
  uint32_t num_segs = 0;
  int cyl_split = 32;     // most segments a cylinder is cut into (tunable "cyl_split"; 1: never; read by nrtSetCylinders)
  int cyl_seg_radii = 8;  // ... one per this many tube radii of its length (tunable "cyl_seg_radii")
  DevBuf b_verts, b_radii, b_faces; // grow-only: a per-frame SetMesh allocates nothing in the steady state
  void *d_verts = nullptr;          // == b_verts.p while primitives are set
  void *d_radii = nullptr;
  uint32_t *d_faces = nullptr;
  uint32_t num_faces = 0, num_verts = 0;
  // nrtSetMeshDevice (prims.hip): the largest face index, reduced on the device and read back through a page-locked word
  DevBuf b_max_index;
  uint32_t *h_max_index = nullptr;

  // tree (grow-only buffers: a per-frame rebuild allocates nothing in the steady state)
  DevBuf b_nodes, b_indices, b_tris, b_wide, b_wide4, b_wide_scratch, b_build_ws;
  void *d_nodes = nullptr;       // == b_nodes.p while a tree is present
  uint32_t *d_indices = nullptr; // == b_indices.p
  void *d_tris = nullptr;        // LeafTri<T>[num_indices] == b_tris.p
  void *d_wide = nullptr;        // WideNode<T>[branches]   == b_wide.p
  void *d_wide4 = nullptr;       // Wide4Node<T>[branches]  == b_wide4.p (triangle trees only, and only when wide4 is on)
  uint32_t num_branch_records = 0; // nodes with flag == 0 in the node array (reachable or not)
  uint64_t num_nodes = 0, num_indices = 0;
  uint32_t tree_depth = 0;
  uint32_t max_leaf_count = 0, min_leaf_count = 0; // over the leaves of the current tree
  uint32_t packed_leaves = 0;
  uint32_t root_is_branch = 0; // node 0 has flag == 0
  uint32_t tree_nested = 1;    // every child box lies inside its parent's (always true of trees built here; checked for adopted ones)
  nrt_build_stats stats = {0, 0, 0, 0.f};
  uint64_t generation = 0; // bumped whenever the tree or the primitives are replaced (free_tree) or refit
  // refit (refit.hip): the level plan of the current tree, built on the device by the first refit after the tree changed
  DevBuf b_refit_plan, b_refit_stage; // (stage: the host form's upload of the caller's vertex block)
  bool refit_planned = false;
  // a Device refit enqueued on a caller's stream: every later traversal launch waits for ev_refit on the device until the
  // host sees it complete, every host-side reader of the tree (nrtGetTree, a rebuild, a scene commit) waits for it on the host
  hipEvent_t ev_refit = nullptr;
  bool refit_pending = false;

  // traversal scratch.  Every launch owns one LaunchSlot (work cursors + overflow stacks) until it
  // completes, so launches issued on different streams may overlap on the GPU: the drain tail of one
  // batch is filled by the start of the next.  Launches on one stream keep reusing one slot.
  struct LaunchSlot {
    uint32_t *d_cursor = nullptr; // two sets of ray cursors (one per partition, 4 KiB apart): a launch uses one and zeroes the other
    unsigned parity = 0;
    DevBuf spill, spill_tmin;
    DevBuf cyl_hits, cyl_bits;    // cylinder / curve kinds: compact records + {hit, cap} bits between the traversal and its post pass
    hipEvent_t done = nullptr;    // recorded after the slot's last launch (launches that do not publish a completion record)
    hipEvent_t t0 = nullptr, t1 = nullptr; // event timing of the slot's last launch (per slot: launches on different streams overlap)
    hipStream_t stream = nullptr; // stream of that launch
    bool used = false;
    // completion record (common.h, DoneRec): page-locked, written by the last wave of a launch — no event in the stream
    DoneRec *h_done = nullptr, *d_done = nullptr; // host / device address of the same record
    DoneCount *d_count = nullptr;                 // the device words that go with it
    uint32_t seq = 0;             // sequence number of the slot's last launch that publishes a record
    bool rec_pending = false;     // the slot's last launch publishes a record and nobody has seen it complete yet
    bool last_has_rec = false;    // the slot's last launch publishes a record (nrtLastTraverseMs reads its stamps)
    bool last_timed = false;      // ... or was bracketed by the t0 / t1 events
  };
  static constexpr int kSlots = 4;
  LaunchSlot slots[kSlots];
  unsigned next_victim = 0;
  std::mutex launch_mutex; // slot selection + launch (nrtTraverseBatchDevice may be called from several host threads)
  std::mutex host_mutex;   // the host-buffer traversal calls share one set of staging buffers: one at a time
  unsigned long long *d_counters = nullptr;  // 16 x u64 (counting pass / profiling instantiation only)
  DevBuf st_rays, st_hits, st_mask;
  DevBuf st_skip; // per-ray skip ids of the staged host forms, beside st_rays
  // host entry point with page-locked caller buffers: upload / trace / download pipelined over three streams
  hipStream_t copy_in = nullptr, copy_out = nullptr;
  hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_tr[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
  int host_pipeline = 1; // (env NRT_HOST_PIPELINE=0: one upload, one launch, one download)
  DevBuf b_wave_clock; // profiling (NRT_DEBUG bit 8192)
  uint32_t wave_clock_waves = 0;

  // traversal tuning (env NRT_LDS_STACK / NRT_REFILL_MIN / NRT_TRAV_MIN / NRT_CHUNK override)
  int lds_stack = kLdsStackDefault;
  unsigned chunk = 128, chunk_tail_pct = 0, refill_min = 44, trav_min = 16, leaf_min = 32; // (trav_min: 8 until round 3; 12-14 was the optimum of the two-level walk before its inner loop ran two rounds per trip, profiles/r03t_trav_min.txt; 16 with two rounds per trip in the fp64 walk, profiles/r03ZA)
  int f64_row_fetch = 1; // fp64 walk: fetch the plane rows of a WideNode<double> by the ray's signs (0: fetch the record and select; the path arrays of 4 GiB and more take)
  unsigned tail_quad = 4; // traverse.hip "four lanes to a ray": live lanes of a wave that is out of rays at or below which it finishes them a quad per ray (0: never; records bit-identical at every value).  4 was the smallest threshold whose slowest bench run beat the library before the tail (C3 +2.5 %; 8: +3.5 %, 16: +5 %), measured while the tail stood inside the walk's loop and cost every launch 2.3 % in registers: profiles/r07a_tail_quad.txt.  The tail stands behind the loop now (84 VGPRs, as without it: profiles/r07b_tail_behind_loop.txt).  The sweep that r07b owed, in that library (profiles/r12a_tail_rows.txt, C3 ms per step): 0: 0.599, 2: 0.585, 4: 0.574, 8: 0.565, 12: 0.563, 16: 0.562 — monotone, 16 is 2.2 % ahead of 4.  The default stays 4 all the same: it is the value tests/test_gpu_tail_quad_default.py pins, and moving it is a change of its own, with the other configs measured at 16
  unsigned trav_min4 = 24; // the same threshold for the fp32 two-level walk, whose inner loop runs two pop + step rounds per trip (profiles/r03Z_threshold_resweep*.txt)
  unsigned num_parts = 8; // ray partitions == XCDs (env NRT_PARTS)
  unsigned debug_flags = 0;
  int subtree_rows = 1; // builder: subtree phase in row form (up to four nodes per step); 0 (profiling build only): one node per step — same tree, the cross-check (tests/test_gpu_build.py)
  int morton = 0; // Morton-order the primitive records before the build (env NRT_MORTON=1): measured +0.4 ms at 1M tris for an identical tree, so off by default
  // share of a batch handed out statically, percent (tunable static_pct).  75 until the end of round 6; 16 since: with ~400 rays per
  // wave (a 1080p wave on this grid) a wave's static share was 256 of them, and whenever the cost per ray is uneven over the image
  // (C2: 40 % sky) the waves with cheap slices drained the dynamic rest while the others were still on rays nobody could take from
  // them.  One 64-ray group per wave there (it starts every wave without an atomic) and the rest claimed in chunks:
  // C3 +2.8 %, C2 +7 %, C4 tile +2.9 %, C5 +0.9 %, a 2560x1440 view of C2's mesh +17 %; balanced frames of other sizes -3.3 ... +1 %
  // (profiles/r06y_distribution_*.txt)
  unsigned static_pct = 16;
  unsigned static_bands = 8; // ... as up to this many slices per wave, one in each band of the batch
  unsigned static_slice_groups = 2; // ... each of at least this many 64-ray groups
  unsigned max_blocks_per_cu = 0; // env NRT_BLOCKS_PER_CU caps the persistent grid
  int wide = 1, wide_stack = 10; // production path: WideNode kernel (env NRT_WIDE=0 selects the binary kernel)
  // Two tree levels per step (Wide4Node records, walk_dev.h NRT_STEP_NODE4): the production walk of fp32 triangle trees
  // whose child boxes lie inside their parents'.  env NRT_WIDE4=0 goes back to one level per step.
  int wide4 = 1;
  int wide4_big_ok = 1; // ... also when the record array reaches 4 GiB (tunable wide4_big; 0: such trees walk one level per step, as until round 6)
  // two-level walk, order of a record's four slots.  0 (default since round 5): the binary loop's order — the same leaves in the
  // same order as nanort.h:2526-2548, every field of every record bit-identical to the reference on the same node array.
  // 1 (opt-in): by entry distance, +2...5 % — the closest t is the reference's except where a leaf box's entry distance rounds
  // above a hit inside it, and among primitives at exactly the same t another one may be named (contract-level parity)
  int order4 = 0;
  int leaf_compact = 1; // walk_dev.h "leaf items" (leaf_items_one_trip, round 6): when the records of all the lanes waiting at a leaf fit one trip of the wave, they are tested one per lane with the owner's ray constants and accepted by the owner in record order — records bit-identical, C3 +2 %, C4 tile +2.8 %; 0: every owner tests its own records
  int dyn_head = 1; // batches too small for a static group per wave: every wave's first chunk is its own (traverse.hip claim_init; tunable dyn_head)
  int wide_scramble = 0; // probe (tunable wide_scramble): the private node records in a pseudo-random order instead of pre-order
  // resident blocks per CU of the variants launched so far, by what selects the kernel: [walk][primitive kind] at `lds_entries` (a context
  // keeps one precision; api_query.hip, size_grid).  A row per Walk, the own walks' rows (kernels.h, OwnWalk) in the place of Walk::Own's.
  struct { int lds_entries; unsigned blocks_per_cu; } occupancy[(int)Walk::Own + kNumOwnWalks][kNumPrimKinds] = {};

  unsigned closest_blocks_per_cu = 0; // ... and of k_closest_point (closest.hip; 0: not asked for yet)
  unsigned signed_blocks_per_cu = 0;  // ... and of k_signed_distance
  unsigned nearest_blocks_per_cu = 0; // ... and of k_nearest_faces (nearest.hip)

  hipEvent_t ev_b0 = nullptr, ev_b1 = nullptr;
  hipEvent_t ev_build_state = nullptr; // the builder's state block has reached build_state
  void *build_state = nullptr;         // page-locked, kBuildPinnedBytes
  int last_timed_slot = -1; // slot of the most recent timed traversal launch (nrtLastTraverseMs)
  int launch_timing = 0;    // 1: bracket every traversal launch with timing events and follow it with a completion event (nrtSetLaunchTiming); 0: completion records
  bool have_build_time = false;
  float segment_ms = 0.f; // cylinders: wall time nrtSetCylinders spent cutting them into segments (counted into the next build's time)
  const char *last_kernel = ""; // variant of the most recent traversal launch (nrtLastKernelName)

  // motion blur (nrtSetMeshMotion*): the second vertex keyframe of a triangle mesh (tight xyz, num_verts rows) and,
  // while a tree is present, its LeafTri<T> records in leaf order beside d_tris
  DevBuf b_verts1, b_tris1, st_times; // (st_times: per-ray times of the staged host forms, beside st_rays)
  void *d_verts1 = nullptr; // == b_verts1.p while a keyframe is set
  void *d_tris1 = nullptr;  // == b_tris1.p while a keyframe and a tree are present

  // visibility masks (nrtSetPrimMasks*): one word per face in face order, and the same words in leaf order beside
  // d_tris (prims.hip, k_permute_masks).  leaf_masks_stale: b_leaf_masks is not the permutation of b_prim_masks by the current
  // leaf order.  Set by the two events that can make it so — the setter (new words) and free_tree (every path to a new leaf order
  // passes it: nrtBuild, nrtSetTree, the mesh and keyframe setters; a refit rewrites d_tris in the same order and leaves it) —
  // and cleared by the one place that derives the array, the first masked query behind them (api_query.hip, refresh_leaf_masks).
  DevBuf b_prim_masks, b_leaf_masks, st_ray_masks; // (st_ray_masks: per-ray words of the staged host forms, beside st_rays)
  uint32_t *d_prim_masks = nullptr; // == b_prim_masks.p while masks are set
  bool leaf_masks_stale = true;

  // signed distance (nrtSignedDistanceBatch*): the pseudonormals of the triangle mesh (sdf.hip) — per face its unit
  // normal and its three edge normals [num_faces][4][3], per vertex the angle-weighted normal [num_verts][3] — and the workspace of
  // their derivation.  They belong to the MESH, not to the tree.  feature_normals_stale: the buffers do not hold the normals of
  // d_verts / d_faces.  Set by the events that change the mesh — every triangle mesh setter (free_mesh: all of them pass it) and
  // every triangle refit, host and Device forms — and not by nrtBuild, nrtSetTree, the mask setters or the second keyframe's
  // setter; cleared by the one place that derives them, the first signed query or nrtGetFeatureNormals behind the change
  // (api_query.hip, refresh_feature_normals).
  DevBuf b_face_normals, b_vertex_normals, b_sdf_ws;
  bool feature_normals_stale = true;
};

inline nrt_status fail(nrt_ctx *c, nrt_status st, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c)
    c->err = buf;
  else
    g_create_error = buf;
  return st;
}

#define HIPCHK(c, call)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail((c), NRT_ERR_DEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                  __FILE__, __LINE__);                                                    \
  } while (0)

inline nrt_status ensure(nrt_ctx *c, DevBuf &b, size_t bytes) {
  HIPCHK(c, devbuf_ensure(&b, bytes));
  return NRT_OK;
}

// Every call that rewrites the tree or the primitive buffers in place (nrtSetMesh / nrtSetSpheres / nrtSetCylinders /
// nrtSetTree / nrtBuild) first waits for the traversal launches still in flight on the CALLER's streams: they read
// b_nodes / b_tris / b_wide, which the rebuild reuses without reallocating (a per-frame "trace asynchronously on my
// stream, then rebuild" loop is therefore safe without a synchronisation of the caller's own).
// Event records between two kernels of a stream keep the second from starting for several microseconds each (measured:
// the three records per launch — a timing pair and the slot's `done` — held C3 at 24 us of idle time per launch).  So the
// triangle launches of the production kernel record NONE by default: the kernel's last wave publishes a completion record
// (sequence number + start / end stamps) in page-locked memory, and whoever has to wait for the launch — a rebuild, destroy,
// another stream taking the slot over, nrtLastTraverseMs — polls that record: precise, and nothing else on the device is
// waited for.  (Sphere and cylinder launches: their post pass closes the record.  The literal kernel keeps the events.)
inline hipError_t wait_record(nrt_ctx::LaunchSlot &sl) {
  if (!sl.rec_pending) return hipSuccess;
  volatile uint32_t *seq = &sl.h_done->seq;
  const auto t_start = std::chrono::steady_clock::now();
  for (unsigned long spins = 0; *seq != sl.seq; spins++) {
    if (spins < 4000) continue; // (a launch lasts a fraction of a millisecond)
    std::this_thread::sleep_for(std::chrono::microseconds(20));
    if ((spins & 1023) == 0 && std::chrono::steady_clock::now() - t_start > std::chrono::seconds(30)) {
      // something is wrong (a faulted launch never writes its record): let the runtime report it
      hipError_t e = hipDeviceSynchronize();
      if (e != hipSuccess) return e;
      if (*seq != sl.seq) return hipErrorUnknown;
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  sl.rec_pending = false;
  return hipSuccess;
}

// The slot's last launch is over (host-side wait).
inline hipError_t slot_done(nrt_ctx *c, nrt_ctx::LaunchSlot &sl) {
  (void)c;
  if (!sl.used) return hipSuccess;
  if (sl.last_has_rec) return wait_record(sl);
  return sl.done ? hipEventSynchronize(sl.done) : hipSuccess;
}

// The host waits for a Device refit still in flight (before anything reads or rewrites the tree on the host's behalf).
inline hipError_t refit_host_wait_locked(nrt_ctx *c) { // (caller holds launch_mutex)
  if (!c->refit_pending) return hipSuccess;
  hipError_t e = hipEventSynchronize(c->ev_refit);
  if (e != hipSuccess) return e;
  c->refit_pending = false;
  return hipSuccess;
}
inline hipError_t refit_host_wait(nrt_ctx *c) {
  std::lock_guard<std::mutex> lock(c->launch_mutex);
  return refit_host_wait_locked(c);
}

// A traversal launch on stream `s` is ordered after a Device refit in flight (under launch_mutex).  Every launch waits on the
// event until the host sees it complete — not once per stream handle: a destroyed stream's handle may come back as a new
// stream that has never waited.  (A wait on the same stream again costs one barrier packet.)
inline hipError_t refit_stream_wait(nrt_ctx *c, hipStream_t s) {
  if (!c->refit_pending) return hipSuccess;
  const hipError_t q = hipEventQuery(c->ev_refit);
  if (q == hipSuccess) { // (complete: nobody has to wait any more)
    c->refit_pending = false;
    return hipSuccess;
  }
  if (q != hipErrorNotReady) return q;
  return hipStreamWaitEvent(s, c->ev_refit, 0);
}

inline hipError_t wait_for_launches(nrt_ctx *c) {
  std::lock_guard<std::mutex> lock(c->launch_mutex);
  hipError_t re = refit_host_wait_locked(c);
  if (re != hipSuccess) return re;
  for (nrt_ctx::LaunchSlot &sl : c->slots) {
    hipError_t e = slot_done(c, sl);
    if (e != hipSuccess) return e;
  }
  return hipStreamSynchronize(c->stream);
}

// Forget the current tree (the buffers stay allocated for the next one).
inline void free_tree(nrt_ctx *c) {
  c->generation++; // whoever cached device addresses / flags of the old tree (a committed nrt_scene) can tell
  c->d_wide = nullptr;
  c->d_wide4 = nullptr;
  c->d_nodes = nullptr;
  c->d_indices = nullptr;
  c->d_tris = nullptr;
  c->d_tris1 = nullptr;
  c->leaf_masks_stale = true; // (whatever tree comes next has a leaf order of its own)
  c->num_nodes = c->num_indices = 0;
  c->tree_depth = 0;
  c->refit_planned = false;
}

inline void free_mesh(nrt_ctx *c) {
  c->d_verts = nullptr; // (the buffers stay allocated for the next primitives)
  c->d_faces = nullptr;
  c->d_radii = nullptr;
  c->d_verts1 = nullptr; // (the motion keyframe goes with the mesh it belongs to)
  c->d_prim_masks = nullptr; // (... and so do the visibility masks)
  c->feature_normals_stale = true; // (... and so do the pseudonormals of the signed distance query)
  c->num_faces = c->num_verts = 0;
  c->num_segs = 0;
}
