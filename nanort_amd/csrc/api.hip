// nanort_amd/csrc/api.hip — the C ABI of libnanort_hip.so (include/nanort_hip.h).
//
// One nrt_ctx == one reference BVHAccel<T> (nanort.h:698-860) resident on one
// MI355X: mesh, node array, index permutation and the leaf-ordered triangle
// records live in HBM for the lifetime of the context; the host entry points
// stage rays/hits through grow-only device buffers.
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

static thread_local std::string g_create_error;

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
  // resident blocks per CU of the variants launched so far, by what selects the kernel: [walk][primitive kind] at `lds_entries` (a context keeps one precision; size_grid)
  struct { int lds_entries; unsigned blocks_per_cu; } occupancy[5][kNumPrimKinds] = {};

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
};

static nrt_status fail(nrt_ctx *c, nrt_status st, const char *fmt, ...) {
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

static nrt_status ensure(nrt_ctx *c, DevBuf &b, size_t bytes) {
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
static hipError_t wait_record(nrt_ctx::LaunchSlot &sl) {
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
static hipError_t slot_done(nrt_ctx *c, nrt_ctx::LaunchSlot &sl) {
  (void)c;
  if (!sl.used) return hipSuccess;
  if (sl.last_has_rec) return wait_record(sl);
  return sl.done ? hipEventSynchronize(sl.done) : hipSuccess;
}

// The host waits for a Device refit still in flight (before anything reads or rewrites the tree on the host's behalf).
static hipError_t refit_host_wait_locked(nrt_ctx *c) { // (caller holds launch_mutex)
  if (!c->refit_pending) return hipSuccess;
  hipError_t e = hipEventSynchronize(c->ev_refit);
  if (e != hipSuccess) return e;
  c->refit_pending = false;
  return hipSuccess;
}
static hipError_t refit_host_wait(nrt_ctx *c) {
  std::lock_guard<std::mutex> lock(c->launch_mutex);
  return refit_host_wait_locked(c);
}

// A traversal launch on stream `s` is ordered after a Device refit in flight (under launch_mutex).  Every launch waits on the
// event until the host sees it complete — not once per stream handle: a destroyed stream's handle may come back as a new
// stream that has never waited.  (A wait on the same stream again costs one barrier packet.)
static hipError_t refit_stream_wait(nrt_ctx *c, hipStream_t s) {
  if (!c->refit_pending) return hipSuccess;
  const hipError_t q = hipEventQuery(c->ev_refit);
  if (q == hipSuccess) { // (complete: nobody has to wait any more)
    c->refit_pending = false;
    return hipSuccess;
  }
  if (q != hipErrorNotReady) return q;
  return hipStreamWaitEvent(s, c->ev_refit, 0);
}

static hipError_t wait_for_launches(nrt_ctx *c) {
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
static void free_tree(nrt_ctx *c) {
  c->generation++; // whoever cached device addresses / flags of the old tree (a committed nrt_scene) can tell
  c->d_wide = nullptr;
  c->d_wide4 = nullptr;
  c->d_nodes = nullptr;
  c->d_indices = nullptr;
  c->d_tris = nullptr;
  c->d_tris1 = nullptr;
  c->num_nodes = c->num_indices = 0;
  c->tree_depth = 0;
  c->refit_planned = false;
}

static void free_mesh(nrt_ctx *c) {
  c->d_verts = nullptr; // (the buffers stay allocated for the next primitives)
  c->d_faces = nullptr;
  c->d_radii = nullptr;
  c->d_verts1 = nullptr; // (the motion keyframe goes with the mesh it belongs to)
  c->num_faces = c->num_verts = 0;
  c->num_segs = 0;
}

// ---------------------------------------------------------------------------
// Tunables (nrtSetTunable / nrtGetTunable; the environment variable NRT_<NAME> overrides the default at nrtCreate).
// ---------------------------------------------------------------------------
struct TunableDesc {
  const char *name;
  long long lo, hi;
  long long (*get)(const nrt_ctx *);
  void (*set)(nrt_ctx *, long long);
};
#define NRT_TUNABLE(name_, lo_, hi_, field_, type_)                                                          \
  {name_, lo_, hi_, [](const nrt_ctx *c) -> long long { return (long long)c->field_; },                      \
   [](nrt_ctx *c, long long v) { c->field_ = (type_)v; }}
static const TunableDesc kTunables[] = {
    NRT_TUNABLE("refill_min", 1, 64, refill_min, unsigned),       // idle lanes of a wave before it claims more rays
    NRT_TUNABLE("trav_min", 1, 64, trav_min, unsigned),           // lanes still walking below which the inner-node phase ends (one level per step)
    NRT_TUNABLE("trav_min4", 1, 64, trav_min4, unsigned),         // ... of the two-level walk
    NRT_TUNABLE("f64_row_fetch", 0, 1, f64_row_fetch, int),       // 0: the fp64 walk reads whole WideNode records and selects the planes (what arrays >= 4 GiB do)
    NRT_TUNABLE("leaf_min", 1, 64, leaf_min, unsigned),           // lanes at a leaf below which a due refill goes first
    NRT_TUNABLE("chunk_tail_pct", 0, 100, chunk_tail_pct, unsigned), // share of the dynamic rays handed out in half chunks (the end of a launch)
    NRT_TUNABLE("parts", 1, kMaxParts, num_parts, unsigned),      // ray partitions (== XCDs)
    NRT_TUNABLE("static_pct", 0, 100, static_pct, unsigned),      // share of a batch owned statically, percent
    NRT_TUNABLE("static_bands", 1, 64, static_bands, unsigned),   // ... in up to this many slices per wave, one per band
    NRT_TUNABLE("static_slice_groups", 1, 64, static_slice_groups, unsigned), // ... of at least this many 64-ray groups each
    NRT_TUNABLE("blocks_per_cu", 0, 8, max_blocks_per_cu, unsigned), // cap on the persistent grid (0: occupancy)
    NRT_TUNABLE("debug", 0, 0x7FFFFFFF, debug_flags, unsigned),   // profiling bit mask
    NRT_TUNABLE("morton", 0, 1, morton, int),                     // Morton pre-pass of the builder (next build)
    NRT_TUNABLE("cyl_split", 1, 64, cyl_split, int),              // cylinders: most segments one is cut into for the builder (1: never; next nrtSetCylinders)
    NRT_TUNABLE("cyl_seg_radii", 1, 1024, cyl_seg_radii, int),    // ... one segment per this many tube radii of length (next nrtSetCylinders)
#ifdef NRT_PROF
    NRT_TUNABLE("subtree_rows", 0, 1, subtree_rows, int),         // 0: the builder's one-node-per-step subtree kernel (next build; same tree) — libnanort_hip_prof.so only
#endif
    NRT_TUNABLE("wide", 0, 1, wide, int),                         // 0: the literal BVHNode loop
    NRT_TUNABLE("wide4_big", 0, 2, wide4_big_ok, int),            // ... also for record arrays of 4 GiB and more (64-bit offsets; next build / set_tree); 2: 64-bit offsets whatever the size (tests)
    NRT_TUNABLE("wide4", 0, 1, wide4, int),                       // two tree levels per step (next build / set_tree)
    NRT_TUNABLE("leaf_compact", 0, 1, leaf_compact, int),         // two-level walk, triangle trees with leaves of <= 4 records: leaf phase over items (records bit-identical)
    NRT_TUNABLE("tail_quad", 0, 16, tail_quad, unsigned),         // two-level triangle walk: a wave out of rays with at most this many live lanes finishes them four lanes to a ray (0: never; records bit-identical)
    NRT_TUNABLE("dyn_head", 0, 1, dyn_head, int),                 // a batch without a static share: a wave's first chunk without an atomic
    NRT_TUNABLE("order4", 0, 1, order4, int),                     // two-level walk: 0 (default) = the reference's order, every field bit-identical; 1 = slots by entry distance (faster; contract-level parity at ties)
    NRT_TUNABLE("launch_timing", 0, 1, launch_timing, int),       // == nrtSetLaunchTiming
    NRT_TUNABLE("host_pipeline", 0, 1, host_pipeline, int),       // pipelined host entry point
    NRT_TUNABLE("wide_scramble", 0, 1, wide_scramble, int),       // probe: WideNode / Wide4Node records in a pseudo-random order (next build)
    {"chunk", 32, 1 << 20, [](const nrt_ctx *c) -> long long { return c->chunk; },
     [](nrt_ctx *c, long long v) { c->chunk = (unsigned)(v / 32) * 32u; }}, // rays claimed per atomic (whole and half chunks are multiples of 16)
    {"lds_stack", 16, 32, [](const nrt_ctx *c) -> long long { return c->lds_stack; },
     [](nrt_ctx *c, long long v) { if (v == 16 || v == 24 || v == 32) c->lds_stack = (int)v; }},
    {"wide_stack", 8, 16, [](const nrt_ctx *c) -> long long { return c->wide_stack; },
     [](nrt_ctx *c, long long v) { if (v == 8 || v == 10 || v == 12 || v == 16) c->wide_stack = (int)v; }},
};
#undef NRT_TUNABLE

static const TunableDesc *tunable_find(const char *name) {
  if (!name) return nullptr;
  for (const TunableDesc &d : kTunables)
    if (!strcmp(d.name, name)) return &d;
  return nullptr;
}
static bool tunable_set(nrt_ctx *c, const char *name, long long v) {
  const TunableDesc *d = tunable_find(name);
  if (!d) return false;
  d->set(c, std::min(d->hi, std::max(d->lo, v)));
  memset(c->occupancy, 0, sizeof(c->occupancy)); // the figures depend on the variant the tunables select: ask again on the next launch
  return true;
}

extern "C" {

const char *nrtVersion(void) { return "libnanort_hip 0.1 (gfx950, HIP)"; }

// Page-locked host memory for ray / hit buffers handed to the host entry points: the copies then run at PCIe speed
// (pageable memory is staged by the runtime at roughly half of it) — for callers that do not link HIP themselves.
nrt_status nrtHostAlloc(size_t bytes, void **out) {
  if (!out) return fail(nullptr, NRT_ERR_INVALID, "nrtHostAlloc: out == NULL");
  *out = nullptr;
  if (bytes == 0) return NRT_OK;
  const hipError_t e = hipHostMalloc(out, bytes, hipHostMallocPortable);
  if (e != hipSuccess) {
    *out = nullptr;
    return fail(nullptr, NRT_ERR_DEVICE, "nrtHostAlloc: hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  }
  return NRT_OK;
}
void nrtHostFree(void *p) {
  if (p) (void)hipHostFree(p);
}

nrt_status nrtCreate(int device, nrt_ctx **out) {
  if (!out) return fail(nullptr, NRT_ERR_INVALID, "nrtCreate: out == NULL");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(nullptr, NRT_ERR_DEVICE, "nrtCreate: no HIP device visible (%s)",
                e == hipSuccess ? "count == 0" : hipGetErrorString(e));
  if (device < 0 || device >= ndev)
    return fail(nullptr, NRT_ERR_INVALID, "nrtCreate: device %d out of range [0,%d)", device, ndev);
  nrt_ctx *c = new nrt_ctx();
  c->device = device;
  if ((e = hipSetDevice(device)) != hipSuccess ||
      (e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreate(&c->ev_b0)) != hipSuccess || (e = hipEventCreate(&c->ev_b1)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev_build_state, hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev_refit, hipEventDisableTiming)) != hipSuccess ||
      (e = hipHostMalloc(&c->build_state, kBuildPinnedBytes, hipHostMallocDefault)) != hipSuccess ||
      (e = hipMalloc((void **)&c->d_counters, 16 * sizeof(unsigned long long))) != hipSuccess) {
    fail(nullptr, NRT_ERR_DEVICE, "nrtCreate: %s", hipGetErrorString(e));
    nrtDestroy(c);
    return NRT_ERR_DEVICE;
  }
  for (nrt_ctx::LaunchSlot &sl : c->slots) {
    if ((e = hipMalloc((void **)&sl.d_cursor, 2 * kCursorStrideWords * 4 * kMaxParts)) != hipSuccess ||
        (e = hipMemset(sl.d_cursor, 0, 2 * kCursorStrideWords * 4 * kMaxParts)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&sl.done, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreate(&sl.t0)) != hipSuccess || (e = hipEventCreate(&sl.t1)) != hipSuccess ||
        (e = hipHostMalloc((void **)&sl.h_done, sizeof(DoneRec), hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess ||
        (e = hipHostGetDevicePointer((void **)&sl.d_done, sl.h_done, 0)) != hipSuccess ||
        (e = hipMalloc((void **)&sl.d_count, sizeof(DoneCount))) != hipSuccess ||
        (e = hipMemset(sl.d_count, 0, sizeof(DoneCount))) != hipSuccess ||
        (e = hipMemset((char *)sl.d_count + offsetof(DoneCount, t_begin), 0xFF, sizeof(unsigned long long))) != hipSuccess) {
      fail(nullptr, NRT_ERR_DEVICE, "nrtCreate: %s", hipGetErrorString(e));
      nrtDestroy(c);
      return NRT_ERR_DEVICE;
    }
  }
  for (nrt_ctx::LaunchSlot &sl : c->slots) memset(sl.h_done, 0, sizeof(DoneRec));
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
    c->num_cus = prop.multiProcessorCount;
  // Environment overrides (debugging aid): NRT_<NAME> for every tunable of nrtSetTunable, applied once at creation — in the
  // profiling library always, in the product library only when the process opts in with NRT_ALLOW_ENV=1: a stray variable in
  // a user's environment must not move the product between parity classes (order4) or walks.
  const bool allow_env = env_overrides_allowed();
  for (const TunableDesc &d : kTunables) {
    if (!allow_env) break;
    char env[64] = "NRT_";
    size_t k = 4;
    for (const char *p = d.name; *p && k + 1 < sizeof(env); p++) env[k++] = (char)toupper((unsigned char)*p);
    env[k] = 0;
    if (const char *e = getenv(env)) (void)tunable_set(c, d.name, atoll(e));
  }
  *out = c;
  return NRT_OK;
}

void nrtDestroy(nrt_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->ev_refit) (void)refit_host_wait_locked(c);
  for (nrt_ctx::LaunchSlot &sl : c->slots) { // launches still in flight on the caller's streams
    if (sl.h_done || sl.done) (void)slot_done(c, sl);
    if (sl.d_cursor) (void)hipFree(sl.d_cursor);
    if (sl.d_count) (void)hipFree(sl.d_count);
    if (sl.h_done) (void)hipHostFree(sl.h_done);
    if (sl.spill.p) (void)hipFree(sl.spill.p);
    if (sl.spill_tmin.p) (void)hipFree(sl.spill_tmin.p);
    if (sl.cyl_hits.p) (void)hipFree(sl.cyl_hits.p);
    if (sl.cyl_bits.p) (void)hipFree(sl.cyl_bits.p);
    if (sl.done) (void)hipEventDestroy(sl.done);
    if (sl.t0) (void)hipEventDestroy(sl.t0);
    if (sl.t1) (void)hipEventDestroy(sl.t1);
  }
  free_tree(c);
  free_mesh(c);
  DevBuf *bufs[] = {&c->b_verts, &c->b_radii, &c->b_faces, &c->st_rays, &c->st_hits, &c->st_mask, &c->st_skip, &c->b_nodes, &c->b_indices, &c->b_tris, &c->b_wide, &c->b_wide4, &c->b_wide_scratch, &c->b_build_ws, &c->b_wave_clock, &c->b_seg_verts, &c->b_seg_radii, &c->b_seg_prim, &c->b_seg_off, &c->b_refit_plan, &c->b_refit_stage, &c->b_max_index, &c->b_verts1, &c->b_tris1, &c->st_times};
  for (DevBuf *b : bufs)
    if (b->p) (void)hipFree(b->p);
  if (c->d_counters) (void)hipFree(c->d_counters);
  if (c->build_state) (void)hipHostFree(c->build_state);
  if (c->h_max_index) (void)hipHostFree(c->h_max_index);
  hipEvent_t evs[] = {c->ev_b0, c->ev_b1, c->ev_build_state, c->ev_refit};
  for (hipEvent_t ev : evs)
    if (ev) (void)hipEventDestroy(ev);
  for (int k = 0; k < 2; k++)
    for (hipEvent_t e : {c->ev_in[k], c->ev_tr[k], c->ev_out[k]})
      if (e) (void)hipEventDestroy(e);
  if (c->copy_in) (void)hipStreamDestroy(c->copy_in);
  if (c->copy_out) (void)hipStreamDestroy(c->copy_out);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

const char *nrtLastError(const nrt_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

} // extern "C"

// ---------------------------------------------------------------------------
// primitives: one path for the setters of every kind (prim_kinds.h), from host memory or (the *Device forms: copied on the
// caller's stream) from HBM.  Every refusal comes before anything changes; the counts are set once the primitives are in place,
// so a failed upload leaves an empty context.
// ---------------------------------------------------------------------------
// The first refusal of every setter.
static nrt_status refuse_precision(nrt_ctx *c, const char *fn, int kind, int prec) {
  if (!c) return NRT_ERR_INVALID;
  if (c->prec == 0 || c->prec == prec) return NRT_OK;
  return fail(c, NRT_ERR_PRECISION, kind == kPrimTriangles ? "%s: context already holds a %s mesh" : "%s: context already holds %s primitives", fn,
              c->prec == 4 ? "f32" : "f64");
}

// Nothing is refused any more: the old tree and primitives go, the context is of this kind and precision.
static void drop_primitives(nrt_ctx *c, int kind, int prec) {
  free_tree(c);
  free_mesh(c);
  c->prec = prec;
  c->prim_kind = kind;
}
static nrt_status begin_set(nrt_ctx *c, int kind, int prec) {
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, wait_for_launches(c));
  drop_primitives(c, kind, prec);
  return NRT_OK;
}

// What remains of a Device set call once the old primitives are gone and a HIP call fails: an empty context and the reason.
static nrt_status set_device_failed(nrt_ctx *c, const char *fn, hipStream_t s, hipError_t e) {
  (void)hipStreamSynchronize(s);
  free_mesh(c);
  return fail(c, NRT_ERR_DEVICE, "%s: %s (the context's primitives were dropped: set them again)", fn, hipGetErrorString(e));
}

// `src` (null: nothing to copy yet) into the grow-only buffer `b`: from the host, or (`device`) from HBM on `s`.
static nrt_status upload(nrt_ctx *c, const char *fn, DevBuf &b, const void *src, size_t bytes, bool device, hipStream_t s) {
  if (!device) {
    if (nrt_status st = ensure(c, b, bytes)) return st;
    if (src) HIPCHK(c, hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return NRT_OK;
  }
  hipError_t e = devbuf_ensure(&b, bytes);
  if (e == hipSuccess && src) e = hipMemcpyAsync(b.p, src, bytes, hipMemcpyDeviceToDevice, s);
  return e == hipSuccess ? NRT_OK : set_device_failed(c, fn, s, e);
}
// The tail of every setter: a Device form waits for its copies (the context owns its copy: the caller's buffers are free again),
// and the primitives are in place.
static nrt_status adopt_primitives(nrt_ctx *c, const char *fn, bool device, hipStream_t s, bool faces, bool radii, uint32_t n, uint32_t num_verts) {
  if (device) {
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return set_device_failed(c, fn, s, e);
  }
  c->d_verts = c->b_verts.p;
  c->d_faces = faces ? (uint32_t *)c->b_faces.p : nullptr;
  c->d_radii = radii ? c->b_radii.p : nullptr;
  c->num_faces = n;
  c->num_verts = num_verts;
  return NRT_OK;
}

template <typename T>
static nrt_status set_mesh(nrt_ctx *c, const T *vertices, size_t stride, const uint32_t *faces,
                           uint32_t num_faces) {
  const char *fn = "nrtSetMesh";
  if (nrt_status st = refuse_precision(c, fn, kPrimTriangles, (int)sizeof(T))) return st;
  if (num_faces && (!vertices || !faces)) return fail(c, NRT_ERR_INVALID, "nrtSetMesh: NULL mesh pointer");
  if (stride < 3 * sizeof(T) && num_faces)
    return fail(c, NRT_ERR_INVALID, "nrtSetMesh: vertex stride %zu < %zu", stride, 3 * sizeof(T));
  NRT_RANGE("nrtSetMesh (compaction + upload)");
  if (nrt_status st = begin_set(c, kPrimTriangles, (int)sizeof(T))) return st;
  if (num_faces == 0) return NRT_OK;
  // The reference's mesh carries no vertex count (nanort.h:925-930): derive it.
  uint32_t maxv = 0;
  const size_t ni = 3 * (size_t)num_faces;
  for (size_t i = 0; i < ni; i++) maxv = faces[i] > maxv ? faces[i] : maxv;
  const uint32_t nv = maxv + 1;
  // Compact the strided vertex array (get_vertex_addr, nanort.h:467-472) to tight xyz.
  const T *src = vertices;
  std::vector<T> tight;
  if (stride != 3 * sizeof(T)) {
    tight.resize(3 * (size_t)nv);
    const unsigned char *base = reinterpret_cast<const unsigned char *>(vertices);
    for (uint32_t v = 0; v < nv; v++) {
      const T *p = reinterpret_cast<const T *>(base + (size_t)v * stride);
      tight[3 * (size_t)v + 0] = p[0];
      tight[3 * (size_t)v + 1] = p[1];
      tight[3 * (size_t)v + 2] = p[2];
    }
    src = tight.data();
  }
  nrt_status st;
  if ((st = upload(c, fn, c->b_verts, src, 3 * (size_t)nv * sizeof(T), false, nullptr)) || (st = upload(c, fn, c->b_faces, faces, ni * sizeof(uint32_t), false, nullptr)))
    return st;
  return adopt_primitives(c, fn, false, nullptr, true, false, num_faces, nv);
}

// nrtSetMesh for arrays in HBM: the same state as set_mesh leaves, the vertex count derived and the caller's `num_vertices`
// checked on the device before any vertex is read and before anything of the context is dropped.
template <typename T>
static nrt_status set_mesh_device(nrt_ctx *c, const T *vertices, uint32_t num_vertices, size_t stride, const uint32_t *faces,
                                  uint32_t num_faces, hipStream_t s) {
  const char *fn = "nrtSetMeshDevice";
  if (nrt_status st = refuse_precision(c, fn, kPrimTriangles, (int)sizeof(T))) return st;
  if (num_faces) {
    if (!vertices || !faces) return fail(c, NRT_ERR_INVALID, "%s: NULL mesh pointer", fn);
    if (num_vertices == 0) return fail(c, NRT_ERR_INVALID, "%s: num_vertices == 0 with %u faces", fn, num_faces);
    if (stride < 3 * sizeof(T)) return fail(c, NRT_ERR_INVALID, "%s: vertex stride %zu < %zu", fn, stride, 3 * sizeof(T));
    if (stride % sizeof(T) != 0 || (uintptr_t)vertices % sizeof(T) != 0)
      return fail(c, NRT_ERR_INVALID, "%s: vertex stride %zu or pointer not aligned to %zu bytes", fn, stride, sizeof(T));
    if ((uintptr_t)faces % sizeof(uint32_t) != 0) return fail(c, NRT_ERR_INVALID, "%s: face pointer not aligned to 4 bytes", fn);
  }
  NRT_RANGE("nrtSetMeshDevice");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, wait_for_launches(c));
  uint32_t nv = 0;
  const size_t ni = 3 * (size_t)num_faces;
  if (num_faces) { // the guard: nothing of the context has changed yet
    if (!c->h_max_index) HIPCHK(c, hipHostMalloc((void **)&c->h_max_index, sizeof(uint32_t), hipHostMallocDefault));
    nrt_status st;
    if ((st = ensure(c, c->b_max_index, sizeof(uint32_t)))) return st;
    HIPCHK(c, launch_max_index(faces, ni, (uint32_t *)c->b_max_index.p, s));
    HIPCHK(c, hipMemcpyAsync(c->h_max_index, c->b_max_index.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const uint32_t maxv = *c->h_max_index;
    if (maxv >= num_vertices)
      return fail(c, NRT_ERR_INVALID, "%s: face index %u is out of range: the vertex block holds %u rows", fn, maxv, num_vertices);
    nv = maxv + 1;
  }
  drop_primitives(c, kPrimTriangles, (int)sizeof(T));
  if (num_faces == 0) return NRT_OK;
  const bool tight = stride == 3 * sizeof(T); // (tight already: a copy; else the gather kernel)
  nrt_status st;
  if ((st = upload(c, fn, c->b_verts, tight ? vertices : nullptr, 3 * (size_t)nv * sizeof(T), true, s))) return st;
  if (!tight) {
    const hipError_t e = launch_gather_vertices<T>(vertices, stride, nv, (T *)c->b_verts.p, s);
    if (e != hipSuccess) return set_device_failed(c, fn, s, e);
  }
  if ((st = upload(c, fn, c->b_faces, faces, ni * sizeof(uint32_t), true, s))) return st;
  return adopt_primitives(c, fn, true, s, true, false, num_faces, nv);
}

// The kinds with radii — spheres (SphereGeometry of examples/particle_primitive/main.cc:113-147), cylinders (CylinderGeometry of
// examples/cylinder_primitive/main.cc:124-210), curves (CurveGeometry of examples/curves_primitive/main.cc:513-604) — as their
// row of kPrimKinds describes them: `n` times pos_floats positions and radius_floats radii of `prec` bytes each.
// `extra_refusal`: the caller's own refusal (null: none), in its place among the shared ones.
static nrt_status set_radius_prims(nrt_ctx *c, const char *fn, int kind, int prec, const void *positions, const void *radii, uint32_t n, bool device,
                                   hipStream_t s, const char *extra_refusal = nullptr) {
  const PrimKind &k = kPrimKinds[kind];
  if (nrt_status st = refuse_precision(c, fn, kind, prec)) return st;
  if (extra_refusal) return fail(c, NRT_ERR_INVALID, "%s: %s", fn, extra_refusal);
  if (n && (!positions || !radii)) return fail(c, NRT_ERR_INVALID, "%s: NULL pointer", fn);
  if (k.max_count && n >= k.max_count) return fail(c, NRT_ERR_INVALID, "%s: too many %s", fn, k.name);
  if (device && n && ((uintptr_t)positions % (size_t)prec != 0 || (uintptr_t)radii % (size_t)prec != 0))
    return fail(c, NRT_ERR_INVALID, "%s: pointer not aligned to %d bytes", fn, prec);
  if (nrt_status st = begin_set(c, kind, prec)) return st;
  if (n == 0) return NRT_OK;
  nrt_status st;
  if ((st = upload(c, fn, c->b_verts, positions, (size_t)k.pos_floats * n * (size_t)prec, device, s)) ||
      (st = upload(c, fn, c->b_radii, radii, (size_t)k.radius_floats * n * (size_t)prec, device, s)))
    return st;
  return adopt_primitives(c, fn, device, s, false, true, n, (uint32_t)k.num_verts * n);
}

// Segments for the builder (prims.hip, k_cylinder_segments): a cylinder many radii long is handed over as several pieces
// with their own tight boxes and the cylinder's id.  Counts on the host (the arrays are here anyway), pieces on the device.
static nrt_status segment_cylinders(nrt_ctx *c, const float *endpoints, const float *radii, uint32_t n) {
  c->num_segs = 0;
  c->segment_ms = 0.f;
  // (zero-radius "cylinders" are boxes — the top-level tree of a scene is built over them — and cyl_split = 1 asks for the
  // example's own boxes: neither needs the counting pass or its array)
  bool any_radius = false;
  for (size_t i = 0; i < 2 * (size_t)n && !any_radius; i++) any_radius = radii[i] > 0.0f;
  if (c->cyl_split <= 1 || !any_radius) return NRT_OK;
  const auto seg_t0 = std::chrono::steady_clock::now();
  std::vector<uint32_t> off((size_t)n + 1);
  const uint64_t total = cylinder_segment_offsets(endpoints, radii, n, c->cyl_seg_radii, (uint32_t)c->cyl_split, kPackedFirstMask, off.data());
  if (total > (uint64_t)n) {
    nrt_status st;
    if ((st = ensure(c, c->b_seg_off, ((size_t)n + 1) * sizeof(uint32_t))) || (st = ensure(c, c->b_seg_verts, 6 * (size_t)total * sizeof(float))) ||
        (st = ensure(c, c->b_seg_radii, 2 * (size_t)total * sizeof(float))) || (st = ensure(c, c->b_seg_prim, (size_t)total * sizeof(uint32_t))))
      return st;
    HIPCHK(c, hipMemcpyAsync(c->b_seg_off.p, off.data(), ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_cylinder_segments((const float *)c->d_verts, (const float *)c->d_radii, (const uint32_t *)c->b_seg_off.p, n,
                                       (float *)c->b_seg_verts.p, (float *)c->b_seg_radii.p, (uint32_t *)c->b_seg_prim.p, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (`off` is pageable host memory)
    c->num_segs = (uint32_t)total;
  }
  // the segmentation is part of building this tree: its wall time is added to the build's (nrtLastBuildMs, build_secs)
  c->segment_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - seg_t0).count();
  return NRT_OK;
}

static nrt_status set_cylinders(nrt_ctx *c, const float *endpoints, const float *radii, uint32_t n, int test_cap) {
  if (nrt_status st = set_radius_prims(c, "nrtSetCylinders", kPrimCylinders, 4, endpoints, radii, n, false, nullptr)) return st;
  c->cyl_test_cap = test_cap ? 1u : 0u;
  return n ? segment_cylinders(c, endpoints, radii, n) : NRT_OK;
}

static nrt_status set_curves(nrt_ctx *c, const float *cps, const float *radii, uint32_t n, uint32_t subdiv, bool device, hipStream_t s) {
  char refusal[64] = "";
  if (subdiv < 1u || subdiv > 64u) snprintf(refusal, sizeof(refusal), "num_subdivisions %u outside 1..64", subdiv);
  if (nrt_status st = set_radius_prims(c, device ? "nrtSetCurvesDevice" : "nrtSetCurves", kPrimCurves, 4, cps, radii, n, device, s, refusal[0] ? refusal : nullptr))
    return st;
  c->curve_subdiv = subdiv;
  return NRT_OK;
}

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

// Library-internal (scene.hip): where a built fp32 context keeps its tree on the device.  Waits for the context's own
// stream, so the arrays are complete; they stay valid until the context is rebuilt or destroyed.
nrt_status nrt_internal_tree_view(nrt_ctx *c, nrt::TreeViewF32 *out) {
  if (!c || !out) return NRT_ERR_INVALID;
  if (c->prec != 4 || !c->d_nodes || !c->d_wide) return fail(c, NRT_ERR_INVALID, "no fp32 tree on the device");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, refit_host_wait(c));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  out->nodes = (const nrt_node_f32 *)c->d_nodes;
  out->indices = c->d_indices;
  out->wide = c->d_wide;
  out->wide4 = c->d_wide4;
  out->prims = c->d_tris;
  out->num_nodes = (uint32_t)c->num_nodes;
  out->num_indices = (uint32_t)c->num_indices;
  out->packed_leaves = c->packed_leaves;
  out->root_is_branch = c->root_is_branch;
  out->tree_nested = c->tree_nested;
  out->prim_kind = (uint32_t)c->prim_kind;
  out->tree_depth = c->tree_depth;
  out->max_leaf_count = c->max_leaf_count;
  out->generation = c->generation;
  return NRT_OK;
}
uint64_t nrt_internal_generation(const nrt_ctx *c) { return c ? c->generation : 0; }
int nrt_internal_device(const nrt_ctx *c) { return c ? c->device : 0; } // group.hip
int nrt_internal_prim_kind(const nrt_ctx *c) { return c ? c->prim_kind : (int)kPrimTriangles; } // scene.hip

// ---------------------------------------------------------------------------
// traverse
// ---------------------------------------------------------------------------
static const nrt_trace_options kDefaultTrace = {{0u, 0x7FFFFFFFu}, 0xFFFFFFFFu, 0, {0, 0, 0}}; // nanort.h:617-623

// Several batches for one launch (nrtTraverseBatchesDevice): fp32 triangle contexts on the WideNode kernels.
template <typename T>
struct TraverseBatches {
  uint32_t nb;
  const typename Wire<T>::Ray *rays[kMaxBatches];
  typename Wire<T>::Hit *hits[kMaxBatches];
  uint8_t *mask[kMaxBatches];
  uint64_t count[kMaxBatches];
  const uint32_t *skip[kMaxBatches]; // per-ray skip ids of batch k, or null: the call's skip_prim_id
  uint32_t anyhit; // bit k: batch k is an occlusion query
};

// What one traversal launch is asked for: the query kind says which of the outputs it reads.  (Occlusion: every ray stops at the
// first primitive it accepts; Count: the literal kernel's counting pass into d_counters, no output of its own; OcclusionPrims: the
// occlusion query of nrtOccludedBatchPrims*, which every primitive kind takes — flags straight into the caller's mask, no compact
// records, no post pass; on a triangle context it IS Occlusion: traverse_device says so under the lock.)
// (Motion / MotionOcclusion: the closest-hit and occlusion queries of nrt*BatchMotion*, every ray at its own time: motion.hip)
enum class Query { Closest, Occlusion, Count, MultiHit, Cylinders, MultiBatch, Curves, OcclusionPrims, Motion, MotionOcclusion };
template <typename T>
struct TraverseLaunch {
  Query kind;
  const typename Wire<T>::Ray *rays;
  uint64_t n;
  const nrt_trace_options *opt; // null: the reference's defaults
  hipStream_t stream;
  bool timed = false; // bracket the launch with the slot's timing events (when it publishes no completion record)
  typename Wire<T>::Hit *hits = nullptr; // Closest (null: flags only); MultiHit: max_hits records per ray
  uint8_t *mask = nullptr;               // Closest (may be null), Occlusion, OcclusionPrims, Cylinders, Curves
  void *cyl_hits = nullptr;              // Cylinders: 28-byte records, Curves: 40-byte records, written by the post pass
  uint32_t max_hits = 0;
  uint32_t *hit_counts = nullptr;        // MultiHit (may be null): one word per ray
  const TraverseBatches<T> *batches = nullptr; // MultiBatch: rays and outputs per batch, n = all their rays (the context takes one launch: the caller checked)
  const uint32_t *skip_ids = nullptr;    // Closest, Occlusion (nrt*BatchSkip*): one skip id per ray in the place of opt->skip_prim_id (MultiBatch: batches->skip[])
  const T *times = nullptr;              // Motion, MotionOcclusion: one time per ray (null: every ray at time 0)
  bool motion() const { return kind == Query::Motion || kind == Query::MotionOcclusion; }
  // the launch carries per-ray skip ids
  bool has_skip_ids() const {
    if (skip_ids) return true;
    if (batches)
      for (uint32_t k = 0; k < batches->nb; k++)
        if (batches->skip[k]) return true;
    return false;
  }
};

// Every combination a launch cannot be is refused here (under launch_mutex: the tunables hold still).
template <typename T>
static nrt_status validate_launch(nrt_ctx *c, const TraverseLaunch<T> &l) {
  const bool custom = c->prim_kind != kPrimTriangles; // spheres / cylinders
  if (c->prec != (int)sizeof(T)) return fail(c, NRT_ERR_PRECISION, "nrtTraverseBatch: precision mismatch");
  if (l.motion()) { // (include/nanort_hip.h, "motion blur")
    if (custom) return fail(c, NRT_ERR_INVALID, "motion queries: triangle contexts only (this context holds %s)", kPrimKinds[c->prim_kind].name);
    if (!c->d_verts1) return fail(c, NRT_ERR_INVALID, "motion queries: the context holds no motion keyframe (nrtSetMeshMotion)");
    if (c->d_nodes && !c->d_tris1) return fail(c, NRT_ERR_INVALID, "motion queries: internal: no keyframe-1 leaf records");
    if (((uintptr_t)l.times % sizeof(T)) != 0u) return fail(c, NRT_ERR_INVALID, "motion queries: the times array is not aligned to %zu bytes", sizeof(T));
    if (l.kind == Query::MotionOcclusion && !l.mask && l.n) return fail(c, NRT_ERR_INVALID, "nrtOccludedBatchMotion: NULL mask");
  }
  if (l.has_skip_ids()) { // (include/nanort_hip.h, "per-ray skip ids")
    if (custom)
      return fail(c, NRT_ERR_INVALID, "per-ray skip ids: triangle contexts only (the sphere, cylinder and curve intersectors have no skip id)");
    if (l.kind != Query::Closest && l.kind != Query::Occlusion && l.kind != Query::MultiBatch)
      return fail(c, NRT_ERR_INVALID, "per-ray skip ids: closest-hit and occlusion queries only");
    bool aligned = ((uintptr_t)l.skip_ids & 3u) == 0u;
    if (l.batches)
      for (uint32_t k = 0; k < l.batches->nb; k++) aligned = aligned && ((uintptr_t)l.batches->skip[k] & 3u) == 0u;
    if (!aligned) return fail(c, NRT_ERR_INVALID, "per-ray skip ids: the device array is not 4-byte aligned");
  }
  const bool prims = l.kind == Query::OcclusionPrims; // (a sphere, cylinder or curve context: traverse_device)
  if (prims && !l.mask && l.n) return fail(c, NRT_ERR_INVALID, "nrtOccludedBatchPrims: NULL mask");
  if (!prims && (c->prim_kind == kPrimCylinders) != (l.kind == Query::Cylinders))
    return fail(c, NRT_ERR_INVALID, "cylinder primitives are traced with nrtTraverseBatchCylinders*_f32 (28-byte records), "
                                    "every other primitive kind with nrtTraverseBatch*");
  if (!prims && (c->prim_kind == kPrimCurves) != (l.kind == Query::Curves))
    return fail(c, NRT_ERR_INVALID, "curve primitives are traced with nrtTraverseBatchCurves*_f32 (40-byte records) and by nothing else, "
                                    "every other primitive kind by its own entry points");
  if (!c->d_nodes) return fail(c, NRT_ERR_INVALID, "nrtTraverseBatch: no tree (call nrtBuild or nrtSetTree)");
  if (l.n == 0) return NRT_OK;
  if (!l.rays) return fail(c, NRT_ERR_INVALID, "nrtTraverseBatch: NULL rays");
  if (l.n > 0x7FFFFFFFull) return fail(c, NRT_ERR_INVALID, "nrtTraverseBatch: more than 2^31-1 rays in one call");
  if (custom && (l.kind == Query::Count || !c->d_wide))
    return fail(c, NRT_ERR_INVALID, "nrtTraverse: custom primitives run on the WideNode kernel only (no counting pass)");
  if (l.kind == Query::Occlusion && (custom || !c->d_wide))
    return fail(c, NRT_ERR_INVALID, "nrtOccludedBatch: occlusion queries run on the triangle WideNode kernel only");
  if (l.kind == Query::MultiBatch && (sizeof(T) != 4 || custom || !c->wide || !c->d_wide))
    return fail(c, NRT_ERR_INVALID, "internal: multi-batch launch on a context that cannot take it");
  return NRT_OK;
}

// Launch slot: the one this stream used last (stream order already serialises the two launches), else
// a fresh one, else the oldest — whose previous launch this stream then waits for on the device
static nrt_status take_slot(nrt_ctx *c, hipStream_t s, nrt_ctx::LaunchSlot **out) {
  for (int pass = 0; pass < 2; pass++) // (0: this stream's own slot, 1: a fresh one)
    for (nrt_ctx::LaunchSlot &sl : c->slots)
      if (pass == 0 ? (sl.used && sl.stream == s) : !sl.used) {
        *out = &sl;
        return NRT_OK;
      }
  nrt_ctx::LaunchSlot *slot = *out = &c->slots[c->next_victim];
  c->next_victim = (c->next_victim + 1) % nrt_ctx::kSlots;
  if (slot->last_has_rec)
    HIPCHK(c, wait_record(*slot)); // (the host waits: a fifth concurrent stream is the rare case)
  else
    HIPCHK(c, hipStreamWaitEvent(s, slot->done, 0));
  return NRT_OK;
}

// The kernel a launch runs, from the context's tree and tunables and the launch's kind and options.
enum class Walk { Literal, OneLevel, TwoLevel, MultiHit, Motion }; // k_traverse, k_traverse_wide of WIDTH 2 / 4, k_traverse_multihit, k_traverse_motion
struct WalkChoice {
  Walk walk;
  bool plain_options; // prim ids are < num_faces: nothing can be rejected by the trace options -> the kernel variant without the id tests
  bool wide4_big;     // the two-level records are addressed with 64-bit offsets
  int lds_entries;    // per-lane stack entries the variant keeps in LDS
  unsigned dbg;
  bool wide() const { return walk == Walk::OneLevel || walk == Walk::TwoLevel; }
  bool wide4() const { return walk == Walk::TwoLevel; }
};
template <typename T>
static WalkChoice choose_walk(const nrt_ctx *c, const TraverseLaunch<T> &l) {
  WalkChoice w;
#ifdef NRT_PROF
  w.dbg = c->debug_flags;
#else
  w.dbg = c->debug_flags & ~(32u | 64u | 8192u); // (the counting / clocked instantiations live in libnanort_hip_prof.so)
#endif
  const bool custom = c->prim_kind != kPrimTriangles; // the custom primitives share one launch geometry
  const bool multihit = l.kind == Query::MultiHit;
  const bool use_wide = (c->wide || custom || l.kind == Query::Occlusion) && l.kind != Query::Count && c->d_wide && !multihit && !l.motion();
  // two levels per step: closest-hit walks of nested fp32 triangle trees, outside the profiling / splitting variants
  w.plain_options = l.opt->prim_ids_range[0] == 0u && l.opt->prim_ids_range[1] >= c->num_faces && l.opt->skip_prim_id >= c->num_faces &&
                    !l.opt->cull_back_face;
  if (l.has_skip_ids()) w.plain_options = false; // (any ray may carry an id that rejects a primitive: the id tests stay)
  // (the profiling instantiations of the two-level walk are built for the default trace options only: with options that can
  // reject a primitive a profiled launch walks one level per step, whose profiling variant honours them)
  const bool prof_needs_w2 = (w.dbg & (32u | 8192u)) && !w.plain_options && !custom;
  // (a record array of 4 GiB or more is walked two levels per step by the default walk of triangle trees only: closest hits in the
  // reference's order, outside the profiling instantiations)
  w.wide4_big = c->num_branch_records >= (1ull << 25) || (c->wide4_big_ok == 2 && c->prim_kind == kPrimTriangles); // (2: forced, for the tests)
  const bool use_wide4 = use_wide && c->d_wide4 && c->wide_stack == 10 && c->tree_nested && c->root_is_branch && !prof_needs_w2 &&
                         (!w.wide4_big || (!custom && !c->order4 && !(w.dbg & (32u | 8192u))));
  w.walk = l.motion() ? Walk::Motion : multihit ? Walk::MultiHit : (use_wide4 ? Walk::TwoLevel : (use_wide ? Walk::OneLevel : Walk::Literal));
  w.lds_entries = (multihit || l.motion()) ? kLdsStackDefault : (use_wide4 ? kWide4LdsStack : (custom ? 10 : (use_wide ? c->wide_stack : c->lds_stack)));
  return w;
}

// Persistent grid: every block resident.  A variant's occupancy is asked for once per context and key (what selects the kernel).
template <typename T>
static GridPlan size_grid(nrt_ctx *c, const WalkChoice &w, uint64_t n) {
  auto &e = c->occupancy[(int)w.walk][c->prim_kind];
  if (e.blocks_per_cu == 0 || e.lds_entries != w.lds_entries)
    e = {w.lds_entries, (unsigned)(w.walk == Walk::Motion    ? traverse_motion_blocks_per_cu<T>()
                        : w.walk == Walk::MultiHit  ? traverse_multihit_blocks_per_cu<T>()
                        : w.walk == Walk::Literal ? traverse_blocks_per_cu<T>(w.lds_entries)
                                                  : traverse_wide_blocks_per_cu<T>(w.lds_entries, c->prim_kind, w.wide4()))};
  const unsigned per_cu = c->max_blocks_per_cu && e.blocks_per_cu > c->max_blocks_per_cu ? c->max_blocks_per_cu : e.blocks_per_cu;
  return plan_grid(n, kTraverseBlock, (uint32_t)c->num_cus, per_cu, c->num_parts);
}

// TraverseArgs, part 1: the tree, the trace options and the tunables of the walk.
template <typename T>
static void fill_walk_args(const nrt_ctx *c, const TraverseLaunch<T> &l, const WalkChoice &w, TraverseArgs<T> &a) {
  const bool profiled = (w.dbg & (32u | 8192u)) != 0u;
  a.nodes = (const typename Wire<T>::Node *)c->d_nodes;
  a.tris = (const LeafTri<T> *)c->d_tris;
  a.spheres = (const LeafSphere<T> *)c->d_tris;
  a.centers = (const T *)c->d_verts;
  a.cylinders = (const LeafCylinder<T> *)c->d_tris;
  a.cyl_test_cap = c->cyl_test_cap;
  a.curves = (const LeafCurve *)c->d_tris;
  a.curve_subdiv = c->curve_subdiv;
  a.wide = (const WideNode<T> *)c->d_wide;
  a.wide4 = w.wide4() ? (const Wide4Node<T> *)c->d_wide4 : nullptr;
  a.packed_leaves = c->packed_leaves;
  a.wide4_big = (w.wide4() && w.wide4_big) ? 1u : 0u;
  a.wide_below_4g = (c->f64_row_fetch && (uint64_t)c->num_branch_records * sizeof(WideNode<T>) < (1ull << 32)) ? 1u : 0u;
  a.root_is_branch = c->root_is_branch;
  a.debug_flags = w.dbg;
  a.range0 = l.opt->prim_ids_range[0];
  a.range1 = l.opt->prim_ids_range[1];
  a.skip_prim = l.opt->skip_prim_id;
  a.skip_ids = l.skip_ids; // (MultiBatch: null, the table's skip_v instead)
  a.cull_back_face = l.opt->cull_back_face ? 1u : 0u;
  a.any_hit = (l.kind == Query::Occlusion || l.kind == Query::OcclusionPrims || l.kind == Query::MotionOcclusion) ? 1u : 0u;
  a.plain_options = w.plain_options ? 1u : 0u;
  a.root_test = c->tree_nested ? 0u : 1u;
  a.order4 = (c->order4 && w.wide4() && c->prim_kind == kPrimTriangles && l.kind != Query::Occlusion && !profiled) ? 1u : 0u;
  a.leaf_items = (c->leaf_compact && w.wide4() && c->prim_kind == kPrimTriangles && c->max_leaf_count <= 4u && !profiled) ? 1u : 0u;
  a.dyn_head = c->dyn_head ? 1u : 0u;
  a.counters = c->d_counters;
  a.wave_clock = (w.dbg & 8192u) ? (unsigned long long *)c->b_wave_clock.p : nullptr; // (sized by traverse_device; the bit is the profiling library's)
  a.chunk = c->chunk;
  a.chunk_tail_pct = c->chunk_tail_pct;
  a.refill_min = c->refill_min;
  a.trav_min = w.wide4() ? c->trav_min4 : c->trav_min;
  a.leaf_min = c->leaf_min;
  a.tail_lanes = c->tail_quad;
}

// ... part 2: the slot's scratch, the grid and the work distribution (launch_plan.h), the rays and where their records go.
template <typename T>
static void fill_launch_args(const TraverseLaunch<T> &l, const nrt_ctx::LaunchSlot *slot, const GridPlan &g, const DistributionPlan &d,
                             uint32_t levels, TraverseArgs<T> &a) {
  a.spill = (uint32_t *)slot->spill.p;
  a.spill_tmin = (T *)slot->spill_tmin.p;
  a.spill_stride = g.grid * kTraverseBlock;
  a.spill_levels = levels;
  a.ray_cursor = slot->d_cursor + (size_t)slot->parity * kCursorStrideWords * kMaxParts;
  a.next_cursor = slot->d_cursor + (size_t)(slot->parity ^ 1u) * kCursorStrideWords * kMaxParts;
  a.num_parts = g.parts;
  a.blocks_per_part = g.blocks_per_part;
  a.static_per_wave = d.static_per_wave;
  a.static_bands = d.static_bands;
  a.band_len = d.band_len;
  a.band_static = d.band_static;
  a.dyn_per_band = d.dyn_per_band;
  a.dyn_banded = d.dyn_banded;
  a.tail_begin = d.tail_begin;
  a.dyn_total = d.dyn_total;
  a.dyn_per_part = d.dyn_per_part;
  a.rays = l.rays;
  a.hits = l.hits;
  a.mask = l.mask;
  if (l.kind == Query::Cylinders || l.kind == Query::Curves) {
    a.hits = (typename Wire<T>::Hit *)slot->cyl_hits.p;
    a.mask = (uint8_t *)slot->cyl_bits.p;
  }
  a.num_rays = (uint32_t)l.n;
  a.num_batches = 1u;
  a.batch_anyhit = 0u;
  for (int k = 0; k < kMaxBatches; k++) {
    a.batch_end[k] = (uint32_t)l.n;
    a.batches[k] = BatchPtrs{nullptr, nullptr, nullptr, nullptr};
  }
  if (l.kind != Query::MultiBatch) return;
  const TraverseBatches<T> *mb = l.batches;
  a.num_batches = mb->nb;
  a.batch_anyhit = mb->anyhit;
  uint64_t start = 0;
  for (uint32_t k = 0; k < mb->nb; k++) { // pointers addressed by the virtual index: base - start
    a.batches[k].rays_v = mb->rays[k] - start;
    a.batches[k].hits_v = mb->hits[k] ? mb->hits[k] - start : nullptr;
    a.batches[k].mask_v = mb->mask[k] ? mb->mask[k] - start : nullptr;
    a.batches[k].skip_v = mb->skip[k] ? mb->skip[k] - start : nullptr;
    start += mb->count[k];
    a.batch_end[k] = (uint32_t)start;
  }
  for (uint32_t k = mb->nb; k < (uint32_t)kMaxBatches; k++) a.batch_end[k] = (uint32_t)start;
}

// The kernel, the slot's bookkeeping, what runs behind the kernel.
template <typename T>
static nrt_status enqueue_launch(nrt_ctx *c, const TraverseLaunch<T> &l, const WalkChoice &w, nrt_ctx::LaunchSlot *slot, TraverseArgs<T> &a,
                                 unsigned grid) {
  const hipStream_t s = l.stream;
  const bool count = l.kind == Query::Count;
  if (count || (w.dbg & 32u)) HIPCHK(c, hipMemsetAsync(c->d_counters, 0, 16 * sizeof(unsigned long long), s));
  // completion record instead of events: the traversal kernel is the launch's last kernel and events were not asked for
  const bool use_rec = w.wide() && !count && !c->launch_timing;
  // (the sphere kind's u/v pass and the cylinder kind's normal pass run behind the traversal kernel and close the record in its place)
  // (an occlusion query of these kinds has no records to finish: no pass, and the walk's last wave closes the record itself — left
  // to a pass that never runs, wait_for_launches would poll it for ever)
  const bool post_pass = kPrimKinds[c->prim_kind].post_pass && (c->prim_kind != kPrimSpheres || l.hits != nullptr) &&
                         l.kind != Query::OcclusionPrims; // (validate_launch: such a context takes its kind's own query or that one only)
  a.done_rec = use_rec ? slot->d_done : nullptr;
  a.done_count = slot->d_count;
  a.done_seq = use_rec ? slot->seq + 1u : 0u;
  a.done_publish = post_pass ? 0u : 1u;
  const bool timed = l.timed && !use_rec;
  if (timed) HIPCHK(c, hipEventRecord(slot->t0, s));
  if (w.walk == Walk::Motion) {
    HIPCHK(c, launch_traverse_motion<T>(a, c->d_tris1, l.times, grid, s));
    c->last_kernel = sizeof(T) == 4 ? "nrt::k_traverse_motion<float>" : "nrt::k_traverse_motion<double>";
  } else if (w.walk == Walk::MultiHit) {
    HIPCHK(c, launch_traverse_multihit<T>(a, l.max_hits, l.hit_counts, grid, s));
    c->last_kernel = sizeof(T) == 4 ? "nrt::k_traverse_multihit<float>" : "nrt::k_traverse_multihit<double>";
  } else if (w.wide()) {
    HIPCHK(c, launch_traverse_wide<T>(a, grid, w.lds_entries, c->prim_kind, s, &c->last_kernel));
  } else {
    HIPCHK(c, launch_traverse<T>(a, grid, count, c->lds_stack, s));
    c->last_kernel = sizeof(T) == 4 ? "nrt::k_traverse<float>" : "nrt::k_traverse<double>";
  }
  // The kernel is enqueued: the slot's state follows it NOW, before any later call of this function can fail — a launch
  // that is in flight publishes seq + 1 and flips the cursor sets whatever happens to the calls behind it.
  if (use_rec) {
    slot->seq++;
    slot->rec_pending = true;
  }
  slot->last_has_rec = use_rec;
  slot->last_timed = false;
  slot->parity ^= 1u;
  slot->stream = s;
  slot->used = true;
  if (use_rec) c->last_timed_slot = (int)(slot - c->slots);
  if (post_pass) // (fill_launch_args: a.hits / a.mask are the slot's compact records and bits where the pass writes the caller's records)
    HIPCHK(c, launch_post_pass<T>(c->prim_kind, l.rays, a.hits, a.mask, (const T *)c->d_verts, (uint32_t)l.n, l.cyl_hits, l.mask, a.done_rec, a.done_count,
                                  a.done_seq, s));
  if (timed) {
    HIPCHK(c, hipEventRecord(slot->t1, s));
    slot->last_timed = true;
    c->last_timed_slot = (int)(slot - c->slots);
  }
  if (!use_rec) HIPCHK(c, hipEventRecord(slot->done, s));
  return NRT_OK;
}

// Every ray query of the C ABI ends here.  launch_mutex is held from the checks to the last event record.
template <typename T>
static nrt_status traverse_device(nrt_ctx *c, TraverseLaunch<T> l) {
  if (!l.opt) l.opt = &kDefaultTrace;
  std::lock_guard<std::mutex> lock(c->launch_mutex);
  if (l.kind == Query::OcclusionPrims && c->prim_kind == kPrimTriangles) l.kind = Query::Occlusion; // (the same launch, byte for byte)
  nrt_status st = validate_launch(c, l);
  if (st || l.n == 0) return st;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, refit_stream_wait(c, l.stream)); // (a Device refit in flight on another stream)
  nrt_ctx::LaunchSlot *slot = nullptr;
  if ((st = take_slot(c, l.stream, &slot))) return st;
  const WalkChoice w = choose_walk(c, l);
  const GridPlan g = size_grid<T>(c, w, l.n);
  const uint32_t total_threads = g.grid * kTraverseBlock, total_waves = g.grid * (kTraverseBlock / kWave);
  const DistributionPlan d = plan_distribution((uint32_t)l.n, total_waves, g.parts, c->static_pct, c->static_bands, c->static_slice_groups, c->chunk);
  const uint32_t levels = plan_spill_levels(c->tree_depth, w.wide4(), (uint32_t)w.lds_entries);
  if (levels) { // (growing a buffer frees the old one, which waits for every launch in flight)
    if ((st = ensure(c, slot->spill, (size_t)levels * total_threads * sizeof(uint32_t)))) return st;
    if (w.wide() && (st = ensure(c, slot->spill_tmin, (size_t)levels * total_threads * sizeof(T)))) return st;
  }
  if (l.kind == Query::Cylinders || l.kind == Query::Curves) { // compact records + {hit, cap} bits, expanded by the post pass
    if ((st = ensure(c, slot->cyl_hits, (size_t)l.n * sizeof(typename Wire<T>::Hit)))) return st;
    if ((st = ensure(c, slot->cyl_bits, (size_t)l.n))) return st;
  }
  if (w.dbg & 8192u) { // profiling library only: per-wave time stamps of this launch (nrtDebugWaveClocks)
    if ((st = ensure(c, c->b_wave_clock, (size_t)total_waves * kWaveClockWords * sizeof(unsigned long long)))) return st;
    c->wave_clock_waves = total_waves;
  }
  TraverseArgs<T> a;
  fill_walk_args(c, l, w, a);
  fill_launch_args(l, slot, g, d, levels, a);
  return enqueue_launch(c, l, w, slot, a, g.grid);
}

const uint64_t kStagedRays = 1ull << 26; // rays per launch of the staged host paths (keeps staging bounded)
const uint64_t kPiece = 1ull << 19; // rays per pipeline stage of traverse_host (19 MB up, 8 MB down in fp32), and per launch of the motion queries' staged path

// The staged host path of every ray query (the caller holds host_mutex), in pieces of `chunk` rays: upload into st_rays, the launch
// `make(rays in the piece)` asks for, rec_bytes / flag_bytes per ray of st_hits / st_mask back into recs / flags (null: not copied).
// `skip_ids` (may be null): one skip id per ray; every piece's slice of it is uploaded into st_skip beside the piece's rays.
// `times` (may be null; the motion queries): one time per ray, staged and advanced per piece in the same way, into st_times.
template <typename T, typename MakeLaunch>
static nrt_status staged_host_loop(nrt_ctx *c, const typename Wire<T>::Ray *rays, uint64_t n, uint64_t chunk, size_t rec_bytes, size_t flag_bytes,
                                   void *recs, void *flags, MakeLaunch make, const uint32_t *skip_ids = nullptr, const T *times = nullptr) {
  const size_t ray_bytes = sizeof(typename Wire<T>::Ray);
  for (uint64_t off = 0; off < n; off += chunk) {
    const uint64_t m = std::min(chunk, n - off);
    nrt_status st;
    if ((st = ensure(c, c->st_rays, m * ray_bytes)) || (rec_bytes && (st = ensure(c, c->st_hits, m * rec_bytes))) || (st = ensure(c, c->st_mask, m * flag_bytes)))
      return st;
    HIPCHK(c, hipMemcpyAsync(c->st_rays.p, rays + off, m * ray_bytes, hipMemcpyHostToDevice, c->stream));
    if (skip_ids) {
      if ((st = ensure(c, c->st_skip, m * sizeof(uint32_t)))) return st;
      HIPCHK(c, hipMemcpyAsync(c->st_skip.p, skip_ids + off, m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    }
    if (times) {
      if ((st = ensure(c, c->st_times, m * sizeof(T)))) return st;
      HIPCHK(c, hipMemcpyAsync(c->st_times.p, times + off, m * sizeof(T), hipMemcpyHostToDevice, c->stream));
    }
    if ((st = traverse_device<T>(c, make(m)))) return st;
    if (recs) HIPCHK(c, hipMemcpyAsync((char *)recs + off * rec_bytes, c->st_hits.p, m * rec_bytes, hipMemcpyDeviceToHost, c->stream));
    if (flags) HIPCHK(c, hipMemcpyAsync((char *)flags + off * flag_bytes, c->st_mask.p, m * flag_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return NRT_OK;
}
// Is `p` page-locked host memory the device can copy from / to asynchronously (hipHostMalloc / nrtHostAlloc / registered)?
static bool is_pinned_host(const void *p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError(); // (plain malloc'd memory: "invalid value", not an error of ours)
    return false;
  }
  return at.type == hipMemoryTypeHost;
}

// Host entry point.  With pageable caller buffers the copies are staged by the runtime and block the host: upload ->
// trace -> download, one after the other.  With PAGE-LOCKED buffers (nrtHostAlloc) the batch is cut into pieces and
// pipelined over three streams — piece k+1 uploads while piece k is traced and piece k-1 downloads (PCIe is full duplex) —
// so the call approaches the slower of the two copy directions instead of their sum plus the kernel.
template <typename T>
static nrt_status traverse_host(nrt_ctx *c, const typename Wire<T>::Ray *rays, uint64_t n,
                                const nrt_trace_options *opt, typename Wire<T>::Hit *hits, uint8_t *mask, const uint32_t *skip_ids = nullptr,
                                Query kind = Query::Closest, const T *times = nullptr) { // (kind: Closest, or Motion with its `times`, which may be null)
  if (!c) return NRT_ERR_INVALID;
  if (n == 0) return NRT_OK;
  if (!rays || !hits) return fail(c, NRT_ERR_INVALID, "nrtTraverseBatch: NULL rays/hits");
  typedef typename Wire<T>::Ray Ray;
  typedef typename Wire<T>::Hit Hit;
  std::lock_guard<std::mutex> host_lock(c->host_mutex);
  HIPCHK(c, hipSetDevice(c->device));
  if (n >= 2 * kPiece && c->host_pipeline && is_pinned_host(rays) && is_pinned_host(hits) && (!mask || is_pinned_host(mask)) &&
      (!skip_ids || is_pinned_host(skip_ids)) && (!times || is_pinned_host(times))) {
    if (!c->copy_in) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_in, hipStreamNonBlocking));
    if (!c->copy_out) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_out, hipStreamNonBlocking));
    for (int k = 0; k < 2; k++)
      for (hipEvent_t *e : {&c->ev_in[k], &c->ev_tr[k], &c->ev_out[k]})
        if (!*e) HIPCHK(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    nrt_status st;
    if ((st = ensure(c, c->st_rays, 2 * kPiece * sizeof(Ray))) || (st = ensure(c, c->st_hits, 2 * kPiece * sizeof(Hit))) ||
        (st = ensure(c, c->st_mask, 2 * kPiece)) || (skip_ids && (st = ensure(c, c->st_skip, 2 * kPiece * sizeof(uint32_t)))) ||
        (times && (st = ensure(c, c->st_times, 2 * kPiece * sizeof(T)))))
      return st;
    uint64_t piece = 0;
    for (uint64_t off = 0; off < n; off += kPiece, piece++) {
      const uint64_t m = std::min(kPiece, n - off);
      const int b = (int)(piece & 1);
      Ray *d_r = (Ray *)c->st_rays.p + (size_t)b * kPiece;
      Hit *d_h = (Hit *)c->st_hits.p + (size_t)b * kPiece;
      uint8_t *d_m = (uint8_t *)c->st_mask.p + (size_t)b * kPiece;
      uint32_t *d_s = skip_ids ? (uint32_t *)c->st_skip.p + (size_t)b * kPiece : nullptr; // (the piece's slice of the ids travels with its rays)
      T *d_t = times ? (T *)c->st_times.p + (size_t)b * kPiece : nullptr;                 // (... and its slice of the times)
      // the ray slot is free once the trace that read it (two pieces ago) is done; the record slot once its download is
      if (piece >= 2) HIPCHK(c, hipStreamWaitEvent(c->copy_in, c->ev_tr[b], 0));
      HIPCHK(c, hipMemcpyAsync(d_r, rays + off, m * sizeof(Ray), hipMemcpyHostToDevice, c->copy_in));
      if (d_s) HIPCHK(c, hipMemcpyAsync(d_s, skip_ids + off, m * sizeof(uint32_t), hipMemcpyHostToDevice, c->copy_in));
      if (d_t) HIPCHK(c, hipMemcpyAsync(d_t, times + off, m * sizeof(T), hipMemcpyHostToDevice, c->copy_in));
      HIPCHK(c, hipEventRecord(c->ev_in[b], c->copy_in));
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_in[b], 0));
      if (piece >= 2) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_out[b], 0));
      st = traverse_device<T>(c, {.kind = kind, .rays = d_r, .n = m, .opt = opt, .stream = c->stream, .timed = true, .hits = d_h, .mask = d_m,
                                  .skip_ids = d_s, .times = d_t});
      if (st) { // (copies into the caller's buffers may still be in flight: let them land before the call returns)
        (void)hipStreamSynchronize(c->copy_in);
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamSynchronize(c->copy_out);
        return st;
      }
      HIPCHK(c, hipEventRecord(c->ev_tr[b], c->stream));
      HIPCHK(c, hipStreamWaitEvent(c->copy_out, c->ev_tr[b], 0));
      HIPCHK(c, hipMemcpyAsync(hits + off, d_h, m * sizeof(Hit), hipMemcpyDeviceToHost, c->copy_out));
      if (mask) HIPCHK(c, hipMemcpyAsync(mask + off, d_m, m, hipMemcpyDeviceToHost, c->copy_out));
      HIPCHK(c, hipEventRecord(c->ev_out[b], c->copy_out));
    }
    HIPCHK(c, hipStreamSynchronize(c->copy_out));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return NRT_OK;
  }
  // (the motion queries go in pieces of kPiece rays here too: their staging stays as small as the pipeline's)
  return staged_host_loop<T>(c, rays, n, kind == Query::Motion ? kPiece : kStagedRays, sizeof(Hit), 1, hits, mask, [&](uint64_t m) -> TraverseLaunch<T> {
    return {.kind = kind, .rays = (const Ray *)c->st_rays.p, .n = m, .opt = opt, .stream = c->stream, .timed = true,
            .hits = (Hit *)c->st_hits.p, .mask = (uint8_t *)c->st_mask.p, .skip_ids = skip_ids ? (const uint32_t *)c->st_skip.p : nullptr,
            .times = times ? (const T *)c->st_times.p : nullptr};
  }, skip_ids, times);
}

// One host batch spread over several contexts — one per GPU of the node, each holding the same tree (the build is
// deterministic: replicas are bit-identical).  The batch is cut into rows of `row_len` rays (an image row; 4096 rays when 0) and
// row r goes to context r % num_ctx — interleaved, so that no device gets the empty sky or the dense ground alone.  Every
// context is driven by a host thread of its own: strided copy of its rows up (one 2-D copy), one launch, strided copies of its
// records and flags straight into the caller's arrays.  No collective: the results are host-resident and every GPU writes its
// own rows of them.  Records are exactly those of a single-context nrtTraverseBatch over the whole batch.
template <typename T>
static nrt_status traverse_share(nrt_ctx *c, uint32_t k, uint32_t num_ctx, const typename Wire<T>::Ray *rays, uint64_t n, uint64_t row_len,
                                 const nrt_trace_options *opt, typename Wire<T>::Hit *hits, uint8_t *mask) {
  typedef typename Wire<T>::Ray Ray;
  typedef typename Wire<T>::Hit Hit;
  const uint64_t rows_total = (n + row_len - 1) / row_len;
  if (k >= rows_total) return NRT_OK;
  const uint64_t my_rows = (rows_total - k + num_ctx - 1) / num_ctx; // rows k, k + num_ctx, ...
  const uint64_t last_row = k + (my_rows - 1) * num_ctx;
  const uint64_t last_len = (last_row == rows_total - 1) ? n - last_row * row_len : row_len; // only the batch's final row can be short
  const uint64_t full_rows = last_len == row_len ? my_rows : my_rows - 1;
  const uint64_t m = full_rows * row_len + (full_rows < my_rows ? last_len : 0);
  std::lock_guard<std::mutex> host_lock(c->host_mutex);
  HIPCHK(c, hipSetDevice(c->device));
  nrt_status st;
  if ((st = ensure(c, c->st_rays, m * sizeof(Ray))) || (st = ensure(c, c->st_hits, m * sizeof(Hit))) || (st = ensure(c, c->st_mask, m))) return st;
  Ray *d_r = (Ray *)c->st_rays.p;
  Hit *d_h = (Hit *)c->st_hits.p;
  uint8_t *d_m = (uint8_t *)c->st_mask.p;
  const size_t rb = (size_t)row_len * sizeof(Ray), hb = (size_t)row_len * sizeof(Hit), mbytes = (size_t)row_len;
  if (full_rows) HIPCHK(c, hipMemcpy2DAsync(d_r, rb, rays + k * row_len, rb * num_ctx, rb, full_rows, hipMemcpyHostToDevice, c->stream));
  if (full_rows < my_rows)
    HIPCHK(c, hipMemcpyAsync(d_r + full_rows * row_len, rays + last_row * row_len, last_len * sizeof(Ray), hipMemcpyHostToDevice, c->stream));
  if ((st = traverse_device<T>(c, {.kind = Query::Closest, .rays = d_r, .n = m, .opt = opt, .stream = c->stream, .hits = d_h, .mask = d_m}))) return st;
  if (full_rows) {
    HIPCHK(c, hipMemcpy2DAsync(hits + k * row_len, hb * num_ctx, d_h, hb, hb, full_rows, hipMemcpyDeviceToHost, c->stream));
    if (mask) HIPCHK(c, hipMemcpy2DAsync(mask + k * row_len, mbytes * num_ctx, d_m, mbytes, mbytes, full_rows, hipMemcpyDeviceToHost, c->stream));
  }
  if (full_rows < my_rows) {
    HIPCHK(c, hipMemcpyAsync(hits + last_row * row_len, d_h + full_rows * row_len, last_len * sizeof(Hit), hipMemcpyDeviceToHost, c->stream));
    if (mask) HIPCHK(c, hipMemcpyAsync(mask + last_row * row_len, d_m + full_rows * row_len, last_len, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NRT_OK;
}

template <typename T>
static nrt_status traverse_multi(nrt_ctx *const *ctxs, uint32_t num_ctx, const typename Wire<T>::Ray *rays, uint64_t n, uint64_t row_len,
                                 const nrt_trace_options *opt, typename Wire<T>::Hit *hits, uint8_t *mask) {
  if (!ctxs || num_ctx == 0 || !ctxs[0]) return NRT_ERR_INVALID;
  nrt_ctx *c0 = ctxs[0];
  if (n == 0) return NRT_OK;
  if (!rays || !hits) return fail(c0, NRT_ERR_INVALID, "nrtTraverseBatchMulti: NULL rays/hits");
  for (uint32_t k = 0; k < num_ctx; k++) {
    if (!ctxs[k]) return fail(c0, NRT_ERR_INVALID, "nrtTraverseBatchMulti: context %u is NULL", k);
    for (uint32_t j = 0; j < k; j++)
      if (ctxs[j] == ctxs[k]) return fail(c0, NRT_ERR_INVALID, "nrtTraverseBatchMulti: context %u is listed twice", k);
    if (ctxs[k]->prec != (int)sizeof(T) || !ctxs[k]->d_nodes || ctxs[k]->prim_kind != kPrimTriangles)
      return fail(c0, NRT_ERR_INVALID, "nrtTraverseBatchMulti: context %u holds no triangle tree of this precision", k);
    if (ctxs[k]->num_nodes != c0->num_nodes || ctxs[k]->num_indices != c0->num_indices)
      return fail(c0, NRT_ERR_INVALID, "nrtTraverseBatchMulti: context %u holds another tree (%llu nodes, context 0 has %llu)", k,
                  (unsigned long long)ctxs[k]->num_nodes, (unsigned long long)c0->num_nodes);
  }
  if (row_len == 0) row_len = 4096;
  if (num_ctx == 1) return traverse_host<T>(c0, rays, n, opt, hits, mask);
  std::vector<nrt_status> st(num_ctx, NRT_OK);
  std::vector<std::thread> th;
  for (uint32_t k = 1; k < num_ctx; k++)
    th.emplace_back([&, k]() { st[k] = traverse_share<T>(ctxs[k], k, num_ctx, rays, n, row_len, opt, hits, mask); });
  st[0] = traverse_share<T>(c0, 0, num_ctx, rays, n, row_len, opt, hits, mask);
  for (std::thread &t : th) t.join();
  for (uint32_t k = 0; k < num_ctx; k++)
    if (st[k]) {
      if (k) c0->err = "context " + std::to_string(k) + ": " + ctxs[k]->err;
      return st[k];
    }
  return NRT_OK;
}

template <typename T>
static nrt_status traverse_count(nrt_ctx *c, const typename Wire<T>::Ray *d_rays, uint64_t n,
                                 const nrt_trace_options *opt, nrt_trace_counters *out) {
  if (!c || !out) return NRT_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  nrt_status st = traverse_device<T>(c, {.kind = Query::Count, .rays = d_rays, .n = n, .opt = opt, .stream = c->stream});
  if (st) return st;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  unsigned long long h[4];
  HIPCHK(c, hipMemcpy(h, c->d_counters, sizeof(h), hipMemcpyDeviceToHost));
  out->nodes_visited = h[0];
  out->leaves_tested = h[1];
  out->tris_tested = h[2];
  out->max_stack = h[3];
  return NRT_OK;
}

// The batch tables of nrtTraverseBatches* (`fn`: the entry point the messages name): a non-empty batch has rays, an occlusion batch
// its flag array, a closest-hit batch its record array (a call of occlusion batches only may pass no record table).  Counts the rays.
template <typename T>
static nrt_status check_batches(nrt_ctx *c, const char *fn, uint32_t nb, const typename Wire<T>::Ray *const *rays, const uint64_t *counts,
                                typename Wire<T>::Hit *const *hits, uint8_t *const *masks, const uint32_t *flags, uint64_t *total,
                                uint64_t *total_closest) {
  *total = *total_closest = 0;
  if (!rays || !counts) return fail(c, NRT_ERR_INVALID, "%s: NULL argument", fn);
  for (uint32_t k = 0; k < nb; k++) {
    if (!counts[k]) continue;
    const bool occ = flags && (flags[k] & NRT_BATCH_OCCLUSION);
    if (!rays[k]) return fail(c, NRT_ERR_INVALID, "%s: batch %u has no rays", fn, k);
    if (occ && !(masks && masks[k])) return fail(c, NRT_ERR_INVALID, "%s: occlusion batch %u has no flag array", fn, k);
    if (!occ && !(hits && hits[k])) return fail(c, NRT_ERR_INVALID, "%s: batch %u has no hit array", fn, k);
    *total += counts[k];
    if (!occ) *total_closest += counts[k];
  }
  return NRT_OK;
}

// One persistent launch over several independent batches (same trace options): the claim machinery hands out one virtual
// array, so the waves that run dry at the end of one batch carry on with the next — one tail and one completion record for
// all.  Contexts that cannot (fp64, custom primitives, the literal kernel) launch the batches one after the other on the
// same stream: the records are the same either way.
template <typename T>
static nrt_status traverse_batches_device(nrt_ctx *c, uint32_t nb, const typename Wire<T>::Ray *const *d_rays, const uint64_t *counts,
                                          const nrt_trace_options *opt, typename Wire<T>::Hit *const *d_hits,
                                          uint8_t *const *d_masks, const uint32_t *flags, hipStream_t s, const uint32_t *const *d_skip = nullptr) {
  if (!c) return NRT_ERR_INVALID;
  if (nb == 0) return NRT_OK;
  uint64_t total, total_closest;
  const nrt_status bad = check_batches<T>(c, "nrtTraverseBatchesDevice", nb, d_rays, counts, d_hits, d_masks, flags, &total, &total_closest);
  if (bad || total == 0) return bad;
  TraverseBatches<T> mb;
  const bool one_launch = sizeof(T) == 4 && c->prec == 4 && c->prim_kind == kPrimTriangles && c->wide && c->d_wide && total <= 0x7FFFFFFFull;
  uint32_t k = 0;
  while (k < nb) { // groups of up to kMaxBatches non-empty batches per launch
    mb.nb = 0;
    mb.anyhit = 0;
    uint64_t n = 0;
    while (k < nb && mb.nb < (uint32_t)kMaxBatches) {
      if (counts[k]) {
        const bool occ = flags && (flags[k] & NRT_BATCH_OCCLUSION);
        mb.rays[mb.nb] = d_rays[k];
        mb.hits[mb.nb] = occ ? nullptr : d_hits[k]; // (an occlusion query writes the flags only: its call may have no record table)
        mb.mask[mb.nb] = d_masks ? d_masks[k] : nullptr;
        mb.count[mb.nb] = counts[k];
        mb.skip[mb.nb] = d_skip ? d_skip[k] : nullptr;
        if (occ) mb.anyhit |= 1u << mb.nb;
        n += counts[k];
        mb.nb++;
      }
      k++;
    }
    if (mb.nb == 0) break;
    nrt_status st;
    if (one_launch && mb.nb > 1) {
      st = traverse_device<T>(c, {.kind = Query::MultiBatch, .rays = mb.rays[0], .n = n, .opt = opt, .stream = s, .hits = mb.hits[0],
                                  .mask = mb.mask[0], .batches = &mb}); // (rays / hits / mask: the first batch's — the kernel reads the table)
      if (st) return st;
    } else {
      for (uint32_t j = 0; j < mb.nb; j++) {
        const Query kind = ((mb.anyhit >> j) & 1u) ? Query::Occlusion : Query::Closest;
        st = traverse_device<T>(c, {.kind = kind, .rays = mb.rays[j], .n = mb.count[j], .opt = opt, .stream = s, .hits = mb.hits[j], .mask = mb.mask[j],
                                    .skip_ids = mb.skip[j]});
        if (st) return st;
      }
    }
  }
  return NRT_OK;
}

// The same for HOST batches (nrtTraverseBatches): every batch is staged next to the others, ONE launch walks them all (one
// launch tail: a host renderer's shadow query of one depth and its path wave of the next), the records come back batch by
// batch.  Like nrtTraverseBatch the staging buffers are the context's: one host call at a time.
template <typename T>
static nrt_status traverse_batches_host(nrt_ctx *c, uint32_t nb, const typename Wire<T>::Ray *const *rays, const uint64_t *counts,
                                        const nrt_trace_options *opt, typename Wire<T>::Hit *const *hits, uint8_t *const *masks,
                                        const uint32_t *flags, const uint32_t *const *skip_ids = nullptr) {
  typedef typename Wire<T>::Ray Ray;
  typedef typename Wire<T>::Hit Hit;
  if (!c) return NRT_ERR_INVALID;
  if (nb == 0) return NRT_OK;
  uint64_t total, total_closest; // (record staging is sized over the closest-hit batches only)
  nrt_status st = check_batches<T>(c, "nrtTraverseBatches", nb, rays, counts, hits, masks, flags, &total, &total_closest);
  if (st || total == 0) return st;
  if (total > kStagedRays) return fail(c, NRT_ERR_INVALID, "nrtTraverseBatches: more than 2^26 rays in one call");
  std::lock_guard<std::mutex> host_lock(c->host_mutex);
  HIPCHK(c, hipSetDevice(c->device));
  if ((st = ensure(c, c->st_rays, total * sizeof(Ray))) || (st = ensure(c, c->st_hits, std::max<uint64_t>(1, total_closest) * sizeof(Hit))) ||
      (st = ensure(c, c->st_mask, total)) || (skip_ids && (st = ensure(c, c->st_skip, total * sizeof(uint32_t)))))
    return st;
  std::vector<const uint32_t *> d_s(nb, nullptr); // (a batch's ids are staged at its rays' offset)
  std::vector<const Ray *> d_r(nb, nullptr);
  std::vector<Hit *> d_h(nb, nullptr);
  std::vector<uint8_t *> d_m(nb, nullptr);
  uint64_t off = 0, off_closest = 0;
  for (uint32_t k = 0; k < nb; k++) {
    if (!counts[k]) continue;
    const bool occ = flags && (flags[k] & NRT_BATCH_OCCLUSION);
    d_r[k] = (const Ray *)c->st_rays.p + off;
    if (!occ) {
      d_h[k] = (Hit *)c->st_hits.p + off_closest;
      off_closest += counts[k];
    }
    d_m[k] = (uint8_t *)c->st_mask.p + off;
    HIPCHK(c, hipMemcpyAsync((void *)d_r[k], rays[k], counts[k] * sizeof(Ray), hipMemcpyHostToDevice, c->stream));
    if (skip_ids && skip_ids[k]) {
      d_s[k] = (const uint32_t *)c->st_skip.p + off;
      HIPCHK(c, hipMemcpyAsync((void *)d_s[k], skip_ids[k], counts[k] * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    }
    off += counts[k];
  }
  st = traverse_batches_device<T>(c, nb, d_r.data(), counts, opt, d_h.data(), d_m.data(), flags, c->stream, skip_ids ? d_s.data() : nullptr);
  if (st) {
    (void)hipStreamSynchronize(c->stream);
    return st;
  }
  for (uint32_t k = 0; k < nb; k++) {
    if (!counts[k]) continue;
    const bool occ = flags && (flags[k] & NRT_BATCH_OCCLUSION);
    if (!occ) HIPCHK(c, hipMemcpyAsync(hits[k], d_h[k], counts[k] * sizeof(Hit), hipMemcpyDeviceToHost, c->stream));
    if (masks && masks[k]) HIPCHK(c, hipMemcpyAsync(masks[k], d_m[k], counts[k], hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NRT_OK;
}

template <typename T>
static nrt_status occluded_host(nrt_ctx *c, const typename Wire<T>::Ray *rays, uint64_t n, const nrt_trace_options *opt, uint8_t *mask,
                                const uint32_t *skip_ids = nullptr, Query kind = Query::Occlusion, const T *times = nullptr) {
  if (!c) return NRT_ERR_INVALID;
  if (n == 0) return NRT_OK;
  if (!rays || !mask) return fail(c, NRT_ERR_INVALID, "nrtOccludedBatch: NULL rays/mask");
  std::lock_guard<std::mutex> host_lock(c->host_mutex);
  HIPCHK(c, hipSetDevice(c->device));
  const uint64_t chunk = kind == Query::MotionOcclusion ? kPiece : kStagedRays; // (motion: traverse_host's pieces)
  return staged_host_loop<T>(c, rays, n, chunk, 0, 1, nullptr, mask, [&](uint64_t m) -> TraverseLaunch<T> {
    return {.kind = kind, .rays = (const typename Wire<T>::Ray *)c->st_rays.p, .n = m, .opt = opt, .stream = c->stream, .timed = true,
            .mask = (uint8_t *)c->st_mask.p, .skip_ids = skip_ids ? (const uint32_t *)c->st_skip.p : nullptr,
            .times = times ? (const T *)c->st_times.p : nullptr};
  }, skip_ids, times);
}

// ---------------------------------------------------------------------------
// multi-hit (include/nanort_hip.h, nrtMultiHitTraverseBatch*)
// ---------------------------------------------------------------------------
template <typename T>
static nrt_status multihit_check(nrt_ctx *c, const void *rays, uint64_t n, uint32_t max_hits, const void *hits) {
  if (!c->d_nodes) return fail(c, NRT_ERR_INVALID, "nrtMultiHitTraverseBatch: no tree (call nrtBuild or nrtSetTree)");
  if (c->prec != (int)sizeof(T)) return fail(c, NRT_ERR_PRECISION, "nrtMultiHitTraverseBatch: precision mismatch");
  if (max_hits == 0u || max_hits > NRT_MAX_MULTIHIT)
    return fail(c, NRT_ERR_INVALID, "nrtMultiHitTraverseBatch: max_hits %u outside 1..%u", max_hits, NRT_MAX_MULTIHIT);
  if (c->prim_kind != kPrimTriangles) return fail(c, NRT_ERR_INVALID, "nrtMultiHitTraverseBatch: triangle contexts only");
  if (n == 0) return NRT_OK;
  if (!rays || !hits) return fail(c, NRT_ERR_INVALID, "nrtMultiHitTraverseBatch: NULL rays/hits");
  if (n > 0x7FFFFFFFull) return fail(c, NRT_ERR_INVALID, "nrtMultiHitTraverseBatch: more than 2^31-1 rays in one call");
  return NRT_OK;
}

template <typename T>
static nrt_status multihit_device(nrt_ctx *c, const typename Wire<T>::Ray *d_rays, uint64_t n, uint32_t max_hits, const nrt_trace_options *opt,
                                  typename Wire<T>::Hit *d_hits, uint32_t *d_counts, hipStream_t s) {
  if (!c) return NRT_ERR_INVALID;
  nrt_status st = multihit_check<T>(c, d_rays, n, max_hits, d_hits);
  if (st || n == 0) return st;
  return traverse_device<T>(c, {.kind = Query::MultiHit, .rays = d_rays, .n = n, .opt = opt, .stream = s, .timed = true, .hits = d_hits,
                                .max_hits = max_hits, .hit_counts = d_counts});
}

template <typename T>
static nrt_status multihit_host(nrt_ctx *c, const typename Wire<T>::Ray *rays, uint64_t n, uint32_t max_hits, const nrt_trace_options *opt,
                                typename Wire<T>::Hit *hits, uint32_t *counts) {
  if (!c) return NRT_ERR_INVALID;
  nrt_status st = multihit_check<T>(c, rays, n, max_hits, hits);
  if (st || n == 0) return st;
  typedef typename Wire<T>::Ray Ray;
  typedef typename Wire<T>::Hit Hit;
  std::lock_guard<std::mutex> host_lock(c->host_mutex);
  HIPCHK(c, hipSetDevice(c->device));
  // rays per launch: the staged records stay within 256 MiB whatever K is
  const uint64_t chunk = std::max<uint64_t>(1u, std::min<uint64_t>(1ull << 26, (256ull << 20) / ((uint64_t)max_hits * sizeof(Hit))));
  return staged_host_loop<T>(c, rays, n, chunk, max_hits * sizeof(Hit), sizeof(uint32_t), hits, counts, [&](uint64_t m) -> TraverseLaunch<T> {
    return {.kind = Query::MultiHit, .rays = (const Ray *)c->st_rays.p, .n = m, .opt = opt, .stream = c->stream, .timed = true,
            .hits = (Hit *)c->st_hits.p, .max_hits = max_hits, .hit_counts = counts ? (uint32_t *)c->st_mask.p : nullptr};
  });
}

// ---------------------------------------------------------------------------
// motion blur (include/nanort_hip.h, nrtSetMeshMotion* / nrt*BatchMotion*)
// ---------------------------------------------------------------------------
// The second vertex keyframe of the context's triangle mesh, from host memory or (`device`: read on `s`) from HBM, into the context's
// own tight array through launch_gather_vertices.  Every refusal comes before anything changes or is enqueued; then the tree goes
// (its boxes and leaf records belong to the keyframes it was built over) and the call returns when the context owns its copy.
// `vertices` == NULL removes the keyframe.
template <typename T>
static nrt_status set_mesh_motion(nrt_ctx *c, const T *vertices, uint32_t num_vertices, size_t stride, bool device, hipStream_t s) {
  const char *fn = device ? "nrtSetMeshMotionDevice" : "nrtSetMeshMotion";
  if (!c) return NRT_ERR_INVALID;
  if (c->prec != 0 && c->prec != (int)sizeof(T))
    return fail(c, NRT_ERR_PRECISION, "%s: the context holds %s primitives", fn, c->prec == 8 ? "f64" : "f32");
  if (c->prec == 0 || c->prim_kind != kPrimTriangles || !c->d_verts || c->num_faces == 0)
    return fail(c, NRT_ERR_INVALID, "%s: set a triangle mesh first (nrtSetMesh): the keyframe shares its faces and its vertex count", fn);
  if (vertices) {
    if (stride < 3 * sizeof(T)) return fail(c, NRT_ERR_INVALID, "%s: vertex stride %zu < %zu", fn, stride, 3 * sizeof(T));
    if (device && (stride % sizeof(T) != 0 || (uintptr_t)vertices % sizeof(T) != 0))
      return fail(c, NRT_ERR_INVALID, "%s: vertex stride %zu or pointer not aligned to %zu bytes", fn, stride, sizeof(T));
    // (the faces were validated against num_verts when the mesh was set: a block of that many rows is all the gather reads — what
    // DESIGN 3.7 asks of nrtSetMeshDevice, without an index reduction)
    if (device && num_vertices < c->num_verts)
      return fail(c, NRT_ERR_INVALID, "%s: the vertex block holds %u rows, the context's mesh has %u vertices", fn, num_vertices, c->num_verts);
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, wait_for_launches(c));
  free_tree(c); // (bumps generation)
  c->d_verts1 = nullptr;
  if (!vertices) return NRT_OK;
  const uint32_t nv = c->num_verts;
  if (nrt_status st = ensure(c, c->b_verts1, 3 * (size_t)nv * sizeof(T))) return st;
  if (!device) s = c->stream;
  const void *src = vertices;
  if (!device) { // the caller's block, as it lies, into the staging buffer the host refit uses
    const size_t block = (size_t)(nv - 1) * stride + 3 * sizeof(T);
    if (nrt_status st = ensure(c, c->b_refit_stage, block)) return st;
    HIPCHK(c, hipMemcpyAsync(c->b_refit_stage.p, vertices, block, hipMemcpyHostToDevice, s));
    src = c->b_refit_stage.p;
  }
  HIPCHK(c, launch_gather_vertices<T>(src, stride, nv, (T *)c->b_verts1.p, s));
  HIPCHK(c, hipStreamSynchronize(s)); // the context owns its copy: the caller's buffer is free again
  c->d_verts1 = c->b_verts1.p;
  return NRT_OK;
}

template <typename T>
static nrt_status traverse_motion_host(nrt_ctx *c, const typename Wire<T>::Ray *r, const T *times, uint64_t n, const nrt_trace_options *o,
                                       typename Wire<T>::Hit *h, uint8_t *m) {
  return traverse_host<T>(c, r, n, o, h, m, nullptr, Query::Motion, times);
}
template <typename T>
static nrt_status traverse_motion_device(nrt_ctx *c, const typename Wire<T>::Ray *r, const T *times, uint64_t n, const nrt_trace_options *o,
                                         typename Wire<T>::Hit *h, uint8_t *m, void *s) {
  if (!c) return NRT_ERR_INVALID;
  if (n && !h) return fail(c, NRT_ERR_INVALID, "nrtTraverseBatchMotionDevice: NULL hits");
  return traverse_device<T>(c, {.kind = Query::Motion, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true, .hits = h, .mask = m,
                                .times = times});
}
template <typename T>
static nrt_status occluded_motion_device(nrt_ctx *c, const typename Wire<T>::Ray *r, const T *times, uint64_t n, const nrt_trace_options *o,
                                         uint8_t *m, void *s) {
  if (!c) return NRT_ERR_INVALID;
  if (n && !m) return fail(c, NRT_ERR_INVALID, "nrtOccludedBatchMotionDevice: NULL mask");
  return traverse_device<T>(c, {.kind = Query::MotionOcclusion, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true, .mask = m,
                                .times = times});
}

// Per-ray skip ids (include/nanort_hip.h): the entry points above with one skip id per ray; a NULL array is the call above itself.
template <typename T>
static nrt_status traverse_skip_device(nrt_ctx *c, const typename Wire<T>::Ray *r, uint64_t n, const nrt_trace_options *o, const uint32_t *ids,
                                       typename Wire<T>::Hit *h, uint8_t *m, void *s) {
  if (!c) return NRT_ERR_INVALID;
  if (n && !h) return fail(c, NRT_ERR_INVALID, "nrtTraverseBatchSkipDevice: NULL hits");
  return traverse_device<T>(c, {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true, .hits = h, .mask = m,
                                .skip_ids = ids});
}
template <typename T>
static nrt_status occluded_skip_device(nrt_ctx *c, const typename Wire<T>::Ray *r, uint64_t n, const nrt_trace_options *o, const uint32_t *ids,
                                       uint8_t *m, void *s) {
  if (!c) return NRT_ERR_INVALID;
  if (n && !m) return fail(c, NRT_ERR_INVALID, "nrtOccludedBatchSkipDevice: NULL mask");
  return traverse_device<T>(c, {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true, .mask = m, .skip_ids = ids});
}
extern "C" {

nrt_status nrtMultiHitTraverseBatch_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, uint32_t k, const nrt_trace_options *o, nrt_hit_f32 *h,
                                        uint32_t *cnt) {
  return multihit_host<float>(c, r, n, k, o, h, cnt);
}
nrt_status nrtMultiHitTraverseBatch_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, uint32_t k, const nrt_trace_options *o, nrt_hit_f64 *h,
                                        uint32_t *cnt) {
  return multihit_host<double>(c, r, n, k, o, h, cnt);
}
nrt_status nrtMultiHitTraverseBatchDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, uint32_t k, const nrt_trace_options *o,
                                              nrt_hit_f32 *h, uint32_t *cnt, void *s) {
  return multihit_device<float>(c, r, n, k, o, h, cnt, (hipStream_t)s);
}
nrt_status nrtMultiHitTraverseBatchDevice_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, uint32_t k, const nrt_trace_options *o,
                                              nrt_hit_f64 *h, uint32_t *cnt, void *s) {
  return multihit_device<double>(c, r, n, k, o, h, cnt, (hipStream_t)s);
}

nrt_status nrtSetMeshMotion_f32(nrt_ctx *c, const float *v, size_t stride) { return set_mesh_motion<float>(c, v, 0, stride, false, nullptr); }
nrt_status nrtSetMeshMotion_f64(nrt_ctx *c, const double *v, size_t stride) { return set_mesh_motion<double>(c, v, 0, stride, false, nullptr); }
nrt_status nrtSetMeshMotionDevice_f32(nrt_ctx *c, const float *v, uint32_t nv, size_t stride, void *s) {
  return set_mesh_motion<float>(c, v, nv, stride, true, (hipStream_t)s);
}
nrt_status nrtSetMeshMotionDevice_f64(nrt_ctx *c, const double *v, uint32_t nv, size_t stride, void *s) {
  return set_mesh_motion<double>(c, v, nv, stride, true, (hipStream_t)s);
}
nrt_status nrtTraverseBatchMotion_f32(nrt_ctx *c, const nrt_ray_f32 *r, const float *t, uint64_t n, const nrt_trace_options *o, nrt_hit_f32 *h,
                                      uint8_t *m) {
  return traverse_motion_host<float>(c, r, t, n, o, h, m);
}
nrt_status nrtTraverseBatchMotion_f64(nrt_ctx *c, const nrt_ray_f64 *r, const double *t, uint64_t n, const nrt_trace_options *o, nrt_hit_f64 *h,
                                      uint8_t *m) {
  return traverse_motion_host<double>(c, r, t, n, o, h, m);
}
nrt_status nrtTraverseBatchMotionDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, const float *t, uint64_t n, const nrt_trace_options *o,
                                            nrt_hit_f32 *h, uint8_t *m, void *s) {
  return traverse_motion_device<float>(c, r, t, n, o, h, m, s);
}
nrt_status nrtTraverseBatchMotionDevice_f64(nrt_ctx *c, const nrt_ray_f64 *r, const double *t, uint64_t n, const nrt_trace_options *o,
                                            nrt_hit_f64 *h, uint8_t *m, void *s) {
  return traverse_motion_device<double>(c, r, t, n, o, h, m, s);
}
nrt_status nrtOccludedBatchMotion_f32(nrt_ctx *c, const nrt_ray_f32 *r, const float *t, uint64_t n, const nrt_trace_options *o, uint8_t *m) {
  return occluded_host<float>(c, r, n, o, m, nullptr, Query::MotionOcclusion, t);
}
nrt_status nrtOccludedBatchMotion_f64(nrt_ctx *c, const nrt_ray_f64 *r, const double *t, uint64_t n, const nrt_trace_options *o, uint8_t *m) {
  return occluded_host<double>(c, r, n, o, m, nullptr, Query::MotionOcclusion, t);
}
nrt_status nrtOccludedBatchMotionDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, const float *t, uint64_t n, const nrt_trace_options *o, uint8_t *m,
                                            void *s) {
  return occluded_motion_device<float>(c, r, t, n, o, m, s);
}
nrt_status nrtOccludedBatchMotionDevice_f64(nrt_ctx *c, const nrt_ray_f64 *r, const double *t, uint64_t n, const nrt_trace_options *o, uint8_t *m,
                                            void *s) {
  return occluded_motion_device<double>(c, r, t, n, o, m, s);
}

nrt_status nrtRefit_f32(nrt_ctx *c, const float *v, size_t stride) { return refit<float>(c, v, stride, false, nullptr); }
nrt_status nrtRefit_f64(nrt_ctx *c, const double *v, size_t stride) { return refit<double>(c, v, stride, false, nullptr); }
nrt_status nrtRefitDevice_f32(nrt_ctx *c, const float *v, size_t stride, void *s) { return refit<float>(c, v, stride, true, (hipStream_t)s); }
nrt_status nrtRefitDevice_f64(nrt_ctx *c, const double *v, size_t stride, void *s) { return refit<double>(c, v, stride, true, (hipStream_t)s); }
nrt_status nrtRefitPrims_f32(nrt_ctx *c, const float *p, const float *r, uint32_t n) { return refit_prims(c, p, r, n, false, nullptr); }
nrt_status nrtRefitPrimsDevice_f32(nrt_ctx *c, const float *p, const float *r, uint32_t n, void *s) { return refit_prims(c, p, r, n, true, (hipStream_t)s); }

nrt_status nrtSetMesh_f32(nrt_ctx *c, const float *v, size_t stride, const uint32_t *f, uint32_t nf) {
  return set_mesh<float>(c, v, stride, f, nf);
}
nrt_status nrtSetMesh_f64(nrt_ctx *c, const double *v, size_t stride, const uint32_t *f, uint32_t nf) {
  return set_mesh<double>(c, v, stride, f, nf);
}

nrt_status nrtSetCylinders_f32(nrt_ctx *c, const float *endpoints, const float *radii, uint32_t n, int test_cap) {
  return set_cylinders(c, endpoints, radii, n, test_cap);
}

nrt_status nrtTraverseBatchCylindersDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o,
                                               nrt_cyl_hit_f32 *h, uint8_t *m, void *s) {
  if (!c) return NRT_ERR_INVALID;
  if (n && !h) return fail(c, NRT_ERR_INVALID, "nrtTraverseBatchCylindersDevice: NULL hits");
  return traverse_device<float>(c, {.kind = Query::Cylinders, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true, .mask = m,
                                    .cyl_hits = h});
}

nrt_status nrtTraverseBatchCylinders_f32(nrt_ctx *c, const nrt_ray_f32 *rays, uint64_t n, const nrt_trace_options *opt,
                                         nrt_cyl_hit_f32 *hits, uint8_t *mask) {
  if (!c) return NRT_ERR_INVALID;
  if (n == 0) return NRT_OK;
  if (!rays || !hits) return fail(c, NRT_ERR_INVALID, "nrtTraverseBatchCylinders: NULL rays/hits");
  std::lock_guard<std::mutex> host_lock(c->host_mutex);
  HIPCHK(c, hipSetDevice(c->device));
  return staged_host_loop<float>(c, rays, n, kStagedRays, sizeof(nrt_cyl_hit_f32), 1, hits, mask, [&](uint64_t m) -> TraverseLaunch<float> {
    return {.kind = Query::Cylinders, .rays = (const nrt_ray_f32 *)c->st_rays.p, .n = m, .opt = opt, .stream = c->stream, .timed = true,
            .mask = (uint8_t *)c->st_mask.p, .cyl_hits = c->st_hits.p};
  });
}

nrt_status nrtSetCurves_f32(nrt_ctx *c, const float *cps, const float *radii, uint32_t n, uint32_t subdiv) {
  return set_curves(c, cps, radii, n, subdiv, false, nullptr);
}
nrt_status nrtSetCurvesDevice_f32(nrt_ctx *c, const float *cps, const float *radii, uint32_t n, uint32_t subdiv, void *s) {
  return set_curves(c, cps, radii, n, subdiv, true, (hipStream_t)s);
}

nrt_status nrtTraverseBatchCurvesDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, nrt_curve_hit_f32 *h,
                                            uint8_t *m, void *s) {
  if (!c) return NRT_ERR_INVALID;
  if (n && !h) return fail(c, NRT_ERR_INVALID, "nrtTraverseBatchCurvesDevice: NULL hits");
  return traverse_device<float>(c, {.kind = Query::Curves, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true, .mask = m,
                                    .cyl_hits = h});
}

nrt_status nrtTraverseBatchCurves_f32(nrt_ctx *c, const nrt_ray_f32 *rays, uint64_t n, const nrt_trace_options *opt, nrt_curve_hit_f32 *hits,
                                      uint8_t *mask) {
  if (!c) return NRT_ERR_INVALID;
  if (n == 0) return NRT_OK;
  if (!rays || !hits) return fail(c, NRT_ERR_INVALID, "nrtTraverseBatchCurves: NULL rays/hits");
  std::lock_guard<std::mutex> host_lock(c->host_mutex);
  HIPCHK(c, hipSetDevice(c->device));
  return staged_host_loop<float>(c, rays, n, kStagedRays, sizeof(nrt_curve_hit_f32), 1, hits, mask, [&](uint64_t m) -> TraverseLaunch<float> {
    return {.kind = Query::Curves, .rays = (const nrt_ray_f32 *)c->st_rays.p, .n = m, .opt = opt, .stream = c->stream, .timed = true,
            .mask = (uint8_t *)c->st_mask.p, .cyl_hits = c->st_hits.p};
  });
}

nrt_status nrtOccludedBatch_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, uint8_t *m) {
  return occluded_host<float>(c, r, n, o, m);
}
nrt_status nrtOccludedBatch_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, const nrt_trace_options *o, uint8_t *m) {
  return occluded_host<double>(c, r, n, o, m);
}
nrt_status nrtOccludedBatchDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, uint8_t *m, void *s) {
  if (!c) return NRT_ERR_INVALID;
  if (n && !m) return fail(c, NRT_ERR_INVALID, "nrtOccludedBatchDevice: NULL mask");
  return traverse_device<float>(c, {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true, .mask = m});
}
// Occlusion queries of whatever kind the context holds (include/nanort_hip.h, "occlusion queries for every primitive kind").
nrt_status nrtOccludedBatchPrims_f32(nrt_ctx *c, const nrt_ray_f32 *rays, uint64_t n, const nrt_trace_options *opt, uint8_t *mask) {
  if (!c) return NRT_ERR_INVALID;
  if (n == 0) return NRT_OK;
  if (!rays || !mask) return fail(c, NRT_ERR_INVALID, "nrtOccludedBatchPrims: NULL rays/mask");
  std::lock_guard<std::mutex> host_lock(c->host_mutex);
  HIPCHK(c, hipSetDevice(c->device));
  return staged_host_loop<float>(c, rays, n, kStagedRays, 0, 1, nullptr, mask, [&](uint64_t m) -> TraverseLaunch<float> {
    return {.kind = Query::OcclusionPrims, .rays = (const nrt_ray_f32 *)c->st_rays.p, .n = m, .opt = opt, .stream = c->stream, .timed = true,
            .mask = (uint8_t *)c->st_mask.p};
  });
}
nrt_status nrtOccludedBatchPrimsDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, uint8_t *m, void *s) {
  if (!c) return NRT_ERR_INVALID;
  if (n && !m) return fail(c, NRT_ERR_INVALID, "nrtOccludedBatchPrimsDevice: NULL mask");
  return traverse_device<float>(c, {.kind = Query::OcclusionPrims, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true, .mask = m});
}
nrt_status nrtOccludedBatchDevice_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, const nrt_trace_options *o, uint8_t *m, void *s) {
  if (!c) return NRT_ERR_INVALID;
  if (n && !m) return fail(c, NRT_ERR_INVALID, "nrtOccludedBatchDevice: NULL mask");
  return traverse_device<double>(c, {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true, .mask = m});
}

nrt_status nrtSetMeshDevice_f32(nrt_ctx *c, const float *v, uint32_t nv, size_t stride, const uint32_t *f, uint32_t nf, void *s) {
  return set_mesh_device<float>(c, v, nv, stride, f, nf, (hipStream_t)s);
}
nrt_status nrtSetMeshDevice_f64(nrt_ctx *c, const double *v, uint32_t nv, size_t stride, const uint32_t *f, uint32_t nf, void *s) {
  return set_mesh_device<double>(c, v, nv, stride, f, nf, (hipStream_t)s);
}
nrt_status nrtSetSpheresDevice_f32(nrt_ctx *c, const float *centers, const float *radii, uint32_t n, void *s) {
  return set_radius_prims(c, "nrtSetSpheresDevice", kPrimSpheres, 4, centers, radii, n, true, (hipStream_t)s);
}
nrt_status nrtSetSpheres_f32(nrt_ctx *c, const float *centers, const float *radii, uint32_t n) {
  return set_radius_prims(c, "nrtSetSpheres", kPrimSpheres, 4, centers, radii, n, false, nullptr);
}

nrt_status nrtBuild_f32(nrt_ctx *c, const nrt_build_options_f32 *o, nrt_build_stats *st, uint64_t *nn) {
  return build<float>(c, o, st, nn);
}
nrt_status nrtBuild_f64(nrt_ctx *c, const nrt_build_options_f64 *o, nrt_build_stats *st, uint64_t *nn) {
  return build<double>(c, o, st, nn);
}

nrt_status nrtGetTree_f32(nrt_ctx *c, nrt_node_f32 *n, uint32_t *i) { return get_tree<float>(c, n, i); }
nrt_status nrtGetTree_f64(nrt_ctx *c, nrt_node_f64 *n, uint32_t *i) { return get_tree<double>(c, n, i); }

nrt_status nrtGetTreeBounds_f32(nrt_ctx *c, float *lo, float *hi) { return get_tree_bounds<float>(c, lo, hi); }
nrt_status nrtGetTreeBounds_f64(nrt_ctx *c, double *lo, double *hi) { return get_tree_bounds<double>(c, lo, hi); }

nrt_status nrtTreeSize(nrt_ctx *c, uint64_t *nn, uint64_t *ni) {
  if (!c) return NRT_ERR_INVALID;
  if (nn) *nn = c->num_nodes;
  if (ni) *ni = c->num_indices;
  return NRT_OK;
}

nrt_status nrtSetTree_f32(nrt_ctx *c, const nrt_node_f32 *n, uint64_t nn, const uint32_t *i, uint64_t ni) {
  return set_tree<float>(c, n, nn, i, ni);
}
nrt_status nrtSetTree_f64(nrt_ctx *c, const nrt_node_f64 *n, uint64_t nn, const uint32_t *i, uint64_t ni) {
  return set_tree<double>(c, n, nn, i, ni);
}

nrt_status nrtTraverseBatch_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o,
                                nrt_hit_f32 *h, uint8_t *m) {
  return traverse_host<float>(c, r, n, o, h, m);
}
nrt_status nrtTraverseBatch_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, const nrt_trace_options *o,
                                nrt_hit_f64 *h, uint8_t *m) {
  return traverse_host<double>(c, r, n, o, h, m);
}

nrt_status nrtTraverseBatchDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o,
                                      nrt_hit_f32 *h, uint8_t *m, void *s) {
  if (!c) return NRT_ERR_INVALID;
  if (n && !h) return fail(c, NRT_ERR_INVALID, "nrtTraverseBatchDevice: NULL hits");
  return traverse_device<float>(c, {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true, .hits = h, .mask = m});
}
nrt_status nrtTraverseBatchDevice_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, const nrt_trace_options *o,
                                      nrt_hit_f64 *h, uint8_t *m, void *s) {
  if (!c) return NRT_ERR_INVALID;
  if (n && !h) return fail(c, NRT_ERR_INVALID, "nrtTraverseBatchDevice: NULL hits");
  return traverse_device<double>(c, {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true, .hits = h, .mask = m});
}

// Per-ray skip ids (include/nanort_hip.h): the entry points above with one skip id per ray; a NULL array is the call above itself.
nrt_status nrtTraverseBatchSkip_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, const uint32_t *ids, nrt_hit_f32 *h,
                                    uint8_t *m) {
  return traverse_host<float>(c, r, n, o, h, m, ids);
}
nrt_status nrtTraverseBatchSkip_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, const nrt_trace_options *o, const uint32_t *ids, nrt_hit_f64 *h,
                                    uint8_t *m) {
  return traverse_host<double>(c, r, n, o, h, m, ids);
}
nrt_status nrtTraverseBatchSkipDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, const uint32_t *ids,
                                          nrt_hit_f32 *h, uint8_t *m, void *s) {
  return traverse_skip_device<float>(c, r, n, o, ids, h, m, s);
}
nrt_status nrtTraverseBatchSkipDevice_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, const nrt_trace_options *o, const uint32_t *ids,
                                          nrt_hit_f64 *h, uint8_t *m, void *s) {
  return traverse_skip_device<double>(c, r, n, o, ids, h, m, s);
}
nrt_status nrtOccludedBatchSkip_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, const uint32_t *ids, uint8_t *m) {
  return occluded_host<float>(c, r, n, o, m, ids);
}
nrt_status nrtOccludedBatchSkip_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, const nrt_trace_options *o, const uint32_t *ids, uint8_t *m) {
  return occluded_host<double>(c, r, n, o, m, ids);
}
nrt_status nrtOccludedBatchSkipDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, const uint32_t *ids, uint8_t *m,
                                          void *s) {
  return occluded_skip_device<float>(c, r, n, o, ids, m, s);
}
nrt_status nrtOccludedBatchSkipDevice_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, const nrt_trace_options *o, const uint32_t *ids, uint8_t *m,
                                          void *s) {
  return occluded_skip_device<double>(c, r, n, o, ids, m, s);
}
nrt_status nrtTraverseBatchesSkipDevice_f32(nrt_ctx *c, uint32_t nb, const nrt_ray_f32 *const *r, const uint64_t *n, const nrt_trace_options *o,
                                            const uint32_t *const *ids, nrt_hit_f32 *const *h, uint8_t *const *m, const uint32_t *fl, void *s) {
  return traverse_batches_device<float>(c, nb, r, n, o, h, m, fl, (hipStream_t)s, ids);
}
nrt_status nrtTraverseBatchesSkipDevice_f64(nrt_ctx *c, uint32_t nb, const nrt_ray_f64 *const *r, const uint64_t *n, const nrt_trace_options *o,
                                            const uint32_t *const *ids, nrt_hit_f64 *const *h, uint8_t *const *m, const uint32_t *fl, void *s) {
  return traverse_batches_device<double>(c, nb, r, n, o, h, m, fl, (hipStream_t)s, ids);
}
nrt_status nrtTraverseBatchesSkip_f32(nrt_ctx *c, uint32_t nb, const nrt_ray_f32 *const *r, const uint64_t *n, const nrt_trace_options *o,
                                      const uint32_t *const *ids, nrt_hit_f32 *const *h, uint8_t *const *m, const uint32_t *fl) {
  return traverse_batches_host<float>(c, nb, r, n, o, h, m, fl, ids);
}
nrt_status nrtTraverseBatchesSkip_f64(nrt_ctx *c, uint32_t nb, const nrt_ray_f64 *const *r, const uint64_t *n, const nrt_trace_options *o,
                                      const uint32_t *const *ids, nrt_hit_f64 *const *h, uint8_t *const *m, const uint32_t *fl) {
  return traverse_batches_host<double>(c, nb, r, n, o, h, m, fl, ids);
}

nrt_status nrtTraverseBatchMulti_f32(nrt_ctx *const *ctxs, uint32_t num_ctx, const nrt_ray_f32 *r, uint64_t n, uint64_t row_len,
                                     const nrt_trace_options *o, nrt_hit_f32 *h, uint8_t *m) {
  return traverse_multi<float>(ctxs, num_ctx, r, n, row_len, o, h, m);
}
nrt_status nrtTraverseBatchMulti_f64(nrt_ctx *const *ctxs, uint32_t num_ctx, const nrt_ray_f64 *r, uint64_t n, uint64_t row_len,
                                     const nrt_trace_options *o, nrt_hit_f64 *h, uint8_t *m) {
  return traverse_multi<double>(ctxs, num_ctx, r, n, row_len, o, h, m);
}
int nrtDeviceCount(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}
nrt_status nrtTraverseBatchesDevice_f32(nrt_ctx *c, uint32_t nb, const nrt_ray_f32 *const *r, const uint64_t *n, const nrt_trace_options *o,
                                        nrt_hit_f32 *const *h, uint8_t *const *m, const uint32_t *fl, void *s) {
  return traverse_batches_device<float>(c, nb, r, n, o, h, m, fl, (hipStream_t)s);
}
nrt_status nrtTraverseBatchesDevice_f64(nrt_ctx *c, uint32_t nb, const nrt_ray_f64 *const *r, const uint64_t *n, const nrt_trace_options *o,
                                        nrt_hit_f64 *const *h, uint8_t *const *m, const uint32_t *fl, void *s) {
  return traverse_batches_device<double>(c, nb, r, n, o, h, m, fl, (hipStream_t)s);
}
nrt_status nrtTraverseBatches_f32(nrt_ctx *c, uint32_t nb, const nrt_ray_f32 *const *r, const uint64_t *n, const nrt_trace_options *o,
                                  nrt_hit_f32 *const *h, uint8_t *const *m, const uint32_t *fl) {
  return traverse_batches_host<float>(c, nb, r, n, o, h, m, fl);
}
nrt_status nrtTraverseBatches_f64(nrt_ctx *c, uint32_t nb, const nrt_ray_f64 *const *r, const uint64_t *n, const nrt_trace_options *o,
                                  nrt_hit_f64 *const *h, uint8_t *const *m, const uint32_t *fl) {
  return traverse_batches_host<double>(c, nb, r, n, o, h, m, fl);
}
nrt_status nrtTraverseCountDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o,
                                      nrt_trace_counters *out) {
  return traverse_count<float>(c, r, n, o, out);
}
nrt_status nrtTraverseCountDevice_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, const nrt_trace_options *o,
                                      nrt_trace_counters *out) {
  return traverse_count<double>(c, r, n, o, out);
}

// on = 1: events around every traversal launch (a timing pair nrtLastTraverseMs reads, the slot's completion event) — the
// cross-check of the default, which records no event at all: the kernel's last wave publishes a completion record with its
// own start / end stamps (see slot_done / wait_record for who waits on what).
nrt_status nrtSetLaunchTiming(nrt_ctx *c, int on) {
  if (!c) return NRT_ERR_INVALID;
  std::lock_guard<std::mutex> lock(c->launch_mutex);
  c->launch_timing = on ? 1 : 0;
  return NRT_OK;
}

// Traversal / build tunables by name (the table above).  Values are clamped to the tunable's range; a tunable that shapes
// the private tree layout (wide4, wide_scramble, morton) takes effect with the next nrtBuild / nrtSetTree.
nrt_status nrtSetTunable(nrt_ctx *c, const char *name, long long value) {
  if (!c) return NRT_ERR_INVALID;
  std::lock_guard<std::mutex> lock(c->launch_mutex);
  if (!tunable_set(c, name, value)) return fail(c, NRT_ERR_INVALID, "nrtSetTunable: unknown tunable '%s'", name ? name : "(null)");
  return NRT_OK;
}
nrt_status nrtGetTunable(nrt_ctx *c, const char *name, long long *value_out) {
  if (!c || !value_out) return NRT_ERR_INVALID;
  const TunableDesc *d = tunable_find(name);
  if (!d) return fail(c, NRT_ERR_INVALID, "nrtGetTunable: unknown tunable '%s'", name ? name : "(null)");
  std::lock_guard<std::mutex> lock(c->launch_mutex);
  *value_out = d->get(c);
  return NRT_OK;
}

float nrtLastTraverseMs(nrt_ctx *c) {
  if (!c) return -1.f;
  hipEvent_t t0, t1;
  {
    std::unique_lock<std::mutex> lock(c->launch_mutex);
    if (c->last_timed_slot < 0) return -1.f;
    nrt_ctx::LaunchSlot &sl = c->slots[c->last_timed_slot];
    if (sl.last_has_rec) { // the kernel's own stamps: first block started -> last wave finished (100 MHz realtime ticks)
      if (wait_record(sl) != hipSuccess) return -1.f;
      const unsigned long long b = sl.h_done->t_begin, e = sl.h_done->t_end;
      // The record says that every wave has stopped reading; the hit records' non-temporal stores are not fenced by it
      // (traverse.hip, done_end).  This call is documented as the caller's synchronisation point, so it also drains the
      // launch's stream (the stamps are taken: the reported time is unaffected).
      const hipStream_t s = sl.stream;
      lock.unlock();
      if (hipStreamSynchronize(s) != hipSuccess) return -1.f;
      return e >= b ? (float)((double)(e - b) * 1e-5) : -1.f;
    }
    if (!sl.last_timed) return -1.f;
    t0 = sl.t0;
    t1 = sl.t1;
  }
  if (hipEventSynchronize(t1) != hipSuccess) return -1.f;
  float ms = -1.f;
  if (hipEventElapsedTime(&ms, t0, t1) != hipSuccess) return -1.f;
  return ms;
}

// Name of the traversal kernel variant the most recent launch of this context used (as rocprofv3 prints it, without
// the argument list) — bench.py reports it instead of guessing.
const char *nrtLastKernelName(const nrt_ctx *c) { return c ? c->last_kernel : ""; }

#ifdef NRT_PROF // libnanort_hip_prof.so only (include/nanort_hip_prof.h)
// Profiling aid (not part of the public header): loop-occupancy counters of the last launch made with
// NRT_DEBUG bit 32 set.  out[0..6] = it1, act1, trav1, it2, act2, refills, refilled.
int nrtDebugCounters(nrt_ctx *c, unsigned long long *out, int cap) {
  if (!c || !out || cap < 16) return 1; // (sixteen counters are written)
  if (hipStreamSynchronize(c->stream) != hipSuccess) return 1;
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  return hipMemcpy(out, c->d_counters, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
}

// Profiling aid (not part of the public header): with NRT_DEBUG bit 8192 every wave of a traversal launch records when
// it started, ran out of rays and finished (100 MHz realtime ticks).  Copies up to `cap` records (3 x u64 each) of the
// last launch; returns the number of waves, or -1.
long nrtDebugWaveClocks(nrt_ctx *c, unsigned long long *out, long cap) {
  if (!c || !out || !c->b_wave_clock.p) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  const long n = std::min<long>(cap, (long)c->wave_clock_waves);
  if (hipMemcpy(out, c->b_wave_clock.p, (size_t)n * kWaveClockWords * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (long)c->wave_clock_waves;
}

#endif

float nrtLastBuildMs(nrt_ctx *c) {
  if (!c || !c->have_build_time) return -1.f;
  return c->stats.build_secs * 1e3f;
}

} // extern "C"
