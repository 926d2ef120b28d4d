// nanort_amd/csrc/api_ctx.hip — the context's life cycle behind the C ABI (include/nanort_hip.h): nrtCreate / nrtDestroy, page-locked
// host memory, the tunable table, the timing and nrtLast* calls, the accessors scene.hip and group.hip reach a context through
// (kernels.h), and the profiling library's entry points.
#include "ctx.h"

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
  DevBuf *bufs[] = {&c->b_verts, &c->b_radii, &c->b_faces, &c->st_rays, &c->st_hits, &c->st_mask, &c->st_skip, &c->b_nodes, &c->b_indices, &c->b_tris, &c->b_wide, &c->b_wide4, &c->b_wide_scratch, &c->b_build_ws, &c->b_wave_clock, &c->b_seg_verts, &c->b_seg_radii, &c->b_seg_prim, &c->b_seg_off, &c->b_refit_plan, &c->b_refit_stage, &c->b_max_index, &c->b_verts1, &c->b_tris1, &c->st_times, &c->b_prim_masks, &c->b_leaf_masks, &c->st_ray_masks, &c->b_face_normals, &c->b_vertex_normals, &c->b_sdf_ws};
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

int nrtDeviceCount(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
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

float nrtLastBuildMs(nrt_ctx *c) {
  if (!c || !c->have_build_time) return -1.f;
  return c->stats.build_secs * 1e3f;
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

} // extern "C"

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
