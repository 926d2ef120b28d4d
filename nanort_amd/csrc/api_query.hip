// nanort_amd/csrc/api_query.hip — every ray query behind the C ABI (include/nanort_hip.h).  What a launch is asked for
// (TraverseLaunch) and the path every launch takes (traverse_device: validate_launch ... enqueue_launch); the two entries of a
// query into that path, query_device for buffers in HBM and query_host for the caller's host arrays (staged, or pipelined from
// page-locked memory: traverse_host); the multi-batch, multi-context and counting forms; then the entry points.
#include "ctx.h"

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

// What one traversal launch is asked for: the query kind names an OUTPUT — which of the outputs below the launch writes.  (Occlusion:
// every ray stops at the first primitive it accepts; Count: the literal kernel's counting pass into d_counters, no output of its own;
// OcclusionPrims: the occlusion query of nrtOccludedBatchPrims*, which every primitive kind takes — flags straight into the caller's
// mask, no compact records, no post pass; on a triangle context it IS Occlusion: traverse_device says so under the lock.)
// What a triangle launch reads per ray besides its rays — skip ids, shutter times, visibility words — is three independent facts of
// the launch (skip_ids, motion, masked), and own_walk_id() says which kernel they make of it.
enum class Query { Closest, Occlusion, Count, MultiHit, Cylinders, MultiBatch, Curves, OcclusionPrims };
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
  const uint32_t *skip_ids = nullptr;    // Closest, Occlusion, MultiHit: one skip id per ray in the place of opt->skip_prim_id (MultiBatch: batches->skip[])
  const T *times = nullptr;              // motion: one time per ray (null: every ray at time 0)
  const uint32_t *ray_masks = nullptr;   // masked: one visibility word per ray (null: every ray 0xFFFFFFFF)
  // Closest, Occlusion, MultiHit: every ray at its own time (nrt*BatchMotion*, NRT_QUERY_MOTION) / with its own visibility word
  // (nrt*BatchMasked*, NRT_QUERY_MASKED).  Set by what the entry point is, not by whether the array is there.
  bool motion = false, masked = false;
  bool descriptor = false;               // the launch came through nrtQueryBatch*: triangle contexts only, whatever it was routed to
  bool multihit_descriptor = false;      // the launch came through nrtMultiHitQueryBatch* (its refusals are multihit_query_batch's)
  bool multihit() const { return kind == Query::MultiHit; } // rows of max_hits records and a count per ray
  // THE routing: the binary walk of its own the launch runs (own_walks.hip), or kNumOwnWalks for none — the wide or the literal walk.
  // A launch an older entry point can express is that entry point's launch: the same kernel, the same bytes.
  OwnWalk own_walk_id() const {
    const bool ids = skip_ids != nullptr;
    if (multihit()) // nrtMultiHitTraverseBatch*; with any of the three, k_multihit_query<motion, masked>
      return !(ids || motion || masked) ? kOwnMultiHit
             : motion                   ? (masked ? kOwnMultiHitMotionMasked : kOwnMultiHitMotion)
                                        : (masked ? kOwnMultiHitMasked : kOwnMultiHitIds);
    if ((int)ids + (int)motion + (int)masked >= 2) // k_traverse_query<motion, masked>
      return motion ? (masked ? kOwnQueryMotionMasked : kOwnQueryMotion) : kOwnQueryMasked;
    return motion ? kOwnMotion : masked ? kOwnMasked : kNumOwnWalks; // nrt*BatchMotion*, nrt*BatchMasked*; ids alone or nothing: none
  }
  bool own_walk() const { return own_walk_id() != kNumOwnWalks; } // no wide records, no completion record
  // the output the kind is for — what a call with rays cannot do without — is its flags; else its records: hits, or (Cylinders, Curves) cyl_hits
  bool flags_only() const { return kind == Query::Occlusion || kind == Query::OcclusionPrims; }
  void *records() const { return (kind == Query::Cylinders || kind == Query::Curves) ? cyl_hits : (void *)hits; }
  // the launch carries per-ray skip ids
  bool has_skip_ids() const {
    if (skip_ids) return true;
    if (batches)
      for (uint32_t k = 0; k < batches->nb; k++)
        if (batches->skip[k]) return true;
    return false;
  }
};

// Every combination a launch cannot be is refused here (under launch_mutex: the tunables hold still).  (A launch without the output
// its kind is for never arrives: query_device / query_host refuse it, the batch forms check their tables.)
template <typename T>
static nrt_status validate_launch(nrt_ctx *c, const TraverseLaunch<T> &l) {
  const bool custom = c->prim_kind != kPrimTriangles; // spheres / cylinders
  if (c->prec != (int)sizeof(T)) return fail(c, NRT_ERR_PRECISION, "nrtTraverseBatch: precision mismatch");
  if (l.descriptor && custom) // (include/nanort_hip.h, "one descriptor for every triangle ray query")
    return fail(c, NRT_ERR_INVALID, "nrtQueryBatch: triangle contexts only (this context holds %s)", kPrimKinds[c->prim_kind].name);
  if (l.motion) { // (include/nanort_hip.h, "motion blur")
    if (custom) return fail(c, NRT_ERR_INVALID, "motion queries: triangle contexts only (this context holds %s)", kPrimKinds[c->prim_kind].name);
    if (!c->d_verts1) return fail(c, NRT_ERR_INVALID, "motion queries: the context holds no motion keyframe (nrtSetMeshMotion)");
    if (c->d_nodes && !c->d_tris1) return fail(c, NRT_ERR_INVALID, "motion queries: internal: no keyframe-1 leaf records");
    if (((uintptr_t)l.times % sizeof(T)) != 0u) return fail(c, NRT_ERR_INVALID, "motion queries: the times array is not aligned to %zu bytes", sizeof(T));
  }
  if (l.masked) { // (include/nanort_hip.h, "visibility masks"; the masked-alone walk reports as its own entry points, whoever asked)
    const char *fn = l.multihit() ? "nrtMultiHitQueryBatch" : l.own_walk_id() != kOwnMasked ? "nrtQueryBatch" : l.flags_only() ? "nrtOccludedBatchMasked" : "nrtTraverseBatchMasked";
    if (custom) return fail(c, NRT_ERR_INVALID, "%s: masked queries: triangle contexts only (this context holds %s)", fn, kPrimKinds[c->prim_kind].name);
    if (!c->d_prim_masks) return fail(c, NRT_ERR_INVALID, "%s: masked queries: the context holds no visibility masks (nrtSetPrimMasks)", fn);
    if (((uintptr_t)l.ray_masks & 3u) != 0u) return fail(c, NRT_ERR_INVALID, "%s: masked queries: the ray_masks array is not 4-byte aligned", fn);
  }
  if (l.has_skip_ids()) { // (include/nanort_hip.h, "per-ray skip ids")
    if (custom)
      return fail(c, NRT_ERR_INVALID, "per-ray skip ids: triangle contexts only (the sphere, cylinder and curve intersectors have no skip id)");
    if (l.kind != Query::Closest && l.kind != Query::Occlusion && l.kind != Query::MultiBatch && !l.multihit())
      return fail(c, NRT_ERR_INVALID, "per-ray skip ids: closest-hit, occlusion and nrtMultiHitQueryBatch queries only");
    bool aligned = ((uintptr_t)l.skip_ids & 3u) == 0u;
    if (l.batches)
      for (uint32_t k = 0; k < l.batches->nb; k++) aligned = aligned && ((uintptr_t)l.batches->skip[k] & 3u) == 0u;
    if (!aligned) return fail(c, NRT_ERR_INVALID, "per-ray skip ids: the device array is not 4-byte aligned");
  }
  const bool prims = l.kind == Query::OcclusionPrims; // (a sphere, cylinder or curve context: traverse_device)
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
  if (l.kind == Query::Occlusion && !l.own_walk() && (custom || !c->d_wide))
    return fail(c, NRT_ERR_INVALID, "nrtOccludedBatch: occlusion queries run on the triangle WideNode kernel only");
  if (l.kind == Query::MultiBatch && (sizeof(T) != 4 || custom || !c->wide || !c->d_wide))
    return fail(c, NRT_ERR_INVALID, "internal: multi-batch launch on a context that cannot take it");
  return NRT_OK;
}

// The entry checks of the three point queries — closest point, signed distance, nearest faces (include/nanort_hip.h, "closest-point
// queries", "nearest-faces queries") — in the ray queries' order and with their statuses (under launch_mutex).  `device`: the arrays
// are the caller's device memory, whose alignment the kernel's loads and stores rely on (the host form stages them).  `flags`: the
// found bytes, or the nearest-faces query's count words (either may be NULL).
enum class PointQuery { Closest, Signed, Nearest };
struct PointKind {
  PointQuery query = PointQuery::Closest;
  uint32_t max_faces = 1; // Nearest: K, 1..NRT_MAX_NEAREST records per point
  bool nearest() const { return query == PointQuery::Nearest; }
};
template <typename T>
static nrt_status validate_closest(nrt_ctx *c, const char *fn, const PointKind &k, const void *points, uint64_t n, const void *out, const void *flags,
                                   bool device) {
  if (c->prec != (int)sizeof(T)) return fail(c, NRT_ERR_PRECISION, "%s: precision mismatch", fn);
  if (c->prim_kind != kPrimTriangles) return fail(c, NRT_ERR_INVALID, "%s: triangle contexts only (this context holds %s)", fn, kPrimKinds[c->prim_kind].name);
  if (!c->d_nodes) return fail(c, NRT_ERR_INVALID, "%s: no tree (call nrtBuild or nrtSetTree)", fn);
  if (k.nearest() && (k.max_faces == 0u || k.max_faces > NRT_MAX_NEAREST))
    return fail(c, NRT_ERR_INVALID, "%s: max_faces %u outside 1..%u", fn, k.max_faces, NRT_MAX_NEAREST);
  if (n == 0) return NRT_OK;
  if (!points || !out) return fail(c, NRT_ERR_INVALID, "%s: NULL points/%s", fn, k.nearest() ? "nearest_out" : "closest_out");
  if (n > 0x7FFFFFFFull) return fail(c, NRT_ERR_INVALID, "%s: more than 2^31-1 points in one call", fn);
  const uintptr_t align = sizeof(T) == 4 ? 16u : 8u;
  if (device && (((uintptr_t)points % align) != 0u || ((uintptr_t)out % align) != 0u))
    return fail(c, NRT_ERR_INVALID, "%s: the device arrays are not aligned to %zu bytes", fn, (size_t)align);
  if (device && k.nearest() && ((uintptr_t)flags % sizeof(uint32_t)) != 0u) // (a found byte has no alignment to check)
    return fail(c, NRT_ERR_INVALID, "%s: counts_out is not aligned to 4 bytes", fn);
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

// The kernel a launch runs (Walk: ctx.h), from the context's tree and tunables and the launch's kind and options.
struct WalkChoice {
  Walk walk;
  OwnWalk own;        // Walk::Own: which of own_walks.hip's kernels
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
  const bool use_wide = (c->wide || custom || l.kind == Query::Occlusion) && l.kind != Query::Count && c->d_wide && !l.own_walk();
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
  w.own = l.own_walk_id();
  w.walk = l.own_walk() ? Walk::Own : (use_wide4 ? Walk::TwoLevel : (use_wide ? Walk::OneLevel : Walk::Literal));
  w.lds_entries = l.own_walk() ? kLdsStackDefault : (use_wide4 ? kWide4LdsStack : (custom ? 10 : (use_wide ? c->wide_stack : c->lds_stack)));
  return w;
}

// Persistent grid: every block resident.  A variant's occupancy is asked for once per context and key (what selects the kernel).
template <typename T>
static GridPlan size_grid(nrt_ctx *c, const WalkChoice &w, uint64_t n) {
  auto &e = c->occupancy[(int)w.walk + (w.walk == Walk::Own ? (int)w.own : 0)][c->prim_kind];
  if (e.blocks_per_cu == 0 || e.lds_entries != w.lds_entries)
    e = {w.lds_entries, (unsigned)(w.walk == Walk::Own       ? own_walk_blocks_per_cu<T>(w.own)
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
  a.any_hit = l.flags_only() ? 1u : 0u; // (every kind that writes flags only is an occlusion query)
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
  if (w.walk == Walk::Own) {
    HIPCHK(c, (launch_own_walk<T>(w.own, a, {l.max_hits, l.hit_counts, c->d_tris1, l.times, (const uint32_t *)c->b_leaf_masks.p, l.ray_masks}, grid, s,
                                  &c->last_kernel)));
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

// The leaf-order words of a masked launch (prims.hip, k_permute_masks): b_leaf_masks[k] = b_prim_masks[d_tris[k].prim_id], derived again whenever the
// setter or free_tree said that it no longer is (ctx.h, leaf_masks_stale).  Under launch_mutex.  No launch reads the array meanwhile:
// whoever set the flag waited for the launches in flight first, and no masked launch starts without passing here.  The host waits for
// the kernel, on the context's own stream: launches on every stream may read the array once this returns, with no event between them
// (once per change of the masks or of the tree, some tens of microseconds; a Device refit in flight rewrites d_tris — in the same
// order — so it is waited for first).
template <typename T>
static nrt_status refresh_leaf_masks(nrt_ctx *c) {
  if (!c->leaf_masks_stale) return NRT_OK;
  HIPCHK(c, refit_host_wait_locked(c));
  if (nrt_status st = ensure(c, c->b_leaf_masks, std::max<size_t>(1, c->num_indices) * sizeof(uint32_t))) return st;
  HIPCHK(c, launch_permute_masks<T>(c->d_tris, c->d_prim_masks, c->num_faces, (uint32_t *)c->b_leaf_masks.p, (uint32_t)c->num_indices, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->leaf_masks_stale = false;
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
  if (l.masked && (st = refresh_leaf_masks<T>(c))) return st;
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

// The pseudonormals of the signed distance query (sdf.hip): derived again from d_verts / d_faces whenever a mesh setter or a refit
// said that they no longer are the mesh's (ctx.h, feature_normals_stale).  As refresh_leaf_masks: under launch_mutex, a Device refit
// in flight (it rewrites d_verts) waited for first, on the context's own stream, and the host waits for the kernels — launches on
// every stream may read the buffers once this returns.  No launch reads them meanwhile: whoever set the flag waited for the
// launches in flight first.  More than floor((2^32 - 1) / 3) faces are refused: a corner id has 32 bits.
template <typename T>
static nrt_status refresh_feature_normals(nrt_ctx *c, const char *fn) {
  if (!c->feature_normals_stale) return NRT_OK;
  if (c->num_faces > 0xFFFFFFFFu / 3u) return fail(c, NRT_ERR_INVALID, "%s: more than %u faces: a corner id 3 * face + k has 32 bits", fn, 0xFFFFFFFFu / 3u);
  HIPCHK(c, refit_host_wait_locked(c));
  nrt_status st;
  if ((st = ensure(c, c->b_face_normals, std::max<size_t>(1, c->num_faces) * 12 * sizeof(T))) ||
      (st = ensure(c, c->b_vertex_normals, std::max<size_t>(1, c->num_verts) * 3 * sizeof(T))) ||
      (st = ensure(c, c->b_sdf_ws, std::max<size_t>(1, feature_normals_workspace_bytes<T>(c->num_faces, c->num_verts)))))
    return st;
  HIPCHK(c, launch_feature_normals<T>((const T *)c->d_verts, c->d_faces, c->num_faces, c->num_verts, c->b_sdf_ws.p, (T *)c->b_face_normals.p,
                                      (T *)c->b_vertex_normals.p, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->feature_normals_stale = false;
  return NRT_OK;
}

// nrtGetFeatureNormals_*: the normals (refreshed if stale) to the host.  Either pointer may be NULL.  Needs a triangle mesh, not a tree.
template <typename T>
static nrt_status get_feature_normals(nrt_ctx *c, T *face_normals, T *vertex_normals) {
  const char *fn = "nrtGetFeatureNormals";
  if (!c) return NRT_ERR_INVALID;
  std::lock_guard<std::mutex> lock(c->launch_mutex);
  if (c->prec != (int)sizeof(T)) return fail(c, NRT_ERR_PRECISION, "%s: precision mismatch", fn);
  if (c->prim_kind != kPrimTriangles) return fail(c, NRT_ERR_INVALID, "%s: triangle contexts only (this context holds %s)", fn, kPrimKinds[c->prim_kind].name);
  if (!c->d_verts || !c->d_faces) return fail(c, NRT_ERR_INVALID, "%s: no mesh (call nrtSetMesh)", fn);
  HIPCHK(c, hipSetDevice(c->device));
  if (nrt_status st = refresh_feature_normals<T>(c, fn)) return st;
  if (face_normals) HIPCHK(c, hipMemcpy(face_normals, c->b_face_normals.p, (size_t)c->num_faces * 12 * sizeof(T), hipMemcpyDeviceToHost));
  if (vertex_normals) HIPCHK(c, hipMemcpy(vertex_normals, c->b_vertex_normals.p, (size_t)c->num_verts * 3 * sizeof(T), hipMemcpyDeviceToHost));
  return NRT_OK;
}

// The closest-point query (closest.hip, k_closest_point) takes the path of a ray launch — launch_mutex from the checks to the slot's
// event, a launch slot for its cursors and its overflow stack, the persistent grid and the claim plan of launch_plan.h — with points
// in the place of rays: `points`, `out` and `found` are device arrays, `s` the stream the launch is enqueued on.  It publishes no
// completion record: the slot is closed by its event, which is what a rebuild or a refit waits for (wait_for_launches).
// `k`: which of the three point queries.  Signed (k_signed_distance): the same checks, slot and events, the pseudonormals refreshed
// first.  Nearest (nearest.hip, k_nearest_faces): `out` holds k.max_faces records per point and `flags` a count word per point where
// the other two have a found byte.
template <typename T>
static nrt_status closest_device(nrt_ctx *c, const char *fn, const void *points, uint64_t n, const nrt_trace_options *opt, void *out, void *flags,
                                 bool device, hipStream_t s, const PointKind &k = {}) {
  const bool is_signed = k.query == PointQuery::Signed;
  uint8_t *found = (uint8_t *)flags;
  if (!c) return NRT_ERR_INVALID;
  if (!opt) opt = &kDefaultTrace;
  std::lock_guard<std::mutex> lock(c->launch_mutex);
  nrt_status st = validate_closest<T>(c, fn, k, points, n, out, flags, device);
  if (st || n == 0) return st;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, refit_stream_wait(c, s)); // (a Device refit in flight on another stream)
  if (is_signed && (st = refresh_feature_normals<T>(c, fn))) return st;
  nrt_ctx::LaunchSlot *slot = nullptr;
  if ((st = take_slot(c, s, &slot))) return st;
  if (c->closest_blocks_per_cu == 0) c->closest_blocks_per_cu = (unsigned)closest_point_blocks_per_cu<T>();
  if (is_signed && c->signed_blocks_per_cu == 0) c->signed_blocks_per_cu = (unsigned)signed_distance_blocks_per_cu<T>();
  if (k.nearest() && c->nearest_blocks_per_cu == 0) c->nearest_blocks_per_cu = (unsigned)nearest_faces_blocks_per_cu<T>();
  const unsigned resident = is_signed ? c->signed_blocks_per_cu : k.nearest() ? c->nearest_blocks_per_cu : c->closest_blocks_per_cu;
  const unsigned per_cu = c->max_blocks_per_cu && resident > c->max_blocks_per_cu ? c->max_blocks_per_cu : resident;
  const GridPlan g = plan_grid(n, kTraverseBlock, (uint32_t)c->num_cus, per_cu, c->num_parts);
  const uint32_t total_threads = g.grid * kTraverseBlock, total_waves = g.grid * (kTraverseBlock / kWave);
  const DistributionPlan d = plan_distribution((uint32_t)n, total_waves, g.parts, c->static_pct, c->static_bands, c->static_slice_groups, c->chunk);
  // (one pending sibling per level of the path, as the binary walk: trees deeper than the LDS stack go on in the slot's overflow area)
  const uint32_t levels = plan_spill_levels(c->tree_depth, false, (uint32_t)kLdsStackDefault);
  if (levels && (st = ensure(c, slot->spill, (size_t)levels * total_threads * sizeof(uint32_t)))) return st;
  TraverseLaunch<T> l = {};
  l.kind = Query::Closest;
  l.n = n;
  l.opt = opt;
  l.stream = s;
  WalkChoice w = {};
  w.walk = Walk::Literal; // (the node array, no private records)
  w.own = kNumOwnWalks;
  w.lds_entries = kLdsStackDefault;
  TraverseArgs<T> a = {};
  fill_walk_args(c, l, w, a);
  fill_launch_args(l, slot, g, d, levels, a);
#ifdef NRT_PROF
  HIPCHK(c, hipMemsetAsync(c->d_counters, 0, 16 * sizeof(unsigned long long), s)); // (nodes opened, triangles tested: nrtDebugCounters [0], [2])
#else
  a.counters = nullptr;
#endif
  HIPCHK(c, hipEventRecord(slot->t0, s));
  if (is_signed) {
    const SignedInputs<T> in = {(const T *)c->b_face_normals.p, (const T *)c->b_vertex_normals.p, c->d_faces, c->num_faces, c->num_verts};
    HIPCHK(c, launch_signed_distance<T>(a, in, points, out, found, g.grid, s, &c->last_kernel));
  } else if (k.nearest()) {
    HIPCHK(c, launch_nearest_faces<T>(a, points, k.max_faces, out, (uint32_t *)flags, g.grid, s, &c->last_kernel));
  } else {
    HIPCHK(c, launch_closest_point<T>(a, points, out, found, g.grid, s, &c->last_kernel));
  }
  // (the kernel is enqueued: the slot's state follows it now, as in enqueue_launch)
  slot->last_has_rec = false;
  slot->last_timed = false;
  slot->parity ^= 1u;
  slot->stream = s;
  slot->used = true;
  HIPCHK(c, hipEventRecord(slot->t1, s));
  slot->last_timed = true;
  c->last_timed_slot = (int)(slot - c->slots);
  HIPCHK(c, hipEventRecord(slot->done, s));
  return NRT_OK;
}

const uint64_t kClosestPiece = 1ull << 20; // points per launch of the staged host form (16 MB up, 33 MB down in fp32)

// ... over the caller's HOST arrays: one call at a time (host_mutex: the staging buffers are the context's), in pieces of kClosestPiece
// points — the piece up into st_rays, the launch over the staging buffers, its records and bytes of st_hits / st_mask back.  The
// nearest-faces query has K = k.max_faces records and one count word per point: its pieces are max(1, kClosestPiece / K) points, so
// that a piece stages no more records than the other two queries'.
template <typename T>
static nrt_status closest_host(nrt_ctx *c, const typename ClosestWire<T>::Point *points, uint64_t n, const nrt_trace_options *opt,
                               typename ClosestWire<T>::Record *out, void *flags, const PointKind &k = {}) {
  typedef typename ClosestWire<T>::Point Point;
  typedef typename ClosestWire<T>::Record Record;
  const char *fn = k.query == PointQuery::Signed ? "nrtSignedDistanceBatch" : k.nearest() ? "nrtNearestFacesBatch" : "nrtClosestPointBatch";
  if (!c) return NRT_ERR_INVALID;
  {
    std::lock_guard<std::mutex> lock(c->launch_mutex);
    const nrt_status st = validate_closest<T>(c, fn, k, points, n, out, flags, false);
    if (st || n == 0) return st;
  }
  std::lock_guard<std::mutex> host_lock(c->host_mutex);
  HIPCHK(c, hipSetDevice(c->device));
  const uint64_t per_point = k.nearest() ? k.max_faces : 1u;           // records
  const uint64_t flag_bytes = k.nearest() ? sizeof(uint32_t) : 1u;     // a count word or a found byte
  const uint64_t piece = std::max<uint64_t>(1, kClosestPiece / per_point);
  for (uint64_t off = 0; off < n; off += piece) {
    const uint64_t m = std::min(piece, n - off);
    nrt_status st;
    if ((st = ensure(c, c->st_rays, m * sizeof(Point))) || (st = ensure(c, c->st_hits, m * per_point * sizeof(Record))) ||
        (st = ensure(c, c->st_mask, m * flag_bytes)))
      return st;
    HIPCHK(c, hipMemcpyAsync(c->st_rays.p, points + off, m * sizeof(Point), hipMemcpyHostToDevice, c->stream));
    if ((st = closest_device<T>(c, fn, c->st_rays.p, m, opt, c->st_hits.p, c->st_mask.p, false, c->stream, k))) {
      (void)hipStreamSynchronize(c->stream);
      return st;
    }
    HIPCHK(c, hipMemcpyAsync(out + off * per_point, c->st_hits.p, m * per_point * sizeof(Record), hipMemcpyDeviceToHost, c->stream));
    if (flags) HIPCHK(c, hipMemcpyAsync((uint8_t *)flags + off * flag_bytes, c->st_mask.p, m * flag_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return NRT_OK;
}

const uint64_t kStagedRays = 1ull << 26; // rays per launch of the staged host paths (keeps staging bounded)
const uint64_t kMultiHitStagedBytes = 256ull << 20; // record bytes per launch of the staged multi-hit paths, whatever K is
const uint64_t kPiece = 1ull << 19; // rays per pipeline stage of traverse_host (19 MB up, 8 MB down in fp32), and per launch of the motion and masked queries' staged path

// Multi-hit (include/nanort_hip.h, nrtMultiHitTraverseBatch*): the kind's own refusals, ahead of the ones every query shares.
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

// The entry of every Device form (`fn`: the entry point its message names): `l` carries the caller's device pointers and stream.
// Refused before the context is looked at: a NULL context, and a launch without the output its kind is for — its flags
// (flags_only) or its records.
template <typename T>
static nrt_status query_device(nrt_ctx *c, const char *fn, const TraverseLaunch<T> &l) {
  if (!c) return NRT_ERR_INVALID;
  if (l.multihit() && !l.multihit_descriptor) {
    const nrt_status st = multihit_check<T>(c, l.rays, l.n, l.max_hits, l.hits);
    if (st || l.n == 0) return st;
  }
  if (l.n && !(l.flags_only() ? (const void *)l.mask : l.records())) return fail(c, NRT_ERR_INVALID, "%s: NULL %s", fn, l.flags_only() ? "mask" : "hits");
  return traverse_device<T>(c, l);
}

// The entry of every host form (`fn`: the entry point its message names): `host` carries the caller's HOST pointers, and no stream.
// Its refusals in the order a caller has always seen them; then one call at a time (host_mutex: the staging buffers are the
// context's), in pieces: the piece's rays — and its slice of the skip ids, of the times and of the ray masks, where the query has them — up into
// st_rays (st_skip, st_times, st_ray_masks), the launch over the staging buffers, the kind's record and flag bytes per ray of st_hits / st_mask
// back into the caller's arrays (a null one is not copied).
template <typename T>
static nrt_status query_host(nrt_ctx *c, const char *fn, const TraverseLaunch<T> &host) {
  typedef typename Wire<T>::Ray Ray;
  typedef typename Wire<T>::Hit Hit;
  if (!c) return NRT_ERR_INVALID;
  const bool multihit = host.multihit(), own_records = host.kind == Query::Cylinders || host.kind == Query::Curves;
  if (multihit && !host.multihit_descriptor) // (a descriptor's refusals carry its own entry point's name: multihit_query_batch)
    if (nrt_status st = multihit_check<T>(c, host.rays, host.n, host.max_hits, host.hits)) return st;
  if (host.n == 0) return NRT_OK;
  void *recs = host.records(), *flags = multihit ? (void *)host.hit_counts : (void *)host.mask;
  if (!host.rays || !(host.flags_only() ? flags : recs)) return fail(c, NRT_ERR_INVALID, "%s: NULL rays/%s", fn, host.flags_only() ? "mask" : "hits");
  const size_t rec_bytes = host.flags_only() ? 0
                           : own_records     ? (size_t)kPrimKinds[host.kind == Query::Cylinders ? kPrimCylinders : kPrimCurves].hit_bytes
                           : multihit        ? host.max_hits * sizeof(Hit)
                                             : sizeof(Hit);
  const size_t flag_bytes = multihit ? sizeof(uint32_t) : 1;
  // rays per launch: multi-hit keeps the staged records within kMultiHitStagedBytes (256 MiB) whatever K is; the motion queries go in traverse_host's pieces
  // (their staging stays as small as the pipeline's)
  const uint64_t chunk = multihit        ? std::max<uint64_t>(1u, std::min<uint64_t>(1ull << 26, kMultiHitStagedBytes / rec_bytes))
                         : (host.motion || host.masked) ? kPiece
                                         : kStagedRays;
  std::lock_guard<std::mutex> host_lock(c->host_mutex);
  HIPCHK(c, hipSetDevice(c->device));
  TraverseLaunch<T> l = host;
  l.stream = c->stream;
  l.timed = true;
  for (uint64_t off = 0; off < host.n; off += chunk) {
    const uint64_t m = l.n = std::min(chunk, host.n - off);
    nrt_status st;
    if ((st = ensure(c, c->st_rays, m * sizeof(Ray))) || (rec_bytes && (st = ensure(c, c->st_hits, m * rec_bytes))) || (st = ensure(c, c->st_mask, m * flag_bytes)))
      return st;
    HIPCHK(c, hipMemcpyAsync(c->st_rays.p, host.rays + off, m * sizeof(Ray), hipMemcpyHostToDevice, c->stream));
    if (host.skip_ids) {
      if ((st = ensure(c, c->st_skip, m * sizeof(uint32_t)))) return st;
      HIPCHK(c, hipMemcpyAsync(c->st_skip.p, host.skip_ids + off, m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
      l.skip_ids = (const uint32_t *)c->st_skip.p;
    }
    if (host.times) {
      if ((st = ensure(c, c->st_times, m * sizeof(T)))) return st;
      HIPCHK(c, hipMemcpyAsync(c->st_times.p, host.times + off, m * sizeof(T), hipMemcpyHostToDevice, c->stream));
      l.times = (const T *)c->st_times.p;
    }
    if (host.ray_masks) {
      if ((st = ensure(c, c->st_ray_masks, m * sizeof(uint32_t)))) return st;
      HIPCHK(c, hipMemcpyAsync(c->st_ray_masks.p, host.ray_masks + off, m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
      l.ray_masks = (const uint32_t *)c->st_ray_masks.p;
    }
    l.rays = (const Ray *)c->st_rays.p;
    if (own_records) l.cyl_hits = c->st_hits.p;
    else if (rec_bytes) l.hits = (Hit *)c->st_hits.p;
    if (multihit) l.hit_counts = flags ? (uint32_t *)c->st_mask.p : nullptr;
    else l.mask = (uint8_t *)c->st_mask.p; // (also where the caller passed none: the walk writes its flags either way)
    if ((st = traverse_device<T>(c, l))) return st;
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
// `host`: a Closest query, with or without motion and masks, over the caller's host arrays (skip ids, times and ray masks may be null).  Whether the call takes the
// pipeline is read off its size and its pointers before the lock; every other call, the refusals included, is query_host's.
template <typename T>
static nrt_status traverse_host(nrt_ctx *c, const TraverseLaunch<T> &host) {
  typedef typename Wire<T>::Ray Ray;
  typedef typename Wire<T>::Hit Hit;
  const Ray *rays = host.rays;
  Hit *hits = host.hits;
  uint8_t *mask = host.mask;
  const uint32_t *skip_ids = host.skip_ids;
  const T *times = host.times;
  const uint32_t *ray_masks = host.ray_masks;
  const uint64_t n = host.n;
  if (c && n >= 2 * kPiece && c->host_pipeline && rays && hits && is_pinned_host(rays) && is_pinned_host(hits) && (!mask || is_pinned_host(mask)) &&
      (!skip_ids || is_pinned_host(skip_ids)) && (!times || is_pinned_host(times)) &&
      (!ray_masks || is_pinned_host(ray_masks))) {
    std::lock_guard<std::mutex> host_lock(c->host_mutex);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->copy_in) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_in, hipStreamNonBlocking));
    if (!c->copy_out) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_out, hipStreamNonBlocking));
    for (int k = 0; k < 2; k++)
      for (hipEvent_t *e : {&c->ev_in[k], &c->ev_tr[k], &c->ev_out[k]})
        if (!*e) HIPCHK(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    nrt_status st;
    if ((st = ensure(c, c->st_rays, 2 * kPiece * sizeof(Ray))) || (st = ensure(c, c->st_hits, 2 * kPiece * sizeof(Hit))) ||
        (st = ensure(c, c->st_mask, 2 * kPiece)) || (skip_ids && (st = ensure(c, c->st_skip, 2 * kPiece * sizeof(uint32_t)))) ||
        (times && (st = ensure(c, c->st_times, 2 * kPiece * sizeof(T)))) || (ray_masks && (st = ensure(c, c->st_ray_masks, 2 * kPiece * sizeof(uint32_t)))))
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
      uint32_t *d_v = ray_masks ? (uint32_t *)c->st_ray_masks.p + (size_t)b * kPiece : nullptr; // (... and of the visibility words)
      // the ray slot is free once the trace that read it (two pieces ago) is done; the record slot once its download is
      if (piece >= 2) HIPCHK(c, hipStreamWaitEvent(c->copy_in, c->ev_tr[b], 0));
      HIPCHK(c, hipMemcpyAsync(d_r, rays + off, m * sizeof(Ray), hipMemcpyHostToDevice, c->copy_in));
      if (d_s) HIPCHK(c, hipMemcpyAsync(d_s, skip_ids + off, m * sizeof(uint32_t), hipMemcpyHostToDevice, c->copy_in));
      if (d_t) HIPCHK(c, hipMemcpyAsync(d_t, times + off, m * sizeof(T), hipMemcpyHostToDevice, c->copy_in));
      if (d_v) HIPCHK(c, hipMemcpyAsync(d_v, ray_masks + off, m * sizeof(uint32_t), hipMemcpyHostToDevice, c->copy_in));
      HIPCHK(c, hipEventRecord(c->ev_in[b], c->copy_in));
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_in[b], 0));
      if (piece >= 2) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_out[b], 0));
      TraverseLaunch<T> l = host; // (its kind, motion, masked and where it came from)
      l.rays = d_r, l.n = m, l.stream = c->stream, l.timed = true, l.hits = d_h, l.mask = d_m, l.skip_ids = d_s, l.times = d_t, l.ray_masks = d_v;
      st = traverse_device<T>(c, l);
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
  return query_host<T>(c, host.descriptor ? "nrtQueryBatch" : host.masked ? "nrtTraverseBatchMasked" : "nrtTraverseBatch", host);
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
  if (num_ctx == 1) return traverse_host<T>(c0, {.kind = Query::Closest, .rays = rays, .n = n, .opt = opt, .hits = hits, .mask = mask});
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

// nrtQueryBatch* (include/nanort_hip.h, "one descriptor for every triangle ray query"): the descriptor's own refusals, then the launch
// it describes — its arrays and flags copied into a TraverseLaunch.  That a descriptor an existing entry point can express runs that
// entry point's kernel and writes its bytes follows from own_walk_id(), which sees no difference between the two launches.
// D: nrt_ray_query_f32 / _f64.  `device`: the arrays are the caller's device memory and `stream` its stream.
template <typename T, typename D>
static nrt_status query_batch(nrt_ctx *c, const D *q, bool device, void *stream) {
  const char *fn = device ? "nrtQueryBatchDevice" : "nrtQueryBatch";
  if (!c) return NRT_ERR_INVALID;
  if (!q) return fail(c, NRT_ERR_INVALID, "%s: NULL descriptor", fn);
  if (q->struct_size != sizeof(D)) return fail(c, NRT_ERR_INVALID, "%s: struct_size %u, this library's descriptor has %zu bytes", fn, q->struct_size, sizeof(D));
  const uint32_t known = NRT_QUERY_OCCLUSION | NRT_QUERY_MOTION | NRT_QUERY_MASKED;
  if (q->flags & ~known) return fail(c, NRT_ERR_INVALID, "%s: unknown flag bits 0x%x", fn, q->flags & ~known);
  const bool occ = (q->flags & NRT_QUERY_OCCLUSION) != 0u, motion = (q->flags & NRT_QUERY_MOTION) != 0u, masked = (q->flags & NRT_QUERY_MASKED) != 0u;
  if (q->num_rays > 0x7FFFFFFFull) return fail(c, NRT_ERR_INVALID, "%s: more than 2^31-1 rays in one call", fn);
  if (q->num_rays && !q->rays) return fail(c, NRT_ERR_INVALID, "%s: NULL rays", fn);
  if (q->num_rays && !(occ ? (const void *)q->mask_out : (const void *)q->hits_out)) return fail(c, NRT_ERR_INVALID, "%s: NULL %s", fn, occ ? "mask_out" : "hits_out");
  TraverseLaunch<T> l = {};
  l.kind = occ ? Query::Occlusion : Query::Closest;
  l.rays = q->rays;
  l.n = q->num_rays;
  l.opt = q->options;
  l.hits = occ ? nullptr : q->hits_out; // (an occlusion query does not read hits_out)
  l.mask = q->mask_out;
  l.skip_ids = q->skip_prim_ids;
  l.times = motion ? q->times : nullptr;         // (an array whose flag is not set is not read)
  l.ray_masks = masked ? q->ray_masks : nullptr;
  l.motion = motion;
  l.masked = masked;
  l.descriptor = true;
  if (device) {
    l.stream = (hipStream_t)stream;
    l.timed = true;
    return query_device<T>(c, fn, l);
  }
  return occ ? query_host<T>(c, fn, l) : traverse_host<T>(c, l);
}

// nrtMultiHitQueryBatch* (include/nanort_hip.h, "multi-hit with per-ray skip ids, visibility words and motion times"): the descriptor's
// own refusals and the context's, every one under the entry point's name, then the launch it describes: a MultiHit launch with the
// descriptor's arrays and flags (none of them: nrtMultiHitTraverseBatch*'s kernel and bytes — own_walk_id()).
// D: nrt_multihit_query_f32 / _f64.  `device`: as query_batch's.
template <typename T, typename D>
static nrt_status multihit_query_batch(nrt_ctx *c, const D *q, bool device, void *stream) {
  const char *fn = device ? "nrtMultiHitQueryBatchDevice" : "nrtMultiHitQueryBatch";
  if (!c) return NRT_ERR_INVALID;
  if (!q) return fail(c, NRT_ERR_INVALID, "%s: NULL descriptor", fn);
  if (q->struct_size != sizeof(D)) return fail(c, NRT_ERR_INVALID, "%s: struct_size %u, this library's descriptor has %zu bytes", fn, q->struct_size, sizeof(D));
  const uint32_t known = NRT_QUERY_MOTION | NRT_QUERY_MASKED;
  if (q->flags & NRT_QUERY_OCCLUSION) return fail(c, NRT_ERR_INVALID, "%s: NRT_QUERY_OCCLUSION: a multi-hit query has no occlusion form", fn);
  if (q->flags & ~known) return fail(c, NRT_ERR_INVALID, "%s: unknown flag bits 0x%x", fn, q->flags & ~known);
  if (q->reserved != 0u) return fail(c, NRT_ERR_INVALID, "%s: reserved is %u, must be 0", fn, q->reserved);
  if (q->max_hits == 0u || q->max_hits > NRT_MAX_MULTIHIT) return fail(c, NRT_ERR_INVALID, "%s: max_hits %u outside 1..%u", fn, q->max_hits, NRT_MAX_MULTIHIT);
  const bool motion = (q->flags & NRT_QUERY_MOTION) != 0u, masked = (q->flags & NRT_QUERY_MASKED) != 0u;
  if (q->num_rays > 0x7FFFFFFFull) return fail(c, NRT_ERR_INVALID, "%s: more than 2^31-1 rays in one call", fn);
  if (q->num_rays && !q->rays) return fail(c, NRT_ERR_INVALID, "%s: NULL rays", fn);
  if (q->num_rays && !q->hits_out) return fail(c, NRT_ERR_INVALID, "%s: NULL hits_out", fn);
  if (c->prec != (int)sizeof(T)) return fail(c, NRT_ERR_PRECISION, "%s: precision mismatch", fn);
  if (c->prim_kind != kPrimTriangles) return fail(c, NRT_ERR_INVALID, "%s: triangle contexts only (this context holds %s)", fn, kPrimKinds[c->prim_kind].name);
  if (motion && !c->d_verts1) return fail(c, NRT_ERR_INVALID, "%s: MOTION: the context holds no motion keyframe (nrtSetMeshMotion)", fn);
  if (masked && !c->d_prim_masks) return fail(c, NRT_ERR_INVALID, "%s: MASKED: the context holds no visibility masks (nrtSetPrimMasks)", fn);
  if (device) { // (the host form stages every array: any alignment does)
    if (motion && ((uintptr_t)q->times % sizeof(T)) != 0u) return fail(c, NRT_ERR_INVALID, "%s: the times array is not aligned to %zu bytes", fn, sizeof(T));
    if (masked && ((uintptr_t)q->ray_masks & 3u) != 0u) return fail(c, NRT_ERR_INVALID, "%s: the ray_masks array is not 4-byte aligned", fn);
    if (((uintptr_t)q->skip_prim_ids & 3u) != 0u) return fail(c, NRT_ERR_INVALID, "%s: the skip_prim_ids array is not 4-byte aligned", fn);
    if (((uintptr_t)q->counts_out & 3u) != 0u) return fail(c, NRT_ERR_INVALID, "%s: the counts_out array is not 4-byte aligned", fn);
  }
  if (!c->d_nodes) return fail(c, NRT_ERR_INVALID, "%s: no tree (call nrtBuild or nrtSetTree)", fn);
  if (q->num_rays == 0) return NRT_OK;
  TraverseLaunch<T> l = {};
  l.kind = Query::MultiHit;
  l.rays = q->rays;
  l.n = q->num_rays;
  l.opt = q->options;
  l.hits = q->hits_out;
  l.max_hits = q->max_hits;
  l.hit_counts = q->counts_out;
  l.skip_ids = q->skip_prim_ids;
  l.times = motion ? q->times : nullptr;         // (an array whose flag is not set is not read)
  l.ray_masks = masked ? q->ray_masks : nullptr;
  l.motion = motion;
  l.masked = masked;
  l.multihit_descriptor = true;
  if (device) {
    l.stream = (hipStream_t)stream;
    l.timed = true;
    return query_device<T>(c, fn, l);
  }
  return query_host<T>(c, fn, l);
}

// ---------------------------------------------------------------------------
// The entry points, in the order of include/nanort_hip.h.  A host form names its arrays and goes through query_host (closest hits:
// traverse_host), a Device form names its arrays and its stream and goes through query_device; the string is the name its
// messages carry.
// ---------------------------------------------------------------------------
extern "C" {

nrt_status nrtOccludedBatch_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, uint8_t *m) {
  return query_host<float>(c, "nrtOccludedBatch", {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .mask = m});
}
nrt_status nrtOccludedBatch_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, const nrt_trace_options *o, uint8_t *m) {
  return query_host<double>(c, "nrtOccludedBatch", {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .mask = m});
}
nrt_status nrtOccludedBatchDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, uint8_t *m, void *s) {
  return query_device<float>(c, "nrtOccludedBatchDevice", {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true, .mask = m});
}
nrt_status nrtOccludedBatchDevice_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, const nrt_trace_options *o, uint8_t *m, void *s) {
  return query_device<double>(c, "nrtOccludedBatchDevice", {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true, .mask = m});
}

nrt_status nrtMultiHitTraverseBatch_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, uint32_t k, const nrt_trace_options *o, nrt_hit_f32 *h,
                                        uint32_t *cnt) {
  return query_host<float>(c, "nrtMultiHitTraverseBatch", {.kind = Query::MultiHit, .rays = r, .n = n, .opt = o, .hits = h, .max_hits = k, .hit_counts = cnt});
}
nrt_status nrtMultiHitTraverseBatch_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, uint32_t k, const nrt_trace_options *o, nrt_hit_f64 *h,
                                        uint32_t *cnt) {
  return query_host<double>(c, "nrtMultiHitTraverseBatch", {.kind = Query::MultiHit, .rays = r, .n = n, .opt = o, .hits = h, .max_hits = k, .hit_counts = cnt});
}
nrt_status nrtMultiHitTraverseBatchDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, uint32_t k, const nrt_trace_options *o,
                                              nrt_hit_f32 *h, uint32_t *cnt, void *s) {
  return query_device<float>(c, "nrtMultiHitTraverseBatchDevice", {.kind = Query::MultiHit, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                                   .hits = h, .max_hits = k, .hit_counts = cnt});
}
nrt_status nrtMultiHitTraverseBatchDevice_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, uint32_t k, const nrt_trace_options *o,
                                              nrt_hit_f64 *h, uint32_t *cnt, void *s) {
  return query_device<double>(c, "nrtMultiHitTraverseBatchDevice", {.kind = Query::MultiHit, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                                    .hits = h, .max_hits = k, .hit_counts = cnt});
}

nrt_status nrtTraverseBatchCylinders_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, nrt_cyl_hit_f32 *h, uint8_t *m) {
  return query_host<float>(c, "nrtTraverseBatchCylinders", {.kind = Query::Cylinders, .rays = r, .n = n, .opt = o, .mask = m, .cyl_hits = h});
}
nrt_status nrtTraverseBatchCylindersDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o,
                                               nrt_cyl_hit_f32 *h, uint8_t *m, void *s) {
  return query_device<float>(c, "nrtTraverseBatchCylindersDevice", {.kind = Query::Cylinders, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                                    .mask = m, .cyl_hits = h});
}

nrt_status nrtTraverseBatchCurves_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, nrt_curve_hit_f32 *h, uint8_t *m) {
  return query_host<float>(c, "nrtTraverseBatchCurves", {.kind = Query::Curves, .rays = r, .n = n, .opt = o, .mask = m, .cyl_hits = h});
}
nrt_status nrtTraverseBatchCurvesDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, nrt_curve_hit_f32 *h,
                                            uint8_t *m, void *s) {
  return query_device<float>(c, "nrtTraverseBatchCurvesDevice", {.kind = Query::Curves, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                                 .mask = m, .cyl_hits = h});
}

// Occlusion queries of whatever kind the context holds (include/nanort_hip.h, "occlusion queries for every primitive kind").
nrt_status nrtOccludedBatchPrims_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, uint8_t *m) {
  return query_host<float>(c, "nrtOccludedBatchPrims", {.kind = Query::OcclusionPrims, .rays = r, .n = n, .opt = o, .mask = m});
}
nrt_status nrtOccludedBatchPrimsDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, uint8_t *m, void *s) {
  return query_device<float>(c, "nrtOccludedBatchPrimsDevice", {.kind = Query::OcclusionPrims, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                                .mask = m});
}

nrt_status nrtTraverseBatch_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, nrt_hit_f32 *h, uint8_t *m) {
  return traverse_host<float>(c, {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .hits = h, .mask = m});
}
nrt_status nrtTraverseBatch_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, const nrt_trace_options *o, nrt_hit_f64 *h, uint8_t *m) {
  return traverse_host<double>(c, {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .hits = h, .mask = m});
}
nrt_status nrtTraverseBatchDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, nrt_hit_f32 *h, uint8_t *m, void *s) {
  return query_device<float>(c, "nrtTraverseBatchDevice", {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                           .hits = h, .mask = m});
}
nrt_status nrtTraverseBatchDevice_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, const nrt_trace_options *o, nrt_hit_f64 *h, uint8_t *m, void *s) {
  return query_device<double>(c, "nrtTraverseBatchDevice", {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                            .hits = h, .mask = m});
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

// Per-ray skip ids (include/nanort_hip.h): the entry points above with one skip id per ray; a NULL array is the call above itself.
nrt_status nrtTraverseBatchSkip_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, const uint32_t *ids, nrt_hit_f32 *h,
                                    uint8_t *m) {
  return traverse_host<float>(c, {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .hits = h, .mask = m, .skip_ids = ids});
}
nrt_status nrtTraverseBatchSkip_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, const nrt_trace_options *o, const uint32_t *ids, nrt_hit_f64 *h,
                                    uint8_t *m) {
  return traverse_host<double>(c, {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .hits = h, .mask = m, .skip_ids = ids});
}
nrt_status nrtTraverseBatchSkipDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, const uint32_t *ids,
                                          nrt_hit_f32 *h, uint8_t *m, void *s) {
  return query_device<float>(c, "nrtTraverseBatchSkipDevice", {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                               .hits = h, .mask = m, .skip_ids = ids});
}
nrt_status nrtTraverseBatchSkipDevice_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, const nrt_trace_options *o, const uint32_t *ids,
                                          nrt_hit_f64 *h, uint8_t *m, void *s) {
  return query_device<double>(c, "nrtTraverseBatchSkipDevice", {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                                .hits = h, .mask = m, .skip_ids = ids});
}
nrt_status nrtOccludedBatchSkip_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, const uint32_t *ids, uint8_t *m) {
  return query_host<float>(c, "nrtOccludedBatch", {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .mask = m, .skip_ids = ids});
}
nrt_status nrtOccludedBatchSkip_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, const nrt_trace_options *o, const uint32_t *ids, uint8_t *m) {
  return query_host<double>(c, "nrtOccludedBatch", {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .mask = m, .skip_ids = ids});
}
nrt_status nrtOccludedBatchSkipDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, const uint32_t *ids, uint8_t *m,
                                          void *s) {
  return query_device<float>(c, "nrtOccludedBatchSkipDevice", {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                               .mask = m, .skip_ids = ids});
}
nrt_status nrtOccludedBatchSkipDevice_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, const nrt_trace_options *o, const uint32_t *ids, uint8_t *m,
                                          void *s) {
  return query_device<double>(c, "nrtOccludedBatchSkipDevice", {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                                .mask = m, .skip_ids = ids});
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

// Motion blur (include/nanort_hip.h; the keyframe's setter: api_geometry.hip): the closest-hit and occlusion queries with one time per ray.
nrt_status nrtTraverseBatchMotion_f32(nrt_ctx *c, const nrt_ray_f32 *r, const float *t, uint64_t n, const nrt_trace_options *o, nrt_hit_f32 *h,
                                      uint8_t *m) {
  return traverse_host<float>(c, {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .hits = h, .mask = m, .times = t, .motion = true});
}
nrt_status nrtTraverseBatchMotion_f64(nrt_ctx *c, const nrt_ray_f64 *r, const double *t, uint64_t n, const nrt_trace_options *o, nrt_hit_f64 *h,
                                      uint8_t *m) {
  return traverse_host<double>(c, {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .hits = h, .mask = m, .times = t, .motion = true});
}
nrt_status nrtTraverseBatchMotionDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, const float *t, uint64_t n, const nrt_trace_options *o,
                                            nrt_hit_f32 *h, uint8_t *m, void *s) {
  return query_device<float>(c, "nrtTraverseBatchMotionDevice", {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                                 .hits = h, .mask = m, .times = t, .motion = true});
}
nrt_status nrtTraverseBatchMotionDevice_f64(nrt_ctx *c, const nrt_ray_f64 *r, const double *t, uint64_t n, const nrt_trace_options *o,
                                            nrt_hit_f64 *h, uint8_t *m, void *s) {
  return query_device<double>(c, "nrtTraverseBatchMotionDevice", {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                                  .hits = h, .mask = m, .times = t, .motion = true});
}
nrt_status nrtOccludedBatchMotion_f32(nrt_ctx *c, const nrt_ray_f32 *r, const float *t, uint64_t n, const nrt_trace_options *o, uint8_t *m) {
  return query_host<float>(c, "nrtOccludedBatch", {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .mask = m, .times = t, .motion = true});
}
nrt_status nrtOccludedBatchMotion_f64(nrt_ctx *c, const nrt_ray_f64 *r, const double *t, uint64_t n, const nrt_trace_options *o, uint8_t *m) {
  return query_host<double>(c, "nrtOccludedBatch", {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .mask = m, .times = t, .motion = true});
}
nrt_status nrtOccludedBatchMotionDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, const float *t, uint64_t n, const nrt_trace_options *o, uint8_t *m,
                                            void *s) {
  return query_device<float>(c, "nrtOccludedBatchMotionDevice", {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                                 .mask = m, .times = t, .motion = true});
}
nrt_status nrtOccludedBatchMotionDevice_f64(nrt_ctx *c, const nrt_ray_f64 *r, const double *t, uint64_t n, const nrt_trace_options *o, uint8_t *m,
                                            void *s) {
  return query_device<double>(c, "nrtOccludedBatchMotionDevice", {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                                  .mask = m, .times = t, .motion = true});
}

// Visibility masks (include/nanort_hip.h; the triangles' words: api_geometry.hip): the closest-hit and occlusion queries with one word per ray.
nrt_status nrtTraverseBatchMasked_f32(nrt_ctx *c, const nrt_ray_f32 *r, const uint32_t *v, uint64_t n, const nrt_trace_options *o, nrt_hit_f32 *h,
                                      uint8_t *m) {
  return traverse_host<float>(c, {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .hits = h, .mask = m, .ray_masks = v, .masked = true});
}
nrt_status nrtTraverseBatchMasked_f64(nrt_ctx *c, const nrt_ray_f64 *r, const uint32_t *v, uint64_t n, const nrt_trace_options *o, nrt_hit_f64 *h,
                                      uint8_t *m) {
  return traverse_host<double>(c, {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .hits = h, .mask = m, .ray_masks = v, .masked = true});
}
nrt_status nrtTraverseBatchMaskedDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, const uint32_t *v, uint64_t n, const nrt_trace_options *o,
                                            nrt_hit_f32 *h, uint8_t *m, void *s) {
  return query_device<float>(c, "nrtTraverseBatchMaskedDevice", {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                                 .hits = h, .mask = m, .ray_masks = v, .masked = true});
}
nrt_status nrtTraverseBatchMaskedDevice_f64(nrt_ctx *c, const nrt_ray_f64 *r, const uint32_t *v, uint64_t n, const nrt_trace_options *o,
                                            nrt_hit_f64 *h, uint8_t *m, void *s) {
  return query_device<double>(c, "nrtTraverseBatchMaskedDevice", {.kind = Query::Closest, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                                  .hits = h, .mask = m, .ray_masks = v, .masked = true});
}
nrt_status nrtOccludedBatchMasked_f32(nrt_ctx *c, const nrt_ray_f32 *r, const uint32_t *v, uint64_t n, const nrt_trace_options *o, uint8_t *m) {
  return query_host<float>(c, "nrtOccludedBatchMasked", {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .mask = m, .ray_masks = v, .masked = true});
}
nrt_status nrtOccludedBatchMasked_f64(nrt_ctx *c, const nrt_ray_f64 *r, const uint32_t *v, uint64_t n, const nrt_trace_options *o, uint8_t *m) {
  return query_host<double>(c, "nrtOccludedBatchMasked", {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .mask = m, .ray_masks = v, .masked = true});
}
nrt_status nrtOccludedBatchMaskedDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, const uint32_t *v, uint64_t n, const nrt_trace_options *o, uint8_t *m,
                                            void *s) {
  return query_device<float>(c, "nrtOccludedBatchMaskedDevice", {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                                 .mask = m, .ray_masks = v, .masked = true});
}
nrt_status nrtOccludedBatchMaskedDevice_f64(nrt_ctx *c, const nrt_ray_f64 *r, const uint32_t *v, uint64_t n, const nrt_trace_options *o, uint8_t *m,
                                            void *s) {
  return query_device<double>(c, "nrtOccludedBatchMaskedDevice", {.kind = Query::Occlusion, .rays = r, .n = n, .opt = o, .stream = (hipStream_t)s, .timed = true,
                                                                  .mask = m, .ray_masks = v, .masked = true});
}

// One descriptor for every triangle ray query (include/nanort_hip.h): skip ids, words and times on the same ray.
nrt_status nrtQueryBatch_f32(nrt_ctx *c, const nrt_ray_query_f32 *q) { return query_batch<float>(c, q, false, nullptr); }
nrt_status nrtQueryBatch_f64(nrt_ctx *c, const nrt_ray_query_f64 *q) { return query_batch<double>(c, q, false, nullptr); }
nrt_status nrtQueryBatchDevice_f32(nrt_ctx *c, const nrt_ray_query_f32 *q, void *s) { return query_batch<float>(c, q, true, s); }
nrt_status nrtQueryBatchDevice_f64(nrt_ctx *c, const nrt_ray_query_f64 *q, void *s) { return query_batch<double>(c, q, true, s); }

// Multi-hit under the same three per-ray inputs (include/nanort_hip.h): the K frontmost triangles of the combined intersector.
nrt_status nrtMultiHitQueryBatch_f32(nrt_ctx *c, const nrt_multihit_query_f32 *q) { return multihit_query_batch<float>(c, q, false, nullptr); }
nrt_status nrtMultiHitQueryBatch_f64(nrt_ctx *c, const nrt_multihit_query_f64 *q) { return multihit_query_batch<double>(c, q, false, nullptr); }
nrt_status nrtMultiHitQueryBatchDevice_f32(nrt_ctx *c, const nrt_multihit_query_f32 *q, void *s) { return multihit_query_batch<float>(c, q, true, s); }
nrt_status nrtMultiHitQueryBatchDevice_f64(nrt_ctx *c, const nrt_multihit_query_f64 *q, void *s) { return multihit_query_batch<double>(c, q, true, s); }

// Closest-point queries (include/nanort_hip.h): the nearest face of the mesh to each point.
nrt_status nrtClosestPointBatch_f32(nrt_ctx *c, const nrt_point_f32 *p, uint64_t n, const nrt_trace_options *o, nrt_closest_f32 *out, uint8_t *f) {
  return closest_host<float>(c, p, n, o, out, f);
}
nrt_status nrtClosestPointBatch_f64(nrt_ctx *c, const nrt_point_f64 *p, uint64_t n, const nrt_trace_options *o, nrt_closest_f64 *out, uint8_t *f) {
  return closest_host<double>(c, p, n, o, out, f);
}
nrt_status nrtClosestPointBatchDevice_f32(nrt_ctx *c, const nrt_point_f32 *p, uint64_t n, const nrt_trace_options *o, nrt_closest_f32 *out, uint8_t *f,
                                          void *s) {
  return closest_device<float>(c, "nrtClosestPointBatchDevice", p, n, o, out, f, true, (hipStream_t)s);
}
nrt_status nrtClosestPointBatchDevice_f64(nrt_ctx *c, const nrt_point_f64 *p, uint64_t n, const nrt_trace_options *o, nrt_closest_f64 *out, uint8_t *f,
                                          void *s) {
  return closest_device<double>(c, "nrtClosestPointBatchDevice", p, n, o, out, f, true, (hipStream_t)s);
}

nrt_status nrtTraverseBatchMulti_f32(nrt_ctx *const *ctxs, uint32_t num_ctx, const nrt_ray_f32 *r, uint64_t n, uint64_t row_len,
                                     const nrt_trace_options *o, nrt_hit_f32 *h, uint8_t *m) {
  return traverse_multi<float>(ctxs, num_ctx, r, n, row_len, o, h, m);
}
nrt_status nrtTraverseBatchMulti_f64(nrt_ctx *const *ctxs, uint32_t num_ctx, const nrt_ray_f64 *r, uint64_t n, uint64_t row_len,
                                     const nrt_trace_options *o, nrt_hit_f64 *h, uint8_t *m) {
  return traverse_multi<double>(ctxs, num_ctx, r, n, row_len, o, h, m);
}

nrt_status nrtTraverseCountDevice_f32(nrt_ctx *c, const nrt_ray_f32 *r, uint64_t n, const nrt_trace_options *o, nrt_trace_counters *out) {
  return traverse_count<float>(c, r, n, o, out);
}
nrt_status nrtTraverseCountDevice_f64(nrt_ctx *c, const nrt_ray_f64 *r, uint64_t n, const nrt_trace_options *o, nrt_trace_counters *out) {
  return traverse_count<double>(c, r, n, o, out);
}

} // extern "C"

// Nearest-faces queries (include/nanort_hip.h): the K nearest faces of the mesh to each point, a sorted row of closest-point records.
nrt_status nrtNearestFacesBatch_f32(nrt_ctx *c, const nrt_point_f32 *p, uint64_t n, uint32_t k, const nrt_trace_options *o, nrt_closest_f32 *out,
                                    uint32_t *counts) {
  return closest_host<float>(c, p, n, o, out, counts, {PointQuery::Nearest, k});
}
nrt_status nrtNearestFacesBatch_f64(nrt_ctx *c, const nrt_point_f64 *p, uint64_t n, uint32_t k, const nrt_trace_options *o, nrt_closest_f64 *out,
                                    uint32_t *counts) {
  return closest_host<double>(c, p, n, o, out, counts, {PointQuery::Nearest, k});
}
nrt_status nrtNearestFacesBatchDevice_f32(nrt_ctx *c, const nrt_point_f32 *p, uint64_t n, uint32_t k, const nrt_trace_options *o, nrt_closest_f32 *out,
                                          uint32_t *counts, void *s) {
  return closest_device<float>(c, "nrtNearestFacesBatchDevice", p, n, o, out, counts, true, (hipStream_t)s, {PointQuery::Nearest, k});
}
nrt_status nrtNearestFacesBatchDevice_f64(nrt_ctx *c, const nrt_point_f64 *p, uint64_t n, uint32_t k, const nrt_trace_options *o, nrt_closest_f64 *out,
                                          uint32_t *counts, void *s) {
  return closest_device<double>(c, "nrtNearestFacesBatchDevice", p, n, o, out, counts, true, (hipStream_t)s, {PointQuery::Nearest, k});
}

// Signed distance queries (include/nanort_hip.h): the closest-point query with the side of the surface; the records share the layout.
static_assert(sizeof(nrt_signed_f32) == sizeof(nrt_closest_f32) && sizeof(nrt_signed_f64) == sizeof(nrt_closest_f64) &&
                  offsetof(nrt_signed_f32, feature) == offsetof(nrt_closest_f32, _pad) && offsetof(nrt_signed_f64, feature) == offsetof(nrt_closest_f64, _pad),
              "a signed record is a closest-point record with `feature` in the place of `_pad`");
nrt_status nrtSignedDistanceBatch_f32(nrt_ctx *c, const nrt_point_f32 *p, uint64_t n, const nrt_trace_options *o, nrt_signed_f32 *out, uint8_t *f) {
  return closest_host<float>(c, p, n, o, (nrt_closest_f32 *)out, f, {PointQuery::Signed});
}
nrt_status nrtSignedDistanceBatch_f64(nrt_ctx *c, const nrt_point_f64 *p, uint64_t n, const nrt_trace_options *o, nrt_signed_f64 *out, uint8_t *f) {
  return closest_host<double>(c, p, n, o, (nrt_closest_f64 *)out, f, {PointQuery::Signed});
}
nrt_status nrtSignedDistanceBatchDevice_f32(nrt_ctx *c, const nrt_point_f32 *p, uint64_t n, const nrt_trace_options *o, nrt_signed_f32 *out, uint8_t *f,
                                            void *s) {
  return closest_device<float>(c, "nrtSignedDistanceBatchDevice", p, n, o, out, f, true, (hipStream_t)s, {PointQuery::Signed});
}
nrt_status nrtSignedDistanceBatchDevice_f64(nrt_ctx *c, const nrt_point_f64 *p, uint64_t n, const nrt_trace_options *o, nrt_signed_f64 *out, uint8_t *f,
                                            void *s) {
  return closest_device<double>(c, "nrtSignedDistanceBatchDevice", p, n, o, out, f, true, (hipStream_t)s, {PointQuery::Signed});
}
nrt_status nrtGetFeatureNormals_f32(nrt_ctx *c, float *fn, float *vn) { return get_feature_normals<float>(c, fn, vn); }
nrt_status nrtGetFeatureNormals_f64(nrt_ctx *c, double *fn, double *vn) { return get_feature_normals<double>(c, fn, vn); }
