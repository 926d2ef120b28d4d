/* include/nanort_hip.h — C ABI of libnanort_hip.so (MI355X / gfx950 backend).
 *
 * The drop-in boundary for the hot path of lighttransport/nanort:
 * BVHAccel<T>::Build() + BVHAccel<T>::Traverse() for the built-in triangle
 * plugin.  The reference has no FFI of its own — its boundary is a C++
 * template API in one header — so the entry points below are what the inline
 * code of include/nanort.h (this repo's API-compatible header) binds when
 * NANORT_USE_HIP_BACKEND is defined.  Each entry point cites the reference
 * interface it replaces (file:line relative to the reference tree).
 *
 * Conventions
 *   - plain C: pointers and sizes only, no C++ / torch types;
 *   - PODs are layout-identical to the reference's (static_asserts below);
 *   - nrt_status 0 == the reference's `true`; non-zero == `false`, with a
 *     human-readable reason from nrtLastError() (the reference has no error
 *     channel beyond bool/assert, nanort.h:1905-1909);
 *   - "host" entry points take host pointers in/out and own all device
 *     memory; "Device" entry points take device pointers (HBM-resident
 *     buffers, e.g. torch tensors) and a hipStream_t passed as void*;
 *   - one nrt_ctx per BVHAccel object; a context is bound to one GPU.  The
 *     primitive / build / tree calls are not re-entrant on one context (like
 *     BVHAccel::Build, nanort.h:1892).  The traversal calls may be issued
 *     from several host threads: the host-buffer ones share the context's
 *     staging buffers and are served one at a time; the Device ones run
 *     concurrently, on several streams at once, and launches on different
 *     streams overlap on the GPU (each launch owns its scratch until it
 *     completes).  Distinct contexts may be used from distinct host threads.
 *
 * Beyond the triangle path: nrtSetSpheres_f32 /
 * nrtSetCylinders_f32 (the reference's two custom-primitive examples as
 * device primitives) and nrtScene* (NanoSG's instanced two-level traversal).
 */
#ifndef NANORT_HIP_H_
#define NANORT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRT_API __attribute__((visibility("default")))

typedef int nrt_status;
enum {
  NRT_OK = 0,
  NRT_ERR_INVALID = 1,  /* bad argument / call order                  */
  NRT_ERR_EMPTY = 2,    /* n == 0: the reference's Build() == false   */
  NRT_ERR_DEVICE = 3,   /* a HIP call failed (see nrtLastError)       */
  NRT_ERR_PRECISION = 4 /* _f32 call on an _f64 context or vice versa */
};

typedef struct nrt_ctx nrt_ctx;

/* ---- PODs: wire formats shared with the reference ----------------------- */

/* nanort::Ray<float> / Ray<double> — nanort.h:474-496. */
typedef struct {
  float org[3];
  float dir[3];
  float min_t;
  float max_t;
  uint32_t type;
} nrt_ray_f32;
typedef struct {
  double org[3];
  double dir[3];
  double min_t;
  double max_t;
  uint32_t type;
  uint32_t _pad;
} nrt_ray_f64;

/* nanort::BVHNode<T> — nanort.h:498-550.
 * leaf: flag=1, data={count, first slot in indices}; branch: flag=0,
 * axis in {0,1,2}, data={low-side child, high-side child}. */
typedef struct {
  float bmin[3];
  float bmax[3];
  int32_t flag;
  int32_t axis;
  uint32_t data[2];
} nrt_node_f32;
typedef struct {
  double bmin[3];
  double bmax[3];
  int32_t flag;
  int32_t axis;
  uint32_t data[2];
} nrt_node_f64;

/* nanort::TriangleIntersection<T> — nanort.h:996-1005.
 * The batched entry points write EVERY record: on a miss the record is
 * {u=0, v=0, t=ray.max_t, prim_id=0xFFFFFFFF} and hit_mask[i]=0 (the
 * reference leaves the caller's struct untouched on a miss, nanort.h:1206;
 * include/nanort.h's TraverseBatch restores that behaviour on the host). */
typedef struct {
  float u;
  float v;
  float t;
  uint32_t prim_id;
} nrt_hit_f32;
typedef struct {
  double u;
  double v;
  double t;
  uint32_t prim_id;
  uint32_t _pad;
} nrt_hit_f64;

/* nanort::BVHBuildOptions<T> — nanort.h:559-583. */
typedef struct {
  float cost_t_aabb;
  uint32_t min_leaf_primitives;
  uint32_t max_tree_depth;
  uint32_t bin_size;
  uint32_t shallow_depth;
  uint32_t min_primitives_for_parallel_build;
  uint8_t cache_bbox;
  uint8_t pad[3];
} nrt_build_options_f32;
typedef struct {
  double cost_t_aabb;
  uint32_t min_leaf_primitives;
  uint32_t max_tree_depth;
  uint32_t bin_size;
  uint32_t shallow_depth;
  uint32_t min_primitives_for_parallel_build;
  uint8_t cache_bbox;
  uint8_t pad[3];
} nrt_build_options_f64;

/* nanort::BVHBuildStatistics — nanort.h:586-599.  build_secs IS filled here
 * (device time of the build; the reference declares it but never writes it). */
typedef struct {
  uint32_t max_tree_depth;
  uint32_t num_leaf_nodes;
  uint32_t num_branch_nodes;
  float build_secs;
} nrt_build_stats;

/* nanort::BVHTraceOptions — nanort.h:604-624. */
typedef struct {
  uint32_t prim_ids_range[2]; /* half-open [r0, r1)            nanort.h:1055 */
  uint32_t skip_prim_id;      /* 0xFFFFFFFF = none             nanort.h:1061 */
  uint8_t cull_back_face;     /*                               nanort.h:1111 */
  uint8_t pad[3];
} nrt_trace_options;

/* Work counters of one batched traversal, in the units SURVEY.md §8(d)
 * defines the algorithmic bytes on (counted on the reference's traversal
 * order over the node array actually traversed). */
typedef struct {
  uint64_t nodes_visited; /* stack pops == BVHNode fetches + slab tests */
  uint64_t leaves_tested;
  uint64_t tris_tested;   /* Intersect() calls                          */
  uint64_t max_stack;     /* deepest stack (entries) any ray needed     */
} nrt_trace_counters;

/* The descriptor of nrtQueryBatch* ("one descriptor for every triangle ray query" below, where every field is explained). */
#define NRT_QUERY_OCCLUSION 1u /* flags only: mask_out[i] is exactly the closest-hit flag; hits_out is not read */
#define NRT_QUERY_MOTION 2u    /* every ray at its own time (times == NULL: every ray at time 0) */
#define NRT_QUERY_MASKED 4u    /* every ray with its own word (ray_masks == NULL: every ray 0xFFFFFFFF) */
typedef struct nrt_ray_query_f32 {
  uint32_t struct_size; /* sizeof(nrt_ray_query_f32): lets the struct grow */
  uint32_t flags;       /* NRT_QUERY_* */
  const nrt_ray_f32 *rays;
  uint64_t num_rays;
  const nrt_trace_options *options; /* NULL: defaults */
  const uint32_t *skip_prim_ids;    /* NULL: options->skip_prim_id for every ray */
  const float *times;               /* read with NRT_QUERY_MOTION only */
  const uint32_t *ray_masks;        /* read with NRT_QUERY_MASKED only */
  nrt_hit_f32 *hits_out;
  uint8_t *mask_out;
} nrt_ray_query_f32;
typedef struct nrt_ray_query_f64 {
  uint32_t struct_size; /* sizeof(nrt_ray_query_f64) */
  uint32_t flags;
  const nrt_ray_f64 *rays;
  uint64_t num_rays;
  const nrt_trace_options *options;
  const uint32_t *skip_prim_ids;
  const double *times;
  const uint32_t *ray_masks;
  nrt_hit_f64 *hits_out;
  uint8_t *mask_out;
} nrt_ray_query_f64;

/* The descriptor of nrtMultiHitQueryBatch* ("multi-hit with per-ray skip ids, visibility words and motion times" below).  Its first
 * 56 bytes lie as in nrt_ray_query_*. */
typedef struct nrt_multihit_query_f32 {
  uint32_t struct_size;             /* sizeof(nrt_multihit_query_f32) */
  uint32_t flags;                   /* NRT_QUERY_MOTION | NRT_QUERY_MASKED; NRT_QUERY_OCCLUSION is refused */
  const nrt_ray_f32 *rays;
  uint64_t num_rays;
  const nrt_trace_options *options; /* NULL: defaults */
  const uint32_t *skip_prim_ids;    /* NULL: options->skip_prim_id for every ray */
  const float *times;               /* read with NRT_QUERY_MOTION only; NULL: every ray at time 0 */
  const uint32_t *ray_masks;        /* read with NRT_QUERY_MASKED only; NULL: every ray 0xFFFFFFFF */
  nrt_hit_f32 *hits_out;            /* num_rays * max_hits records */
  uint32_t *counts_out;             /* may be NULL */
  uint32_t max_hits;                /* K, 1..NRT_MAX_MULTIHIT */
  uint32_t reserved;                /* must be 0 */
} nrt_multihit_query_f32;
typedef struct nrt_multihit_query_f64 {
  uint32_t struct_size;             /* sizeof(nrt_multihit_query_f64) */
  uint32_t flags;
  const nrt_ray_f64 *rays;
  uint64_t num_rays;
  const nrt_trace_options *options;
  const uint32_t *skip_prim_ids;
  const double *times;
  const uint32_t *ray_masks;
  nrt_hit_f64 *hits_out;
  uint32_t *counts_out;
  uint32_t max_hits;
  uint32_t reserved;
} nrt_multihit_query_f64;

/* The query and the answer of nrtClosestPointBatch* ("closest-point queries" below). */
typedef struct { float  p[3]; float  max_dist; } nrt_point_f32;
typedef struct { double p[3]; double max_dist; } nrt_point_f64;
typedef struct { float  point[3]; float  dist2; float  u, v; uint32_t prim_id; uint32_t _pad; } nrt_closest_f32;
typedef struct { double point[3]; double dist2; double u, v; uint32_t prim_id; uint32_t _pad; } nrt_closest_f64;
/* The answer of nrtSignedDistanceBatch* ("signed distance queries" below): a closest-point record with `feature` in the place of
 * `_pad` — bits 0..2 the feature of the face that holds the nearest point (NRT_FEATURE_*), bit 31 set exactly when the point is
 * inside, every other bit 0. */
typedef struct { float  point[3]; float  dist2; float  u, v; uint32_t prim_id; uint32_t feature; } nrt_signed_f32;
typedef struct { double point[3]; double dist2; double u, v; uint32_t prim_id; uint32_t feature; } nrt_signed_f64;
#define NRT_FEATURE_FACE 0u      /* the face's interior */
#define NRT_FEATURE_EDGE_AB 1u   /* an edge: between the face's first and second, first and third, second and third vertex */
#define NRT_FEATURE_EDGE_AC 2u
#define NRT_FEATURE_EDGE_BC 3u
#define NRT_FEATURE_VERTEX_A 4u  /* the face's first, second, third vertex */
#define NRT_FEATURE_VERTEX_B 5u
#define NRT_FEATURE_VERTEX_C 6u
#define NRT_FEATURE_MASK 7u
#define NRT_SIGNED_INSIDE 0x80000000u

#ifdef __cplusplus
static_assert(sizeof(nrt_point_f32) == 16 && sizeof(nrt_point_f64) == 32, "closest-point query layout");
static_assert(sizeof(nrt_closest_f32) == 32 && sizeof(nrt_closest_f64) == 56, "closest-point record layout");
static_assert(sizeof(nrt_signed_f32) == 32 && sizeof(nrt_signed_f64) == 56, "signed distance record layout");
static_assert(sizeof(nrt_ray_f32) == 36 && sizeof(nrt_ray_f64) == 72, "Ray layout");
static_assert(sizeof(nrt_node_f32) == 40 && sizeof(nrt_node_f64) == 64, "BVHNode layout");
static_assert(sizeof(nrt_hit_f32) == 16 && sizeof(nrt_hit_f64) == 32, "TriangleIntersection layout");
static_assert(sizeof(nrt_build_options_f32) == 28 && sizeof(nrt_build_options_f64) == 32, "BVHBuildOptions layout");
static_assert(sizeof(nrt_build_stats) == 16 && sizeof(nrt_trace_options) == 16, "stats/options layout");
static_assert(sizeof(nrt_ray_query_f32) == 72 && sizeof(nrt_ray_query_f64) == 72, "ray query descriptor layout");
static_assert(sizeof(nrt_multihit_query_f32) == 80 && sizeof(nrt_multihit_query_f64) == 80, "multi-hit query descriptor layout");
#endif

/* ---- context ------------------------------------------------------------ */

/* One context == one nanort::BVHAccel<T> (nanort.h:698-860) living on GPU
 * `device`.  Precision is fixed by the first nrtSetMesh_* call. */
NRT_API nrt_status nrtCreate(int device, nrt_ctx **out);
NRT_API void nrtDestroy(nrt_ctx *ctx);
/* Reason of the last failure on this context (or of the last failed
 * nrtCreate when ctx == NULL).  Never NULL. */
NRT_API const char *nrtLastError(const nrt_ctx *ctx);
/* Library / device identification, e.g. "libnanort_hip gfx950 ...". */
NRT_API const char *nrtVersion(void);

/* Page-locked (pinned) host memory, for callers that do not link HIP themselves: ray / hit arrays allocated here make
 * the copies inside the host entry points (nrtTraverseBatch_*, nrtSceneTraverseBatch_f32, ...) run at PCIe speed instead of
 * being staged through the runtime's bounce buffers.  No reference counterpart.  nrtHostFree(NULL) is a no-op. */
NRT_API nrt_status nrtHostAlloc(size_t bytes, void **out);
NRT_API void nrtHostFree(void *p);

/* ---- mesh: replaces the TriangleMesh / TriangleSAHPred / TriangleIntersector
 * constructors (nanort.h:866-873, 925-930, 1032-1039) ----------------------
 * vertices are read through `vertex_stride_bytes` exactly like
 * get_vertex_addr (nanort.h:467-472); faces are tight 3 x u32.  The mesh
 * carries no vertex count in the reference, so it is derived as
 * max(faces)+1.  The data is copied to HBM; the caller's arrays are not
 * referenced after the call returns. */
NRT_API nrt_status nrtSetMesh_f32(nrt_ctx *ctx, const float *vertices, size_t vertex_stride_bytes,
                                  const uint32_t *faces, uint32_t num_faces);
NRT_API nrt_status nrtSetMesh_f64(nrt_ctx *ctx, const double *vertices, size_t vertex_stride_bytes,
                                  const uint32_t *faces, uint32_t num_faces);

/* ---- occlusion queries: an OPT-IN EXTENSION with no reference counterpart ----------------------------------
 * The reference answers "is anything in the way?" with a closest-hit Traverse (CheckForOccluder,
 * examples/path_tracer/main.cc:675-701).  These entry points return only the hit flag — mask_out[i] is exactly what
 * nrtTraverseBatch* would put in hit_mask_out[i], for every ray and option — but a ray stops at the first primitive it
 * accepts instead of looking for the nearest one.  These four take triangle contexts only and refuse every other kind;
 * sphere, cylinder and curve contexts are asked through nrtOccludedBatchPrims*_f32 (below, behind the curve primitives). */
NRT_API nrt_status nrtOccludedBatch_f32(nrt_ctx *ctx, const nrt_ray_f32 *rays, uint64_t num_rays,
                                        const nrt_trace_options *options, uint8_t *mask_out);
NRT_API nrt_status nrtOccludedBatch_f64(nrt_ctx *ctx, const nrt_ray_f64 *rays, uint64_t num_rays,
                                        const nrt_trace_options *options, uint8_t *mask_out);
NRT_API nrt_status nrtOccludedBatchDevice_f32(nrt_ctx *ctx, const nrt_ray_f32 *d_rays, uint64_t num_rays,
                                              const nrt_trace_options *options, uint8_t *d_mask_out, void *hip_stream);
NRT_API nrt_status nrtOccludedBatchDevice_f64(nrt_ctx *ctx, const nrt_ray_f64 *d_rays, uint64_t num_rays,
                                              const nrt_trace_options *options, uint8_t *d_mask_out, void *hip_stream);

/* ---- multi-hit traversal: the K frontmost triangles of every ray ------------------------------------------
 * The reference declares BVHAccel::MultiHitTraverse (nanort.h:761-770, 2694-2797) but never compiles it (`#if 0`).  Contract,
 * per ray, with K = max_hits, 1 <= K <= NRT_MAX_MULTIHIT, on a triangle context of the call's precision:
 *   1. Candidate: a primitive that TriangleIntersector::Intersect accepts against the current bound B (trace options, the
 *      watertight test with its fp64 edge fallback, `tt > B` rejected, `tt < min_t` rejected — exactly the closest-hit test)
 *      and whose t is < ray.max_t.  min_t is INCLUSIVE, as in the closest-hit walk (the reference's dead code tests
 *      `local_t > ray.min_t`).  A NaN t is never reported.
 *   2. Order: hits are ranked by the key (t, prim_id), ascending; t compares numerically (-0 == +0) and prim_id breaks every
 *      tie, so which candidates are held never depends on the order in which they were tested.
 *   3. Walk: the reference's binary loop over the context's node array (nanort.h:2487-2556): pop, slab test on [ray.min_t, B],
 *      near child first by dir_sign[axis].  B = ray.max_t while fewer than K hits are held, else the t of the worst held hit.
 *      A candidate enters when fewer than K are held or when its key is smaller than the worst held key, which is evicted.
 *      The bound only prunes: the result is the K smallest keys among the candidates of the leaves the walk reaches.
 *   4. Output: hits_out[ray * K + j], j < count, holds the held hits in ascending key order; slots j >= count hold the miss
 *      record {0, 0, ray.max_t, 0xFFFFFFFF} (every byte is written).  counts_out[ray] (may be NULL) receives count, 0..K.
 *   5. K = 1: t and the hit flag (count) equal nrtTraverseBatch*'s on every ray; prim_id / u / v differ only where another
 *      candidate has exactly the same t (multi-hit names the smaller prim_id, closest hit the last one accepted).
 * options == NULL means the BVHTraceOptions() defaults.  NRT_ERR_INVALID: K == 0 or K > NRT_MAX_MULTIHIT, no tree, NULL rays or
 * hits (num_rays > 0), a sphere or cylinder context, more than 2^31-1 rays; NRT_ERR_PRECISION: the context's precision is the
 * other one.  num_rays == 0 returns NRT_OK.  Launches share the context's launch slots: nrtBuild / nrtSetTree / nrtSetMesh /
 * nrtDestroy wait for them as for closest-hit launches. */
#define NRT_MAX_MULTIHIT 64u
NRT_API nrt_status nrtMultiHitTraverseBatch_f32(nrt_ctx *ctx, const nrt_ray_f32 *rays, uint64_t num_rays, uint32_t max_hits,
                                                const nrt_trace_options *options, nrt_hit_f32 *hits_out, uint32_t *counts_out);
NRT_API nrt_status nrtMultiHitTraverseBatch_f64(nrt_ctx *ctx, const nrt_ray_f64 *rays, uint64_t num_rays, uint32_t max_hits,
                                                const nrt_trace_options *options, nrt_hit_f64 *hits_out, uint32_t *counts_out);
/* Same, on HBM-resident buffers, asynchronously on `hip_stream` (a hipStream_t; NULL = the default stream). */
NRT_API nrt_status nrtMultiHitTraverseBatchDevice_f32(nrt_ctx *ctx, const nrt_ray_f32 *d_rays, uint64_t num_rays, uint32_t max_hits,
                                                      const nrt_trace_options *options, nrt_hit_f32 *d_hits_out, uint32_t *d_counts_out,
                                                      void *hip_stream);
NRT_API nrt_status nrtMultiHitTraverseBatchDevice_f64(nrt_ctx *ctx, const nrt_ray_f64 *d_rays, uint64_t num_rays, uint32_t max_hits,
                                                      const nrt_trace_options *options, nrt_hit_f64 *d_hits_out, uint32_t *d_counts_out,
                                                      void *hip_stream);

/* ---- sphere primitives: replaces the SpherePred / SphereGeometry / SphereIntersector constructors of the
 * reference's custom-primitive example (examples/particle_primitive/main.cc:82-147, 161-166) -------------
 * `centers` holds xyz per sphere (tight), `radii` one radius per sphere.  After this call nrtBuild_f32 builds
 * over the spheres' boxes (centre +- radius, SAH position = the centre) and nrtTraverseBatch*_f32 runs that
 * example's intersector: nearest root of the quadratic with the reference's acceptance rules (main.cc:174-236),
 * hit record {u, v, t, prim_id} with u, v the spherical coordinates of the hit normal (main.cc:262-277).
 * BVHTraceOptions: prim_ids_range is honoured; skip_prim_id and cull_back_face do not exist in that intersector
 * and are ignored.  Replaces the mesh of the context (one primitive kind per context). */
NRT_API nrt_status nrtSetSpheres_f32(nrt_ctx *ctx, const float *centers, const float *radii, uint32_t num_spheres);

/* ---- cylinder primitives: replaces the CylinderPred / CylinderGeometry / CylinderIntersector constructors of the
 * reference's second custom-primitive example (examples/cylinder_primitive/main.cc:94-232) ------------------
 * `endpoints` holds two xyz points per cylinder (tight), `radii` two radii per cylinder (the example's intersector
 * uses the larger of the two for the whole cylinder), `test_cap` is that intersector's constructor flag.
 * nrtBuild_f32 then builds over the example's boxes (union of end point +- radius, SAH position = the midpoint)
 * and nrtTraverseBatchCylinders*_f32 runs its intersector (main.cc:237-343: two cap planes, then the side via
 * solve2e :61-90) and PostTraversal (:367-418).  Hit record: the example's CylinderIntersection (:213-224) —
 * {u, v, normal[3], t, prim_id}; `t` is the intersector's hit distance (the example itself never stores it).
 * A miss leaves {0, 0, (0,0,0), ray.max_t, 0xFFFFFFFF}.  Of BVHTraceOptions only prim_ids_range exists there.
 * SEGMENTS (tunables "cyl_split", default 32, and "cyl_seg_radii", default 8; read here): a cylinder many radii long — the
 * example's own scene is box-spanning needles, over whose whole boxes a tree prunes nothing — is handed to the builder as
 * up to cyl_split pieces of its axis, one per cyl_seg_radii tube radii of length, each with the tight box of its piece
 * (end points of the piece +- max(r0, r1), the radius the intersector uses) and the CYLINDER's id.  The index array of the
 * built tree then names a cylinder once per segment (nrtTreeSize gives its length), a leaf tests the whole cylinder, and
 * the intersector — a pure function of (ray, cylinder, current t) — returns the same record or rejects when a cylinder is
 * tested again.  The example's scene at 1920x1080: 44 -> 2 100 Mrays/s.  The reference's Traverse over the same arrays gives
 * the same records (the restated example walks them in the tests).  cyl_split = 1: the example's own whole-cylinder boxes. */
typedef struct nrt_cyl_hit_f32 {
  float u, v;
  float normal[3];
  float t;
  uint32_t prim_id;
} nrt_cyl_hit_f32;
NRT_API nrt_status nrtSetCylinders_f32(nrt_ctx *ctx, const float *endpoints, const float *radii, uint32_t num_cylinders,
                                       int test_cap);
NRT_API nrt_status nrtTraverseBatchCylinders_f32(nrt_ctx *ctx, const nrt_ray_f32 *rays, uint64_t num_rays,
                                                 const nrt_trace_options *options, nrt_cyl_hit_f32 *hits_out,
                                                 uint8_t *hit_mask_out);
/* Same with HBM-resident buffers, asynchronous on `hip_stream` (a hipStream_t). */
NRT_API nrt_status nrtTraverseBatchCylindersDevice_f32(nrt_ctx *ctx, const nrt_ray_f32 *d_rays, uint64_t num_rays,
                                                       const nrt_trace_options *options, nrt_cyl_hit_f32 *d_hits_out,
                                                       uint8_t *d_hit_mask_out, void *hip_stream);

/* ---- curve primitives: replaces the CurvePred / CurveGeometry / CurveIntersector constructors of the reference's
 * third custom-primitive example, hair and fur as cubic Bezier curves (examples/curves_primitive/main.cc:481-840) ----
 * `control_points` holds four xyz points per curve (tight, 12 floats), `radii` four radii per curve, `num_subdivisions`
 * (1..64; the example's default is 4) is the intersector's constructor argument.  fp32 only, as the example.  Contract:
 *   1. Box (CurveGeometry::BoundingBoxAndCenter, :557-597): min / max over the four `point -/+ its radius`; SAH position
 *      ((p0 + p1) + p2 + p3) / 4.  nrtBuild_f32 builds over these; nrtGetTree_f32 / nrtSetTree_f32 / nrtTreeSize /
 *      nrtGetTreeBounds_f32 work as for every kind.
 *   2. Intersect (:637-759), per (ray, curve, current t): prim_ids_range; the frame that puts the ray on the z axis
 *      (GetZAlign :382-417, both branches); the four points in that frame; reject when the largest z (from 0) is below
 *      4 * (max(r[0], r[3]) / 2); then for s < n the segment from the curve at s / n to the curve at (s + 1) / n (de
 *      Casteljau, :432-454): u = the origin's foot on the 2-D segment clamped as max(0, min(1, u)) in std::min / std::max
 *      operand order (a NaN u becomes 1), radius interpolated from 0.5 r[0] to 0.5 r[3], accepted when d2 <= r2 and
 *      t < current; later segments see the lowered t.  No min_t test, no t >= 0 test.  Only radii 0 and 3 are read.
 *      skip_prim_id and cull_back_face do not exist in that intersector and are ignored.
 *   3. The current distance starts at ray.max_t (BVHAccel::Traverse, nanort.h:2494-2501), as for every kind.
 *   4. Hit record: the example's CurveIntersection (:606-619), 40 bytes — {t, prim_id, u, v, tangent[3], normal[3]} with
 *      u = (u_segment + s) / n, v = sqrt(d2), tangent = vnormalize(EvaluateBezierTangent(points, u)) and normal =
 *      vnormalize(cross(cross(dir, tangent), tangent)) (PostTraversal :789-823; vnormalize, nanort.h:388-398, leaves a
 *      vector no longer than epsilon as it is).  A miss leaves {ray.max_t, 0xFFFFFFFF, 0, 0, (0,0,0), (0,0,0)}: every
 *      byte of every record is written.
 *   5. Parity: the reference's Traverse with that intersector over the same node and index arrays gives the same bits.
 * nrtSetCurvesDevice_f32 takes the two arrays from HBM under the contract of nrtSetSpheresDevice_f32 below (4-byte
 * alignment, copied on `hip_stream`, the caller may free them on return, a following build is byte-identical to the host
 * form's).  Refusals leave the context untouched: NRT_ERR_INVALID for a NULL context, num_subdivisions outside 1..64, a
 * NULL or (Device) misaligned pointer with num_curves > 0; NRT_ERR_PRECISION on a context that holds fp64 primitives.
 * A curve context is traced by nrtTraverseBatchCurves*_f32 and nrtOccludedBatchPrims*_f32 (below) only: every other traversal,
 * occlusion, multi-hit, counting, refit, scene and multi-context entry point refuses it with an error string (and the two
 * nrtTraverseBatchCurves*_f32 refuse every other kind). */
typedef struct nrt_curve_hit_f32 {
  float t;
  uint32_t prim_id;
  float u, v;
  float tangent[3];
  float normal[3];
} nrt_curve_hit_f32;
NRT_API nrt_status nrtSetCurves_f32(nrt_ctx *ctx, const float *control_points, const float *radii, uint32_t num_curves,
                                    uint32_t num_subdivisions);
NRT_API nrt_status nrtSetCurvesDevice_f32(nrt_ctx *ctx, const float *d_control_points, const float *d_radii, uint32_t num_curves,
                                          uint32_t num_subdivisions, void *hip_stream);
NRT_API nrt_status nrtTraverseBatchCurves_f32(nrt_ctx *ctx, const nrt_ray_f32 *rays, uint64_t num_rays,
                                              const nrt_trace_options *options, nrt_curve_hit_f32 *hits_out,
                                              uint8_t *hit_mask_out);
/* Same with HBM-resident buffers, asynchronous on `hip_stream` (a hipStream_t). */
NRT_API nrt_status nrtTraverseBatchCurvesDevice_f32(nrt_ctx *ctx, const nrt_ray_f32 *d_rays, uint64_t num_rays,
                                                    const nrt_trace_options *options, nrt_curve_hit_f32 *d_hits_out,
                                                    uint8_t *d_hit_mask_out, void *hip_stream);

/* ---- occlusion queries for every primitive kind: an OPT-IN EXTENSION with no reference counterpart ----------------------
 * "Is anything in the way?" for whatever kind the context holds — spheres, cylinders, curves, triangles.  fp32 only (the setters
 * of the three custom kinds are).  Contract:
 *   1. Result: mask_out[i] is exactly 0 or 1, and 1 exactly when the closest-hit call of the context's kind writes a non-zero
 *      hit_mask_out[i] for the same ray and options: nrtTraverseBatch_f32 (spheres, triangles), nrtTraverseBatchCylinders_f32,
 *      nrtTraverseBatchCurves_f32.  Under both walks (tunable "wide4" 0 and 1) and every scheduling tunable.  The cylinder
 *      calls' cap bit (bit 1 of their mask) never appears here.
 *   2. Options: sphere, cylinder and curve contexts honour prim_ids_range; their intersectors have no skip_prim_id and no
 *      cull_back_face, which are ignored as in their closest-hit calls.  A triangle context honours all three and goes straight
 *      to the path of nrtOccludedBatch*_f32: the same bytes.  Cylinders use the context's test_cap, curves its num_subdivisions.
 *   3. Exactness: the agreement is exact, not approximate.  Until a ray's first acceptance its pops, steps and leaf tests are
 *      those of the closest-hit walk (the bound is still max_t); the ray stops once `hit_t < max_t` holds, the very predicate
 *      of the closest-hit flag — a sphere accepted at t == max_t, or an acceptance that leaves a NaN, does not stop it, as it
 *      leaves the closest-hit flag 0; cylinders and curves only ever lower an accepted distance, so the predicate is final when
 *      it first holds.  One case is outside this: the SPHERE intersector accepts a NaN distance (`if (t > t_inout) return
 *      false`), so a sphere with a NaN centre or radius (or an overflow inside the quadratic) met AFTER a finite hit clears the
 *      closest-hit flag again, where this call has answered 1.  Finite spheres, and rays whose every test yields NaN, agree.
 *   4. Output: one byte per ray is the whole result; no hit record is produced, staged or copied, no compact record is
 *      written to scratch and no pass runs behind the walk.  The host form stages rays in and flags out; the Device form is
 *      asynchronous on `hip_stream`, like nrtOccludedBatchDevice_f32.  nrtLastTraverseMs / nrtLastKernelName describe the
 *      launch as any other.
 *   5. Errors: NRT_ERR_INVALID for a NULL context, NULL rays or mask with num_rays > 0, a context without a tree, more than
 *      2^31-1 rays; NRT_ERR_PRECISION for an fp64 context; num_rays == 0 is NRT_OK.  A refusal writes nothing to the mask and
 *      sets nrtLastError.
 * Unchanged, and out of scope here: nrtOccludedBatch* above keep refusing sphere, cylinder and curve contexts, as do
 * NRT_BATCH_OCCLUSION batches of nrtTraverseBatches*; there is no multi-hit, per-ray skip id, group or scene form for these
 * kinds. */
NRT_API nrt_status nrtOccludedBatchPrims_f32(nrt_ctx *ctx, const nrt_ray_f32 *rays, uint64_t num_rays,
                                             const nrt_trace_options *options, uint8_t *mask_out);
NRT_API nrt_status nrtOccludedBatchPrimsDevice_f32(nrt_ctx *ctx, const nrt_ray_f32 *d_rays, uint64_t num_rays,
                                                   const nrt_trace_options *options, uint8_t *d_mask_out, void *hip_stream);

/* ---- build: replaces BVHAccel<T>::Build (nanort.h:716-718, 1892-2149) ----
 * Binned-SAH construction on the GPU over the mesh set above.  Honours
 * min_leaf_primitives and max_tree_depth (the reference's leaf rule,
 * nanort.h:1781-1783) and bin_size — with two caps the reference does not
 * have (nanort.h:574-582, 1314-1367 take any bin_size): at most 64 bins for a
 * node of more than 256 primitives (one lane of a wave per bin) and at most
 * 16 bins for a node of 256 primitives or fewer (the one-wave-per-subtree
 * phase: one 16-lane row per axis).  A larger bin_size is clamped, not
 * rejected; hit records never depend on it.  shallow_depth,
 * min_primitives_for_parallel_build, cache_bbox and cost_t_aabb are CPU
 * scheduling knobs (or dead, nanort.h:574) and are ignored.  options == NULL
 * means BVHBuildOptions<T>() defaults.  Emits the reference's node format
 * and invariants (root = node 0; indices a permutation of [0, n) — for
 * cylinders cut into segments, nrtSetCylinders_f32, every id once per
 * segment —; DFS pre-order, left child = parent + 1).  NRT_ERR_EMPTY iff num_faces == 0. */
NRT_API nrt_status nrtBuild_f32(nrt_ctx *ctx, const nrt_build_options_f32 *options,
                                nrt_build_stats *stats_out, uint64_t *num_nodes_out);
NRT_API nrt_status nrtBuild_f64(nrt_ctx *ctx, const nrt_build_options_f64 *options,
                                nrt_build_stats *stats_out, uint64_t *num_nodes_out);

/* Copy the built tree to the host: feeds BVHAccel::nodes_ / indices_ so
 * GetNodes/GetIndices/BoundingBox/Dump and the per-ray CPU Traverse keep
 * working (nanort.h:786-806, 2164-2217).  nodes_out holds num_nodes records,
 * indices_out holds num_faces entries. */
NRT_API nrt_status nrtGetTree_f32(nrt_ctx *ctx, nrt_node_f32 *nodes_out, uint32_t *indices_out);
NRT_API nrt_status nrtGetTree_f64(nrt_ctx *ctx, nrt_node_f64 *nodes_out, uint32_t *indices_out);
NRT_API nrt_status nrtTreeSize(nrt_ctx *ctx, uint64_t *num_nodes_out, uint64_t *num_indices_out);
/* The root node's box alone (24 / 48 bytes instead of the whole array): what BVHAccel::BoundingBox returns (nanort.h:786-799)
 * while the header leaves the tree on the device until the host asks for it (include/nanort.h: EnsureHostTree). */
NRT_API nrt_status nrtGetTreeBounds_f32(nrt_ctx *ctx, float bmin_out[3], float bmax_out[3]);
NRT_API nrt_status nrtGetTreeBounds_f64(nrt_ctx *ctx, double bmin_out[3], double bmax_out[3]);

/* Adopt a tree built elsewhere: BVHAccel<T>::Load (nanort.h:2219-2275) or a
 * CPU Build().  Validates child / slot bounds and measures the depth. */
NRT_API nrt_status nrtSetTree_f32(nrt_ctx *ctx, const nrt_node_f32 *nodes, uint64_t num_nodes,
                                  const uint32_t *indices, uint64_t num_indices);
NRT_API nrt_status nrtSetTree_f64(nrt_ctx *ctx, const nrt_node_f64 *nodes, uint64_t num_nodes,
                                  const uint32_t *indices, uint64_t num_indices);

/* ---- refit: the tree's boxes recomputed from moved vertices, its topology kept ------------------------------
 * For a mesh whose vertices move while its faces stay fixed: instead of nrtSetMesh + nrtBuild every frame.  Contract, on a
 * triangle context of the call's precision that holds a tree (from nrtBuild_* or nrtSetTree_*):
 *   1. Input: the context's num_verts vertices (max(faces) + 1, fixed at nrtSetMesh), vertex i at byte offset
 *      i * vertex_stride_bytes, xyz first (get_vertex_addr, nanort.h:467-472).  Faces are not passed: the context keeps its own.
 *   2. Result: the context's vertex positions become the new ones (a later nrtBuild builds over them).  Every node record's
 *      flag, axis and data[] and the index array stay byte-identical.  Each reachable leaf's box is the min / max over every
 *      coordinate of its triangles; each reachable branch's box is the min / max of its two children's boxes; an empty leaf
 *      (adopted trees only) gets {+max, -max} and adds nothing to its parent.  Records the walk from the root never reaches
 *      are left untouched.  The boxes never depend on scheduling; refit with the vertices of the build reproduces its boxes.
 *      nrtGetTree_* / nrtGetTreeBounds_* return the refit tree.  Build statistics and nrtLastBuildMs do not change.
 *   3. A committed nrt_scene that instances this context refuses to trace until it is committed again (its top-level boxes
 *      are stale), as after nrtBuild.
 *   4. Ordering: the call-order rules of nrtBuild (not re-entrant with the primitive, build or tree calls on one context).
 *      Both forms first wait on the host for the context's traversal launches in flight.  nrtRefit_* returns when the refit
 *      is complete.  nrtRefitDevice_* reads `d_vertices` (device memory; never staged through the host) and enqueues
 *      everything on `hip_stream` (a hipStream_t; NULL = the default stream) and returns without synchronising: the caller
 *      keeps d_vertices unchanged until the stream reaches the refit.  Every traversal call issued after a refit, on any
 *      stream and through any entry point, is ordered after it.
 *   5. Cost: the first refit after a tree changes builds the tree's level plan on the device; in the steady state (same tree,
 *      repeated frames) a refit allocates nothing.
 * Refusals write nothing (nrtLastError gives the reason): NRT_ERR_INVALID for a NULL context or vertices, no tree (a fresh
 * context included), a sphere or cylinder context, a stride below 3 * sizeof(T), and (Device form) a stride or pointer not
 * aligned to sizeof(T); NRT_ERR_PRECISION when the context holds primitives of the other precision.  The caller's block must
 * hold all num_verts rows: (num_verts - 1) * stride + 3 * sizeof(T) bytes are read.  NRT_ERR_DEVICE (a HIP error once the
 * rewrite has started): the context drops its tree and its primitives rather than keep a half-refit tree; set the mesh again. */
NRT_API nrt_status nrtRefit_f32(nrt_ctx *ctx, const float *vertices, size_t vertex_stride_bytes);
NRT_API nrt_status nrtRefit_f64(nrt_ctx *ctx, const double *vertices, size_t vertex_stride_bytes);
NRT_API nrt_status nrtRefitDevice_f32(nrt_ctx *ctx, const float *d_vertices, size_t vertex_stride_bytes, void *hip_stream);
NRT_API nrt_status nrtRefitDevice_f64(nrt_ctx *ctx, const double *d_vertices, size_t vertex_stride_bytes, void *hip_stream);

/* ---- refit of spheres and curves: the tree's boxes recomputed from moved primitives, its topology kept -------
 * For particles that move and hair that is combed: instead of nrtSetSpheres[Device] / nrtSetCurves[Device] + nrtBuild every
 * frame.  Contract, on a sphere or curve context (fp32) that holds a tree (from nrtBuild_f32 or nrtSetTree_f32):
 *   1. Input: tight arrays in the layout of the kind's setter.  Spheres: `positions` 3 floats and `radii` 1 float per sphere;
 *      curves: `positions` 12 floats (four control points) and `radii` 4 floats per curve.  radii == NULL keeps the context's
 *      radii (particles that move at a fixed size).  `num_prims` is a guard: it must equal the count the context was set with.
 *   2. Result: the context's positions (and radii, if given) become the new ones (a later nrtBuild builds over them).  Every
 *      node record's flag, axis and data[] and the index array stay byte-identical.  Each reachable leaf's box is the min / max
 *      over its slots, in slot order, of the primitive's box as the builder computes it — sphere: centre -/+ radius; curve:
 *      min / max over the four `control point -/+ its radius` — so a refit with the arrays of the build reproduces the build's
 *      boxes.  Each reachable branch's box is the min / max of its two children's; an empty leaf (adopted trees only) gets
 *      {+max, -max}; records the walk from the root never reaches are left untouched.  The leaf records and the private node
 *      arrays of the traversal are derived again as after a build.  num_subdivisions, build statistics and nrtLastBuildMs do
 *      not change.  Inputs that are not finite are outside the box contract: the boxes of a leaf that holds a NaN or an
 *      infinity, and of its ancestors, are unspecified (nothing is read or written out of bounds).
 *   3. A committed nrt_scene that instances this context refuses to trace until it is committed again, as after nrtRefit.
 *   4. Ordering: exactly that of nrtRefit_* / nrtRefitDevice_*.  Both forms first wait on the host for the context's launches
 *      in flight.  nrtRefitPrims_f32 returns when the refit is complete.  nrtRefitPrimsDevice_f32 copies the caller's device
 *      arrays into the context's own buffers and enqueues everything on `hip_stream` (a hipStream_t; NULL = the default stream)
 *      and returns without synchronising: the caller keeps the arrays unchanged until the stream reaches the refit.  Every
 *      traversal call issued after a refit, on any stream and through any entry point, is ordered after it.
 *   5. Cost: as nrtRefit — the first refit of a tree builds its level plan; in the steady state a refit allocates nothing.
 * Refusals write nothing (nrtLastError gives the reason): NRT_ERR_INVALID for a NULL context or NULL positions, no tree (a
 * fresh context included), a triangle context (use nrtRefit_*), a cylinder context (its tree is built over segments the
 * builder cut the cylinders into, and they are not recoverable from the index array), num_prims different from the context's
 * count, and (Device form) a pointer not aligned to 4 bytes; NRT_ERR_PRECISION for a context that holds fp64 primitives.
 * NRT_ERR_DEVICE (a HIP error once the rewrite has started): the context drops its tree and its primitives, as nrtRefit does. */
NRT_API nrt_status nrtRefitPrims_f32(nrt_ctx *ctx, const float *positions, const float *radii, uint32_t num_prims);
NRT_API nrt_status nrtRefitPrimsDevice_f32(nrt_ctx *ctx, const float *d_positions, const float *d_radii, uint32_t num_prims,
                                           void *hip_stream);

/* ---- device-resident geometry: nrtSetMesh_* / nrtSetSpheres_f32 for arrays that are already in HBM ------------------
 * For a mesh or a particle set produced on the GPU (a tensor, a simulation, a remesher): no copy to the host and back.
 * Contract:
 *   1. Input: every pointer is device memory on the context's GPU.  `d_vertices` holds `num_vertices` rows, row i at byte
 *      offset i * vertex_stride_bytes, xyz first; `d_faces` is tight 3 x u32 per face; `d_centers` is tight xyz per sphere and
 *      `d_radii` one radius per sphere.  `hip_stream` is a hipStream_t; NULL = the default stream.
 *   2. Result: exactly the state the matching host call (nrtSetMesh_f32 / _f64, nrtSetSpheres_f32) leaves, given the same array
 *      contents: the same precision, primitive kind and num_faces, positions stored as tight xyz, the tree dropped (a committed
 *      nrt_scene over the context refuses until it is committed again).  A following nrtBuild_* produces a node array and an
 *      index array byte-identical to the host path's.  The context's num_verts is max(faces) + 1 — NOT num_vertices —, so
 *      the refit contract above is unchanged.
 *   3. num_vertices, the guard the host form has no need of: the number of rows the caller's vertex block really holds (a
 *      tensor's shape[0]).  The library computes the largest face index on the device; when it is >= num_vertices the call
 *      returns NRT_ERR_INVALID before it reads a single vertex and before it drops anything: the context keeps its primitives
 *      and its tree and still traces.  A bad index buffer becomes an error string, never an out-of-bounds read.  Rows
 *      0 .. max(faces) are read: at most (num_vertices - 1) * stride + 3 * sizeof(T) bytes.
 *   4. Ordering: the call-order rules of nrtBuild.  The call first waits on the host for the context's launches in flight,
 *      as nrtSetMesh does.  The work is enqueued on `hip_stream`, behind whatever the caller queued there to produce the
 *      buffers, and the call returns when the context owns its copy: the caller may reuse or free the buffers at once, and
 *      a later nrtBuild (on the context's own stream) needs no extra ordering.  The cost of this simplicity is two host
 *      waits per mesh call — a 4-byte read-back of the largest index, and the final wait — and one for spheres.
 * Refusals leave the context untouched (nrtLastError gives the reason): NRT_ERR_INVALID for a NULL context and, with
 * num_faces (num_spheres) > 0, for a NULL pointer, num_vertices == 0, a stride below 3 * sizeof(T), a stride or vertex
 * pointer not aligned to sizeof(T) (the rule of nrtRefitDevice), d_faces not 4-byte aligned (centres or radii not
 * 4-byte aligned), and a face index out of range; NRT_ERR_PRECISION when the context holds primitives of the other precision.
 * num_faces == 0 behaves as in nrtSetMesh: NRT_OK, an empty triangle context, nrtBuild then returns NRT_ERR_EMPTY.
 * NRT_ERR_DEVICE: a HIP error; once the old primitives have been dropped it leaves an empty context.
 * Cylinders have no device form: nrtSetCylinders_f32 plans their segments on the host. */
NRT_API nrt_status nrtSetMeshDevice_f32(nrt_ctx *ctx, const float *d_vertices, uint32_t num_vertices, size_t vertex_stride_bytes,
                                        const uint32_t *d_faces, uint32_t num_faces, void *hip_stream);
NRT_API nrt_status nrtSetMeshDevice_f64(nrt_ctx *ctx, const double *d_vertices, uint32_t num_vertices, size_t vertex_stride_bytes,
                                        const uint32_t *d_faces, uint32_t num_faces, void *hip_stream);
NRT_API nrt_status nrtSetSpheresDevice_f32(nrt_ctx *ctx, const float *d_centers, const float *d_radii, uint32_t num_spheres,
                                           void *hip_stream);

/* ---- traverse: replaces N calls of BVHAccel<T>::Traverse with a
 * TriangleIntersector (nanort.h:757-759, 2487-2556, 1014-1229) -------------
 * Closest hit per ray, same arithmetic as the reference (no contraction,
 * fp64 edge fallback, MaxMult slab test).  options == NULL means
 * BVHTraceOptions() defaults.  hit_mask_out may be NULL. */
NRT_API nrt_status nrtTraverseBatch_f32(nrt_ctx *ctx, const nrt_ray_f32 *rays, uint64_t num_rays,
                                        const nrt_trace_options *options, nrt_hit_f32 *hits_out,
                                        uint8_t *hit_mask_out);
NRT_API nrt_status nrtTraverseBatch_f64(nrt_ctx *ctx, const nrt_ray_f64 *rays, uint64_t num_rays,
                                        const nrt_trace_options *options, nrt_hit_f64 *hits_out,
                                        uint8_t *hit_mask_out);

/* Same, on HBM-resident buffers, asynchronously on `hip_stream`
 * (a hipStream_t; NULL = the default stream).  No host synchronisation. */
NRT_API nrt_status nrtTraverseBatchDevice_f32(nrt_ctx *ctx, const nrt_ray_f32 *d_rays,
                                              uint64_t num_rays, const nrt_trace_options *options,
                                              nrt_hit_f32 *d_hits_out, uint8_t *d_hit_mask_out,
                                              void *hip_stream);
NRT_API nrt_status nrtTraverseBatchDevice_f64(nrt_ctx *ctx, const nrt_ray_f64 *d_rays,
                                              uint64_t num_rays, const nrt_trace_options *options,
                                              nrt_hit_f64 *d_hits_out, uint8_t *d_hit_mask_out,
                                              void *hip_stream);

/* Several independent HBM-resident batches in ONE launch (same trace options; arrays of `num_batches` device pointers and
 * counts; d_masks or any of its entries may be NULL; batch_flags may be NULL).  The persistent kernel hands out the batches as
 * one virtual ray array, so the waves that run dry at the end of one batch carry on with the next: one launch tail instead of
 * `num_batches` (a renderer's shadow and bounce waves, or two tiles, without a second stream).  A batch flagged
 * NRT_BATCH_OCCLUSION is an occlusion query (nrtOccludedBatchDevice's contract: its d_masks entry receives the flags, its
 * d_hits entry is ignored).  Records are exactly those of separate nrtTraverseBatchDevice / nrtOccludedBatchDevice calls.
 * fp64, sphere and cylinder contexts launch the batches one after the other.  Asynchronous on `hip_stream` like
 * nrtTraverseBatchDevice.  (No reference counterpart: nanort.h traces one ray per call, :2487-2556.) */
#define NRT_BATCH_OCCLUSION 1u
NRT_API nrt_status nrtTraverseBatchesDevice_f32(nrt_ctx *ctx, uint32_t num_batches, const nrt_ray_f32 *const *d_rays,
                                                const uint64_t *num_rays, const nrt_trace_options *options,
                                                nrt_hit_f32 *const *d_hits_out, uint8_t *const *d_masks_out,
                                                const uint32_t *batch_flags, void *hip_stream);
NRT_API nrt_status nrtTraverseBatchesDevice_f64(nrt_ctx *ctx, uint32_t num_batches, const nrt_ray_f64 *const *d_rays,
                                                const uint64_t *num_rays, const nrt_trace_options *options,
                                                nrt_hit_f64 *const *d_hits_out, uint8_t *const *d_masks_out,
                                                const uint32_t *batch_flags, void *hip_stream);

/* The same for HOST batches: every batch is uploaded next to the others, ONE launch walks them all, the records come back batch
 * by batch — what a host-shaded wavefront renderer submits together (the shadow query of one depth and the path wave of the
 * next), with one launch tail instead of `num_batches`.  Host pointers in and out, synchronous; at most 2^26 rays per call.
 * An occlusion batch needs its masks_out entry; a closest-hit batch its hits_out entry (masks_out[k] may be NULL).  Unlike the
 * reference's Traverse (nanort.h:1205-1211) — and like nrtTraverseBatch — every record of a closest-hit batch is written: a
 * miss stores {0, 0, ray.max_t, 0xFFFFFFFF}.  Records are exactly those of separate nrtTraverseBatch / nrtOccludedBatch calls. */
NRT_API nrt_status nrtTraverseBatches_f32(nrt_ctx *ctx, uint32_t num_batches, const nrt_ray_f32 *const *rays, const uint64_t *num_rays,
                                          const nrt_trace_options *options, nrt_hit_f32 *const *hits_out, uint8_t *const *masks_out,
                                          const uint32_t *batch_flags);
NRT_API nrt_status nrtTraverseBatches_f64(nrt_ctx *ctx, uint32_t num_batches, const nrt_ray_f64 *const *rays, const uint64_t *num_rays,
                                          const nrt_trace_options *options, nrt_hit_f64 *const *hits_out, uint8_t *const *masks_out,
                                          const uint32_t *batch_flags);

/* ---- per-ray skip ids: BVHTraceOptions::skip_prim_id (nanort.h:617-623, 2387-2395) for every ray of a batch -----------------
 * The reference's answer to self-intersection — a ray that leaves triangle p is traced with skip_prim_id = p and needs no
 * epsilon — works per ray there, because Traverse() takes one ray and that ray's own options.  The batch calls above take one
 * nrt_trace_options per launch; these take, besides it, one id per ray (a bounce or shadow wave: the previous wave's prim_id
 * column; fed back wave after wave: depth peeling).  The contract, for a call that passes `skip_prim_ids`:
 *  - every output of ray i is exactly what the same entry point without the array returns for that ray traced alone with
 *    options->skip_prim_id replaced by skip_prim_ids[i] — bit for bit, under every walk and tunable;
 *  - 0xFFFFFFFF skips nothing, and so does any id at or above the context's number of faces;
 *  - options->skip_prim_id is not read; prim_ids_range and cull_back_face keep their launch-wide meaning;
 *  - skip_prim_ids == NULL is the existing call: the same kernel variant, the same bytes out.
 * Triangle contexts only, both precisions.  Sphere, cylinder and curve contexts refuse with NRT_ERR_INVALID (their intersectors
 * have no skip id), a context of the other precision with NRT_ERR_PRECISION, a device array that is not 4-byte aligned with
 * NRT_ERR_INVALID; a refusal sets nrtLastError and writes nothing.  The host forms upload the ids beside the rays (a batch
 * traced in pieces: each piece with its slice); the Device forms read `d_skip_prim_ids` (num_rays words in HBM) during the
 * launch, asynchronously on `hip_stream`.  nrtOccludedBatchSkip*: mask[i] is the hit flag of the closest-hit form with the same ids.
 * nrtTraverseBatchesSkip*: an array of `num_batches` pointers; the array or any entry of it may be NULL, and a batch with a NULL
 * entry uses options->skip_prim_id; records are exactly those of separate calls (fp32: still one launch, fp64: one after the other).
 * Not covered: nrtMultiHitTraverseBatch*, nrtTraverseCountDevice, nrtTraverseBatchMulti, nrtGroup* and the Embree shim take no per-ray
 * ids; multi-hit takes them through nrtMultiHitQueryBatch* (below), scenes take (primitive, node) pairs through nrtSceneQueryBatch* (below).
 * These calls take Closest / Occlusion launches only; ids together with motion times or visibility words: nrtQueryBatch* below. */
NRT_API nrt_status nrtTraverseBatchSkip_f32(nrt_ctx *ctx, const nrt_ray_f32 *rays, uint64_t num_rays, const nrt_trace_options *options,
                                            const uint32_t *skip_prim_ids, nrt_hit_f32 *hits_out, uint8_t *hit_mask_out);
NRT_API nrt_status nrtTraverseBatchSkip_f64(nrt_ctx *ctx, const nrt_ray_f64 *rays, uint64_t num_rays, const nrt_trace_options *options,
                                            const uint32_t *skip_prim_ids, nrt_hit_f64 *hits_out, uint8_t *hit_mask_out);
NRT_API nrt_status nrtTraverseBatchSkipDevice_f32(nrt_ctx *ctx, const nrt_ray_f32 *d_rays, uint64_t num_rays, const nrt_trace_options *options,
                                                  const uint32_t *d_skip_prim_ids, nrt_hit_f32 *d_hits_out, uint8_t *d_hit_mask_out,
                                                  void *hip_stream);
NRT_API nrt_status nrtTraverseBatchSkipDevice_f64(nrt_ctx *ctx, const nrt_ray_f64 *d_rays, uint64_t num_rays, const nrt_trace_options *options,
                                                  const uint32_t *d_skip_prim_ids, nrt_hit_f64 *d_hits_out, uint8_t *d_hit_mask_out,
                                                  void *hip_stream);
NRT_API nrt_status nrtOccludedBatchSkip_f32(nrt_ctx *ctx, const nrt_ray_f32 *rays, uint64_t num_rays, const nrt_trace_options *options,
                                            const uint32_t *skip_prim_ids, uint8_t *mask_out);
NRT_API nrt_status nrtOccludedBatchSkip_f64(nrt_ctx *ctx, const nrt_ray_f64 *rays, uint64_t num_rays, const nrt_trace_options *options,
                                            const uint32_t *skip_prim_ids, uint8_t *mask_out);
NRT_API nrt_status nrtOccludedBatchSkipDevice_f32(nrt_ctx *ctx, const nrt_ray_f32 *d_rays, uint64_t num_rays, const nrt_trace_options *options,
                                                  const uint32_t *d_skip_prim_ids, uint8_t *d_mask_out, void *hip_stream);
NRT_API nrt_status nrtOccludedBatchSkipDevice_f64(nrt_ctx *ctx, const nrt_ray_f64 *d_rays, uint64_t num_rays, const nrt_trace_options *options,
                                                  const uint32_t *d_skip_prim_ids, uint8_t *d_mask_out, void *hip_stream);
NRT_API nrt_status nrtTraverseBatchesSkipDevice_f32(nrt_ctx *ctx, uint32_t num_batches, const nrt_ray_f32 *const *d_rays,
                                                    const uint64_t *num_rays, const nrt_trace_options *options,
                                                    const uint32_t *const *d_skip_prim_ids, nrt_hit_f32 *const *d_hits_out,
                                                    uint8_t *const *d_masks_out, const uint32_t *batch_flags, void *hip_stream);
NRT_API nrt_status nrtTraverseBatchesSkipDevice_f64(nrt_ctx *ctx, uint32_t num_batches, const nrt_ray_f64 *const *d_rays,
                                                    const uint64_t *num_rays, const nrt_trace_options *options,
                                                    const uint32_t *const *d_skip_prim_ids, nrt_hit_f64 *const *d_hits_out,
                                                    uint8_t *const *d_masks_out, const uint32_t *batch_flags, void *hip_stream);
NRT_API nrt_status nrtTraverseBatchesSkip_f32(nrt_ctx *ctx, uint32_t num_batches, const nrt_ray_f32 *const *rays, const uint64_t *num_rays,
                                              const nrt_trace_options *options, const uint32_t *const *skip_prim_ids,
                                              nrt_hit_f32 *const *hits_out, uint8_t *const *masks_out, const uint32_t *batch_flags);
NRT_API nrt_status nrtTraverseBatchesSkip_f64(nrt_ctx *ctx, uint32_t num_batches, const nrt_ray_f64 *const *rays, const uint64_t *num_rays,
                                              const nrt_trace_options *options, const uint32_t *const *skip_prim_ids,
                                              nrt_hit_f64 *const *hits_out, uint8_t *const *masks_out, const uint32_t *batch_flags);

/* ---- motion blur: a second vertex keyframe and a time per ray ----------------------------------------------------------------
 * An OPT-IN EXTENSION (the reference lists motion blur as open in its TODO).  A triangle context may hold a SECOND VERTEX KEYFRAME:
 * keyframe 0 is what nrtSetMesh* gave, keyframe 1 has the same faces and the same vertex count.  A vertex moves linearly between
 * the two; its position at a ray's time is defined per component, each operation rounded on its own (include/nanort_motion.h — the
 * one statement of the rule, which the device walk and nanort.h's MotionTriangleIntersector both include):
 *
 *     s = (time > 0) ? (time < 1 ? time : 1) : 0        NaN and negatives -> 0, above 1 -> 1
 *     x = (T(1) - s) * a + s * b                          a: keyframe 0, b: keyframe 1
 *     x = x < min(a,b) ? min(a,b) : (x > max(a,b) ? max(a,b) : x)
 *
 * so time 0 is keyframe 0, time 1 is keyframe 1, and every interpolated vertex lies inside the box the builder gives the triangle.
 *
 * Setters.  nrtSetMeshMotion_* copies `vertices_t1` (rows of vertex_stride_bytes, xyz first, as many rows as the mesh has
 * vertices) into the context; nrtSetMeshMotionDevice_* reads device memory on `hip_stream` and refuses a `num_vertices` below the
 * context's vertex count before anything is enqueued.  Both need a triangle context of that precision with a mesh set
 * (NRT_ERR_INVALID / NRT_ERR_PRECISION otherwise, nothing changed), wait for the launches in flight, DROP THE TREE and return when
 * the context owns its copy.  vertices_t1 == NULL removes the keyframe (and drops the tree too).  Every nrtSetMesh* /
 * nrtSetSpheres* / nrtSetCylinders* / nrtSetCurves* removes the keyframe.
 *
 * Trees.  nrtBuild_* on such a context gives every triangle the union of its two keyframes' boxes (per axis the triangle rule on
 * each keyframe, then min / max of the two) and bins it at (c0 + c1) * 0.5; everything else of the build is unchanged, so a
 * keyframe 1 equal to keyframe 0 builds the bytes of a plain build.  nrtSetTree_* adopts the caller's tree as it does today: its
 * boxes are the caller's business (they have to hold both keyframes).  nrtRefit* refuses a context that holds a keyframe.
 *
 * Queries.  `times`: one value per ray, NULL = every ray at time 0.  Records, miss records ({0, 0, max_t, 0xFFFFFFFF}) and masks
 * are those of nrtTraverseBatch*, all three trace options apply; nrtOccludedBatchMotion* writes exactly the closest-hit flag (a ray
 * is settled once its hit distance is < max_t).  The walk is the reference's binary loop over the context's node array with the
 * leaf records of both keyframes interpolated to the ray's time in front of the triangle test: every field of every record is
 * bit-identical to the reference's Traverse over vertices interpolated by the rule above.  The *Device forms are asynchronous on
 * `hip_stream`; nrtBuild / nrtSetTree / nrtSetMesh* / nrtSetMeshMotion* / nrtDestroy wait for them.  A context without a keyframe
 * and contexts of the other primitive kinds are refused (NRT_ERR_INVALID).
 *
 * Every other entry point keeps working on a motion context and answers for keyframe 0 (over the wider boxes).
 * Not covered: the motion queries take one launch-wide skip_prim_id and no visibility words; a time per ray together with an id or
 * a word per ray: nrtQueryBatch* below. */
NRT_API nrt_status nrtSetMeshMotion_f32(nrt_ctx *ctx, const float *vertices_t1, size_t vertex_stride_bytes);
NRT_API nrt_status nrtSetMeshMotion_f64(nrt_ctx *ctx, const double *vertices_t1, size_t vertex_stride_bytes);
NRT_API nrt_status nrtSetMeshMotionDevice_f32(nrt_ctx *ctx, const float *d_vertices_t1, uint32_t num_vertices, size_t vertex_stride_bytes,
                                              void *hip_stream);
NRT_API nrt_status nrtSetMeshMotionDevice_f64(nrt_ctx *ctx, const double *d_vertices_t1, uint32_t num_vertices, size_t vertex_stride_bytes,
                                              void *hip_stream);
NRT_API nrt_status nrtTraverseBatchMotion_f32(nrt_ctx *ctx, const nrt_ray_f32 *rays, const float *times, uint64_t num_rays,
                                              const nrt_trace_options *options, nrt_hit_f32 *hits_out, uint8_t *hit_mask_out);
NRT_API nrt_status nrtTraverseBatchMotion_f64(nrt_ctx *ctx, const nrt_ray_f64 *rays, const double *times, uint64_t num_rays,
                                              const nrt_trace_options *options, nrt_hit_f64 *hits_out, uint8_t *hit_mask_out);
NRT_API nrt_status nrtTraverseBatchMotionDevice_f32(nrt_ctx *ctx, const nrt_ray_f32 *d_rays, const float *d_times, uint64_t num_rays,
                                                    const nrt_trace_options *options, nrt_hit_f32 *d_hits_out, uint8_t *d_mask_out,
                                                    void *hip_stream);
NRT_API nrt_status nrtTraverseBatchMotionDevice_f64(nrt_ctx *ctx, const nrt_ray_f64 *d_rays, const double *d_times, uint64_t num_rays,
                                                    const nrt_trace_options *options, nrt_hit_f64 *d_hits_out, uint8_t *d_mask_out,
                                                    void *hip_stream);
NRT_API nrt_status nrtOccludedBatchMotion_f32(nrt_ctx *ctx, const nrt_ray_f32 *rays, const float *times, uint64_t num_rays,
                                              const nrt_trace_options *options, uint8_t *mask_out);
NRT_API nrt_status nrtOccludedBatchMotion_f64(nrt_ctx *ctx, const nrt_ray_f64 *rays, const double *times, uint64_t num_rays,
                                              const nrt_trace_options *options, uint8_t *mask_out);
NRT_API nrt_status nrtOccludedBatchMotionDevice_f32(nrt_ctx *ctx, const nrt_ray_f32 *d_rays, const float *d_times, uint64_t num_rays,
                                                    const nrt_trace_options *options, uint8_t *d_mask_out, void *hip_stream);
NRT_API nrt_status nrtOccludedBatchMotionDevice_f64(nrt_ctx *ctx, const nrt_ray_f64 *d_rays, const double *d_times, uint64_t num_rays,
                                                    const nrt_trace_options *options, uint8_t *d_mask_out, void *hip_stream);

/* ---- visibility masks: 32 bits per triangle, 32 bits per ray -------------------------------------------------------------------
 * An OPT-IN EXTENSION: visibility by ray type (Embree's ray.mask / rtcSetMask, the instance masks of DXR and OptiX).  The reference's
 * answer is a custom intersection filter through its TriangleIntersector template; user code does not run on the GPU, so here the
 * filter is data: a triangle context may hold ONE 32-BIT WORD PER FACE, a masked query carries one word per ray, and
 *
 *     a triangle exists for a ray  iff  (prim_mask & ray_mask) != 0.
 *
 * (A camera bit, a shadow bit, a reflection bit: a light's geometry without the camera bit, a shadow catcher without the reflection
 * bit, a matte object without the shadow bit; INTEGRATION.md.)
 *
 * Setters.  nrtSetPrimMasks copies `count` words from host memory, one per face in face (prim id) order; nrtSetPrimMasksDevice
 * copies them from device memory on `hip_stream` (4-byte aligned) and returns when the context owns its copy.  Masks have no
 * precision: one pair serves both.  Both need a triangle context with a mesh set and count == its number of faces (NRT_ERR_INVALID
 * otherwise, naming the kind the context holds; nothing changed).  masks == NULL removes the masks (count is not read).
 * The masks belong to the mesh: every nrtSetMesh* / nrtSetSpheres* / nrtSetCylinders* / nrtSetCurves* drops them, as it drops the
 * motion keyframe.  They are NO PART OF THE TREE: setting, changing or removing them keeps the tree, before or after nrtBuild, and
 * nrtBuild / nrtSetTree / nrtRefit* / nrtSetMeshMotion* keep the masks — visibility changes between two queries with no build and
 * no refit.  (The setters wait for the launches in flight; the first masked query behind a change of the masks or of the tree
 * re-derives the words' leaf-order copy on the device and waits for it on the host, some tens of microseconds.)
 *
 * Queries.  nrtTraverseBatchMasked* / nrtOccludedBatchMasked* are nrtTraverseBatch* / nrtOccludedBatch* with `ray_masks`: one word
 * per ray, NULL = every ray carries 0xFFFFFFFF; a ray whose word is 0 sees nothing.  A record is that of the reference's Traverse
 * (nanort.h:2487-2556) over the context's own node array with an intersector that returns false for every triangle the ray does not
 * see: every field of every record is bit-identical to that, a miss is the usual miss record ({0, 0, max_t, 0xFFFFFFFF}), and the
 * occlusion flags are exactly the closest-hit flags.  prim_ids_range, skip_prim_id and cull_back_face keep their launch-wide
 * meaning, on the triangles the ray sees.  With all-ones words on both sides the records are those of nrtTraverseBatch*.  On a
 * context with a motion keyframe they answer for keyframe 0, as nrtTraverseBatch* does.  The host forms upload the words beside
 * the rays (a batch traced in pieces: each piece with its slice); the *Device forms read `d_ray_masks` (num_rays words in HBM,
 * 4-byte aligned) during the launch, asynchronously on `hip_stream`; nrtBuild / nrtSetTree / nrtSetMesh* / nrtSetPrimMasks* /
 * nrtDestroy wait for them.  NRT_ERR_INVALID: a context without masks, a context of another primitive kind, a misaligned
 * `d_ray_masks`; NRT_ERR_PRECISION: a context of the other precision.  A refusal sets nrtLastError and writes nothing.
 *
 * Not covered: every other entry point but nrtQueryBatch* (below: words together with motion times and per-ray skip ids) ignores
 * the masks — multi-hit, the motion queries, the per-ray skip id calls, the batch tables, nrtTraverseBatchMulti, nrtGroup*; inside a
 * scene the triangle words of its mesh contexts are ignored (scenes have words per INSTANCE: "instance visibility masks on a scene",
 * below; the Embree shim's ray.mask stays ignored); spheres, cylinders and curves take no masks. */
NRT_API nrt_status nrtSetPrimMasks(nrt_ctx *ctx, const uint32_t *masks, uint64_t count);
NRT_API nrt_status nrtSetPrimMasksDevice(nrt_ctx *ctx, const uint32_t *d_masks, uint64_t count, void *hip_stream);
NRT_API nrt_status nrtTraverseBatchMasked_f32(nrt_ctx *ctx, const nrt_ray_f32 *rays, const uint32_t *ray_masks, uint64_t num_rays,
                                              const nrt_trace_options *options, nrt_hit_f32 *hits_out, uint8_t *hit_mask_out);
NRT_API nrt_status nrtTraverseBatchMasked_f64(nrt_ctx *ctx, const nrt_ray_f64 *rays, const uint32_t *ray_masks, uint64_t num_rays,
                                              const nrt_trace_options *options, nrt_hit_f64 *hits_out, uint8_t *hit_mask_out);
NRT_API nrt_status nrtTraverseBatchMaskedDevice_f32(nrt_ctx *ctx, const nrt_ray_f32 *d_rays, const uint32_t *d_ray_masks, uint64_t num_rays,
                                                    const nrt_trace_options *options, nrt_hit_f32 *d_hits_out, uint8_t *d_mask_out,
                                                    void *hip_stream);
NRT_API nrt_status nrtTraverseBatchMaskedDevice_f64(nrt_ctx *ctx, const nrt_ray_f64 *d_rays, const uint32_t *d_ray_masks, uint64_t num_rays,
                                                    const nrt_trace_options *options, nrt_hit_f64 *d_hits_out, uint8_t *d_mask_out,
                                                    void *hip_stream);
NRT_API nrt_status nrtOccludedBatchMasked_f32(nrt_ctx *ctx, const nrt_ray_f32 *rays, const uint32_t *ray_masks, uint64_t num_rays,
                                              const nrt_trace_options *options, uint8_t *mask_out);
NRT_API nrt_status nrtOccludedBatchMasked_f64(nrt_ctx *ctx, const nrt_ray_f64 *rays, const uint32_t *ray_masks, uint64_t num_rays,
                                              const nrt_trace_options *options, uint8_t *mask_out);
NRT_API nrt_status nrtOccludedBatchMaskedDevice_f32(nrt_ctx *ctx, const nrt_ray_f32 *d_rays, const uint32_t *d_ray_masks, uint64_t num_rays,
                                                    const nrt_trace_options *options, uint8_t *d_mask_out, void *hip_stream);
NRT_API nrt_status nrtOccludedBatchMaskedDevice_f64(nrt_ctx *ctx, const nrt_ray_f64 *d_rays, const uint32_t *d_ray_masks, uint64_t num_rays,
                                                    const nrt_trace_options *options, uint8_t *d_mask_out, void *hip_stream);

/* ---- one descriptor for every triangle ray query: skip ids, visibility words and motion times on the SAME ray -----------------
 * An OPT-IN EXTENSION.  The three families above each apply one thing per ray and ignore the other two.  A renderer's bounce or
 * shadow wave needs all three at once: the ray leaves a triangle (its skip id), has a type (its word) and, on a moving mesh, a
 * shutter time.  nrtQueryBatch* takes a DESCRIPTOR (nrt_ray_query_f32 / _f64, among the PODs above) that names whichever of them
 * the wave has:
 *
 *     struct_size    sizeof(the descriptor): lets the struct grow
 *     flags          NRT_QUERY_OCCLUSION | NRT_QUERY_MOTION | NRT_QUERY_MASKED
 *     rays, num_rays
 *     options        NULL: the reference's defaults
 *     skip_prim_ids  one id per ray, NULL: options->skip_prim_id for every ray
 *     times          read with MOTION only; NULL: every ray at time 0
 *     ray_masks      read with MASKED only; NULL: every ray 0xFFFFFFFF
 *     hits_out       the records (not read with OCCLUSION)
 *     mask_out       the flags (optional without OCCLUSION, the output with it)
 *
 * Triangle contexts of the call's precision only.
 *
 * Contract.  A record is that of the reference's Traverse (nanort.h:2487-2556) over the context's own node array with an
 * intersector that, for primitive p and ray i,
 *  - returns false WITHOUT TOUCHING THE RAY'S STATE when MASKED is set and (prim_mask[p] & ray_masks[i]) == 0, when p is outside
 *    options->prim_ids_range, or when p is the ray's skip id;
 *  - the ray's skip id is skip_prim_ids[i], or options->skip_prim_id where the array is NULL; 0xFFFFFFFF and every id at or above
 *    the context's number of faces skip nothing;
 *  - with MOTION takes the three corners interpolated to ClampTime(times[i]) by include/nanort_motion.h's rule (the motion blur
 *    section above); without MOTION the corners of keyframe 0;
 *  - then runs TriangleIntersector's own test (nanort.h:1054-1150), cull_back_face included.
 * Every field of every record is bit-identical to that; a miss is {0, 0, max_t, 0xFFFFFFFF}; every record is written.  With
 * OCCLUSION a ray is settled once its hit distance is < max_t, and mask_out[i] is exactly the closest-hit flag.
 *
 * Routing.  A descriptor that an existing call can express IS that call — the same kernel (nrtLastKernelName), the same bytes out:
 *     no flag but OCCLUSION, no ids           nrtTraverseBatch* / nrtOccludedBatch*
 *     ids only                                nrtTraverseBatchSkip* / nrtOccludedBatchSkip*
 *     MOTION only                             nrtTraverseBatchMotion* / nrtOccludedBatchMotion*      (k_traverse_motion)
 *     MASKED only                             nrtTraverseBatchMasked* / nrtOccludedBatchMasked*      (k_traverse_masked)
 *     two or three of ids, MOTION, MASKED     the combined walk (k_traverse_query)
 *
 * Refusals; each writes nothing and sets nrtLastError.  NRT_ERR_INVALID: a NULL context (no message to set) or descriptor; a
 * struct_size other than the struct's; unknown flag bits; NULL rays with num_rays > 0; the kind's output missing (hits_out without
 * OCCLUSION, mask_out with it); MOTION on a context without a keyframe; MASKED on a context without masks; a sphere, cylinder or
 * curve context; a Device array (times, ray_masks, skip_prim_ids) that is not aligned to its element size; no tree; more than
 * 2^31-1 rays.  NRT_ERR_PRECISION: a context of the other precision.  num_rays == 0 is NRT_OK.
 *
 * Ordering: the rules of the motion and masked queries.  nrtQueryBatchDevice_* reads and writes device memory, asynchronously on
 * `hip_stream`; nrtSetMesh* / nrtSetMeshMotion* / nrtSetPrimMasks* / nrtBuild / nrtSetTree / nrtDestroy wait for it.  nrtQueryBatch_*
 * takes host arrays through the staged and (page-locked arrays, nrtHostAlloc) pipelined paths of the calls above; a batch traced
 * in pieces carries, with each piece, its slices of all three per-ray arrays.  The first MASKED query behind a change of the masks
 * or of the tree re-derives the words' leaf-order copy, as a masked query does.
 *
 * Not covered: the batch tables, nrtTraverseBatchMulti, nrtGroup*, scenes and the Embree shim, and the sphere, cylinder and curve
 * kinds keep ignoring what they ignore today.  Multi-hit takes the same three inputs through a descriptor of its own:
 * nrtMultiHitQueryBatch* (next). */
NRT_API nrt_status nrtQueryBatch_f32(nrt_ctx *ctx, const nrt_ray_query_f32 *query);
NRT_API nrt_status nrtQueryBatch_f64(nrt_ctx *ctx, const nrt_ray_query_f64 *query);
NRT_API nrt_status nrtQueryBatchDevice_f32(nrt_ctx *ctx, const nrt_ray_query_f32 *query, void *hip_stream);
NRT_API nrt_status nrtQueryBatchDevice_f64(nrt_ctx *ctx, const nrt_ray_query_f64 *query, void *hip_stream);

/* ---- multi-hit with per-ray skip ids, visibility words and motion times ---------------------------------------------------------
 * An OPT-IN EXTENSION.  A transparent-shadow or transmission wave wants the K frontmost triangles of every ray, and it starts on a
 * surface (its skip id), has a ray type (its word) and, on a moving mesh, a shutter time.  nrtMultiHitQueryBatch* takes a DESCRIPTOR
 * (nrt_multihit_query_f32 / _f64, among the PODs above):
 *
 *     struct_size    sizeof(the descriptor)
 *     flags          NRT_QUERY_MOTION | NRT_QUERY_MASKED  (NRT_QUERY_OCCLUSION is refused: multi-hit has no occlusion form)
 *     rays, num_rays
 *     options        NULL: the reference's defaults
 *     skip_prim_ids  one id per ray, NULL: options->skip_prim_id for every ray
 *     times          read with MOTION only; NULL: every ray at time 0
 *     ray_masks      read with MASKED only; NULL: every ray 0xFFFFFFFF
 *     hits_out       num_rays * max_hits records
 *     counts_out     one word per ray, may be NULL
 *     max_hits       K, 1..NRT_MAX_MULTIHIT
 *     reserved       must be 0
 *
 * Triangle contexts of the call's precision only.
 *
 * Contract.  The multi-hit contract (items 1-5 above nrtMultiHitTraverseBatch*) in which "TriangleIntersector::Intersect" is the
 * intersector of the nrtQueryBatch* contract.  For primitive p and ray i that intersector returns false WITHOUT TOUCHING THE RAY'S
 * STATE — p is no candidate — when MASKED is set and (prim_mask[p] & ray_masks[i]) == 0, when p is outside options->prim_ids_range,
 * or when p is the ray's skip id: skip_prim_ids[i], or options->skip_prim_id where the array is NULL; 0xFFFFFFFF and every id at or
 * above the context's number of faces skip nothing.  Otherwise it tests, with MOTION, the three corners interpolated to
 * ClampTime(times[i]) by include/nanort_motion.h's rule, and without MOTION the corners of keyframe 0.  The rest is the multi-hit
 * contract unchanged: the reference's binary loop over the context's node array with B as defined there, ranking by (t, prim_id),
 * the K-buffer in the ray's own row, unused slots = the miss record {0, 0, max_t, 0xFFFFFFFF}, every byte written.
 * K = 1: count and t equal nrtQueryBatch*'s flag and t with the same arrays and flags on every ray; prim_id / u / v differ only at
 * exact-t ties, where multi-hit names the smaller id.
 *
 * Routing.  A descriptor with no flag and no ids IS nrtMultiHitTraverseBatch* — the same kernel (nrtLastKernelName:
 * nrt::k_traverse_multihit<...>), the same bytes out.  Everything else — ids alone included, which no other call can express — runs
 * nrt::k_multihit_query<T, 32, MOTION, MASKED>.
 *
 * Refusals; each writes nothing and sets nrtLastError, naming nrtMultiHitQueryBatch.  NRT_ERR_INVALID: a NULL context (no message to
 * set) or descriptor; a struct_size other than the struct's; unknown flag bits or NRT_QUERY_OCCLUSION; reserved != 0; K == 0 or
 * K > NRT_MAX_MULTIHIT; NULL rays or hits_out with num_rays > 0; MOTION on a context without a keyframe; MASKED on a context without
 * masks; a sphere, cylinder or curve context; a Device array (times, ray_masks, skip_prim_ids, counts_out) that is not aligned to its
 * element size; no tree; more than 2^31-1 rays.  NRT_ERR_PRECISION: a context of the other precision.  num_rays == 0 is NRT_OK.
 *
 * Ordering: the rules of multi-hit and of the masked queries.  The launch takes one of the context's launch slots and closes it with
 * an event; nrtSetMesh* / nrtSetMeshMotion* / nrtSetPrimMasks* / nrtBuild / nrtSetTree / nrtDestroy wait for it.  The first MASKED
 * query behind a change of the masks or of the tree re-derives the words' leaf-order copy.  nrtMultiHitQueryBatch_* takes host arrays
 * through the staged path of nrtMultiHitTraverseBatch_* (pieces whose rows stay within 256 MiB); each piece carries its slices of
 * all three per-ray arrays.
 *
 * Not covered: scenes, the sphere, cylinder and curve kinds, the batch tables, nrtTraverseBatchMulti, nrtGroup* and the Embree shim. */
NRT_API nrt_status nrtMultiHitQueryBatch_f32(nrt_ctx *ctx, const nrt_multihit_query_f32 *query);
NRT_API nrt_status nrtMultiHitQueryBatch_f64(nrt_ctx *ctx, const nrt_multihit_query_f64 *query);
NRT_API nrt_status nrtMultiHitQueryBatchDevice_f32(nrt_ctx *ctx, const nrt_multihit_query_f32 *query, void *hip_stream);
NRT_API nrt_status nrtMultiHitQueryBatchDevice_f64(nrt_ctx *ctx, const nrt_multihit_query_f64 *query, void *hip_stream);

/* ---- closest-point queries ------------------------------------------------------------------------------------------------------
 * Which triangle of the context's mesh is nearest to a point, and where on it — the question Embree answers with rtcPointQuery, over
 * the tree nrtBuild / nrtSetTree / nrtRefit left in HBM.  (No reference counterpart.)  DESIGN.md §3.17.
 *
 * The rule is include/nanort_closest.h's, in the context's precision, every operation rounded on its own: per face
 * ClosestPointOnTriangle takes the nearest of the three clamped edge projections and, where it falls inside, the foot of the
 * perpendicular, and gives (u, v) — u the weight of the face's second vertex, v of its third, as in the ray hit records — the point
 * and dist2.  Accuracy: sqrt(dist2) is within 8 eps S of the true distance to the nearest admitted face, eps the precision's and S
 * the largest absolute coordinate among the points and the vertices, on triangles of any shape — slivers, needles, corners in line.
 * Among the faces the options admit (prim_ids_range, skip_prim_id as in a ray query;
 * cull_back_face is ignored) the answer is the face with the smallest dist2, among equal dist2 the smallest prim_id.  A face counts
 * only if dist2 <= r2 = max_dist * max_dist: equality counts, max_dist = +inf is allowed, a NaN or negative max_dist finds nothing,
 * a face whose dist2 is NaN is never the answer, a point with a non-finite coordinate finds nothing.  The answer is a minimum with a
 * total tie-break, so it does not depend on the tree: a record is byte-identical to a loop over all the faces with the same rule.
 *
 * Found: point = the nearest point, dist2, u, v, prim_id.  Not found: point = p, dist2 = r2, u = v = 0, prim_id = 0xFFFFFFFF.
 * _pad is written as 0.  found_out (may be NULL) receives 1 / 0 per point.
 *
 * A context with a motion keyframe answers for keyframe 0.  An adopted tree (nrtSetTree) is inside the contract when every box
 * contains the triangles below it.  Runs nrt::k_closest_point<T, 32> (nrtLastKernelName).
 *
 * Refusals; each writes nothing and sets nrtLastError.  NRT_ERR_INVALID: a NULL context (no message to set); NULL points or
 * closest_out with num_points > 0; no tree; a sphere, cylinder or curve context; more than 2^31-1 points; a Device array that is not
 * aligned (points and closest_out to 16 bytes in fp32 and 8 in fp64).  NRT_ERR_PRECISION: a context of the other precision.
 * num_points == 0 is NRT_OK.
 *
 * nrtClosestPointBatch_* takes host arrays, staged through the context's grow-only buffers in pieces of 2^20 points, one host call at
 * a time.  nrtClosestPointBatchDevice_* takes device arrays and is asynchronous on `hip_stream`; it takes one of the context's launch
 * slots and closes it with an event, so nrtSetMesh* / nrtBuild / nrtSetTree / nrtRefit* / nrtDestroy wait for it.
 *
 * Not covered: the sphere, cylinder and curve kinds, per-point skip ids or masks, motion time.  (The k nearest faces:
 * "nearest-faces queries" below; instanced scenes: nrtSceneClosestPointBatch*, at the end of the scene calls.) */
NRT_API nrt_status nrtClosestPointBatch_f32(nrt_ctx *ctx, const nrt_point_f32 *points, uint64_t num_points, const nrt_trace_options *options,
                                            nrt_closest_f32 *closest_out, uint8_t *found_out);
NRT_API nrt_status nrtClosestPointBatch_f64(nrt_ctx *ctx, const nrt_point_f64 *points, uint64_t num_points, const nrt_trace_options *options,
                                            nrt_closest_f64 *closest_out, uint8_t *found_out);
NRT_API nrt_status nrtClosestPointBatchDevice_f32(nrt_ctx *ctx, const nrt_point_f32 *points, uint64_t num_points, const nrt_trace_options *options,
                                                  nrt_closest_f32 *closest_out, uint8_t *found_out, void *hip_stream);
NRT_API nrt_status nrtClosestPointBatchDevice_f64(nrt_ctx *ctx, const nrt_point_f64 *points, uint64_t num_points, const nrt_trace_options *options,
                                                  nrt_closest_f64 *closest_out, uint8_t *found_out, void *hip_stream);

/* ---- signed distance queries ----------------------------------------------------------------------------------------------------
 * The closest-point query above, and on which side of the surface the point lies: what a signed distance field, a voxelisation or
 * a containment test needs.  DESIGN.md §3.18.
 *
 * The rule is include/nanort_sdf.h's (Baerentzen and Aanaes 2005, the angle-weighted pseudonormal).  ClosestFeatureOnTriangle is
 * ClosestPointOnTriangle — point, dist2, u, v and prim_id are the closest-point query's, byte for byte — and also says which of
 * its candidates won: the face's interior, one of its edges, one of its vertices (an edge candidate clamped to an end is that
 * vertex).  The point is inside exactly when (p - point) . n < 0 for the pseudonormal n of that feature: the face's unit normal; at
 * an edge the sum of the unit normals of all faces that hold both of its vertex indices; at a vertex the sum over its corners of
 * corner angle times unit normal.  Outside is the side from which a face's vertices run counter-clockwise.  A zero or NaN product —
 * a point on the surface, a zero normal — is "not inside".  The squared distance stays unsigned: sign it by bit 31 of `feature`.
 *
 * The normals are derived on the GPU from the mesh where it lies, by the first signed query (or nrtGetFeatureNormals_*) after any
 * nrtSetMesh* or nrtRefit*: nothing is downloaded, and the same mesh gives the same bytes on every run (no floating-point atomics).
 * They belong to the mesh, not to the tree: nrtBuild, nrtSetTree, nrtSetPrimMasks* and nrtSetMeshMotion* leave them alone, and
 * prim_ids_range and skip_prim_id restrict the faces SEARCHED as before while the normals are always those of the WHOLE mesh (an
 * edge normal still sums faces the options exclude).  Vertices are identified by index, not by position: an unwelded mesh has
 * only boundary edges, and its signs are those of the face normals.  A context with a motion keyframe answers for keyframe 0.
 *
 * Not found: the closest-point query's record, feature = 0.  Runs nrt::k_signed_distance<T, 32> (nrtLastKernelName).
 *
 * Arguments, entry checks, refusals (each writes nothing), staging, launch slots and events are nrtClosestPointBatch*'s; one more
 * refusal, NRT_ERR_INVALID: a mesh of more than floor((2^32 - 1) / 3) faces.
 *
 * nrtGetFeatureNormals_*: face_normals_out [num_faces][4][3] (the unit normal, then the edge normals of ab, ac, bc) and
 * vertex_normals_out [num_verts][3] (num_verts: the mesh's largest vertex index + 1), refreshed first if stale, to HOST arrays;
 * either pointer may be NULL.  Needs a triangle mesh, not a tree.  For shading with the normals, and for the tests.
 *
 * The sign is guaranteed on closed, consistently oriented meshes without zero-area faces.  Elsewhere — open boundaries, zero-area
 * faces, non-manifold edges — it is what the rule gives: byte-reproducible, not guaranteed to be meaningful.
 * Not covered: scenes, the sphere, cylinder and curve kinds, welding by position. */
NRT_API nrt_status nrtSignedDistanceBatch_f32(nrt_ctx *ctx, const nrt_point_f32 *points, uint64_t num_points, const nrt_trace_options *options,
                                              nrt_signed_f32 *signed_out, uint8_t *found_out);
NRT_API nrt_status nrtSignedDistanceBatch_f64(nrt_ctx *ctx, const nrt_point_f64 *points, uint64_t num_points, const nrt_trace_options *options,
                                              nrt_signed_f64 *signed_out, uint8_t *found_out);
NRT_API nrt_status nrtSignedDistanceBatchDevice_f32(nrt_ctx *ctx, const nrt_point_f32 *points, uint64_t num_points, const nrt_trace_options *options,
                                                    nrt_signed_f32 *signed_out, uint8_t *found_out, void *hip_stream);
NRT_API nrt_status nrtSignedDistanceBatchDevice_f64(nrt_ctx *ctx, const nrt_point_f64 *points, uint64_t num_points, const nrt_trace_options *options,
                                                    nrt_signed_f64 *signed_out, uint8_t *found_out, void *hip_stream);
NRT_API nrt_status nrtGetFeatureNormals_f32(nrt_ctx *ctx, float *face_normals_out /* [num_faces][4][3] */, float *vertex_normals_out /* [num_verts][3] */);
NRT_API nrt_status nrtGetFeatureNormals_f64(nrt_ctx *ctx, double *face_normals_out /* [num_faces][4][3] */, double *vertex_normals_out /* [num_verts][3] */);

/* ---- nearest-faces queries ------------------------------------------------------------------------------------------------------
 * The K = max_faces faces of the context's mesh nearest to a point, in order, 1 <= K <= NRT_MAX_NEAREST — what contact generation
 * (every face within a radius), attribute transfer (the few nearest faces) and inside/outside voting need, and what an Embree user
 * writes as an rtcPointQuery callback that collects.  It is to nrtClosestPointBatch* what nrtMultiHitTraverseBatch* is to the
 * closest hit.  DESIGN.md §3.19.
 *
 * The rule is include/nanort_closest.h's.  The CANDIDATES of point i are the faces the options admit (prim_ids_range, skip_prim_id
 * exactly as in nrtClosestPointBatch*; cull_back_face is ignored) whose dist2 from ClosestPointOnTriangle is not NaN and
 * <= r2 = max_dist * max_dist; a point with a non-finite coordinate, a NaN or a negative max_dist has none.  They are ranked by the
 * key (dist2, prim_id) ascending: dist2 numerically, then prim_id.
 *
 *   nearest_out[i * K + j], j < count[i]   the candidates with the K smallest keys, in ascending key order; each is exactly the FOUND
 *                                          record nrtClosestPointBatch* would write for that face alone: point, dist2, u, v, prim_id,
 *                                          _pad = 0
 *   nearest_out[i * K + j], j >= count[i]  the NOT FOUND record: point = p, dist2 = r2, u = v = 0, prim_id = 0xFFFFFFFF, _pad = 0
 *   counts_out[i] (may be NULL)            count[i] = min(K, number of candidates)
 *
 * Every byte of every row is written.  The result is byte-identical to sorting all admitted faces by the key and taking the first
 * K: it does not depend on the tree (nrtBuild, nrtSetTree, nrtRefit) nor on the order in which a walk meets the faces.  With K = 1
 * the record is nrtClosestPointBatch*'s byte for byte and count equals its found byte.
 *
 * A context with a motion keyframe answers for keyframe 0.  An adopted tree (nrtSetTree) is inside the contract when every box
 * contains the triangles below it.  Runs nrt::k_nearest_faces<T, 32> (nrtLastKernelName).
 *
 * Refusals; each writes nothing and sets nrtLastError.  NRT_ERR_INVALID: max_faces == 0 or > NRT_MAX_NEAREST, and everything
 * nrtClosestPointBatch* refuses — a NULL context (no message to set); NULL points or nearest_out with num_points > 0; no tree; a
 * sphere, cylinder or curve context; more than 2^31-1 points; a Device array that is not aligned (points and nearest_out to 16 bytes
 * in fp32 and 8 in fp64, counts_out to 4).  NRT_ERR_PRECISION: a context of the other precision.  num_points == 0 is NRT_OK.
 *
 * nrtNearestFacesBatch_* takes host arrays, staged through the context's grow-only buffers, one host call at a time, in pieces of
 * max(1, 2^20 / K) points (integer division): a piece stages no more records than a piece of nrtClosestPointBatch_*.
 * nrtNearestFacesBatchDevice_* takes device arrays and is asynchronous on `hip_stream`; launch slot and event as
 * nrtClosestPointBatchDevice_*'s.  While it runs, a point's row holds the candidates found so far: read it after the stream has passed
 * the launch.
 *
 * Not covered: scenes, the sphere, cylinder and curve kinds, a signed form, per-point skip ids or masks, motion time, more than
 * NRT_MAX_NEAREST faces per point. */
#define NRT_MAX_NEAREST 64u
NRT_API nrt_status nrtNearestFacesBatch_f32(nrt_ctx *ctx, const nrt_point_f32 *points, uint64_t num_points, uint32_t max_faces,
                                            const nrt_trace_options *options, nrt_closest_f32 *nearest_out, uint32_t *counts_out);
NRT_API nrt_status nrtNearestFacesBatch_f64(nrt_ctx *ctx, const nrt_point_f64 *points, uint64_t num_points, uint32_t max_faces,
                                            const nrt_trace_options *options, nrt_closest_f64 *nearest_out, uint32_t *counts_out);
NRT_API nrt_status nrtNearestFacesBatchDevice_f32(nrt_ctx *ctx, const nrt_point_f32 *points, uint64_t num_points, uint32_t max_faces,
                                                  const nrt_trace_options *options, nrt_closest_f32 *nearest_out, uint32_t *counts_out, void *hip_stream);
NRT_API nrt_status nrtNearestFacesBatchDevice_f64(nrt_ctx *ctx, const nrt_point_f64 *points, uint64_t num_points, uint32_t max_faces,
                                                  const nrt_trace_options *options, nrt_closest_f64 *nearest_out, uint32_t *counts_out, void *hip_stream);

/* One HOST batch spread over several contexts — typically one per GPU of the node (nrtDeviceCount), each holding the same
 * tree: nrtBuild is deterministic, so building the same mesh on every context gives bit-identical replicas (or nrtSetTree the
 * same arrays).  The batch is cut into rows of `row_len` rays (an image row; 0 = 4096) and row r is traced by context
 * r % num_ctx — the interleaved image-tile split of SURVEY.md §8(e); each context is driven by its own host thread and its
 * GPU copies its rows of the records (and flags, when hit_mask_out is not NULL) straight into the caller's arrays, which are
 * written in full like nrtTraverseBatch's.  Records are exactly those of nrtTraverseBatch on one context.  Page-locked caller
 * buffers (nrtHostAlloc) let the copies of different GPUs overlap at PCIe speed.  Errors: NRT_ERR_INVALID when a context is
 * NULL, listed twice, of another precision, without a triangle tree or with another tree than context 0's.
 * (No reference counterpart: the reference's only parallel loop is the example's OpenMP row loop,
 * examples/path_tracer/main.cc:785-806.) */
NRT_API nrt_status nrtTraverseBatchMulti_f32(nrt_ctx *const *ctxs, uint32_t num_ctx, const nrt_ray_f32 *rays, uint64_t num_rays,
                                             uint64_t row_len, const nrt_trace_options *options, nrt_hit_f32 *hits_out,
                                             uint8_t *hit_mask_out);
NRT_API nrt_status nrtTraverseBatchMulti_f64(nrt_ctx *const *ctxs, uint32_t num_ctx, const nrt_ray_f64 *rays, uint64_t num_rays,
                                             uint64_t row_len, const nrt_trace_options *options, nrt_hit_f64 *hits_out,
                                             uint8_t *hit_mask_out);
/* HIP devices visible to this process (0 when there is none or the runtime cannot be initialised). */
NRT_API int nrtDeviceCount(void);

/* ---- multi-GPU with DEVICE-RESIDENT rays: tiles traced where they live, hit records gathered to one GPU by RCCL ----------
 * replicated BVH, image-tile split, RCCL gather of the 16 / 32-byte records over xGMI.  (No reference
 * counterpart: examples/path_tracer/main.cc:785-806 is the reference's only parallel loop.)  A frame of `total_rays` rays is
 * cut into rows of `row_len` rays (0 = 4096); tile t of N owns the interleaved rows t, t + N, t + 2N, ... in that order
 * (nrtGroupTileRays gives its size) — the split of nrtTraverseBatchMulti.  Every tile belongs to one context holding a replica
 * of the tree (nrtBuild is deterministic: the same mesh gives bit-identical replicas).
 *   nrtGroupCreate        ONE process drives all N contexts, normally one per GPU (several on one GPU work: their records are
 *                         read in place); one RCCL rank per distinct device.
 *   nrtGroupCreateRanked  one process per GPU: this process owns tile `rank` of `nranks`; `unique_id` = the 128 bytes rank 0
 *                         got from nrtGroupUniqueId, handed round by the host program.
 * RCCL is bound at run time (librccl.so.1 — the process's own copy when a framework has loaded one); when it cannot be, a
 * single-process group moves the records with hipMemcpyPeerAsync instead and nrtGroupLastError(group) says so.
 * nrtGroupTraverseGather_*: d_rays[k] / counts[k] describe this process's k-th tile (device pointers on that tile's GPU,
 * complete before the call).  Every tile is traced on a stream of the group (nrtTraverseBatchDevice_* semantics: every record
 * written, a miss = {0, 0, max_t, ~0}); tiles on other GPUs than the root tile's send their records (ncclSend / ncclRecv in one
 * group call); a kernel on the root GPU writes them to d_frame_hits[total_rays] (and flags to d_frame_mask, optional) in FRAME
 * order.  Only the process owning `root_tile` passes frame pointers (memory of the root tile's GPU); the others pass NULL.  The
 * call returns once everything is enqueued: nrtGroupSynchronize before reading the frame or reusing the ray buffers.  Frames
 * are byte-identical to nrtTraverseBatchDevice_* over the whole ray array on one context.
 * Tunables: "transport" (0 RCCL, 1 peer copies; single-process groups), "self_send" (1: the root tile's own records take the
 * send / receive path too — lets a one-GPU box execute the exchange). */
typedef struct nrt_group nrt_group;
NRT_API nrt_status nrtGroupUniqueId(void *id_out, size_t bytes /* >= 128 */);
NRT_API nrt_status nrtGroupCreate(nrt_ctx *const *ctxs, uint32_t num_ctx, nrt_group **out);
NRT_API nrt_status nrtGroupCreateRanked(nrt_ctx *ctx, const void *unique_id, int rank, int nranks, nrt_group **out);
NRT_API void nrtGroupDestroy(nrt_group *group);
NRT_API const char *nrtGroupLastError(const nrt_group *group); /* NULL: the calling thread's last creation error */
NRT_API nrt_status nrtGroupSetTunable(nrt_group *group, const char *name, long long value);
NRT_API nrt_status nrtGroupInfo(const nrt_group *group, uint32_t *num_tiles_out, uint32_t *num_local_out, int *nranks_out, int *rccl_bound_out);
NRT_API uint64_t nrtGroupTileRays(uint64_t total_rays, uint64_t row_len, uint32_t tile, uint32_t num_tiles);
NRT_API nrt_status nrtGroupTraverseGather_f32(nrt_group *group, const nrt_ray_f32 *const *d_rays, const uint64_t *counts, uint64_t total_rays,
                                              uint64_t row_len, const nrt_trace_options *options, uint32_t root_tile, nrt_hit_f32 *d_frame_hits,
                                              uint8_t *d_frame_mask);
NRT_API nrt_status nrtGroupTraverseGather_f64(nrt_group *group, const nrt_ray_f64 *const *d_rays, const uint64_t *counts, uint64_t total_rays,
                                              uint64_t row_len, const nrt_trace_options *options, uint32_t root_tile, nrt_hit_f64 *d_frame_hits,
                                              uint8_t *d_frame_mask);
/* Ragged waves (secondary rays: every tile has its own number of them) — TILE-MAJOR gather: tile t traces counts[k] <= slot_rays
 * rays and the root receives the tile's whole slot at d_tiles_hits + t * slot_rays (and d_tiles_mask + t * slot_rays, optional);
 * records past a tile's count are undefined.  No frame order to restore: RCCL receives straight into the caller's array. */
NRT_API nrt_status nrtGroupTraverseGatherTiles_f32(nrt_group *group, const nrt_ray_f32 *const *d_rays, const uint64_t *counts, uint64_t slot_rays,
                                                   const nrt_trace_options *options, uint32_t root_tile, nrt_hit_f32 *d_tiles_hits,
                                                   uint8_t *d_tiles_mask);
NRT_API nrt_status nrtGroupTraverseGatherTiles_f64(nrt_group *group, const nrt_ray_f64 *const *d_rays, const uint64_t *counts, uint64_t slot_rays,
                                                   const nrt_trace_options *options, uint32_t root_tile, nrt_hit_f64 *d_tiles_hits,
                                                   uint8_t *d_tiles_mask);
NRT_API nrt_status nrtGroupSynchronize(nrt_group *group);
/* bytes the last gather moved by RCCL / by peer copies / read in place on the root GPU */
NRT_API nrt_status nrtGroupLastTraffic(const nrt_group *group, uint64_t *bytes_rccl, uint64_t *bytes_peer, uint64_t *bytes_in_place);

/* Measurement aid: run the batch once on HBM-resident rays with the work
 * counters on (synchronous; results are not written).  Used by bench.py to
 * turn kernel time into algorithmic bytes per SURVEY.md §8(d). */
NRT_API nrt_status nrtTraverseCountDevice_f32(nrt_ctx *ctx, const nrt_ray_f32 *d_rays,
                                              uint64_t num_rays, const nrt_trace_options *options,
                                              nrt_trace_counters *counters_out);
NRT_API nrt_status nrtTraverseCountDevice_f64(nrt_ctx *ctx, const nrt_ray_f64 *d_rays,
                                              uint64_t num_rays, const nrt_trace_options *options,
                                              nrt_trace_counters *counters_out);

/* Device time (ms) of the most recent traversal launch (the kernel's own start / end stamps, or HIP events on the
 * launch stream: see nrtSetLaunchTiming) / build (HIP events) on this context; < 0 if none has completed.
 * Synchronises with that work: when it returns, the launch's stream has drained (the records have landed). */
NRT_API float nrtLastTraverseMs(nrt_ctx *ctx);
NRT_API float nrtLastBuildMs(nrt_ctx *ctx);
/* By default a traversal launch records NO event in the caller's stream (an event record between two kernels of a stream
 * keeps the second from starting for ~8 us; three per launch cost C3 6.5 % of a step): the kernel's last wave publishes a
 * completion record — sequence number, start and end stamps — in page-locked memory.  nrtLastTraverseMs reads those stamps
 * (first block started -> last wave finished), and whatever must wait for launches in flight (nrtBuild / nrtSetMesh /
 * nrtSetTree / nrtDestroy, a fifth stream launching concurrently on one context) waits for exactly those launches by polling
 * their records.  on = 1 brackets every launch with a pair of timing events and follows it with a completion event instead
 * (nrtLastTraverseMs then reports the event time, dispatch included) — a cross-check, not the fast path.  A launch made while
 * its stream is being CAPTURED into a graph does not run, so its record never completes: capture traversal launches only on
 * contexts that are not rebuilt or destroyed before the graph has been launched and has finished (or use on = 1 while capturing).  (For the sphere
 * and cylinder kinds the record is closed by their post pass; the literal BVHNode kernel always uses events.)
 * (No reference counterpart.) */
NRT_API nrt_status nrtSetLaunchTiming(nrt_ctx *ctx, int on);
/* Traversal / build tunables by name (no reference counterpart; the library's defaults are the measured optimum on MI355X):
 *   which walk        "wide" (0: the literal BVHNode loop), "wide4" (two tree levels per step; next build / set_tree),
 *                     "order4" (0, the default: a record's four slots in the binary loop's order, nanort.h:2538-2543 — the same
 *                     leaves in the same order as the reference, every field of every record bit-identical to it on the same
 *                     node array; 1, opt-in, 2...5 % faster: slots entered by entry distance — another leaf sequence, so among
 *                     primitives at EXACTLY the same t another one may be named (prim_id / u / v), and where a leaf box's entry
 *                     distance rounds above the distance of a hit inside it the box may be culled under another hit and t itself
 *                     differ by its last bits: contract-level parity, SURVEY.md §8d, not the bit-exact class), "f64_row_fetch"
 *   scheduling        "refill_min", "trav_min", "trav_min4", "leaf_min", "chunk", "chunk_tail_pct", "parts",
 *                     "static_pct", "static_bands", "static_slice_groups", "blocks_per_cu", "lds_stack", "wide_stack"
 *   builder           "morton" (Morton pre-pass); libnanort_hip_prof.so only: "subtree_rows" (0: the one-node-per-step subtree kernel; same tree)
 *   launches / host   "launch_timing" (== nrtSetLaunchTiming), "host_pipeline"
 *   probes            "debug" (bit mask: 1 / 2 skip triangle tests / traversal; the profiling bits 4 — non-temporal ray loads —,
 *                     32 / 64 / 8192 act in libnanort_hip_prof.so only), "wide_scramble" (layout probe; next build)
 * Values are clamped to the tunable's range; an unknown name is NRT_ERR_INVALID.  Tunables that shape the private tree layout
 * ("wide4", "wide_scramble", "morton") take effect with the next nrtBuild / nrtSetTree.  The environment variable
 * NRT_<NAME> (upper case) overrides a default at nrtCreate ONLY when the process also sets NRT_ALLOW_ENV=1 (libnanort_hip_prof.so:
 * always) — a debugging aid; a stray variable cannot move a product context to another walk.  Programs use these calls. */
NRT_API nrt_status nrtSetTunable(nrt_ctx *ctx, const char *name, long long value);
NRT_API nrt_status nrtGetTunable(nrt_ctx *ctx, const char *name, long long *value_out);
/* Name of the traversal kernel variant the most recent traversal launch of this context used, spelled as
 * rocprofv3 prints it without the argument list (static storage; "" before the first launch).  bench.py
 * reports it in `roofline.kernel` and matches the counter rows of its PMC passes against it. */
NRT_API const char *nrtLastKernelName(const nrt_ctx *ctx);
/* (The profiling entry points — loop-occupancy counters, per-wave time stamps — are not part of this library: they live in
 * libnanort_hip_prof.so, declared in nanort_hip_prof.h, together with the counting / clocked kernel instantiations.) */

/* ---- two-level scenes (instancing): replaces nanosg::Scene<float, M> -----------------------
 * examples/nanosg/nanosg.h — AddNode :682, Commit :700-760 (per-node world AABB / inverse
 * transforms, nanosg.h:397-437), Traverse :773-870 on top of BVHAccel::ListNodeIntersections
 * (nanort.h:781-784, 2608-2692).  Semantics kept, including the reference's quirks: the 64 nearest
 * node boxes by entry distance are considered (kMaxIntersections), front to back with the early
 * cull `t_nearest < t_min`; the local ray carries the default [0, FLT_MAX] interval and default
 * trace options (the world ray's interval and the cull flag never reach the per-node Traverse);
 * the reported t is the WORLD distance |xform(P_local) - org| and a node replaces the current hit
 * only when strictly nearer.  Nodes entered at exactly the same distance are visited in node order (the
 * reference: in the order its std::priority_queue pops them), which only shows when several COINCIDENT
 * instances produce the same hit record: either may be named in node_id.  A node is a built nrt_ctx (f32) plus nanosg's T[4][4] local transform
 * (row 3 = translation, nanosg.h:232-240); the mesh contexts must outlive the scene, and nrtSceneCommit caches where their trees
 * live: after nrtBuild / nrtSetMesh / nrtSetTree on a mesh context the scene has to be committed again (until then
 * nrtSceneTraverseBatch* fail with NRT_ERR_INVALID instead of walking the old buffers). */
typedef struct nrt_scene nrt_scene;
typedef struct {
  float t;
  float u;
  float v;
  uint32_t prim_id;
  uint32_t node_id;
} nrt_scene_hit_f32; /* the fields of nanosg::Intersection<float> the traversal fills; miss: t = ray.max_t, ids = 0xFFFFFFFF */

NRT_API nrt_status nrtSceneCreate(int device, nrt_scene **out);
NRT_API void nrtSceneDestroy(nrt_scene *scene);
NRT_API const char *nrtSceneLastError(const nrt_scene *scene);
NRT_API nrt_status nrtSceneAddNode_f32(nrt_scene *scene, nrt_ctx *built_mesh, const float local_xform[16],
                                       uint32_t *node_id_out);
NRT_API nrt_status nrtSceneCommit(nrt_scene *scene);
/* The matrices Node::Update derives for node `node_id` (nanosg.h:397-437), valid after nrtSceneCommit: xform,
 * inv_xform, inv_xform33, inv_transpose_xform33 — 16 floats each (nanosg's row-major T[4][4]), 64 in all. */
NRT_API nrt_status nrtSceneNodeState_f32(nrt_scene *scene, uint32_t node_id, float out[64]);
/* Scene::GetBoundingBox (nanosg.h:761-769): union of the nodes' world boxes, valid after nrtSceneCommit. */
NRT_API nrt_status nrtSceneBounds_f32(nrt_scene *scene, float bmin[3], float bmax[3]);
NRT_API nrt_status nrtSceneTraverseBatch_f32(nrt_scene *scene, const nrt_ray_f32 *rays, uint64_t num_rays,
                                             nrt_scene_hit_f32 *hits_out, uint8_t *hit_mask_out);

/* The same traversal with rays and results resident in HBM (device pointers; d_mask_out may be NULL): no PCIe traffic.
 * On the scene's own stream: scenes of 64 nodes or more — ONE launch of the single-pass walk (top-level tree and instance trees on
 * one per-lane stack, no per-ray list), a 4-byte read-back, and only if the walk handed rays over, the two launches below on
 * those; scenes of at most 8 nodes — ONE launch (the trace kernel tests every world box itself as it fetches a ray); 9 to 63
 * nodes — two launches (the listing over the top-level BVH, then one trace kernel for the whole batch).  The call
 * is SYNCHRONOUS (the scene owns the per-ray scratch), and the caller makes sure `d_rays` is complete before calling. */
NRT_API nrt_status nrtSceneTraverseBatchDevice_f32(nrt_scene *scene, const nrt_ray_f32 *d_rays, uint64_t num_rays,
                                                   nrt_scene_hit_f32 *d_hits_out, uint8_t *d_mask_out);
/* Scheduling knobs of the scene kernels by name (they never change a result): "single_pass" (1: scenes of 64 nodes or more
 * are traced by the single-pass walk — top-level tree and instance trees on one stack, no per-ray list; rays it cannot certify
 * are re-done by the listing path; 2: every scene of two nodes or more; 0: listing + trace for every ray), "trav_min", "refill_min"
 * (listing path), "walk_trav_min", "walk_refill_min" (the walk's), "cand_min",
 * "cand_busy_max" (lane-count thresholds of the phases), "prune_min" (instance count from which the listing prunes beyond a
 * full list), "walk_min" (instance count from which single_pass = 1 uses the walk; 64), "scan_max" (scenes of at most this many
 * nodes get no top-level tree: every world box is tested per ray; 8, at most 64; takes effect at the next nrtSceneCommit),
 * "fuse_scan" (1: such a scene is listed inside the trace kernel, one launch; 0: by a listing launch of its own).  After a batch of which the walk had to
 * hand more than a quarter ("walk_backoff_pct", 25) to the listing path (direction vectors far shorter than 1, where the reference's cull compares a
 * distance with a parameter) the next 15 calls use the listing path directly. */
NRT_API nrt_status nrtSceneSetTunable(nrt_scene *scene, const char *name, int value);
/* How many rays of the last nrtSceneTraverseBatch* call the single-pass walk handed to the listing path. */
NRT_API uint64_t nrtSceneLastRedone(const nrt_scene *scene);
/* Which path the last nrtSceneTraverseBatch* call took: 1 = the single-pass walk (plus the listing path for the rays it handed
 * over), 0 = the listing path alone (small scenes, single_pass = 0, a mesh whose tree the walk cannot step through, back-off).
 * After nrtSceneClosestPointBatch* (below): 2 = its one kernel, nrt::k_scene_closest_point<32>. */
NRT_API int nrtSceneLastPath(const nrt_scene *scene);

/* ---- occlusion queries on a scene: is the ray blocked at all? (shadow rays, rtcOccluded) --------------------------
 * The any-hit form of nrtSceneTraverseBatch*: a ray stops at the first instance in which it finds a hit instead of looking for
 * the nearest one, and one byte per ray is the whole result.  Contract, on a committed scene:
 *   1. Result: mask_out[i] is exactly what nrtSceneTraverseBatch_f32 / nrtSceneTraverseBatchDevice_f32 would put in
 *      hit_mask_out[i] for the same committed scene and ray: 1 = blocked, 0 = not.  The query changes how much work is done,
 *      never the answer — the reference's quirks included: only the 64 nearest entered node boxes by (entry distance, node id)
 *      count (kMaxIntersections, nanosg.h:786), so a blocker that ranks 65th or later does not occlude; the local ray carries the
 *      default [0, FLT_MAX] interval and default trace options; a local hit counts only when its world distance is < FLT_MAX
 *      (nanosg.h:848 with t_nearest initialised to max); the world ray's min_t / max_t act on the box listing only.
 *   2. Limit of exactness: 1. holds for rays on which the world distance of every local hit is finite.  Where a world distance
 *      overflows or is NaN, the first accepted primitive of an instance and its nearest one may disagree on
 *      `t_world < FLT_MAX`; such rays are outside the contract.
 *   3. Output: no hit records are produced, staged or copied; one byte per ray leaves the GPU (host form) or is written to
 *      d_mask_out (Device form), nothing else.
 *   4. Ordering: as the closest-hit scene calls — synchronous, on the scene's stream, `d_rays` complete before the call; the
 *      scene owns its scratch (not re-entrant with any other call on the same scene).
 *   5. Errors, as nrtSceneTraverseBatch*: NRT_ERR_INVALID for a NULL scene, for NULL rays or a NULL mask with num_rays > 0, for
 *      an uncommitted scene, for a scene made stale by nrtBuild / nrtSetMesh / nrtSetTree / nrtRefit* on one of its meshes (until
 *      it is committed again), and for more rays than the closest-hit call accepts (2^31 - 1); num_rays == 0 returns NRT_OK.
 *   6. Path reporting: nrtSceneLastRedone / nrtSceneLastPath describe an occlusion call as they describe a closest-hit call;
 *      "single_pass", "walk_min", "scan_max", "fuse_scan" and the phase thresholds select paths for it the same way and never
 *      change a flag.  The single-pass walk certifies a flag by a rule of its own (scene_kernels.hip, above k_scene_walk): no
 *      traced hit at all is 0; a hit in an instance with provably fewer than 64 entered boxes ranking before it is 1; any other
 *      ray is re-done by the listing path, which applies the reference's loop literally.
 *   7. Back-off: the closest-hit back-off ("walk_backoff_pct") is neither consulted nor updated by occlusion calls — its cause,
 *      the reference's cull comparing a distance with a parameter, cannot hand an occlusion ray over. */
NRT_API nrt_status nrtSceneOccludedBatch_f32(nrt_scene *scene, const nrt_ray_f32 *rays, uint64_t num_rays, uint8_t *mask_out);
NRT_API nrt_status nrtSceneOccludedBatchDevice_f32(nrt_scene *scene, const nrt_ray_f32 *d_rays, uint64_t num_rays, uint8_t *d_mask_out);

/* ---- instance visibility masks on a scene: 32 bits per node, 32 bits per ray ------------------------------------------------------
 * An OPT-IN EXTENSION, the scene-level counterpart of "visibility masks" above (the instance masks of DXR and OptiX; a camera bit,
 * a shadow bit, a reflection bit — INTEGRATION.md): one scene serves every ray type instead of one committed scene per type.
 *
 *     an instance exists for a ray  iff  (node_mask & ray_mask) != 0;
 *     a masked query answers exactly as the unmasked query would on a scene committed from the visible nodes alone, with the
 *     node ids kept.
 *
 * "Does not exist" is stronger than "is skipped when reached": of the reference's quirks, the 64 nearest entered node boxes by
 * (entry distance, node id) are counted among the VISIBLE nodes (kMaxIntersections) — a hidden instance takes no place among them.
 *
 * Setter.  nrtSceneSetNodeMasks takes one word per node in node-id order; `count` must equal the number of nodes added so far
 * (NRT_ERR_INVALID otherwise, nothing changed).  masks == NULL resets every node to 0xFFFFFFFF (count is not read).  A node
 * added later starts at 0xFFFFFFFF.  The words are NO PART OF THE TOP-LEVEL TREE: the setter works before or after nrtSceneCommit,
 * nrtSceneCommit keeps them, and a change after Commit needs no new Commit — it takes effect at the next masked query, which
 * uploads the words on the scene's stream first (scene calls are synchronous, so nothing is in flight).
 *
 * Queries.  nrtSceneTraverseBatchMasked* / nrtSceneOccludedBatchMasked* are the four scene queries above with `ray_masks`: one word
 * per ray, NULL = every ray carries 0xFFFFFFFF; a ray whose word is 0 sees nothing and gets the miss record (flag 0) of the unmasked
 * call.  Contract, on a committed scene:
 *   1. Records: every field of every record is bit-identical to what nrtSceneTraverseBatch* returns on the scene of the nodes
 *      visible to that ray (same mesh contexts, same transforms, in node order), with node_id mapped back to the node's id in
 *      THIS scene; flags likewise.
 *   2. Occlusion: the flags of nrtSceneOccludedBatchMasked* are exactly the masked closest-hit flags, within the limit of
 *      exactness of item 2 of the occlusion contract above.
 *   3. With all-ones words on either side (every node 0xFFFFFFFF, or every ray 0xFFFFFFFF / ray_masks == NULL and no node word 0)
 *      the bytes are those of the unmasked call.
 *   4. Ordering, ray limit (2^31 - 1), the stale-mesh check, nrtSceneLastPath / nrtSceneLastRedone and every tunable: as for the
 *      unmasked calls ("scan_max" and "walk_min" keep comparing the node count, not the visible count).  The masked closest-hit
 *      call consults and updates the walk back-off exactly as the unmasked one does; the masked occlusion call does neither.
 *   5. Refusals, each NRT_ERR_INVALID with nrtSceneLastError set and nothing written: those of the unmasked forms (NULL rays,
 *      NULL hits or mask, an uncommitted or stale scene, too many rays) and a `d_ray_masks` that is not 4-byte aligned.
 *      The host forms upload the words beside the rays; the Device forms read num_rays words in HBM.
 *
 * The unmasked calls ignore node masks entirely.  Triangle masks of a mesh context (nrtSetPrimMasks) remain ignored inside scenes,
 * by the masked and the unmasked scene calls alike.  Not covered: the Embree shim (its ray.mask stays ignored; rtcSetMask is not
 * offered), nrtGroup*.  (Per-ray skip ids on scenes: nrtSceneQueryBatch*, below.) */
NRT_API nrt_status nrtSceneSetNodeMasks(nrt_scene *scene, const uint32_t *masks, uint32_t count);
NRT_API nrt_status nrtSceneTraverseBatchMasked_f32(nrt_scene *scene, const nrt_ray_f32 *rays, const uint32_t *ray_masks, uint64_t num_rays,
                                                   nrt_scene_hit_f32 *hits_out, uint8_t *hit_mask_out);
NRT_API nrt_status nrtSceneTraverseBatchMaskedDevice_f32(nrt_scene *scene, const nrt_ray_f32 *d_rays, const uint32_t *d_ray_masks,
                                                         uint64_t num_rays, nrt_scene_hit_f32 *d_hits_out, uint8_t *d_mask_out);
NRT_API nrt_status nrtSceneOccludedBatchMasked_f32(nrt_scene *scene, const nrt_ray_f32 *rays, const uint32_t *ray_masks, uint64_t num_rays,
                                                   uint8_t *mask_out);
NRT_API nrt_status nrtSceneOccludedBatchMaskedDevice_f32(nrt_scene *scene, const nrt_ray_f32 *d_rays, const uint32_t *d_ray_masks,
                                                         uint64_t num_rays, uint8_t *d_mask_out);

/* ---- one descriptor for the scene queries, with per-ray skip (node, primitive) pairs ---------------------------------------------
 * An OPT-IN EXTENSION, the scene-level counterpart of nrtQueryBatch* and of per-ray skip_prim_id: a bounce or shadow ray that starts
 * ON a triangle of an instanced scene names that triangle and leaves it without an epsilon offset.  The scene calls above trace every
 * instance with the reference's literal local ray on [0, FLT_MAX] and default trace options, so without this about half of the
 * secondary rays of a path tracer over nrtScene* hit the triangle they start from (min_t acts on the box listing only).
 *
 * The descriptor names the kind in `flags` and carries what the kind reads:
 *     NRT_SCENE_QUERY_OCCLUSION  flags only (nrtSceneOccludedBatch*): mask_out is the output, hits_out is not read;
 *     NRT_SCENE_QUERY_MASKED     instance visibility masks (nrtScene*BatchMasked*): ray_masks is read (NULL: every ray 0xFFFFFFFF);
 *     NRT_SCENE_QUERY_SKIP       skip pairs: skip_pairs and skip_stride_bytes are read (skip_pairs == NULL: no ray skips anything).
 *
 * The pair.  Two uint32_t, {prim_id, node_id} IN THAT ORDER — the order of the last two fields of nrt_scene_hit_f32 — and ray i's
 * pair lies at (const char *)skip_pairs + i * skip_stride_bytes.  That layout is chosen so that a bounce wave passes the previous
 * wave's records as they lie, with no packing pass:
 *     q.skip_pairs = &hits[0].prim_id;  q.skip_stride_bytes = sizeof(nrt_scene_hit_f32);
 * A tightly packed array of pairs uses stride 8.
 *
 * Contract, on a committed scene: every field of every record is bit-identical to the same query without SKIP, with ONE change — in
 * the per-node Traverse of node n, the trace options carry skip_prim_id = p for a ray whose pair is (p, n); every other node gets
 * the default options.  The intersector returns false for that one primitive of that one instance without touching the ray's state.
 *   1. Nothing else moves: the box listing, the 64 nearest entered boxes, the early cull, the world distance and the
 *      strictly-nearer rule are those of the calls above.
 *   2. A pair skips nothing when node_id is 0xFFFFFFFF or >= the node count, or prim_id is 0xFFFFFFFF or >= the node's face count:
 *      the miss record of a previous wave is a valid "no skip".
 *   3. Instances that share a mesh context are distinct: (p, n) leaves primitive p of every other node alone.
 *   4. With MASKED, the visibility rule applies first (the scene of the visible nodes, ids kept), the skip on top of it.
 *   5. With OCCLUSION, the flags are exactly the closest-hit flags of the same descriptor, within item 2 of the occlusion contract.
 *   6. Routing: a descriptor without SKIP, or with SKIP and skip_pairs == NULL, IS the corresponding call above
 *      (nrtSceneTraverseBatch*, nrtSceneOccludedBatch*, their Masked forms): same path, same kernels, same bytes, same
 *      nrtSceneLastPath / nrtSceneLastRedone.  Path selection and every tunable act on a SKIP query as on the unskipped one; the
 *      SKIP closest-hit call consults and updates the walk back-off like the unskipped call, the SKIP occlusion call does neither.
 *   7. Refusals, each NRT_ERR_INVALID with nrtSceneLastError set and nothing written: a NULL scene or descriptor; a wrong
 *      struct_size, unknown flag bits, a non-zero `reserved`; NULL rays with num_rays > 0; the kind's output missing (hits_out
 *      without OCCLUSION, mask_out with it); an uncommitted or stale scene; more than 2^31 - 1 rays; with SKIP and a non-NULL
 *      array, a stride below 8 or not a multiple of 4; in the Device form, a skip_pairs or ray_masks pointer that is not 4-byte
 *      aligned, and a skip_pairs range that overlaps hits_out or mask_out (the walk re-reads a pair while other rays' records are
 *      being written).  num_rays == 0 on a committed scene is NRT_OK.
 * The host form stages the pairs packed to 8 bytes beside the rays; the Device form reads them where they lie, and is synchronous
 * like every scene call.  Not covered: the Embree shim, nrtGroup*. */
#define NRT_SCENE_QUERY_OCCLUSION 1u
#define NRT_SCENE_QUERY_MASKED 2u
#define NRT_SCENE_QUERY_SKIP 4u
typedef struct {
  uint32_t struct_size;        /* sizeof(nrt_scene_query_f32): lets the struct grow */
  uint32_t flags;              /* NRT_SCENE_QUERY_OCCLUSION | NRT_SCENE_QUERY_MASKED | NRT_SCENE_QUERY_SKIP */
  const nrt_ray_f32 *rays;
  uint64_t num_rays;
  const uint32_t *ray_masks;   /* read with MASKED only; NULL: every ray 0xFFFFFFFF */
  const void *skip_pairs;      /* read with SKIP only; NULL: no ray skips anything */
  uint32_t skip_stride_bytes;  /* distance between two rays' pairs; >= 8, a multiple of 4 */
  uint32_t reserved;           /* 0 */
  nrt_scene_hit_f32 *hits_out; /* not read with OCCLUSION */
  uint8_t *mask_out;           /* optional without OCCLUSION, the output with it */
} nrt_scene_query_f32;         /* 64 bytes */
NRT_API nrt_status nrtSceneQueryBatch_f32(nrt_scene *scene, const nrt_scene_query_f32 *query);
NRT_API nrt_status nrtSceneQueryBatchDevice_f32(nrt_scene *scene, const nrt_scene_query_f32 *query);

/* ---- closest-point queries on scenes ------------------------------------------------------------------------------------------------
 * Which face of which node of a committed scene is nearest to a point, and where on it: "closest-point queries" above, over the
 * instances of a scene instead of one mesh — Embree's rtcPointQuery with its instance stack.  (No reference counterpart.)  DESIGN.md §3.20.
 *
 * The rule is include/nanort_closest.h's, in fp32, every operation rounded on its own.  A face of a node IS the triangle of the three
 * XformPoint images of its local vertices — w_k = m[0][k]*v0 + m[1][k]*v1 + m[2][k]*v2 + m[3][k] summed left to right, m the node's
 * xform (nrtSceneNodeState_f32) — and ClosestPointOnTriangle of the world point against that triangle gives point (world), dist2, u
 * and v.  The answer is taken over all (node, face) pairs of the admitted nodes: the smallest dist2, then the smallest node_id, then
 * the smallest prim_id.  max_dist, non-finite points, NaN faces and equality at r2 = max_dist * max_dist are as in the single-mesh
 * query.  The record is therefore byte-identical to nrtClosestPointBatch_f32's on ONE mesh — the world vertices of all nodes
 * concatenated in node order — with that mesh's face index mapped back to (node_id, prim_id); the accuracy contract (8 eps S) holds
 * against the triangles of the rounded world vertices.  No matrix is inverted: a singular xform (a node flattened to a plane) is
 * inside the contract, finite matrices and vertices are.
 *
 * Found: point = the nearest point (world), dist2, u, v, prim_id, node_id.  Not found: point = p, dist2 = r2, u = v = 0,
 * prim_id = node_id = 0xFFFFFFFF.  found_out (may be NULL) receives 1 / 0 per point.
 *
 * Masks.  point_masks == NULL: every node is admitted, whatever its word.  Otherwise one word per point, and a node is admitted for
 * a point iff (node word & point word) != 0 — the words of nrtSceneSetNodeMasks, as "instance visibility masks" above defines them
 * for rays: 0xFFFFFFFF until set, no part of the top-level tree, no Commit needed on a change.
 *
 * Runs nrt::k_scene_closest_point<32>, one launch per call (per piece in the host form): the top-level tree where nrtSceneCommit
 * built one and a scan of the nodes' world boxes where it did not ("scan_max"), and the nodes' own trees, on one stack per point;
 * nrtSceneLastPath reports 2.  Mesh trees adopted with nrtSetTree are inside the contract when every box contains the triangles
 * below it.  The trace options of a mesh context, its triangle masks and its motion keyframe 1 are not read.
 *
 * Refusals; each NRT_ERR_INVALID, writes nothing and sets nrtSceneLastError: a NULL scene; a scene that is not committed; a mesh
 * context rebuilt, re-set or refitted since nrtSceneCommit; NULL points or closest_out with num_points > 0; more than 2^31-1
 * points; in the Device form, points or closest_out not aligned to 16 bytes or point_masks not to 4.  num_points == 0 on a committed
 * scene is NRT_OK.
 *
 * nrtSceneClosestPointBatch_f32 takes host arrays, staged through the scene's grow-only buffers in pieces of 2^20 points.
 * nrtSceneClosestPointBatchDevice_f32 takes device arrays; like every scene call it runs on the scene's own stream and is
 * SYNCHRONOUS, and the caller makes sure the inputs are complete before calling.
 *
 * Not covered: signed distance and the K nearest faces on scenes, per-point skip pairs, fp64. */
typedef struct { float point[3]; float dist2; float u, v; uint32_t prim_id; uint32_t node_id; } nrt_scene_closest_f32;
#ifdef __cplusplus
static_assert(sizeof(nrt_scene_closest_f32) == 32, "scene closest-point record layout");
#endif
NRT_API nrt_status nrtSceneClosestPointBatch_f32(nrt_scene *scene, const nrt_point_f32 *points, uint64_t num_points, const uint32_t *point_masks,
                                                 nrt_scene_closest_f32 *closest_out, uint8_t *found_out);
NRT_API nrt_status nrtSceneClosestPointBatchDevice_f32(nrt_scene *scene, const nrt_point_f32 *d_points, uint64_t num_points,
                                                       const uint32_t *d_point_masks, nrt_scene_closest_f32 *d_closest_out, uint8_t *d_found_out);

#ifdef __cplusplus
}
#endif
#endif /* NANORT_HIP_H_ */
