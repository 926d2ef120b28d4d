// nanort_amd/csrc/walk_variant.h — which instantiation of k_traverse_wide (traverse.hip) a launch runs, as a pure function of
// what the launch asks for, and the one list of the instantiations that exist.  Plain C++ without a HIP include, like
// launch_plan.h, so that tests/cpp/walk_variant_check.cc can sweep the whole input space on a machine without a GPU: hit
// records are identical under every variant, so no parity test notices a wrong pick.
#pragma once
#include "prim_kinds.h" // kPrim*

namespace nrt {

#ifndef NRT_W4_LDS_STACK
#define NRT_W4_LDS_STACK 12
#endif
constexpr int kWide4LdsStack = NRT_W4_LDS_STACK; // per-lane LDS stack entries of the WIDTH = 4 variants (24 KiB per block: six blocks per CU)

// The template arguments of k_traverse_wide<T, STACK, STATS, KIND, PLAIN, CLOCK, WIDTH, ORDER> as data.
struct WalkVariant {
  bool f32;  // T: float or double
  int stack; // per-lane stack entries kept in LDS
  bool stats;
  int kind;   // kPrim*
  bool plain; // without the primitive id / cull tests
  bool clock;
  int width; // tree levels per record: 2 = one, 4 = two
  int order; // (WIDTH = 4) bit 0: slots by entry distance, bit 1: leaf items, bit 2: 64-bit record offsets
};
inline bool operator==(const WalkVariant &a, const WalkVariant &b) {
  return a.f32 == b.f32 && a.stack == b.stack && a.stats == b.stats && a.kind == b.kind && a.plain == b.plain && a.clock == b.clock &&
         a.width == b.width && a.order == b.order;
}

static_assert(kPrimTriangles == 0 && kPrimSpheres == 1 && kPrimCylinders == 2 && kPrimCurves == 3, "the rows below spell KIND as its number");
// Every instantiation there is: X(T, STACK, STATS, KIND, PLAIN, CLOCK, WIDTH, ORDER), KIND spelled as its number (the row is also
// the kernel's printed name).  traverse.hip builds its kernel table from these rows and walk_variant_exists() its membership
// test, so a variant that is picked but not listed fails tests/test_walk_variant.py, not a launch.
#define NRT_WALK_VARIANTS(X)                                                                                        \
  X(float, NRT_W4_LDS_STACK, false, 1, false, false, 4, 0) /* spheres, cylinders, curves: the id tests stay */     \
  X(float, 10, false, 1, false, false, 2, 0)                                                                        \
  X(float, NRT_W4_LDS_STACK, false, 2, false, false, 4, 0)                                                          \
  X(float, 10, false, 2, false, false, 2, 0)                                                                        \
  X(float, NRT_W4_LDS_STACK, false, 3, false, false, 4, 0) /* (curves are fp32 only, as their example) */           \
  X(float, 10, false, 3, false, false, 2, 0)                                                                        \
  X(float, NRT_W4_LDS_STACK, false, 0, true, false, 4, 6) /* triangles, two levels per step: PLAIN x ORDER */      \
  X(float, NRT_W4_LDS_STACK, false, 0, false, false, 4, 6)                                                          \
  X(float, NRT_W4_LDS_STACK, false, 0, true, false, 4, 4)                                                           \
  X(float, NRT_W4_LDS_STACK, false, 0, false, false, 4, 4)                                                          \
  X(float, NRT_W4_LDS_STACK, false, 0, true, false, 4, 2)                                                           \
  X(float, NRT_W4_LDS_STACK, false, 0, false, false, 4, 2)                                                          \
  X(float, NRT_W4_LDS_STACK, false, 0, true, false, 4, 3)                                                           \
  X(float, NRT_W4_LDS_STACK, false, 0, false, false, 4, 3)                                                          \
  X(float, NRT_W4_LDS_STACK, false, 0, true, false, 4, 1)                                                           \
  X(float, NRT_W4_LDS_STACK, false, 0, false, false, 4, 1)                                                          \
  X(float, NRT_W4_LDS_STACK, false, 0, true, false, 4, 0)                                                           \
  X(float, NRT_W4_LDS_STACK, false, 0, false, false, 4, 0)                                                          \
  X(float, 8, false, 0, false, false, 2, 0) /* triangles, one level per step: PLAIN at the default depth only */   \
  X(float, 10, false, 0, true, false, 2, 0)                                                                         \
  X(float, 10, false, 0, false, false, 2, 0)                                                                        \
  X(float, 12, false, 0, false, false, 2, 0)                                                                        \
  X(float, 16, false, 0, false, false, 2, 0)                                                                        \
  X(double, 10, false, 1, false, false, 2, 0) /* fp64: one level per step */                                        \
  X(double, 10, false, 2, false, false, 2, 0)                                                                       \
  X(double, 8, false, 0, false, false, 2, 0)                                                                        \
  X(double, 10, false, 0, true, false, 2, 0)                                                                        \
  X(double, 10, false, 0, false, false, 2, 0)                                                                       \
  X(double, 12, false, 0, false, false, 2, 0)                                                                       \
  X(double, 16, false, 0, false, false, 2, 0)
// ... and the counting (STATS) and time-stamping (CLOCK) ones that only the profiling library carries
#define NRT_WALK_VARIANTS_PROF(X)                            \
  X(float, NRT_W4_LDS_STACK, true, 0, true, false, 4, 0)     \
  X(float, NRT_W4_LDS_STACK, false, 0, true, true, 4, 0)     \
  X(float, 10, true, 0, false, false, 2, 0)                  \
  X(float, 10, false, 0, true, true, 2, 0)                   \
  X(double, 10, true, 0, false, false, 2, 0)                 \
  X(double, 10, false, 0, true, true, 2, 0)

inline bool walk_variant_exists(const WalkVariant &v, bool prof_build) {
#define NRT_WALK_VARIANT_IS(T_, ...) \
  if (v == WalkVariant{sizeof(T_) == 4, __VA_ARGS__}) return true;
  NRT_WALK_VARIANTS(NRT_WALK_VARIANT_IS)
  if (prof_build) {
    NRT_WALK_VARIANTS_PROF(NRT_WALK_VARIANT_IS)
  }
#undef NRT_WALK_VARIANT_IS
  return false;
}

// What a launch asks of the walk: the fields of TraverseArgs that select the kernel, and the context's primitive kind.
struct WalkRequest {
  bool f32;
  int kind;        // kPrim*
  int lds_entries; // one level per step over triangles: 8, 10, 12, anything else -> 16; every other walk has one depth
  bool wide4;      // two levels per step (fp32 only: fp64 trees have no Wide4Node array)
  bool wide4_big, leaf_items, order4, plain_options;
  bool stats, clock; // profiling requests (debug flag 32, a wave_clock array): the profiling build's default-depth triangle walks only
};

inline WalkVariant pick_wide_variant(const WalkRequest &r, bool prof_build) {
  const bool two = r.wide4 && r.f32;
  if (r.kind != kPrimTriangles) // 10 LDS entries walking one level per step (the caller sizes the overflow stack)
    return {r.f32, two ? kWide4LdsStack : 10, false, r.kind, false, false, two ? 4 : 2, 0};
  const bool stats = prof_build && r.stats, clock = prof_build && r.clock && !stats;
  if (two) {
    if (stats || clock) return {true, kWide4LdsStack, stats, kPrimTriangles, true, clock, 4, 0}; // (default trace options only)
    // a record array of 4 GiB or more: the default walk with 64-bit record offsets (api_query.hip sends nothing else here); else
    // bit 1: leaf phase over items (tunable leaf_compact), bit 0: slots entered by entry distance (tunable order4)
    const int order = r.wide4_big ? (r.leaf_items ? 6 : 4) : ((r.leaf_items ? 2 : 0) | (r.order4 ? 1 : 0));
    return {true, kWide4LdsStack, false, kPrimTriangles, r.plain_options, false, 4, order};
  }
  if (r.lds_entries == 10) {
    if (stats) return {r.f32, 10, true, kPrimTriangles, false, false, 2, 0};
    return {r.f32, 10, false, kPrimTriangles, clock || r.plain_options, clock, 2, 0};
  }
  const int stack = (r.lds_entries == 8 || r.lds_entries == 12) ? r.lds_entries : 16;
  return {r.f32, stack, false, kPrimTriangles, false, false, 2, 0};
}

// The instantiation whose occupancy sizes the persistent grid of such a launch.  A REPRESENTATIVE of the launch's family (its
// precision, kind, width and depth), not the variant picked above: two-level triangle walks are all sized by the PLAIN one in
// the reference's order, one-level walks of depth 10 by the PLAIN one.  The grid sizes, and with them the measured speeds,
// rest on exactly these, so it does not follow the pick.
inline WalkVariant occupancy_variant(bool f32, int kind, int lds_entries, bool wide4) {
  WalkRequest r = {f32, kind, lds_entries, wide4, false, false, false, true, false, false};
  return pick_wide_variant(r, false);
}

} // namespace nrt
