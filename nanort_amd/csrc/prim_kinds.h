// nanort_amd/csrc/prim_kinds.h — the primitive kinds of the library as data: what a kind's arrays hold per primitive, which
// precisions and counts its setter accepts, and whether a traversal launch is followed by a post pass.  Also the one host rule
// a kind brings along: into how many segments a cylinder is cut for the builder.  Plain C++ without a HIP include, like
// launch_plan.h and walk_variant.h, so that tests/cpp/prim_kinds_check.cc runs on a machine without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

namespace nrt {

enum : int { kPrimTriangles = 0, kPrimSpheres = 1, kPrimCylinders = 2, kPrimCurves = 3 };
constexpr int kNumPrimKinds = 4;

struct PrimKind {
  const char *name;  // as the error texts spell it
  int pos_floats;    // position scalars per primitive in d_verts (triangles: per VERTEX, the faces name the vertices)
  int radius_floats; // radius scalars per primitive in d_radii
  int num_verts;     // positions per primitive (triangles: 0, the mesh says how many vertices it has)
  bool fp64;         // the kind exists in double precision
  uint32_t max_count; // counts at or above are refused (0: every uint32_t count is taken)
  bool post_pass;    // a kernel behind the walk finishes the records (spheres: only where records were asked for)
  int hit_bytes;     // the caller's record where that pass writes one of its own (0: nrt_hit_f32 / _f64, finished in place)
};
constexpr PrimKind kPrimKinds[kNumPrimKinds] = {
    {"triangles", 3, 0, 0, true, 0u, false, 0},
    {"spheres", 3, 1, 1, true, 0u, true, 0},             // centre, radius; u / v from the unit normal
    {"cylinders", 6, 2, 2, false, 0x40000000u, true, 28}, // two end points, two radii; nrt_cyl_hit_f32
    {"curves", 12, 4, 4, false, 1u << 28, true, 40},      // four control points, four radii; nrt_curve_hit_f32
};

// Segments of one cylinder for the builder (prims.hip, k_cylinder_segments): one per `seg_radii` tube radii of its length, `kmax`
// at the most.  Zero-radius "cylinders" are boxes (the top-level tree of a scene) and stay whole, as does whatever is not finite.
inline uint32_t cylinder_segment_count(const float *p0, const float *p1, float r0, float r1, int seg_radii, uint32_t kmax) {
  const float rr = r0 > r1 ? r0 : r1;
  const double dx = (double)p1[0] - p0[0], dy = (double)p1[1] - p0[1], dz = (double)p1[2] - p0[2];
  const double len = sqrt(dx * dx + dy * dy + dz * dz);
  if (!(kmax > 1 && rr > 0.0f && std::isfinite(len) && std::isfinite(rr) && len > 0.0)) return 1u;
  const double want = ceil(len / ((double)seg_radii * (double)rr));
  return want >= (double)kmax ? kmax : (want < 1.0 ? 1u : (uint32_t)want);
}

// First segment of every cylinder into off[0 .. n] (off[n]: all of them) and their number.  A total that reaches `limit` (the
// segment array would not fit the packed leaf references) is tried once more with half as many pieces at the most; 0 if that
// does not fit either.
inline uint64_t cylinder_segment_offsets(const float *endpoints, const float *radii, uint32_t n, int seg_radii, uint32_t split,
                                         uint64_t limit, uint32_t *off) {
  for (int pass = 0; pass < 2; pass++) {
    const uint32_t kmax = split >> pass;
    uint64_t t = 0;
    for (uint32_t i = 0; i < n; i++) {
      const float *p0 = endpoints + 6 * (size_t)i;
      off[i] = (uint32_t)t;
      t += cylinder_segment_count(p0, p0 + 3, radii[2 * (size_t)i], radii[2 * (size_t)i + 1], seg_radii, kmax);
    }
    off[n] = (uint32_t)t;
    if (t < limit) return t;
  }
  return 0;
}

} // namespace nrt
