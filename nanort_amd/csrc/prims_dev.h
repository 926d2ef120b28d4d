// nanort_amd/csrc/prims_dev.h — the per-kind device rule of the builder (build.hip, k_prim_records), kept with the kinds' other
// rules (prim_kinds.h, prims.hip) and out of the builder's file.
#pragma once
#include "common.h"
#include "minmax_dev.h"

namespace nrt {

// Box and centre of primitive `i` on axis `k`, as the reference's BoundingBoxAndCenter of each kind computes them.  Triangles:
// p0, p1, p2 are the three vertices' components on that axis (the builder loads a vertex in one piece); the other kinds read
// `verts` and `radii`.
template <typename T>
__device__ __forceinline__ void prim_box_axis(bool tri, int kind, uint32_t i, int k, const T *__restrict__ verts, const T *__restrict__ radii, T p0, T p1, T p2,
                                              T &bmin, T &bmax, T &centre) {
  if (tri) {
    bmin = tmin(p0, tmin(p1, p2)); // nanort.h:967-968
    bmax = tmax(p0, tmax(p1, p2));
    centre = ((p0 + p1) + p2) * (T(1) / T(3)); // nanort.h:970
  } else if (kind == kPrimSpheres) { // SphereGeometry::BoundingBoxAndCenter (examples/particle_primitive/main.cc:124-136)
    const T c = verts[3 * (size_t)i + k], rad = radii[i];
    bmin = c - rad;
    bmax = c + rad;
    centre = c;
  } else if (kind == kPrimCylinders) { // CylinderGeometry::BoundingBoxAndCenter (examples/cylinder_primitive/main.cc:166-205)
    const T a0 = verts[3 * (size_t)(2 * i) + k], a1 = verts[3 * (size_t)(2 * i + 1) + k];
    const T r0 = radii[2 * (size_t)i], r1 = radii[2 * (size_t)i + 1];
    bmin = tmin(a1 - r1, a0 - r0); // std::min(second, first): identical unless NaN
    bmax = tmax(a1 + r1, a0 + r0);
    centre = (a0 + a1) / T(2.0);
  } else { // CurveGeometry::BoundingBoxAndCenter (examples/curves_primitive/main.cc:557-597): control point -+ its radius
    const T *cp = verts + 12 * (size_t)i + k, *rad = radii + 4 * (size_t)i;
    T lo = cp[0] - rad[0], hi = cp[0] + rad[0];
#pragma unroll
    for (int j = 1; j < 4; j++) {
      lo = tmin(cp[3 * j] - rad[j], lo); // std::min(new, running) / std::max(new, running), operands in the example's order
      hi = tmax(cp[3 * j] + rad[j], hi);
    }
    bmin = lo;
    bmax = hi;
    centre = (((cp[0] + cp[3]) + cp[6]) + cp[9]) / T(4.0);
  }
}

} // namespace nrt
