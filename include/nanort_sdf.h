// include/nanort_sdf.h — THE one statement of the signed-distance rule (include/nanort_hip.h, "signed distance
// queries"): on which side of a mesh a point lies, from the closest-point answer of include/nanort_closest.h and the angle-weighted
// pseudonormal of the feature that holds the nearest point (Baerentzen and Aanaes, "Signed distance computation using the angle
// weighted pseudonormal", 2005).  As in nanort_closest.h every operation is rounded on its own (no contraction) and dots are summed
// left to right.
//
//   ClosestFeatureOnTriangle(p, a, b, c, &u, &v, q, &feature) -> dist2
//       ClosestPointOnTriangle's candidates in its order — (u, v), q and dist2 are its, bit for bit — and the code of the candidate
//       that won: 0 the face candidate, 1 / 2 / 3 the edge ab / ac / bc, 4 / 5 / 6 the vertex a / b / c.  An edge candidate whose
//       clamped t is exactly 0 or 1 is a vertex: ab -> a, b; ac -> a, c; bc -> b, c.  The code is the WINNING candidate's: it cannot be
//       recovered from (u, v) afterwards (the face candidate may land on an edge, and two candidates may name the same point).
//   UnitNormal(a, b, c, n)    (b - a) x (c - a) divided by its length; the zero vector where the length is 0 or not finite.  Outside
//                             is the side from which a, b, c run counter-clockwise.
//   CornerAngle(e1, e2)       atan2(|e1 x e2|, e1 . e2): the angle at a corner between its two edges.
//   Inside(p, q, n)           Dot(p - q, n) < 0.  A zero or NaN product, a point on the surface and a zero normal are all "not inside".
//
// The normals of a mesh (FeatureNormals, BuildFeatureNormals below):
//   per face, four normals [4][3]: the unit normal, then for each of the edges ab, ac, bc the sum of the unit normals of ALL faces
//       that hold both of the edge's vertex indices — in ascending face id, each face once, starting from zero (a boundary
//       edge has one term, a non-manifold edge several);
//   per vertex [3]: the sum over its incident corners of angle * unit normal, in ascending corner id 3 * face + k, starting from
//       zero (0 + angle * n first); an unreferenced vertex gets zero.
// The normal of feature f of face `prim`: f = 0..3 -> face_normals[prim][f]; f = 4..6 -> vertex_normals[faces[3 * prim + f - 4]].
//
// Vertices are identified by INDEX, not by position: two vertices at the same place are two vertices, and a mesh whose faces share
// no indices (an unwelded "soup") has only boundary edges — every edge and vertex normal is then its own face's, and the sign
// across a sharp edge is the face normal's.  Weld such a mesh first.  On a closed, consistently oriented mesh without zero-area
// faces the sign is provably the side (the paper's theorem); elsewhere it is what the rule gives: reproducible, not guaranteed to
// mean anything.
//
// Included by the device kernels (nanort_amd/csrc/sdf.hip, closest.hip), by the host classes of nanort.h and by the tests' CPU model.
#ifndef NANORT_SDF_H_
#define NANORT_SDF_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "nanort_closest.h"

namespace nanort_sdf {

using namespace nanort_closest::feature_codes;
enum : unsigned int { kFeatureMask = 7u, kInsideBit = 0x80000000u };  // the `feature` word of a signed record

using nanort_closest::ClosestFeatureOnTriangle;  // (stated in nanort_closest.h, where ClosestPointOnTriangle is a call of it)

// x cross y, each component one rounded difference of two rounded products.
template <typename T>
NANORT_CLOSEST_FN void Cross(const T x[3], const T y[3], T out[3]) {
  out[0] = x[1] * y[2] - x[2] * y[1];
  out[1] = x[2] * y[0] - x[0] * y[2];
  out[2] = x[0] * y[1] - x[1] * y[0];
}

NANORT_CLOSEST_FN float Sqrt(float x) { return sqrtf(x); }
NANORT_CLOSEST_FN double Sqrt(double x) { return sqrt(x); }
NANORT_CLOSEST_FN float Atan2(float y, float x) { return atan2f(y, x); }
NANORT_CLOSEST_FN double Atan2(double y, double x) { return atan2(y, x); }

template <typename T>
NANORT_CLOSEST_FN void UnitNormal(const T a[3], const T b[3], const T c[3], T n[3]) {
  const T ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  T x[3];
  Cross(ab, ac, x);
  const T len = Sqrt(nanort_closest::Dot(x[0], x[1], x[2], x[0], x[1], x[2]));
  const bool ok = len > T(0) && len - len == T(0);  // (false for 0, NaN and inf)
  n[0] = ok ? x[0] / len : T(0);
  n[1] = ok ? x[1] / len : T(0);
  n[2] = ok ? x[2] / len : T(0);
}

// The angle between the edges e1 and e2 that leave a corner.
template <typename T>
NANORT_CLOSEST_FN T CornerAngle(const T e1[3], const T e2[3]) {
  T x[3];
  Cross(e1, e2, x);
  return Atan2(Sqrt(nanort_closest::Dot(x[0], x[1], x[2], x[0], x[1], x[2])), nanort_closest::Dot(e1[0], e1[1], e1[2], e2[0], e2[1], e2[2]));
}

// The three corner angles of a face, at a, b and c.
template <typename T>
NANORT_CLOSEST_FN void CornerAngles(const T a[3], const T b[3], const T c[3], T angles[3]) {
  const T ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const T ba[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]}, bc[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]};
  const T ca[3] = {a[0] - c[0], a[1] - c[1], a[2] - c[2]}, cb[3] = {b[0] - c[0], b[1] - c[1], b[2] - c[2]};
  angles[0] = CornerAngle(ab, ac);
  angles[1] = CornerAngle(bc, ba);
  angles[2] = CornerAngle(ca, cb);
}

template <typename T>
NANORT_CLOSEST_FN bool Inside(const T p[3], const T q[3], const T n[3]) {
  return nanort_closest::Dot(p[0] - q[0], p[1] - q[1], p[2] - q[2], n[0], n[1], n[2]) < T(0);
}

// The `feature` word of a signed record: the code, and bit 31 exactly when the point is inside.
template <typename T>
NANORT_CLOSEST_FN unsigned int FeatureWord(const T p[3], const T q[3], const T n[3], unsigned int feature) {
  return feature | (Inside(p, q, n) ? (unsigned int)kInsideBit : 0u);
}

// The vertex indices (slots 0..2 of the face) of edge e = 1 / 2 / 3: ab, ac, bc.
NANORT_CLOSEST_FN void EdgeSlots(unsigned int e, unsigned int *s0, unsigned int *s1) {
  *s0 = e == 3u ? 1u : 0u;
  *s1 = e == 1u ? 1u : 2u;
}

}  // namespace nanort_sdf

#include <vector>

namespace nanort_sdf {

// The normals of a mesh on the host, by the rule at the head of the file.  face_normals: [num_faces][4][3], vertex_normals:
// [num_verts][3].  Faces naming a vertex >= num_verts are the caller's fault (not checked).
template <typename T>
inline void BuildFeatureNormals(const T *verts, const unsigned int *faces, size_t num_faces, size_t num_verts, T *face_normals, T *vertex_normals) {
  std::vector<T> angles(3 * num_faces);
  for (size_t f = 0; f < num_faces; f++) {
    const T *a = verts + 3 * (size_t)faces[3 * f + 0], *b = verts + 3 * (size_t)faces[3 * f + 1], *c = verts + 3 * (size_t)faces[3 * f + 2];
    UnitNormal(a, b, c, face_normals + 12 * f);
    CornerAngles(a, b, c, &angles[3 * f]);
  }
  // the corners of every vertex in ascending corner id (a counting sort by vertex index: stable)
  std::vector<size_t> start(num_verts + 1, 0);
  for (size_t k = 0; k < 3 * num_faces; k++) start[(size_t)faces[k] + 1]++;
  for (size_t v = 0; v < num_verts; v++) start[v + 1] += start[v];
  std::vector<size_t> corner(3 * num_faces), fill(start.begin(), start.end() - 1);
  for (size_t k = 0; k < 3 * num_faces; k++) corner[fill[faces[k]]++] = k;
  for (size_t v = 0; v < num_verts; v++) {
    T acc[3] = {T(0), T(0), T(0)};
    for (size_t i = start[v]; i < start[v + 1]; i++) {
      const size_t f = corner[i] / 3;
      const T w = angles[corner[i]];
      for (int k = 0; k < 3; k++) acc[k] = acc[k] + w * face_normals[12 * f + k];
    }
    for (int k = 0; k < 3; k++) vertex_normals[3 * v + k] = acc[k];
  }
  for (size_t f = 0; f < num_faces; f++)
    for (unsigned int e = 1; e <= 3; e++) {
      unsigned int s0, s1;
      EdgeSlots(e, &s0, &s1);
      const unsigned int i = faces[3 * f + s0], j = faces[3 * f + s1];
      T acc[3] = {T(0), T(0), T(0)};
      size_t last = (size_t)-1;
      for (size_t r = start[i]; r < start[(size_t)i + 1]; r++) {
        const size_t g = corner[r] / 3;
        if (g == last) continue;  // (a face that names i twice: once)
        last = g;
        if (faces[3 * g] != j && faces[3 * g + 1] != j && faces[3 * g + 2] != j) continue;
        for (int k = 0; k < 3; k++) acc[k] = acc[k] + face_normals[12 * g + k];
      }
      for (int k = 0; k < 3; k++) face_normals[12 * f + 3 * e + k] = acc[k];
    }
}

}  // namespace nanort_sdf

#endif  // NANORT_SDF_H_
