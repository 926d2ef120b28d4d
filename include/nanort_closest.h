// include/nanort_closest.h — THE one statement of the closest-point rule (include/nanort_hip.h, "closest-point
// queries").
//
// Which triangle of a mesh is nearest to a point, and where on it.  Every operation is rounded on its own (no contraction: the
// library and every program that wants its bits compile with -ffp-contract=off), dots and sums of squares are summed left to right,
// x*x' + y*y' + z*z'.
//
//   ClosestUV(p, a, b, c) -> (u, v)      Ericson's region test (Real-Time Collision Detection 5.1.5), in the book's order.  u is the
//                                        weight of the triangle's second vertex and v of its third — the convention of the ray hit
//                                        records (nanort.h, TriangleIntersector: u_ = V * rcpDet weighs p1, v_ = W * rcpDet p2).
//   ClosestOnTriangle(p, a, b, c, u, v)  q_k = w0*a_k + u*b_k + v*c_k with w0 = (1 - u) - v, clamped per component to
//                                        [min(a_k, b_k, c_k), max(a_k, b_k, c_k)]; dist2 = (p0-q0)^2 + (p1-q1)^2 + (p2-q2)^2.  The
//                                        weighted form returns a vertex exactly in the vertex regions, and the clamp (what
//                                        nanort_motion::Lerp does for the same reason) puts q inside every box that contains the
//                                        triangle.
//   BoxDist2(p, bmin, bmax)              m_k = max(bmin_k - p_k, p_k - bmax_k, 0), the squares summed in the same order.
//
// Because q_k lies in the box and each of subtraction, square and sum is monotone under rounding, BoxDist2 <= dist2 holds IN
// FLOATING POINT for every box that contains the triangle's vertices: a subtree whose box lies farther than the best distance found
// holds no nearer face, exactly.
//
// The answer of a query (p, max_dist) over a set of admitted faces: the face with the smallest dist2, among equal dist2 the smallest
// prim_id (Better).  A face counts only if dist2 <= r2 = max_dist * max_dist (equality counts, +inf is allowed); a NaN or negative
// max_dist finds nothing; a face whose dist2 is NaN is never the answer; a point with a non-finite coordinate finds nothing
// (Searchable).  A minimum with a total tie-break: it does not depend on the tree.  A subtree is skipped iff BoxDist2 > best,
// strictly, where best starts at r2 (Culled): a box at exactly best is entered, because the tie-break may prefer a face inside it.
//
// Included by the device kernel (nanort_amd/csrc/closest.hip), by the host classes of nanort.h and by the CPU model of the tests.
#ifndef NANORT_CLOSEST_H_
#define NANORT_CLOSEST_H_

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NANORT_CLOSEST_FN __host__ __device__ inline
#else
#define NANORT_CLOSEST_FN inline
#endif

namespace nanort_closest {

template <typename T>
NANORT_CLOSEST_FN T Dot(T x0, T x1, T x2, T y0, T y1, T y2) {
  return x0 * y0 + x1 * y1 + x2 * y2;
}

template <typename T>
NANORT_CLOSEST_FN void ClosestUV(const T p[3], const T a[3], const T b[3], const T c[3], T *u, T *v) {
  const T ab0 = b[0] - a[0], ab1 = b[1] - a[1], ab2 = b[2] - a[2];
  const T ac0 = c[0] - a[0], ac1 = c[1] - a[1], ac2 = c[2] - a[2];
  const T ap0 = p[0] - a[0], ap1 = p[1] - a[1], ap2 = p[2] - a[2];
  const T d1 = Dot(ab0, ab1, ab2, ap0, ap1, ap2), d2 = Dot(ac0, ac1, ac2, ap0, ap1, ap2);
  if (d1 <= T(0) && d2 <= T(0)) { // vertex a
    *u = T(0), *v = T(0);
    return;
  }
  const T bp0 = p[0] - b[0], bp1 = p[1] - b[1], bp2 = p[2] - b[2];
  const T d3 = Dot(ab0, ab1, ab2, bp0, bp1, bp2), d4 = Dot(ac0, ac1, ac2, bp0, bp1, bp2);
  if (d3 >= T(0) && d4 <= d3) { // vertex b
    *u = T(1), *v = T(0);
    return;
  }
  const T vc = d1 * d4 - d3 * d2;
  if (vc <= T(0) && d1 >= T(0) && d3 <= T(0)) { // edge ab
    *u = d1 / (d1 - d3), *v = T(0);
    return;
  }
  const T cp0 = p[0] - c[0], cp1 = p[1] - c[1], cp2 = p[2] - c[2];
  const T d5 = Dot(ab0, ab1, ab2, cp0, cp1, cp2), d6 = Dot(ac0, ac1, ac2, cp0, cp1, cp2);
  if (d6 >= T(0) && d5 <= d6) { // vertex c
    *u = T(0), *v = T(1);
    return;
  }
  const T vb = d5 * d2 - d1 * d6;
  if (vb <= T(0) && d2 >= T(0) && d6 <= T(0)) { // edge ac
    *u = T(0), *v = d2 / (d2 - d6);
    return;
  }
  const T va = d3 * d6 - d5 * d4;
  if (va <= T(0) && d4 - d3 >= T(0) && d5 - d6 >= T(0)) { // edge bc
    const T w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    *u = T(1) - w, *v = w;
    return;
  }
  const T den = T(1) / (va + vb + vc); // the face
  *u = vb * den, *v = vc * den;
}

// One component of the point (u, v) names, inside [min(a, b, c), max(a, b, c)].
template <typename T>
NANORT_CLOSEST_FN T ClampedWeighted(T a, T b, T c, T w0, T u, T v) {
  T lo = (b < a) ? b : a, hi = (a < b) ? b : a;
  lo = (c < lo) ? c : lo;
  hi = (hi < c) ? c : hi;
  const T x = w0 * a + u * b + v * c;
  return x < lo ? lo : (x > hi ? hi : x);
}

// The point of the triangle that (u, v) of ClosestUV name, into q; returns its squared distance to p.
template <typename T>
NANORT_CLOSEST_FN T ClosestOnTriangle(const T p[3], const T a[3], const T b[3], const T c[3], T u, T v, T q[3]) {
  const T w0 = (T(1) - u) - v;
  q[0] = ClampedWeighted(a[0], b[0], c[0], w0, u, v);
  q[1] = ClampedWeighted(a[1], b[1], c[1], w0, u, v);
  q[2] = ClampedWeighted(a[2], b[2], c[2], w0, u, v);
  const T e0 = p[0] - q[0], e1 = p[1] - q[1], e2 = p[2] - q[2];
  return e0 * e0 + e1 * e1 + e2 * e2;
}

// One component of the box distance: max(bmin - p, p - bmax, 0).  (A NaN bound drops out: such a box is never culled.)
template <typename T>
NANORT_CLOSEST_FN T BoxGap(T p, T bmin, T bmax) {
  const T lo = bmin - p, hi = p - bmax;
  T m = T(0);
  m = (lo > m) ? lo : m;
  m = (hi > m) ? hi : m;
  return m;
}
template <typename T>
NANORT_CLOSEST_FN T BoxDist2(const T p[3], const T bmin[3], const T bmax[3]) {
  const T m0 = BoxGap(p[0], bmin[0], bmax[0]), m1 = BoxGap(p[1], bmin[1], bmax[1]), m2 = BoxGap(p[2], bmin[2], bmax[2]);
  return m0 * m0 + m1 * m1 + m2 * m2;
}

// Does the query look at anything?  Every coordinate finite (x - x == 0 for exactly those) and max_dist >= 0 (false for NaN).
template <typename T>
NANORT_CLOSEST_FN bool Searchable(const T p[3], T max_dist) {
  return (p[0] - p[0] == T(0)) && (p[1] - p[1] == T(0)) && (p[2] - p[2] == T(0)) && (max_dist >= T(0));
}

// Is the face (dist2, prim_id) a better answer than the best so far?  `best` starts at r2 with best_prim = 0xFFFFFFFF, which no face
// carries: dist2 == r2 counts, a NaN dist2 never does.
template <typename T>
NANORT_CLOSEST_FN bool Better(T dist2, unsigned int prim_id, T best, unsigned int best_prim) {
  return dist2 < best || (dist2 == best && prim_id < best_prim);
}

// Is a subtree whose box lies at `box_dist2` skipped?  Strictly farther only.
template <typename T>
NANORT_CLOSEST_FN bool Culled(T box_dist2, T best) {
  return box_dist2 > best;
}

}  // namespace nanort_closest

#endif  // NANORT_CLOSEST_H_
