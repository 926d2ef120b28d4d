// include/nanort_closest.h — THE one statement of the closest-point rule (include/nanort_hip.h, "closest-point
// queries").
//
// Which triangle of a mesh is nearest to a point, and where on it.  Every operation is rounded on its own (no contraction: the
// library and every program that wants its bits compile with -ffp-contract=off), dots and sums of squares are summed left to right,
// x*x' + y*y' + z*z'.
//
//   ClosestOnTriangle(p, a, b, c, u, v)  q_k = w0*a_k + u*b_k + v*c_k with w0 = (1 - u) - v, clamped per component to
//                                        [min(a_k, b_k, c_k), max(a_k, b_k, c_k)]; dist2 = (p0-q0)^2 + (p1-q1)^2 + (p2-q2)^2.  u is the
//                                        weight of the triangle's second vertex and v of its third — the convention of the ray hit
//                                        records (nanort.h, TriangleIntersector: u_ = V * rcpDet weighs p1, v_ = W * rcpDet p2).
//                                        The weighted form returns a vertex exactly where (u, v) is (0, 0), (1, 0) or (0, 1), and
//                                        the clamp (what nanort_motion::Lerp does for the same reason) puts q inside every box
//                                        that contains the triangle.
//   ClosestPointOnTriangle(p, a, b, c)   -> (u, v), q, dist2: the nearest of up to four candidates, each valued by ClosestOnTriangle,
//                                        in this order, a later one taken only when strictly nearer (or when all before it are NaN):
//                                          edge ab  (t, 0),      t = clamp(((p-a).(b-a)) / ((b-a).(b-a)), 0, 1)
//                                          edge ac  (0, t),      t = clamp(((p-a).(c-a)) / ((c-a).(c-a)), 0, 1)
//                                          edge bc  (1 - t, t),  t = clamp(((p-b).(c-b)) / ((c-b).(c-b)), 0, 1)
//                                          face     (s - v m, v) with s = ((p-a).(b-a)) / ((b-a).(b-a)), m = ((b-a).(c-a)) / ((b-a).(b-a)),
//                                                   e = (c-a) - m (b-a), r = (p-a) - s (b-a), v = (r.e) / (e.e) — only where
//                                                   u >= 0, v >= 0 and u + v <= 1
//                                        (t = 0 for an edge of no length).  A clamped t is exactly 0 or 1, so the vertex regions
//                                        return their vertex exactly; dist2 is NaN only where every candidate's is.
//   ClosestFeatureOnTriangle(..., &feature)  the same, and the code of the candidate that WON: 0 the face candidate, 1 / 2 / 3 the edge
//                                        ab / ac / bc, 4 / 5 / 6 the vertex a / b / c — an edge candidate whose clamped t is exactly 0
//                                        or 1 is a vertex (ab: a, b; ac: a, c; bc: b, c).  It cannot be recovered from (u, v)
//                                        afterwards; include/nanort_sdf.h signs the distance by it.
//   ClosestUV(p, a, b, c) -> (u, v)      the same (u, v) alone; ClosestOnTriangle of them gives the same q and dist2, bit for bit
//                                        (the tests' model states the rule in these two calls).
//   BoxDist2(p, bmin, bmax)              m_k = max(bmin_k - p_k, p_k - bmax_k, 0), the squares summed in the same order.
//
// Why candidates and not a region test.  Ericson's cascade (Real-Time Collision Detection 5.1.5), which this rule was first, decides
// the region from vc = d1*d4 - d3*d2 and its siblings and divides by their sum.  On a triangle whose corners are nearly in line
// those cancel to rounding noise: the point went to the wrong region and the answer was off by a few hundredths on a mesh of size 1, in
// both precisions ("Accuracy").  A minimum over candidates cannot leave the triangle and cannot miss by more than
// its best candidate does.  The edges are exact to rounding whatever the shape.  The foot of the perpendicular is found along ab and
// along e, what is left of ac without its part along ab, after the part of p - a along ab is taken off as well: the error of e's
// direction, which grows as the triangle narrows, then meets only the short vector r and not all of p - a.  Where the foot is
// still uncertain by more than rounding — a narrow triangle seen from afar — the nearest edge point is within the triangle's width
// of it, and the two errors cannot both be large.  The contract the tests hold it to: sqrt(dist2) within 8 eps(T) S of the true
// distance, S the largest absolute coordinate involved; measured 1.1 at most.
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
// The K nearest faces in the place of the nearest one: the K-nearest rule at the end of the file (NearestBound, NearestEnters).
// The faces of an instanced scene in the place of one mesh's: XformPoint, XformBox, BetterInScene, before it.
//
// Included by the device kernels (nanort_amd/csrc/closest.hip, nearest.hip, scene_closest.hip), by the host classes of nanort.h and by the CPU models
// of the tests.
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

// One component of the point (u, v) names, inside [min(a, b, c), max(a, b, c)].
template <typename T>
NANORT_CLOSEST_FN T ClampedWeighted(T a, T b, T c, T w0, T u, T v) {
  T lo = (b < a) ? b : a, hi = (a < b) ? b : a;
  lo = (c < lo) ? c : lo;
  hi = (hi < c) ? c : hi;
  const T x = w0 * a + u * b + v * c;
  return x < lo ? lo : (x > hi ? hi : x);
}

// The point of the triangle that (u, v) name, into q; returns its squared distance to p.
template <typename T>
NANORT_CLOSEST_FN T ClosestOnTriangle(const T p[3], const T a[3], const T b[3], const T c[3], T u, T v, T q[3]) {
  const T w0 = (T(1) - u) - v;
  q[0] = ClampedWeighted(a[0], b[0], c[0], w0, u, v);
  q[1] = ClampedWeighted(a[1], b[1], c[1], w0, u, v);
  q[2] = ClampedWeighted(a[2], b[2], c[2], w0, u, v);
  const T e0 = p[0] - q[0], e1 = p[1] - q[1], e2 = p[2] - q[2];
  return e0 * e0 + e1 * e1 + e2 * e2;
}

// Where on the segment x + t (y - x) the point projects: num / den = ((p - x).(y - x)) / ((y - x).(y - x)) clamped to [0, 1]; 0 for a
// segment of no length (den is a sum of squares: not above 0 only when it is 0 or NaN).
template <typename T>
NANORT_CLOSEST_FN T SegmentParam(T num, T den) {
  if (!(den > T(0))) return T(0);
  const T t = num / den;
  return t < T(0) ? T(0) : (t > T(1) ? T(1) : t);
}

// Which candidate won (ClosestFeatureOnTriangle): the face's interior, an edge or a vertex.
namespace feature_codes {
enum : unsigned int { kFeatureFace = 0u, kFeatureEdgeAB = 1u, kFeatureEdgeAC = 2u, kFeatureEdgeBC = 3u, kFeatureVertexA = 4u, kFeatureVertexB = 5u, kFeatureVertexC = 6u };
}
using namespace feature_codes;

// The code of an edge candidate at parameter t: the vertex at t == 0, the vertex at t == 1, the edge between them otherwise.
template <typename T>
NANORT_CLOSEST_FN unsigned int EdgeFeature(T t, unsigned int edge, unsigned int at0, unsigned int at1) {
  return t == T(0) ? at0 : (t == T(1) ? at1 : edge);
}

// The candidate (cu, cv) with code cf against the best so far (*u, *v, q, *dist2, *feature): taken when strictly nearer, or when the
// best is NaN.
template <typename T>
NANORT_CLOSEST_FN void FeatureCandidate(const T p[3], const T a[3], const T b[3], const T c[3], T cu, T cv, unsigned int cf, T *u, T *v, T q[3],
                                        T *dist2, unsigned int *feature) {
  T cq[3];
  const T d = ClosestOnTriangle(p, a, b, c, cu, cv, cq);
  const bool take = d < *dist2 || *dist2 != *dist2;
  *u = take ? cu : *u, *v = take ? cv : *v;
  q[0] = take ? cq[0] : q[0], q[1] = take ? cq[1] : q[1], q[2] = take ? cq[2] : q[2];
  *dist2 = take ? d : *dist2;
  *feature = take ? cf : *feature;
}

// The nearest point of the triangle to p: (u, v), the point into q and the code of the winning candidate; returns dist2.  See the
// head of the file.
template <typename T>
NANORT_CLOSEST_FN T ClosestFeatureOnTriangle(const T p[3], const T a[3], const T b[3], const T c[3], T *u, T *v, T q[3], unsigned int *feature) {
  const T ab0 = b[0] - a[0], ab1 = b[1] - a[1], ab2 = b[2] - a[2];
  const T ac0 = c[0] - a[0], ac1 = c[1] - a[1], ac2 = c[2] - a[2];
  const T bc0 = c[0] - b[0], bc1 = c[1] - b[1], bc2 = c[2] - b[2];
  const T ap0 = p[0] - a[0], ap1 = p[1] - a[1], ap2 = p[2] - a[2];
  const T bp0 = p[0] - b[0], bp1 = p[1] - b[1], bp2 = p[2] - b[2];
  const T d00 = Dot(ab0, ab1, ab2, ab0, ab1, ab2), d01 = Dot(ab0, ab1, ab2, ac0, ac1, ac2), d11 = Dot(ac0, ac1, ac2, ac0, ac1, ac2);
  const T d1 = Dot(ab0, ab1, ab2, ap0, ap1, ap2), d2 = Dot(ac0, ac1, ac2, ap0, ap1, ap2);
  // the three edges: ab, ac, bc
  const T tab = SegmentParam(d1, d00), tac = SegmentParam(d2, d11);
  const T tbc = SegmentParam(Dot(bc0, bc1, bc2, bp0, bp1, bp2), Dot(bc0, bc1, bc2, bc0, bc1, bc2));
  *u = tab, *v = T(0);
  *feature = EdgeFeature(tab, kFeatureEdgeAB, kFeatureVertexA, kFeatureVertexB);
  T dist2 = ClosestOnTriangle(p, a, b, c, tab, T(0), q);
  FeatureCandidate(p, a, b, c, T(0), tac, EdgeFeature(tac, kFeatureEdgeAC, kFeatureVertexA, kFeatureVertexC), u, v, q, &dist2, feature);
  FeatureCandidate(p, a, b, c, T(1) - tbc, tbc, EdgeFeature(tbc, kFeatureEdgeBC, kFeatureVertexB, kFeatureVertexC), u, v, q, &dist2, feature);
  // the foot of the perpendicular, where its weights say it lies inside (false for the NaN of a triangle without area): along ab,
  // then along what is left of ac once its part along ab is taken off — of p - a, too, before the two meet in a dot product
  const T s = d1 / d00, m = d01 / d00;
  const T e0 = ac0 - m * ab0, e1 = ac1 - m * ab1, e2 = ac2 - m * ab2;
  const T r0 = ap0 - s * ab0, r1 = ap1 - s * ab1, r2 = ap2 - s * ab2;
  const T fv = Dot(r0, r1, r2, e0, e1, e2) / Dot(e0, e1, e2, e0, e1, e2), fu = s - fv * m;
  if (fu >= T(0) && fv >= T(0) && fu + fv <= T(1)) FeatureCandidate(p, a, b, c, fu, fv, (unsigned int)kFeatureFace, u, v, q, &dist2, feature);
  return dist2;
}

// The same without the code.
template <typename T>
NANORT_CLOSEST_FN T ClosestPointOnTriangle(const T p[3], const T a[3], const T b[3], const T c[3], T *u, T *v, T q[3]) {
  unsigned int feature;
  return ClosestFeatureOnTriangle(p, a, b, c, u, v, q, &feature);
}

// The (u, v) alone, for a caller that values them itself: ClosestOnTriangle(p, a, b, c, u, v, q) then gives the q and the dist2 of
// ClosestPointOnTriangle, bit for bit (it is the function that valued the winning candidate).
template <typename T>
NANORT_CLOSEST_FN void ClosestUV(const T p[3], const T a[3], const T b[3], const T c[3], T *u, T *v) {
  T q[3];
  ClosestPointOnTriangle(p, a, b, c, u, v, q);
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

// ---- instanced scenes (include/nanort_hip.h, "closest-point queries on scenes") ---------------------------------
// fp32, as scenes are.  A face of an instance IS the triangle of the three XformPoint images of its local vertices, m the instance's
// local -> world matrix (row 3 the translation: nanosg's convention), and the answer of a query over a scene is the rule above over
// all (node, face) pairs of admitted nodes: the smallest dist2, then the smallest node_id, then the smallest prim_id (BetterInScene) —
// byte for byte the answer over ONE mesh, the world vertices of all instances concatenated in node order.  Nothing is inverted, so a
// singular matrix (an instance flattened to a plane) is inside the contract; finite matrices and vertices are.
//
//   XformPoint(m, v)             w_k = m[0][k]*v0 + m[1][k]*v1 + m[2][k]*v2 + m[3][k], summed left to right: Matrix::MultV of the
//                                scene code (nanort_amd/csrc/common.h, mult_v), operation for operation.
//   XformBox(m, bmin, bmax)      per output component k, the low side is XformPoint's sum over bmin_j where m[j][k] >= 0 and bmax_j
//                                otherwise, the high side over the opposite choice.  Each product and each sum is monotone under
//                                rounding, so in floating point (a) the result is the min / max over the eight XformPoint corner
//                                images — the world box Commit stores for an instance — and (b) it contains XformPoint(m, v) for
//                                every v inside [bmin, bmax].
//
// The clamp of ClosestOnTriangle puts q inside every box that contains the three world vertices, so BoxDist2(p, XformBox(node box))
// <= dist2 holds in floating point for every face below a node of an instance's tree, BoxDist2 of the instance's world box likewise,
// and of every box of a top-level tree over those boxes: Culled hides nothing at either level.
template <typename T, int W>
NANORT_CLOSEST_FN void XformPoint(const T (&m)[4][W], const T v[3], T w[3]) {
  const T w0 = m[0][0] * v[0] + m[1][0] * v[1] + m[2][0] * v[2] + m[3][0];
  const T w1 = m[0][1] * v[0] + m[1][1] * v[1] + m[2][1] * v[2] + m[3][1];
  const T w2 = m[0][2] * v[0] + m[1][2] * v[1] + m[2][2] * v[2] + m[3][2];
  w[0] = w0, w[1] = w1, w[2] = w2;
}

template <typename T, int W>
NANORT_CLOSEST_FN void XformBox(const T (&m)[4][W], const T bmin[3], const T bmax[3], T wmin[3], T wmax[3]) {
  T lo[3], hi[3];
  for (int k = 0; k < 3; k++) {
    const bool up0 = m[0][k] >= T(0), up1 = m[1][k] >= T(0), up2 = m[2][k] >= T(0);
    lo[k] = m[0][k] * (up0 ? bmin[0] : bmax[0]) + m[1][k] * (up1 ? bmin[1] : bmax[1]) + m[2][k] * (up2 ? bmin[2] : bmax[2]) + m[3][k];
    hi[k] = m[0][k] * (up0 ? bmax[0] : bmin[0]) + m[1][k] * (up1 ? bmax[1] : bmin[1]) + m[2][k] * (up2 ? bmax[2] : bmin[2]) + m[3][k];
  }
  for (int k = 0; k < 3; k++) wmin[k] = lo[k], wmax[k] = hi[k];
}

// Better, over the faces of a scene: (dist2, node_id, prim_id) ascending.  `best` starts at r2 with both ids 0xFFFFFFFF.
template <typename T>
NANORT_CLOSEST_FN bool BetterInScene(T dist2, unsigned int node_id, unsigned int prim_id, T best, unsigned int best_node, unsigned int best_prim) {
  return dist2 < best || (dist2 == best && (node_id < best_node || (node_id == best_node && prim_id < best_prim)));
}

// ---- the K nearest faces (include/nanort_hip.h, "nearest-faces queries") -----------------------------------------
// The answer of a query (p, max_dist, K) over a set of admitted faces: the CANDIDATES are the faces whose dist2 is not NaN and
// <= r2 = max_dist * max_dist (a point that is not Searchable has none); they are ranked by the key (dist2, prim_id) ascending —
// dist2 numerically, then prim_id — and the K with the smallest keys are the answer, in that order.  The key is total over the faces
// of a mesh, so which candidates are held never depends on the order in which they were tested, nor on the tree.
//
// A walk holds at most K candidates.  Its BOUND is r2 while fewer than K are held and the worst held dist2 once K are; a subtree is
// skipped iff Culled(BoxDist2, bound) — strictly farther, as above: a box at exactly the bound may hold a face that the prim_id
// prefers.  A candidate ENTERS when fewer than K are held or when Better(dist2, prim_id, worst_dist2, worst_prim_id); the worst is
// then evicted.  With K = 1 this is the rule above.

// The bound of a walk that holds `held` of at most `k` candidates, the worst of them at worst_dist2.
template <typename T>
NANORT_CLOSEST_FN T NearestBound(unsigned int held, unsigned int k, T r2, T worst_dist2) {
  return held < k ? r2 : worst_dist2;
}

// Does the face (dist2, prim_id) enter a held set of `held` of at most `k` candidates whose worst key is (worst_dist2, worst_prim)?
template <typename T>
NANORT_CLOSEST_FN bool NearestEnters(T dist2, unsigned int prim_id, T r2, unsigned int held, unsigned int k, T worst_dist2, unsigned int worst_prim) {
  if (!(dist2 <= r2)) return false;  // (not a candidate: too far, or NaN)
  return held < k || Better<T>(dist2, prim_id, worst_dist2, worst_prim);
}

// A candidate that NearestEnters admitted, into the sorted row[0 .. held) of at most k records (R: any record with the members dist2
// and prim_id): the records behind it move one slot up, the worst is dropped when the row is full.  Returns the new count.
template <typename R>
NANORT_CLOSEST_FN unsigned int NearestInsert(R *row, unsigned int held, unsigned int k, const R &rec) {
  unsigned int j = held < k ? held : k - 1u;  // the slot the shift starts from
  while (j > 0u && Better(rec.dist2, rec.prim_id, row[j - 1u].dist2, row[j - 1u].prim_id)) {
    row[j] = row[j - 1u];
    j--;
  }
  row[j] = rec;
  return held < k ? held + 1u : k;
}

}  // namespace nanort_closest

#endif  // NANORT_CLOSEST_H_
