// tests/sdf_model.cc — the CPU model of the signed distance query (tests/sdf_fixture.py compiles it with g++ -O2 -ffp-contract=off
// -fno-fast-math): include/nanort_sdf.h's rule as a brute-force loop over the faces — THE statement of what every implementation has
// to answer, byte for byte, for GIVEN normals — a plain restatement of the walk over a given node and index array, the normals of a
// mesh by the header's host builder, and ClosestFeatureOnTriangle beside ClosestPointOnTriangle for the bit-for-bit check.
//
// Records are the library's: point {T p[3], max_dist}, answer {T point[3], dist2, u, v; u32 prim_id, feature}; nodes are BVHNode<T>.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "nanort_sdf.h"

namespace {

template <typename T>
struct Point {
  T p[3];
  T max_dist;
};
template <typename T>
struct Record {
  T point[3];
  T dist2, u, v;
  uint32_t prim_id, feature;
};
template <typename T>
struct Node {
  T bmin[3], bmax[3];
  int32_t flag, axis;
  uint32_t data[2];
};
static_assert(sizeof(Record<float>) == 32 && sizeof(Record<double>) == 56 && sizeof(Node<float>) == 40 && sizeof(Node<double>) == 64, "layouts");

struct Options {
  uint32_t range0, range1, skip;
};

template <typename T>
struct Mesh {
  const T *verts;
  const uint32_t *faces;
  const T *fnormals, *vnormals; // [nf][4][3], [nv][3]
  bool face_normal_only;        // the shortcut the wedge class exposes: sign by the face's unit normal whatever the feature
};

template <typename T>
void begin(const Point<T> &q, Record<T> *r) {
  r->point[0] = q.p[0], r->point[1] = q.p[1], r->point[2] = q.p[2];
  r->dist2 = q.max_dist * q.max_dist;
  r->u = r->v = T(0);
  r->prim_id = 0xFFFFFFFFu;
  r->feature = 0u;
}

// Face `prim` against the best so far; r->feature carries the bare code until finish().
template <typename T>
void offer(const Point<T> &q, const Mesh<T> &m, uint32_t prim, const Options &o, Record<T> *r) {
  if (prim < o.range0 || prim >= o.range1 || prim == o.skip) return;
  const T *a = m.verts + 3 * (size_t)m.faces[3 * (size_t)prim + 0], *b = m.verts + 3 * (size_t)m.faces[3 * (size_t)prim + 1],
          *c = m.verts + 3 * (size_t)m.faces[3 * (size_t)prim + 2];
  T u, v, pt[3];
  unsigned int feature;
  const T dist2 = nanort_sdf::ClosestFeatureOnTriangle<T>(q.p, a, b, c, &u, &v, pt, &feature);
  if (!nanort_closest::Better<T>(dist2, prim, r->dist2, r->prim_id)) return;
  r->point[0] = pt[0], r->point[1] = pt[1], r->point[2] = pt[2];
  r->dist2 = dist2;
  r->u = u, r->v = v;
  r->prim_id = prim;
  r->feature = feature;
}

// The sign, once per query.
template <typename T>
void finish(const Point<T> &q, const Mesh<T> &m, Record<T> *r, uint8_t *found) {
  const bool have = r->prim_id != 0xFFFFFFFFu;
  if (found) *found = have ? 1 : 0;
  if (!have) return;
  const uint32_t f = r->feature;
  const T *n = m.fnormals + 12 * (size_t)r->prim_id + (m.face_normal_only ? 0 : 3 * f);
  if (f >= 4u && !m.face_normal_only) n = m.vnormals + 3 * (size_t)m.faces[3 * (size_t)r->prim_id + (f - 4u)];
  r->feature = nanort_sdf::FeatureWord<T>(q.p, r->point, n, f);
}

template <typename T>
void brute(const Mesh<T> &m, uint32_t nf, const Point<T> *pts, uint64_t n, const Options &o, Record<T> *out, uint8_t *found) {
  for (uint64_t i = 0; i < n; i++) {
    begin(pts[i], &out[i]);
    if (nanort_closest::Searchable<T>(pts[i].p, pts[i].max_dist))
      for (uint32_t f = 0; f < nf; f++) offer(pts[i], m, f, o, &out[i]);
    finish(pts[i], m, &out[i], found ? found + i : nullptr);
  }
}

// The walk of tests/closest_model.cc: a subtree is skipped iff its box lies strictly farther than the best so far.
template <typename T>
void walk(const Node<T> *nodes, const uint32_t *indices, const Mesh<T> &m, const Point<T> *pts, uint64_t n, const Options &o, Record<T> *out,
          uint8_t *found) {
  std::vector<uint32_t> todo;
  for (uint64_t i = 0; i < n; i++) {
    begin(pts[i], &out[i]);
    if (nanort_closest::Searchable<T>(pts[i].p, pts[i].max_dist)) {
      todo.assign(1, 0u);
      while (!todo.empty()) {
        const Node<T> &nd = nodes[todo.back()];
        todo.pop_back();
        if (nanort_closest::Culled<T>(nanort_closest::BoxDist2<T>(pts[i].p, nd.bmin, nd.bmax), out[i].dist2)) continue;
        if (nd.flag == 0) {
          const Node<T> &n0 = nodes[nd.data[0]], &n1 = nodes[nd.data[1]];
          const T d0 = nanort_closest::BoxDist2<T>(pts[i].p, n0.bmin, n0.bmax), d1 = nanort_closest::BoxDist2<T>(pts[i].p, n1.bmin, n1.bmax);
          const bool second = d1 < d0;
          if (!nanort_closest::Culled<T>(second ? d0 : d1, out[i].dist2)) todo.push_back(nd.data[second ? 0 : 1]);
          if (!nanort_closest::Culled<T>(second ? d1 : d0, out[i].dist2)) todo.push_back(nd.data[second ? 1 : 0]);
        } else {
          for (uint32_t k = 0; k < nd.data[0]; k++) offer(pts[i], m, indices[nd.data[1] + k], o, &out[i]);
        }
      }
    }
    finish(pts[i], m, &out[i], found ? found + i : nullptr);
  }
}

// cases[i] = {p[3], a[3], b[3], c[3]} (12 T).  out[i] = {u, v, q[3], dist2} twice (ClosestFeatureOnTriangle, then
// ClosestPointOnTriangle: 12 T), features[i] the code.
template <typename T>
void feature_cases(const T *cases, uint64_t n, T *out, uint32_t *features) {
  for (uint64_t i = 0; i < n; i++) {
    const T *p = cases + 12 * i, *a = p + 3, *b = p + 6, *c = p + 9;
    T *o = out + 12 * i;
    unsigned int f = 99u;
    o[5] = nanort_sdf::ClosestFeatureOnTriangle<T>(p, a, b, c, &o[0], &o[1], &o[2], &f);
    o[11] = nanort_closest::ClosestPointOnTriangle<T>(p, a, b, c, &o[6], &o[7], &o[8]);
    features[i] = f;
  }
}

} // namespace

#define SDM_EXPORTS(T, S)                                                                                                                      \
  void sdm_normals_##S(const T *verts, const uint32_t *faces, uint32_t nf, uint32_t nv, T *fnormals, T *vnormals) {                            \
    nanort_sdf::BuildFeatureNormals<T>(verts, faces, nf, nv, fnormals, vnormals);                                                              \
  }                                                                                                                                            \
  void sdm_brute_##S(const T *verts, const uint32_t *faces, uint32_t nf, const T *fnormals, const T *vnormals, int face_normal_only,          \
                     const void *pts, uint64_t n, const uint32_t *opt3, void *out, uint8_t *found) {                                           \
    const Mesh<T> m = {verts, faces, fnormals, vnormals, face_normal_only != 0};                                                               \
    brute<T>(m, nf, (const Point<T> *)pts, n, Options{opt3[0], opt3[1], opt3[2]}, (Record<T> *)out, found);                                    \
  }                                                                                                                                            \
  void sdm_walk_##S(const void *nodes, const uint32_t *indices, const T *verts, const uint32_t *faces, const T *fnormals, const T *vnormals,  \
                    const void *pts, uint64_t n, const uint32_t *opt3, void *out, uint8_t *found) {                                            \
    const Mesh<T> m = {verts, faces, fnormals, vnormals, false};                                                                               \
    walk<T>((const Node<T> *)nodes, indices, m, (const Point<T> *)pts, n, Options{opt3[0], opt3[1], opt3[2]}, (Record<T> *)out, found);        \
  }                                                                                                                                            \
  void sdm_feature_cases_##S(const T *cases, uint64_t n, T *out, uint32_t *features) { feature_cases<T>(cases, n, out, features); }

extern "C" {
SDM_EXPORTS(float, f32)
SDM_EXPORTS(double, f64)
}
