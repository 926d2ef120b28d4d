// tests/closest_model.cc — the CPU model of the closest-point query (tests/closest_fixture.py compiles it with
// g++ -O2 -ffp-contract=off -fno-fast-math): include/nanort_closest.h's rule as a brute-force loop over the faces — THE statement of
// what every implementation has to answer, byte for byte — and a plain restatement of the walk over a given node and index array,
// which must give the same bytes on any tree whose boxes contain their triangles.  Also the search for a violation of
// BoxDist2 <= dist2, the property the walk's cull rests on.
//
// Records are the library's: point {T p[3], max_dist}, answer {T point[3], dist2, u, v; u32 prim_id, pad}; nodes are BVHNode<T>
// {T bmin[3], bmax[3]; i32 flag, axis; u32 data[2]}.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "nanort_closest.h"

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
  uint32_t prim_id, pad;
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
void begin(const Point<T> &q, Record<T> *r) {
  r->point[0] = q.p[0], r->point[1] = q.p[1], r->point[2] = q.p[2];
  r->dist2 = q.max_dist * q.max_dist;
  r->u = r->v = T(0);
  r->prim_id = 0xFFFFFFFFu;
  r->pad = 0u;
}

// Face `prim` against the best so far.  *dist2_out (optional): the face's own dist2.
template <typename T>
void offer(const Point<T> &q, const T *verts, const uint32_t *faces, uint32_t prim, const Options &o, Record<T> *r, T *dist2_out = nullptr) {
  if (prim < o.range0 || prim >= o.range1 || prim == o.skip) return;
  const T *a = verts + 3 * (size_t)faces[3 * (size_t)prim + 0], *b = verts + 3 * (size_t)faces[3 * (size_t)prim + 1],
          *c = verts + 3 * (size_t)faces[3 * (size_t)prim + 2];
  T u, v, pt[3];
  nanort_closest::ClosestUV<T>(q.p, a, b, c, &u, &v);
  const T dist2 = nanort_closest::ClosestOnTriangle<T>(q.p, a, b, c, u, v, pt);
  if (dist2_out) *dist2_out = dist2;
  if (!nanort_closest::Better<T>(dist2, prim, r->dist2, r->prim_id)) return;
  r->point[0] = pt[0], r->point[1] = pt[1], r->point[2] = pt[2];
  r->dist2 = dist2;
  r->u = u, r->v = v;
  r->prim_id = prim;
}

// Brute force.  ties_out[i] (optional): how many admitted faces attain point i's minimum (0 when nothing is found).
template <typename T>
void brute(const T *verts, const uint32_t *faces, uint32_t nf, const Point<T> *pts, uint64_t n, const Options &o, Record<T> *out, uint8_t *found,
           uint32_t *ties_out) {
  std::vector<T> d2(ties_out ? nf : 0);
  for (uint64_t i = 0; i < n; i++) {
    begin(pts[i], &out[i]);
    uint32_t ties = 0;
    if (nanort_closest::Searchable<T>(pts[i].p, pts[i].max_dist)) {
      for (uint32_t f = 0; f < nf; f++) {
        T d = T(-1);
        offer(pts[i], verts, faces, f, o, &out[i], &d);
        if (ties_out) d2[f] = d; // (-1: not admitted; dist2 is never negative)
      }
      if (ties_out && out[i].prim_id != 0xFFFFFFFFu)
        for (uint32_t f = 0; f < nf; f++) ties += d2[f] == out[i].dist2 ? 1u : 0u;
    }
    if (found) found[i] = out[i].prim_id != 0xFFFFFFFFu ? 1 : 0;
    if (ties_out) ties_out[i] = ties;
  }
}

// The walk: a subtree is skipped iff its box lies strictly farther than the best so far, tested when the node is opened; at a branch
// the nearer child is opened first (on ties the first), the farther one waits unless it is culled already.
template <typename T>
void walk(const Node<T> *nodes, const uint32_t *indices, const T *verts, const uint32_t *faces, const Point<T> *pts, uint64_t n, const Options &o,
          Record<T> *out, uint8_t *found, uint64_t *opened_out) {
  std::vector<uint32_t> todo;
  uint64_t opened = 0, deepest = 0; // deepest: most entries WAITING at once (the node about to be opened is not one of them)
  for (uint64_t i = 0; i < n; i++) {
    begin(pts[i], &out[i]);
    if (nanort_closest::Searchable<T>(pts[i].p, pts[i].max_dist)) {
      todo.assign(1, 0u);
      while (!todo.empty()) {
        const Node<T> &nd = nodes[todo.back()];
        todo.pop_back();
        opened++;
        if (nanort_closest::Culled<T>(nanort_closest::BoxDist2<T>(pts[i].p, nd.bmin, nd.bmax), out[i].dist2)) continue;
        if (nd.flag == 0) {
          const Node<T> &n0 = nodes[nd.data[0]], &n1 = nodes[nd.data[1]];
          const T d0 = nanort_closest::BoxDist2<T>(pts[i].p, n0.bmin, n0.bmax), d1 = nanort_closest::BoxDist2<T>(pts[i].p, n1.bmin, n1.bmax);
          const bool second = d1 < d0;
          if (!nanort_closest::Culled<T>(second ? d0 : d1, out[i].dist2)) todo.push_back(nd.data[second ? 0 : 1]);
          const bool enter = !nanort_closest::Culled<T>(second ? d1 : d0, out[i].dist2);
          if (enter) todo.push_back(nd.data[second ? 1 : 0]);
          if (todo.size() - (enter ? 1 : 0) > deepest) deepest = todo.size() - (enter ? 1 : 0);
        } else {
          for (uint32_t k = 0; k < nd.data[0]; k++) offer(pts[i], verts, faces, indices[nd.data[1] + k], o, &out[i]);
        }
      }
    }
    if (found) found[i] = out[i].prim_id != 0xFFFFFFFFu ? 1 : 0;
  }
  if (opened_out) opened_out[0] = opened, opened_out[1] = deepest;
}

// cases[i] = {p[3], a[3], b[3], c[3], bmin[3], bmax[3]} (18 T): counts[0] += BoxDist2 > dist2 (violations), counts[1] += equalities,
// counts[2] += cases whose box does not contain the three vertices (a fault of the caller's: not looked at).
template <typename T>
void bound_search(const T *cases, uint64_t n, uint64_t *counts) {
  for (uint64_t i = 0; i < n; i++) {
    const T *p = cases + 18 * i, *a = p + 3, *b = p + 6, *c = p + 9, *bmin = p + 12, *bmax = p + 15;
    bool inside = true;
    for (int k = 0; k < 3; k++)
      inside = inside && bmin[k] <= a[k] && a[k] <= bmax[k] && bmin[k] <= b[k] && b[k] <= bmax[k] && bmin[k] <= c[k] && c[k] <= bmax[k];
    if (!inside) {
      counts[2]++;
      continue;
    }
    T u, v, q[3];
    nanort_closest::ClosestUV<T>(p, a, b, c, &u, &v);
    const T dist2 = nanort_closest::ClosestOnTriangle<T>(p, a, b, c, u, v, q);
    const T box = nanort_closest::BoxDist2<T>(p, bmin, bmax);
    if (!(dist2 == dist2)) continue; // (a NaN dist2 is never an answer)
    counts[0] += box > dist2 ? 1u : 0u;
    counts[1] += box == dist2 ? 1u : 0u;
  }
}

} // namespace

#define CLM_EXPORTS(T, S)                                                                                                                          \
  void clm_brute_##S(const T *verts, const uint32_t *faces, uint32_t nf, const void *pts, uint64_t n, const uint32_t *opt3, void *out,            \
                     uint8_t *found, uint32_t *ties_out) {                                                                                         \
    brute<T>(verts, faces, nf, (const Point<T> *)pts, n, Options{opt3[0], opt3[1], opt3[2]}, (Record<T> *)out, found, ties_out);                   \
  }                                                                                                                                                \
  void clm_walk_##S(const void *nodes, const uint32_t *indices, const T *verts, const uint32_t *faces, const void *pts, uint64_t n,                \
                    const uint32_t *opt3, void *out, uint8_t *found, uint64_t *opened_out /* [2] */) {                                             \
    walk<T>((const Node<T> *)nodes, indices, verts, faces, (const Point<T> *)pts, n, Options{opt3[0], opt3[1], opt3[2]}, (Record<T> *)out, found, \
            opened_out);                                                                                                                           \
  }                                                                                                                                                \
  void clm_bound_search_##S(const T *cases, uint64_t n, uint64_t *counts3) { bound_search<T>(cases, n, counts3); }

extern "C" {
CLM_EXPORTS(float, f32)
CLM_EXPORTS(double, f64)
}
