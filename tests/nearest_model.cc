// tests/nearest_model.cc — the CPU model of the nearest-faces query (tests/nearest_fixture.py compiles it with
// g++ -O2 -ffp-contract=off -fno-fast-math): include/nanort_closest.h's K-nearest rule as a brute-force loop over the faces with the
// K-buffer — THE statement of what every implementation has to answer, byte for byte — and a plain restatement of the walk over a
// given node and index array, which must give the same bytes on any tree whose boxes contain their triangles.
//
// The model shares NearestEnters / NearestInsert with the code under test, so it cannot vouch for them: tests/nearest_fixture.py
// checks it against a numpy sort of per-face distances (independent_rows).
//
// Records are the library's (tests/closest_model.cc): point {T p[3], max_dist}, answer {T point[3], dist2, u, v; u32 prim_id, pad};
// a row is K answers, counts a u32 per point.
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

// The held set of one point: row[0 .. held), sorted.
template <typename T>
struct Held {
  Record<T> *row;
  uint32_t k, held;
  T r2;
  T worst_dist2() const { return held == k ? row[k - 1].dist2 : r2; }
  uint32_t worst_prim() const { return held == k ? row[k - 1].prim_id : 0xFFFFFFFFu; }
  T bound() const { return nanort_closest::NearestBound<T>(held, k, r2, worst_dist2()); }
};

// Face `prim` against the held set.
template <typename T>
void offer(const Point<T> &q, const T *verts, const uint32_t *faces, uint32_t prim, const Options &o, Held<T> *h) {
  if (prim < o.range0 || prim >= o.range1 || prim == o.skip) return;
  const T *a = verts + 3 * (size_t)faces[3 * (size_t)prim + 0], *b = verts + 3 * (size_t)faces[3 * (size_t)prim + 1],
          *c = verts + 3 * (size_t)faces[3 * (size_t)prim + 2];
  Record<T> rec;
  nanort_closest::ClosestUV<T>(q.p, a, b, c, &rec.u, &rec.v);
  rec.dist2 = nanort_closest::ClosestOnTriangle<T>(q.p, a, b, c, rec.u, rec.v, rec.point);
  rec.prim_id = prim;
  rec.pad = 0u;
  if (!nanort_closest::NearestEnters<T>(rec.dist2, prim, h->r2, h->held, h->k, h->worst_dist2(), h->worst_prim())) return;
  h->held = nanort_closest::NearestInsert(h->row, h->held, h->k, rec);
}

template <typename T>
void finish(const Point<T> &q, const Held<T> &h, uint32_t *count) {
  for (uint32_t j = h.held; j < h.k; j++) {
    Record<T> &r = h.row[j];
    r.point[0] = q.p[0], r.point[1] = q.p[1], r.point[2] = q.p[2];
    r.dist2 = h.r2;
    r.u = r.v = T(0);
    r.prim_id = 0xFFFFFFFFu;
    r.pad = 0u;
  }
  if (count) *count = h.held;
}

// Brute force: every face in id order, or in DESCENDING id order (`reversed`: the held set must not depend on the order).
template <typename T>
void brute(const T *verts, const uint32_t *faces, uint32_t nf, const Point<T> *pts, uint64_t n, uint32_t k, const Options &o, Record<T> *out,
           uint32_t *counts, int reversed) {
  for (uint64_t i = 0; i < n; i++) {
    Held<T> h = {out + i * (size_t)k, k, 0u, pts[i].max_dist * pts[i].max_dist};
    if (nanort_closest::Searchable<T>(pts[i].p, pts[i].max_dist))
      for (uint32_t f = 0; f < nf; f++) offer(pts[i], verts, faces, reversed ? nf - 1u - f : f, o, &h);
    finish(pts[i], h, counts ? counts + i : nullptr);
  }
}

// The walk of tests/closest_model.cc with the K-nearest bound in the place of the best distance.
template <typename T>
void walk(const Node<T> *nodes, const uint32_t *indices, const T *verts, const uint32_t *faces, const Point<T> *pts, uint64_t n, uint32_t k,
          const Options &o, Record<T> *out, uint32_t *counts, uint64_t *opened_out) {
  std::vector<uint32_t> todo;
  uint64_t opened = 0, deepest = 0; // deepest: most entries WAITING at once (the node about to be opened is not one of them)
  for (uint64_t i = 0; i < n; i++) {
    Held<T> h = {out + i * (size_t)k, k, 0u, pts[i].max_dist * pts[i].max_dist};
    if (nanort_closest::Searchable<T>(pts[i].p, pts[i].max_dist)) {
      todo.assign(1, 0u);
      while (!todo.empty()) {
        const Node<T> &nd = nodes[todo.back()];
        todo.pop_back();
        opened++;
        if (nanort_closest::Culled<T>(nanort_closest::BoxDist2<T>(pts[i].p, nd.bmin, nd.bmax), h.bound())) continue;
        if (nd.flag == 0) {
          const Node<T> &n0 = nodes[nd.data[0]], &n1 = nodes[nd.data[1]];
          const T d0 = nanort_closest::BoxDist2<T>(pts[i].p, n0.bmin, n0.bmax), d1 = nanort_closest::BoxDist2<T>(pts[i].p, n1.bmin, n1.bmax);
          const bool second = d1 < d0;
          if (!nanort_closest::Culled<T>(second ? d0 : d1, h.bound())) todo.push_back(nd.data[second ? 0 : 1]);
          const bool enter = !nanort_closest::Culled<T>(second ? d1 : d0, h.bound());
          if (enter) todo.push_back(nd.data[second ? 1 : 0]);
          if (todo.size() - (enter ? 1 : 0) > deepest) deepest = todo.size() - (enter ? 1 : 0);
        } else {
          for (uint32_t j = 0; j < nd.data[0]; j++) offer(pts[i], verts, faces, indices[nd.data[1] + j], o, &h);
        }
      }
    }
    finish(pts[i], h, counts ? counts + i : nullptr);
  }
  if (opened_out) opened_out[0] = opened, opened_out[1] = deepest;
}

} // namespace

#define NRM_EXPORTS(T, S)                                                                                                                       \
  void nrm_brute_##S(const T *verts, const uint32_t *faces, uint32_t nf, const void *pts, uint64_t n, uint32_t k, const uint32_t *opt3,         \
                     void *out, uint32_t *counts, int reversed) {                                                                               \
    brute<T>(verts, faces, nf, (const Point<T> *)pts, n, k, Options{opt3[0], opt3[1], opt3[2]}, (Record<T> *)out, counts, reversed);            \
  }                                                                                                                                             \
  void nrm_walk_##S(const void *nodes, const uint32_t *indices, const T *verts, const uint32_t *faces, const void *pts, uint64_t n, uint32_t k, \
                    const uint32_t *opt3, void *out, uint32_t *counts, uint64_t *opened_out /* [2] */) {                                        \
    walk<T>((const Node<T> *)nodes, indices, verts, faces, (const Point<T> *)pts, n, k, Options{opt3[0], opt3[1], opt3[2]}, (Record<T> *)out,   \
            counts, opened_out);                                                                                                                \
  }

extern "C" {
NRM_EXPORTS(float, f32)
NRM_EXPORTS(double, f64)
}
