// tests/scene_closest_model.cc — the CPU model of the closest-point query on an instanced scene (tests/scene_closest_fixture.py
// compiles it with g++ -O2 -ffp-contract=off -fno-fast-math): a plain restatement of the two-level walk of
// nanort_amd/csrc/scene_closest.hip over given trees — a top-level tree over the instances' world boxes or a scan of them in a given
// order, then each instance's own tree through XformBox, its faces through XformPoint — with include/nanort_closest.h's functions.
// It must give the bytes of the brute force over the concatenated world mesh (tests/closest_model.cc) whatever the trees and the order.
// Also XformPoint and XformBox themselves for the numpy restatements of the fixture, and the search for a violation of
// BoxDist2(p, XformBox(box)) <= dist2, the property the cull inside an instance rests on.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "nanort_closest.h"

namespace {

struct Point {
  float p[3];
  float max_dist;
};
struct Record {
  float point[3];
  float dist2, u, v;
  uint32_t prim_id, node_id;
};
struct Node {
  float bmin[3], bmax[3];
  int32_t flag, axis;
  uint32_t data[2];
};
struct Inst { // (the layout of the fixture's ctypes structure)
  const Node *nodes;
  const uint32_t *indices;
  const float *verts;
  const uint32_t *faces;
  float m[4][4];
  float xbmin[3], xbmax[3];
};
static_assert(sizeof(Record) == 32 && sizeof(Node) == 40 && sizeof(Inst) == 32 + 64 + 24, "layouts");

struct Entry {
  uint32_t ref;
  bool inst; // an instance id; else a node of the level's tree
};

void walk_instance(const Inst &in, uint32_t id, const Point &q, Record *r, uint64_t *opened, uint64_t *tested, uint64_t *deepest) {
  std::vector<uint32_t> todo(1, 0u);
  while (!todo.empty()) {
    const Node &nd = in.nodes[todo.back()];
    todo.pop_back();
    (*opened)++;
    float wmin[3], wmax[3];
    nanort_closest::XformBox<float, 4>(in.m, nd.bmin, nd.bmax, wmin, wmax);
    if (nanort_closest::Culled<float>(nanort_closest::BoxDist2<float>(q.p, wmin, wmax), r->dist2)) continue;
    if (nd.flag == 0) {
      float d[2];
      for (int c = 0; c < 2; c++) {
        const Node &ch = in.nodes[nd.data[c]];
        nanort_closest::XformBox<float, 4>(in.m, ch.bmin, ch.bmax, wmin, wmax);
        d[c] = nanort_closest::BoxDist2<float>(q.p, wmin, wmax);
      }
      const bool second = d[1] < d[0];
      if (!nanort_closest::Culled<float>(second ? d[0] : d[1], r->dist2)) todo.push_back(nd.data[second ? 0 : 1]);
      const bool enter = !nanort_closest::Culled<float>(second ? d[1] : d[0], r->dist2);
      if (enter) todo.push_back(nd.data[second ? 1 : 0]);
      if (todo.size() - (enter ? 1 : 0) > *deepest) *deepest = todo.size() - (enter ? 1 : 0); // (the node about to be opened does not wait)
    } else {
      for (uint32_t k = 0; k < nd.data[0]; k++) {
        const uint32_t prim = in.indices[nd.data[1] + k];
        float w[3][3];
        for (int c = 0; c < 3; c++) nanort_closest::XformPoint<float, 4>(in.m, in.verts + 3 * (size_t)in.faces[3 * (size_t)prim + c], w[c]);
        float u, v, pt[3];
        const float dist2 = nanort_closest::ClosestPointOnTriangle<float>(q.p, w[0], w[1], w[2], &u, &v, pt);
        (*tested)++;
        if (!nanort_closest::BetterInScene<float>(dist2, id, prim, r->dist2, r->node_id, r->prim_id)) continue;
        r->point[0] = pt[0], r->point[1] = pt[1], r->point[2] = pt[2];
        r->dist2 = dist2;
        r->u = u, r->v = v;
        r->prim_id = prim, r->node_id = id;
      }
    }
  }
}

} // namespace

extern "C" {

// top_nodes == NULL: the instances are scanned in the order `scan_order` names them (num_insts ids).  node_masks / point_masks: both
// or neither.  stats[0] += nodes opened (both levels), [1] += instances entered, [2] += triangles tested; stats[3]: the most entries
// of an instance's tree waiting at once.
void scm_walk(const void *insts_v, uint32_t num_insts, const void *top_nodes_v, const uint32_t *top_indices, const uint32_t *scan_order,
              const uint32_t *node_masks, const uint32_t *point_masks, const void *pts_v, uint64_t n, void *out_v, uint8_t *found, uint64_t *stats) {
  const Inst *insts = (const Inst *)insts_v;
  const Node *top = (const Node *)top_nodes_v;
  const Point *pts = (const Point *)pts_v;
  Record *out = (Record *)out_v;
  std::vector<Entry> todo;
  for (uint64_t i = 0; i < n; i++) {
    const Point &q = pts[i];
    Record *r = &out[i];
    r->point[0] = q.p[0], r->point[1] = q.p[1], r->point[2] = q.p[2];
    r->dist2 = q.max_dist * q.max_dist;
    r->u = r->v = 0.0f;
    r->prim_id = r->node_id = 0xFFFFFFFFu;
    if (nanort_closest::Searchable<float>(q.p, q.max_dist)) {
      todo.clear();
      if (top)
        todo.push_back(Entry{0u, false});
      else
        for (uint32_t k = num_insts; k > 0; k--) todo.push_back(Entry{scan_order[k - 1], true});
      while (!todo.empty()) {
        const Entry e = todo.back();
        todo.pop_back();
        if (e.inst) {
          const Inst &in = insts[e.ref];
          if (node_masks && (node_masks[e.ref] & point_masks[i]) == 0u) continue;
          if (nanort_closest::Culled<float>(nanort_closest::BoxDist2<float>(q.p, in.xbmin, in.xbmax), r->dist2)) continue;
          stats[1]++;
          walk_instance(in, e.ref, q, r, &stats[0], &stats[2], &stats[3]);
          continue;
        }
        const Node &nd = top[e.ref];
        stats[0]++;
        if (nanort_closest::Culled<float>(nanort_closest::BoxDist2<float>(q.p, nd.bmin, nd.bmax), r->dist2)) continue;
        if (nd.flag == 0) {
          const Node &n0 = top[nd.data[0]], &n1 = top[nd.data[1]];
          const float d0 = nanort_closest::BoxDist2<float>(q.p, n0.bmin, n0.bmax), d1 = nanort_closest::BoxDist2<float>(q.p, n1.bmin, n1.bmax);
          const bool second = d1 < d0;
          if (!nanort_closest::Culled<float>(second ? d0 : d1, r->dist2)) todo.push_back(Entry{nd.data[second ? 0 : 1], false});
          if (!nanort_closest::Culled<float>(second ? d1 : d0, r->dist2)) todo.push_back(Entry{nd.data[second ? 1 : 0], false});
        } else {
          for (uint32_t k = nd.data[0]; k > 0; k--) todo.push_back(Entry{top_indices[nd.data[1] + k - 1], true});
        }
      }
    }
    if (found) found[i] = r->prim_id != 0xFFFFFFFFu ? 1 : 0;
  }
}

// out[i] = XformPoint(m[i], v[i]): m 16 floats, v and out 3.
void scm_xform_points(const float *m, const float *v, uint64_t n, float *out) {
  for (uint64_t i = 0; i < n; i++) nanort_closest::XformPoint<float, 4>(*(const float(*)[4][4])(m + 16 * i), v + 3 * i, out + 3 * i);
}

// (wmin[i], wmax[i]) = XformBox(m[i], bmin[i], bmax[i]).
void scm_xform_boxes(const float *m, const float *bmin, const float *bmax, uint64_t n, float *wmin, float *wmax) {
  for (uint64_t i = 0; i < n; i++) nanort_closest::XformBox<float, 4>(*(const float(*)[4][4])(m + 16 * i), bmin + 3 * i, bmax + 3 * i, wmin + 3 * i, wmax + 3 * i);
}

// cases[i] = {m[16], bmin[3], bmax[3], a[3], b[3], c[3] (local), p[3] (world)} (34 floats): counts[0] += BoxDist2(p, XformBox) > dist2
// (violations), counts[1] += equalities, counts[2] += cases whose box does not contain the three local vertices (not looked at).
void scm_bound_search(const float *cases, uint64_t n, uint64_t *counts) {
  for (uint64_t i = 0; i < n; i++) {
    const float *c = cases + 34 * i, *bmin = c + 16, *bmax = c + 19, *p = c + 31;
    const float(&m)[4][4] = *(const float(*)[4][4])c;
    bool inside = true;
    for (int t = 0; t < 3; t++)
      for (int k = 0; k < 3; k++) inside = inside && bmin[k] <= c[22 + 3 * t + k] && c[22 + 3 * t + k] <= bmax[k];
    if (!inside) {
      counts[2]++;
      continue;
    }
    float w[3][3], wmin[3], wmax[3], u, v, q[3];
    for (int t = 0; t < 3; t++) nanort_closest::XformPoint<float, 4>(m, c + 22 + 3 * t, w[t]);
    nanort_closest::XformBox<float, 4>(m, bmin, bmax, wmin, wmax);
    const float dist2 = nanort_closest::ClosestPointOnTriangle<float>(p, w[0], w[1], w[2], &u, &v, q);
    const float box = nanort_closest::BoxDist2<float>(p, wmin, wmax);
    if (!(dist2 == dist2)) continue; // (a NaN dist2 is never an answer)
    counts[0] += box > dist2 ? 1u : 0u;
    counts[1] += box == dist2 ? 1u : 0u;
  }
}

} // extern "C"
