// tests/cpp/refit_prims_check.cc — BVHAccel::RefitGeometry of include/nanort.h with the HIP backend (tests/test_gpu_refit_prims.py).
//
//   refit_prims_check DIR
// DIR holds spheres0.bin, spheres1.bin ({u32 n, float centres[n][3], float radii[n]}), curves0.bin, curves1.bin ({u32 n, float
// cps[n][12], float radii[n][4]}), the same counts in both of a pair, and srays.bin, crays.bin ({u64 m, Ray<float>[m]}).
// Per kind: Build on set 0, copy, RefitGeometry to set 1: the refit object answers on set 1, the copy still on set 0 and its old
// tree; kind and count mismatches refuse with a reason and change nothing; Refit(geometry) still refuses.  "Answers on" means:
// TraverseBatch equals the same object's per-ray host Traverse over the arrays it was last given (t and prim_id bit for bit,
// the flags; the spheres' u / v, which the host derives in double, within 1e-6).
// Writes DIR/spheres_out.bin and DIR/curves_out.bin: {u64 num_nodes, u64 num_indices, nodes before, indices, nodes after}.
// Prints `devices D checks N mismatches M`; exits 1 on a mismatch.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "nanort.h"

using nanort::BVHAccel;
using nanort::Ray;

namespace {

unsigned long long g_checks = 0, g_bad = 0;

void expect(const char *where, const char *what, bool cond) {
  g_checks++;
  if (!cond) {
    g_bad++;
    fprintf(stderr, "MISMATCH %s: %s\n", where, what);
  }
}

struct Prims {
  unsigned int n = 0;
  std::vector<float> pos, radii;
};

bool read_prims(const std::string &path, size_t pos_floats, size_t radius_floats, Prims *p) {
  FILE *fp = fopen(path.c_str(), "rb");
  if (!fp) return false;
  uint32_t n = 0;
  bool ok = fread(&n, 4, 1, fp) == 1;
  p->n = n;
  p->pos.resize(pos_floats * n);
  p->radii.resize(radius_floats * n);
  ok = ok && fread(p->pos.data(), 4, p->pos.size(), fp) == p->pos.size() && fread(p->radii.data(), 4, p->radii.size(), fp) == p->radii.size();
  fclose(fp);
  return ok;
}

bool read_rays(const std::string &path, std::vector<Ray<float> > *out) {
  FILE *fp = fopen(path.c_str(), "rb");
  if (!fp) return false;
  uint64_t m = 0;
  bool ok = fread(&m, 8, 1, fp) == 1;
  out->resize((size_t)m);
  ok = ok && fread(static_cast<void *>(out->data()), sizeof(Ray<float>), out->size(), fp) == out->size();
  fclose(fp);
  return ok;
}

void check_spheres(const char *where, const BVHAccel<float> &a, const Prims &p, const std::vector<Ray<float> > &rays) {
  typedef nanort::SphereIntersection H;
  const size_t m = rays.size();
  std::vector<H> bh(m);
  std::vector<unsigned char> bm(m, 7);
  expect(where, "TraverseBatch", a.TraverseBatch(rays.data(), m, bh.data(), bm.data()));
  unsigned long long bad = 0, hits = 0;
  for (size_t i = 0; i < m; i++) {
    nanort::SphereIntersector<> isect(p.pos.data(), p.radii.data());
    H hh;
    const unsigned char hm = a.Traverse(rays[i], isect, &hh) ? 1 : 0;
    hits += hm;
    bad += bm[i] != hm || (hm && (memcmp(&bh[i].t, &hh.t, 4) != 0 || bh[i].prim_id != hh.prim_id || !(fabsf(bh[i].u - hh.u) <= 1e-6f) ||
                                  !(fabsf(bh[i].v - hh.v) <= 1e-6f)));
  }
  expect(where, "TraverseBatch == Traverse", bad == 0);
  expect(where, "some rays hit", hits > 0);
}

void check_curves(const char *where, const BVHAccel<float> &a, const Prims &p, const std::vector<Ray<float> > &rays) {
  typedef nanort::BezierCurveIntersection H;
  const size_t m = rays.size();
  std::vector<H> bh(m);
  std::vector<unsigned char> bm(m, 7);
  expect(where, "TraverseBatch", a.TraverseBatch(rays.data(), m, bh.data(), bm.data()));
  unsigned long long bad = 0, hits = 0;
  for (size_t i = 0; i < m; i++) {
    nanort::BezierCurveIntersector<> isect(p.pos.data(), p.radii.data(), 4);
    H hh;
    const unsigned char hm = a.Traverse(rays[i], isect, &hh) ? 1 : 0;
    hits += hm;
    bad += bm[i] != hm || (hm && memcmp(static_cast<const void *>(&bh[i]), static_cast<const void *>(&hh), sizeof(H)) != 0);
  }
  expect(where, "TraverseBatch == Traverse", bad == 0);
  expect(where, "some rays hit", hits > 0);
}

typedef std::vector<nanort::BVHNode<float> > Nodes;

bool same_nodes(const Nodes &a, const Nodes &b) { return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0; }

bool write_trees(const std::string &path, const Nodes &before, const std::vector<unsigned int> &indices, const Nodes &after) {
  FILE *fp = fopen(path.c_str(), "wb");
  if (!fp) return false;
  const uint64_t nn = before.size(), ni = indices.size();
  bool ok = after.size() == before.size() && fwrite(&nn, 8, 1, fp) == 1 && fwrite(&ni, 8, 1, fp) == 1;
  ok = ok && fwrite(before.data(), sizeof(before[0]), nn, fp) == nn && fwrite(indices.data(), 4, ni, fp) == ni;
  ok = ok && fwrite(after.data(), sizeof(after[0]), nn, fp) == nn;
  fclose(fp);
  return ok;
}

// The scenario of one kind.  `Geom(p)` / `Pred(p)` wrap a set's arrays, `check` compares the batch call with the host walk,
// `OtherGeom` is the other kind's geometry over whatever arrays (it must be refused before they are read).
template <class Geom, class Pred, class OtherGeom, class Check>
void scenario(const char *kind, const Prims &p0, const Prims &p1, const std::vector<Ray<float> > &rays, Check check, const std::string &out, size_t *devices) {
  const std::string w = kind;
  BVHAccel<float> a;
  Geom g0(p0.pos.data(), p0.radii.data()), g1(p1.pos.data(), p1.radii.data());
  expect(kind, "Build", a.Build(p0.n, g0, Pred(p0.pos.data())));
  *devices = a.NumHipDevices();
  check((w + ": built").c_str(), a, p0, rays);
  const Nodes nodes0 = a.GetNodes();
  const std::vector<unsigned int> indices0 = a.GetIndices();
  BVHAccel<float> copy = a;
  // refusals first: another kind, another count — each with a reason, the object unchanged
  OtherGeom other(p1.pos.data(), p1.radii.data());
  expect(kind, "another kind refused", !a.RefitGeometry(other) && !a.LastBackendError().empty());
  expect(kind, "another count refused", !a.RefitGeometry(g1, p0.n + 1) && a.LastBackendError().find("number of primitives") != std::string::npos);
  expect(kind, "Refit(geometry) still refuses", !a.Refit(g1) && a.LastBackendError().find("do not refit") != std::string::npos);
  expect(kind, "refusals changed nothing", same_nodes(a.GetNodes(), nodes0));
  check((w + ": after the refusals").c_str(), a, p0, rays);
  // the refit
  expect(kind, "RefitGeometry", a.RefitGeometry(g1));
  expect(kind, "RefitGeometry (again, with the count)", a.RefitGeometry(g1, p0.n));
  check((w + ": refit object").c_str(), a, p1, rays);
  check((w + ": copy made before").c_str(), copy, p0, rays);
  expect(kind, "the copy keeps the old tree", same_nodes(copy.GetNodes(), nodes0));
  expect(kind, "the refit tree differs", !same_nodes(a.GetNodes(), nodes0));
  expect(kind, "the index array is kept", a.GetIndices() == indices0);
  float lo[3], hi[3];
  a.BoundingBox(lo, hi);
  const Nodes nodes1 = a.GetNodes();
  expect(kind, "BoundingBox() is the refit root's", !nodes1.empty() && memcmp(lo, nodes1[0].bmin, 12) == 0 && memcmp(hi, nodes1[0].bmax, 12) == 0);
  expect(kind, "trees written", write_trees(out, nodes0, indices0, nodes1));
  // the copy refits on its own (it moves to contexts of its own); the first object keeps its positions
  expect(kind, "copy RefitGeometry", copy.RefitGeometry(g1));
  check((w + ": copy refit").c_str(), copy, p1, rays);
  expect(kind, "both hold the same refit tree", same_nodes(copy.GetNodes(), nodes1));
  check((w + ": untouched by the copy's refit").c_str(), a, p1, rays);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: refit_prims_check DIR\n");
    return 2;
  }
  const std::string dir = argv[1];
  Prims s0, s1, c0, c1;
  std::vector<Ray<float> > srays, crays;
  if (!read_prims(dir + "/spheres0.bin", 3, 1, &s0) || !read_prims(dir + "/spheres1.bin", 3, 1, &s1) || !read_prims(dir + "/curves0.bin", 12, 4, &c0) ||
      !read_prims(dir + "/curves1.bin", 12, 4, &c1) || !read_rays(dir + "/srays.bin", &srays) || !read_rays(dir + "/crays.bin", &crays) || s0.n != s1.n ||
      c0.n != c1.n)
    return 2;
  size_t devices = 0;
  scenario<nanort::SphereGeometry, nanort::SpherePred, nanort::BezierCurveGeometry>("spheres", s0, s1, srays, check_spheres, dir + "/spheres_out.bin", &devices);
  scenario<nanort::BezierCurveGeometry, nanort::BezierCurvePred, nanort::SphereGeometry>("curves", c0, c1, crays, check_curves, dir + "/curves_out.bin", &devices);
  {  // a triangle accel and an accel without a tree refuse too
    BVHAccel<float> none;
    expect("kinds", "no tree refused", !none.RefitGeometry(nanort::SphereGeometry(s1.pos.data(), s1.radii.data())) && !none.LastBackendError().empty());
  }
  printf("devices %zu checks %llu mismatches %llu\n", devices, g_checks, g_bad);
  return g_bad ? 1 : 0;
}
